"""classify --report-spans on a few dozen reads cut from the committed reference sequence: every line of classified_spans.tsv against
what tests/spans_rules.py and tests/locate_rules.py derive from the oracle, with and without --bin-map, alone and beside the other
reports; a run without the flag writes no such file and its other outputs are the same bytes."""
import hashlib
import os
import subprocess

import numpy as np
import pytest

from oracle import pyoracle as po
from tests import helpers as H
from tests.locate_rules import reduce_locate
from tests.spans_rules import position_hits, record

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "readbouncer_amd", "readbouncer_amd_cli")
CHUNK, MAX_CHUNKS, K = 250, 5, 13


def run(*args):
    p = subprocess.run([CLI] + list(args), capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
    return p.stdout


def config(path, usage, out, **ibf):
    lines = ['usage = "%s"' % usage, "output_directory = '%s'" % out, "log_directory = '%s/logs'" % out, "", "[IBF]"]
    for key, v in ibf.items():
        lines.append("%s = [%s]" % (key, ", ".join("'%s'" % x for x in v)) if isinstance(v, list) else "%s = %s" % (key, v))
    path.write_text("\n".join(lines) + "\n")


def make_reads(ref, rng):
    """36 reads: cut from the reference with errors (classified by the first chunk), chimeric ones whose first chunks are random
    (classified by a later chunk: the chunk start is added to the positions), reverse-complemented ones, random ones, one with Ns"""
    comp = str.maketrans("ACGT", "TGCA")
    reads = []
    for i in range(36):
        L = CHUNK * int(rng.integers(1, 4)) + int(rng.integers(60, 240))
        s = int(rng.integers(0, len(ref) - L))
        r = H.mutate(rng, ref[s:s + L].upper(), float(rng.uniform(0.0, 0.1)))
        if i % 4 == 1:
            r = H.random_dna(rng, CHUNK * int(rng.integers(1, 3))) + r  # host part first, target part after it
        elif i % 4 == 2:
            r = r[::-1].translate(comp)
        elif i % 9 == 3:
            r = H.random_dna(rng, L)
        if i == 8:
            r = r[:100] + "NNNN" + r[104:180] + "N" + r[181:]
        reads.append(("read%02d extra words" % i, r))
    return reads


@pytest.mark.gpu
def test_cli_report_spans(tmp_path, refdata):
    tgt_fa = os.path.join(refdata, "classifyTests_test.fasta")
    out_b = tmp_path / "built"
    config(tmp_path / "b.toml", "build", out_b, kmer_size=K, fragment_size=1000, target_files=[tgt_fa])
    run("--config", str(tmp_path / "b.toml"), "--write-bin-map")
    name = "classifyTests_test"
    rows = [l.split("\t") for l in (out_b / (name + ".bins.tsv")).read_text().splitlines() if not l.startswith("#")][1:]
    record_of = {int(r[0]): r[1] for r in rows}
    oracle = po.OracleIBF.load(str(out_b / (name + ".ibf")))
    assert oracle.n_bins == len(record_of) >= 9
    ref = "".join(s for _, s in H.read_fasta(tgt_fa))
    reads = make_reads(po.cut_out_nnns(ref), np.random.default_rng(21))
    fq = tmp_path / "reads.fastq"
    fq.write_text("".join("@%s\n%s\n+\n%s\n" % (rid, s, "I" * len(s)) for rid, s in reads))

    def expectation(with_map):
        lines = ["read_id\tfilter\tbin" + ("\trecord_id" if with_map else "") + "\tstrand\tn_kmers\tcount\tfirst\tlast\trun_start\trun_len\tcovered"]
        later = 0
        for rid, s in reads:
            rid = rid.split()[0]
            for c in range(MAX_CHUNKS):
                if c * CHUNK > len(s):
                    break  # the reference's undefined infix: the read fails
                chunk = s[c * CHUNK:(c + 1) * CHUNK]
                if len(chunk) < K:
                    break  # a short chunk fails the read
                o = po.encode(chunk)
                t = po.threshold(len(o), K, 0.1, 0.95)
                fwd, rev = oracle.count(o), oracle.count(po.revcomp(o))
                m, b, strand, _ = reduce_locate(fwd, rev, t)
                if m > 0 and m >= t:  # the chunk that classifies the read: where its best bin matched, on its best strand
                    hits = position_hits(oracle, chunk, [b])[strand, 0]
                    cnt, first, last, rs, rl, cov = record(hits, K)
                    assert cnt & 0xFFFF == m
                    at = c * CHUNK
                    lines.append("%s\t%s\t%d%s\t%s\t%d\t%d\t%d\t%d\t%d\t%d\t%d" % (rid, name, b, "\t" + record_of[b] if with_map else "", "-" if strand else "+",
                                                                                 len(hits), cnt, first + at, last + at, rs + at, rl, cov))
                    later += c > 0
                    break
        return lines, later

    outs = {}
    bin_map = str(out_b / (name + ".bins.tsv"))
    for tag, extra in (("plain", []), ("spans", ["--report-spans", "--bin-map", bin_map]), ("nomap", ["--report-spans"]),
                       ("all", ["--report-bins", "--report-spans", "--report-hits"]),
                       ("segments", ["--report-spans", "--segment-bytes", "3000", "--classify-threads", "3"])):  # several segments, in file order
        out = tmp_path / ("out_" + tag)
        config(tmp_path / (tag + ".toml"), "classify", out, kmer_size=K, fragment_size=1000, target_files=[out_b / (name + ".ibf")], read_files=[fq],
               chunk_length=CHUNK, max_chunks=MAX_CHUNKS)
        run("--config", str(tmp_path / (tag + ".toml")), *extra)
        outs[tag] = {p.name: hashlib.sha256(p.read_bytes()).hexdigest() for p in sorted(out.iterdir()) if p.is_file()}
    new = {"classified_spans.tsv"}
    assert not new & set(outs["plain"])
    for tag, more in (("spans", set()), ("nomap", set()), ("segments", set()), ("all", {"classified_bins.tsv", "classified_hits.tsv", "bin_profile.tsv"})):
        assert set(outs[tag]) == set(outs["plain"]) | new | more, tag
        for f in outs["plain"]:
            if f != "configLog.toml":  # (the echo of the configuration names the run's own output directory)
                assert outs["plain"][f] == outs[tag][f], (tag, f)
    for tag, with_map in (("spans", True), ("nomap", False), ("all", False), ("segments", False)):
        lines, later = expectation(with_map)
        assert len(lines) >= 20 and later >= 4  # most reads are classified, several of them by a later chunk
        assert any(l.split("\t")[-8] == "-" for l in lines[1:]) and any(l.split("\t")[-8] == "+" for l in lines[1:])
        assert (tmp_path / ("out_" + tag) / "classified_spans.tsv").read_text().splitlines() == lines, tag

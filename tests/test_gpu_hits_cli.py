"""classify --report-hits on the committed reference reads: classified_hits.tsv and bin_profile.tsv against what tests/hits_rules.py
derives from the oracle, with and without --bin-map and under a small --max-hits; a run without the flag writes neither file and
its other outputs are the same bytes."""
import hashlib
import os
import subprocess

import pytest

from oracle import pyoracle as po
from tests import helpers as H
from tests.hits_rules import reduce_hits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "readbouncer_amd", "readbouncer_amd_cli")


def run(*args):
    p = subprocess.run([CLI] + list(args), capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
    return p.stdout


def config(path, usage, out, **ibf):
    lines = ['usage = "%s"' % usage, "output_directory = '%s'" % out, "log_directory = '%s/logs'" % out, "", "[IBF]"]
    for key, v in ibf.items():
        lines.append("%s = [%s]" % (key, ", ".join("'%s'" % x for x in v)) if isinstance(v, list) else "%s = %s" % (key, v))
    path.write_text("\n".join(lines) + "\n")


@pytest.mark.gpu
def test_cli_report_hits_and_bin_profile(tmp_path, refdata):
    tgt_fa = os.path.join(refdata, "classifyTests_test.fasta")
    fq = os.path.join(refdata, "classifyTests_test.fastq")
    out_b = tmp_path / "built"
    config(tmp_path / "b.toml", "build", out_b, kmer_size=13, fragment_size=1000, target_files=[tgt_fa])
    run("--config", str(tmp_path / "b.toml"), "--write-bin-map")
    name = "classifyTests_test"
    rows = [l.split("\t") for l in (out_b / (name + ".bins.tsv")).read_text().splitlines() if not l.startswith("#")][1:]
    record_of = {int(r[0]): r[1] for r in rows}
    oracle = po.OracleIBF.load(str(out_b / (name + ".ibf")))
    assert oracle.n_bins == len(record_of) >= 9
    reads = H.read_fastq(fq)
    assert len(reads) == 3

    def expectation(cap, with_map):
        lines = ["read_id\tfilter\tbin" + ("\trecord_id" if with_map else "") + "\tstrand\tcount\tthreshold\tn_hits"]
        profile = {}
        for rid, s in reads:
            rid = rid.split()[0]
            for c in range(5):
                chunk = s[c * 250:(c + 1) * 250]
                o = po.encode(chunk)
                t = po.threshold(len(o), 13, 0.1, 0.95)
                fwd, rev = oracle.count(o), oracle.count(po.revcomp(o))
                m = max(int(fwd.max()), int(rev.max()))
                if m > 0 and m >= t:  # the chunk that classifies the read: its hits are reported
                    rec = reduce_hits(fwd, rev, t)
                    for b, strand, cnt in rec[:cap]:
                        lines.append("%s\t%s\t%d%s\t%s\t%d\t%d\t%d" % (rid, name, b, "\t" + record_of[b] if with_map else "", "-" if strand else "+", cnt, t, len(rec)))
                    for b in {b for b, _, _ in rec}:
                        profile[b] = profile.get(b, 0) + 1
                    break
        prof = ["filter\tbin\trecord_id\treads"] + ["%s\t%d\t%s\t%d" % (name, b, record_of[b] if with_map else "-", n) for b, n in sorted(profile.items())]
        return lines, prof

    outs = {}
    for tag, extra in (("plain", []), ("hits", ["--report-hits", "--bin-map", str(out_b / (name + ".bins.tsv"))]), ("nomap", ["--report-hits"]),
                       ("cap1", ["--report-hits", "--max-hits", "1"]),
                       ("segments", ["--report-hits", "--segment-bytes", "2000", "--classify-threads", "3"])):  # a segment per read: the profile is merged
        out = tmp_path / ("out_" + tag)
        config(tmp_path / (tag + ".toml"), "classify", out, kmer_size=13, fragment_size=1000, target_files=[out_b / (name + ".ibf")], read_files=[fq],
               chunk_length=250, max_chunks=5)
        run("--config", str(tmp_path / (tag + ".toml")), *extra)
        outs[tag] = {p.name: hashlib.sha256(p.read_bytes()).hexdigest() for p in sorted(out.iterdir()) if p.is_file()}
    new = {"classified_hits.tsv", "bin_profile.tsv"}
    assert not new & set(outs["plain"])
    for tag in ("hits", "nomap", "cap1", "segments"):
        assert set(outs[tag]) == set(outs["plain"]) | new, tag
        for f in outs["plain"]:
            if f != "configLog.toml":  # (the echo of the configuration names the run's own output directory; logs/ is a directory of time stamps)
                assert outs["plain"][f] == outs[tag][f], (tag, f)
    full, _ = expectation(64, False)
    assert any(int(l.split("\t")[-1]) > 1 for l in full[1:])  # a list that --max-hits 1 really cuts
    for tag, cap, with_map in (("hits", 64, True), ("nomap", 64, False), ("cap1", 1, False), ("segments", 64, False)):
        lines, prof = expectation(cap, with_map)
        assert len(lines) >= 4 and len(prof) >= 2  # the three target reads are classified and hit
        assert (tmp_path / ("out_" + tag) / "classified_hits.tsv").read_text().splitlines() == lines, tag
        assert (tmp_path / ("out_" + tag) / "bin_profile.tsv").read_text().splitlines() == prof, tag

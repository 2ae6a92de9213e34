"""classify --report-prefixes through the command-line tool: filters built by the tool, a FASTQ of about 60 reads, and both reports
compared with tests/prefix_rules.py (the oracle on the ASCII prefixes); the ordinary outputs are the bytes of a run without the flag."""
import hashlib
import os
import subprocess

import numpy as np
import pytest

from oracle import pyoracle as po
from tests import helpers as H
from tests import prefix_rules as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "readbouncer_amd", "readbouncer_amd_cli")
CHECKPOINTS = (140, 204, 360)


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
def test_cli_report_prefixes(tmp_path):
    rng = np.random.default_rng(31)
    g_dep, g_tgt = H.random_dna(rng, 4200), H.random_dna(rng, 3600)
    (tmp_path / "dep.fasta").write_text(">depA\n%s\n" % g_dep)
    (tmp_path / "tgt.fasta").write_text(">tgtA\n%s\n" % g_tgt)
    out_b = tmp_path / "built"
    config(tmp_path / "b.toml", "build", out_b, kmer_size=13, fragment_size=1000, target_files=[tmp_path / "tgt.fasta"],
           deplete_files=[tmp_path / "dep.fasta"])
    run("--config", str(tmp_path / "b.toml"))
    odep, otgt = po.OracleIBF.load(str(out_b / "dep.ibf")), po.OracleIBF.load(str(out_b / "tgt.ibf"))

    reads = []
    for i in range(60):
        L = int(rng.integers(100, 700))  # some end before a checkpoint, some are shorter than the run's chunk_length
        if i % 3 == 0:
            s = H.random_dna(rng, L)
        else:
            g = g_dep if i % 3 == 1 else g_tgt
            p = int(rng.integers(0, len(g) - L))
            s = H.mutate(rng, g[p:p + L], 0.08)
            if i % 4 == 0:
                s = s[::-1].translate(str.maketrans("ACGT", "TGCA"))
            if i % 5 == 0:  # random first 150 bases, reference after them: decided late
                s = H.random_dna(rng, 150) + s[150:]
        reads.append(("r%d" % i, s))
    reads.append(("tiny", "ACGTACGT"))  # shorter than k
    fq = tmp_path / "reads.fastq"
    with open(fq, "w") as fh:
        for n, s in reads:
            fh.write("@%s some comment\n%s\n+\n%s\n" % (n, s, "I" * len(s)))
    outs = {}
    for tag, extra in (("plain", []), ("prefixes", ["--report-prefixes", "--prefix-lens", ",".join(str(c) for c in CHECKPOINTS)])):
        out = tmp_path / ("out_" + tag)
        config(tmp_path / (tag + ".toml"), "classify", out, kmer_size=13, fragment_size=1000, target_files=[out_b / "tgt.ibf"],
               deplete_files=[out_b / "dep.ibf"], read_files=[fq], chunk_length=250, max_chunks=2)
        run("--config", str(tmp_path / (tag + ".toml")), "--segment-bytes", "20000", *extra)
        outs[tag] = {p.name: hashlib.sha256(p.read_bytes()).hexdigest() for p in sorted(out.iterdir()) if p.is_file()}
    assert set(outs["prefixes"]) == set(outs["plain"]) | {"classified_prefixes.tsv", "prefix_summary.tsv"}
    assert not set(outs["plain"]) & {"classified_prefixes.tsv", "prefix_summary.tsv"}
    fastas = [name for name in outs["plain"] if name.endswith(".fasta")]
    assert "unclassified.fasta" in fastas and "tgt.fasta" in fastas
    for name in fastas:
        assert outs["plain"][name] == outs["prefixes"][name], name

    # every read of the run, in file order, in the run's mode (classify: one chunk of the prefix)
    head = "read_id\tlength"
    for c in CHECKPOINTS:
        head += "\tprefix_len@%d\tdecision@%d\tbest_target@%d\tmax_dep@%d\tmax_tgt@%d" % (c, c, c, c, c)
    want = [head]
    tally = np.zeros((len(CHECKPOINTS), 6), dtype=np.int64)
    for n, s in reads:
        rows = PR.expected_rows(s, CHECKPOINTS, [odep], [otgt], PR.MODE_CLASSIFY_CHUNK, r=0.1, conf=0.95)
        line = "%s\t%d" % (n, len(s))
        for p, c in enumerate(CHECKPOINTS):
            d = int(rows["decision"][p])
            line += "\t%d\t%d\t%d\t%d\t%d" % (rows["prefix_len"][p], d, rows["best_target"][p], rows["max_count"][p, 0], rows["max_count"][p, 1])
            tally[p] += [len(s) >= c, d == 0, d == 1, d == 2, rows["first_decided"] == p, p > 0 and d != int(rows["decision"][p - 1])]
        want.append(line)
    got = (tmp_path / "out_prefixes" / "classified_prefixes.tsv").read_text().splitlines()
    assert got == want
    # the cases are there: reads decided at the first checkpoint, later, never; reads that end before a checkpoint; a decision that changes
    assert tally[0, 4] >= 10 and tally[1:, 4].sum() >= 3 and tally[:, 4].sum() <= len(reads) - 10
    assert tally[-1, 0] < len(reads) and tally[:, 5].sum() >= 3
    want_sum = ["prefix_len\treads_reaching\tdecision_0\tdecision_1\tdecision_2\tfirst_decided\tchanged"]
    want_sum += ["%d\t%s" % (c, "\t".join(str(int(v)) for v in tally[p])) for p, c in enumerate(CHECKPOINTS)]
    assert (tmp_path / "out_prefixes" / "prefix_summary.tsv").read_text().splitlines() == want_sum

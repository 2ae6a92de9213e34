"""classify --report-prefixes with --prefix-lists off and with --prefix-lists build on the small filter of tests/test_gpu_pass_lists_cli.py,
which the list form serves (k = 7, 2150 bins of 200 bases: blocks of 34 words, a table of 4^7 slots): classified_prefixes.tsv and
prefix_summary.tsv are the same bytes either way, and so is every other output."""
import hashlib

import numpy as np
import pytest

from tests import helpers as H
from tests.test_gpu_hits_cli import config, run


@pytest.mark.gpu
def test_cli_prefix_lists_files_are_the_same_bytes(tmp_path):
    rng = np.random.default_rng(31)
    ref = H.random_dna(rng, 430_000)
    (tmp_path / "tgt.fasta").write_text(">chr\n%s\n" % ref)
    out_b = tmp_path / "built"
    config(tmp_path / "b.toml", "build", out_b, kmer_size=7, fragment_size=200, target_files=[tmp_path / "tgt.fasta"])
    run("--config", str(tmp_path / "b.toml"))
    reads = []
    for i in range(60):
        L = int(rng.integers(120, 260))
        p = int(rng.integers(0, len(ref) - L))
        s = H.mutate(rng, ref[p:p + L], 0.03) if i % 3 else H.random_dna(rng, L)
        if i % 7 == 0:
            s = s[:50] + "N" + s[51:]  # inside the last checkpoint: the plain form's item
        if i % 7 == 1:
            s = s[:-1] + "N"           # some of these lie behind it
        reads.append(("r%d" % i, s))
    fq = tmp_path / "reads.fastq"
    with open(fq, "w") as fh:
        for n, s in reads:
            fh.write("@%s\n%s\n+\n%s\n" % (n, s, "I" * len(s)))
    outs = {}
    for tag in ("off", "build"):
        out = tmp_path / ("out_" + tag)
        config(tmp_path / (tag + ".toml"), "classify", out, kmer_size=7, fragment_size=200, target_files=[out_b / "tgt.ibf"], read_files=[fq],
               chunk_length=250, max_chunks=1)
        run("--config", str(tmp_path / (tag + ".toml")), "--report-prefixes", "--prefix-lens", "6,7,70,71,134,200", "--prefix-lists", tag)
        outs[tag] = {p.name: hashlib.sha256(p.read_bytes()).hexdigest() for p in sorted(out.iterdir()) if p.is_file()}
        assert len((out / "classified_prefixes.tsv").read_text().splitlines()) >= len(reads)  # a line per read of the run
    assert {"classified_prefixes.tsv", "prefix_summary.tsv"} <= set(outs["off"]) and set(outs["off"]) == set(outs["build"])
    for name in outs["off"]:
        if name != "configLog.toml":  # (the echo of the configuration names the run's own output directory)
            assert outs["off"][name] == outs["build"][name], name

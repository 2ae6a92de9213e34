"""classify --report-prefixes --wide-lists build with --wide-prefix-lists current and off, on a filter the wide list form serves
(k = 9, 10 000 bins of 200 bases: a table of 4^9 slots, and a batch that repays it; at k = 7 the rows of such a filter are too dense
for every slot size and the table is refused): classified_prefixes.tsv and prefix_summary.tsv -- every output file -- are the same
bytes either way.  That a prefix call of this shape on this filter does take the wide form once the table stands is read from
rb_engine_wide_prefix_lines, on the very file the CLI built."""
import hashlib

import numpy as np
import pytest

from oracle import pyoracle as po
from readbouncer_amd import capi
from tests import helpers as H
from tests.test_gpu_hits_cli import config, run
from tests.test_gpu_wide_lists import BUILD, WIDE_KERNEL, upload


@pytest.mark.gpu
def test_cli_wide_prefix_lists_files_are_the_same_bytes(tmp_path):
    rng = np.random.default_rng(39)
    ref = H.random_dna(rng, 2_000_000)
    (tmp_path / "tgt.fasta").write_text(">chr\n%s\n" % ref)
    out_b = tmp_path / "built"
    config(tmp_path / "b.toml", "build", out_b, kmer_size=9, fragment_size=200, target_files=[tmp_path / "tgt.fasta"])
    run("--config", str(tmp_path / "b.toml"))
    o = po.OracleIBF.load(str(out_b / "tgt.ibf"))
    assert 8193 <= o.n_bins <= 32256 and o.n_hash == 3 and o.kmer_size == 9
    reads = []
    for i in range(2400):  # (up to 2048 items the engine takes the latency form, which the wide table does not serve)
        L = int(rng.integers(150, 250))
        p = int(rng.integers(0, len(ref) - L))
        s = H.mutate(rng, ref[p:p + L], 0.03) if i % 3 else H.random_dna(rng, L)
        if i % 7 == 0:
            s = s[:50] + "N" + s[51:]
        if i % 7 == 1:
            s = "N" + s[1:-1] + "N"
        reads.append(("r%d" % i, s))
    d = upload(o)
    eng = capi.Engine(0, [d], [])
    eng.set_wide_lists(BUILD)
    eng.set_wide_prefix_lists(capi.RB_PASS_LISTS_CURRENT)
    assert eng.plan(0, len(reads), 250)["kernel"] == WIDE_KERNEL and eng.wide_prefix_lines(0, 250, 1500) == 0
    info = d.wide_list_table_build()
    assert info["refused"] == 0 and info["builds"] == 1 and eng.wide_prefix_lines(0, 250, 1500) == info["lines"] > 0, info
    eng.destroy(), d.free()
    fq = tmp_path / "reads.fastq"
    with open(fq, "w") as fh:
        for n, s in reads:
            fh.write("@%s\n%s\n+\n%s\n" % (n, s, "I" * len(s)))
    outs = {}
    for tag in ("off", "current"):
        out = tmp_path / ("out_" + tag)
        config(tmp_path / (tag + ".toml"), "classify", out, kmer_size=9, fragment_size=200, target_files=[out_b / "tgt.ibf"], read_files=[fq],
               chunk_length=250, max_chunks=1)
        run("--config", str(tmp_path / (tag + ".toml")), "--report-prefixes", "--prefix-lens", "50,100,150,200,250", "--wide-lists", "build", "--wide-prefix-lists", tag)
        outs[tag] = {p.name: hashlib.sha256(p.read_bytes()).hexdigest() for p in sorted(out.iterdir()) if p.is_file()}
    assert {"classified_prefixes.tsv", "prefix_summary.tsv"} <= set(outs["off"]) and set(outs["off"]) == set(outs["current"])
    for name in outs["off"]:
        if name != "configLog.toml":  # (the echo of the configuration names the run's own output directory)
            assert outs["off"][name] == outs["current"][name], name

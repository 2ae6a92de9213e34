"""classify with --wide-lists off and with --wide-lists build on a filter the wide list form serves (k = 7, 10 000 bins of 200 bases:
blocks of 157 words, a table of 4^7 slots, a batch that repays it): every output file is the same bytes either way.  That a classify
call of this shape on this filter does take ibf_count_wide_lists_kernel is read from rb_engine_plan on the very file the CLI built."""
import hashlib

import numpy as np
import pytest

from oracle import pyoracle as po
from readbouncer_amd import capi
from tests import helpers as H
from tests.test_gpu_hits_cli import config, run
from tests.test_gpu_wide_lists import BUILD, WIDE_KERNEL, upload


@pytest.mark.gpu
def test_cli_wide_lists_files_are_the_same_bytes(tmp_path):
    rng = np.random.default_rng(37)
    ref = H.random_dna(rng, 2_000_000)
    (tmp_path / "tgt.fasta").write_text(">chr\n%s\n" % ref)
    out_b = tmp_path / "built"
    config(tmp_path / "b.toml", "build", out_b, kmer_size=7, fragment_size=200, target_files=[tmp_path / "tgt.fasta"])
    run("--config", str(tmp_path / "b.toml"))
    o = po.OracleIBF.load(str(out_b / "tgt.ibf"))
    assert 8193 <= o.n_bins <= 32256 and o.n_hash == 3 and o.kmer_size == 7
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
    eng = capi.Engine(0, [d], [])  # the engine as the CLI has it, but for the one setting
    eng.set_wide_lists(BUILD)
    assert eng.plan(0, len(reads), 250)["kernel"] == WIDE_KERNEL
    eng.destroy(), d.free()
    fq = tmp_path / "reads.fastq"
    with open(fq, "w") as fh:
        for n, s in reads:
            fh.write("@%s\n%s\n+\n%s\n" % (n, s, "I" * len(s)))
    outs = {}
    for tag in ("off", "build"):
        out = tmp_path / ("out_" + tag)
        config(tmp_path / (tag + ".toml"), "classify", out, kmer_size=7, fragment_size=200, target_files=[out_b / "tgt.ibf"], read_files=[fq],
               chunk_length=250, max_chunks=1)
        run("--config", str(tmp_path / (tag + ".toml")), "--wide-lists", tag)
        outs[tag] = {p.name: hashlib.sha256(p.read_bytes()).hexdigest() for p in sorted(out.iterdir()) if p.is_file()}
    assert outs["off"] and set(outs["off"]) == set(outs["build"])
    for name in outs["off"]:
        if name != "configLog.toml":  # (the echo of the configuration names the run's own output directory)
            assert outs["off"][name] == outs["build"][name], name

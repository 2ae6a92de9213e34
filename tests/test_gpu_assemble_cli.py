"""`readbouncer_amd_cli --edit-ibf`: two small filters and their bin maps built by the CLI's own `build --write-bin-map`, then a plan
file, --merge-every and --drop-records, each against the numpy model of tests/assemble_rules.py over the stored source files and
against the <out>.bins.tsv the bin maps imply; the EDIT_IBF line; --filter-stats on the assembled table; and the refusals."""
import os
import re
import subprocess

import numpy as np
import pytest

from oracle import pyoracle as po
from readbouncer_amd import capi
from tests import assemble_rules as R
from tests import helpers as H
from tests.occupancy_rules import bin_occupancy

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "readbouncer_amd", "readbouncer_amd_cli")
K = 13


def run(*args, expect=0):
    p = subprocess.run([CLI] + [str(a) for a in args], capture_output=True, text=True, timeout=600)
    assert p.returncode == expect, (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
    return p.stdout, p.stderr


def build(tmp_path, name, records, fragment_size):
    fa = tmp_path / (name + ".fasta")
    fa.write_text("".join(">%s some text\n%s\n" % r for r in records))
    out = tmp_path / ("built_" + name)
    (tmp_path / (name + ".toml")).write_text(
        "usage = \"build\"\noutput_directory = '%s'\nlog_directory = '%s/logs'\n\n[IBF]\nkmer_size = %d\nfragment_size = %d\ntarget_files = ['%s']\n"
        % (out, out, K, fragment_size, fa))
    run("--config", tmp_path / (name + ".toml"), "--write-bin-map")
    return out / (name + ".ibf"), out / (name + ".bins.tsv")


def load(path):
    f = po.OracleIBF.load(str(path))
    return f, (f.words().copy(), f.n_bins, f.n_blocks)


def map_rows(path):
    rows = [l.split("\t") for l in path.read_text().splitlines() if l and not l.startswith("#") and not l.startswith("bin\t")]
    return {int(r[0]): (r[1], int(r[2]), int(r[3])) for r in rows}


def expected_map(plan, maps, head):
    """head: the two head lines of a bin map, as `build --write-bin-map` wrote them"""
    lines = list(head)
    for j, refs in enumerate(plan):
        if not refs:
            continue
        rows = [maps[f][b] for f, b in refs]
        ids = list(dict.fromkeys(r[0] for r in rows))
        if len(ids) == 1:
            lines.append("%d\t%s\t%d\t%d" % (j, ids[0], min(r[1] for r in rows), max(r[2] for r in rows)))
        else:
            lines.append("%d\t%s\t\t" % (j, ",".join(ids)))
    return "\n".join(lines) + "\n"


def check_output(out_ibf, sources, plan):
    got = po.OracleIBF.load(str(out_ibf))
    n_blocks = sources[0][2]
    want = R.assemble_words(sources, plan)
    payload = n_blocks * ((len(plan) + 63) // 64)
    assert got.n_bins == len(plan) and got.n_blocks == n_blocks and got.kmer_size == K and got.n_hash == 3
    assert np.array_equal(got.words()[:payload], want[:payload])
    return want


def edit_line(text):
    m = re.search(r"^EDIT_IBF sources=(\d+) bins_in=(\d+) bins_out=(\d+) refs=(\d+) kernel_seconds=(\S+) output=(\S+)$", text, re.M)
    assert m, text
    return [int(x) for x in m.groups()[:4]], float(m.group(5)), m.group(6)


def test_edit_ibf(tmp_path):
    rng = np.random.default_rng(41)
    recs_a = [("chrA", H.random_dna(rng, 5300)), ("chrB", H.random_dna(rng, 1500) + "N" * 40 + H.random_dna(rng, 2200)), ("chrC", H.random_dna(rng, 700))]
    recs_b = [("plasmid1", H.random_dna(rng, 2600)), ("chrB", H.random_dna(rng, 900))]
    a_ibf, a_map = build(tmp_path, "a", recs_a, 1000)
    b_ibf, b_map = build(tmp_path, "b", recs_b, 1000)
    c_ibf, _ = build(tmp_path, "c", recs_b, 500)  # another fragment size: another n_blocks
    (fa, sa), (fb, sb), (fc, _) = load(a_ibf), load(b_ibf), load(c_ibf)
    ma, mb = map_rows(a_map), map_rows(b_map)
    head = a_map.read_text().splitlines()[:2]
    assert head[0].startswith("#") and head[1] == "bin\trecord_id\tstart\tend" and b_map.read_text().splitlines()[:2] == head
    assert fa.n_blocks == fb.n_blocks != fc.n_blocks and len(ma) == fa.n_bins >= 9 and len(mb) == fb.n_bins >= 4
    na, nb = fa.n_bins, fb.n_bins

    # --plan: a join with a reordering, a merge inside one record, a merge across records and filters, empty bins and a fixed bin count
    plan = [[(0, na - 1)], [(1, 0), (1, 1)], [], [(0, 0), (1, nb - 1), (0, 0)], [(0, 1), (0, 3), (0, 2)], [], []]
    text = "# a comment\n# bins=7\n"
    for j, refs in enumerate(plan):
        for f, b in refs:
            text += "%d\t%d\t%d%s\n" % (j, f, b, "   # the trailing kind" if j == 1 else "")
    (tmp_path / "plan.tsv").write_text(text + "\n")
    out1 = tmp_path / "joined.ibf"
    stdout, _ = run("--edit-ibf", a_ibf, "--with", b_ibf, "--output", out1, "--plan", tmp_path / "plan.tsv", "--bin-map", "%s,%s" % (a_map, b_map))
    counts, secs, path = edit_line(stdout)
    assert counts == [2, na + nb, 7, sum(len(l) for l in plan)] and secs > 0.0 and path == str(out1)
    check_output(out1, [sa, sb], plan)
    assert (tmp_path / "joined.bins.tsv").read_text() == expected_map(plan, [ma, mb], head)
    # without `# bins=`: highest out bin + 1; without --bin-map: no bin map is written
    (tmp_path / "plan2.tsv").write_text("3\t0\t2\n0\t0\t1\n")
    stdout, _ = run("--edit-ibf", a_ibf, "--output", tmp_path / "short.ibf", "--plan", tmp_path / "plan2.tsv")
    assert edit_line(stdout)[0] == [1, na, 4, 2]
    check_output(tmp_path / "short.ibf", [sa], [[(0, 1)], [], [], [(0, 2)]])
    assert not (tmp_path / "short.bins.tsv").exists()

    # --merge-every 4, with --filter-stats on the assembled table while it is in HBM
    out2 = tmp_path / "merged.ibf"
    stdout, _ = run("--edit-ibf", a_ibf, "--output", out2, "--merge-every", "4", "--bin-map", a_map, "--max-fp", "0.9", "--filter-stats")
    plan = R.groups_of(na, 4)
    assert edit_line(stdout)[0] == [1, na, len(plan), na]
    want = check_output(out2, [sa], plan)
    assert (tmp_path / "merged.bins.tsv").read_text() == expected_map(plan, [ma], head)
    assert "FILTER_STATS file=%s bins=%d " % (out2, len(plan)) in stdout and "bins_over_max_fp=0\n" in stdout
    rows = [l.split("\t") for l in (tmp_path / "merged.binstats.tsv").read_text().splitlines()]
    assert rows[0] == ["bin", "bits", "load", "fpr", "est_kmers", "record_id", "start", "end"]
    assert np.array_equal(np.array([int(r[1]) for r in rows[1:]], dtype=np.uint64), bin_occupancy(want, len(plan), fa.n_blocks))
    assert [r[5] for r in rows[1:]] == [l.split("\t")[1] for l in expected_map(plan, [ma], head).splitlines()[2:]]
    # ... four fragments in a bin sized for one are over the default max_fp: exit code 3, the file is written all the same
    stdout, _ = run("--edit-ibf", a_ibf, "--output", tmp_path / "merged3.ibf", "--merge-every", "4", "--filter-stats", expect=3)
    assert "EDIT_IBF" in stdout and "FILTER_STATS" in stdout and not re.search(r"bins_over_max_fp=0\n", stdout)
    check_output(tmp_path / "merged3.ibf", [sa], plan)

    # --drop-records: every bin of the other records, in order, over both filters
    out3 = tmp_path / "dropped.ibf"
    stdout, _ = run("--edit-ibf", a_ibf, "--with", b_ibf, "--output", out3, "--drop-records", "chrB,chrC", "--bin-map", a_map, "--bin-map", b_map)
    plan = [[(f, b)] for f, m in enumerate((ma, mb)) for b in sorted(m) if m[b][0] not in ("chrB", "chrC")]
    assert 0 < len(plan) < na + nb and edit_line(stdout)[0] == [2, na + nb, len(plan), len(plan)]
    check_output(out3, [sa, sb], plan)
    assert (tmp_path / "dropped.bins.tsv").read_text() == expected_map(plan, [ma, mb], head)
    assert {l.split("\t")[1] for l in (tmp_path / "dropped.bins.tsv").read_text().splitlines()[2:]} == {"chrA", "plasmid1"}

    # refusals: a message and exit code 1, nothing written
    bad = tmp_path / "bad.ibf"
    (tmp_path / "oob.tsv").write_text("0\t0\t%d\n" % na)
    _, err = run("--edit-ibf", a_ibf, "--output", bad, "--plan", tmp_path / "oob.tsv", expect=1)
    assert "out bin 0 names bin %d of source 0" % na in err
    (tmp_path / "oob2.tsv").write_text("# bins=2\n2\t0\t0\n")
    _, err = run("--edit-ibf", a_ibf, "--output", bad, "--plan", tmp_path / "oob2.tsv", expect=1)
    assert "out of range" in err
    (tmp_path / "oob3.tsv").write_text("0\t1\t0\n")
    _, err = run("--edit-ibf", a_ibf, "--output", bad, "--plan", tmp_path / "oob3.tsv", expect=1)
    assert "names filter 1 of 1" in err
    (tmp_path / "mal.tsv").write_text("0\t0\n")
    _, err = run("--edit-ibf", a_ibf, "--output", bad, "--plan", tmp_path / "mal.tsv", expect=1)
    assert "malformed" in err and "mal.tsv:1" in err
    _, err = run("--edit-ibf", a_ibf, "--output", bad, "--drop-records", "chrA,chrZ", "--bin-map", a_map, expect=1)
    assert "chrZ" in err
    _, err = run("--edit-ibf", a_ibf, "--output", bad, "--drop-records", "chrA", expect=1)
    assert "--bin-map" in err
    _, err = run("--edit-ibf", a_ibf, "--with", c_ibf, "--output", bad, "--plan", tmp_path / "plan2.tsv", expect=1)
    assert "source 1 differs from source 0" in err
    _, err = run("--edit-ibf", a_ibf, "--with", b_ibf, "--output", bad, "--merge-every", "2", expect=1)
    assert "one filter" in err
    # a typo in the out-bin column is a message, not an allocation of two thousand million empty bins
    (tmp_path / "typo.tsv").write_text("0\t0\t0\n2000000000\t0\t1\n")
    _, err = run("--edit-ibf", a_ibf, "--output", bad, "--plan", tmp_path / "typo.tsv", expect=1)
    assert "out of range" in err and "2000000000" in err
    (tmp_path / "typo2.tsv").write_text("# bins=4\n0\t0\t0\n2000000000\t0\t1\n")
    _, err = run("--edit-ibf", a_ibf, "--output", bad, "--plan", tmp_path / "typo2.tsv", expect=1)
    assert "typo2.tsv:3" in err and "out of range" in err
    # the flags of --edit-ibf without it are refused, not ignored
    for flags in (["--output", bad], ["--plan", tmp_path / "plan.tsv"], ["--merge-every", "2"], ["--with", b_ibf], ["--drop-records", "chrA"]):
        _, err = run(*flags, expect=1)
        assert "--edit-ibf" in err, flags
    assert not bad.exists()
    # the library the CLI runs is the one under test
    assert capi.device_count() > 0

"""What the tests of the wide forms of locate and hits rest on, checked without a GPU: on the oracle alone, that the fixtures of
tests/wide_pass_lists_rig.py hold what tests/test_gpu_wide_pass_lists.py claims of them -- which bins tie and where they lie in the four
waves' shares of the scan, that the min_count = 1 reads exceed every cap used -- that the new calls are declared and bound, and the
resources of the kernels of rb_wide_pass_lists.hip at build time (hipcc -Rpass-analysis=kernel-resource-usage); and the host arithmetic
of the scan's shares as a stand-alone C++ program, plain and under sanitizers."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from oracle import pyoracle as po
from readbouncer_amd import capi
from tests import wide_lists_rig as WR
from tests import wide_pass_lists_rig as WP
from tests.hits_rules import reduce_hits
from tests.locate_rules import reduce_locate
from tests.test_row_lists_cpu import FLAGS, LDS_PER_CU, parse
from tests.test_wide_lists_cpu import build_layout_program

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "readbouncer_amd", "csrc")
K = WP.K


@pytest.mark.parametrize("sanitize", (False, True))
def test_host_arithmetic_of_the_shares(tmp_path, sanitize):
    """tests/cpp/test_wide_pass_lists.cpp: the LDS the pass kernels declare and the waves' shares of the scan, for every bin count served,
    plain and under the address and undefined-behaviour sanitizers -- and the rig's share_of_bin agrees with the header's"""
    exe = str(tmp_path / ("test_wide_pass_lists" + ("_san" if sanitize else "")))
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall"] + flags + [os.path.join(ROOT, "tests", "cpp", "test_wide_pass_lists.cpp"), "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and "failures: 0" in run.stdout, run.stdout + run.stderr
    assert [WP.share_of_bin(32256, b) for b in (0, 8191, 8192, 32255)] == [0, 0, 1, 3] and WP.share_of_bin(8193, 8192) == 3  # (the program's own cases)


def counts(o, read):
    return o.count(po.encode(read)), o.count(po.encode(WR.revcomp(read)))


@pytest.mark.parametrize("name", list(WR.COUNT_FIXTURES))
def test_the_tie_rows_tie_where_the_rig_says(name):
    c = WP.pass_fixture(name)
    n_bins = c.n_bins
    rows = WR.expected_rows(c.o)
    assert WR.census(WR.populations(rows))[0] == c.lines  # the rewritten blocks leave the census verdict alone
    for tie, read in zip(("two_waves", "one_piece", "same_bin", "rev_lower"), c.tie_reads()):
        fwd, rev = counts(c.o, read)
        want_fwd, want_rev = c.tie_rows[tie]
        assert np.nonzero(fwd)[0].tolist() == sorted(want_fwd) and np.nonzero(rev)[0].tolist() == sorted(want_rev), tie
        assert int(fwd.max()) == 1 and int(max(fwd.max(), rev.max())) == 1
        m, b, s, _ = reduce_locate(fwd, rev, 1)
        assert (m, b, s) == (1,) + c.tie_want[tie], tie
    a, b = c.tie_rows["two_waves"][0]
    assert WP.share_of_bin(n_bins, a) == 0 and WP.share_of_bin(n_bins, b) == max(WP.share_of_bin(n_bins, x) for x in range(n_bins)) > 0
    a, b = c.tie_rows["one_piece"][0]
    assert a // WP.PIECE_BINS == b // WP.PIECE_BINS and a < b
    assert c.tie_rows["same_bin"][0] == c.tie_rows["same_bin"][1]
    assert c.tie_rows["rev_lower"][1][0] < c.tie_rows["rev_lower"][0][0]
    assert WP.share_of_bin(n_bins, c.tie_rows["rev_lower"][1][0]) != WP.share_of_bin(n_bins, c.tie_rows["rev_lower"][0][0])


@pytest.mark.parametrize("name", list(WR.COUNT_FIXTURES))
def test_the_planted_bins_cover_every_waves_share_and_min_count_1_exceeds_the_caps(name):
    c = WP.pass_fixture(name)
    n_bins = c.n_bins
    shares = [WP.share_of_bin(n_bins, b) for b in range(0, n_bins, WP.ROUND_BINS)]
    assert sorted(set(shares)) == list(range(WR.WAVES)) and shares == sorted(shares)  # four stretches of rising bins
    per = max(shares.count(w) for w in range(WR.WAVES))
    assert per <= 16  # a thread's pieces fit its 16 mask bytes
    planted = {WP.share_of_bin(n_bins, b) for _, b in c.plants}
    assert {0, WR.WAVES - 1} <= planted and (n_bins < 16384 or len(planted) >= 3)
    for read, b in c.planted_reads():  # the plants still peak where the rig says, behind the tie rows' rewritten blocks
        fwd, rev = counts(c.o, read)
        both = np.maximum(fwd, rev)
        assert int(both.argmax()) == b and int(np.sort(both)[-2]) < int(both.max())
    # min_count 1 on a planted read: hits in every wave's share, far beyond every cap used
    fwd, rev = counts(c.o, c.plants[0][0])
    recs = reduce_hits(fwd, rev, 1)
    assert len(recs) > 20 * max(WP.CAPS)
    assert {WP.share_of_bin(n_bins, b) for b, _, _ in recs} == set(range(WR.WAVES))
    # the order read: the crafted row's cap + 1 bins twenty times on the forward strand (and the few its junction k-mers add), across
    # every wave boundary
    fwd, rev = counts(c.o, c.order_read())
    bins = np.nonzero(fwd >= 20)[0]
    assert len(bins) >= c.cap + 1 and {WP.share_of_bin(n_bins, int(b)) for b in bins} == set(range(WR.WAVES))
    # items the form leaves stand between items it takes
    left = c.left_reads()
    assert [len(r) >= K for r in left] == [True, False, True, False, True, False, True] and "N" in left[-1]


def test_the_new_calls_are_declared_and_bound():
    tuning = open(os.path.join(ROOT, "include", "readbouncer_amd_tuning.h")).read()
    assert "RB_API int rb_engine_set_wide_pass_lists(rb_engine *e, int mode);" in tuning
    assert "RB_API int rb_engine_wide_pass_lines(rb_engine *e, size_t filter_index, uint32_t max_len, uint32_t *lines_out);" in tuning
    assert "locate, hits, spans, prefix and resume do not read the wide table" not in tuning
    assert {"rb_engine_set_wide_pass_lists", "rb_engine_wide_pass_lines"} <= set(capi.SIGNATURES)
    assert callable(capi.Engine.set_wide_pass_lists) and callable(capi.Engine.wide_pass_lines)
    main = open(os.path.join(ROOT, "readbouncer_amd", "host", "rb_main.cpp")).read()
    assert '"--wide-pass-lists"' in main and "int wide_pass_lists = RB_PASS_LISTS_CURRENT;" in main
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert mk.count("rb_wide_pass_lists.o:") == 1 and "rb_wide_pass_lists.o" in mk.split("OBJS")[1].split("\n")[0]


def compile_unit(tmp_path, unit):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        pytest.skip("no hipcc on this box: the resources are pinned where the library is built")
    p = subprocess.run([hipcc] + FLAGS + ["-c", os.path.join(CSRC, unit + ".hip"), "-o", str(tmp_path / (unit + ".o"))],
                       capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    return parse(p.stderr)


def test_wide_pass_kernels_resources(tmp_path):
    found = compile_unit(tmp_path, "rb_wide_pass_lists")
    want = {"%s<%d,%d,4>" % (kern, lines, nt) for kern in ("ibf_locate_wide_lists_kernel", "ibf_hits_wide_lists_kernel")
            for lines in WR.WIDE_LINES for nt in (0, 1)} | {"wide_pass_lists_prep_kernel"}
    assert set(found) == want, sorted(set(found) ^ want)
    assert not {k: v for k, v in found.items() if v["scratch"]}, found
    assert all(v["lds"] == 0 for v in found.values()), found  # static LDS 0: what the pass kernels use is dynamic
    # the declared dynamic LDS is the count kernel's, to the byte: rbwide::pass_lds_bytes returns count_lds_bytes
    hdr = open(os.path.join(CSRC, "rb_wide_lists.h")).read()
    assert "constexpr uint32_t pass_lds_bytes(uint32_t n_bins, uint32_t waves = kWideWaves) { return count_lds_bytes(n_bins, waves); }" in hdr
    src = open(os.path.join(CSRC, "rb_wide_pass_lists.hip")).read()
    assert src.count("lds = rbwide::pass_lds_bytes(a.f.n_bins, NW)") == 2 and "hipFuncAttributeMaxDynamicSharedMemorySize" not in src
    out = subprocess.run([build_layout_program(tmp_path, False)], capture_output=True, text=True, check=True).stdout
    lds = {int(a): (int(b), int(c)) for a, b, c in re.findall(r"wide_count_lds n_bins (\d+) bytes (\d+) resident (\d+)", out)}
    assert lds[32256] == (65344, 2) and lds[32256][0] <= 64 * 1024 and lds[31000][1] == 2
    for name, r in found.items():
        if name.startswith("wide_pass_lists_prep_kernel"):
            continue
        for n_bins in (31000, 32256):  # a workgroup is one wave per SIMD: the registers allow what the LDS allows
            assert lds[n_bins][0] * lds[n_bins][1] <= LDS_PER_CU and r["occ"] >= lds[n_bins][1], (name, r, n_bins)


def test_the_wide_unit_still_holds_its_seven_kernels(tmp_path):
    found = compile_unit(tmp_path, "rb_wide_lists")
    want = {"ibf_count_wide_lists_kernel<%d,%d,4>" % (lines, nt) for lines in WR.WIDE_LINES for nt in (0, 1)} | {"ibf_wide_list_table_kernel"}
    assert set(found) == want and len(found) == 7, sorted(set(found) ^ want)
    src = open(os.path.join(CSRC, "rb_wide_lists.hip")).read()
    assert '#include "rb_wide_lists_device.h"' in src and "lds = rbwide::count_lds_bytes(a.f.n_bins, NW)" in src
    dev = open(os.path.join(CSRC, "rb_wide_lists_device.h")).read()
    assert all(s in dev for s in ("struct WideVec", "void wide_count_word(", "void wide_batch(", "void wide_count_strand("))

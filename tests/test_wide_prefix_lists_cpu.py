"""What the tests of the wide list form of the prefix pass rest on, checked without a GPU: on the oracle alone, that the fixtures of
tests/wide_prefix_lists_rig.py hold what tests/test_gpu_wide_prefix_lists.py claims of them -- the long read's maxima rise one by one,
which share of the scan each planted bin falls into, where the maxima move, what the take model counts --; that the three new calls
are declared and bound; and the resources of the kernels of rb_wide_prefix_lists.hip at build time (hipcc
-Rpass-analysis=kernel-resource-usage).  The form adds no host arithmetic to rb_wide_lists.h, so there is no stand-alone C++ program."""
import os
import re
import subprocess

import numpy as np
import pytest

from oracle import pyoracle as po
from readbouncer_amd import capi
from tests import prefix_lists_rig as XL
from tests import prefix_rules as PR
from tests import wide_lists_rig as WR
from tests import wide_prefix_lists_rig as WX
from tests.test_row_lists_cpu import LDS_PER_CU
from tests.test_wide_lists_cpu import build_layout_program
from tests.test_wide_pass_lists_cpu import compile_unit

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "readbouncer_amd", "csrc")
K = WX.K


@pytest.mark.parametrize("name", list(WR.COUNT_FIXTURES))
def test_the_planted_reads_are_what_the_rig_says(name):
    c = WX.prefix_fixture(name)
    n_bins = c.n_bins
    rows = WR.expected_rows(c.o)
    pc = WR.populations(rows)
    assert WR.census(pc)[0] == c.lines  # the reads planted on top leave the census verdict alone
    assert [int(pc[r]) for r in c.ranks] == list(c.want)  # ... and the crafted rows: an overflow slot, swapped halves, exactly cap bins
    for tie, read in zip(("two_waves", "one_piece", "same_bin", "rev_lower"), c.tie_reads()):
        want_fwd, want_rev = c.tie_rows[tie]
        assert np.nonzero(c.o.count(po.encode(read)))[0].tolist() == sorted(want_fwd), tie
        assert np.nonzero(c.o.count(po.encode(WR.revcomp(read))))[0].tolist() == sorted(want_rev), tie
    # the long read: a prefix of n k-mers has the maximum n, at every seam checkpoint
    got = [max(f, r) for f, _, r, _ in WX.strand_maxima(c.o, c.long, WX.SEAM_CHECKPOINTS)]
    assert got == [min(n, WX.LONG_KMERS) for n in WX.SEAM_KMERS] + [WX.LONG_KMERS] * 2
    # (from a tile on no other bin ties with it)
    assert all(f == n and b == c.long_bin == 5 for (f, b, _, _), n in zip(WX.strand_maxima(c.o, c.long, WX.SEAM_CHECKPOINTS), WX.SEAM_KMERS) if n >= 63)
    assert len(c.random_long) == len(c.long) and c.random_long in c.seam_reads()
    # the seams the checkpoints straddle, and the ranges between them
    steps = list(zip(WX.SEAM_KMERS, WX.SEAM_KMERS[1:]))
    for seam in (16, 64, 256):
        assert (seam - 1, seam) in steps and (seam, seam + 1) in steps
    assert (65, 100) in steps and 65 % 64 and 100 - 65 < 64            # off a multiple of 64, shorter than a tile: wave 0 alone
    assert (100, 228) in steps and 100 % 64 and (228 - 100) == 2 * 64  # two tiles, off a multiple of 64
    assert [(b - a) / 64 for a, b in steps[-3:]] == [4, 5, 9]
    assert WX.SEAM_CHECKPOINTS[0] == K - 1 and WX.SEAM_CHECKPOINTS[1] == K and WX.SEAM_CHECKPOINTS[-2] > len(c.long)
    assert len(WX.SIXTY_FOUR) == 64 and {b - a for a, b in zip(WX.SIXTY_FOUR, WX.SIXTY_FOUR[1:])} == {3} and len(WX.ONE_CHECKPOINT) == 1
    reads = c.seam_reads()
    assert "" in reads and any(0 < len(r) < K for r in reads) and max(len(r) for r in reads) == len(c.long)


@pytest.mark.parametrize("name", list(WR.COUNT_FIXTURES))
def test_the_maxima_move_where_the_rig_says(name):
    c = WX.prefix_fixture(name)
    n_bins = c.n_bins
    shares = [(WX.share_of_bin(n_bins, a), WX.share_of_bin(n_bins, b)) for a, b in c.pairs]
    assert shares[0] == (0, WR.WAVES - 1)  # from wave 0's share of the scan to wave 3's, and back
    bins = {x for p in c.pairs for x in p}
    last_dword = ((n_bins - 1) // 2) * 2
    assert {0, 8191, 8192, last_dword, n_bins - 1} <= bins
    assert (last_dword + 1 in bins) == (n_bins % 2 == 0)  # the odd bin count: the pad half is nobody's bin
    kmers = [c - K + 1 for c in WX.BACK_CHECKPOINTS]
    for (a, b), z, x, y in zip(c.pairs, c.back, c.whole, c.tail):
        # there and back, on strand 0
        at = WX.strand_maxima(c.o, z, WX.BACK_CHECKPOINTS)
        # (the planted bins hold several reads and count some k-mers they were not given: where the maximum stands is what is claimed)
        where = [fbin for _, fbin, _, _ in at]
        if (a, b) == c.pairs[0]:  # wave 0's share, wave 3's, and wave 0's again (the later pairs share bins with it, and theirs fill up)
            assert where[1] == a and where[5] == b and (where[8] == a or n_bins == 8193) and all(fwd > rev for fwd, _, rev, _ in at)  # (c8193: three pairs share its last bin, which fills up)
        assert at[1][0] >= 30 and at[5][0] >= 50 and at[8][0] >= 130 and at[1][0] < at[5][0] < at[8][0]
        # strand 0 to strand 1
        mk = [c - K + 1 for c in WX.MOVE_CHECKPOINTS]
        for n, (fwd, fbin, rev, rbin) in zip(mk, WX.strand_maxima(c.o, x, WX.MOVE_CHECKPOINTS)):
            assert rev == n and rbin == b and fwd <= n
        tail = WX.strand_maxima(c.o, y, WX.MOVE_CHECKPOINTS)
        assert tail[0][0] == 10 >= tail[0][2]                   # strand 0 holds the maximum at the first checkpoint (c8193's shared last bin ties)
        assert tail[0][0] > tail[0][2] or n_bins == 8193
        assert tail[-1][2] > tail[-1][0] and tail[-1][3] == b   # ... strand 1 and bin B at the last


def test_the_n_and_crafted_reads_and_the_counters_end():
    c = WX.prefix_fixture("c31000")
    # the N-carrying sequence: k-mers 54 .. 60 hold the N and are in the filter; checkpoints on either side and inside
    assert c.n_seq.index("N") == 60 and len(c.n_seq) == 121
    kmers = [x - K + 1 for x in WX.N_CHECKPOINTS[:-1]]
    assert {54, 57, 58, 61} <= set(kmers) and {1, 2, 69, 72, 76, 143, 144} <= set(kmers)
    fwd = [f for f, _, _, _ in WX.strand_maxima(c.o, c.n_seq, WX.N_CHECKPOINTS)]
    assert fwd[kmers.index(57)] > fwd[kmers.index(54)] and fwd[kmers.index(61)] > fwd[kmers.index(58)]  # the N k-mers count
    reads = c.n_checkpoint_reads()
    assert "N" * 40 in reads and any(r.startswith("N") for r in reads) and any(r.endswith("N") and len(r) == 150 for r in reads)
    assert any(r.find("N") == 75 for r in reads)
    # the crafted k-mers: the last k-mer of the range [20, 41) and the first of [41, 90)
    crafted = c.crafted_reads()[:2 * len(WR.CRAFTED)]
    ck = [x - K + 1 for x in WX.CRAFT_CHECKPOINTS[:-1]]
    assert ck == [20, WX.CRAFT_AT + 1, 90]
    for i, s in enumerate(WR.CRAFTED):
        assert crafted[2 * i][WX.CRAFT_AT:WX.CRAFT_AT + K] == s and crafted[2 * i + 1][WX.CRAFT_AT + 1:WX.CRAFT_AT + 1 + K] == s
    # the counter's end (on a cut of the read: the whole is the GPU test's business)
    assert len(WX.edge_read()) == WX.MAX_KMERS + K - 1 and set(WX.edge_read()) == {"C"}
    short = "C" * WX.bases(500)
    f = c.o.count(po.encode(short))
    assert int(f.max()) == 500 and int(f.argmax()) == 5
    assert [x - K + 1 for x in WX.EDGE_CHECKPOINTS] == [0xFFFE, 0xFFFF] and WX.OVER_CHECKPOINTS[-1] - K + 1 == 0x10000


def test_the_take_model():
    """every kind of item, whole and behind an odd chunk_start, under both bounds: an N changes nothing, a short or empty item is taken,
    a chunk beyond the read and an item beyond an understated bound are left"""
    seen = set()
    for start in (0, WX.ODD_START):
        reads, kinds = WX.mixed_items(start)
        for bound in (WX.WIDE_BOUND, WX.UNDERSTATED):
            for r, kind in zip(reads, kinds):
                t = WX.takes(r, WX.C_LAST, chunk_start=start, max_len=bound)
                assert t == WX.want_taken(kind, start, bound), (kind, start, bound)
                seen.add((kind, t))
            model = WX.taken_counts(reads, WX.C_LAST, chunk_start=start, max_len=bound)
            lists = XL.taken_counts(reads, WX.C_LAST, chunk_start=start, max_len=bound)
            assert model[0] > lists[0] and sum(model) == sum(lists) == len(reads)  # the items with an N are the difference
            assert model[1] >= (1 if bound == WX.UNDERSTATED or start else 0)
    assert {("n_first", True), ("n_before_last", True), ("n_at_last", True), ("short", True), ("empty", True), ("beyond", False), ("under", False),
            ("under", True), ("free_long", False), ("free_long", True)} <= seen


def test_the_three_calls_are_declared_and_bound():
    tuning = open(os.path.join(ROOT, "include", "readbouncer_amd_tuning.h")).read()
    assert "RB_API int rb_engine_set_wide_prefix_lists(rb_engine *e, int mode);" in tuning
    assert "RB_API int rb_engine_wide_prefix_lines(rb_engine *e, size_t filter_index, uint32_t max_len, uint32_t last_checkpoint, uint32_t *lines_out);" in tuning
    assert "RB_API int rb_engine_wide_prefix_lists_items(rb_engine *e, uint64_t *listed, uint64_t *plain, int reset);" in tuning
    boundary = open(os.path.join(ROOT, "include", "readbouncer_amd.h")).read()
    names = ("rb_engine_set_wide_prefix_lists", "rb_engine_wide_prefix_lines", "rb_engine_wide_prefix_lists_items")
    assert not any(n in boundary for n in names)
    assert set(names) <= set(capi.SIGNATURES)
    assert all(callable(getattr(capi.Engine, m)) for m in ("set_wide_prefix_lists", "wide_prefix_lines", "wide_prefix_lists_items"))
    assert [n for n, _ in capi.PrefixPlan._fields_][-1] == "list_lines" and len(capi.PrefixPlan._fields_) == 7  # rb_prefix_plan_info is as it was
    main = open(os.path.join(ROOT, "readbouncer_amd", "host", "rb_main.cpp")).read()
    assert '"--wide-prefix-lists"' in main and "int wide_prefix_lists = RB_PASS_LISTS_OFF;" in main and main.count("--wide-prefix-lists off|current|build") >= 3
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert mk.count("rb_wide_prefix_lists.o:") == 1 and "rb_wide_prefix_lists.o" in mk.split("OBJS")[1].split("\n")[0]


def test_wide_prefix_kernels_resources(tmp_path):
    found = compile_unit(tmp_path, "rb_wide_prefix_lists")
    want = {"ibf_prefix_wide_lists_kernel<%d,%d,4>" % (lines, nt) for lines in WR.WIDE_LINES for nt in (0, 1)} | {"wide_prefix_lists_prep_kernel"}
    assert set(found) == want and len(found) == 7, sorted(set(found) ^ want)  # the unit holds these kernels and no other
    assert not {k: v for k, v in found.items() if v["scratch"]}, found
    assert all(v["lds"] == 0 for v in found.values()), found  # static LDS 0: what the kernel uses is dynamic
    # the declared dynamic LDS is the count kernel's, to the byte
    src = open(os.path.join(CSRC, "rb_wide_prefix_lists.hip")).read()
    assert src.count("lds = rbwide::count_lds_bytes(a.f.n_bins, NW)") == 1 and "hipFuncAttributeMaxDynamicSharedMemorySize" not in src
    assert src.count("hipLaunchKernelGGL(kern, dim3(a.n_items), dim3(64 * NW), lds, st,") == 1
    out = subprocess.run([build_layout_program(tmp_path, False)], capture_output=True, text=True, check=True).stdout
    lds = {int(a): (int(b), int(c)) for a, b, c in re.findall(r"wide_count_lds n_bins (\d+) bytes (\d+) resident (\d+)", out)}
    assert lds[32256] == (65344, 2) and lds[31000][1] == 2
    for name, r in found.items():
        if name.startswith("wide_prefix_lists_prep_kernel"):
            continue
        assert r["vgpr"] <= 128 and r["occ"] >= 4, (name, r)  # four waves per SIMD: a workgroup is one wave per SIMD
        for n_bins in (31000, 32256):
            assert lds[n_bins][0] * lds[n_bins][1] <= LDS_PER_CU and r["occ"] >= lds[n_bins][1], (name, r, n_bins)


def test_the_sibling_units_hold_the_kernels_they_held(tmp_path):
    """WideShare moved into the shared header and wide_count_range stands beside wide_count_strand: the units that include the header
    hold the kernels they held"""
    assert len(compile_unit(tmp_path, "rb_wide_pass_lists")) == 13
    assert len(compile_unit(tmp_path, "rb_wide_lists")) == 7
    dev = open(os.path.join(CSRC, "rb_wide_lists_device.h")).read()
    assert all(s in dev for s in ("void wide_count_strand(", "void wide_count_range(", "struct WideShare {"))
    assert "wide_prefix" not in open(os.path.join(CSRC, "rb_kernels.hip")).read()

"""The list forms of locate and hits (rb_pass_lists.hip: ibf_locate_lists_kernel, ibf_hits_lists_kernel) at the edges of their 16-bit LDS
counters, bit for bit against the oracle through tests/locate_rules.py, tests/hits_rules.py and GP.run_both -- which also asserts that
Engine.plan_pass names the list form at the fixture's slot size and that RB_PASS_LISTS_OFF returns the same bytes:
  a. strands of 32 767 to 65 535 k-mers on filters with bins set in every block (tests/pass_lists_edges_rig.py): both halves of a counter
     dword at 0xFFFF, a saturated low half beside a pad half and beside a high half a little below it; the packed maximum above 32 767,
     the key (m << 16) | (0xFFFF - bin) at m = 65 535 and records of count 65 535 on either strand; then the list COUNT kernel on the
     same filters, which had met large counts in odd bins only;
  b. the guard: 65 535 k-mers is the last strand the list form serves, 65 536 takes the plain form (the saturated bins wrap to 0);
  c. truncation of the record lists at t == 0, where every lane of the scan holds eight hits: caps inside a piece, at a piece's edge, at
     a round's edge (512 bins) and around n_bins;
  d. an engine whose list-served filters differ in k (5 and 7), and the strand loop of list_count_strand at k = 5 (k = 13:
     tests/test_gpu_row_lists_wide_k.py).
What the fixtures claim of themselves is asserted without a GPU in tests/test_pass_lists_edges_cpu.py.  No tolerance, no assertion on
elapsed time."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from readbouncer_amd import capi
from tests import helpers as H
from tests import list_scan_rig as SR
from tests import pass_edges as PE
from tests import pass_lists_edges_rig as ER
from tests import pass_lists_rig as PL
from tests import test_gpu_hits as GH
from tests import test_gpu_list_scan as LS
from tests import test_gpu_locate as GL
from tests import test_gpu_pass_lists as GP
from tests import test_gpu_row_lists as LT
from tests import test_gpu_row_table as RT
from tests.hits_rules import expected_arrays

K, R, CONF = ER.K, PL.R, PL.CONF
TOP = ER.MAX_KMERS


def resident(n_bins, lines):
    return LS.resident(lambda words, info: ER.Edges(n_bins, lines, words), n_bins, SR.N_BLOCKS, lines)


# ------------------------------------------------------------------------------------------------ a. the top of the counters
@pytest.mark.parametrize("n_bins,lines", ER.GEOMETRIES)
def test_counter_top(n_bins, lines):
    """min_count 1 with room for every bin is every counter of both strands; min_count 0 the decision thresholds; min_count 65 535 the
    saturated bins alone"""
    d, f = resident(n_bins, lines)
    reads = ER.reads()
    top = [i for i, r in enumerate(reads) if len(r) - K + 1 == TOP]
    eng = GP.lists_engine([d])
    for nt in (0, 1):
        eng.set_nt_threshold(0 if nt else GP.NT_DEFAULT)
        exp, exp_n = GP.run_both(eng, [f.o], reads, [lines], ("edges", n_bins, lines, nt, "every counter"), min_count=1)
        assert exp_n[top, 0].tolist() == [2 * n_bins] * len(top)  # every bin of both strands has counted something by then
        GP.run_both(eng, [f.o], reads, [lines], ("edges", n_bins, lines, nt, "decision thresholds"), min_count=0)
        exp, exp_n = GP.run_both(eng, [f.o], reads, [lines], ("edges", n_bins, lines, nt, "at the top"), min_count=TOP)
        assert exp_n[:, 0].tolist() == [2 * len(f.sat) if i in top else 0 for i in range(len(reads))]
    assert len(top) == 2 and exp["max_count"][top, 0].tolist() == [TOP] * 2 and exp["best_bin"][top, 0].tolist() == [f.sat[0]] * 2
    eng.destroy()
    # the count kernel over the same filter and reads: large counts in even bins, and a dword with both halves at the top
    batch = H.pack_reads(reads)
    expected = RT.reference(f.raw, batch)
    assert expected[0][top, 0].tolist() == [TOP] * 2
    for nt in (0, 1):
        ce = LT.lists_engine(d, nt)
        for prune in (1, 0):
            ce.set_bound_pruning(prune)
            p = LT.check(ce, batch, expected, ("edges, count kernel", n_bins, lines, nt, prune), LT.LISTS_KERNEL, repeats=1)
            assert p["nontemporal"] == nt
        ce.destroy()
    d.free()


# ------------------------------------------------------------------------------------------------ b. the guard
def test_the_guard_at_65535_kmers():
    """one read per call: the call's max_len is the read's length"""
    n_bins, lines = 2112, 1
    d, f = resident(n_bins, lines)
    eng = GP.lists_engine([d])
    last = ER.reads()[ER.BIG.index(TOP)]
    assert len(last) == K + TOP - 1
    for min_count in (1, TOP):
        exp, exp_n = GP.run_both(eng, [f.o], [last], [lines], ("guard, 65535", min_count), min_count=min_count)
    assert (int(exp["max_count"][0, 0]), int(exp["best_bin"][0, 0]), int(exp["best_strand"][0, 0])) == (TOP, f.sat[0], 0)
    assert int(exp_n[0, 0]) == 2 * len(f.sat)
    # one k-mer more, with a current table: the plain form, whose counters are wider; as uint16_t the saturated bins are 0 again
    over = ER.over_read()
    assert len(over) == K + TOP and d.list_table_info()["bytes"] > 0 and d.list_table_info()["lines"] == lines
    exp, _ = GP.run_both(eng, [f.o], [over], [0], "guard, 65536", min_count=1)
    assert int(exp["best_bin"][0, 0]) == ER.EVEN_SAT + 1 and 0.9 * 65536 < int(exp["max_count"][0, 0]) < 65536
    # a batch with longer reads still: the whole call takes the plain form
    reads, _ = PE.batch("BIG", K)
    GP.run_both(eng, [f.o], list(reads), [0], "guard, BIG", min_count=1)
    eng.destroy()
    d.free()


# ------------------------------------------------------------------------------------------------ c. truncation with every lane full
def caps(n_bins):
    return (1, 3, 7, 8, 9, 511, 512, 513, n_bins - 1, n_bins, n_bins + 5)


@pytest.mark.parametrize("n_bins,lines", ((2112, 1), ER.ODD))
def test_truncation_with_every_lane_full(n_bins, lines):
    """t == 0: every existing bin is a hit on both strands, so every lane's piece places eight records (fewer where the bins end) in every
    round; whole record buffers over the sentinel: order, per-strand truncation, untouched slots"""
    reads, n_zero, _ = PL.threshold_reads()
    reads = reads[:n_zero]
    assert n_zero == 2
    d, f = resident(n_bins, lines)
    eng = GP.lists_engine([d])
    buf, offs, lens = H.pack_reads(reads)
    assert GP.plan_lines(eng, int(lens.max())) == [lines]
    ok = np.ones(len(reads), bool)
    st = np.zeros(len(reads), np.uint8)
    full = np.full((len(reads), 1), 2 * n_bins, np.uint32)
    for cap in caps(n_bins):
        exp_hits, exp_n, exp_prof, _ = expected_arrays([f.o], reads, ok, cap, min_count=0, r=R, conf=CONF, sentinel=GH.SENT)
        assert np.array_equal(exp_n, full)  # n_hits is exact whatever the cap
        got = eng.hits(buf, offs, lens, error_rate=R, significance=CONF, min_count=0, max_hits=cap, hits=GH.sentinel_hits(len(reads), 1, cap))
        GH.check(got, exp_hits, exp_n, st, ("t == 0", n_bins, "cap %d" % cap))
    prof = np.zeros(n_bins, np.uint64)
    got = eng.hits(buf, offs, lens, error_rate=R, significance=CONF, min_count=0, max_hits=0, bin_reads=prof)
    assert np.array_equal(got["n_hits"], full) and np.array_equal(got["status"], st)
    assert np.array_equal(prof, exp_prof) and prof.tolist() == [len(reads)] * n_bins
    eng.destroy()
    d.free()


# ------------------------------------------------------------------------------------------------ d. filters of different k
@pytest.fixture(scope="module")
def mixed():
    n5, blocks5 = ER.K5_GEOMETRY[:2]
    n7 = ER.K7_GEOMETRY[0]
    h5 = capi.HostIBF.create(n5, 3, ER.K5, SR.n_bits(n5, blocks5))
    h7 = capi.HostIBF.create(n7, 3, K, SR.n_bits(n7))
    m = ER.MixedK(h5.words(), h7.words(), ER.make_narrow())
    m._hosts = (h5, h7)  # (keep the words the oracles look at)
    d5, d7, dn = capi.DeviceIBF.upload(0, h5), capi.DeviceIBF.upload(0, h7), GL.upload(m.narrow)
    for d, want in ((d5, m.lines5), (d7, m.lines7)):
        info = d.list_table_build()
        assert info["refused"] == 0 and info["lines"] == want, info
    yield m, d5, d7, dn
    for d in (d5, d7, dn):
        d.free()


def test_list_served_filters_of_different_k(mixed):
    """the prep kernel decides once per call, with the engine's largest k, which items the list kernels take; each list kernel counts
    len - k + 1 k-mers with its own k.  GL.oracle_rows applies the engine's largest k: the reads of 5 and 6 bases are RB_ERR_SHORT_READ
    and report nothing, though the k = 5 filter holds their k-mers"""
    m, d5, d7, dn = mixed
    eng = GP.lists_engine([d5, d7, dn])
    exp, exp_n = GP.run_both(eng, m.filters(), m.reads, [m.lines5, m.lines7, 0], "mixed k")
    assert exp["status"].tolist() == [capi.RB_ERR_SHORT_READ] * 3 + [capi.RB_OK] * 4
    assert not exp["max_count"][:3].any() and not exp_n[:3].any()
    long = m.reads.index(max(m.reads[:-1], key=len))
    assert exp["max_count"][long].tolist() == [70 - ER.K5 + 1, 70 - K + 1, 70 - K + 1] and exp["best_bin"][long].tolist() == [ER.BIN_LONG] * 3
    GP.run_both(eng, m.filters(), m.reads, [m.lines5, m.lines7, 0], "mixed k, ids", ids=[6, 1, 5, 5, 2, 3, 0])
    eng.destroy()


def test_strand_loop_at_k5(mixed):
    """list_count_strand is a second copy of the count kernel's tile loop: strands of 1, 63, 64, 65 and 129 k-mers and ranks 0 and 4^k - 1
    on either strand, at k = 5 (a tile's bases: lanes 0 to 3 of the second load)"""
    m, d5, _, _ = mixed
    eng = GP.lists_engine([d5])
    for nt in (0, 1):
        eng.set_nt_threshold(0 if nt else GP.NT_DEFAULT)
        GP.run_both(eng, [m.o5], ER.strand_reads(ER.K5), [m.lines5], ("k = 5 strands", nt))
    eng.destroy()

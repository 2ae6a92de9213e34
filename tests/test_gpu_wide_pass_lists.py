"""Locate and hits from a filter's WIDE list table (rb_engine_set_wide_pass_lists; rb_wide_pass_lists.hip, ibf_locate_wide_lists_kernel
and ibf_hits_wide_lists_kernel: filters of 8193 to 32 256 bins, one workgroup of four waves per item) against the oracle, bit for bit,
through the C ABI and the existing reductions (tests/locate_rules.py, tests/hits_rules.py), and against the same call with the setting
OFF: the same bytes.  Every case asserts through Engine.wide_pass_lines that the wide form is what the call takes -- a call that silently
ran the plain form would prove nothing.  The fixtures are tests/wide_lists_rig.py's with the tie rows of tests/wide_pass_lists_rig.py
(k = 7: tables of 4^7 slots, filters of a few MB); what they claim of themselves is asserted without a GPU in
tests/test_wide_pass_lists_cpu.py.  No tolerance, no assertion on elapsed time."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import pyoracle as po
from readbouncer_amd import capi
from tests import helpers as H
from tests import test_gpu_hits as GH
from tests import test_gpu_locate as GL
from tests import test_gpu_row_table as RT
from tests import test_gpu_wide_lists as WL
from tests import wide_lists_rig as WR
from tests import wide_pass_lists_rig as WP
from tests.hits_rules import expected_arrays

K, R, CONF = WP.K, WP.R, WP.CONF
OFF, CURRENT, BUILD = capi.RB_PASS_LISTS_OFF, capi.RB_PASS_LISTS_CURRENT, capi.RB_PASS_LISTS_BUILD
CAP = 64
REACHED = set()  # (lines, non-temporal) of the wide launches the tests made: the closing test wants all six builds of each kernel


def engine(filters, mode=CURRENT, nt=0):
    eng = capi.Engine(0, list(filters), [])
    eng.set_nt_threshold(0 if nt else RT.NT_NEVER)
    eng.set_wide_pass_lists(mode)
    return eng


def same_bytes(a, b, what):
    for key in a:
        if isinstance(a[key], np.ndarray):
            assert a[key].tobytes() == b[key].tobytes(), (what, key)


@functools.lru_cache(maxsize=None)
def expectation(name, which):
    """the oracle's answer for a list of reads of a fixture, computed once: locate's rows, and hits at min_count 0 (the decision
    threshold) and 1 with room for CAP records"""
    c = WP.pass_fixture(name)
    reads = {"all": c.all_reads, "ties": c.tie_reads, "left": c.left_reads, "order": lambda: [c.order_read()] + c.tie_reads()}[which]()
    exp, _, _ = GL.oracle_rows([c.o], reads, R, CONF)
    ok = exp["status"] == capi.RB_OK
    hits = {mc: expected_arrays([c.o], reads, ok, CAP, min_count=mc, r=R, conf=CONF, sentinel=GH.SENT) for mc in (0, 1)}
    return reads, exp, hits


def run_both(eng, reads, exp, hits, lines, label, caps=(CAP,), min_counts=(0, 1)):
    """locate and hits of `reads` on a one-filter engine with the setting CURRENT -- the wide form: wide_pass_lines says `lines` --
    against the oracle, then with the setting OFF: the same bytes"""
    buf, offs, lens = H.pack_reads(list(reads))
    max_len = int(lens.max())
    n = len(reads)
    got = {}
    for setting in (CURRENT, OFF):
        eng.set_wide_pass_lists(setting)
        assert eng.wide_pass_lines(0, max_len) == (lines if setting == CURRENT else 0), (label, setting)
        loc = eng.locate(buf, offs, lens, error_rate=R, significance=CONF)
        GL.assert_same(loc, exp, "%s locate, setting %d" % (label, setting))
        out = [loc]
        for mc in min_counts:
            exp_hits, exp_n, exp_prof, _ = hits[mc]
            for cap in caps:  # (a shorter buffer holds the first records, and the sentinel behind a shorter list)
                prof = np.zeros(len(exp_prof), np.uint64)
                hit = eng.hits(buf, offs, lens, error_rate=R, significance=CONF, min_count=mc, max_hits=cap, bin_reads=prof,
                               hits=GH.sentinel_hits(n, 1, cap) if cap else None)
                GH.check(hit, np.ascontiguousarray(exp_hits[:, :, :cap]) if cap else None, exp_n, exp["status"],
                         "%s hits, min_count %d, cap %d, setting %d" % (label, mc, cap, setting))
                assert np.array_equal(prof, exp_prof), (label, setting, mc, cap)
                out += [hit, prof]
        got[setting] = out
    eng.set_wide_pass_lists(CURRENT)
    for a, b in zip(got[CURRENT], got[OFF]):
        if isinstance(a, dict):
            same_bytes(a, b, label)
        else:
            assert a.tobytes() == b.tobytes(), label


@pytest.fixture(scope="module", params=list(WR.COUNT_FIXTURES))
def served(request):
    c = WP.pass_fixture(request.param)
    d = WL.upload(c.o)
    info = d.wide_list_table_build()
    assert info["refused"] == 0 and info["lines"] == c.lines, info
    yield request.param, c, d
    d.free()


# ---------------------------------------------------------------- 1. every read of the fixture, both twins
@pytest.mark.parametrize("nt", (0, 1))
def test_all_reads_through_locate_and_hits(served, nt):
    """planted maxima at bins 0, 8191, 8192, 8193, both halves of the last counter dword and the last bin (the scan's ends, every wave's
    share); strands of 1 to 263 k-mers (the tile deal); counts that one wave alone added; flagged, swapped and overflow slots; N at the
    first, a middle and the last base and N alone; "", k - 1 bases and silent reads -- in ONE batch, hits at the decision threshold and at
    min_count 1, where every wave's share holds hits and n_hits far exceeds the cap"""
    name, c, d = served
    reads, exp, hits = expectation(name, "all")
    eng = engine([d], CURRENT, nt)
    run_both(eng, reads, exp, hits, c.lines, (name, "all", nt))
    REACHED.add((eng.wide_pass_lines(0, 400), nt))
    assert int(hits[1][1].max()) > 20 * CAP  # n_hits stays exact far beyond the cap
    eng.destroy()


# ---------------------------------------------------------------- 2. ties
def test_ties_across_waves_pieces_and_strands(served):
    name, c, d = served
    reads, exp, hits = expectation(name, "ties")
    eng = engine([d])
    run_both(eng, reads, exp, hits, c.lines, (name, "ties"))
    assert list(zip(exp["best_bin"][:, 0].tolist(), exp["best_strand"][:, 0].tolist())) == \
        [c.tie_want[t] for t in ("two_waves", "one_piece", "same_bin", "rev_lower")]
    assert exp["max_count"][:, 0].tolist() == [1, 1, 1, 1]
    eng.destroy()


# ---------------------------------------------------------------- 3. caps, record order, the profile
def test_caps_order_and_the_profile(served):
    """max_hits 0, 1, 64 and above the total; CRAFTED[0] x 20 -- cap + 1 random bins from an overflow slot -- puts records across every
    wave boundary of the scan; the profile accumulates over two calls"""
    name, c, d = served
    reads, exp, hits = expectation(name, "order")
    eng = engine([d])
    run_both(eng, reads, exp, hits, c.lines, (name, "caps"), caps=(0, 1, CAP))
    total = int(hits[1][1].max())
    assert total >= c.cap + 1
    ok = exp["status"] == capi.RB_OK
    above = total + 5
    exp_hits, exp_n, exp_prof, lists = expected_arrays([c.o], reads, ok, above, min_count=1, r=R, conf=CONF, sentinel=GH.SENT)
    bins = [b for b, _, _ in lists[0][0]]
    assert {WP.share_of_bin(c.n_bins, b) for b in bins} == set(range(WR.WAVES))  # records in every wave's share
    buf, offs, lens = H.pack_reads(reads)
    assert eng.wide_pass_lines(0, int(lens.max())) == c.lines
    prof = np.zeros(c.n_bins, np.uint64)
    for rep in range(2):
        got = eng.hits(buf, offs, lens, error_rate=R, significance=CONF, min_count=1, max_hits=above, bin_reads=prof,
                       hits=GH.sentinel_hits(len(reads), 1, above))
        GH.check(got, exp_hits, exp_n, exp["status"], (name, "above the total", rep))
    assert np.array_equal(prof, 2 * exp_prof)
    eng.destroy()


# ---------------------------------------------------------------- 4. the counter's end
def test_the_counters_end_and_a_strand_too_long():
    c = WP.pass_fixture("c8193")
    d = WL.upload(c.o)
    d.wide_list_table_build()
    eng = engine([d])
    full = ["C" * (65535 + K - 1), "C" * 500]
    exp, _, _ = GL.oracle_rows([c.o], full, R, CONF)
    assert exp["max_count"][:, 0].tolist() == [65535, 500 - K + 1] and exp["best_bin"][:, 0].tolist() == [5, 5]
    ok = exp["status"] == capi.RB_OK
    hits = {1: expected_arrays([c.o], full, ok, CAP, min_count=1, r=R, conf=CONF, sentinel=GH.SENT)}
    run_both(eng, full, exp, hits, c.lines, "65535 k-mers", min_counts=(1,))
    # 65 536 k-mers: wide_form_serves refuses the call's max_len, and the plain form answers
    longer = ["C" * (65536 + K - 1), "C" * 500]
    buf, offs, lens = H.pack_reads(longer)
    assert eng.wide_pass_lines(0, int(lens.max())) == 0 and eng.wide_pass_lines(0, 65535 + K - 1) == c.lines
    exp2, _, _ = GL.oracle_rows([c.o], longer, R, CONF)
    GL.assert_same(eng.locate(buf, offs, lens, error_rate=R, significance=CONF), exp2, "65536 k-mers")
    eng.destroy(), d.free()


# ---------------------------------------------------------------- 5. items the form leaves
def chunk_expectation(o, reads, start, length, max_len, cap):
    chunks = [(r[start:start + length] if length else r[start:]) for r in reads]
    exp, _, _ = GL.oracle_rows([o], chunks, R, CONF)
    for i, r in enumerate(reads):
        bad = capi.RB_ERR_BAD_CHUNK if start > len(r) else (capi.RB_ERR_INVALID_ARG if len(chunks[i]) > max_len else None)
        if bad is not None:
            exp["status"][i] = bad
            exp["max_count"][i], exp["best_bin"][i], exp["best_strand"][i], exp["hit_bins"][i] = 0, -1, 0, 0
    return exp, expected_arrays([o], chunks, exp["status"] == capi.RB_OK, cap, min_count=1, r=R, conf=CONF, sentinel=GH.SENT)


def test_items_the_form_leaves():
    """one batch interleaves items the wide kernels take -- N-free and with N -- with items they leave: shorter than k, empty, longer
    than the declared max_len, a chunk that begins beyond the read; as ASCII and as packed 2-bit + N mask, whole and in chunk windows,
    with read_ids (a permuted subset with a repeat), through the host and the device forms"""
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda:0")
    name = "c31000"
    c = WP.pass_fixture(name)
    d = WL.upload(c.o)
    d.wide_list_table_build()
    eng = engine([d])
    reads, exp, hits = expectation(name, "left")
    run_both(eng, reads, exp, hits, c.lines, "left, host")
    n, cap, n_bins = len(reads), CAP, c.n_bins
    max_len = 140  # below the longest item (150 bases): RB_ERR_INVALID_ARG, and the wide kernels leave it
    assert sum(len(r) > max_len for r in reads) >= 1
    buf, offs, lens = H.pack_reads(reads)
    packed, p_offs, nmask, n_offs = capi.pack_reads(buf, offs, lens)
    t = {k: torch.from_numpy(np.ascontiguousarray(a)).to(dev) for k, a in (("seq", buf), ("off", offs.view(np.int64)), ("len", lens.view(np.int32)),
         ("p", packed), ("po", p_offs.view(np.int64)), ("nm", nmask), ("no", n_offs.view(np.int64)))}
    ids = np.array([6, 2, 2, 0, 4, 1, 3], dtype=np.uint32)
    t["ids"] = torch.from_numpy(ids.view(np.int32)).to(dev)

    def run(setting, packed_form, start, length, with_ids):
        eng.set_wide_pass_lists(setting)
        m = len(ids) if with_ids else n
        o = {"max_count": torch.full((m, 1), 77, dtype=torch.int16, device=dev), "best_bin": torch.full((m, 1), 77, dtype=torch.int32, device=dev),
             "best_strand": torch.full((m, 1), 77, dtype=torch.uint8, device=dev), "hit_bins": torch.full((m, 1), 77, dtype=torch.int32, device=dev),
             "status": torch.full((m,), 77, dtype=torch.uint8, device=dev), "hits": torch.full((m, 1, cap, 8), GH.SENT, dtype=torch.uint8, device=dev),
             "n_hits": torch.full((m, 1), 77, dtype=torch.int32, device=dev), "hstatus": torch.full((m,), 77, dtype=torch.uint8, device=dev),
             "prof": torch.zeros(n_bins, dtype=torch.int64, device=dev)}
        torch.cuda.synchronize()
        src = dict(d_nmask=t["nm"].data_ptr(), d_nmask_offsets=t["no"].data_ptr()) if packed_form else {}
        seq, off = (t["p"], t["po"]) if packed_form else (t["seq"], t["off"])
        kw = dict(chunk_start=start, chunk_length=length, d_read_ids=t["ids"].data_ptr() if with_ids else None, error_rate=R, significance=CONF, **src)
        eng.locate_device(seq.data_ptr(), off.data_ptr(), t["len"].data_ptr(), m, max_len, d_max_count=o["max_count"].data_ptr(),
                          d_best_bin=o["best_bin"].data_ptr(), d_best_strand=o["best_strand"].data_ptr(), d_hit_bins=o["hit_bins"].data_ptr(),
                          d_status=o["status"].data_ptr(), **kw)
        eng.hits_device(seq.data_ptr(), off.data_ptr(), t["len"].data_ptr(), m, max_len, min_count=1, max_hits=cap, d_hits=o["hits"].data_ptr(),
                        d_n_hits=o["n_hits"].data_ptr(), d_status=o["hstatus"].data_ptr(), d_bin_reads=o["prof"].data_ptr(), **kw)
        torch.cuda.synchronize()
        return {k: v.cpu().numpy() for k, v in o.items()}

    assert eng.wide_pass_lines(0, max_len) == c.lines
    for start, length in ((0, 0), (3, 100), (95, 0), (55, 30)):  # whole; a window; beyond the short items; a window around the N
        cexp, (exp_hits, exp_n, exp_prof, _) = chunk_expectation(c.o, reads, start, length, max_len, cap)
        assert (cexp["status"] == capi.RB_OK).sum() >= 3 and (cexp["status"] != capi.RB_OK).sum() >= 2
        for packed_form in (False, True):
            for with_ids in (False, True):
                sel = ids.astype(np.int64) if with_ids else np.arange(n)
                got = {s: run(s, packed_form, start, length, with_ids) for s in (CURRENT, OFF)}
                what = ("device", start, length, packed_form, with_ids)
                for s in (CURRENT, OFF):
                    g = got[s]
                    loc = {"max_count": g["max_count"].view(np.uint16), "best_bin": g["best_bin"], "best_strand": g["best_strand"],
                           "hit_bins": g["hit_bins"].view(np.uint32), "status": g["status"]}
                    GL.assert_same(loc, {k: v[sel] for k, v in cexp.items()}, what + (s,))
                    hit = {"hits": g["hits"].view(GH.HIT).reshape(len(sel), 1, cap), "n_hits": g["n_hits"].view(np.uint32), "status": g["hstatus"]}
                    GH.check(hit, exp_hits[sel], exp_n[sel], cexp["status"][sel], what + (s,))
                assert all(got[CURRENT][k].tobytes() == got[OFF][k].tobytes() for k in got[OFF]), what
    eng.destroy(), d.free()


# ---------------------------------------------------------------- 6. engines of several filters
def test_a_wide_filter_beside_a_narrow_and_a_list_served_one():
    """the form is per filter: a wide-served filter, a 600-bin filter on the plain form and an 8192-bin filter on the one-wave list form
    (rb_engine_set_pass_lists on as well) in one call"""
    name = "c8193"
    c = WP.pass_fixture(name)
    wide = WL.upload(c.o)
    wide.wide_list_table_build()
    narrow, o_nar = RT.device_filter(600, 4099, 3, K, seed=4, plant=[(c.plants[1][0], 7)])
    lst, o_lst = RT.device_filter(8192, 16381, 3, K, seed=9, plant=[(c.plants[0][0], 100)])
    lst.list_table_build()
    reads = [r for r, _ in c.planted_reads()][:9] + c.n_reads()[:6] + c.tie_reads() + ["ACGT"]
    buf, offs, lens = H.pack_reads(reads)
    max_len = int(lens.max())
    for filters, oracles, pass_lists in (([wide, narrow], [c.o, o_nar], OFF), ([narrow, wide, lst], [o_nar, c.o, o_lst], CURRENT)):
        eng = engine(filters)
        eng.set_pass_lists(pass_lists)
        fi = filters.index(wide)
        exp, _, _ = GL.oracle_rows(oracles, reads, R, CONF)
        ok = exp["status"] == capi.RB_OK
        exp_hits, exp_n, exp_prof, _ = expected_arrays(oracles, reads, ok, CAP, min_count=1, r=R, conf=CONF, sentinel=GH.SENT)
        got = {}
        for setting in (CURRENT, OFF):
            eng.set_wide_pass_lists(setting)
            want_lines = [c.lines if (f is wide and setting == CURRENT) else 0 for f in filters]
            assert [eng.wide_pass_lines(j, max_len) for j in range(len(filters))] == want_lines
            assert [eng.plan_pass(j, max_len)["list_lines"] > 0 for j in range(len(filters))] == [f is lst and pass_lists != OFF for f in filters]
            loc = eng.locate(buf, offs, lens, error_rate=R, significance=CONF)
            GL.assert_same(loc, exp, ("engines", len(filters), setting))
            prof = np.zeros(len(exp_prof), np.uint64)
            hit = eng.hits(buf, offs, lens, error_rate=R, significance=CONF, min_count=1, max_hits=CAP, bin_reads=prof,
                           hits=GH.sentinel_hits(len(reads), len(filters), CAP))
            GH.check(hit, exp_hits, exp_n, exp["status"], ("engines", len(filters), setting))
            assert np.array_equal(prof, exp_prof)
            got[setting] = (loc, hit)
        same_bytes(got[CURRENT][0], got[OFF][0], "engines locate")
        same_bytes(got[CURRENT][1], got[OFF][1], "engines hits")
        assert eng.wide_pass_lines(fi, max_len) == 0  # (left OFF)
        eng.destroy()
    for d in (wide, narrow, lst):
        d.free()


# ---------------------------------------------------------------- 7. the setting
def test_the_setting():
    name = "c8193"
    c = WP.pass_fixture(name)
    d = WL.upload(c.o)
    rng = np.random.default_rng(41)  # (48 random reads of 400 bases: with them the batch alone repays a table of 4^7 slots)
    reads = [r for r, _ in c.planted_reads()] + c.n_reads() + c.tie_reads() + [WR.random_dna(rng, 400) for _ in range(48)]
    buf, offs, lens = H.pack_reads(reads)
    max_len = int(lens.max())
    exp, _, _ = GL.oracle_rows([c.o], reads, R, CONF)
    eng = capi.Engine(0, [d], [])

    def locate_is(want_lines, expectation, what):
        assert eng.wide_pass_lines(0, max_len) == want_lines, what
        GL.assert_same(eng.locate(buf, offs, lens, error_rate=R, significance=CONF), expectation, what)

    locate_is(0, exp, "default: off")
    for bad in (3, -1):
        with pytest.raises(Exception):
            eng.set_wide_pass_lists(bad)
    # the other settings do not reach locate or hits
    eng.set_wide_lists(BUILD), eng.set_pass_lists(BUILD)
    locate_is(0, exp, "wide_lists and pass_lists alone")
    assert d.wide_list_table_info()["builds"] == 0 and d.list_table_info()["builds"] == 0
    eng.set_wide_lists(OFF), eng.set_pass_lists(OFF)
    # CURRENT without a table: the plain form, and the call builds none
    eng.set_wide_pass_lists(CURRENT)
    locate_is(0, exp, "current, no table")
    assert d.wide_list_table_info()["builds"] == 0 and d.wide_list_table_info()["bytes"] == 0
    # BUILD: a batch that does not repay the build stays plain; this one builds, 0 -> 1
    eng.set_wide_pass_lists(BUILD)
    small = H.pack_reads(reads[:2])
    eng.locate(*small, error_rate=R, significance=CONF)
    assert d.wide_list_table_info()["builds"] == 0
    assert eng.wide_pass_lines(0, max_len) == 0  # (asking builds nothing)
    GL.assert_same(eng.locate(buf, offs, lens, error_rate=R, significance=CONF), exp, "build")
    info = d.wide_list_table_info()
    assert info["builds"] == 1 and info["lines"] == c.lines and eng.wide_pass_lines(0, max_len) == c.lines, info
    ok = exp["status"] == capi.RB_OK
    exp_hits, exp_n, _, _ = expected_arrays([c.o], reads, ok, CAP, min_count=1, r=R, conf=CONF, sentinel=GH.SENT)
    GH.check(eng.hits(buf, offs, lens, error_rate=R, significance=CONF, min_count=1, max_hits=CAP, hits=GH.sentinel_hits(len(reads), 1, CAP)),
             exp_hits, exp_n, exp["status"], "hits under build")
    assert d.wide_list_table_info()["builds"] == 1
    # OFF with a table: plain
    eng.set_wide_pass_lists(OFF)
    locate_is(0, exp, "off, table present")
    # an insert drops the table: CURRENT is plain and follows the new bits
    eng.set_wide_pass_lists(CURRENT)
    locate_is(c.lines, exp, "current")
    moved = reads[0]
    d.insert(moved, [0], [len(moved)], [100])
    after, _, _ = GL.oracle_rows([RT.oracle_view(d)], reads, R, CONF)
    assert not np.array_equal(after["hit_bins"], exp["hit_bins"])
    locate_is(0, after, "current, after the insert")
    assert d.wide_list_table_info()["builds"] == 1 and d.wide_list_table_info()["bytes"] == 0
    eng.destroy(), d.free()
    # the dense filter is refused and served plain
    dense = WL.upload(WR.table_fixture("dense"))
    o = WR.table_fixture("dense")
    eng = engine([dense], BUILD)
    rng = np.random.default_rng(7)
    batch = [WR.random_dna(rng, 300) for _ in range(64)]
    dexp, _, _ = GL.oracle_rows([o], batch, R, CONF)
    b = H.pack_reads(batch)
    GL.assert_same(eng.locate(*b, error_rate=R, significance=CONF), dexp, "dense")
    info = dense.wide_list_table_info()
    assert info["refused"] == capi.RB_LIST_REFUSED_DENSITY and info["builds"] == 0 and eng.wide_pass_lines(0, 300) == 0, info
    eng.destroy(), dense.free()


def test_every_slot_size_and_both_twins_were_reached():
    assert REACHED == {(lines, nt) for lines in WR.WIDE_LINES for nt in (0, 1)}, sorted(REACHED)

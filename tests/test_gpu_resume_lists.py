"""The resume pass from a filter's list table (rb_resume_set_lists; rb_resume_lists.hip, ibf_resume_lists_kernel) against the oracle, bit
for bit, through the C ABI and tests/resume_rules.py: rows after every feed, and Resume.counts of every bin on both strands at the points
named.  Every case asserts that Resume.plan names the list form at the fixture's slot size -- a call that silently ran the plain form
would prove nothing --, that at least one item of the call is N-free (the list kernel's item), and runs the same schedule on a second
slot set under RB_PASS_LISTS_OFF whose rows and counts must be the same bytes.  The fixtures are the k = 7 rigs of
tests/list_scan_rig.py, tests/pass_lists_rig.py and tests/pass_lists_edges_rig.py (tables of 4^7 slots, 1021 blocks); what the new cases
claim of them is asserted without a GPU in tests/test_resume_lists_cpu.py.  No tolerance, no assertion on elapsed time."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import pyoracle as po
from readbouncer_amd import capi
from tests import helpers as H
from tests import list_scan_rig as SR
from tests import pass_edges as PE
from tests import pass_lists_edges_rig as ER
from tests import resume_lists_rig as RL
from tests import resume_rules as RR
from tests import test_gpu_list_scan as LS
from tests import test_gpu_resume as GR
from tests.test_gpu_hits import upload

K, R, CONF = SR.K, PE.R, PE.CONF
OFF, CURRENT, BUILD = capi.RB_PASS_LISTS_OFF, capi.RB_PASS_LISTS_CURRENT, capi.RB_PASS_LISTS_BUILD
FIRST, PEEK = capi.RB_RESUME_FIRST, capi.RB_RESUME_PEEK
MODE = capi.RB_MODE_CHECK_UNBLOCK
NT_DEFAULT = 512 << 20


def plan_lines(rs, nf=1):
    return [rs.plan(j)["list_lines"] for j in range(nf)]


class Twin:
    """One engine, two slot sets fed the same items: `rs` under the setting, `off` under RB_PASS_LISTS_OFF, and the oracle's model of
    both.  feed() checks the plan, that the call holds an item the list kernel takes, the rows against the oracle and the two sets'
    rows against each other; check() does the same for the counters."""

    def __init__(self, eng, filters, lines, n_slots, max_chunk_len, max_total_len, mode=CURRENT):
        self.eng, self.filters, self.lines, self.nf = eng, list(filters), list(lines), len(filters)
        self.rs = eng.resume(n_slots, max_chunk_len, max_total_len)
        self.off = eng.resume(n_slots, max_chunk_len, max_total_len)
        self.rs.set_lists(mode)
        self.model = RR.Model(n_slots, max_chunk_len, max_total_len)

    def feed(self, items, what, lines=None, need_free=True, bad_chunk=(), feeder=None):
        lines = self.lines if lines is None else lines
        assert plan_lines(self.rs, self.nf) == list(lines), (what, plan_lines(self.rs, self.nf))
        assert plan_lines(self.off, self.nf) == [0] * self.nf, what
        taken = RL.taken_items(self.model, items, K, bad_chunk)
        assert any(taken) or not need_free, what
        feeder = feeder or (lambda rs: GR.feed(rs, items, MODE, R, CONF))
        got = feeder(self.rs)
        exp = self.model.feed(items, self.filters, [], MODE, R, CONF, bad_chunk=bad_chunk)
        RR.assert_same(got, exp, "%s, list form" % (what,))
        plain = feeder(self.off)
        RR.assert_same(plain, exp, "%s, setting off" % (what,))
        for key in RR.KEYS:
            assert got[key].tobytes() == plain[key].tobytes(), (what, key)
        return got, exp, taken

    def check(self, slots, what):
        for s in slots:
            for fi, f in enumerate(self.filters):
                exp = self.model.counts(s, f)
                a, ta = self.rs.counts(s, fi)
                b, tb = self.off.counts(s, fi)
                RR.assert_counts(a, exp, "%s slot %d filter %d, list form" % (what, s, fi))
                RR.assert_counts(b, exp, "%s slot %d filter %d, setting off" % (what, s, fi))
                assert a.tobytes() == b.tobytes() and ta == tb == self.model.total(s), (what, s, fi)

    def close(self):
        self.rs.destroy()
        self.off.destroy()


# ------------------------------------------------------------------------------------------------ 1. a schedule per geometry
@pytest.mark.parametrize("n_bins,lines", SR.GEOMETRIES)
def test_schedule_per_geometry(n_bins, lines):
    """chunks below k, across the seam, an empty chunk, a full tile and a part tile, on reads planted where a lane's columns begin and
    end; temporal gathers and, on a third slot set, non-temporal ones"""
    d, f = LS.resident(lambda words, info: SR.Planted(n_bins, lines, words), n_bins, SR.N_BLOCKS, lines)
    eng = capi.Engine(0, [d], [])
    reads = RL.schedule_reads(f)
    n = len(reads)
    tw = Twin(eng, [f.o], [lines], n, RL.MAX_CHUNK, RL.MAX_TOTAL)
    nt = eng.resume(n, RL.MAX_CHUNK, RL.MAX_TOTAL)
    nt.set_lists(CURRENT)
    try:
        pos = [0] * n
        for step, c in enumerate(RL.schedule(K)):
            items = []
            for s in range(n):
                chunk = reads[s][pos[s]:pos[s] + c]
                pos[s] += len(chunk)
                items.append((s, chunk, FIRST if step == 0 else 0))
            got, exp, _ = tw.feed(items, ("schedule", n_bins, lines, step, c))
            eng.set_nt_threshold(0)
            again = GR.feed(nt, items, MODE, R, CONF)
            eng.set_nt_threshold(NT_DEFAULT)
            for key in RR.KEYS:
                assert again[key].tobytes() == got[key].tobytes(), (n_bins, lines, step, key)
            if step in RL.COUNT_CHECKS:
                tw.check(range(n), ("schedule", n_bins, lines, step))
                for s in range(n):
                    assert nt.counts(s, 0)[0].tobytes() == tw.rs.counts(s, 0)[0].tobytes()
        # a planted read counts all of its k-mers in its bin
        assert int(tw.rs.counts(0, 0)[0][0, f.bins[0]]) == f.kmers[0]
    finally:
        nt.destroy()
        tw.close()
        eng.destroy()
        d.free()


# ------------------------------------------------------------------------------------------------ 2. the wrap and the carry
@pytest.mark.parametrize("n_bins,lines", RL.WRAP_GEOMETRIES)
def test_the_wrap_and_the_carry(n_bins, lines):
    """the bins set in every block stand at 0xFFFF, then 0, then 1; EVEN_SAT + 1 takes no carry from EVEN_SAT; the pad half beside the
    last bin of an odd bin count never shows; on a read and on its reverse complement"""
    d, f = LS.resident(lambda words, info: ER.Edges(n_bins, lines, words), n_bins, SR.N_BLOCKS, lines)
    eng = capi.Engine(0, [d], [])
    ends = RL.wrap_ends(K)
    max_chunk = max(b - a for a, b in zip((0,) + ends, ends))
    assert max_chunk < 65536
    tw = Twin(eng, [f.o], [lines], 2, max_chunk, RL.WRAP_MAX_TOTAL)
    reads = RL.wrap_reads(K)
    try:
        pos = 0
        for step, (e, sat) in enumerate(zip(ends, RL.WRAP_SAT)):
            items = [(s, reads[s][pos:e], FIRST if step == 0 else 0) for s in range(2)]
            got, exp, taken = tw.feed(items, ("wrap", n_bins, e - K + 1))
            pos = e
            assert taken == [True, True]
            tw.check(range(2), ("wrap", n_bins, e - K + 1))
            for s in range(2):
                counts, total = tw.rs.counts(s, 0)
                assert total == e
                for b in f.sat:
                    assert counts[:, b].tolist() == [sat, sat], (n_bins, e, s, b)
                assert int(got["max_count"][s, 0]) == int(counts.max()) == int(exp["max_count"][s, 0])
        counts, _ = tw.rs.counts(0, 0)
        assert 0 < int(counts[0, ER.EVEN_SAT + 1]) < 70000 - 65536 + 1  # wrapped by itself, not pushed by its neighbour
    finally:
        tw.close()
        eng.destroy()
        d.free()


# ------------------------------------------------------------------------------------------------ small rigs for the other cases
def planted(n_bins=2112, lines=1):
    d, f = LS.resident(lambda words, info: SR.Planted(n_bins, lines, words), n_bins, SR.N_BLOCKS, lines)
    return d, f, capi.Engine(0, [d], [])


# ------------------------------------------------------------------------------------------------ 3. FIRST and PEEK
def test_first_and_peek():
    d, f, eng = planted()
    a, b = f.plants[3] + f.plants[4], SR.rc(f.plants[5] + f.plants[6])
    tw = Twin(eng, [f.o], [1], 4, 200, 1000)
    try:
        tw.feed([(0, a[:100], FIRST), (1, b[:90], FIRST)], "first chunks")
        before = [tw.rs.counts(s, 0) for s in range(2)]
        rows = [tw.feed([(0, a[100:170], PEEK), (1, b[90:95], PEEK)], "peek %d" % i)[0] for i in range(2)]
        assert all(rows[0][key].tobytes() == rows[1][key].tobytes() for key in RR.KEYS)
        for s in range(2):  # the PEEKs changed nothing
            after = tw.rs.counts(s, 0)
            assert after[0].tobytes() == before[s][0].tobytes() and after[1] == before[s][1]
        same, _, _ = tw.feed([(0, a[100:170], 0), (1, b[90:95], 0)], "the same chunks, committed")
        assert all(same[key].tobytes() == rows[0][key].tobytes() for key in RR.KEYS)
        tw.check(range(2), "after the commit")
        # FIRST on a used slot equals a fresh slot (slot 2 was never fed)
        g, _, _ = tw.feed([(0, b[:150], FIRST), (2, b[:150], FIRST)], "FIRST on a used and on a fresh slot")
        assert all(g[key][0].tobytes() == g[key][1].tobytes() for key in RR.KEYS)
        assert tw.rs.counts(0, 0)[0].tobytes() == tw.rs.counts(2, 0)[0].tobytes()
        tw.check((0, 2), "after FIRST")
        # FIRST | PEEK leaves the slot as it was
        before = tw.rs.counts(1, 0)
        tw.feed([(1, a[:120], FIRST | PEEK)], "FIRST | PEEK")
        after = tw.rs.counts(1, 0)
        assert after[0].tobytes() == before[0].tobytes() and after[1] == before[1]
        tw.check((1,), "after FIRST | PEEK")
        # FIRST with an empty chunk: the slot reads all zero afterwards
        tw.feed([(1, "", FIRST), (0, a[150:160], 0)], "FIRST with an empty chunk")
        counts, total = tw.rs.counts(1, 0)
        assert total == 0 and not counts.any()
        tw.check((0, 1), "after the empty FIRST")
    finally:
        tw.close()
        eng.destroy()
        d.free()


# ------------------------------------------------------------------------------------------------ 4. who takes which item
def test_who_takes_which_item():
    torch = pytest.importorskip("torch")
    d, f, eng = planted(4090, 2)
    tw = Twin(eng, [f.o], [2], RL.MIX_SLOTS, RL.MIX_MAX_CHUNK, 2000)
    try:
        first, second, third, kinds = RL.mixed_feeds(f)

        def through_device(items):  # (the device form refuses item by item)
            return lambda rs: GR.device_feed(torch, rs, 1, [c for _, c, _ in items], [s for s, _, _ in items], [fl for _, _, fl in items])
        _, exp, taken = tw.feed(first, "mixed, first feed", feeder=through_device(first))
        assert exp["status"][kinds.index("bad_slot")] == exp["status"][kinds.index("too_long")] == capi.RB_ERR_INVALID_ARG
        assert taken == [k in ("free", "short") for k in kinds], list(zip(kinds, taken))
        tw.check(range(RL.MIX_SLOTS), "mixed, first feed")
        # N-free chunks everywhere: the slot whose tail carries the N stays with the plain form, the others return to the list form
        _, _, taken = tw.feed(second, "mixed, second feed", feeder=through_device(second))
        assert taken == [k not in ("n_last", "bad_slot", "too_long") for k in kinds], list(zip(kinds, taken))
        tw.check(range(RL.MIX_SLOTS), "mixed, second feed")
        # ... and that slot returns to the list form on state the plain form wrote
        _, _, taken = tw.feed(third, "mixed, third feed", feeder=through_device(third))
        assert taken[kinds.index("n_last")] and taken[kinds.index("n_first")]
        tw.check(range(RL.MIX_SLOTS), "mixed, third feed")
    finally:
        tw.close()
        eng.destroy()
        d.free()


# ------------------------------------------------------------------------------------------------ 5. alternating forms on one slot
def test_alternating_forms_on_one_slot():
    """list, plain, list, plain on one slot set against a twin whose setting never changes: the slot format is one"""
    d, f, eng = planted(8192, 2)
    reads = RL.schedule_reads(f)[:8]
    tw = Twin(eng, [f.o], [2], len(reads), 100, 1000)
    try:
        for step in range(4):
            mode = CURRENT if step % 2 == 0 else OFF
            tw.rs.set_lists(mode)
            items = [(s, r[60 * step:60 * step + 60], FIRST if step == 0 else 0) for s, r in enumerate(reads)]
            tw.feed(items, ("alternating", step), lines=[2] if mode == CURRENT else [0])
            tw.check(range(len(reads)), ("alternating", step))
    finally:
        tw.close()
        eng.destroy()
        d.free()


# ------------------------------------------------------------------------------------------------ 6. engines of several filters
def test_engines_of_several_filters():
    """a list-served filter, a narrow one that does not qualify, and a second list-served filter of another slot size, under all three
    modes in one schedule"""
    d0, f0 = LS.resident(lambda words, info: SR.Planted(2112, 1, words), 2112, SR.N_BLOCKS, 1)
    d2, f2 = LS.resident(lambda words, info: SR.Planted(8192, 4, words), 8192, SR.N_BLOCKS, 4)
    narrow = ER.make_narrow()
    reads = [f0.plants[2] + f2.plants[5], SR.rc(f2.plants[1] + f0.plants[7]), f0.plants[9][:40] + "N" + f2.plants[9], f2.plants[3]]
    narrow.insert(po.encode(reads[0]), 77)
    d1 = upload(narrow)
    eng = capi.Engine(0, [d0, d1, d2], [])
    filters = [f0.o, narrow, f2.o]
    tw = Twin(eng, filters, [1, 0, 4], len(reads), 64, 1000)
    try:
        d2.list_table_drop()
        for step, (mode, lines) in enumerate(((CURRENT, [1, 0, 0]), (OFF, [0, 0, 0]), (BUILD, [1, 0, 0]), (BUILD, [1, 0, 4]), (CURRENT, [1, 0, 4]))):
            tw.rs.set_lists(mode)
            items = [(s, r[50 * step:50 * step + 50], FIRST if step == 0 else 0) for s, r in enumerate(reads)]
            tw.feed(items, ("several filters", step), lines=lines)  # (under BUILD the call builds; the plan names the table afterwards)
            tw.check(range(len(reads)), ("several filters", step))
        assert int(tw.rs.counts(0, 1)[0].max()) > 100  # the narrow filter counted too
    finally:
        tw.close()
        eng.destroy()
        for dev in (d0, d1, d2):
            dev.free()


# ------------------------------------------------------------------------------------------------ 7. the setting
def test_the_setting():
    n_bins, lines = 2112, 1
    made = {}
    from tests import test_gpu_row_lists as LT
    d, owner = LT.uploaded(n_bins, SR.N_BLOCKS, K, lambda w, host: made.update(f=SR.Planted(n_bins, lines, host.words())))
    f = made["f"]
    eng = capi.Engine(0, [d], [])
    reads = RL.schedule_reads(f)[:6]
    tw = Twin(eng, [f.o], [0], len(reads), 100, 1000, mode=OFF)
    try:
        def step(i, lines_now):
            items = [(s, r[40 * i:40 * i + 40], FIRST if i == 0 else 0) for s, r in enumerate(reads)]
            tw.feed(items, ("setting", i), lines=lines_now)
            tw.check(range(len(reads)), ("setting", i))
        step(0, [0])                       # OFF
        tw.rs.set_lists(CURRENT)
        step(1, [0])                       # CURRENT and no table: the plain form, the oracle's results
        eng.set_pass_lists(BUILD)          # the engine's setting does not reach resume
        tw.rs.set_lists(OFF)
        assert plan_lines(tw.rs) == [0]
        eng.locate(*H.pack_reads(reads[:2]), error_rate=R, significance=CONF)  # (builds the table for locate)
        assert eng.plan_pass(0, 300)["list_lines"] == lines and plan_lines(tw.rs) == [0]
        step(2, [0])
        d.list_table_drop()
        eng.set_pass_lists(OFF)
        tw.rs.set_lists(BUILD)
        assert plan_lines(tw.rs) == [0]    # nothing is built by asking
        items = [(s, r[120:160], 0) for s, r in enumerate(reads)]
        tw.feed(items, "BUILD builds", lines=[0])
        assert plan_lines(tw.rs) == [lines]  # ... and the plan then names the table
        tw.check(range(len(reads)), "BUILD")
        step(4, [lines])
        # an unknown mode is refused and changes nothing
        for bad in (-1, 3, 99):
            with pytest.raises(capi.RBError) as err:
                tw.rs.set_lists(bad)
            assert err.value.status == capi.RB_ERR_INVALID_ARG
        assert plan_lines(tw.rs) == [lines]
        # max_chunk_len 65 536: too many k-mers for the 16-bit counters, the plan says 0 and the call takes the plain form
        big = eng.resume(2, 65536, 70000)
        big.set_lists(CURRENT)
        assert plan_lines(big) == [0]
        model = RR.Model(2, 65536, 70000)
        items = [(0, reads[0][:120], FIRST), (1, reads[1][:120], FIRST)]
        RR.assert_same(GR.feed(big, items, MODE, R, CONF), model.feed(items, [f.o], [], MODE, R, CONF), "max_chunk_len 65536")
        GR.check_slots(big, model, [f.o], range(2), "max_chunk_len 65536")
        big.destroy()
        small = eng.resume(2, 65535 - 31 + K - 1, 70000)  # the largest bound the list form serves
        small.set_lists(CURRENT)
        assert plan_lines(small) == [lines]
        small.destroy()
        # a filter whose bits change refuses the set as stale, as without the setting
        d.add_sequence("ACGTACGTACGTAAC", 100, 0)
        with pytest.raises(capi.RBError) as err:
            GR.feed(tw.rs, [(0, "ACGTACGTAA", 0)], MODE, R, CONF)
        assert err.value.status == capi.RB_ERR_INVALID_ARG
    finally:
        tw.close()
        eng.destroy()
        d.free()


# ------------------------------------------------------------------------------------------------ 8. packed reads and d_read_ids
def test_packed_reads_and_read_ids():
    torch = pytest.importorskip("torch")
    d, f, eng = planted(4090, 2)
    reads = RL.schedule_reads(f)[-7:]  # (206 bases and more: every chunk below starts inside its read)
    reads[2] = reads[2][:90] + "N" + reads[2][91:]
    reads[5] = reads[5][:133]  # not a multiple of four bases, and it ends inside the second chunk
    ids = [5, 0, 6, 2, 3]
    tw = Twin(eng, [f.o], [2], 16, 128, 1000)
    try:
        for form, base in (("packed", 0), ("ascii", 8)):
            slots = [base + j for j in range(len(ids))]
            for step, (start, length) in enumerate(((0, 83), (83, 50), (133, 0))):  # (83: a chunk starts inside a byte of the 2-bit source)
                flags = [FIRST if step == 0 else 0] * len(ids)
                chunks = [reads[i][start:start + length] if length else reads[i][start:start + 128] for i in ids]
                items = list(zip(slots, chunks, flags))
                if form == "packed":
                    full = [r[:start + 128] for r in reads]  # (the chunk to the end of the read stays within max_chunk_len)
                    feeder = lambda rs: GR.device_feed(torch, rs, 1, full, slots, flags, chunk_start=start, chunk_length=length, ids=ids, packed=True)
                else:
                    feeder = lambda rs: GR.device_feed(torch, rs, 1, chunks, slots, flags)
                tw.feed(items, (form, step), feeder=feeder)
            tw.check(slots, form)
        for j in range(len(ids)):
            assert tw.rs.counts(j, 0)[0].tobytes() == tw.rs.counts(8 + j, 0)[0].tobytes()
    finally:
        tw.close()
        eng.destroy()
        d.free()

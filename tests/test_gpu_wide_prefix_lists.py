"""The prefix pass from a filter's WIDE list table (rb_engine_set_wide_prefix_lists; rb_wide_prefix_lists.hip,
ibf_prefix_wide_lists_kernel: filters of 8193 to 32 256 bins, one workgroup of four waves per item) against the oracle, bit for bit,
through the C ABI; expected rows come from tests/prefix_rules.py alone.  Every case asserts that Engine.wide_prefix_lines names the
fixture's slot size -- a call that silently ran the plain form would prove nothing -- that Engine.wide_prefix_lists_items equals the
taken / left counts of the rig's model of the take rule (tests/wide_prefix_lists_rig.py, takes()), with at least one item taken, and
that the same call under RB_PASS_LISTS_OFF returns the same bytes for all six outputs.  The fixtures are the k = 7 count fixtures of
tests/wide_lists_rig.py with the rig's reads planted on top; what they claim of themselves is asserted without a GPU in
tests/test_wide_prefix_lists_cpu.py.  No tolerance, no assertion on elapsed time."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import pyoracle as po
from readbouncer_amd import capi
from tests import helpers as H
from tests import list_scan_rig as SR
from tests import prefix_lists_rig as XL
from tests import prefix_rules as PR
from tests import test_gpu_list_scan as LS
from tests import test_gpu_locate as GL
from tests import test_gpu_prefix_lists as GP
from tests import test_gpu_row_table as RT
from tests import test_gpu_wide_lists as WL
from tests import wide_lists_rig as WR
from tests import wide_prefix_lists_rig as WX

K, R, CONF = WX.K, WX.R, WX.CONF
OFF, CURRENT, BUILD = capi.RB_PASS_LISTS_OFF, capi.RB_PASS_LISTS_CURRENT, capi.RB_PASS_LISTS_BUILD
UNBLOCK = capi.RB_MODE_CHECK_UNBLOCK
KEYS = GP.KEYS
same_bytes = GP.same_bytes
REACHED = set()  # (lines, non-temporal) of the wide launches the tests made: the closing test wants all six builds of the kernel


def wide_lines(eng, max_len, c_last, nf=1):
    return [eng.wide_prefix_lines(j, max_len, c_last) for j in range(nf)]


def engine(dep, tgt=(), mode=CURRENT, nt=0):
    eng = capi.Engine(0, list(dep), list(tgt))
    eng.set_nt_threshold(0 if nt else RT.NT_NEVER)
    eng.set_wide_prefix_lists(mode)
    return eng


@functools.lru_cache(maxsize=None)
def expectation(name, which):
    """the oracle's rows for a list of reads of a fixture under its checkpoints, computed once and shared"""
    c = WX.prefix_fixture(name)
    reads, cps = {"seams": (c.seam_reads, WX.SEAM_CHECKPOINTS), "one": (c.seam_reads, WX.ONE_CHECKPOINT), "64": (c.seam_reads, WX.SIXTY_FOUR),
                  "back": (lambda: c.back, WX.BACK_CHECKPOINTS), "moves": (lambda: c.whole + c.tail, WX.MOVE_CHECKPOINTS),
                  "n": (c.n_checkpoint_reads, WX.N_CHECKPOINTS), "crafted": (c.crafted_reads, WX.CRAFT_CHECKPOINTS)}[which]
    reads = reads()
    return reads, cps, PR.expected_batch(reads, cps, [c.o], [], UNBLOCK, r=R, conf=CONF)


def run_both(eng, dep, tgt, reads, cps, lines, label, mode=UNBLOCK, setting=CURRENT, exp=None, ids=None, lists_model=None):
    """Engine.prefixes of `reads` on the wide form (wide_prefix_lines says so: `lines` per filter; the item counters say who was taken)
    against the oracle, then the same call with the setting off: the same bytes -> the expectation.  lists_model: what the LIST form's
    counters must read after each call (an engine with rb_engine_set_prefix_lists on); (0, 0) otherwise"""
    nf = len(dep) + len(tgt)
    buf, offs, lens = H.pack_reads(list(reads))
    max_len = int(lens.max())  # the host form's bound: the longest read of the batch
    items = list(reads) if ids is None else [reads[i] for i in ids]
    if exp is None:
        exp = PR.expected_batch(items, cps, dep, tgt, mode, r=R, conf=CONF)
    rid = None if ids is None else np.array(ids, dtype=np.uint32)
    got = {}
    for s in (setting, OFF):
        eng.set_wide_prefix_lists(s)
        assert wide_lines(eng, max_len, cps[-1], nf) == (list(lines) if s != OFF else [0] * nf), (label, s)
        eng.wide_prefix_lists_items(reset=True)
        eng.prefix_lists_items(reset=True)
        got[s] = eng.prefixes(buf, offs, lens, cps, read_ids=rid, error_rate=R, significance=CONF, mode=mode)
        PR.assert_same(got[s], exp, "%s, setting %d" % (label, s))
        counted = eng.wide_prefix_lists_items()
        if s != OFF and any(lines):
            assert counted == WX.taken_counts(items, cps[-1], max_len=max_len) and counted[0] >= 1, (label, counted)
        else:
            assert counted == (0, 0), (label, s, counted)
        assert eng.prefix_lists_items() == (lists_model or (0, 0)), (label, s)  # the list form's pair is its own
    eng.set_wide_prefix_lists(setting)
    same_bytes(got[setting], got[OFF], label)
    return exp


@pytest.fixture(scope="module", params=list(WR.COUNT_FIXTURES))
def served(request):
    c = WX.prefix_fixture(request.param)
    d = WL.upload(c.o)
    info = d.wide_list_table_build()
    assert info["refused"] == 0 and info["lines"] == c.lines, info
    yield request.param, c, d
    d.free()


# ------------------------------------------------------------------------------------------------ 1. checkpoint seams
@pytest.mark.parametrize("nt", (0, 1))
def test_checkpoint_seams(served, nt):
    """checkpoints one k-mer apart across the seam of a batch of 16 slots, of a tile and of a round of four tiles; ranges that start off
    a multiple of 64, shorter than a tile, and of 2, 4, 5 and 9 tiles; below k, at k, beyond the read; one checkpoint and sixty-four"""
    name, c, d = served
    eng = engine([d], mode=CURRENT, nt=nt)
    for which in ("seams", "one", "64"):
        reads, cps, exp = expectation(name, which)
        run_both(eng, [c.o], [], reads, cps, [c.lines], (name, which, nt), exp=exp)
        if which == "seams":  # the long read counts every k-mer of its prefix in its bin: the maxima rise one by one across the seams
            assert exp["max_count"][0, :len(WX.SEAM_KMERS), 0].tolist() == list(WX.SEAM_KMERS)
            assert exp["max_count"][0, -2:, 0].tolist() == [WX.LONG_KMERS] * 2
    REACHED.add((eng.wide_prefix_lines(0, 400, 400), nt))
    eng.destroy()


# ------------------------------------------------------------------------------------------------ 2. the maximum moves
def test_the_maximum_moves_between_shares_and_strands(served):
    """from a bin in wave 0's share of the scan to one in wave 3's and back, from strand 0 to strand 1; bins 0, 8191, 8192, both halves of
    the last counter dword, the last bin (c8193: the pad half)"""
    name, c, d = served
    eng = engine([d])
    reads, cps, exp = expectation(name, "back")
    run_both(eng, [c.o], [], reads, cps, [c.lines], (name, "back"), exp=exp)
    reads, cps, exp = expectation(name, "moves")
    run_both(eng, [c.o], [], reads, cps, [c.lines], (name, "moves"), exp=exp)
    kmers = [x - K + 1 for x in cps]
    for i in range(len(c.pairs)):  # the whole reverse complement is planted: strand 1 counts every k-mer
        assert exp["max_count"][i, :, 0].tolist() == kmers
    eng.destroy()


# ------------------------------------------------------------------------------------------------ 3. N, flagged and overflow slots
def test_n_flagged_and_overflow_slots(served):
    """the N-carrying sequence and plants with an N at the first, a middle and the last base, checkpoints on either side of the N k-mers
    and inside them; N alone; each crafted k-mer (swapped halves, exactly cap bins, the overflow slot) as the last k-mer of one range and
    the first of the next"""
    name, c, d = served
    eng = engine([d])
    for which in ("n", "crafted"):
        reads, cps, exp = expectation(name, which)
        run_both(eng, [c.o], [], reads, cps, [c.lines], (name, which), exp=exp)
    eng.destroy()


# ------------------------------------------------------------------------------------------------ 4. the counter's end
def test_the_counters_end():
    """one read of 65 535 k-mers with checkpoints at its last two k-mers: bin 5 stands at 0xFFFE, then 0xFFFF; a last checkpoint worth
    65 536 k-mers reports 0 lines and runs the plain form"""
    c = WX.prefix_fixture("c8193")
    d = WL.upload(c.o)
    d.wide_list_table_build()
    eng = engine([d])
    exp = run_both(eng, [c.o], [], [WX.edge_read()], WX.EDGE_CHECKPOINTS, [c.lines], "edge")
    assert exp["max_count"][0, :, 0].tolist() == [0xFFFE, 0xFFFF]
    over = WX.edge_read() + "C"
    assert wide_lines(eng, len(over), WX.OVER_CHECKPOINTS[-1]) == [0]
    assert wide_lines(eng, len(over), WX.EDGE_CHECKPOINTS[-1]) == [c.lines]  # the rule is asked of the last checkpoint, not of the read
    run_both(eng, [c.o], [], [over], WX.OVER_CHECKPOINTS, [0], "edge, one k-mer more")
    run_both(eng, [c.o], [], [over], WX.EDGE_CHECKPOINTS, [c.lines], "edge, a longer read", exp=exp)
    eng.destroy(), d.free()


# ------------------------------------------------------------------------------------------------ 5. items the form leaves
def test_items_the_form_leaves():
    """one batch holds every kind of item (tests/prefix_lists_rig.py, KINDS) through the device form: ASCII and packed with an N bitmap,
    whole and with an odd chunk_start, with read_ids (a permuted subset with repeats), under a bound beyond the last checkpoint and an
    understated one; items shorter than k and empty are taken, a pre-status other than RB_OK is left"""
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda:0")
    c = WX.prefix_fixture("c31000")
    d = WL.upload(c.o)
    d.wide_list_table_build()
    eng = engine([d])
    cps = WX.MIXED_CHECKPOINTS
    seen = set()
    for start in (0, WX.ODD_START):
        reads, kinds = WX.mixed_items(start)
        pad = reads[kinds.index("free_long")][:start]
        reads = reads + [pad + c.long[:300], pad + WX.rc(c.plants[1][0])]  # and two reads the filter holds
        batch = GP.DeviceReads(torch, dev, reads)
        n = len(reads)
        for bound in (WX.WIDE_BOUND, WX.UNDERSTATED):
            eng.set_wide_prefix_lists(CURRENT)
            assert wide_lines(eng, bound, cps[-1]) == [c.lines]
            for ids in (None, [n - 1, 3, 3, 0, 16, 5, 2, 4, 14, n - 2, 6, 8, 10, 12]):
                items = reads if ids is None else [reads[i] for i in ids]
                exp = PR.expected_batch(items, cps, [c.o], [], UNBLOCK, r=R, conf=CONF, chunk_start=start, max_len=bound)
                model = WX.taken_counts(items, cps[-1], chunk_start=start, max_len=bound)
                assert model[0] >= 1 and (model[1] >= 1 or (start == 0 and bound == WX.WIDE_BOUND))
                for packed_form in (False, True):
                    what = ("device", start, bound, ids is not None, packed_form)
                    got = {}
                    for s in (CURRENT, OFF):
                        eng.set_wide_prefix_lists(s)
                        eng.wide_prefix_lists_items(reset=True)
                        got[s] = batch.run(eng, 1, cps, bound, packed_form, start, ids)
                        PR.assert_same(got[s], exp, what + (s,))
                        assert eng.wide_prefix_lists_items() == (model if s == CURRENT else (0, 0)), what + (s,)
                    same_bytes(got[CURRENT], got[OFF], what)
                seen |= set(exp["status"].ravel().tolist())
    assert seen == {capi.RB_OK, capi.RB_ERR_SHORT_READ, capi.RB_ERR_BAD_CHUNK, capi.RB_ERR_INVALID_ARG}
    eng.destroy(), d.free()


# ------------------------------------------------------------------------------------------------ 6. engines of several filters
def test_engines_of_several_filters():
    """one engine with a list-served filter (2112 bins, rb_engine_set_prefix_lists), a wide-served one and a narrow one, as deplete +
    target, in all three modes; each setting alone and both together, both pairs of item counters"""
    c = WX.prefix_fixture("c8193")
    wide = WL.upload(c.o)
    wide.wide_list_table_build()
    d1, f1 = LS.resident(lambda words, info: SR.Planted(2112, 1, words), 2112, SR.N_BLOCKS, 1)
    narrow = po.OracleIBF(200, 3, K, 64 * 4 * 1021)
    planted = H.random_dna(np.random.default_rng(3), 300)
    narrow.insert(po.encode(planted), 77)
    d2 = GL.upload(narrow)
    eng = engine([d1, d2], [wide])
    dep, tgt = [f1.o, narrow], [c.o]
    reads = f1.reads()[-6:] + [c.long[:400], c.back[0], c.whole[1], c.n_seq, planted[20:200], "ACGT", "ACGTNACGTACGTAACCGGTT" * 4, ""]
    cps = (K - 1, K, WX.bases(64), WX.bases(65), 134, 160, 300)
    max_len = max(len(r) for r in reads)
    lists_taken = XL.taken_counts(reads, cps[-1], max_len=max_len)
    assert lists_taken[0] >= 1 and lists_taken[1] >= 1 and WX.taken_counts(reads, cps[-1], max_len=max_len) == (len(reads), 0)
    decisions = set()
    exp = {}
    for mode in (capi.RB_MODE_CHECK_UNBLOCK, capi.RB_MODE_CLASSIFY_CHUNK, capi.RB_MODE_CLASSIFY_ANY):
        # the wide setting alone
        eng.set_prefix_lists(OFF)
        exp[mode] = run_both(eng, dep, tgt, reads, cps, [0, 0, c.lines], ("three filters, wide alone", mode), mode=mode)
        assert GP.plan_lines(eng, max_len, cps[-1], 3) == [0, 0, 0]
        # both together: two prep results in one call, and the narrow filter on the plain form
        eng.set_prefix_lists(CURRENT)
        assert GP.plan_lines(eng, max_len, cps[-1], 3) == [1, 0, 0]
        run_both(eng, dep, tgt, reads, cps, [0, 0, c.lines], ("three filters, both", mode), mode=mode, exp=exp[mode], lists_model=lists_taken)
        decisions |= set(exp[mode]["decision"].ravel().tolist())
    assert {0, 1} <= decisions
    # the list setting alone: the wide form's counters stay untouched
    eng.set_wide_prefix_lists(OFF)
    buf, offs, lens = H.pack_reads(reads)
    eng.wide_prefix_lists_items(reset=True), eng.prefix_lists_items(reset=True)
    assert wide_lines(eng, max_len, cps[-1], 3) == [0, 0, 0]
    PR.assert_same(eng.prefixes(buf, offs, lens, cps, error_rate=R, significance=CONF), exp[UNBLOCK], "list alone")
    assert eng.wide_prefix_lists_items() == (0, 0) and eng.prefix_lists_items() == lists_taken
    eng.destroy()
    for x in (wide, d1, d2):
        x.free()


# ------------------------------------------------------------------------------------------------ 7. the setting
def test_the_setting():
    c = WX.prefix_fixture("c8193")
    d = WL.upload(c.o)
    rng = np.random.default_rng(41)  # (48 random reads of 400 bases: with them the batch alone repays a table of 4^7 slots)
    reads = [c.long[:400], c.back[0], c.n_seq] + [r for r, _ in c.planted_reads()][:6] + [WR.random_dna(rng, 400) for _ in range(48)]
    cps = (K, 71, 134, 180, 400)
    buf, offs, lens = H.pack_reads(reads)
    max_len = int(lens.max())
    exp = PR.expected_batch(reads, cps, [c.o], [], UNBLOCK, r=R, conf=CONF)
    model = WX.taken_counts(reads, cps[-1], max_len=max_len)
    eng = capi.Engine(0, [d], [])

    def prefixes_are(want_lines, expectation, what):
        assert wide_lines(eng, max_len, cps[-1]) == [want_lines], what
        eng.wide_prefix_lists_items(reset=True)
        PR.assert_same(eng.prefixes(buf, offs, lens, cps, error_rate=R, significance=CONF), expectation, what)
        assert eng.wide_prefix_lists_items() == (model if want_lines else (0, 0)), what

    prefixes_are(0, exp, "default: off")
    for bad in (-1, 3):
        with pytest.raises(capi.RBError) as ei:
            eng.set_wide_prefix_lists(bad)
        assert ei.value.status == capi.RB_ERR_INVALID_ARG
    # the other settings do not reach the wide form of the prefix pass
    eng.set_wide_lists(BUILD), eng.set_wide_pass_lists(BUILD), eng.set_prefix_lists(BUILD), eng.set_pass_lists(BUILD)
    prefixes_are(0, exp, "the four other settings alone")
    assert d.wide_list_table_info()["builds"] == 0 and d.list_table_info()["builds"] == 0
    eng.set_wide_lists(OFF), eng.set_wide_pass_lists(OFF), eng.set_prefix_lists(OFF), eng.set_pass_lists(OFF)
    # CURRENT without a table: the plain form, and the call builds none
    eng.set_wide_prefix_lists(CURRENT)
    prefixes_are(0, exp, "current, no table")
    assert d.wide_list_table_info()["builds"] == 0 and d.wide_list_table_info()["bytes"] == 0
    # BUILD: a batch that does not repay the build stays plain; this one builds, 0 -> 1
    eng.set_wide_prefix_lists(BUILD)
    small = H.pack_reads(reads[:2])
    eng.prefixes(*small, cps, error_rate=R, significance=CONF)
    assert d.wide_list_table_info()["builds"] == 0
    assert wide_lines(eng, max_len, cps[-1]) == [0]  # (asking builds nothing)
    PR.assert_same(eng.prefixes(buf, offs, lens, cps, error_rate=R, significance=CONF), exp, "build")
    info = d.wide_list_table_info()
    assert info["builds"] == 1 and info["lines"] == c.lines, info
    prefixes_are(c.lines, exp, "build, the table stands")
    # ... and this setting reaches none of the others: locate, hits and the list form's plan stay where they were
    assert eng.wide_pass_lines(0, max_len) == 0 and eng.plan_prefix(0, max_len, cps[-1])["list_lines"] == 0
    assert eng.plan_pass(0, max_len)["list_lines"] == 0
    eng.set_wide_pass_lists(CURRENT)
    assert eng.wide_pass_lines(0, max_len) == c.lines  # (its own setting does)
    eng.set_wide_pass_lists(OFF)
    # OFF with a table: plain
    eng.set_wide_prefix_lists(OFF)
    prefixes_are(0, exp, "off, table present")
    # an insert drops the table: CURRENT is plain and follows the new bits
    eng.set_wide_prefix_lists(CURRENT)
    prefixes_are(c.lines, exp, "current")
    moved = reads[-1]
    d.insert(moved, [0], [len(moved)], [100])
    after = PR.expected_batch(reads, cps, [RT.oracle_view(d)], [], UNBLOCK, r=R, conf=CONF)
    assert not np.array_equal(after["max_count"], exp["max_count"])
    prefixes_are(0, after, "current, after the insert")
    eng.destroy(), d.free()
    # the dense filter is refused and served plain
    o = WR.table_fixture("dense")
    dense = WL.upload(o)
    eng = engine([dense], mode=BUILD)
    batch = [WR.random_dna(np.random.default_rng(7), 300) for _ in range(64)]
    b = H.pack_reads(batch)
    dcps = (100, 300)
    PR.assert_same(eng.prefixes(*b, dcps, error_rate=R, significance=CONF), PR.expected_batch(batch, dcps, [o], [], UNBLOCK, r=R, conf=CONF), "dense")
    info = dense.wide_list_table_info()
    assert info["refused"] == capi.RB_LIST_REFUSED_DENSITY and info["builds"] == 0 and wide_lines(eng, 300, 300) == [0], info
    assert eng.wide_prefix_lists_items() == (0, 0)
    eng.destroy(), dense.free()


def test_every_slot_size_and_both_twins_were_reached():
    assert REACHED == {(lines, nt) for lines in WR.WIDE_LINES for nt in (0, 1)}, sorted(REACHED)

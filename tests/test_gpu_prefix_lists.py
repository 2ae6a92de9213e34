"""The prefix pass from a filter's list table (rb_engine_set_prefix_lists; rb_prefix_lists.hip, ibf_prefix_lists_kernel) against the
oracle, bit for bit, through the C ABI; expected rows come from tests/prefix_rules.py alone.  Every case asserts that Engine.plan_prefix
names the list form at the fixture's slot size -- a call that silently ran the plain form would prove nothing -- that
Engine.prefix_lists_items equals the taken / left counts of the rig's model of the take rule (tests/prefix_lists_rig.py, takes()), with
at least one item taken, and that the same call under RB_PASS_LISTS_OFF returns the same bytes.  The fixtures are the k = 7 rigs
(tables of 4^7 slots, 1 021 blocks); what the new ones claim of themselves is asserted without a GPU in tests/test_prefix_lists_cpu.py.
No tolerance, no assertion on elapsed time."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import pyoracle as po
from readbouncer_amd import capi
from tests import helpers as H
from tests import list_scan_rig as SR
from tests import pass_lists_edges_rig as ER
from tests import prefix_lists_rig as XL
from tests import prefix_rules as PR
from tests import test_gpu_list_scan as LS
from tests import test_gpu_locate as GL

K, R, CONF = XL.K, XL.R, XL.CONF
OFF, CURRENT, BUILD = capi.RB_PASS_LISTS_OFF, capi.RB_PASS_LISTS_CURRENT, capi.RB_PASS_LISTS_BUILD
NT_DEFAULT = 512 << 20
UNBLOCK = capi.RB_MODE_CHECK_UNBLOCK
KEYS = ("max_count", "decision", "best_target", "status", "prefix_len", "first_decided")


def plan_lines(eng, max_len, c_last, nf=1):
    return [eng.plan_prefix(j, max_len, c_last)["list_lines"] for j in range(nf)]


def same_bytes(a, b, what):
    for key in KEYS:
        assert a[key].tobytes() == b[key].tobytes(), (what, key)


def run_both(eng, dep, tgt, reads, cps, lines, label, mode=UNBLOCK, setting=CURRENT, exp=None, ids=None):
    """Engine.prefixes of `reads` on the list form (the plan says so: `lines` per filter; the item counters say who was taken)
    against the oracle, then the same call with the setting off: the same bytes -> the expectation"""
    nf = len(dep) + len(tgt)
    buf, offs, lens = H.pack_reads(list(reads))
    max_len = int(lens.max())  # the host form's bound: the longest read of the batch
    items = list(reads) if ids is None else [reads[i] for i in ids]
    if exp is None:
        exp = PR.expected_batch(items, cps, dep, tgt, mode, r=R, conf=CONF)
    rid = None if ids is None else np.array(ids, dtype=np.uint32)
    got = {}
    for s in (setting, OFF):
        eng.set_prefix_lists(s)
        assert plan_lines(eng, max_len, cps[-1], nf) == (list(lines) if s != OFF else [0] * nf), (label, s)
        eng.prefix_lists_items(reset=True)
        got[s] = eng.prefixes(buf, offs, lens, cps, read_ids=rid, error_rate=R, significance=CONF, mode=mode)
        PR.assert_same(got[s], exp, "%s, setting %d" % (label, s))
        counted = eng.prefix_lists_items()
        if s != OFF and any(lines):
            assert counted == XL.taken_counts(items, cps[-1], max_len=max_len) and counted[0] >= 1, (label, counted)
        else:
            assert counted == (0, 0), (label, s, counted)
    eng.set_prefix_lists(setting)
    same_bytes(got[setting], got[OFF], label)
    return exp


def lists_engine(dep, tgt=(), mode=CURRENT):
    eng = capi.Engine(0, list(dep), list(tgt))
    eng.set_prefix_lists(mode)
    return eng


# ------------------------------------------------------------------------------------------------ 1. checkpoint seams
@pytest.mark.parametrize("n_bins,lines", SR.GEOMETRIES)
def test_checkpoint_seams(n_bins, lines):
    """checkpoints one k-mer apart across a tile's and a batch's seam, below and at k, beyond the reads, one and sixty-four of them;
    temporal and non-temporal"""
    d, f = LS.resident(lambda words, info: SR.Planted(n_bins, lines, words), n_bins, SR.N_BLOCKS, lines)
    eng = lists_engine([d])
    reads = XL.seam_reads(f)
    for name, cps in (("seams", XL.seam_checkpoints(lines)), ("P = 1", XL.ONE_CHECKPOINT), ("P = 64", XL.SIXTY_FOUR)):
        exp = None
        for nt in (0, 1):
            eng.set_nt_threshold(0 if nt else NT_DEFAULT)
            exp = run_both(eng, [f.o], [], reads, cps, [lines], (name, n_bins, lines, nt), exp=exp)
        if name == "seams":  # a planted read counts every k-mer of its prefix in its bin: the maxima rise one by one across the seams
            rows = exp["max_count"][len(f.bins) - 1, :, 0].tolist()  # the read of 200 k-mers
            kmers = [min(max(0, c - K + 1), 200) for c in cps]
            assert rows == kmers, (rows, kmers)
    eng.destroy()
    d.free()


# ------------------------------------------------------------------------------------------------ 2. strands and bins
@pytest.mark.parametrize("n_bins,lines", ((2112, 1), ER.ODD))
def test_strands_and_bins(n_bins, lines):
    """the maximum moves from strand 0 to strand 1 and from bin A to bin B between checkpoints, A and B at the edges of the counters
    and of a lane's scan pieces; an odd bin count for the pad half"""
    d, f = LS.resident(lambda words, info: XL.Moves(n_bins, lines, words), n_bins, SR.N_BLOCKS, lines)
    eng = lists_engine([d])
    exp = run_both(eng, [f.o], [], f.reads(), XL.MOVE_CHECKPOINTS, [lines], ("moves", n_bins))
    kmers = [c - K + 1 for c in XL.MOVE_CHECKPOINTS]
    for i in range(len(f.pairs)):  # the whole reverse complement is planted: strand 1 counts every k-mer
        assert exp["max_count"][i, :, 0].tolist() == kmers
    eng.destroy()
    d.free()


# ------------------------------------------------------------------------------------------------ 3. the counter edge
def test_counter_edge():
    """one read of 65 535 k-mers with checkpoints at its last two k-mers: a bin set in every block stands at 0xFFFE, then 0xFFFF; a last
    checkpoint worth 65 536 k-mers takes the plain form"""
    n_bins, lines = 2112, 1
    d, f = LS.resident(lambda words, info: ER.Edges(n_bins, lines, words), n_bins, SR.N_BLOCKS, lines)
    eng = lists_engine([d])
    exp = run_both(eng, [f.raw], [], [XL.edge_read()], XL.EDGE_CHECKPOINTS, [lines], "edge")
    assert exp["max_count"][0, :, 0].tolist() == [0xFFFE, 0xFFFF]
    over = ER.over_read()
    assert d.list_table_info()["lines"] == lines and plan_lines(eng, len(over), XL.OVER_CHECKPOINTS[-1]) == [0]
    assert plan_lines(eng, len(over), XL.EDGE_CHECKPOINTS[-1]) == [lines]  # the rule is asked of the last checkpoint, not of the read
    run_both(eng, [f.raw], [], [over], XL.OVER_CHECKPOINTS, [0], "edge, one k-mer more")
    # the long read under the served checkpoints: its first 65 535 k-mers are the item
    run_both(eng, [f.raw], [], [over], XL.EDGE_CHECKPOINTS, [lines], "edge, a longer read", exp=exp)
    eng.destroy()
    d.free()


# ------------------------------------------------------------------------------------------------ 4. who takes which item
def device_buffers(torch, dev, n, P, nf):
    return {"max_count": torch.full((n, P, nf), 77, dtype=torch.int16, device=dev), "decision": torch.full((n, P), 77, dtype=torch.uint8, device=dev),
            "best_target": torch.full((n, P), 77, dtype=torch.int32, device=dev), "status": torch.full((n, P), 77, dtype=torch.uint8, device=dev),
            "prefix_len": torch.full((n, P), 77, dtype=torch.int32, device=dev), "first_decided": torch.full((n,), 77, dtype=torch.int32, device=dev)}


def to_host(o):
    return {"max_count": o["max_count"].cpu().numpy().view(np.uint16), "decision": o["decision"].cpu().numpy(), "best_target": o["best_target"].cpu().numpy(),
            "status": o["status"].cpu().numpy(), "prefix_len": o["prefix_len"].cpu().numpy().view(np.uint32),
            "first_decided": o["first_decided"].cpu().numpy().view(np.uint32)}


class DeviceReads:
    """a batch on the device, as ASCII and as packed 2-bit + N mask"""

    def __init__(self, torch, dev, reads):
        buf, offs, lens = H.pack_reads(list(reads))
        packed, p_offs, nmask, n_offs = capi.pack_reads(buf, offs, lens)
        self.t = {k: torch.from_numpy(np.ascontiguousarray(a)).to(dev) for k, a in (("seq", buf), ("off", offs.view(np.int64)), ("len", lens.view(np.int32)),
                  ("p", packed), ("po", p_offs.view(np.int64)), ("nm", nmask), ("no", n_offs.view(np.int64)))}
        self.torch, self.dev, self.n = torch, dev, len(reads)

    def run(self, eng, nf, cps, max_len, packed_form, start=0, ids=None, mode=UNBLOCK, only=None):
        """-> the outputs as host arrays; only: the one output the caller asks for"""
        torch, t = self.torch, self.t
        m = self.n if ids is None else len(ids)
        o = device_buffers(torch, self.dev, m, len(cps), nf)
        t_ids = None if ids is None else torch.from_numpy(np.array(ids, dtype=np.uint32).view(np.int32)).to(self.dev)
        torch.cuda.synchronize()
        src = dict(d_nmask=t["nm"].data_ptr(), d_nmask_offsets=t["no"].data_ptr()) if packed_form else {}
        seq, off = (t["p"], t["po"]) if packed_form else (t["seq"], t["off"])
        outs = {"d_" + key: o[key].data_ptr() for key in KEYS if only is None or key == only}
        eng.prefixes_device(seq.data_ptr(), off.data_ptr(), t["len"].data_ptr(), m, max_len, cps, chunk_start=start,
                            d_read_ids=None if ids is None else t_ids.data_ptr(), error_rate=R, significance=CONF, mode=mode, **src, **outs)
        torch.cuda.synchronize()
        return to_host(o)


def test_who_takes_which_item():
    """one batch holds every kind of item (tests/prefix_lists_rig.py, KINDS) through the device form: ASCII and packed, whole and with an
    odd chunk_start, with read_ids (a permuted subset with a repeat), under a bound beyond the last checkpoint and an understated one"""
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda:0")
    n_bins, lines = 2112, 1
    d, f = LS.resident(lambda words, info: SR.Planted(n_bins, lines, words), n_bins, SR.N_BLOCKS, lines)
    eng = lists_engine([d])
    cps = XL.MIXED_CHECKPOINTS
    seen = set()
    for start in (0, XL.ODD_START):
        reads, kinds = XL.mixed_items(start)
        pad = reads[kinds.index("free_long")][:start]
        reads = reads + [pad + f.plants[-1], pad + SR.rc(f.plants[-2])]  # and two reads the filter holds, longer than the last checkpoint
        batch = DeviceReads(torch, dev, reads)
        n = len(reads)
        for bound in (XL.WIDE_BOUND, XL.UNDERSTATED):
            eng.set_prefix_lists(CURRENT)
            assert plan_lines(eng, bound, cps[-1]) == [lines]
            for ids in (None, [n - 1, 3, 3, 0, 16, 5, 2, 4, 14, n - 2, 6, 8, 10, 12]):
                items = reads if ids is None else [reads[i] for i in ids]
                exp = PR.expected_batch(items, cps, [f.o], [], UNBLOCK, r=R, conf=CONF, chunk_start=start, max_len=bound)
                model = XL.taken_counts(items, cps[-1], chunk_start=start, max_len=bound)
                assert model[0] >= 1 and model[1] >= 1
                for packed_form in (False, True):
                    what = ("device", start, bound, ids is not None, packed_form)
                    got = {}
                    for s in (CURRENT, OFF):
                        eng.set_prefix_lists(s)
                        eng.prefix_lists_items(reset=True)
                        got[s] = batch.run(eng, 1, cps, bound, packed_form, start, ids)
                        PR.assert_same(got[s], exp, what + (s,))
                        assert eng.prefix_lists_items() == (model if s == CURRENT else (0, 0)), what + (s,)
                    same_bytes(got[CURRENT], got[OFF], what)
                seen |= set(exp["status"].ravel().tolist())
    assert seen == {capi.RB_OK, capi.RB_ERR_SHORT_READ, capi.RB_ERR_BAD_CHUNK, capi.RB_ERR_INVALID_ARG}
    eng.destroy()
    d.free()


# ------------------------------------------------------------------------------------------------ 5. engines of several filters
def test_engines_of_several_filters():
    """two list-served filters of different slot sizes and a narrow one served plain, as deplete + target, in all three modes; and
    first_decided alone, where decision and status live in the engine's workspace"""
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda:0")
    d1, f1 = LS.resident(lambda words, info: SR.Planted(2112, 1, words), 2112, SR.N_BLOCKS, 1)
    d3, f3 = LS.resident(lambda words, info: SR.Planted(4090, 2, words), 4090, SR.N_BLOCKS, 2)
    narrow = po.OracleIBF(200, 3, K, 64 * 4 * 1021)
    rng = np.random.default_rng(3)
    planted = H.random_dna(rng, 300)
    narrow.insert(po.encode(planted), 77)
    d2 = GL.upload(narrow)
    eng = lists_engine([d1, d2], [d3])
    dep, tgt = [f1.o, narrow], [f3.o]
    reads = f1.reads()[-8:] + f3.reads()[-8:] + [planted[20:200], "ACGT", "ACGTNACGTACGTAACCGGTT" * 4, ""]
    cps = (K - 1, K, XL.bases(64), XL.bases(65), 134, 160, 300)
    decisions = set()
    for mode in (capi.RB_MODE_CHECK_UNBLOCK, capi.RB_MODE_CLASSIFY_CHUNK, capi.RB_MODE_CLASSIFY_ANY):
        exp = run_both(eng, dep, tgt, reads, cps, [1, 0, 2], ("three filters", mode), mode=mode)
        decisions |= set(exp["decision"].ravel().tolist())
    assert {0, 1} <= decisions
    exp = PR.expected_batch(reads, cps, dep, tgt, UNBLOCK, r=R, conf=CONF)
    batch = DeviceReads(torch, dev, reads)
    max_len = max(len(r) for r in reads)
    model = XL.taken_counts(reads, cps[-1], max_len=max_len)
    got = {}
    for s in (CURRENT, OFF):
        eng.set_prefix_lists(s)
        eng.prefix_lists_items(reset=True)
        got[s] = batch.run(eng, 3, cps, max_len, True, only="first_decided")["first_decided"]
        assert np.array_equal(got[s], exp["first_decided"]), s
        assert eng.prefix_lists_items() == (model if s == CURRENT else (0, 0))
    assert model[0] >= 1 and got[CURRENT].tobytes() == got[OFF].tobytes() and (exp["first_decided"] < len(cps)).any()
    eng.destroy()
    for d in (d1, d2, d3):
        d.free()


# ------------------------------------------------------------------------------------------------ 6. the setting
def test_the_setting():
    n_bins, lines = 2112, 1
    made = {}

    def edit(w, host):
        made["f"] = SR.Planted(n_bins, lines, host.words())

    d, owner = LS.LT.uploaded(n_bins, SR.N_BLOCKS, K, edit)
    f = made["f"]
    eng = capi.Engine(0, [d], [])
    reads = f.reads()[:10] + ["ACGTNACGTACGTAACCGGTT" * 4]
    cps = (K, 71, 134, 180)
    buf, offs, lens = H.pack_reads(reads)
    max_len = int(lens.max())
    exp = PR.expected_batch(reads, cps, [f.o], [], UNBLOCK, r=R, conf=CONF)
    model = XL.taken_counts(reads, cps[-1], max_len=max_len)

    def prefixes_are(want_lines, expectation, what):
        assert plan_lines(eng, max_len, cps[-1]) == [want_lines], what
        eng.prefix_lists_items(reset=True)
        PR.assert_same(eng.prefixes(buf, offs, lens, cps, error_rate=R, significance=CONF), expectation, what)
        assert eng.prefix_lists_items() == (model if want_lines else (0, 0)), what

    # the default is OFF; a bad mode is refused
    eng.set_row_table(capi.RB_ROW_TABLE_OFF)  # (the classify path builds no table either)
    prefixes_are(0, exp, "default")
    for bad in (-1, 3):
        with pytest.raises(capi.RBError) as ei:
            eng.set_prefix_lists(bad)
        assert ei.value.status == capi.RB_ERR_INVALID_ARG
    # CURRENT without a table: the plain form, and the call builds none
    eng.set_prefix_lists(CURRENT)
    prefixes_are(0, exp, "current, no table")
    assert d.list_table_info()["bytes"] == 0 and d.list_table_info()["builds"] == 0
    # after rb_dibf_list_table_build CURRENT gives the lines
    assert d.list_table_build()["lines"] == lines
    prefixes_are(lines, exp, "current")
    # the two settings do not reach each other's passes
    assert eng.plan_pass(0, max_len)["list_lines"] == 0
    eng.set_prefix_lists(OFF)
    eng.set_pass_lists(CURRENT)
    assert eng.plan_pass(0, max_len)["list_lines"] == lines
    prefixes_are(0, exp, "set_pass_lists alone")
    eng.set_pass_lists(OFF)
    # the bits move on: CURRENT reports 0 and the results follow the new bits; BUILD rebuilds
    eng.set_prefix_lists(CURRENT)
    moved = reads[0]
    d.insert(moved, [0], [len(moved)], [100])
    f.o.insert(po.encode(moved), 100)
    exp2 = PR.expected_batch(reads, cps, [f.o], [], UNBLOCK, r=R, conf=CONF)
    prefixes_are(0, exp2, "current, stale table")
    eng.set_prefix_lists(BUILD)
    builds = d.list_table_info()["builds"]
    assert plan_lines(eng, max_len, cps[-1]) == [0]  # (the question builds nothing)
    PR.assert_same(eng.prefixes(buf, offs, lens, cps, error_rate=R, significance=CONF), exp2, "rebuild")
    assert d.list_table_info()["builds"] == builds + 1
    prefixes_are(lines, exp2, "build")
    eng.destroy()
    d.free()


# ------------------------------------------------------------------------------------------------ 7. the host form
def test_host_form_over_prefilled_outputs():
    """rb_prefix_batch itself, every output pre-filled with 0xA5: each byte is written, and the sub-batch rule is untouched"""
    n_bins, lines = 4090, 4
    d, f = LS.resident(lambda words, info: SR.Planted(n_bins, lines, words), n_bins, SR.N_BLOCKS, lines)
    eng = lists_engine([d])
    reads = XL.seam_reads(f)[::3] + ["ACGT", "", "ACGTNACGTACGTAACCGGTT" * 4]
    cps = XL.seam_checkpoints(lines)
    exp = PR.expected_batch(reads, cps, [f.o], [], UNBLOCK, r=R, conf=CONF)
    buf, offs, lens = H.pack_reads(reads)
    n, P = len(reads), len(cps)
    cp = np.array(cps, dtype=np.uint32)
    model = XL.taken_counts(reads, cps[-1], max_len=int(lens.max()))
    got = {}
    for s in (CURRENT, OFF):
        eng.set_prefix_lists(s)
        assert plan_lines(eng, int(lens.max()), cps[-1]) == [lines if s == CURRENT else 0]
        eng.prefix_lists_items(reset=True)
        res = {"max_count": np.full((n, P, 1), 0xA5A5, np.uint16), "decision": np.full((n, P), 0xA5, np.uint8),
               "best_target": np.full((n, P), 0xA5A5A5A5, np.uint32).view(np.int32), "status": np.full((n, P), 0xA5, np.uint8),
               "prefix_len": np.full((n, P), 0xA5A5A5A5, np.uint32), "first_decided": np.full(n, 0xA5A5A5A5, np.uint32)}
        out = capi.PrefixOut(*[capi._ptr(res[key]) for key in KEYS])
        st = capi.lib().rb_prefix_batch(eng.h, capi._ptr(buf), capi._ptr(offs), capi._ptr(lens), n, None, n, capi._ptr(cp), P, R, CONF, UNBLOCK, C.byref(out))
        assert st == capi.RB_OK
        PR.assert_same(res, exp, ("host form", s))
        assert eng.prefix_lists_items() == (model if s == CURRENT else (0, 0)) and model[0] >= 1 and model[1] >= 1
        got[s] = res
    same_bytes(got[CURRENT], got[OFF], "host form")
    eng.destroy()
    d.free()

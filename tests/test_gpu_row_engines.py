"""The row form of the count kernel (ibf_count_rows_kernel, row_policy, row_table_for) inside engines of SEVERAL filters, where production
runs it: tests/test_gpu_row_table.py has one filter per engine, so there the row kernel never writes with an output stride above 1 or
to maxcount + fi, never runs beside another filter's kernel or on an auxiliary stream, never feeds best_target, and the clauses of
row_policy about fused micro-batches and filters that do not qualify never decide anything.

One rig (tests/row_rig.py, Rig) at k = 7: a deplete filter and four targets -- three that take the row form (two words per lane, one
word per lane, two column slices) and two that never do (narrow; run-time hash count).  Everything goes through the C ABI and is
compared bit for bit with the oracle on the filters' downloaded bits: raw maxima [n, 5], best_target, decision, status.  Which kernel a
filter takes is read from rb_engine_plan and checked against what the call DID (rb_dibf_row_table_info's build counter): plan and
effect must agree wherever a setting moves the row form on or off.  What the rig's reads cover is asserted on the oracle first."""
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from readbouncer_amd import capi
from tests import helpers as H
from tests import row_rig as RR
from tests import test_gpu_row_table as RT

K = RR.K
R = RR.R
MODES = RR.MODES
CHECK_UNBLOCK = capi.RB_MODE_CHECK_UNBLOCK
OFF, AUTO, FORCE = RT.OFF, RT.AUTO, RT.FORCE
ROWS_KERNEL = RT.ROWS_KERNEL
NF = 5
ROWS_ON = [True, True, True, False, False]  # D, T0, T1 take the row form where it applies at all; T2 (narrow) and T3 (h = 4) never
# every row build, reached by a launch that writes with an output stride above 1: (words per lane, counter planes, non-temporal)
REACHED = set()
LENS = {10: (40, 70, 71, 354), 16: (354, 1100)}  # the longest read puts the engine on ten or on sixteen counter planes


class World:
    """the rig, its two batches and the oracle's answers: computed once, shared and left unchanged"""

    def __init__(self, t0_k=K):
        self.rig = RR.Rig(t0_k)
        self.reads, self.batch, self.tie = {}, {}, {}
        for planes, lens in LENS.items():
            self.reads[planes] = self.rig.reads(lens)
            self.tie[planes] = list(self.rig.tie_reads)
            self.batch[planes] = H.pack_reads(self.reads[planes])
        self.views = None
        self._ref = {}

    def filters(self):
        """the five filters, fresh (no row table, build counters at 0); the same bits every time"""
        fs = []
        for _, bins, h, k, seed, plant in self.rig.specs:
            d = capi.DeviceIBF.create(0, bins, h, k, self.rig.n_bits(bins))
            d.fill_synth(seed)
            for seq, b in plant:
                d.insert(seq, [0], [len(seq)], [b])
            fs.append(d)
        views = [RT.oracle_view(d) for d in fs]
        if self.views is None:
            self.views = views
        else:
            assert all(np.array_equal(a.words(), b.words()) for a, b in zip(views, self.views))
        return fs

    def ref(self, planes, n_rule, mode):
        key = (planes, n_rule, mode)
        if key not in self._ref:
            out = RR.oracle_reference(self.views, self.reads[planes], self.batch[planes], n_rule, mode)
            for a in out:
                a.setflags(write=False)
            self._ref[key] = out
        return self._ref[key]

    def covered(self, planes):
        self.rig.tie_reads = self.tie[planes]
        for n_rule in (3, 4):
            RR.rig_covers(self.rig, self.reads[planes], {mode: self.ref(planes, n_rule, mode) for mode in MODES})


@pytest.fixture(scope="module")
def world():
    return World()


def make_engine(fs, mode, nt=0, split=0):
    eng = capi.Engine(0, fs[:1], fs[1:])
    eng.set_split_threshold(split)  # 0: every batch in the throughput form
    eng.set_row_table(mode)
    eng.set_nt_threshold(0 if nt else RT.NT_NEVER)
    return eng


def free_all(engines, fs):
    for e in engines:
        e.destroy()
    for f in fs:
        f.free()


def sub(batch, idx):
    buf, offs, lens = batch
    return buf, np.ascontiguousarray(offs[idx]), np.ascontiguousarray(lens[idx])


def tiled(batch, n):
    """n reads: the batch's reads over and over (same bytes, so the oracle's answers repeat with them)"""
    buf, offs, lens = batch
    reps = -(-n // len(lens))
    return buf, np.ascontiguousarray(np.tile(offs, reps)[:n]), np.ascontiguousarray(np.tile(lens, reps)[:n])


def tiled_ref(ref, n):
    reps = -(-n // len(ref[1]))
    return tuple(np.concatenate([a] * reps)[:n] for a in ref)


def builds(fs):
    return [f.row_table_info()["builds"] for f in fs]


def same(out, ref, label):
    mc, best, dec, st = out
    raw, r_best, r_dec, r_st = ref
    bad = np.nonzero((mc != raw).any(axis=1))[0]
    assert len(bad) == 0, (label, "raw maxima", [(int(i), mc[i].tolist(), raw[i].tolist()) for i in bad[:6]])
    for what, got, want in (("best_target", best, r_best), ("decision", dec, r_dec), ("status", st, r_st)):
        bad = np.nonzero(got != want)[0]
        assert len(bad) == 0, (label, what, [(int(i), int(got[i]), int(want[i]), mc[i].tolist()) for i in bad[:6]])


def equal(a, b, label):
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b)), label


def planned(eng, fs, n_reads, max_len):
    return [eng.plan(fi, n_reads, max_len) for fi in range(len(fs))]


def accounted(eng, fs, batch, mode=CHECK_UNBLOCK, label=None, call=None):
    """one classify call with the plan checked against what the call did: a filter's build counter moves exactly where the plan names the
    row kernel and the filter had no current table; -> (outputs, [the plan names the row kernel] per filter)"""
    buf, offs, lens = batch
    plans = planned(eng, fs, len(lens), int(lens.max()))
    before = [f.row_table_info() for f in fs]
    out = call() if call else eng.classify(buf, offs, lens, error_rate=R, mode=mode)
    rows = []
    for fi, (p, b, f) in enumerate(zip(plans, before, fs)):
        a = f.row_table_info()
        on = p["kernel"] == ROWS_KERNEL
        rows.append(on)
        assert a["builds"] - b["builds"] == int(on and b["bytes"] == 0), (label, fi, p["kernel"], b, a)
        if on:
            assert a["bytes"] == a["want_bytes"] == p["row_table_bytes"] > 0 and a["refused"] == 0, (label, fi, p, a)
            assert p["lanes_per_block_log2"] == 6
            if p["column_slices"] == 1 and len(fs) > 1:  # written to maxcount + fi with a stride of len(fs)
                REACHED.add((p["words_per_lane"], p["counter_planes"], p["nontemporal"]))
        else:
            assert p["row_table_bytes"] == 0 and a["bytes"] == b["bytes"], (label, fi, p, b, a)
    return out, rows


# ---------------------------------------------------------------- parity in all three modes
@pytest.mark.parametrize("nt", (0, 1))
@pytest.mark.parametrize("planes", (10, 16))
def test_parity_in_all_three_modes(world, planes, nt):
    fs = world.filters()
    world.covered(planes)
    batch = world.batch[planes]
    off, force = make_engine(fs, OFF, nt), make_engine(fs, FORCE, nt)
    assert builds(fs) == [0] * NF
    for n_rule in (3, 4):
        off.set_revcomp_of_n(n_rule), force.set_revcomp_of_n(n_rule)
        for mode in MODES:
            ref = world.ref(planes, n_rule, mode)
            label = (planes, nt, n_rule, mode)
            a, rows_a = accounted(off, fs, batch, mode, label + ("off",))
            b, rows_b = accounted(force, fs, batch, mode, label + ("force",))
            assert rows_a == [False] * NF and rows_b == ROWS_ON, (label, rows_a, rows_b)
            same(a, ref, label + ("off",))
            same(b, ref, label + ("force",))
            equal(a, b, label)
    assert builds(fs) == [1, 1, 1, 0, 0]  # one table per qualifying filter, built by the first forced call
    plans = planned(force, fs, len(batch[2]), int(batch[2].max()))
    assert [p["counter_planes"] for p in plans[:3]] == [planes] * 3 and [p["nontemporal"] for p in plans[:3]] == [nt] * 3
    assert [p["words_per_lane"] for p in plans[:3]] == [2, 1, 2] and [p["column_slices"] for p in plans[:3]] == [1, 1, 2]
    free_all((off, force), fs)


# ---------------------------------------------------------------- every filter on an auxiliary stream
@pytest.mark.parametrize("planes", (10, 16))
def test_fan_out(world, planes):
    """with a serial-table limit of 0 every filter counts as large: they fan out over the auxiliary streams behind the fork event, the row
    kernels among them, and the first forced call on fresh filters builds three tables inside one fanned-out call"""
    fs = world.filters()
    batch = world.batch[planes]
    engines = {}
    for serial in (0, None):
        for overlap in (1, 0):
            eng = make_engine(fs, FORCE)
            if serial is not None:
                eng.set_serial_table_bytes(serial)
            eng.set_overlap(overlap)
            engines[(serial, overlap)] = eng
    off = make_engine(fs, OFF)
    off.set_serial_table_bytes(0)
    first = True
    for mode in MODES:
        ref = world.ref(planes, 3, mode)
        outs = []
        for key, eng in engines.items():
            for rep in range(2):
                out, rows = accounted(eng, fs, batch, mode, (planes, mode, key, rep))
                assert rows == ROWS_ON
                if first:
                    assert builds(fs) == [1, 1, 1, 0, 0], "three tables inside the first fanned-out call"
                    first = False
                same(out, ref, (planes, mode, key, rep))
                outs.append(out)
        out, rows = accounted(off, fs, batch, mode, (planes, mode, "off"))
        assert rows == [False] * NF
        for o in outs + [out]:
            equal(o, outs[0], (planes, mode))
    assert builds(fs) == [1, 1, 1, 0, 0]
    free_all(list(engines.values()) + [off], fs)


# ---------------------------------------------------------------- the micro-batch edge
@pytest.mark.parametrize("extra", (0, 1))
def test_micro_batch_edge(world, extra):
    """up to the split threshold the filters of an engine share fused launches, which have no row form; one read more and each filter has a
    launch of its own.  Whatever row_policy says on either side, the call does what rb_engine_plan says"""
    T = 40
    batch, reads = world.batch[10], world.reads[10]
    idx = np.array([i for i in range(len(reads)) if len(reads[i]) >= 70][-(T + extra):])
    assert len(idx) == T + extra
    for mode in MODES:
        fs = world.filters()
        ref = tuple(a[idx] for a in world.ref(10, 3, mode))
        force, off = make_engine(fs, FORCE, split=T), make_engine(fs, OFF, split=T)
        a, rows = accounted(force, fs, sub(batch, idx), mode, ("edge", extra, mode))
        if extra:
            assert rows == ROWS_ON  # (not vacuous: beyond the threshold this is the throughput form of the parity test)
        assert builds(fs) == [int(r) for r in rows]
        b, rows_off = accounted(off, fs, sub(batch, idx), mode, ("edge", extra, mode, "off"))
        assert rows_off == [False] * NF
        same(a, ref, ("edge", extra, mode))
        equal(a, b, ("edge", extra, mode))
        free_all((force, off), fs)


# ---------------------------------------------------------------- settings that move the row form off and on
def test_settings_switch_the_row_form_in_one_engine(world):
    fs = world.filters()
    batch = world.batch[10]
    eng = make_engine(fs, OFF)
    seen = []

    def step(label, want_rows=None):
        for mode in (CHECK_UNBLOCK, capi.RB_MODE_CLASSIFY_CHUNK):
            out, rows = accounted(eng, fs, batch, mode, label)
            same(out, world.ref(10, 3, mode), label)
        dec, st = eng.decide(batch[0], batch[1], batch[2], error_rate=R)  # (the call form the early-decision mode applies to)
        ref = world.ref(10, 3, CHECK_UNBLOCK)
        assert np.array_equal(dec, ref[2]) and np.array_equal(st, ref[3]), label
        if want_rows is not None:
            assert rows == want_rows, (label, rows)
        assert not rows[3] and not rows[4], label  # T2 is too narrow and T3 has a run-time hash count, whatever the mode
        seen.append((label, rows, builds(fs)))

    step("off", [False] * NF)
    assert builds(fs) == [0] * NF
    eng.set_row_table(FORCE)
    eng.set_early_decision(1)
    step("force, early decision", [False] * NF)
    assert builds(fs) == [0] * NF
    eng.set_early_decision(0)
    step("force", ROWS_ON)
    assert builds(fs) == [1, 1, 1, 0, 0]
    eng.set_merge(2)
    step("force, merge 2", ROWS_ON)
    eng.set_early_decision(1)
    step("force, merge 2, early decision", [False] * NF)
    eng.set_early_decision(0)
    eng.set_row_table(AUTO)
    step("auto")
    eng.set_merge(0)
    fs[0].row_table_drop()
    step("auto, merge 0, deplete table dropped")
    eng.set_row_table(OFF)
    step("off again", [False] * NF)
    eng.set_merge(1)
    eng.set_row_table(FORCE)
    fs[2].row_table_drop()
    step("force again", ROWS_ON)
    assert builds(fs)[2] == 2 and builds(fs)[3:] == [0, 0], seen
    free_all((eng,), fs)


# ---------------------------------------------------------------- auto, per filter
def test_auto_mode_decides_per_filter():
    """T0 at k = 5 beside filters at k = 7: a batch between the two thresholds of rule (b) builds the k = 5 table alone"""
    w = World(t0_k=5)
    fs = w.filters()
    L = w.rig.CHUNK
    need5, need7 = RR.rule_b_need(5, 3, L), RR.rule_b_need(K, 3, L)
    assert need5 + 1 < need7 - 1
    rng = np.random.default_rng(55)
    reads = []
    for i in range(need7 + 1):
        name = w.rig.NAMES[i % NF]
        reads.append(H.random_dna(rng, L) if i % 3 == 0 else H.mutate(rng, w.rig.chunk(name, i % 8), 0.05))
    batch = H.pack_reads(reads)
    refs = {mode: RR.oracle_reference(w.views, reads, batch, 3, mode) for mode in (CHECK_UNBLOCK, capi.RB_MODE_CLASSIFY_CHUNK)}
    assert len(set(refs[CHECK_UNBLOCK][2].tolist())) >= 2 and len(set(refs[CHECK_UNBLOCK][1].tolist())) >= 3
    eng = make_engine(fs, AUTO)
    for n, want_rows, want_builds in ((need7 - 1, [False, True, False, False, False], [0, 1, 0, 0, 0]),
                                      (need7, ROWS_ON, [1, 1, 1, 0, 0]), (need7 + 1, ROWS_ON, [1, 1, 1, 0, 0])):
        idx = np.arange(n)
        for mode, ref in refs.items():
            out, rows = accounted(eng, fs, sub(batch, idx), mode, ("auto", n, mode))
            assert rows == want_rows, (n, rows)
            same(out, tuple(a[idx] for a in ref), ("auto", n, mode))
        assert builds(fs) == want_builds, n
    free_all((eng,), fs)


# ---------------------------------------------------------------- the sliced host form
def host_slices(lens, slice_bytes):
    """the consecutive reads rb_classify_batch sends per slice: a slice takes reads while their bases fit slice_bytes, and at least one"""
    out, i0 = [], 0
    while i0 < len(lens):
        i1, total = i0, 0
        while i1 < len(lens) and (i1 == i0 or total + int(lens[i1]) <= slice_bytes):
            total += int(lens[i1])
            i1 += 1
        out.append(i1 - i0)
        i0 = i1
    return out


@pytest.mark.parametrize("mode_rows", (FORCE, AUTO))
def test_sliced_host_form(world, mode_rows):
    """a batch beyond the 8 MiB of the one-copy path crosses in slices; the first slice's call builds the tables while the copy stream
    carries the second, and under auto a short last slice stays on the three-hash kernel: one call, both kernels"""
    slice_bytes = 9 << 19  # 4.5 MiB: two full slices are beyond 8 MiB on their own
    base, ref = world.batch[16], world.ref(16, 3, CHECK_UNBLOCK)
    max_len = int(base[2].max())
    need = RR.rule_b_need(K, 3, max_len)
    last = 5
    assert last < need
    _, _, lens_all = tiled(base, 40000)
    cuts = host_slices(lens_all, slice_bytes)
    n = cuts[0] + cuts[1] + last
    batch = tiled(base, n)
    assert host_slices(batch[2], slice_bytes) == [cuts[0], cuts[1], last] and int(batch[2].sum()) + 16 * n > (8 << 20)
    fs = world.filters()
    eng = make_engine(fs, mode_rows)
    eng.set_host_slice_bytes(slice_bytes)
    full = [p["kernel"] == ROWS_KERNEL for p in planned(eng, fs, cuts[0], max_len)]
    short = [p["kernel"] == ROWS_KERNEL for p in planned(eng, fs, last, max_len)]
    assert full == ROWS_ON and short == (ROWS_ON if mode_rows == FORCE else [False] * NF)
    for rep in range(2):
        out = eng.classify(*batch, error_rate=R)
        same(out, tiled_ref(ref, n), ("sliced", mode_rows, rep))
        assert builds(fs) == [1, 1, 1, 0, 0]
    for p in planned(eng, fs, cuts[0], max_len)[:2]:
        REACHED.add((p["words_per_lane"], p["counter_planes"], p["nontemporal"]))
    free_all((eng,), fs)


# ---------------------------------------------------------------- a change of one filter's bits
def test_an_insert_rebuilds_that_filters_table_only(world):
    fs = world.filters()
    batch, reads = world.batch[10], world.reads[10]
    eng = make_engine(fs, FORCE)
    out, _ = accounted(eng, fs, batch, label="before")
    same(out, world.ref(10, 3, CHECK_UNBLOCK), "before")
    i = next(i for i, r in enumerate(reads) if len(r) == 354)  # read_shapes' random read of that length
    before = world.ref(10, 3, CHECK_UNBLOCK)[0][i, 1]
    fs[1].insert(reads[i], [0], [len(reads[i])], [1234])
    assert fs[1].row_table_info()["bytes"] == 0 and fs[0].row_table_info()["bytes"] > 0 and fs[2].row_table_info()["bytes"] > 0
    views = list(world.views)
    views[1] = RT.oracle_view(fs[1])
    for mode in MODES:
        after = RR.oracle_reference(views, reads, batch, 3, mode)
        assert after[0][i, 1] == 354 - K + 1 > before and after[1][i] == 0  # the read is T0's now
        out, rows = accounted(eng, fs, batch, mode, ("after", mode))
        assert rows == ROWS_ON
        same(out, after, ("after the insert", mode))
        assert builds(fs) == [1, 2, 1, 0, 0]
    free_all((eng,), fs)


# ---------------------------------------------------------------- two engines, two host threads
def test_two_engines_build_one_table_per_filter(world):
    fs = world.filters()
    batch = world.batch[10]
    engines = [make_engine(fs, FORCE), make_engine(fs, FORCE)]
    gate = threading.Barrier(2)
    outs, errors = [None, None], []

    def work(i):
        try:
            gate.wait()
            outs[i] = engines[i].classify(*batch, error_rate=R)  # (ctypes releases the interpreter lock for the call)
        except Exception as exc:  # noqa: BLE001
            errors.append((i, repr(exc)))

    threads = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    ref = world.ref(10, 3, CHECK_UNBLOCK)
    for i in range(2):
        same(outs[i], ref, ("thread", i))
    assert builds(fs) == [1, 1, 1, 0, 0]  # the build looks again under the filter's lock: the second engine takes the first one's table
    free_all(engines, fs)


# ---------------------------------------------------------------- the device form
def test_device_form_packed_chunks_ids_and_best_target(world):
    torch = pytest.importorskip("torch")
    fs = world.filters()
    reads = world.reads[10]
    buf, offs, lens = world.batch[10]
    packed, p_offs, nmask, n_offs = capi.pack_reads(buf, offs, lens)
    dev = torch.device("cuda:0")
    t = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (packed, p_offs.view(np.int64), lens.view(np.int32), nmask, n_offs.view(np.int64))]
    ids = np.array([i for i in range(len(reads)) if i % 3 != 1][::-1], dtype=np.uint32)
    t_ids = torch.from_numpy(ids.view(np.int32)).to(dev)
    start, length = 33, 150
    items = [reads[i][start:start + length] for i in ids]
    keep = [i for i, r in enumerate(items) if len(reads[ids[i]]) > start]  # (a chunk beyond the read's end has a status of its own)
    assert len(keep) >= len(items) - 12 and max(len(x) for x in items) == length
    outs = {}
    for mode in MODES:
        ref = RR.oracle_reference(world.views, items, H.pack_reads(items), 3, mode)
        for rows_mode in (OFF, FORCE):
            eng = make_engine(fs, rows_mode)
            t_max = torch.zeros((len(ids), NF), dtype=torch.int16, device=dev)
            t_best = torch.full((len(ids),), -9, dtype=torch.int32, device=dev)
            t_dec = torch.zeros(len(ids), dtype=torch.uint8, device=dev)
            t_st = torch.zeros(len(ids), dtype=torch.uint8, device=dev)
            torch.cuda.synchronize()

            def call():
                eng.classify_device_ex(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), len(ids), int(lens.max()), t[3].data_ptr(), t[4].data_ptr(),
                                       chunk_start=start, chunk_length=length, d_read_ids=t_ids.data_ptr(), error_rate=R, mode=mode,
                                       d_maxcount=t_max.data_ptr(), d_best=t_best.data_ptr(), d_decision=t_dec.data_ptr(), d_status=t_st.data_ptr())
                torch.cuda.synchronize()

            sized = (None, None, np.full(len(ids), lens.max(), dtype=np.uint32))  # (the plan of this call: its items and its max_len)
            _, rows = accounted(eng, fs, sized, mode, ("device", mode, rows_mode), call=call)
            assert rows == (ROWS_ON if rows_mode == FORCE else [False] * NF)
            outs[rows_mode] = (t_max.cpu().numpy().view(np.uint16), t_best.cpu().numpy(), t_dec.cpu().numpy(), t_st.cpu().numpy())
            eng.destroy()
        equal(outs[OFF], outs[FORCE], ("device", mode))
        same(tuple(a[keep] for a in outs[FORCE]), tuple(a[keep] for a in ref), ("device", mode))
    assert builds(fs) == [1, 1, 1, 0, 0]
    free_all((), fs)


# ---------------------------------------------------------------- the pool
def test_pool_workers_above_rule_b(world):
    """three workers on device 0 (the one-GPU stand-in of tests/test_gpu_parity.py), each with a slice beyond the engine's split threshold
    and far above rule (b) at k = 7: their engines are in the default auto mode"""
    fs = world.filters()
    n = 3 * 2200
    batch = tiled(world.batch[10], n)
    assert n // 3 > 2048 and n // 3 > RR.rule_b_need(K, 3, int(batch[2].max()))
    pool = capi.Pool.from_device([0, 0, 0], fs[:1], fs[1:])
    try:
        assert pool.size() == 3
        pool.set_min_split(2100)
        for mode in MODES:
            out = pool.classify(*batch, error_rate=R, mode=mode)
            same(out, tiled_ref(world.ref(10, 3, mode), n), ("pool", mode))
    finally:
        pool.destroy()
    free_all((), fs)


# ---------------------------------------------------------------- closing
def test_every_row_build_was_reached_behind_a_stride_above_one():
    assert REACHED == RT.ROW_BUILDS, sorted(RT.ROW_BUILDS - REACHED)

"""The resume pass (rb_resume_create / rb_resume_batch / rb_resume_batch_device / rb_resume_counts) against the oracle, through the C
ABI, bit for bit: a read's counts stay in HBM between chunks and a feed counts the new k-mers only.

Expectations come from tests/resume_rules.py: the row of a feed is the oracle's answer for the concatenation of everything the slot
was fed, the slot's counters are seqan::count of that concatenation on both strands.  Filters, the sequence S and the planted bins of
the per-build and wrap cases are those of tests/pass_edges.py, read-only.  No tolerance, no assertion on elapsed time."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import pyoracle as po
from readbouncer_amd import capi
from tests import helpers as H
from tests import pass_edges as PE
from tests import resume_rules as RR
from tests.test_gpu_hits import upload

R, CONF = PE.R, PE.CONF
MODES = (capi.RB_MODE_CHECK_UNBLOCK, capi.RB_MODE_CLASSIFY_CHUNK, capi.RB_MODE_CLASSIFY_ANY)
FIRST, PEEK = capi.RB_RESUME_FIRST, capi.RB_RESUME_PEEK
NAMES = sorted(PE.ALL)
GEOMS = ((0, 1), (1, 1), (2, 1), (3, 1), (4, 1), (5, 1), (6, 1), (6, 2))
EXPECTED_CLASSES = {(lg, wpl, h) for lg, wpl in GEOMS for h in (3, 0)}
META_BYTES = 40  # total length, tail length, 32 bytes of tail
_reached = {}    # geometry name -> (lg, wpl, h) its feeds ran on and matched the oracle


def feed(rs, items, mode=capi.RB_MODE_CHECK_UNBLOCK, r=R, conf=CONF):
    """items: [(slot, chunk, flags)] through the host form"""
    buf, offs, lens = H.pack_reads([c for _, c, _ in items])
    return rs.feed(buf, offs, lens, np.array([s for s, _, _ in items], dtype=np.uint32), np.array([f for _, _, f in items], dtype=np.uint8),
                   error_rate=r, significance=conf, mode=mode)


def check_slots(rs, model, filters, slots, what):
    for s in slots:
        for fi, f in enumerate(filters):
            got, total = rs.counts(s, fi)
            RR.assert_counts(got, model.counts(s, f), "%s slot %d filter %d" % (what, s, fi))
            assert total == model.total(s), (what, s, total, model.total(s))


def pad_cols(n_bins):
    """plain_geometry (rb_engine.hip): blocks of up to 64 words on 2^lg lanes, wider ones in slices of 128 words"""
    W = (n_bins + 63) // 64
    if W > 64:
        return (W + 127) // 128 * 128
    p = 1
    while p < W:
        p *= 2
    return p


def slot_bytes(filters):
    return sum(2 * 16 * 8 * pad_cols(f.n_bins) for f in filters) + META_BYTES


def schedule(k):
    """the chunk lengths of the per-build case: around k, an empty chunk, the reference's 360, then single feeds whose stitched items hold
    511, 512, 513, 1023 and 1024 k-mers (the macro-tile boundaries of LG 0 and the ten-plane edge that must not exist here)"""
    return (k - 1, 1, 1, 0, 5, 360, 3, k - 2, 511, 512, 513, 1023, 1024)


COUNT_CHECKS = (0, 4, 5, 12)  # the feeds to k - 1, 5, 360 and the last one


# ------------------------------------------------------------------------------------------------------------ every build
@pytest.mark.parametrize("name", NAMES)
def test_every_build_follows_the_oracle_feed_by_feed(name):
    f = PE.make_filter(name)
    k = f.kmer_size
    S = PE.sequence()
    sched = schedule(k)
    total = sum(sched)
    reads = [S[:total], S[5000:5000 + total], PE.revcomp_str(S[10000:10000 + total]), PE.with_n(S[20000:20000 + total], 7), S[30011:30011 + total],
             S[40000:40000 + k - 1]]
    dev = upload(f)
    eng = capi.Engine(0, [dev], [])
    try:
        p = eng.plan_pass(0, total)
        rs = eng.resume(6, 1024, total)
        assert rs.bytes == 6 * slot_bytes([f])
        model = RR.Model(6, 1024, total)
        pos = [0] * 6
        for step, c in enumerate(sched):
            items = []
            for s in range(6):
                chunk = reads[s][pos[s]:pos[s] + c]  # (the short read runs out after its first chunk: empty chunks from then on)
                pos[s] += len(chunk)
                items.append((s, chunk, FIRST if step == 0 else 0))
            got = feed(rs, items)
            exp = model.feed(items, [f], [], capi.RB_MODE_CHECK_UNBLOCK, R, CONF)
            RR.assert_same(got, exp, "%s feed %d (%d bases)" % (name, step, c))
            assert int(exp["status"][5]) == capi.RB_ERR_SHORT_READ and int(exp["total_len"][5]) == k - 1
            if step in COUNT_CHECKS:
                check_slots(rs, model, [f], range(6), "%s feed %d" % (name, step))
        assert model.total(0) == total and int(got["max_count"][0, 0]) == total - k + 1  # SAT counts every k-mer
        rs.destroy()
        # the non-temporal twin (blocks of a whole wave): a fresh set, two feeds
        if p["lanes_per_block_log2"] == 6:
            eng.set_nt_threshold(0)
            assert eng.plan_pass(0, total)["nontemporal"] == 1
            rs = eng.resume(6, 1024, total)
            model = RR.Model(6, 1024, total)
            for step, c in enumerate((360, 513)):
                items = [(s, reads[s][360 * step:360 * step + c], FIRST if step == 0 else 0) for s in range(5)]
                RR.assert_same(feed(rs, items), model.feed(items, [f], [], capi.RB_MODE_CHECK_UNBLOCK, R, CONF), "%s nt feed %d" % (name, step))
            check_slots(rs, model, [f], range(5), name + " nt")
            rs.destroy()
        _reached[name] = (p["lanes_per_block_log2"], p["words_per_lane"], p["hash_functions"])
    finally:
        eng.destroy()
        dev.free()


def test_the_geometries_reach_every_class_the_pass_dispatches():
    """every (LG, WPL, h) class of the launcher was taken by a geometry above; where this test runs without them, by the plan of a small
    filter of the same block shape and hash count"""
    classes = dict(_reached)
    for name in NAMES:
        if name in classes:
            continue
        n_bins, _, h, k = PE.ALL[name]
        dev = capi.DeviceIBF.create(0, n_bins, h, k, 64 * ((n_bins + 63) // 64) * 1021)
        eng = capi.Engine(0, [dev], [])
        p = eng.plan_pass(0, 4000)
        classes[name] = (p["lanes_per_block_log2"], p["words_per_lane"], p["hash_functions"])
        eng.destroy()
        dev.free()
    assert set(classes.values()) == EXPECTED_CLASSES, sorted(classes.items())


# --------------------------------------------------------------------------------------------------------------- the wrap
WRAP_TOTALS = (65535, 65536, 65537, 70000)  # k-mers


@pytest.mark.parametrize("name", ["lg0", "lg6", "w129", "w129_h4"])
def test_counters_wrap_as_the_reference_uint16_counts_do(name):
    f = PE.make_filter(name)
    k = f.kmer_size
    S = PE.sequence()
    bins = PE.bins_of(name)
    ends = [n + k - 1 for n in WRAP_TOTALS]
    jobs = [("row", e) for e in ends] + [("counts", e) for e in ends]
    exp = dict(zip(jobs, PE._map(lambda j: RR.expected_row(S[:j[1]], [f], [], capi.RB_MODE_CHECK_UNBLOCK, R, CONF, 70100) if j[0] == "row"
                                 else RR.expected_counts(S[:j[1]], f), jobs)))
    dev = upload(f)
    eng = capi.Engine(0, [dev], [])
    try:
        rs = eng.resume(2, 8192, 70100)
        pos, first = 0, True
        for e, sat in zip(ends, (65535, 0, 1, 4464)):
            while pos < e:
                c = min(8192, e - pos)
                got = feed(rs, [(1, S[pos:pos + c], FIRST if first else 0)])
                pos, first = pos + c, False
                assert int(got["status"][0]) == capi.RB_OK and int(got["total_len"][0]) == pos
            row = exp[("row", e)]
            RR.assert_same(got, {key: np.stack([row[key]]) for key in RR.KEYS + ("ok",)}, "%s at %d k-mers" % (name, e - k + 1))
            counts, total = rs.counts(1, 0)
            RR.assert_counts(counts, exp[("counts", e)], "%s at %d k-mers" % (name, e - k + 1))
            assert total == e and counts[:, bins["SAT"]].tolist() == [sat, sat]
            assert int(counts[1, bins["REV"]]) > int(counts[0, bins["REV"]]) + 10000
    finally:
        eng.destroy()
        dev.free()


# ------------------------------------------------------------------------------------- small engines for the other cases
def small_filter(n_bins, seed, n_blocks=4099, h=3, k=13):
    """an oracle filter with stretches of S in a few bins, forward and reverse complement"""
    W = (n_bins + 63) // 64
    f = po.OracleIBF(n_bins, h, k, 64 * W * n_blocks)
    S = PE.sequence()
    rng = np.random.default_rng(seed)
    for b in sorted(set(int(x) for x in rng.integers(0, n_bins, size=6)) | {n_bins - 1}):
        lo = int(rng.integers(0, 3000))
        seg = S[lo:lo + 900]
        f.insert(po.encode(PE.revcomp_str(seg) if b % 2 else seg), b)
    return f


class Rig:
    """deplete (two words) and two targets of different widths (LG 0 and LG 3) behind one engine: two builds per call, best_target"""

    def __init__(self, n_slots=8, max_chunk_len=400, max_total_len=1500):
        self.dep, self.tgt = [small_filter(100, 1)], [small_filter(56, 2), small_filter(300, 3)]
        self.filters = self.dep + self.tgt
        self.devs = [upload(f) for f in self.filters]
        self.eng = capi.Engine(0, self.devs[:1], self.devs[1:])
        self.rs = self.eng.resume(n_slots, max_chunk_len, max_total_len)
        self.model = RR.Model(n_slots, max_chunk_len, max_total_len)

    def feed(self, items, mode=capi.RB_MODE_CHECK_UNBLOCK, r=R, conf=CONF, what=""):
        got = feed(self.rs, items, mode, r, conf)
        RR.assert_same(got, self.model.feed(items, self.dep, self.tgt, mode, r, conf), what)
        return got

    def check(self, slots, what):
        check_slots(self.rs, self.model, self.filters, slots, what)

    def close(self):
        self.rs.destroy()
        self.eng.destroy()
        for d in self.devs:
            d.free()


def reads_of_s(n, length, seed):
    """n reads: cut from S with 3 % substitutions, every third one random"""
    rng = np.random.default_rng(seed)
    S = PE.sequence()
    out = []
    for i in range(n):
        lo = int(rng.integers(0, 3500))
        out.append(H.random_dna(rng, length) if i % 3 == 2 else H.mutate(rng, S[lo:lo + length], 0.03))
    return out


# ------------------------------------------------------------------------------------------------------------------ flags
def test_first_restarts_a_slot_and_peek_leaves_it_alone():
    rig = Rig()
    try:
        a, b = reads_of_s(2, 900, 11)
        rig.feed([(0, a[:300], FIRST), (1, b[:300], FIRST)], what="first chunks")
        rig.feed([(0, a[300:600], 0), (1, b[300:500], 0)], what="without FIRST a slot continues")
        assert rig.model.total(0) == 600 and rig.model.total(1) == 500
        # PEEK: the row of the appended chunk, the slot exactly as it was
        before = [rig.rs.counts(0, fi) for fi in range(3)]
        peek = rig.feed([(0, a[600:900], PEEK), (1, b[500:520], PEEK | FIRST)], what="peek")
        assert peek["total_len"].tolist() == [900, 20]
        rig.check([0, 1], "after a peek")
        after = [rig.rs.counts(0, fi) for fi in range(3)]
        assert all(np.array_equal(x[0], y[0]) and x[1] == y[1] == 600 for x, y in zip(before, after))
        fed = rig.feed([(0, a[600:900], 0)], what="the peeked chunk, fed")
        assert all(np.array_equal(peek[key][0], fed[key][0]) for key in RR.KEYS)
        rig.check([0, 1], "after the feed")
        # FIRST: a fresh read, whatever the slot held
        fresh = rig.feed([(0, b[:350], FIRST), (5, b[:350], FIRST)], what="FIRST on a used and on an unused slot")
        assert all(np.array_equal(fresh[key][0], fresh[key][1]) for key in RR.KEYS) and fresh["total_len"].tolist() == [350, 350]
        rig.check([0, 5], "after FIRST")
        # a slot that was never fed continues from an empty read
        rig.feed([(6, a[:200], 0)], what="a slot never given FIRST")
        rig.check([6], "never given FIRST")
    finally:
        rig.close()


# -------------------------------------------------------------------------------------------------------- the host form
def test_host_form_refuses_a_slot_named_twice():
    rig = Rig()
    try:
        a, b = reads_of_s(2, 300, 12)
        rig.feed([(2, a[:100], FIRST), (3, b[:100], FIRST)], what="before")
        with pytest.raises(capi.RBError) as ei:
            feed(rig.rs, [(2, a[100:200], 0), (3, b[100:200], 0), (2, a[200:300], 0)])
        assert ei.value.status == capi.RB_ERR_INVALID_ARG and "named twice" in capi.lib().rb_last_error().decode()
        rig.check([2, 3], "after the refused call")
        rig.feed([(2, a[100:200], 0), (3, b[100:200], 0)], what="after")
    finally:
        rig.close()


# ------------------------------------------------------------------------------------------------------ modes and engines
def test_modes_engines_settings_and_calls_in_between():
    rig = Rig(n_slots=12)
    try:
        reads = reads_of_s(12, 1100, 13)
        other = H.pack_reads(reads_of_s(40, 300, 14))
        classified = rig.eng.classify(*other, error_rate=R, significance=CONF)
        cuts = (0, 150, 151, 500, 860, 1100)
        rows = []
        for step in range(len(cuts) - 1):
            if step == 2:  # settings that pick other count kernels for rb_classify_batch: the pass does not see them
                rig.eng.set_bound_pruning(True)
                rig.eng.set_early_decision(True)
                rig.eng.set_merge(2)
                rig.eng.set_row_table(capi.RB_ROW_TABLE_FORCE)
            if step == 3:
                rig.eng.set_bound_pruning(False)
            mode = MODES[step % 3]
            items = [(s, reads[s][cuts[step]:cuts[step + 1]], FIRST if step == 0 else 0) for s in range(12)]
            # another error rate on the way: the state holds counts, not decisions
            got = rig.feed(items, mode=mode, r=0.15 if step == 3 else R, what="step %d mode %d" % (step, mode))
            rows.append(got)
            again = rig.eng.classify(*other, error_rate=R, significance=CONF)  # unrelated reads between two feeds
            assert all(x.tobytes() == y.tobytes() for x, y in zip(classified, again)), step
            for m in MODES:  # every mode on the same state, without committing
                rig.feed([(s, "", PEEK) for s in range(12)], mode=m, what="step %d, empty peek in mode %d" % (step, m))
        rig.check(range(12), "at the end")
        last = rows[-1]
        assert (last["best_target"] >= 0).any() and (last["best_target"] == -1).any()
        assert (last["max_count"][:, 0] > 200).any() and (last["max_count"][:, 2] > 200).any()
    finally:
        rig.close()


# ------------------------------------------------------------------------------------------------------------ device form
def device_feed(torch, rs, nf, reads, slots, flags=None, chunk_start=0, chunk_length=0, ids=None, packed=False,
                mode=capi.RB_MODE_CHECK_UNBLOCK):
    dev = torch.device("cuda:0")
    buf, offs, lens = H.pack_reads(list(reads))
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    n = len(slots)
    kw = {}
    if packed:
        pk, p_offs, nmask, n_offs = capi.pack_reads(buf, offs, lens)
        t_seq, t_off, t_nm, t_no = up(pk), up(p_offs.view(np.int64)), up(nmask), up(n_offs.view(np.int64))
        kw = {"d_nmask": t_nm.data_ptr(), "d_nmask_offsets": t_no.data_ptr()}
    else:
        t_seq, t_off = up(buf), up(offs.view(np.int64))
    t_len = up(lens.view(np.int32))
    t_slots = up(np.asarray(slots, dtype=np.uint32).view(np.int32))
    t_flags = None if flags is None else up(np.asarray(flags, dtype=np.uint8))
    t_ids = None if ids is None else up(np.asarray(ids, dtype=np.uint32).view(np.int32))
    o = {"max_count": torch.full((n, nf), 77, dtype=torch.int16, device=dev), "decision": torch.full((n,), 77, dtype=torch.uint8, device=dev),
         "best_target": torch.full((n,), 77, dtype=torch.int32, device=dev), "status": torch.full((n,), 77, dtype=torch.uint8, device=dev),
         "total_len": torch.full((n,), 77, dtype=torch.int32, device=dev)}
    torch.cuda.synchronize()
    rs.feed_device(t_seq.data_ptr(), t_off.data_ptr(), t_len.data_ptr(), n, t_slots.data_ptr(), None if t_flags is None else t_flags.data_ptr(),
                   chunk_start=chunk_start, chunk_length=chunk_length, d_read_ids=None if t_ids is None else t_ids.data_ptr(),
                   error_rate=R, significance=CONF, mode=mode, d_max_count=o["max_count"].data_ptr(), d_decision=o["decision"].data_ptr(),
                   d_best_target=o["best_target"].data_ptr(), d_status=o["status"].data_ptr(), d_total_len=o["total_len"].data_ptr(), **kw)
    return {"max_count": o["max_count"].cpu().numpy().view(np.uint16), "decision": o["decision"].cpu().numpy(),
            "best_target": o["best_target"].cpu().numpy(), "status": o["status"].cpu().numpy(),
            "total_len": o["total_len"].cpu().numpy().view(np.uint32)}


def test_items_are_refused_one_by_one_and_leave_their_slots_alone():
    torch = pytest.importorskip("torch")
    rig = Rig(n_slots=5, max_chunk_len=400, max_total_len=1000)
    try:
        r = reads_of_s(5, 1100, 15)
        rig.feed([(0, r[0][:300], FIRST), (1, r[1][:300], FIRST), (2, r[2][:400], FIRST), (3, r[3][:300], FIRST)], what="before")
        rig.feed([(2, r[2][400:700], 0)], what="slot 2 to 700 bases")
        start = 10
        # every item's chunk is its read from base 10 on
        reads = ["N" * start + r[0][300:500], "N" * start + r[1][300:400], "N" * start + r[1][400:500], "N" * start + r[1][300:701],
                 "N" * start + r[2][700:1001], "ACGTA", "N" * start + r[4][:350], ""]
        assert len(reads[3]) - start == 401 and 700 + len(reads[4]) - start == 1001 > 1000
        slots = [0, 5, 2 ** 32 - 1, 1, 2, 3, 4, 4]
        flags = [0, 0, 0, 0, 0, 0, FIRST, 0]
        ids = [0, 1, 2, 3, 4, 5, 6]
        got = device_feed(torch, rig.rs, 3, reads, slots[:7], flags[:7], chunk_start=start, ids=ids)
        items = [(s, rd[start:], fl) for s, rd, fl in zip(slots[:7], reads[:7], flags[:7])]
        exp = rig.model.feed(items, rig.dep, rig.tgt, capi.RB_MODE_CHECK_UNBLOCK, R, CONF, bad_chunk=(5,))
        INV, BAD = capi.RB_ERR_INVALID_ARG, capi.RB_ERR_BAD_CHUNK
        assert exp["status"].tolist() == [0, INV, INV, INV, INV, BAD, 0]
        RR.assert_same(got, exp, "refusals")
        assert got["total_len"].tolist() == [500, 0, 0, 0, 0, 0, 350]
        assert [rig.model.total(s) for s in range(5)] == [500, 300, 700, 300, 350]
        rig.check(range(5), "after the refusals")
        # the slots go on as if nothing had happened; a chunk that fills the slot to the base is taken
        rig.feed([(1, r[1][300:700], 0), (2, r[2][700:1000], 0), (3, r[3][300:310], 0)], what="afterwards")
        rig.check([1, 2, 3], "afterwards")
    finally:
        rig.close()


def test_packed_reads_and_read_ids_give_the_rows_of_the_ascii_identity_form():
    torch = pytest.importorskip("torch")
    rig = Rig(n_slots=16, max_chunk_len=400, max_total_len=1500)
    try:
        reads = reads_of_s(7, 700, 16)
        reads[2] = PE.with_n(reads[2], 3)
        reads[5] = reads[5][:333]  # not a multiple of four bases, and it ends inside the second chunk
        ids = [5, 0, 6, 2, 3]
        got = {}
        for form, base in (("packed", 0), ("ascii", 8)):
            slots = [base + j for j in range(len(ids))]
            rows = []
            for step, (start, length) in enumerate(((0, 203), (203, 130), (333, 0))):  # (203: a chunk starts inside a byte of the 2-bit source)
                flags = [FIRST if step == 0 else 0] * len(ids)
                if form == "packed":
                    rows.append(device_feed(torch, rig.rs, 3, reads, slots, flags, chunk_start=start, chunk_length=length, ids=ids, packed=True))
                else:
                    chunks = [reads[i][start:start + length] if length else reads[i][start:] for i in ids]
                    rows.append(device_feed(torch, rig.rs, 3, chunks, slots, flags))
                items = [(s, reads[i][start:start + length] if length else reads[i][start:], fl) for s, i, fl in zip(slots, ids, flags)]
                RR.assert_same(rows[-1], rig.model.feed(items, rig.dep, rig.tgt, capi.RB_MODE_CHECK_UNBLOCK, R, CONF), "%s step %d" % (form, step))
            got[form] = rows
            rig.check(slots, form)
        for a, b in zip(got["packed"], got["ascii"]):
            assert all(a[key].tobytes() == b[key].tobytes() for key in RR.KEYS)
        assert got["packed"][2]["total_len"].tolist() == [333, 700, 700, 700, 700]
    finally:
        rig.close()


# ------------------------------------------------------------------------------------------------------------------ order
def test_item_order_and_call_boundaries_do_not_matter():
    rig = Rig(n_slots=16)
    try:
        reads = reads_of_s(8, 700, 17)
        first = [(s, reads[s][:350], FIRST) for s in range(8)]
        second = [(s, reads[s][350:], 0) for s in range(8)]
        rig.feed(first, what="in order")
        rig.feed(second, what="in order")
        # the same pairs on slots 8 to 15: reversed, and split over two calls
        move = lambda items: [(s + 8, c, fl) for s, c, fl in items]
        rig.feed(move(first)[::-1][:3], what="reversed, part 1")
        rig.feed(move(first)[::-1][3:], what="reversed, part 2")
        rig.feed(move(second)[::-1][:5], what="reversed, part 1")
        rig.feed(move(second)[::-1][5:], what="reversed, part 2")
        for s in range(8):
            for fi in range(3):
                a, b = rig.rs.counts(s, fi), rig.rs.counts(s + 8, fi)
                assert np.array_equal(a[0], b[0]) and a[1] == b[1] == 700
        rig.check(range(16), "both halves")
    finally:
        rig.close()


# ------------------------------------------------------------------------------------------------------------------ bytes
def test_bytes_follow_the_formula_of_the_design_document():
    for shapes in ((56,), (100, 300), (8200, 4090, 243)):
        devs = [capi.DeviceIBF.create(0, n, 3, 13, 64 * ((n + 63) // 64) * 1021) for n in shapes]
        eng = capi.Engine(0, devs[:1], devs[1:])
        rs = eng.resume(7, 360, 1440)
        per_slot = sum(2 * 16 * 8 * pad_cols(n) for n in shapes) + META_BYTES
        assert rs.bytes == 7 * per_slot, (shapes, rs.bytes, per_slot)
        rs.destroy()
        eng.destroy()
        for d in devs:
            d.free()
    assert [pad_cols(n) for n in (56, 100, 243, 300, 4090, 8200)] == [1, 2, 4, 8, 64, 256]


# ---------------------------------------------------------------------------------------------------- calls refused whole
def test_calls_are_refused_whole_with_the_fault_named():
    d13, d31 = capi.DeviceIBF.create(0, 70, 3, 13, 128 * 1021), capi.DeviceIBF.create(0, 70, 3, 31, 128 * 1021)

    def refused(fn, text):
        with pytest.raises(capi.RBError) as ei:
            fn()
        assert ei.value.status == capi.RB_ERR_INVALID_ARG and text in capi.lib().rb_last_error().decode(), (text, capi.lib().rb_last_error())

    mixed = capi.Engine(0, [d13], [d31])
    refused(lambda: mixed.resume(4, 360, 1440), "one k")
    mixed.destroy()
    eng = capi.Engine(0, [d13], [])
    refused(lambda: eng.resume(0, 360, 1440), "at least one slot")
    refused(lambda: eng.resume(4, 0, 1440), "max_chunk_len")
    refused(lambda: eng.resume(4, 1441, 1440), "max_chunk_len")
    eng.set_column_shard(0, 2)
    refused(lambda: eng.resume(4, 360, 1440), "column-sharded")
    eng.set_column_shard(0, 1)
    rs = eng.resume(4, 360, 1440)
    read = PE.sequence()[:300]
    assert int(feed(rs, [(0, read, FIRST)])["total_len"][0]) == 300
    refused(lambda: rs.counts(4, 0), "slot")
    refused(lambda: rs.counts(0, 1), "filter")
    eng.set_column_shard(1, 2)
    refused(lambda: feed(rs, [(0, read[:10], 0)]), "column-sharded")
    eng.set_column_shard(0, 1)
    d13.add_sequence(read, 1000, 0)  # the filter's bits move: the counters are stale
    refused(lambda: feed(rs, [(0, read[:10], 0)]), "stale")
    assert rs.counts(0, 0)[1] == 300
    rs.destroy()
    rs = eng.resume(4, 360, 1440)  # a new set counts the new bits
    assert int(feed(rs, [(0, read, FIRST)])["max_count"][0, 0]) == 288
    rs.destroy()
    eng.destroy()
    d13.free()
    d31.free()

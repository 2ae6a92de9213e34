"""The long-read builds of the count kernel (K1) against the oracle, with bin counts at the edges of the bit-sliced counters.

Reads of more than 512 k-mers, filters wider than four words, micro-batches, merged tables and filters with h != 3 are served by the
plain kernel (ibf_count_max_kernel and its early-decision twin), the latency kernels (ibf_count_max_split_kernel, and
ibf_count_max_split_any_kernel for filters of different geometries in one launch), the merged kernel and the general build of the
phased kernel.  Their counters have 10 bit planes when the longest read of the batch has at most 1023 k-mers, 16 above
(rb_engine.hip, plan_geometry and the merged path), and a carry out of the top plane is dropped.  So every batch here carries fully
matched reads -- reads whose whole sequence was inserted into one bin, whose maximum is their k-mer count -- at 511, 512, 513 and 1023
k-mers (the top plane of ten), at 1024 (the switch to sixteen), and at 32767, 32768, 65535, 65536 and 65537 (the top plane of sixteen
and the wrap to 0 and 1 that the reference's uint16_t counters make).  Reads whose maximum sits at t - 1, t and t + 1 of their
thresholds test the decisions and the early-decision twins.  Every launch is compared bit for bit with the oracle, and at the end a test
asserts that every build the launchers can select was reached, so that a planner change cannot make this test less unnoticed."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import pyoracle as po
from readbouncer_amd import capi
from tests import helpers as H

ORACLE_THREADS = 16
# kernel geometries: (log2 lanes per block, words per lane), as rb_kernels.hip dispatch_lg_wpl selects them
GEOMS = ((0, 1), (1, 1), (2, 1), (3, 1), (4, 1), (5, 1), (6, 1), (6, 2))


def _geom(lg, wpl):
    return "LG=%d,WPL=%d" % (lg, wpl)


# every instantiation of the long-read builds the launchers can select (rb_kernels.hip: launch_ibf_count_max, dispatch_planes_hash,
# launch_count_nt, launch_split, the fall-through of launch_phased, launch_ibf_count_max_merged)
EXPECTED_BUILDS = set()
for _lg, _wpl in GEOMS:
    for _nt in (0, 1):
        for _np, _hash in ((10, "h=3"), (16, "h=3"), (16, "generic")):
            EXPECTED_BUILDS.add("plain<%s,NP=%d,%s,NT=%d>" % (_geom(_lg, _wpl), _np, _hash, _nt))
        EXPECTED_BUILDS.add("early<%s,NP=10,h=3,NT=%d>" % (_geom(_lg, _wpl), _nt))
        for _np in (10, 16):
            EXPECTED_BUILDS.add("split<%s,NP=%d,NT=%d>" % (_geom(_lg, _wpl), _np, _nt))
for _np in (10, 16):
    for _wide in (0, 1):
        EXPECTED_BUILDS.add("split_any<NP=%d,WIDE=%d>" % (_np, _wide))
    for _lg in (1, 2, 3, 4):
        for _nt in (0, 1):
            EXPECTED_BUILDS.add("merged<LG=%d,NP=%d,NT=%d>" % (_lg, _np, _nt))
    for _lg in (0, 1):
        EXPECTED_BUILDS.add("phased<LG=%d,NP=%d,general>" % (_lg, _np))
# what plan() does not name but the launch depends on (several workgroups per read or one, idle lanes in a block, two column slices,
# non-temporal filters in a mixed launch), and the k and h values of the matrix: each entry of SINGLE, MIXED and the forms is needed
EXPECTED_RUNTIME = {"split parts %s, %s" % (c, _geom(lg, wpl)) for c in ("> 1", "= 1") for lg, wpl in ((5, 1), (6, 1), (6, 2))}
EXPECTED_RUNTIME |= {"two column slices, latency form", "two column slices, throughput form", "mixed geometries, NT=0",
                     "mixed geometries, NT=1", _geom(2, 1) + ", idle lanes", _geom(2, 1) + ", every lane", _geom(6, 1) + ", idle lanes",
                     _geom(6, 1) + ", every lane", _geom(6, 2) + ", one column slice", "k=31, " + _geom(0, 1), "k=15, " + _geom(1, 1),
                     "k=15, " + _geom(4, 1), "k=31, " + _geom(6, 2)}
EXPECTED_RUNTIME |= {"generic h=%d" % h for h in (1, 2, 4, 5, 8)}

# filters on their own (bins, k): W = 1, 2, 3, 4, 6, 10, 17, 33, 64, 66 and 130 words; k = 15 and 31 on a few of them
SINGLE = ((56, 13), (100, 13), (130, 13), (256, 13), (350, 13), (600, 13), (1030, 13), (2100, 13), (4096, 13), (4200, 13), (8300, 13),
          (56, 31), (100, 15), (600, 15), (4200, 31))
GENERIC_H = (1, 2, 4, 5, 8)
# merged groups (members' bins, log2 lanes per merged block): merged blocks of 2, 4, 7 and 13 words
GROUPS = (((40, 50), 1), ((100, 64, 40), 2), ((200, 130), 3), ((500, 300), 4))
# filters of different geometries fused into one latency launch: without and with 16-byte lanes
MIXED = ((56, 600, 2100), (130, 4200))

FULL_A = (1023, 511, 512, 513)       # k-mers of the fully matched reads of the ten-plane batch
EDGE_A = (1023, 600)                 # read length classes (k-mers) with reads at their thresholds
BIG = (32767, 32768, 65535, 65536, 65537)
BIG_UNITS = (997, 991, 983, 977, 971)  # period of the tandem repeats the big reads are made of (k-mers in a bin stay few)

_reached = {}     # build -> labels of the launches that matched the oracle through it
_batches = {}     # build -> batches it counted
_runtime = set()


def _record(build, batch, label):
    _reached.setdefault(build, set()).add(label)
    _batches.setdefault(build, set()).add(batch)
_tests_run = set()


def rc(s):
    return "".join("ACGTN"[x] for x in po.revcomp(po.encode(s)))


def n_kmers(L, k):
    return L - k + 1 if L >= k else 0


def hbm_stride(W):
    """rb_engine.hip, hbm_stride"""
    if W % 16 == 0:
        return W
    if W < 16:
        s = 1
        while s < W:
            s <<= 1
        return s
    return (W + 15) // 16 * 16


def split_parts(lg, kmers, n_items, max_parts, max_sub):
    """workgroups per read of the latency form (rb_kernels.hip, split_parts_plan): plan() does not report them"""
    if max_parts <= 1 or lg < 5:
        return 1
    bpt = 8 if lg == 6 else 4
    tiles = (kmers + 63) // 64
    if tiles == 0:
        return 1
    wps = 4
    cap = min(max_parts, 200 // n_items if n_items else 1)
    if cap <= 1:
        return 1
    s = 1
    while s * 2 <= bpt and s * 2 <= max_sub:
        s *= 2
    while s >= 1:
        p = min((tiles * s + wps - 1) // wps, cap)
        m = s // wps if s > wps else 1
        p = p // m * m
        if p >= 2:
            return p
        s >>= 1
    return 1


class Plant:
    """Sequences to insert (one bin each) and the batches whose reads they match.  Batch "A": longest read 1023 k-mers (ten planes);
    "B": 1024 (sixteen); "C": 32767 to 65537 k-mers.  full: (batch, read, k-mers, item) of the fully matched reads; edges: (batch, read,
    k-mer class, m) of reads whose item is the first m k-mers of the read."""

    def __init__(self, rng, k, big):
        self.k = k
        self.items, self.full, self.edges = [], [], []
        self.batches = {"A": [], "B": []}
        A, B = self.batches["A"], self.batches["B"]
        for n in FULL_A:
            s = H.random_dna(rng, n + k - 1)
            self._fully_matched("A", s, n, both=True)
        self._edge_reads(rng, "A", EDGE_A)
        A += [H.mutate(rng, A[0], 0.02), rc(H.mutate(rng, A[2], 0.05)), H.random_dna(rng, 700, with_n=0.02), "ACGT" * 3, ""]
        s = H.random_dna(rng, 1024 + k - 1)
        self._fully_matched("B", s, 1024, both=True)
        B.append(A[0])
        self.full.append(("B", len(B) - 1, 1023, 0))
        self._edge_reads(rng, "B", (1024,))
        B.append(H.mutate(rng, s, 0.03))
        if big:
            self.batches["C"] = []
            for n, u in zip(BIG, BIG_UNITS):
                L = n + k - 1
                unit = H.random_dna(rng, u)
                self._fully_matched("C", (unit * (L // u + 1))[:L], n, both=n in (32768, 65536, 65537))

    def _item(self, seq):
        self.items.append(seq)
        return len(self.items) - 1

    def _fully_matched(self, batch, s, n, both):
        it = self._item(s)
        reads = self.batches[batch]
        reads.append(s)
        self.full.append((batch, len(reads) - 1, n, it))
        if both:
            reads.append(rc(s))
            self.full.append((batch, len(reads) - 1, n, it))

    def _edge_reads(self, rng, batch, classes):
        k = self.k
        reads = self.batches[batch]
        for n in classes:
            L = n + k - 1
            ts = {po.threshold(L, k), po.threshold(L, k, 0.08)}  # the decision's threshold and the early twins' larger one
            for m in sorted({t + d for t in ts for d in (-1, 0, 1)}):
                if not 1 <= m <= n:
                    continue
                for rep in range(2):
                    s = H.random_dna(rng, L)
                    self._item(s[:m + k - 1])
                    reads.append(s if rep == 0 else rc(s))
                    self.edges.append((batch, len(reads) - 1, n, m))

    def insert_into(self, d):
        n_bins = d.info["n_bins"]
        starts = np.cumsum([0] + [len(s) for s in self.items[:-1]]).astype(np.uint64)
        ends = starts + np.array([len(s) for s in self.items], dtype=np.uint64)
        d.insert("".join(self.items), starts, ends, np.arange(len(self.items), dtype=np.uint64) % n_bins)


def make_filter(bins, h, k, n_blocks=None):
    W = (bins + 63) // 64
    if n_blocks is None:  # tables of at most 32 MiB, sparse enough that a read's count in a bin it was not put into stays near 0
        n_blocks = min(32749, (32 << 20) // (hbm_stride(W) * 8))
    d = capi.DeviceIBF.create(0, bins, h, k, W * 64 * n_blocks)
    assert d.info["n_blocks"] == n_blocks and d.info["bin_width"] == W
    return d


def oracle_view(d):
    host = d.download()
    i = host.info
    return po.OracleIBF.wrap(i["n_bins"], i["n_hash"], i["kmer_size"], i["n_bits"], host.words()), host


class Batch:
    def __init__(self, name, reads, k):
        self.name, self.reads = name, reads
        self.buf, self.offs, self.lens = H.pack_reads(reads)
        self.n = len(reads)
        self.max_len = int(self.lens.max())
        self.kmers = n_kmers(self.max_len, k)
        self.planes = 10 if self.kmers <= 1023 else 16

    def expect(self, deplete, target):
        exp = np.stack([po.batch_raw_max(v, self.buf, self.offs, self.lens, ORACLE_THREADS) for v in deplete + target], axis=1)
        dec, st = po.batch_check_unblock(deplete, target, self.buf, self.offs, self.lens, n_threads=ORACLE_THREADS)
        return exp, dec, st


def check_fixture(plant, batch, exp, view, h, label):
    """the counts the batch was built for are the oracle's: fully matched reads at their k-mer count (or its uint16_t wrap), and
    with h = 3 the threshold reads at t - 1, t and t + 1"""
    n_bins = view.n_bins
    for b, i, n, it in plant.full:
        if b != batch.name:
            continue
        if n < 65536:
            assert exp[i] == n, (label, batch.name, i, n, int(exp[i]))
        else:
            assert exp[i] < n - 65536 + 4096, (label, batch.name, i, n, int(exp[i]))  # the count wrapped
        cnt = view.count(po.encode(plant.items[it]))
        assert cnt[it % n_bins] == n % 65536, (label, n, int(cnt[it % n_bins]))
    if batch.name == "A":
        assert batch.planes == 10 and batch.kmers == 1023 and exp.max() == 1023
    else:
        assert batch.planes == 16 and batch.kmers == (1024 if batch.name == "B" else 65537)
    if h != 3:
        return
    # (two candidates per count: a k-mer of the rest of a read that hits by chance moves that read off its count)
    want = {(n, m) for b, _, n, m in plant.edges if b == batch.name}
    landed = {(n, m) for b, i, n, m in plant.edges if b == batch.name and exp[i] == m}
    assert (want or batch.name == "C") and landed == want, (label, batch.name, "threshold reads that missed their count", sorted(want - landed))


def configure(eng, form, narrow):
    """engine settings of a form.  narrow: filters of one or two words, which the throughput form sends to the phased kernel unless
    that is switched off"""
    lat = form.startswith("lat")
    eng.set_split_threshold(2048 if lat else 0)
    eng.set_nt_threshold(0 if form.endswith("nt") else 512 << 20)
    if form == "lat-1part":
        eng.set_split_parts(1, 1)
    else:
        eng.set_split_parts(8, 4)
    eng.set_early_decision(form.startswith("early"))
    if form == "phased":
        eng.set_phased(0, 1 << 40, 300, 0, 1)
        eng.set_phase_slices(1, 8)
    elif narrow and not lat:
        eng.set_phased(0, 0, 0, 0, 0)
        eng.set_phase_slices()
    else:
        eng.set_phased()
        eng.set_phase_slices()


def build_of(p, h, form, kmers):
    """the instantiation a single-filter launch used: plan() and the settings of the form"""
    kernel = p["kernel"]
    g = _geom(p["lanes_per_block_log2"], p["words_per_lane"])
    np_, nt = p["counter_planes"], p["nontemporal"]
    if kernel == "ibf_count_max_split_kernel":
        return "split<%s,NP=%d,NT=%d>" % (g, np_, nt)
    if kernel == "ibf_count_max_merged_kernel":
        return "merged<LG=%d,NP=%d,NT=%d>" % (p["lanes_per_block_log2"], np_, nt)
    if kernel == "ibf_count_max_phased_kernel":
        assert kmers > 512, p  # (the short builds are test_gpu_short_builds.py's)
        return "phased<LG=%d,NP=%d,general>" % (p["lanes_per_block_log2"], np_)
    assert kernel == "ibf_count_max_kernel", p
    if h != 3:
        return "plain<%s,NP=16,generic,NT=%d>" % (g, nt)  # (dispatch_planes_hash: 16 planes, run-time hashes, at any read length)
    if form.startswith("early") and np_ == 10:
        return "early<%s,NP=10,h=3,NT=%d>" % (g, nt)
    return "plain<%s,NP=%d,h=3,NT=%d>" % (g, np_, nt)


def run_form(eng, batch, exp, exp_dec, exp_st, form, where):
    """one launch of the batch; raw maxima (unless the form asks for decisions only) and decisions against the oracle"""
    if form.startswith("early"):
        dec, st = eng.decide(batch.buf, batch.offs, batch.lens)
    else:
        mc, _, dec, st = eng.classify(batch.buf, batch.offs, batch.lens)
        bad = np.nonzero((mc != exp).any(axis=1))[0]
        assert len(bad) == 0, (where, [(int(i), int(batch.lens[i]), mc[i].tolist(), exp[i].tolist()) for i in bad[:6]])
    bad = np.nonzero((dec != exp_dec) | (st != exp_st))[0]
    assert len(bad) == 0, (where, "decision/status", [(int(i), int(batch.lens[i]), int(dec[i]), int(exp_dec[i]), int(st[i]), int(exp_st[i]))
                                                      for i in bad[:6]])


@pytest.mark.parametrize("bins,k", SINGLE)
def test_single_filter_builds_match_oracle(bins, k):
    W = (bins + 63) // 64
    big = k == 13
    rng = np.random.default_rng(1000 * W + k)
    plant = Plant(rng, k, big)
    hashes = (3, GENERIC_H[SINGLE.index((bins, k)) % len(GENERIC_H)]) if big else (3,)  # (and the generic-hash build at this geometry)
    filters = [(h, make_filter(bins, h, k)) for h in hashes]
    try:
        for h, d in filters:
            plant.insert_into(d)
            view, _keep = oracle_view(d)
            eng = capi.Engine(0, [d], [])
            try:
                _single(eng, plant, view, h, W, bins, k)
            finally:
                eng.destroy()
    finally:
        for _, d in filters:
            d.free()
    _tests_run.add(("single", bins, k))


def _single(eng, plant, view, h, W, bins, k):
    narrow = W <= 2
    forms = ["lat", "lat-nt", "thr", "thr-nt"]
    if h == 3:
        forms += ["early", "early-nt"] + (["phased"] if narrow else [])
    for name in sorted(plant.batches):
        batch = Batch(name, plant.batches[name], k)
        exp, exp_dec, exp_st = batch.expect([view], [])
        check_fixture(plant, batch, exp[:, 0], view, h, (bins, k, h))
        for form in forms + (["lat-1part"] if h == 3 and W > 16 else []):
            configure(eng, form, narrow)
            p = eng.plan(0, batch.n, batch.max_len)
            assert p["counter_planes"] == batch.planes, (bins, k, name, p)
            build = build_of(p, h, form, batch.kmers)
            if h == 3:  # each form reaches the kernel it is meant for
                want = {"lat": "ibf_count_max_split_kernel", "phased": "ibf_count_max_phased_kernel"}.get(form.split("-")[0], "ibf_count_max_kernel")
                assert p["kernel"] == want, (form, p)
            else:
                assert p["kernel"] == "ibf_count_max_kernel", (form, p)
            where = (bins, k, h, name, form, build)
            run_form(eng, batch, exp, exp_dec, exp_st, form, where)
            _record(build, name, "W=%d,k=%d,h=%d,%s,%s" % (W, k, h, name, form))
            g = _geom(p["lanes_per_block_log2"], p["words_per_lane"])
            if p["split_waves"]:
                parts = split_parts(p["lanes_per_block_log2"], batch.kmers, batch.n * p["column_slices"], 1 if form == "lat-1part" else 8,
                                    1 if form == "lat-1part" else 4)
                if parts > 1:
                    assert p["split_waves"] == 8, (where, p)  # (split_parts_plan gives every multi-workgroup read 2 x 4 waves)
                _runtime.add("split parts %s, %s" % ("> 1" if parts > 1 else "= 1", g))
            lanes = (1 << p["lanes_per_block_log2"]) * p["words_per_lane"]
            _runtime.add("%s, %s" % (g, "every lane" if W % lanes == 0 else "idle lanes"))
            if p["column_slices"] == 2:
                _runtime.add("two column slices, " + ("latency form" if p["split_waves"] else "throughput form"))
            elif p["words_per_lane"] == 2:
                _runtime.add(g + ", one column slice")
            _runtime.add("k=%d, %s" % (k, g))
            if h != 3:
                _runtime.add("generic h=%d" % h)


@pytest.mark.parametrize("members,lg", GROUPS)
def test_merged_builds_match_oracle(members, lg):
    """One merged table per engine (set_merge(2)), served by ibf_count_max_merged_kernel for reads of more than 512 k-mers"""
    k = 13
    rng = np.random.default_rng(77 + lg)
    plant = Plant(rng, k, True)
    n_blocks = 16381
    filters = [make_filter(b, 3, k, n_blocks) for b in members]
    try:
        views = []
        for d in filters:
            plant.insert_into(d)
            views.append(oracle_view(d))
        eng = capi.Engine(0, filters[:1], filters[1:])
        try:
            eng.set_merge(2)
            for name in sorted(plant.batches):
                batch = Batch(name, plant.batches[name], k)
                exp, exp_dec, exp_st = batch.expect([v for v, _ in views[:1]], [v for v, _ in views[1:]])
                for fi, (v, _) in enumerate(views):
                    check_fixture(plant, batch, exp[:, fi], v, 0, (members, fi))
                for form in ("thr", "thr-nt"):
                    configure(eng, form, False)
                    plans = [eng.plan(fi, batch.n, batch.max_len) for fi in range(len(filters))]
                    for p in plans:
                        assert p["kernel"] == "ibf_count_max_merged_kernel" and p["merged_members"] == len(members), p
                        assert p["lanes_per_block_log2"] == lg and p["counter_planes"] == batch.planes, p
                    build = build_of(plans[0], 3, form, batch.kmers)
                    run_form(eng, batch, exp, exp_dec, exp_st, form, (members, name, form, build))
                    assert eng.merge_info()[:2] == (1, len(members))
                    _record(build, name, "merged %s,%s,%s" % (members, name, form))
        finally:
            eng.destroy()
    finally:
        for d in filters:
            d.free()
    _tests_run.add(("merged", members))


@pytest.mark.parametrize("bins", MIXED)
def test_mixed_geometry_latency_builds_match_oracle(bins):
    """Filters of different geometries on a micro-batch: one launch of ibf_count_max_split_any_kernel for all of them"""
    k = 13
    rng = np.random.default_rng(5 + len(bins))
    plant = Plant(rng, k, True)
    filters = [make_filter(b, 3, k) for b in bins]
    nd = (len(bins) + 1) // 2
    try:
        views = []
        for d in filters:
            plant.insert_into(d)
            views.append(oracle_view(d))
        eng = capi.Engine(0, filters[:nd], filters[nd:])
        try:
            for name in sorted(plant.batches):
                batch = Batch(name, plant.batches[name], k)
                assert batch.n <= 64  # (launch_fused_groups mixes geometries in one launch for micro-batches of up to 64 reads)
                exp, exp_dec, exp_st = batch.expect([v for v, _ in views[:nd]], [v for v, _ in views[nd:]])
                for fi, (v, _) in enumerate(views):
                    check_fixture(plant, batch, exp[:, fi], v, 3, (bins, fi))
                for form in ("lat", "lat-nt"):
                    configure(eng, form, False)
                    plans = [eng.plan(fi, batch.n, batch.max_len) for fi in range(len(filters))]
                    geoms = {(p["lanes_per_block_log2"], p["words_per_lane"], p["nontemporal"]) for p in plans}
                    assert all(p["kernel"] == "ibf_count_max_split_kernel" and p["column_slices"] == 1 for p in plans), plans
                    assert len(geoms) == len(bins) and {p["counter_planes"] for p in plans} == {batch.planes}, plans
                    build = "split_any<NP=%d,WIDE=%d>" % (batch.planes, int(any(p["words_per_lane"] == 2 for p in plans)))
                    run_form(eng, batch, exp, exp_dec, exp_st, form, (bins, name, form, build))
                    _record(build, name, "mixed %s,%s,%s" % (bins, name, form))
                    _runtime.add("mixed geometries, NT=%d" % int(form.endswith("nt")))
        finally:
            eng.destroy()
    finally:
        for d in filters:
            d.free()
    _tests_run.add(("mixed", bins))


ALL_TESTS = {("single", b, k) for b, k in SINGLE} | {("merged", m) for m, _ in GROUPS} | {("mixed", b) for b in MIXED}


def test_every_count_build_was_reached():
    """Coverage of the matrix above: every build in EXPECTED_BUILDS matched the oracle at least once, and the launches with several
    workgroups per read and with two column slices ran.  A planner change that stops routing a batch to a build makes this fail
    instead of silently testing less."""
    if _tests_run != ALL_TESTS:
        pytest.skip("runs after the whole matrix of this file")
    missing = EXPECTED_BUILDS - set(_reached)
    assert not missing, ("builds never reached", sorted(missing), "reached", sorted(_reached))
    assert not set(_reached) - EXPECTED_BUILDS, ("builds outside the list", sorted(set(_reached) - EXPECTED_BUILDS))
    assert EXPECTED_RUNTIME <= _runtime, ("runtime cases never reached", sorted(EXPECTED_RUNTIME - _runtime))
    # every sixteen-plane build counted the 1024-k-mer batch and the one up to the uint16_t wrap; every ten-plane build the 1023
    for b in EXPECTED_BUILDS:
        want = {"B", "C"} if "NP=16" in b else {"A"}
        assert want <= _batches[b], (b, "batches never counted", sorted(want - _batches[b]))
    assert len(EXPECTED_BUILDS) == 120
    print("reached builds:\n  " + "\n  ".join("%s: %d launches" % (b, len(v)) for b, v in sorted(_reached.items())))

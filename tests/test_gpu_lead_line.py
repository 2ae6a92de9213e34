"""The lead line of bound pruning (rb_kernels.hip, ibf_count_max_kernel; bit 3 of rb_engine_set_prune_parts): once the probes have chosen
the leading strand, the lanes of the 128-byte line that holds its best probe bin are counted to the end first, alone; the strand's other
lanes are then certified against that count from hash 0, or counted in full against it, or -- after a failed certificate -- cleared and
counted again from k-mer 0.  None of that may change a result: every batch is compared bit for bit -- raw maxima, decisions, status -- with
the oracle and with pruning switched off, under mask 7 (the paths as they were), under mask 15 with the engine's own rule, and under mask
15 with the attempts forced (rb_engine_set_lead_min 0, rb_engine_set_cert_load 0), twice each.  The trace (bits 4-6 of a record) proves,
read by read, that the path a fixture was built for was the one taken.

Bins: with two words per lane a lane holds 128 bins, with one word 64; a 128-byte line holds 1024 bins either way, so bin b lies in line
b // 1024.  Windows and strands as in tests/test_gpu_strand_lead.py: window p is bases [p, p + k) of the read as given, the probe of a
strand is its windows 0..63."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import pyoracle as po
from readbouncer_amd import capi
from tests import helpers as H
from tests import test_gpu_bound_pruning as BP
from tests import test_gpu_strand_lead as SL

K = BP.K
TILE = SL.TILE
LINE_BINS = 1024
# (label, mask, lead_min, cert_load); < 0: the engine derives the value
SETTINGS = (("mask 7", 7, -1, -1.0), ("mask 15", 15, -1, -1.0), ("mask 15, forced", 15, 0, 0.0))


class Trace(SL.Trace):
    def take(self):
        self.torch.cuda.synchronize()
        raw = self.t.cpu().numpy().view(np.uint64).copy()
        t = super().take()
        for name, bit in (("line", 4), ("line_tried", 5), ("line_held", 6)):
            t[name] = ((raw >> np.uint64(bit)) & np.uint64(1)).astype(np.int64)
        return t


def settings(eng, nf, mask, lead_min, load):
    eng.set_prune_parts(mask)
    for fi in range(nf):
        eng.set_lead_min(fi, lead_min)
        eng.set_cert_load(fi, load)


def forced(eng, nf=1):
    settings(eng, nf, 15, 0, 0.0)


def defaults(eng, nf=1):
    settings(eng, nf, 15, -1, -1.0)


def check(eng, batch, ref, label, nf=1):
    """oracle == pruning off == every setting, every repeat"""
    buf, offs, lens = batch
    exp, exp_dec, exp_st = ref

    def run(what):
        mc, _, dec, st = eng.classify(buf, offs, lens)
        bad = np.nonzero((mc != exp).any(axis=1))[0]
        assert len(bad) == 0, (label, what, [(int(i), int(lens[i]), mc[i].tolist(), exp[i].tolist()) for i in bad[:6]])
        assert np.array_equal(dec, exp_dec) and np.array_equal(st, exp_st), (label, what, "decision/status")
        return mc, dec, st

    try:
        eng.set_bound_pruning(0)
        off = run("pruning off")
        eng.set_bound_pruning(1)
        for name, mask, lead_min, load in SETTINGS:
            settings(eng, nf, mask, lead_min, load)
            for rep in range(2):
                out = run((name, rep))
                assert all(np.array_equal(a, b) for a, b in zip(out, off)), (label, name, rep, "differs from pruning off")
    finally:
        eng.set_bound_pruning(1)
        defaults(eng, nf)


def plain_form(eng, fi, n_reads, max_len, wpl=2, slices=1, nt=0, planes=10):
    eng.set_split_threshold(0)
    p = eng.plan(fi, n_reads, max_len)
    got = (p["kernel"], p["lanes_per_block_log2"], p["words_per_lane"], p["column_slices"], p["nontemporal"], p["counter_planes"])
    assert got == ("ibf_count_max_kernel", 6, wpl, slices, nt, planes), p


class LinePlant(BP.Plant):
    """reads whose windows go into chosen bins of chosen lines; per read the maximum it is built for and what the trace has to show under
    the forced setting: (leading strand, line attempted, certificate of the other lanes attempted, held, bin whose wave is meant), or None"""

    def __init__(self, n_bins, seed, wpl=2):
        super().__init__(n_bins, seed)
        self.lane_bins = 64 * wpl
        self.n_lines = min(n_bins, 8192) // LINE_BINS  # (bins of the first column slice; `slice_of` moves a read's bins to another)
        self.expect = []

    def bin_in(self, line, lane=None, base=0):
        for _ in range(10000):
            if lane is None:
                b = base + line * LINE_BINS + int(self.rng.integers(0, LINE_BINS))
            else:
                b = base + line * LINE_BINS + lane * self.lane_bins + int(self.rng.integers(0, self.lane_bins))
            if b < self.n_bins and b not in self.used:
                self.used.add(b)
                return b
        raise AssertionError("no free bin")

    def two_lines(self):
        x, y = self.rng.choice(self.n_lines, size=2, replace=False)
        return int(x), int(y)

    def make(self, n, lead_w, trail_w, want, expect, reverse=False):
        """lead_w / trail_w: (bin, first window, windows) of the strand that is to lead / to trail; reverse: the leader is the reverse strand"""
        R = H.random_dna(self.rng, n + K - 1)
        Q = BP.rc(R)
        fwd, rev = (trail_w, lead_w) if reverse else (lead_w, trail_w)
        for b, s, c in fwd:
            assert 0 <= s and c > 0 and s + c <= n
            self.put(R[s:s + c + K - 1], b)
        for b, s, c in rev:
            assert 0 <= s and c > 0 and s + c <= n
            self.put(Q[n - s - c:n - s + K - 1], b)
        self.read(R, want)
        self.expect.append(None if expect is None else (int(reverse),) + tuple(expect))
        return len(self.reads) - 1


def designed(p, n=348, base=0):
    """the shapes of the issue at n k-mers (n >= 128); returns {name: [read indices]}"""
    lanes = LINE_BINS // p.lane_bins
    idx = {}

    def add(name, i):
        idx.setdefault(name, []).append(i)

    for reverse in (False, True):
        X, Y = p.two_lines()
        A = p.bin_in(X, 1, base)
        # the best bin alone in the probe's line
        add("alone", p.make(n, [(A, 0, 20), (A, 100, 28)], [], 48, (1, 1, 1, A), reverse))
        # ... with a runner-up in its own lane, in another lane of the line, in another line
        A2, A3, B = p.bin_in(X, 1, base), p.bin_in(X, lanes - 1, base), p.bin_in(Y, None, base)
        add("same lane", p.make(n, [(A, 0, 20), (A, 100, 28), (A2, 0, 10), (A2, 80, 15)], [], 48, (1, 1, 1, A), reverse))
        add("same line", p.make(n, [(A, 0, 20), (A, 100, 28), (A3, 0, 10), (A3, 80, 15)], [], 48, (1, 1, 1, A), reverse))
        add("other line", p.make(n, [(A, 0, 20), (A, 100, 28), (B, 0, 10), (B, 80, 5)], [], 48, (1, 1, 1, A), reverse))
        # ... where the runner-up of the same line ends ABOVE the probe's best bin: the line pass itself finds it
        add("line overtakes", p.make(n, [(A, 0, 20), (A, 100, 8), (A3, 0, 10), (A3, 70, 40)], [], 50, (1, 1, 1, A), reverse))
        # the probe's leader in line X, the final best in line Y: windows 0-75 in A, the rest in B; the certificate of the other lanes
        # fails on B (its upper bound is the n - 76 it really has), they are counted again and B is found
        add("crossover", p.make(n, [(A, 0, 76), (B, 76, n - 76)], [], max(76, n - 76), (1, 1, int(n - 76 <= 76), A), reverse))
        # a tie of two lines in the probe: the line of the lower lane is taken, whichever bin wins later
        for winner in (0, 1):
            pair = (A, B)
            taken = min(pair, key=lambda b: (b - base) // p.lane_bins)
            w = pair[winner]
            add("tie", p.make(n, [(A, 0, 20), (B, 0, 20), (w, 100, 10)], [], 30, (1, 1, int(w // LINE_BINS == taken // LINE_BINS), taken), reverse))
        # the read's best on the trailing strand: the leader is done with its line and a certificate, the other strand finds the maximum
        add("trailing best", p.make(n, [(A, 0, 20), (A, 100, 10)], [(B, 0, 10), (B, 70, 40)], 50, (1, 1, 1, A), reverse))
        # a count of n: the other strand is not continued
        R = H.random_dna(p.rng, n + K - 1)
        W = p.bin_in(X, 0, base)
        p.put(R, W)
        p.read(BP.rc(R) if reverse else R, n)
        p.expect.append((int(reverse), 1, 1, 1, W))
        add("whole", len(p.reads) - 1)
    return idx


def assert_trace(t, p, n_of, slices=1, what=""):
    """the forced setting: every designed read shows the path it was built for, in the wave that holds its bin"""
    for i, e in enumerate(p.expect):
        if e is None:
            continue
        lead, line, tried, held, b = e
        r = i * slices + (b // 8192 if slices > 1 else 0)
        rec = {k: int(v[r]) for k, v in t.items()}
        assert rec["written"] == 1 and rec["probed"] == 1 and rec["lead"] == lead, (what, i, e, rec)
        assert (rec["line"], rec["line_tried"], rec["line_held"]) == (line, tried, held), (what, i, int(n_of[i]), e, rec)


def test_lead_line_sparse():
    import torch  # noqa: F401
    d = BP.make_filter(8192)
    p = LinePlant(8192, 501)
    idx = designed(p, 348)
    # the tile edges: the line continues behind the probe for 1, 8, 64, 65 k-mers
    edge = {}
    for n in (65, 72, 128, 129):
        for reverse in (False, True):
            X, Y = p.two_lines()
            A, B = p.bin_in(X), p.bin_in(Y)
            edge[(n, reverse)] = p.make(n, [(A, 0, 20), (A, TILE, n - TILE), (B, 0, 10)], [], 20 + n - TILE, (1, 1, 1, A), reverse)
            # 40 in A, then B of another line to the end: where B ends above A the certificate fails on it and it is found behind the failure
            p.make(n, [(A, 0, 40), (B, 40, n - 40)], [], max(40, n - 40), (1, 1, int(n - 40 <= 40), A), reverse)
    first_short = len(p.reads)
    for reverse in (False, True):  # 64 k-mers: no probe, no line
        X, Y = p.two_lines()
        p.make(64, [(p.bin_in(X), 0, 20), (p.bin_in(Y), 30, 34)], [], 34, None, reverse)
    # the maximum of the line against the upper bound of a bin of another line: one below, equal, one above
    first_edge = len(p.reads)
    edges = []
    for rep in range(3):
        for extra in (-1, 0, 1):
            for reverse in (False, True):
                X, Y = p.two_lines()
                A, B = p.bin_in(X), p.bin_in(Y)
                i = p.make(348, [(A, 0, 20), (A, 100, 20), (B, 0, 10), (B, 200, 30 + extra)], [], max(40, 40 + extra), None, reverse)
                edges.append((i, A, B, reverse))
    p.insert_into(d)
    eng = capi.Engine(0, [d], [])
    batch = H.pack_reads(p.reads)
    buf, offs, lens = batch
    plain_form(eng, 0, len(lens), int(lens.max()))
    n_of = lens.astype(np.int64) - K + 1
    ref = SL.oracle_results(batch, [d], [])
    BP.fixture_holds(p, ref[0][:, 0], "lead line, sparse")  # the fixture on the oracle alone, first
    view, host = BP.oracle_view(d)
    upper = {i: SL.hash0_upper(view, host, p.reads[i], int(reverse), B) for i, A, B, reverse in edges}
    assert {upper[i] - 40 for i, _, _, _ in edges} >= {-1, 0, 1}, sorted(upper.values())
    check(eng, batch, ref, "lead line, sparse")
    tr = Trace(eng, len(lens))
    try:
        forced(eng)
        eng.classify(*batch)
        t = tr.take()
        assert t["written"].all()
        assert_trace(t, p, n_of, what="forced")
        assert not t["probed"][first_short:first_edge].any() and not t["line"][first_short:first_edge].any()
        for i, A, B, reverse in edges:  # held exactly where the other bin's upper bound does not pass the line's maximum
            rec = {k: int(v[i]) for k, v in t.items()}
            assert (rec["lead"], rec["line"], rec["line_tried"]) == (int(reverse), 1, 1), (i, rec)
            assert rec["line_held"] == int(upper[i] <= 40), (i, upper[i], rec)
        # a whole read in one bin: the leader's maximum is n and the other strand stays at its probe
        for i in idx["whole"]:
            trailing = t["stop_rev"][i] if t["lead"][i] == 0 else t["stop_fwd"][i]
            assert trailing == TILE, (i, int(trailing))
        # lead_min picks the attempts: "alone" has 20 in its probe
        for lead_min, want in ((20, 1), (21, 0)):
            eng.set_lead_min(0, lead_min)
            eng.classify(*batch)
            t = tr.take()
            assert [int(t["line"][i]) for i in idx["alone"]] == [want] * len(idx["alone"]), lead_min
            assert all(t["line"][i] == 1 for i in idx["crossover"])  # (64 in its probe)
        # without the bit, or without the certificate it builds on: no attempt, and bits 0-3 as they were
        forced(eng)
        for mask in (7, 8 | 3, 8 | 1, 8 | 5):
            eng.set_prune_parts(mask)
            eng.classify(*batch)
            t7 = tr.take()
            assert not (t7["line"] | t7["line_tried"] | t7["line_held"]).any(), mask
    finally:
        tr.close()
        defaults(eng)


def test_saturated_bin_in_another_line():
    """a bin of another line with the bit of EVERY hash-0 block of the read: its upper bound reaches n, the certificate of the other lanes
    must fail and they are counted again -- with the bin's true count below the line's maximum, and above it"""
    import torch  # noqa: F401
    d0 = BP.make_filter(8192)
    p = LinePlant(8192, 511)
    cases = []
    for above in (False, True):
        for reverse in (False, True):
            X, Y = p.two_lines()
            A, S = p.bin_in(X), p.bin_in(Y)
            extra = [(S, 70, 100)] if above else []
            i = p.make(348, [(A, 0, 20), (A, 100, 30)] + extra, [], 100 if above else 50, (1, 1, 0, A), reverse)
            cases.append((i, S, reverse))
    p.insert_into(d0)
    host = d0.download()
    info = host.info
    words = host.words()
    view = po.OracleIBF.wrap(info["n_bins"], info["n_hash"], info["kmer_size"], info["n_bits"], words)
    W64 = ((info["n_bins"] + 63) // 64) * 64
    for i, S, reverse in cases:
        strand = BP.rc(p.reads[i]) if reverse else p.reads[i]
        o = po.encode(strand)
        for q in range(len(strand) - K + 1):
            pos = view.block_index(po.kmer_value(o[q:q + K], K), 0) * W64 + S
            words[pos >> 6] |= np.uint64(1) << np.uint64(pos & 63)
    d = capi.DeviceIBF.upload(0, host)
    eng = capi.Engine(0, [d], [])
    batch = H.pack_reads(p.reads)
    plain_form(eng, 0, len(p.reads), 360)
    ref = SL.oracle_results(batch, [d], [])
    BP.fixture_holds(p, ref[0][:, 0], "saturated bin")
    for i, S, reverse in cases:
        assert SL.hash0_upper(view, host, p.reads[i], int(reverse), S) >= 348 - TILE, i
    check(eng, batch, ref, "saturated bin")
    tr = Trace(eng, len(p.reads))
    try:
        forced(eng)
        eng.classify(*batch)
        assert_trace(tr.take(), p, np.full(len(p.reads), 348), what="saturated")
    finally:
        tr.close()
        defaults(eng)


BUILDS = {
    # name: (bins, hashes, blocks, non-temporal, words per lane, column slices)
    "one word per lane": (4096, 3, BP.N_BLOCKS, 0, 1, 1),
    "two column slices": (16384, 3, BP.N_BLOCKS // 2, 0, 2, 2),
    "two hashes": (8192, 2, BP.N_BLOCKS, 0, 2, 1),
    "four hashes": (8192, 4, BP.N_BLOCKS, 0, 2, 1),
    "non-temporal": (8192, 3, BP.N_BLOCKS, 1, 2, 1),
    "power-of-two blocks": (8192, 3, 131072, 0, 2, 1),
    "sixteen planes": (8192, 3, BP.N_BLOCKS, 0, 2, 1),
}


@pytest.mark.parametrize("build", sorted(BUILDS))
def test_builds(build):
    """every build the engine can plan for which the kernel leads: the designed shapes at 348 and 129 k-mers, in the second column slice too.
    (Filters of two and of four hashes take the build that hashes at run time, which neither probes nor leads: exact all the same, and the
    trace has to say so.)"""
    import torch  # noqa: F401
    bins, n_hash, n_blocks, nt, wpl, slices = BUILDS[build]
    d = capi.DeviceIBF.create(0, bins, n_hash, K, ((bins + 63) // 64) * 64 * n_blocks)
    p = LinePlant(bins, 520 + len(build), wpl)
    designed(p, 348)
    designed(p, 129)
    if slices > 1:
        designed(p, 348, base=8192)
    planes = 10
    if build == "sixteen planes":  # a read of 1100 k-mers in the batch: its leader's line holds 300, a bin of another line 420
        X, Y = p.two_lines()
        A, B = p.bin_in(X), p.bin_in(Y)
        p.make(1100, [(A, 0, 30), (A, 200, 270), (B, 10, 20), (B, 600, 400)], [], 420, (1, 1, 0, A))
        planes = 16
    p.insert_into(d)
    eng = capi.Engine(0, [d], [])
    if nt:
        eng.set_nt_threshold(1)
    batch = H.pack_reads(p.reads)
    lens = batch[2]
    plain_form(eng, 0, len(lens), int(lens.max()), wpl, slices, nt, planes)
    ref = SL.oracle_results(batch, [d], [])
    BP.fixture_holds(p, ref[0][:, 0], build)
    check(eng, batch, ref, build)
    tr = Trace(eng, len(lens) * slices)
    try:
        forced(eng)
        eng.classify(*batch)
        t = tr.take()
        if n_hash == 3:
            assert_trace(t, p, lens.astype(np.int64) - K + 1, slices, build)
        else:
            assert t["written"].all() and not (t["probed"] | t["line"] | t["line_tried"] | t["line_held"]).any()
    finally:
        tr.close()
        defaults(eng)


def test_lead_line_dense():
    """the bench's bit density and read mix at mixed lengths: exact under every setting; forced, every read with a strand to continue takes
    the line and a certificate, which fails on the reads without a match; by the engine's own rule hardly a read without a match takes it"""
    import torch  # noqa: F401
    from readbouncer_amd import synth
    d = BP.make_filter(8192, n_blocks=32749, fill_seed=5)
    planted, starts, ends = synth.planted_reference(17, n_segments=512)
    d.insert(planted, starts, ends, (np.arange(512, dtype=np.uint64) * np.uint64(7919)) % np.uint64(8192))
    eng = capi.Engine(0, [d], [])
    buf, offs, lens = synth.make_reads(1, 3000, 360, planted, positive_fraction=0.5)
    lens = np.random.default_rng(1).integers(K - 1, 361, size=len(lens)).astype(np.uint32)
    batch = (buf, offs, lens)
    plain_form(eng, 0, len(lens), 360)
    n = np.maximum(lens.astype(np.int64) - K + 1, 0)
    ref = SL.oracle_results(batch, [d], [])
    exp = ref[0][:, 0].astype(np.int64)
    check(eng, batch, ref, "lead line, dense")
    tr = Trace(eng, len(lens))
    try:
        forced(eng)
        eng.classify(*batch)
        t = tr.take()
        probed = (n > TILE).astype(np.int64)
        assert np.array_equal(t["probed"], probed) and np.array_equal(t["line"], probed) and np.array_equal(t["line_tried"], probed)
        # hash 0 alone gives some bin about 0.215 rem + 3.8 sigma: far above a maximum of 0.1 n + 5 once rem >= 128
        negative = (n - TILE >= 128) & (exp <= 0.1 * n + 5)
        assert negative.sum() > 300 and not t["line_held"][negative].any()
        assert t["line_held"].sum() > 300
        # the engine's rule: lead_min is the count a read without a match reaches in a probe with probability <= 1 %
        defaults(eng)
        eng.classify(*batch)
        t = tr.take()
        print("derived rule: %d of %d reads without a match and %d of %d others took the line; certificates %d, held %d" % (
            t["line"][negative].sum(), negative.sum(), t["line"][~negative].sum(), (~negative).sum(), t["line_tried"].sum(), t["line_held"].sum()))
        assert t["line"][negative].mean() <= 0.03
        assert t["line"].sum() > 300
        assert not (t["line_held"] & ~t["line_tried"]).any() and not (t["line_tried"] & ~t["line"]).any()
    finally:
        tr.close()
        defaults(eng)

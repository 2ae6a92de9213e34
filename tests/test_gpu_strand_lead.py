"""The refinements of bound pruning in the plain count kernel (rb_kernels.hip, count_strand / ibf_count_max_kernel;
rb_engine_set_prune_parts): checks after every eight k-mers, the stronger strand finished first, the trailing strand certified from
hash 0 alone.  None of them may change a result, so every batch is compared bit for bit -- raw maxima, decisions, status -- with the
oracle and with pruning switched off, under all 8 masks, and repeated launches must agree.  The trace (rb_engine_set_prune_trace)
proves that the path a fixture was built for was the one taken.

Positions are WINDOWS of the read as given to the engine, in the order the kernel walks them: window p is bases [p, p + k); the
reverse strand's k-mer of window p is the window's reverse complement, i.e. k-mer n - 1 - p of the reverse-complemented read.  The
probe of a strand is its windows 0..63.

The sparse filter (8192 bins x 131 071 blocks) keeps chance hits at 0, so a read comes out at the maximum it was built for -- asserted
on the ORACLE (fixture_holds) before anything is said about the kernel; the dense one (8192 x 32 749, fill_synth) has the bench's bit
density."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import pyoracle as po
from readbouncer_amd import capi
from tests import helpers as H
from tests import test_gpu_bound_pruning as BP

K = BP.K
TILE = 64
ALL_MASKS = tuple(range(8))
SUB, LEAD, CERT = 1, 2, 4


class Trace:
    """device memory for the kernel's records, decoded"""

    def __init__(self, eng, n_records):
        import torch
        self.torch = torch
        self.eng = eng
        self.t = torch.zeros(n_records, dtype=torch.int64, device="cuda:0")
        torch.cuda.synchronize()
        eng.set_prune_trace(self.t.data_ptr())

    def take(self):
        self.torch.cuda.synchronize()
        r = self.t.cpu().numpy().view(np.uint64).copy()
        self.t.zero_()
        self.torch.cuda.synchronize()
        f = lambda sh, m: ((r >> np.uint64(sh)) & np.uint64(m)).astype(np.int64)
        return dict(lead=f(0, 1), probed=f(1, 1), tried=f(2, 1), held=f(3, 1), written=f(15, 1), stop_fwd=f(16, 0xFFFF), stop_rev=f(32, 0xFFFF))

    def close(self):
        self.eng.set_prune_trace(None)


def oracle_results(batch, deplete, target):
    buf, offs, lens = batch
    views = [BP.oracle_view(d) for d in deplete + target]  # (view, downloaded filter): the view reads the download's memory
    ov = [v for v, _ in views]
    exp = np.stack([po.batch_raw_max(v, buf, offs, lens, BP.ORACLE_THREADS) for v in ov], axis=1)
    return (exp,) + tuple(po.batch_check_unblock(ov[:len(deplete)], ov[len(deplete):], buf, offs, lens, n_threads=BP.ORACLE_THREADS))


def check(eng, reads_or_batch, deplete, target, label, masks=ALL_MASKS, repeats=2, ref=None):
    """oracle == pruning off == every mask, every repeat; returns the oracle's maxima (ref: oracle_results of the batch, computed before)"""
    buf, offs, lens = reads_or_batch if isinstance(reads_or_batch, tuple) else H.pack_reads(reads_or_batch)
    exp, exp_dec, exp_st = ref if ref is not None else oracle_results((buf, offs, lens), deplete, target)
    BP.plain_form(eng, len(deplete) + len(target), int(lens.max()), len(lens))

    def run(what):
        mc, _, dec, st = eng.classify(buf, offs, lens)
        bad = np.nonzero((mc != exp).any(axis=1))[0]
        assert len(bad) == 0, (label, what, [(int(i), int(lens[i]), mc[i].tolist(), exp[i].tolist()) for i in bad[:6]])
        assert np.array_equal(dec, exp_dec) and np.array_equal(st, exp_st), (label, what, "decision/status")
        return mc, dec, st

    eng.set_bound_pruning(0)
    off = run("pruning off")
    eng.set_bound_pruning(1)
    for mask in masks:
        eng.set_prune_parts(mask)
        first = None
        for rep in range(repeats):
            out = run(("mask", mask, rep))
            assert all(np.array_equal(a, b) for a, b in zip(out, off)), (label, mask, "differs from pruning off")
            assert first is None or all(np.array_equal(a, b) for a, b in zip(out, first)), (label, mask, "repeat differs")
            first = out
    eng.set_prune_parts(7)
    return exp


class WindowPlant(BP.Plant):
    """reads planted by window ranges per strand; `lead` = the strand the kernel must finish first (None: no probe, or not said)"""

    def __init__(self, n_bins, seed, k=K):
        super().__init__(n_bins, seed, k)
        self.lead = []

    def windows(self, n, fwd, rev, lead, where="lines", want=None):
        """fwd / rev: lists of (first window, windows) put into bin A / B; the read's maximum is `want` (default: the larger total)"""
        R = H.random_dna(self.rng, n + self.k - 1)
        A, B = self.pair(where)
        Q = BP.rc(R)
        for s, c in fwd:
            assert 0 <= s and s + c <= n and c > 0
            self.put(R[s:s + c + self.k - 1], A)
        for s, c in rev:
            assert 0 <= s and s + c <= n and c > 0
            self.put(Q[n - s - c:n - s + self.k - 1], B)
        self.read(R, max(sum(c for _, c in fwd), sum(c for _, c in rev)) if want is None else want)
        self.lead.append(lead)
        return A, B

    def split(self, *a, **kw):
        super().split(*a, **kw)
        self.lead.append(None)

    def whole(self, n, reverse):
        super().whole(n, reverse)
        self.lead.append(None if n <= TILE else int(reverse))


def sub_tile_plant(seed, k=K):
    """B ends one above A (and the mirror) with the crossover at every 8-k-mer offset of the first two tiles and one k-mer either
    side of each; A and B in one lane, two lanes of a line, different lines; the best strand forward and reverse"""
    p = WindowPlant(8192, seed, k)
    for tile in (0, 1):
        for j in range(1, 9):
            for d in (-1, 0, 1):
                a = tile * TILE + 8 * j + d
                n = 2 * a + 1
                for where in ("lane", "line", "lines"):
                    for reverse in (False, True):
                        p.split(n, a, where, reverse)      # A = a, then B = a + 1
                        p.split(n, a + 1, where, reverse)  # the mirror: A = a + 1 comes first
    return p


def test_sub_tile_tightness():
    import torch  # noqa: F401
    d = BP.make_filter(8192)
    cross = sub_tile_plant(301)
    edges = BP.tight_plant(8192, 302, kmers=(63, 64, 65, 72, 73, 128, 348, 401, 1023))
    for b in range(len(edges.bins)):  # (keep the two plants' bins apart: edges takes what cross left)
        while edges.bins[b] in cross.used:
            edges.bins[b] = (edges.bins[b] + 1) % 8192
        cross.used.add(edges.bins[b])
    long16 = WindowPlant(8192, 303)
    # (the leader ends at 100: this filter's fullest bin holds a 1023-k-mer read, a load of 0.024, which asks for ~47 over 1036 k-mers)
    long16.windows(1100, [(0, 30), (200, 70)], [(500, 110)], lead=0)  # forward stronger in the probe, the reverse strand wins behind it
    long16.windows(1100, [(700, 110)], [(0, 30), (300, 70)], lead=1)  # the mirror
    long16.windows(1100, [(0, 30), (200, 70)], [(900, 90)], lead=0)   # the trailing strand stays below the leader: certified from hash 0
    cross.insert_into(d)
    edges.insert_into(d)
    long16.insert_into(d)
    eng = capi.Engine(0, [d], [])
    exp = check(eng, cross.reads, [d], [], "crossovers")
    BP.fixture_holds(cross, exp[:, 0], "crossovers")
    exp = check(eng, edges.reads, [d], [], "tile edges")
    BP.fixture_holds(edges, exp[:, 0], "tile edges")
    # with the sub-tile checks a whole-wave stop may fall inside a tile: some read of the batch shows one (the path ran)
    tr = Trace(eng, len(edges.reads))
    try:
        eng.set_prune_parts(SUB)
        buf, offs, lens = H.pack_reads(edges.reads)
        eng.classify(buf, offs, lens)
        t = tr.take()
        assert t["written"].all() and not t["probed"].any()
        n = lens.astype(np.int64) - K + 1
        inside = ((t["stop_rev"] % TILE != 0) & (t["stop_rev"] < n)) | ((t["stop_fwd"] % TILE != 0) & (t["stop_fwd"] < n))
        assert inside.any(), "no strand was left inside a tile"
        assert ((t["stop_rev"] % 8 == 0) | (t["stop_rev"] == n)).all() and ((t["stop_fwd"] % 8 == 0) | (t["stop_fwd"] == n)).all()
        eng.set_prune_parts(0)  # without them every stop is a tile boundary
        eng.classify(buf, offs, lens)
        t = tr.take()
        assert ((t["stop_rev"] % TILE == 0) | (t["stop_rev"] == n)).all() and ((t["stop_fwd"] % TILE == 0) | (t["stop_fwd"] == n)).all()
    finally:
        tr.close()
        eng.set_prune_parts(7)
    # sixteen planes: the same reads in a batch with reads of 1100 k-mers, which are planted themselves -- one strand stronger in the
    # probe and the other winning behind it (either way round), and a trailing strand that stays below the leader (certified)
    batch16 = cross.reads[:60] + edges.reads[:40] + long16.reads
    exp = check(eng, batch16, [d], [], "sixteen planes", repeats=2)
    BP.fixture_holds(long16, exp[100:, 0], "sixteen planes")
    tr = Trace(eng, len(batch16))
    try:
        buf, offs, lens = H.pack_reads(batch16)
        assert eng.plan(0, len(batch16), int(lens.max()))["counter_planes"] == 16
        eng.classify(buf, offs, lens)
        t = tr.take()
        for i, lead in enumerate(long16.lead):
            rec = {k: int(v[100 + i]) for k, v in t.items()}
            assert rec["probed"] == 1 and rec["lead"] == lead and rec["tried"] == 1, (i, rec)
        assert t["held"][100 + 2] == 1 and t["held"][100] == 0 and t["held"][100 + 1] == 0
    finally:
        tr.close()


def lead_plant(seed, k=K):
    p = WindowPlant(8192, seed, k)
    p.windows(65, [(0, 5)], [(62, 3)], lead=0)  # one k-mer behind the probe: the end of a strand lies inside the other's probe windows
    p.windows(65, [(62, 3)], [(0, 5)], lead=1)
    for n in (65, 128, 348, 401):
        x = 5 if n == 65 else 20
        if n >= 128:
            p.windows(n, [(0, x)], [(n - x - 1, x + 1)], lead=0)    # the forward probe is stronger, the reverse strand wins by one at its end
            p.windows(n, [(n - x - 1, x + 1)], [(0, x)], lead=1)    # the mirror
        if n >= 128:
            p.windows(n, [(0, x)], [(0, x), (TILE + 10, 3)], lead=0)  # a tie in the probe (forward leads), the reverse strand wins later
            p.windows(n, [(0, x), (TILE + 10, 3)], [(0, x)], lead=0)  # ... and the forward strand wins later
        p.windows(n, [(0, x)], [(0, x)], lead=0)                    # a tie in the probe and in the result
        if n >= 128:
            p.windows(n, [(0, x)], [(TILE + 5, x)], lead=0)          # a tie in the result only
            p.windows(n, [(TILE + 5, x)], [(0, x)], lead=1)
        p.whole(n, False)
        p.whole(n, True)
    for n in (1, 64):  # no probe: the strands go forward, reverse
        p.whole(n, False)
        p.whole(n, True)
    p.windows(64, [(0, 9)], [(50, 10)], lead=None)
    return p


def test_lead():
    import torch  # noqa: F401
    d = BP.make_filter(8192)
    plant = lead_plant(311)
    plant.insert_into(d)
    eng = capi.Engine(0, [d], [])
    exp = check(eng, plant.reads, [d], [], "lead")
    BP.fixture_holds(plant, exp[:, 0], "lead")
    buf, offs, lens = H.pack_reads(plant.reads)
    n = lens.astype(np.int64) - K + 1
    tr = Trace(eng, len(plant.reads))
    try:
        for mask in (LEAD, LEAD | SUB, 7):
            eng.set_prune_parts(mask)
            eng.classify(buf, offs, lens)
            t = tr.take()
            assert t["written"].all()
            assert np.array_equal(t["probed"], (n > TILE).astype(np.int64)), mask
            for i, lead in enumerate(plant.lead):
                if lead is not None:
                    assert t["probed"][i] == 1 and t["lead"][i] == lead, (mask, i, int(n[i]), lead, {k: int(v[i]) for k, v in t.items()})
                if n[i] <= TILE:
                    assert t["lead"][i] == 0
            # a leader that reached n drops the other strand behind its probe
            for i, r in enumerate(plant.reads):
                if plant.want[i] == n[i] and n[i] > TILE:
                    trailing = t["stop_rev"][i] if t["lead"][i] == 0 else t["stop_fwd"][i]
                    assert trailing == TILE, (mask, i, int(trailing))
        eng.set_prune_parts(SUB)  # no lead: nothing is probed
        eng.classify(buf, offs, lens)
        t = tr.take()
        assert not t["probed"].any() and not t["lead"].any()
    finally:
        tr.close()
        eng.set_prune_parts(7)


def hash0_upper(view, host, read, strand, bin_no):
    """probe count + hash-0 hits behind the probe of `bin_no` on one strand of `read` (what the certificate pass counts), by hand"""
    info = host.info
    words = host.words()
    W64 = ((info["n_bins"] + 63) // 64) * 64
    n = len(read) - K + 1
    seq = read if strand == 0 else BP.rc(read)
    o = po.encode(seq)

    def bit(block):
        pos = block * W64 + bin_no
        return (int(words[pos >> 6]) >> (pos & 63)) & 1

    total = 0
    for p in range(n):
        q = p if strand == 0 else n - 1 - p
        v = po.kmer_value(o[q:q + K], K)
        hits = [bit(view.block_index(v, h)) for h in range(3)]
        total += int(all(hits)) if p < TILE else hits[0]
    return total


def test_certificate_sparse():
    import torch  # noqa: F401
    d = BP.make_filter(8192)
    p = WindowPlant(8192, 321)
    cases = []  # (read index, A, B, leader's maximum, trailing maximum)
    for n in (128, 348, 401):
        for M in (20, 30):
            for extra in (0, 1):
                for mirror in (False, True):
                    lead_w, trail_w = [(0, M)], [(TILE + 10, M + extra)]
                    A, B = p.windows(n, trail_w if mirror else lead_w, lead_w if mirror else trail_w, lead=int(mirror))
                    cases.append((len(p.reads) - 1, A, B, M, M + extra, int(mirror)))
    p.insert_into(d)
    eng = capi.Engine(0, [d], [])
    exp = check(eng, p.reads, [d], [], "certificate, sparse")
    BP.fixture_holds(p, exp[:, 0], "certificate, sparse")
    # what the certificate pass counts for the trailing strand's planted bin, by hand: the planted hits, and now and then a chance bit
    # of hash 0 (the bin's column holds ~90 bits in 131 071 blocks; every other bin stays at a handful)
    view, host = BP.oracle_view(d)
    upper = {}
    for i, A, B, M, T, lead in cases:
        upper[i] = hash0_upper(view, host, p.reads[i], 1 - lead, A if lead else B)
        assert T <= upper[i] <= T + 3, ("fixture", i, T, upper[i])
    assert sum(upper[i] == M for i, _, _, M, _, _ in cases) >= 4, "no case with the trailing upper bound EQUAL to the leader's maximum"
    assert sum(upper[i] == M + 1 for i, _, _, M, _, _ in cases) >= 4, "no case with the trailing upper bound one ABOVE the leader's maximum"
    buf, offs, lens = H.pack_reads(p.reads)
    tr = Trace(eng, len(p.reads))
    try:
        eng.set_prune_parts(7)
        eng.classify(buf, offs, lens)
        t = tr.take()
        n = lens.astype(np.int64) - K + 1
        for i, A, B, M, T, lead in cases:
            rec = {k: int(v[i]) for k, v in t.items()}
            assert rec["lead"] == lead and rec["tried"] == 1, (i, rec)
            trailing_stop = rec["stop_fwd"] if lead else rec["stop_rev"]
            if upper[i] <= M:
                assert rec["held"] == 1 and trailing_stop == TILE, (i, M, T, rec)  # certified: no full gather behind the probe
            else:
                assert rec["held"] == 0 and trailing_stop > TILE, (i, M, T, rec)   # attempted, failed, counted in full
            assert exp[i, 0] == max(M, T)
        for mask in (LEAD, LEAD | SUB, CERT, CERT | SUB):  # without the certificate bit (or without the lead it builds on): no attempt
            eng.set_prune_parts(mask)
            eng.classify(buf, offs, lens)
            assert not tr.take()["tried"].any(), mask
    finally:
        tr.close()
        eng.set_prune_parts(7)


def test_certificate_dense():
    import torch  # noqa: F401
    from readbouncer_amd import synth
    d = BP.make_filter(8192, n_blocks=32749, fill_seed=5)  # the bench's bit density (rbspec::synth_word)
    planted, starts, ends = synth.planted_reference(17, n_segments=512)
    d.insert(planted, starts, ends, (np.arange(512, dtype=np.uint64) * np.uint64(7919)) % np.uint64(8192))
    eng = capi.Engine(0, [d], [])
    buf, offs, lens = synth.make_reads(1, 3000, 360, planted, positive_fraction=0.5)
    lens = np.random.default_rng(1).integers(K - 1, 361, size=len(lens)).astype(np.uint32)  # mixed lengths (the offsets stay)
    batch = (buf, offs, lens)
    n = np.maximum(lens.astype(np.int64) - K + 1, 0)
    rem = n - TILE
    tr = Trace(eng, len(lens))
    try:
        # always attempt: every read with a trailing strand to continue tries; the negatives all fail; results stay exact
        oracle = oracle_results(batch, [d], [])
        eng.set_cert_load(0, 0.0)
        exp = check(eng, batch, [d], [], "certificate, dense, always", repeats=2, ref=oracle)[:, 0].astype(np.int64)
        eng.classify(*batch)
        t = tr.take()
        eligible = (n > TILE) & (exp < n)
        assert np.array_equal(t["tried"], eligible.astype(np.int64))
        # hash 0 alone gives some bin about 0.215 rem + 3.8 sigma: far above a maximum of 0.1 n + 5 once rem >= 128
        negative = eligible & (rem >= 128) & (exp <= 0.1 * n + 5)
        assert negative.sum() > 300 and not t["held"][negative].any()
        assert t["held"].sum() > 300  # ... and the strong positives hold
        # the default: the engine measures the load of the FULLEST bin, so that the allowance covers every bin.  This filter is
        # unevenly loaded -- its 512 planted bins carry 2000 k-mers each on top of the fill, 6000 more bits in 32 749 blocks: 0.35
        # against a mean of 0.22 (an allowance made for the mean fails on 110 of 839 attempts here: a planted bin that is not the
        # read's own passes it).  Attempts only on strong positives, none on a negative, and NONE fails: a lost z term or a wrong
        # denominator in the allowance would show as failures among the 512 full bins or as attempts gone missing.
        loads = d.bin_occupancy().astype(np.float64) / 32749.0
        assert 0.21 < loads.mean() < 0.24 and 0.33 < loads.max() < 0.38
        eng.set_cert_load(0, -1.0)
        check(eng, batch, [d], [], "certificate, dense, measured", repeats=2, ref=oracle)
        eng.classify(*batch)
        t = tr.take()
        tried = t["tried"] == 1
        failed = tried & (t["held"] == 0)
        print("bin load: mean %.4f, max %.4f; measured load: %d attempts, %d failed" % (loads.mean(), loads.max(), tried.sum(), failed.sum()))
        assert tried.sum() > 300 and not tried[~eligible].any() and not tried[negative].any()
        assert (exp[tried] >= loads.max() * rem[tried]).all(), "an attempt on a read whose maximum is below the expected hash-0 count"
        assert not failed.any(), ("failed attempts", int(failed.sum()), np.nonzero(failed)[0][:8].tolist())
        # the same load given by hand picks the same attempts
        eng.set_cert_load(0, float(loads.max()))
        eng.classify(*batch)
        assert np.array_equal(tr.take()["tried"] == 1, tried)
        # never
        eng.set_cert_load(0, 1.0)
        check(eng, batch, [d], [], "certificate, dense, never", masks=(7,), repeats=1, ref=oracle)
        eng.classify(*batch)
        assert not tr.take()["tried"].any()
    finally:
        tr.close()
        eng.set_cert_load(0, -1.0)
        eng.set_prune_parts(7)


@pytest.mark.parametrize("n_rule", (3, 4))
def test_shapes_slices_two_filters_n_rules(n_rule):
    prev = po.set_revcomp_of_n(n_rule)
    try:
        bins = 8192 + 2048 + 37  # 161 word columns: a slice of 128 and one of 33, the last word partial
        wide = BP.make_filter(bins)
        plant = BP.tight_plant(bins, 402, kmers=(65, 73, 348))
        lo = BP.tight_plant(bins, 403, kmers=(72, 348))  # the same shapes with both bins in the second slice
        for b in range(len(lo.bins)):
            lo.bins[b] = 8192 + (lo.bins[b] % (bins - 8192))
        plant.insert_into(wide)
        lo.insert_into(wide)
        narrow = BP.make_filter(8192)
        tp = lead_plant(404)
        tp.insert_into(narrow)
        eng = capi.Engine(0, [wide], [narrow])  # config 4's shape: a deplete and a target filter in one call
        eng.set_revcomp_of_n(n_rule)
        rng = np.random.default_rng(40 + n_rule)
        with_n = []
        for r in (plant.reads + tp.reads)[::4]:  # N bases (under rule 3 their reverse-strand k-mers hit, under rule 4 they miss)
            a = np.frombuffer(r.encode(), dtype=np.uint8).copy()
            a[rng.random(len(a)) < 0.01] = ord("N")
            with_n.append(a.tobytes().decode())
        reads = plant.reads + tp.reads + lo.reads + with_n
        exp = check(eng, reads, [wide], [narrow], "slices + two filters N%d" % n_rule)
        BP.fixture_holds(plant, exp[:, 0], "W=161")
        BP.fixture_holds(tp, exp[len(plant.reads):, 1], "W=128 target")
        # the trace of two filters: the wide one's records first, [read][slice], then the narrow one's
        import torch  # noqa: F401
        slices = [eng.plan(fi, len(reads), max(len(r) for r in reads))["column_slices"] for fi in (0, 1)]
        assert slices == [2, 1]
        tr = Trace(eng, len(reads) * 3)
        try:
            buf, offs, lens = H.pack_reads(reads)
            eng.classify(buf, offs, lens)
            t = tr.take()
            assert t["written"].all()
            lead_narrow = t["lead"][2 * len(reads):]
            for i, lead in enumerate(tp.lead):
                if lead is not None:
                    assert lead_narrow[len(plant.reads) + i] == lead, (i, lead)
        finally:
            tr.close()
    finally:
        po.set_revcomp_of_n(prev)


def test_shapes_column_shards():
    """two ranks of a column-sharded engine: each rank's partial maxima are the same under every mask as with pruning off, and
    their element-wise maximum is the oracle's"""
    import torch
    d = BP.make_filter(8192)
    plant = lead_plant(411)
    tight = BP.tight_plant(8192, 412, kmers=(73, 348))
    for b in range(len(tight.bins)):
        while tight.bins[b] in plant.used:
            tight.bins[b] = (tight.bins[b] + 1) % 8192
        plant.used.add(tight.bins[b])
    plant.insert_into(d)
    tight.insert_into(d)
    reads = plant.reads + tight.reads
    buf, offs, lens = H.pack_reads(reads)
    view, host = BP.oracle_view(d)  # (the view reads the download's memory: both stay)
    exp = po.batch_raw_max(view, buf, offs, lens, BP.ORACLE_THREADS)
    del view, host
    assert np.array_equal(exp[:len(plant.want)], np.array(plant.want, dtype=exp.dtype))
    dev = torch.device("cuda:0")
    t_seq, t_off, t_len = torch.from_numpy(buf).to(dev), torch.from_numpy(offs.view(np.int64)).to(dev), torch.from_numpy(lens.view(np.int32)).to(dev)
    n = len(reads)
    eng = capi.Engine(0, [d], [])
    eng.set_split_threshold(0)

    def partial(rank):
        eng.set_column_shard(rank, 2)
        t_part = torch.zeros((n, 1), dtype=torch.int16, device=dev)
        torch.cuda.synchronize()
        eng.classify_device(t_seq.data_ptr(), t_off.data_ptr(), t_len.data_ptr(), n, int(lens.max()), d_maxcount=t_part.data_ptr())
        torch.cuda.synchronize()
        return t_part.cpu().numpy().view(np.uint16)[:, 0].copy()

    try:
        eng.set_bound_pruning(0)
        off = [partial(r) for r in (0, 1)]
        assert np.array_equal(np.maximum(off[0], off[1]), exp)
        eng.set_bound_pruning(1)
        for mask in ALL_MASKS:
            eng.set_prune_parts(mask)
            for rep in range(2):
                for r in (0, 1):
                    assert np.array_equal(partial(r), off[r]), (mask, rep, r)
    finally:
        eng.set_column_shard(0, 1)
        eng.set_prune_parts(7)

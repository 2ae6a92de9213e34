"""Bound pruning of the plain count kernel (rb_kernels.hip, count_strand): a lane stops gathering once none of its bins can reach the
read's maximum any more (count + k-mers still to come <= the best count seen on either strand).  The maxima must stay exact, so every
batch here is compared bit for bit -- raw maxima, decisions, status -- with the oracle and with pruning switched off
(rb_engine_set_bound_pruning).

The fixtures make the bound tight: a read whose first a k-mers sit in bin A and whose last n - a sit in bin B (B ends one above A, and
an off-by-one in the k-mers still to come prunes B one k-mer early), with A and B in one lane's 16-byte column, in two lanes of one
128-byte line and in different lines; the best strand forward in some reads and reverse in others; ties between the strands; a strand
whose best is beaten by ONE on the other strand; whole reads in one bin (the second strand is skipped).  Read lengths put n at the
macro-tile edges (63, 64, 65, 128 k-mers), at 360 bp (348) and at the top of the ten counter planes (1023); a batch with longer reads
takes the sixteen-plane build.  Filters of 128 word columns (one column slice) and of 161 (two slices, bins in the partial last word),
both N rules, two filters in one engine (config 4's shape), a seeded fuzz over the bench's read mix on a filter filled at the bench's
bit density, and repeated launches whose outputs must not change."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import pyoracle as po
from readbouncer_amd import capi
from tests import helpers as H

K = 13
ORACLE_THREADS = 16
N_BLOCKS = 131071  # 128 MiB at 128 word columns: sparse enough that a read's chance hits in a bin it was not put into stay at 0
KMERS = (63, 64, 65, 128, 348, 401, 1023)
_COMP = str.maketrans("ACGTN", "TGCAN")


def rc(s):
    return s.translate(_COMP)[::-1]


class Plant:
    """reads + the sequences inserted for them (sequence -> bin) + the maximum each read was built for"""

    def __init__(self, n_bins, seed, k=K):
        self.n_bins = n_bins
        self.k = k
        self.rng = np.random.default_rng(seed)
        self.used = set()
        self.items, self.bins = [], []
        self.reads, self.want = [], []

    def fresh(self, lane=None, line=None, lo=0):
        """an unused bin (optionally inside a given 128-bin lane column or 1024-bin line)"""
        for _ in range(10000):
            if lane is not None:
                b = lane * 128 + int(self.rng.integers(0, 128))
            elif line is not None:
                b = line * 1024 + int(self.rng.integers(0, 1024))
            else:
                b = int(self.rng.integers(lo, self.n_bins))
            if b < self.n_bins and b not in self.used:
                self.used.add(b)
                return b
        raise AssertionError("no free bin")

    def put(self, seq, b):
        self.items.append(seq)
        self.bins.append(b)

    def read(self, r, want):
        self.reads.append(r)
        self.want.append(want)

    def pair(self, where, lo=0):
        if where == "lane":
            c = int(self.rng.integers(0, min(64, self.n_bins // 128)))
            return self.fresh(lane=c), self.fresh(lane=c)
        if where == "line":
            line = int(self.rng.integers(0, max(1, min(8, self.n_bins // 1024))))
            a = self.fresh(line=line)
            for _ in range(1000):
                b = self.fresh(line=line)
                if b // 128 != a // 128:
                    return a, b
                self.used.discard(b)
            raise AssertionError("no second lane")
        a = self.fresh(lo=lo)
        for _ in range(1000):
            b = self.fresh(lo=lo)
            if b // 1024 != a // 1024:
                return a, b
            self.used.discard(b)
        raise AssertionError("no second line")

    def split(self, n, a_kmers, where, reverse, lo=0):
        """first a_kmers k-mers of R into A, the rest into B; the engine sees R (forward best) or rc(R) (reverse best)"""
        R = H.random_dna(self.rng, n + self.k - 1)
        A, B = self.pair(where, lo)
        self.put(R[:a_kmers + self.k - 1], A)
        self.put(R[a_kmers:], B)
        self.read(rc(R) if reverse else R, max(a_kmers, n - a_kmers))

    def strands(self, n, x, y, where):
        """x k-mers of the forward strand's start into A, y k-mers of the reverse strand's END into B: max(x, y)"""
        R = H.random_dna(self.rng, n + self.k - 1)
        A, B = self.pair(where)
        self.put(R[:x + self.k - 1], A)
        Q = rc(R)
        self.put(Q[len(Q) - (y + self.k - 1):], B)
        self.read(R, max(x, y))

    def whole(self, n, reverse):
        R = H.random_dna(self.rng, n + self.k - 1)
        self.put(R, self.fresh())
        self.read(rc(R) if reverse else R, n)

    def insert_into(self, d):
        starts = np.cumsum([0] + [len(s) for s in self.items[:-1]]).astype(np.uint64)
        ends = starts + np.array([len(s) for s in self.items], dtype=np.uint64)
        d.insert("".join(self.items), starts, ends, np.array(self.bins, dtype=np.uint64))


def tight_plant(n_bins, seed, kmers=KMERS, lo=0, k=K):
    p = Plant(n_bins, seed, k)
    for n in kmers:
        for where in ("lane", "line", "lines"):
            for reverse in (False, True):
                p.split(n, (n - 1) // 2, where, reverse, lo)        # B = A + 1 (n odd) or a tie inside the strand (n even)
                p.split(n, n - (n - 1) // 2, where, reverse, lo)    # the mirror: A, which comes first, is the larger
            p.strands(n, n // 3, n // 3 + 1, where)                 # the reverse strand wins by one
            p.strands(n, n // 3 + 1, n // 3, where)                 # the forward strand wins by one
            p.strands(n, n // 3, n // 3, where)                     # tie between the strands
        p.whole(n, False)
        p.whole(n, True)
    return p


def make_filter(bins, n_blocks=N_BLOCKS, fill_seed=None, k=K):
    W = (bins + 63) // 64
    d = capi.DeviceIBF.create(0, bins, 3, k, W * 64 * n_blocks)
    if fill_seed is not None:
        d.fill_synth(fill_seed)
    return d


def oracle_view(d):
    host = d.download()
    i = host.info
    return po.OracleIBF.wrap(i["n_bins"], i["n_hash"], i["kmer_size"], i["n_bits"], host.words()), host


def plain_form(eng, nf, max_len, n_reads):
    """the throughput form, plain kernel with 16-byte lanes, for every filter of the engine"""
    eng.set_split_threshold(0)
    for fi in range(nf):
        p = eng.plan(fi, n_reads, max_len)
        assert p["kernel"] == "ibf_count_max_kernel" and p["lanes_per_block_log2"] == 6 and p["words_per_lane"] == 2, p


def check(eng, reads_or_batch, deplete, target, label, repeats=1):
    buf, offs, lens = reads_or_batch if isinstance(reads_or_batch, tuple) else H.pack_reads(reads_or_batch)
    views = [oracle_view(d) for d in deplete + target]
    ov = [v for v, _ in views]
    exp = np.stack([po.batch_raw_max(v, buf, offs, lens, ORACLE_THREADS) for v in ov], axis=1)
    exp_dec, exp_st = po.batch_check_unblock(ov[:len(deplete)], ov[len(deplete):], buf, offs, lens, n_threads=ORACLE_THREADS)
    plain_form(eng, len(ov), int(lens.max()), len(lens))
    outs = {}
    for on in (0, 1):
        eng.set_bound_pruning(on)
        for rep in range(repeats if on else 1):
            mc, _, dec, st = eng.classify(buf, offs, lens)
            bad = np.nonzero((mc != exp).any(axis=1))[0]
            assert len(bad) == 0, (label, on, rep, [(int(i), int(lens[i]), mc[i].tolist(), exp[i].tolist()) for i in bad[:6]])
            assert np.array_equal(dec, exp_dec) and np.array_equal(st, exp_st), (label, on, rep, "decision/status")
            if on in outs:
                assert all(np.array_equal(a, b) for a, b in zip(outs[on], (mc, dec, st))), (label, "repeat differs", rep)
            outs[on] = (mc, dec, st)
    assert all(np.array_equal(a, b) for a, b in zip(outs[0], outs[1])), label
    eng.set_bound_pruning(1)
    return exp


def fixture_holds(plant, exp_col, label):
    """the reads came out at the maxima they were built for (chance hits did not move them)"""
    got = exp_col[:len(plant.want)]
    bad = [(i, len(plant.reads[i]), plant.want[i], int(got[i])) for i in range(len(plant.want)) if got[i] != plant.want[i]]
    assert not bad, (label, bad[:6])


@pytest.mark.parametrize("n_rule", (3, 4))
def test_tight_bound_one_slice(n_rule):
    prev = po.set_revcomp_of_n(n_rule)
    try:
        d = make_filter(8192)
        plant = tight_plant(8192, 105 + n_rule)
        plant.insert_into(d)
        eng = capi.Engine(0, [d], [])
        eng.set_revcomp_of_n(n_rule)
        # N bases: a copy of some reads with Ns sprinkled in (under rule 3 their reverse-strand k-mers hit, under rule 4 they miss)
        rng = np.random.default_rng(7 + n_rule)
        with_n = []
        for r in plant.reads[::5]:
            a = np.frombuffer(r.encode(), dtype=np.uint8).copy()
            a[rng.random(len(a)) < 0.01] = ord("N")
            with_n.append(a.tobytes().decode())
        short = [r for r in plant.reads + with_n if len(r) - K + 1 <= 1023]
        exp = check(eng, short, [d], [], "tight W=128 N%d" % n_rule, repeats=3)
        fixture_holds(plant, exp[:, 0], "tight W=128")
        # the same reads behind one of 1100 k-mers: the sixteen-plane build, whose bound is on below 65 536 k-mers
        long_read = plant.reads[0] + H.random_dna(rng, 1100)
        check(eng, short[:40] + [long_read], [d], [], "tight W=128 sixteen planes N%d" % n_rule)
    finally:
        po.set_revcomp_of_n(prev)


def test_tight_bound_column_slices_and_two_filters():
    bins = 8192 + 2048 + 37  # 161 word columns: a slice of 128 and one of 33, the last word partial
    wide = make_filter(bins)
    plant = tight_plant(bins, 202, kmers=(64, 65, 348, 401))
    lo = tight_plant(bins, 203, kmers=(65, 348))  # the same shapes with both bins in the second slice
    for b in range(len(lo.bins)):
        lo.bins[b] = 8192 + (lo.bins[b] % (bins - 8192))
    plant.insert_into(wide)
    lo.insert_into(wide)
    narrow = make_filter(8192)
    tp = tight_plant(8192, 204, kmers=(128, 348))
    tp.insert_into(narrow)
    eng = capi.Engine(0, [wide], [narrow])  # config 4's shape: a deplete and a target filter in one call
    reads = plant.reads + tp.reads + lo.reads
    exp = check(eng, reads, [wide], [narrow], "slices + two filters", repeats=2)
    fixture_holds(plant, exp[:, 0], "W=161")
    fixture_holds(tp, exp[len(plant.reads):, 1], "W=128 target")


def test_fuzz_bench_mix():
    from readbouncer_amd import synth
    d = make_filter(8192, n_blocks=32749, fill_seed=5)  # the bench's bit density (rbspec::synth_word)
    ref, starts, ends = synth.planted_reference(17, n_segments=512)
    d.insert(ref, starts, ends, (np.arange(512, dtype=np.uint64) * np.uint64(7919)) % np.uint64(8192))
    eng = capi.Engine(0, [d], [])
    for seed, pos in ((1, 0.5), (2, 1.0), (3, 0.0)):
        buf, offs, lens = synth.make_reads(seed, 3000, 360, ref, positive_fraction=pos)
        # mixed lengths: cut every read at a seeded length (the offsets stay)
        rng = np.random.default_rng(seed)
        lens = rng.integers(K - 1, 361, size=len(lens)).astype(np.uint32)
        check(eng, (buf, offs, lens), [d], [], "fuzz seed %d" % seed, repeats=2)

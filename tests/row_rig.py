"""Fixtures of the row-table tests beyond one filter and beyond k = 7 (tests/test_gpu_row_engines.py, test_gpu_row_table_wide_k.py,
test_gpu_row_pruning.py), kept apart from the tests so that what is a property of the FIXTURES -- the decisions and best targets the
five-filter rig covers, the ranks a wide-k batch reaches, the maxima the pruning plants were built for at k = 11 -- is asserted on the
oracle alone where there is no GPU (tests/test_row_engines_cpu.py).  Everything here is host arithmetic: the GPU tests build the same
filters on the device from the same specs and look at them through their downloaded bits."""
import numpy as np

from oracle import pyoracle as po
from tests import decide_cells as DC
from tests import helpers as H
from tests import pass_edges as PE
from tests import test_gpu_bound_pruning as BP
from tests import test_gpu_row_table as RT
from tests import test_gpu_strand_lead as SL

K = RT.K
N_BLOCKS = 1021
MODES = DC.MODES
# the error rate of every classify call on the rig: at k = 7 a filter at design load gives a random read of 354 bases a maximum of 150 - 180
# somewhere among its bins, above the threshold of the default rate (121 at r = 0.1).  At 0.05 the threshold is 200: random reads and
# reads with 20 % errors stay below it, reads with 5 % errors (290 - 315) pass
R = 0.05


def rc(s):
    return PE.revcomp_str(s)


# ---------------------------------------------------------------- part 1: five filters in one engine
class Rig:
    """a deplete filter and four targets at design load (fill_synth) with planted stretches:
         D   8192 bins  two words per lane            row table
         T0  4096 bins  one word per lane             row table   (k = t0_k: 7, or 5 for the per-filter auto rule)
         T1  8200 bins  two column slices             row table, counted into the engine's per-slice buffer and reduced
         T2   300 bins  narrow                        never a row table
         T3  4096 bins  h = 4 (run-time hash count)   no row build
       `both` lies in D and T0 (a read of it hits deplete and target: wait), `tie` in T0 and T1 (equal maxima: the first target wins)"""
    NAMES = ("D", "T0", "T1", "T2", "T3")
    ROW_FILTERS = (0, 1, 2)

    CHUNK = 360  # bases per planted stretch: 354 k-mers, a load of 0.64 in a bin's column of 1021 blocks (a random read stays below its threshold)

    def __init__(self, t0_k=K):
        rng = np.random.default_rng(4107)
        self.ref = {name: H.random_dna(rng, 8 * self.CHUNK) for name in self.NAMES}
        self.both = H.random_dna(rng, self.CHUNK)
        self.tie = H.random_dna(rng, self.CHUNK)
        bins_of = {"D": 8192, "T0": 4096, "T1": 8200, "T2": 300, "T3": 4096}

        def stretches(name):  # every stretch in a bin of its own, the last one in the filter's last bin
            n = bins_of[name]
            return [(self.chunk(name, i), n - 1 if i == 7 else 3 + i * (n // 8)) for i in range(8)]

        # (name, bins, h, k, fill seed, [(sequence, bin)])
        self.specs = (
            ("D", 8192, 3, K, 31, stretches("D") + [(self.both, 77)]),
            ("T0", 4096, 3, t0_k, 32, stretches("T0") + [(self.both, 100), (self.tie, 200)]),
            ("T1", 8200, 3, K, 33, stretches("T1") + [(self.tie, 8195)]),  # (bins from 8192 on are the second column slice)
            ("T2", 300, 3, K, 34, stretches("T2")),
            ("T3", 4096, 4, K, 35, stretches("T3")),
        )

    def chunk(self, name, i):
        return self.ref[name][i * self.CHUNK:(i + 1) * self.CHUNK]

    @staticmethod
    def n_bits(bins):
        return ((bins + 63) // 64) * 64 * N_BLOCKS

    def oracle_filters(self):
        """the rig's filters built by the oracle itself (no GPU): same fill, same inserts"""
        out = []
        for _, bins, h, k, seed, plant in self.specs:
            o = po.OracleIBF(bins, h, k, self.n_bits(bins))
            o.fill_synth(seed)
            for seq, b in plant:
                o.insert(po.encode(seq), b)
            out.append(o)
        return out

    def reads(self, lens, seed=1):
        """read_shapes' kinds on the deplete reference, then per length reads planted in each target (best_target 0..3), in deplete and
        target at once, and in two row-counted targets with equal maxima.  A read of up to 354 bases lies inside one stretch (one bin
        holds it); a longer one runs over several bins and stays below its threshold everywhere: it is there for the sixteen planes"""
        rng = np.random.default_rng(seed)
        reads, self.tie_reads = [], []
        for L in lens:
            inside = L <= self.CHUNK - 6
            c = int(rng.integers(0, 8))
            reads += RT.read_shapes(rng, self.chunk("D", c) if inside else self.ref["D"], (L,))
            for name in ("T0", "T1", "T2", "T3"):
                src = self.chunk(name, int(rng.integers(0, 8))) if inside else self.ref[name]
                s = int(rng.integers(0, len(src) - L))
                reads += [H.mutate(rng, src[s:s + L], 0.05), rc(H.mutate(rng, src[s:s + L], 0.05))]
            if inside:
                s = int(rng.integers(0, self.CHUNK - L))
                reads += [self.both[s:s + L], rc(self.both[s:s + L])]
                self.tie_reads += [len(reads), len(reads) + 1]
                reads += [self.tie[s:s + L], rc(self.tie[s:s + L])]
        return reads


def oracle_reference(views, reads, batch, n_rule, mode, r=R):
    """-> (raw maxima [n, filters], best_target, decision, status) of the oracle; views[0] is the deplete filter"""
    prev = po.set_revcomp_of_n(n_rule)
    try:
        raw = DC.oracle_raw(views, *batch)
        dec, st, best = DC.oracle_expect(views[:1], views[1:], reads, [po.encode(x) for x in reads], *batch, r, mode)
    finally:
        po.set_revcomp_of_n(prev)
    return raw, best, dec, st


def rig_covers(rig, reads, ref_by_mode):
    """what the rig was built for, on the oracle's answer: every decision of check_unblock, every best_target from -1 to 3, and a tie
    between the two row-counted targets that the first one wins"""
    raw, best, dec, st = ref_by_mode[DC.MODE_CHECK_UNBLOCK]
    assert set(dec.tolist()) == {0, 1, 2}, np.bincount(dec, minlength=3).tolist()
    assert set(best.tolist()) == {-1, 0, 1, 2, 3}, sorted(set(best.tolist()))
    ties = [i for i in rig.tie_reads if raw[i, 1] == raw[i, 2] and raw[i, 1] == len(reads[i]) - K + 1 > 0 and best[i] == 0]
    assert len(ties) >= 2, (rig.tie_reads, raw[rig.tie_reads].tolist(), best[rig.tie_reads].tolist())
    assert ((best == 1) & (raw[:, 2] > raw[:, 1]) & (raw[:, 1] > 0)).any()  # the second target beats a non-zero first one
    for mode in (DC.MODE_CLASSIFY_CHUNK, DC.MODE_CLASSIFY_ANY):
        assert set(ref_by_mode[mode][2].tolist()) == {0, 1}, mode


def rule_b_need(k, h, max_len):
    """the smallest batch the auto mode builds a table for: items x 2 x k-mers x (h - 1) >= 4^k x (h + 1)"""
    kmers = max_len - k + 1
    return -(-(4 ** k * (h + 1)) // (2 * kmers * (h - 1)))


# ---------------------------------------------------------------- part 2: the table at k = 12 and 13
WIDE_CASES = ((12, 4096), (13, 4096), (13, 8192))  # 8, 32 and 64 GiB of rows
WIDE_L = 354
SEG_KMERS = 100  # k-mers per planted stretch: 300 bits in a bin's 1021-block column, a load of 0.25 on top of the fill


class WideCase:
    """one filter of 1021 blocks at design load; a reference of 30 stretches of 100 k-mers, every stretch in a bin of its own and its
    reverse complement in the next one (a bin of 1021 blocks that took the whole reference would be saturated: every read would count
    all its k-mers there, whatever row it gathered); "A" * L and "T" * L in a bin each.  The batch: a read per stretch and strand with
    5 % errors, random reads, reads with N (the three-hash twin), the all-A and all-T reads (ranks 0 and 4^k - 1 on both strands)."""

    def __init__(self, k, n_bins):
        self.k, self.n_bins = k, n_bins
        rng = np.random.default_rng(1000 * k + n_bins)
        seg_len = SEG_KMERS + k - 1
        self.ref = H.random_dna(rng, 30 * seg_len)
        self.segs = [self.ref[i * seg_len:(i + 1) * seg_len] for i in range(30)]
        step = (n_bins - 4) // 30
        self.plant = []
        for i, s in enumerate(self.segs):
            self.plant += [(s, i * step), (rc(s), i * step + 1)]
        self.plant[-2] = (self.segs[-1], n_bins - 2)  # ... the last pair in the last bins of the block
        self.plant[-1] = (rc(self.segs[-1]), n_bins - 1)
        self.bin_a, self.bin_t = step // 2, n_bins // 2 + step // 2 + 7
        assert not {self.bin_a, self.bin_t} & {b for _, b in self.plant}
        self.plant += [("A" * WIDE_L, self.bin_a), ("T" * WIDE_L, self.bin_t)]
        self.reads, self.planted = [], []  # planted[i]: (k-mers of read i that are k-mers of its stretch, in order) or None
        for s in self.segs:
            for q in (s, rc(s)):
                r = H.mutate(rng, q, 0.05)
                self.reads.append(r)
                self.planted.append(sum(r[p:p + k] == q[p:p + k] for p in range(SEG_KMERS)))
        n_planted = len(self.reads)
        self.reads += [H.random_dna(rng, seg_len if i < 12 else WIDE_L) for i in range(24)]
        with_n = []
        for i in range(0, n_planted, 6):
            a = np.frombuffer(self.reads[i].encode(), dtype=np.uint8).copy()
            a[int(rng.integers(0, len(a)))] = ord("N")
            with_n.append(a.tobytes().decode())
        self.reads += with_n + [H.random_dna(rng, WIDE_L, with_n=0.02) for _ in range(4)]
        self.all_a, self.all_t = len(self.reads), len(self.reads) + 1
        self.reads += ["A" * WIDE_L, "T" * WIDE_L]
        self.planted += [None] * (len(self.reads) - n_planted)
        self.random = range(n_planted, n_planted + 12)  # (the random reads of a planted read's length: its noise floor)

    def n_bits(self):
        return ((self.n_bins + 63) // 64) * 64 * N_BLOCKS

    def oracle_filter(self, seed=7):
        o = po.OracleIBF(self.n_bins, 3, self.k, self.n_bits())
        o.fill_synth(seed)
        for seq, b in self.plant:
            o.insert(po.encode(seq), b)
        return o

    def ranks(self):
        """base-4 ranks (first base most significant) of the k-mers of the N-free reads, both strands: the rows the batch gathers"""
        k, out = self.k, []
        code = np.full(256, -1, dtype=np.int64)
        for i, c in enumerate(b"ACGT"):
            code[c] = i
        weights = 4 ** np.arange(k - 1, -1, -1, dtype=np.int64)
        for r in self.reads:
            if len(r) < k or set(r) - set("ACGT"):
                continue
            for s in (r, rc(r)):
                d = code[np.frombuffer(s.encode(), dtype=np.uint8)]
                out.append(np.lib.stride_tricks.sliding_window_view(d, k) @ weights)
        return np.unique(np.concatenate(out))

    def ranks_cover(self):
        k, ranks = self.k, self.ranks()
        assert ranks[0] == 0 and ranks[-1] == 4 ** k - 1
        quarter = 4 ** k // 4
        assert all(((ranks >= q * quarter) & (ranks < (q + 1) * quarter)).any() for q in range(4))
        if k == 12:  # the builder's first 2^22 waves take a row each; the rows from 2^22 on are the strided loop's
            assert (ranks < 2 ** 22).any() and (ranks >= 2 ** 22).any()
        # what only the sizes reach: a gathered row whose byte / word offset is beyond 32 bits
        return int(ranks[-2])

    def fixture_holds(self, raw):
        """on the oracle's maxima: a planted read counts at least the k-mers it kept, far above what a random read reaches in any bin --
        a wrong row drops it to that floor; the all-A and all-T reads count every k-mer"""
        floor = int(max(raw[i] for i in self.random))
        for i, kept in enumerate(self.planted):
            if kept is not None:
                assert kept <= raw[i] <= kept + 12 and raw[i] >= floor + 10, (i, kept, int(raw[i]), floor)
        n = WIDE_L - self.k + 1
        assert raw[self.all_a] == n and raw[self.all_t] == n
        return floor


# ---------------------------------------------------------------- part 3: the pruning fixtures at k = 11
PRUNE_K = 11
PRUNE_SEEDS = {"cross": 301, "edges": 307, "lead": 311}  # seeds at which fixture_holds at k = 11 (302 - 306 repeat a k-mer across a crossover)


def pruning_plants(k=PRUNE_K, seeds=None):
    """the sub-tile crossovers, the tile-edge lengths of BP.KMERS and the lead fixtures on ONE sparse filter of 8192 bins: the three
    plants keep their bins apart (a later plant takes what the earlier ones left)"""
    seeds = seeds or PRUNE_SEEDS
    cross = SL.sub_tile_plant(seeds["cross"], k=k)
    edges = BP.tight_plant(8192, seeds["edges"], kmers=BP.KMERS, k=k)
    lead = SL.lead_plant(seeds["lead"], k=k)
    used = set(cross.used)
    for plant in (edges, lead):
        moved = {}  # (a bin may hold several stretches of one read: they move together)
        for b in sorted(set(plant.bins)):
            to = b
            while to in used:
                to = (to + 1) % 8192
            used.add(to)
            moved[b] = to
        plant.bins = [moved[b] for b in plant.bins]
    return {"cross": cross, "edges": edges, "lead": lead}


def pruning_oracle_filter(plants, k=PRUNE_K):
    o = po.OracleIBF(8192, 3, k, 128 * 64 * BP.N_BLOCKS)
    for plant in plants.values():
        for seq, b in zip(plant.items, plant.bins):
            o.insert(po.encode(seq), b)
    return o

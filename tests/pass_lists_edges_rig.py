"""Fixtures of tests/test_gpu_pass_lists_edges.py: the list forms of locate and hits (rb_pass_lists.hip) at the top of their 16-bit LDS
counters.  A counter dword holds an even bin in its low half and the next odd bin in its high half, and a strand may have 65 535 k-mers
(rblist::kMaxKmers), so a bin whose bit is set in every block counts a strand's every k-mer and reaches 0xFFFF on the longest strand the
list form serves: one k-mer more and a low half would carry into its neighbour's bin.  On top of SR.random_fill at SR.LOADS' load -- the
census still picks the geometry's slot size -- bits are written into the block columns the way tests/pass_edges.py writes them:
  PAIR      n_bins - 2 and n_bins - 1 in every block: both halves of the last counter dword, 0xFFFFFFFF at 65 535 k-mers.  At an odd bin
            count (PL.OddBins.N_BINS) the last bin alone: it is even and the high half of its dword is a pad counter, which must stay 0 and
            must never be reported;
  EVEN_SAT  an even bin in the middle of a scan piece, in every block, and its odd neighbour EVEN_SAT + 1 at load 0.99: a low half at n
            beside a high half near 0.97 n;
  LOW_EVEN  an even bin at load 0.5, far from the others.
Reads are prefixes of PE.sequence().  With 1021 blocks about three rows in a thousand are the AND of two blocks only, so a strand of
65 535 k-mers passes swapped halves and overflow slots while its counters are near the top.  MixedK is the fixture of engines whose
list-served filters differ in k.  Host arithmetic on the oracle's words only: the GPU tests upload the same words, and
tests/test_pass_lists_edges_cpu.py asserts on the oracle alone that the fixtures are what they claim."""
import numpy as np

from oracle import pyoracle as po
from tests import helpers as H
from tests import list_scan_rig as SR
from tests import pass_edges as PE
from tests import pass_lists_rig as PL
from tests import row_lists_rig as LR

K = SR.K
MAX_KMERS = 65535  # rblist::kMaxKmers
rc = LR.revcomp
EVEN_SAT, LOW_EVEN = 812, 1530  # piece 101 (lane 37's second piece), counter 4 of its eight; piece 191, counter 2
ODD = (PL.OddBins.N_BINS, PL.OddBins.LINES)
GEOMETRIES = ((2112, 1), (8192, 2), (8192, 4), ODD)
BIG = (32767, 32768, 65534, 65535)  # k-mers of the long reads
SHORT = SR.TAILS[2:7]               # 8, 9, 63, 64, 65


def load_of(n_bins, lines):
    return PL.OddBins.LOAD if (n_bins, lines) == ODD else SR.LOADS[(n_bins, lines)]


def pair_bins(n_bins):
    return (n_bins - 1,) if n_bins % 2 else (n_bins - 2, n_bins - 1)


def saturated_bins(n_bins):
    """the bins whose bit is set in every block, ascending"""
    return (EVEN_SAT,) + pair_bins(n_bins)


def planted_loads(n_bins):
    return [(b, 2.0) for b in pair_bins(n_bins)] + [(EVEN_SAT, 2.0), (EVEN_SAT + 1, 0.99), (LOW_EVEN, 0.5)]


def reads():
    S = PE.sequence()
    big = [S[:n + K - 1] for n in BIG]
    return big + [rc(big[-1])] + [S[:n + K - 1] for n in SHORT]


def over_read():
    """65 536 k-mers: one more than the list form serves"""
    return PE.sequence()[:MAX_KMERS + K]


class CachedCounts:
    """an oracle whose count() remembers the vectors of the strands it has seen (they are read-only): the long strands take a fraction of a
    second each, and every call of a test asks for the same ones"""

    def __init__(self, o):
        self._o, self._seen = o, {}

    def __getattr__(self, name):
        return getattr(self._o, name)

    def count(self, ords):
        key = bytes(memoryview(np.ascontiguousarray(ords)))
        if key not in self._seen:
            v = self._o.count(ords)
            v.setflags(write=False)
            self._seen[key] = v
        return self._seen[key]


class Edges:
    def __init__(self, n_bins, lines, words):
        self.n_bins, self.lines = n_bins, lines
        SR.random_fill(words, n_bins, SR.N_BLOCKS, load_of(n_bins, lines), seed=n_bins + lines)
        W = (n_bins + 63) // 64
        w = words[:SR.N_BLOCKS * W].reshape(SR.N_BLOCKS, W)
        rng = np.random.default_rng(n_bins * 16 + lines)
        for b, load in planted_loads(n_bins):
            assert b < n_bins
            w[:, b // 64] |= (rng.random(SR.N_BLOCKS) < load).astype(np.uint64) << np.uint64(b % 64)
        self.raw = SR.wrap(n_bins, words)
        self.o = CachedCounts(self.raw)
        self.sat = saturated_bins(n_bins)


# ------------------------------------------------------------------------------------------------ filters of different k in one engine
K5 = 5
K5_GEOMETRY = (8192, 1021, 0.15, 15, 4)  # n_bins, blocks, bit load, seed, lines: the k = 5 filter of tests/test_gpu_row_lists.py
K7_GEOMETRY = (2112, 1)
NARROW_BINS, NARROW_BLOCKS = 200, 1021
MIXED_LENGTHS = (4, 5, 6, 7, 8, 70)
BIN_5MERS, BIN_LONG = 4000, 77


class MixedK:
    """Reads of 4, 5, 6, 7, 8 and 70 bases and one of 70 with an N, for an engine of a k = 5 and a k = 7 list-served filter and a narrow
    k = 7 filter served plain.  The engine's largest k decides which items there are: the reads of 5 and 6 bases are too short for the
    ENGINE although the k = 5 filter could count them, and their 5-mers are planted there (bin BIN_5MERS) so that a kernel that counted
    them would report something.  The read of 70 is planted in BIN_LONG of every filter."""

    def __init__(self, words5, words7, narrow):
        n5, blocks5, load5, seed5, self.lines5 = K5_GEOMETRY
        n7, self.lines7 = K7_GEOMETRY
        SR.random_fill(words5, n5, blocks5, load5, seed5)
        SR.random_fill(words7, n7, SR.N_BLOCKS, SR.LOADS[K7_GEOMETRY], seed=n7 + self.lines7)
        self.o5 = po.OracleIBF.wrap(n5, LR.H_FUNCS, K5, SR.n_bits(n5, blocks5), words5)
        self.o7 = SR.wrap(n7, words7)
        self.narrow = narrow
        rng = np.random.default_rng(57)
        self.reads = [H.random_dna(rng, L) for L in MIXED_LENGTHS]
        long = self.reads[-1]
        self.reads.append(long[:33] + "N" + long[34:])
        for r in self.reads[1:3]:
            self.o5.insert(po.encode(r), BIN_5MERS)
        for o in (self.o5, self.o7, self.narrow):
            o.insert(po.encode(long), BIN_LONG)

    def filters(self):
        return [self.o5, self.o7, self.narrow]


def make_narrow():
    return po.OracleIBF(NARROW_BINS, LR.H_FUNCS, K, 64 * ((NARROW_BINS + 63) // 64) * NARROW_BLOCKS)


def strand_reads(k, seed=13):
    """strands of 1, 63, 64, 65 and 129 k-mers, the all-A and all-T reads (ranks 0 and 4^k - 1), and the reverse complements of all"""
    rng = np.random.default_rng(seed + k)
    out = [H.random_dna(rng, n + k - 1) for n in (1, 63, 64, 65, 129)] + ["A" * (k + 70), "T" * (k + 70)]
    return out + [rc(r) for r in out]

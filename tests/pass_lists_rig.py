"""Fixtures of tests/test_gpu_pass_lists.py: the list forms of locate and hits (rb_pass_lists.hip) scan a strand's 16-bit counters in 16-byte
pieces -- eight bins each, lane l at pieces l, l + 64, ..., 512 bins per round of the wave -- for the maximum, the lowest bin at it, the
bins at the threshold and the records.  The fixtures put ties across those seams and on either strand, find the read lengths whose
threshold is 0 or wraps, and mix the kinds of item the list kernels take and leave.  Host arithmetic on the oracle's words only: the GPU
tests upload the same words, and tests/test_pass_lists_cpu.py asserts on the oracle alone that the fixtures are what they claim."""
import numpy as np

from oracle import pyoracle as po
from tests import helpers as H
from tests import list_scan_rig as SR
from tests import row_lists_rig as LR

K = SR.K
R, CONF = 0.1, 0.95  # the error rate and significance of the other pass tests
rc = LR.revcomp
TIE_GEOMETRIES = ((2112, 1), (8192, 2))
N_KMERS = 150


def seam_pairs(n_bins):
    """two neighbouring bins on either side of a piece's edge, of a round's edge, and the last two bins"""
    return ((7, 8), (511, 512), (n_bins - 2, n_bins - 1))


class Ties:
    """SR's random fill at the geometry's load, and reads of N_KMERS k-mers planted so that the maximum -- every k-mer of the read -- is
    held by two places at once:
      pairs[i]   one read in both bins of seam_pairs()[i]: the lower bin, strand 0
      same       a read and its reverse complement in SAME: both strands reach the maximum in that bin: strand 0, and the bin is one
                 hit bin with two records
      rev_lower  the read in REV_LOWER[1], its reverse complement in REV_LOWER[0]: the reverse strand's bin is lower: that bin, strand 1
      fwd_lower  the read in FWD_LOWER[0], its reverse complement in FWD_LOWER[1]: the forward bin is lower: that bin, strand 0"""
    SAME, REV_LOWER, FWD_LOWER = 20, (300, 600), (100, 900)

    def __init__(self, n_bins, lines, words):
        self.n_bins, self.lines = n_bins, lines
        SR.random_fill(words, n_bins, SR.N_BLOCKS, SR.LOADS[(n_bins, lines)], seed=n_bins + lines)
        self.o = SR.wrap(n_bins, words)
        rng = np.random.default_rng(n_bins * 4 + lines)
        L = N_KMERS + K - 1
        self.pairs = [H.random_dna(rng, L) for _ in seam_pairs(n_bins)]
        for seq, (a, b) in zip(self.pairs, seam_pairs(n_bins)):
            self.o.insert(po.encode(seq), a)
            self.o.insert(po.encode(seq), b)
        self.same, self.rev_lower, self.fwd_lower = (H.random_dna(rng, L) for _ in range(3))
        self.o.insert(po.encode(self.same), self.SAME)
        self.o.insert(po.encode(rc(self.same)), self.SAME)
        self.o.insert(po.encode(self.rev_lower), self.REV_LOWER[1])
        self.o.insert(po.encode(rc(self.rev_lower)), self.REV_LOWER[0])
        self.o.insert(po.encode(self.fwd_lower), self.FWD_LOWER[0])
        self.o.insert(po.encode(rc(self.fwd_lower)), self.FWD_LOWER[1])

    def reads(self):
        return self.pairs + [rc(s) for s in self.pairs] + [self.same, self.rev_lower, self.fwd_lower]

    def want(self):
        """(best_bin, best_strand) per read of reads()"""
        low = [a for a, _ in seam_pairs(self.n_bins)]
        return [(b, 0) for b in low] + [(b, 1) for b in low] + [(self.SAME, 0), (self.REV_LOWER[0], 1), (self.FWD_LOWER[0], 0)]


class OddBins:
    """SR.Sparse's fill at an ODD bin count: the upper half of the last counter dword is a pad counter, and at t == 0 it must not count"""
    N_BINS, LINES, LOAD = 4091, 2, SR.LOADS[(4090, 2)]

    def __init__(self, words):
        self.n_bins, self.lines = self.N_BINS, self.LINES
        SR.random_fill(words, self.N_BINS, SR.N_BLOCKS, self.LOAD, seed=self.N_BINS + self.LINES)
        self.o = LR.silence(self.N_BINS, SR.N_BLOCKS, words, SR.n_bits(self.N_BINS))


def threshold_lengths(k=K, r=R, conf=CONF):
    """-> (lengths in k .. 400 whose threshold is 0, lengths whose threshold wraps to 65 5xx as a uint16_t)"""
    ts = {L: po.threshold(L, k, r, conf) for L in range(k, 401)}
    return [L for L, t in ts.items() if t == 0], [L for L, t in ts.items() if t > 60000]


def threshold_reads(seed=11):
    """a read at the shortest and the longest length of either kind (t == 0: every bin hits; a wrapped t: none), and one ordinary read"""
    zero, wrapped = threshold_lengths()
    rng = np.random.default_rng(seed)
    lens = ([zero[0], zero[-1]] if zero else []) + ([wrapped[0], wrapped[-1]] if wrapped else []) + [250]
    return [H.random_dna(rng, L) for L in lens], len(zero) and 2, len(wrapped) and 2


MAX_LEN = 260


def mixed_batch(seed=5):
    """-> (reads, kinds): the items the list kernels take ("free") between those they leave to the plain kernels -- an N at the first
    base, at the last base and in a middle tile ("n_first", "n_last", "n_mid"), a read shorter than k ("short") and one longer than
    MAX_LEN ("long")"""
    rng = np.random.default_rng(seed)

    def with_n(s, at):
        return s[:at] + "N" + s[at + 1:]

    free = [H.random_dna(rng, L) for L in (K, 70, 71, 200, MAX_LEN, 135)]
    reads = [(free[0], "free"), (with_n(H.random_dna(rng, 150), 0), "n_first"), (free[1], "free"), (with_n(H.random_dna(rng, 150), 149), "n_last"),
             (free[2], "free"), ("ACGT", "short"), (free[3], "free"), (with_n(H.random_dna(rng, 230), 100), "n_mid"), (free[4], "free"),
             (H.random_dna(rng, MAX_LEN + 40), "long"), (free[5], "free"), ("", "short")]
    return [r for r, _ in reads], [kind for _, kind in reads]

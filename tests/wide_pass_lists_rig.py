"""Fixtures of the wide forms of locate and hits (tests/test_gpu_wide_pass_lists.py) beyond tests/wide_lists_rig.py, which is imported
unchanged: the count fixtures with four more crafted k-mers whose rows TIE, and where a bin lies in the four waves' shares of the scan.
Host arithmetic only; what the fixtures claim of themselves is asserted on the oracle alone in tests/test_wide_pass_lists_cpu.py."""
import functools

import numpy as np

from oracle import pyoracle as po
from tests import wide_lists_rig as WR

K = WR.K
R, CONF = 0.1, 0.95
CAPS = (0, 1, 64)          # max_hits of the capped calls; "above the total" is computed per fixture
PIECE_BINS = 8             # a 16-byte piece of the counters
ROUND_BINS = 64 * PIECE_BINS  # a wave's round of the scan: 64 consecutive pieces


def cnt_dwords(n_bins):
    """rblist::count_cnt_dwords"""
    return ((n_bins + 1) // 2 + 255) & ~255


def share_of_bin(n_bins, b, waves=WR.WAVES):
    """which wave of ibf_locate_wide_lists_kernel / ibf_hits_wide_lists_kernel scans bin b: the counters are cnt_dwords / 256 rounds of
    512 bins, wave w takes the rounds [w per, (w + 1) per), per = ceil(rounds / waves)"""
    rounds = cnt_dwords(n_bins) // 256
    per = (rounds + waves - 1) // waves
    return (b // ROUND_BINS) // per


class PassFixture(WR.CountFixture):
    """WR.CountFixture (same numbers, so the same census verdict) and four k-mers more, each with its reverse complement, rewritten as
    the rig rewrites HOMOPOLYMER's blocks -- the three blocks of a k-mer to one row:
      two_waves:  the row {5, n_bins - 1}, two bins in different waves' shares; its reverse complement silent  -> bin 5, strand 0
      one_piece:  two bins of one 16-byte piece, {8 p + 2, 8 p + 6}; its reverse complement silent             -> 8 p + 2, strand 0
      same_bin:   the k-mer and its reverse complement list the same single bin: equal maxima at an equal bin   -> strand 0
      rev_lower:  the k-mer lists one bin, its reverse complement a lower one                                    -> the lower bin, strand 1
    A read of exactly the k-mer is one k-mer per strand: the maxima are 1 and tie."""

    def __init__(self, n_bins, load, seed, lines):
        super().__init__(n_bins, load, seed, lines)
        o, W = self.o, self.W
        w = o.words()[:WR.N_BLOCKS * W].reshape(WR.N_BLOCKS, W)
        used = {b for s in (WR.SILENT, WR.revcomp(WR.SILENT), WR.HOMOPOLYMER) + WR.CRAFTED for b in WR.blocks_of(o, s)}
        rng = np.random.default_rng(seed + 1000)
        picked = []
        while len(picked) < 4:
            s = WR.random_dna(rng, K)
            rc = WR.revcomp(s)
            blocks = WR.blocks_of(o, s) + WR.blocks_of(o, rc)
            if s == rc or len(set(blocks)) != 6 or set(blocks) & used or s in WR.CRAFTED:
                continue
            used |= set(blocks)
            picked.append(s)
        piece = (n_bins // 2) // PIECE_BINS
        self.same, self.hi, self.lo = 4242, n_bins - 3, 4100
        self.ties = dict(zip(("two_waves", "one_piece", "same_bin", "rev_lower"), picked))
        rows = {"two_waves": ([5, n_bins - 1], []), "one_piece": ([PIECE_BINS * piece + 2, PIECE_BINS * piece + 6], []),
                "same_bin": ([self.same], [self.same]), "rev_lower": ([self.hi], [self.lo])}
        self.tie_rows = rows
        for name, s in self.ties.items():
            for kmer, bins in zip((s, WR.revcomp(s)), rows[name]):
                bits = np.zeros(W * 64, dtype=np.uint8)
                bits[bins] = 1
                w[WR.blocks_of(o, kmer)] = np.packbits(bits, bitorder="little").view(np.uint64)
        self.tie_want = {"two_waves": (5, 0), "one_piece": (PIECE_BINS * piece + 2, 0), "same_bin": (self.same, 0), "rev_lower": (self.lo, 1)}

    def tie_reads(self):
        return [self.ties[name] for name in ("two_waves", "one_piece", "same_bin", "rev_lower")]

    def order_read(self):
        """cap + 1 random bins, an overflow slot, twenty times over: records across every wave boundary"""
        return WR.CRAFTED[0] * 20

    def left_reads(self):
        """items the wide form leaves, between items it takes: shorter than the engine's k, and empty"""
        seq = self.plants[0][0]
        return [seq[:90], "ACGT", seq[10:120], "", self.plants[-1][0], "A" * (K - 1), self.n_seq]


@functools.lru_cache(maxsize=None)
def pass_fixture(name):
    return PassFixture(*WR.COUNT_FIXTURES[name])


def threshold(length):
    return po.threshold(length, K, R, CONF)

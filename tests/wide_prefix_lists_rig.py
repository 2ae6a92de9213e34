"""Fixtures of tests/test_gpu_wide_prefix_lists.py: the wide list form of the prefix pass (rb_wide_prefix_lists.hip) counts the k-mers
between two checkpoints from a filter's wide list table with a workgroup of four waves -- tile t of the RANGE to wave t mod 4, wherever
the range begins --, then every wave scans its share of the 16-bit counters and the four maxima meet; lane p keeps checkpoint p's
maximum over the two strands; and it takes every item whose status so far is RB_OK within the call's bound, whatever its bases.  The
fixtures are tests/wide_pass_lists_rig.py's (the k = 7 count fixtures with the tie rows) with reads planted on top, whose maximum moves
between the waves' shares of the scan and between the strands from one checkpoint to the next; the read whose maxima rise one by one
across every seam is the rig's own run of C (HOMOPOLYMER counts bin 5 once per k-mer: a filter of 1 021 blocks holds no planted read of
a thousand k-mers without filling its bin in every block), beside a random read of the same length.  takes() is the take rule itself, written from the
header's words.  Host arithmetic on the oracle's words only: the GPU tests upload the same words, and
tests/test_wide_prefix_lists_cpu.py asserts on the oracle alone that the fixtures are what they claim."""
import functools

import numpy as np

from oracle import pyoracle as po
from tests import prefix_lists_rig as XL
from tests import wide_lists_rig as WR
from tests import wide_pass_lists_rig as WP

K = WR.K
R, CONF = WP.R, WP.CONF
rc = WR.revcomp
MAX_KMERS = 65535  # rbwide::kWideMaxKmers: the last checkpoint the wide form serves
share_of_bin = WP.share_of_bin


def bases(kmers):
    """the prefix length that holds `kmers` k-mers (0: one base short of the first)"""
    return kmers + K - 1


# ------------------------------------------------------------------------------------------------ 1. checkpoint seams
LONG_KMERS = 1450
# k-mers at the checkpoints: none (below k) and one (at k); one k-mer apart across the seam of a batch of 16 slots, of a tile (64) and of
# a round of four tiles (256); a range of 35 k-mers that starts off a multiple of 64 and is wave 0's alone (65 -> 100); ranges of two
# (100 -> 228, off a multiple of 64), four (257 -> 513), five (513 -> 833) and nine tiles (833 -> 1409); then two beyond the long read
SEAM_KMERS = (0, 1, 15, 16, 17, 63, 64, 65, 100, 228, 255, 256, 257, 513, 833, 1409)
SEAM_CHECKPOINTS = tuple(bases(n) for n in SEAM_KMERS) + (bases(LONG_KMERS) + 50, 3000)
ONE_CHECKPOINT = (bases(100),)
SIXTY_FOUR = XL.SIXTY_FOUR  # 6, 9, ... 195 bases: every lane holds a checkpoint, ranges of three k-mers


# ------------------------------------------------------------------------------------------------ 2. the maximum moves
# there and back: k-mers [0, 30) in A alone, [30, 80) in B alone, [80, 180) in A alone -> the maximum stands in A (30), in B (50), in A (130)
BACK = (30, 80, 180)
BACK_CHECKPOINTS = tuple(bases(n) for n in (10, 30, 31, 60, 61, 80, 100, 101, 180))
HEAD, TAIL_FROM, MOVE_KMERS = XL.HEAD, XL.TAIL_FROM, XL.MOVE_KMERS
MOVE_CHECKPOINTS = XL.MOVE_CHECKPOINTS


def move_pairs(n_bins):
    """(A, B), no bin twice (a bin of 1 021 blocks that holds several planted reads fills up): the first bin and one of the last piece
    (wave 0's share of the scan and wave 3's); 8191 and 8192, the list table's last bin and the first beyond it; both halves of the last
    counter dword -- at an odd bin count its high half is a pad counter, 8192 is the last bin, and the pairs are 8191 with bin 8 and the
    last bin with bin 9"""
    if n_bins % 2:
        return [(0, n_bins - 5), (8191, 8), (n_bins - 1, 9)]
    return [(0, n_bins - 5), (8191, 8192), (n_bins - 2, n_bins - 1)]


class PrefixFixture(WP.PassFixture):
    """WP.PassFixture, and on top of it -- inserted behind the rig's rewritten blocks, which are put back afterwards, so every row the
    earlier fixtures craft is what it was; the planted reads hold no k-mer that hashes into one of those blocks, so each of their k-mers
    counts where it was inserted --
      long         LONG_KMERS k-mers of C (not inserted: WR.HOMOPOLYMER's row is bin 5 alone): a prefix of n k-mers has the maximum n
      random_long  as many random k-mers, not inserted
      back[i]      per pair (A, B) of move_pairs(): the three stretches of BACK in A, B, A
      whole[i]     its first HEAD k-mers forward in A and its whole reverse complement in B (XL.Moves' reads)
      tail[i]      its first HEAD k-mers forward in A, the reverse complement of its k-mers from TAIL_FROM on in B"""

    def __init__(self, n_bins, load, seed, lines):
        super().__init__(n_bins, load, seed, lines)
        o, W = self.o, self.W
        w = o.words()[:WR.N_BLOCKS * W].reshape(WR.N_BLOCKS, W)
        named = [WR.SILENT, rc(WR.SILENT), WR.HOMOPOLYMER] + list(WR.CRAFTED)
        for s in self.ties.values():
            named += [s, rc(s)]
        kept = sorted({b for s in named for b in WR.blocks_of(o, s)})
        saved = w[kept].copy()
        self.kept_blocks = set(kept)
        # which k-mers hash into a kept block: by rank, once
        digits = lambda r: np.array([(r >> (2 * (K - 1 - i))) & 3 for i in range(K)], dtype=np.uint8)
        self._touches = np.array([any(o.block_index(po.kmer_value(digits(r), K), h) in self.kept_blocks for h in range(WR.H_FUNCS))
                                  for r in range(4 ** K)])
        rng = np.random.default_rng(seed + 2000)
        self.long = "C" * bases(LONG_KMERS)
        self.long_bin = 5
        self.random_long = WR.random_dna(rng, bases(LONG_KMERS))
        self.pairs = move_pairs(n_bins)
        self.back, self.whole, self.tail = [], [], []
        for a, b in self.pairs:
            z = self.clean_read(rng, bases(BACK[2]))
            o.insert(po.encode(z[:bases(BACK[0])]), a)
            o.insert(po.encode(z[BACK[0]:bases(BACK[1])]), b)
            o.insert(po.encode(z[BACK[1]:]), a)
            x, y = (self.clean_read(rng, bases(MOVE_KMERS), both=True) for _ in range(2))
            o.insert(po.encode(x[:bases(HEAD)]), a)
            o.insert(po.encode(rc(x)), b)
            o.insert(po.encode(y[:bases(HEAD)]), a)
            o.insert(po.encode(rc(y[TAIL_FROM:])), b)
            self.back.append(z)
            self.whole.append(x)
            self.tail.append(y)
        w[kept] = saved

    def clean_read(self, rng, length, both=False):
        """random bases, none of whose k-mers (both: nor their reverse complements) hashes into a kept block"""
        seq = []
        while len(seq) < length:
            seq.append(int(rng.integers(0, 4)))
            if len(seq) >= K:
                r = 0
                for d in seq[-K:]:
                    r = r * 4 + d
                bad = self._touches[r]
                if both and not bad:
                    q = 0
                    for d in reversed(seq[-K:]):
                        q = q * 4 + (3 - d)
                    bad = self._touches[q]
                if bad:
                    del seq[-(1 if rng.integers(0, 4) else 2):]  # another base there; now and then one further back, so no prefix holds it
        return "".join("ACGT"[d] for d in seq)

    def seam_reads(self):
        """the run of C, a random read of its length, their reverse complements, cuts that end inside a batch, a tile and a round, strands of 1 to 263 k-mers in
        steps of seven, and reads shorter than k and empty"""
        cuts = [self.random_long[:bases(n)] for n in (16, 64, 65, 256, 300, 1000)]
        return [self.long, rc(self.long), self.random_long, rc(self.random_long)] + cuts + self.length_reads()[::7] + ["ACGT", "", "A" * (K - 1)]

    def move_reads(self):
        return self.back + self.whole + self.tail

    # ---- N, flagged and overflow slots
    def n_checkpoint_reads(self):
        """WR's N reads: the N-carrying sequence (60 bases, N, 60 bases: its k-mers 54 .. 60 hold the N) and 150-base plants with an N at
        the first (k-mer 0), a middle (k-mers 69 .. 75) and the last base (k-mer 143), both strands; N alone"""
        return self.n_reads()

    def crafted_reads(self):
        """each CRAFTED k-mer as k-mer CRAFT_AT and as k-mer CRAFT_AT + 1 of a read: under CRAFT_CHECKPOINTS the last k-mer of one range
        and the first of the next; and the rig's own flagged reads"""
        rng = np.random.default_rng(self.rng_seed + 5)
        out = []
        for s in WR.CRAFTED:
            for p in (CRAFT_AT, CRAFT_AT + 1):
                out.append(WR.random_dna(rng, p) + s + WR.random_dna(rng, 60))
        return out + self.flagged_reads()


N_CHECKPOINTS = tuple(bases(n) for n in (1, 2, 54, 57, 58, 61, 62, 69, 72, 76, 77, 143, 144)) + (400,)
CRAFT_AT = 40
CRAFT_CHECKPOINTS = tuple(bases(n) for n in (20, CRAFT_AT + 1, 90)) + (600,)


@functools.lru_cache(maxsize=None)
def prefix_fixture(name):
    return PrefixFixture(*WR.COUNT_FIXTURES[name])


def strand_maxima(o, read, checkpoints):
    return XL.strand_maxima(o, read, checkpoints)


# ------------------------------------------------------------------------------------------------ 3. the counter's end
def edge_read():
    """65 535 k-mers of C: HOMOPOLYMER counts bin 5 once per k-mer"""
    return "C" * bases(MAX_KMERS)


EDGE_CHECKPOINTS = (bases(MAX_KMERS - 1), bases(MAX_KMERS))  # bin 5 stands at 0xFFFE, then at 0xFFFF
OVER_CHECKPOINTS = (bases(MAX_KMERS), bases(MAX_KMERS + 1))  # a last checkpoint of 65 536 k-mers: the plain form


# ------------------------------------------------------------------------------------------------ 4. who takes which item
C_LAST = XL.C_LAST
MIXED_CHECKPOINTS = XL.MIXED_CHECKPOINTS
ODD_START = XL.ODD_START
WIDE_BOUND, UNDERSTATED = XL.WIDE_BOUND, XL.UNDERSTATED
mixed_items = XL.mixed_items


def takes(read, c_last, chunk_start=0, max_len=None, chunk_length=0):
    """the take rule of rb_engine_set_wide_prefix_lists for one item: its status so far is RB_OK (the chunk begins within the read) and
    the w = min(bases the descriptor selects, c_last) bases the pass looks at lie within the call's bound min(max_len, c_last); any
    length, and whatever the bases are"""
    if chunk_start > len(read):
        return False
    body = read[chunk_start:chunk_start + chunk_length] if chunk_length else read[chunk_start:]
    w = min(len(body), c_last)
    return max_len is None or w <= min(max_len, c_last)


def taken_counts(reads, c_last, **kw):
    """-> (items the wide form takes, items it leaves)"""
    t = [takes(r, c_last, **kw) for r in reads]
    return sum(t), len(t) - sum(t)


def want_taken(kind, chunk_start, max_len):
    """what the rule says of each kind of XL.KINDS, spelled out: an N changes nothing"""
    if kind == "beyond":
        return chunk_start == 0  # (an empty read then)
    if kind in ("free_long", "n_at_last", "n_before_last"):
        return max_len >= C_LAST  # w = C_LAST
    if kind == "under":
        return max_len >= XL.UNDER_LEN
    return True

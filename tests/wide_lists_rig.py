"""Fixtures of the wide-list-table tests (tests/test_gpu_wide_lists.py), kept apart so that what is a property of the FIXTURES -- the
census verdicts, the bins the planted reads peak at, the populations of the crafted rows, the N-carrying k-mers that count -- is
asserted on the oracle alone where there is no GPU (tests/test_wide_lists_cpu.py).  Host arithmetic only: the GPU tests upload the same
words.  Filters of about a thousand blocks (a few MB), k = 5 and 7 (tables of 4^5 and 4^7 slots)."""
import functools

import numpy as np

from oracle import pyoracle as po

H_FUNCS = 3
N_BLOCKS = 1021
SENTINEL, OVERFLOW_MARK = 0xFFFF, 0xFFFE  # readbouncer_amd/csrc/rb_lists.h
WIDE_LINES = (4, 6, 8)                    # readbouncer_amd/csrc/rb_wide_lists.h: kWideLines
WAVES = 4                                 # ... kWideWaves: tile t of a strand goes to wave t mod 4

# With about a thousand blocks, three k-mers in a thousand have two equal block numbers among their three: their rows are the AND of two
# blocks (n d^2 bins, not n d^3) and, being far more than one row in 1024, THEY decide the census.  So the bit load d of a fixture is
# chosen for n d^2: name -> (n_bins, k, bit load, seed, slot size the census must choose; 0: refused for density)
FILTERS = {
    "b8193": (8193, 5, 0.15, 81, 4),      # 184 bins in a two-block row; W = 129, an odd bin count (the last bin is a low half)
    "b8256": (8256, 5, 0.20, 82, 6),      # 330: beyond four lines, within six; W = 129 full words, the first width beyond 128
    "b31000_4": (31000, 7, 0.080, 83, 4),  # 198; W = 485, odd
    "b31000_6": (31000, 7, 0.1016, 84, 6),  # 320
    "b31000_8": (31000, 5, 0.1191, 85, 8),  # 440
    "b32256": (32256, 5, 0.1168, 86, 8),  # 440; the last bin count that fits
    "dense": (31000, 5, 0.2, 87, 0),      # 1240: beyond eight lines
    "over": (31000, 7, 0.1255, 88, 8),    # 488, sigma 21: a few of the two-block rows pass 512 and take side rows
}


def revcomp(s):
    return s[::-1].translate(str.maketrans("ACGTN", "TGCAN"))


def random_dna(rng, n):
    return "".join("ACGT"[i] for i in rng.integers(0, 4, size=n))


def kmer_rank(s):
    r = 0
    for c in s:
        r = r * 4 + "ACGT".index(c)
    return r


def random_filter(n_bins, k, load, seed, n_blocks=N_BLOCKS):
    W = (n_bins + 63) // 64
    o = po.OracleIBF(n_bins, H_FUNCS, k, W * 64 * n_blocks)
    bits = np.random.default_rng(seed).random((n_blocks, W * 64)) < load
    bits[:, n_bins:] = False
    o.words()[:n_blocks * W].reshape(n_blocks, W)[:] = np.packbits(bits, axis=1, bitorder="little").view(np.uint64)
    return o


def blocks_of(o, kmer):
    return [o.block_index(po.kmer_value(po.encode(kmer), o.kmer_size), h) for h in range(H_FUNCS)]


def expected_rows(o):
    """-> uint64[4^k, W]: per N-free k-mer (row = base-4 rank, first base most significant) the AND of the oracle's h blocks"""
    k, W, n_blocks = o.kmer_size, o.bin_width, o.n_blocks
    blocks = o.words()[:n_blocks * W].reshape(n_blocks, W)
    r = np.arange(4 ** k)
    digits = np.stack([(r >> (2 * (k - 1 - i))) & 3 for i in range(k)], axis=1).astype(np.uint8)
    rows = np.full((4 ** k, W), ~np.uint64(0), dtype=np.uint64)
    for hash_no in range(H_FUNCS):
        idx = np.array([o.block_index(po.kmer_value(np.ascontiguousarray(digits[i]), k), hash_no) for i in range(4 ** k)], dtype=np.int64)
        rows &= blocks[idx]
    return rows


_POP8 = np.array([bin(i).count("1") for i in range(256)], dtype=np.uint8)


def populations(rows):
    """uint64[n, W] -> set bits per row"""
    return _POP8[np.ascontiguousarray(rows).view(np.uint8)].sum(axis=1, dtype=np.int64)


def census(pc):
    """rbwide::choose_lines on every row's population (4^k <= 65 536 rows: the census looks at all) -> (lines or 0, over[3])"""
    over = [int((pc > 64 * lines).sum()) for lines in WIDE_LINES]
    allowed = len(pc) >> 10
    return next((lines for lines, n in zip(WIDE_LINES, over) if n <= allowed), 0), over


def row_bits(rows, n_bins):
    """uint64[n, W] -> bool[n, n_bins]"""
    return np.unpackbits(np.ascontiguousarray(rows).view(np.uint8), axis=1, bitorder="little")[:, :n_bins].astype(bool)


def slots_match_rows(slots, side, rows, n_bins, chunk=1024):
    """the canonical table as rb_dibf_wide_list_table_download returns it against the expected dense rows, 1024 slots at a time (a
    bool matrix of all of them would be half a GB) -> bool[n]: which slots are overflow slots.  Asserts the layout on the way:
    ascending bins, then sentinels only; an overflow slot is the mark, two index entries and sentinels; every side row is used once."""
    n, cap = slots.shape
    over = slots[:, 0] == OVERFLOW_MARK
    idx_all = slots[over, 1].astype(np.int64) | (slots[over, 2].astype(np.int64) << 16)
    assert sorted(idx_all.tolist()) == list(range(len(side))), (sorted(idx_all.tolist())[:8], len(side))
    if len(side):
        assert (slots[over, 3:] == SENTINEL).all()
        assert not np.ascontiguousarray(side).view(np.uint8).reshape(len(side), -1)[:, (n_bins + 7) // 8:].any()  # pad words list nothing
    for lo in range(0, n, chunk):
        s, ov = slots[lo:lo + chunk], over[lo:lo + chunk]
        plain = ~ov
        listed = (s < OVERFLOW_MARK) & plain[:, None]
        assert not (s[plain] == OVERFLOW_MARK).any()
        lp, sp = listed[plain], s[plain].astype(np.int64)
        assert not (lp[:, 1:] & ~lp[:, :-1]).any()                # no bin behind a sentinel
        assert ((sp[:, 1:] > sp[:, :-1]) | ~lp[:, 1:]).all()      # ascending, so distinct
        assert (sp[lp] < n_bins).all()
        got = np.zeros((len(s), n_bins), dtype=bool)
        rr, cc = np.nonzero(listed)
        got[rr, s[rr, cc]] = True
        if ov.any():
            idx = s[ov, 1].astype(np.int64) | (s[ov, 2].astype(np.int64) << 16)
            got[ov] = row_bits(side[idx], n_bins)
        want = row_bits(rows[lo:lo + chunk], n_bins)
        bad = np.nonzero((got != want).any(axis=1))[0]
        assert len(bad) == 0, (lo, bad[:8].tolist())
    return over


# ---------------------------------------------------------------- the count fixture: planted reads, edges of the tile deal, crafted rows, N
K = 7
SILENT = "AAAAAAA"          # its blocks and its reverse complement's are cleared: a k-mer that counts nothing on either strand
HOMOPOLYMER = "CCCCCCC"     # inserted in bin 5 alone of its three blocks' own: a read of C counts bin 5 once per k-mer
CRAFTED = ("ACGTACG", "GATTACA", "CCGGTTA", "TGCATGC")


def best_bins(n_bins):
    """the bins the planted reads peak at: the first, the list table's last, the first two beyond it, both halves of the last counter
    dword in use (for an odd bin count its low half alone: the last bin) and the last bin"""
    last_dword = ((n_bins - 1) // 2) * 2
    return sorted({0, 8191, 8192, min(8193, n_bins - 1), last_dword, min(last_dword + 1, n_bins - 1), n_bins - 1})


class CountFixture:
    """A filter of n_bins bins, k = 7, at the bit load that makes the census choose `lines`, with
    - one 150-base sequence inserted per bin of best_bins(n_bins): a read of it peaks there with nearly every k-mer;
    - SILENT's blocks cleared, HOMOPOLYMER's rewritten to bin 5 alone;
    - the three blocks of each CRAFTED k-mer rewritten to one pattern: cap + 1 bins (an overflow slot), cap / 2 + 40 even bins (a row
      that fits, with swapped halves), cap / 2 + 40 odd bins, exactly cap bins;
    - a sequence with an N in its middle inserted in bin 77: its k-mers that hold the N are in the filter and count."""

    def __init__(self, n_bins, load, seed, lines):
        self.n_bins, self.lines, self.cap = n_bins, lines, 64 * lines
        rng = np.random.default_rng(seed)
        self.o = o = random_filter(n_bins, K, load, seed)
        W = self.W = o.bin_width
        w = o.words()[:N_BLOCKS * W].reshape(N_BLOCKS, W)
        self.plants = [(random_dna(rng, 150), b) for b in best_bins(n_bins)]
        left, right = random_dna(rng, 60), random_dna(rng, 60)
        self.n_seq, self.n_bin = left + "N" + right, 77
        for seq, b in self.plants:
            o.insert(po.encode(seq), b)
        o.insert(po.encode(self.n_seq), self.n_bin)
        # (the blocks below are rewritten behind the inserts, so their rows are exactly what is written here; a plant loses the few
        # k-mers that hash into one of them)
        named = {}
        for s in (SILENT, revcomp(SILENT), HOMOPOLYMER) + CRAFTED:
            named[s] = blocks_of(o, s)
        # no block shared between two of them (the k-mer of A alone has the value 0 and so block 0 three times)
        assert len({b for bs in named.values() for b in bs}) == sum(len(set(bs)) for bs in named.values()), named
        for s in (SILENT, revcomp(SILENT)):
            w[named[s]] = 0
        self.want = (self.cap + 1, self.cap // 2 + 40, self.cap // 2 + 40, self.cap)
        evens, odds = np.arange(0, n_bins, 2), np.arange(1, n_bins, 2)
        pools = (np.arange(n_bins), evens, odds, np.arange(n_bins))
        for s, m, pool in zip(CRAFTED, self.want, pools):
            bits = np.zeros(W * 64, dtype=np.uint8)
            bits[rng.choice(pool, size=m, replace=False)] = 1
            w[named[s]] = np.packbits(bits, bitorder="little").view(np.uint64)
        bits = np.zeros(W * 64, dtype=np.uint8)
        bits[5] = 1
        w[named[HOMOPOLYMER]] = np.packbits(bits, bitorder="little").view(np.uint64)
        self.ranks = [kmer_rank(s) for s in CRAFTED]
        self.rng_seed = seed

    def planted_reads(self):
        """per planted bin: the sequence, its reverse complement, a 100-base piece -> [(read, bin)]"""
        out = []
        for seq, b in self.plants:
            out += [(seq, b), (revcomp(seq), b), (seq[20:120], b)]
        return out

    def length_reads(self):
        """strands of every length from 1 to 4 x 64 + 7 k-mers, cut from a planted sequence repeated"""
        seq = (self.plants[2][0] * 3)[:4 * 64 + 7 + K - 1]
        return [seq[:n + K - 1] for n in range(1, 4 * 64 + 8)]

    def one_wave_reads(self):
        """reads of SILENT k-mers but for one planted stretch that covers exactly the tiles of ONE wave (tile t to wave t mod 4): wave w
        holds k-mers 64 w .. 64 w + 63 and 64 (w + 4) .. of a strand"""
        seq = self.plants[1][0]
        out = []
        for wave in range(WAVES):
            lead = "A" * (64 * wave)
            out.append(lead + seq[:64 + K - 1] + "A" * (64 * (2 * WAVES - wave)))
            out.append(revcomp(out[-1]))
        return out

    def flagged_reads(self):
        """every crafted k-mer at slot positions that are first, middle and last of a group of eight, in the first batch of sixteen and
        in later ones, in the first tile and in tiles of other waves; and all of them in a row"""
        rng = np.random.default_rng(self.rng_seed + 1)
        out = []
        for s in CRAFTED:
            for p in (0, 3, 7, 8, 15, 16, 63, 64, 64 + 11, 3 * 64 + 7, 5 * 64):
                out.append(random_dna(rng, p) + s + random_dna(rng, 9))
            out.append(revcomp(out[-1]))
        out.append("".join(CRAFTED) * 3)
        out.append(CRAFTED[0] * 20)
        return out

    def n_reads(self):
        """the N-carrying sequence whole (its N k-mers are in the filter) and both strands of it; a planted read with an N at the first,
        a middle and the last base, both strands; N alone; and N-free reads between them"""
        seq = self.plants[0][0]
        mid = len(seq) // 2
        with_n = [self.n_seq, revcomp(self.n_seq), "N" + seq[1:], seq[:mid] + "N" + seq[mid + 1:], seq[:-1] + "N"]
        with_n += [revcomp(r) for r in with_n[2:]] + ["N" * 40, seq[:K - 1] + "N", "N" + seq[:K - 1]]
        out = []
        for i, r in enumerate(with_n):
            out += [r, self.plants[i % len(self.plants)][0][:90]]
        return out

    def all_reads(self):
        return [r for r, _ in self.planted_reads()] + self.length_reads() + self.one_wave_reads() + self.flagged_reads() + self.n_reads() + \
               ["C" * 300, "G" * 300, "A" * 100, "ACGT", "A" * (K - 1), ""]


COUNT_FIXTURES = {  # name -> (n_bins, bit load, seed, lines): the three slot sizes, the odd bin count and the last bin count that fits
    "c8193": (8193, 0.15, 91, 4),
    "c31000": (31000, 0.1016, 92, 6),
    "c32256": (32256, 0.1168, 93, 8),
}


@functools.lru_cache(maxsize=None)
def count_fixture(name):
    return CountFixture(*COUNT_FIXTURES[name])


@functools.lru_cache(maxsize=None)
def table_fixture(name):
    n_bins, k, load, seed, _ = FILTERS[name]
    return random_filter(n_bins, k, load, seed)

"""Fixtures of the list-table tests (tests/test_gpu_row_lists.py), kept apart so that what is a property of the FIXTURES -- the
populations of the crafted rows -- is asserted on the oracle alone where there is no GPU (tests/test_row_lists_cpu.py).  Host arithmetic
only: the GPU tests upload the same words."""
import numpy as np

from oracle import pyoracle as po

K, H_FUNCS = 7, 3
SENTINEL, OVERFLOW_MARK = 0xFFFF, 0xFFFE  # readbouncer_amd/csrc/rb_lists.h
# With about a thousand blocks, three of a thousand k-mers have two equal block numbers among their three; such a row is the AND of two
# blocks and overflows every slot the three-block rows would take.  At 16 381 blocks they are three rows in 4^7 and the census follows
# the fill.  The crafted filters rewrite fifteen blocks, three of them to all ones, and every k-mer that shares such a block gets a
# two-block row as well: 65 521 blocks leave a block to less than one k-mer on average.
SPARE_BLOCKS = 16381
CRAFT_BLOCKS = 65521


def expected_rows(o, k, h, n_blocks):
    """-> uint64[4^k, W]: per N-free k-mer (row = base-4 rank, first base most significant) the AND of the oracle's h blocks"""
    W = o.bin_width
    blocks = o.words()[:n_blocks * W].reshape(n_blocks, W)
    r = np.arange(4 ** k)
    digits = np.stack([(r >> (2 * (k - 1 - i))) & 3 for i in range(k)], axis=1).astype(np.uint8)
    rows = np.full((4 ** k, W), ~np.uint64(0), dtype=np.uint64)
    for hash_no in range(h):
        idx = np.array([o.block_index(po.kmer_value(np.ascontiguousarray(digits[i]), k), hash_no) for i in range(4 ** k)], dtype=np.int64)
        rows &= blocks[idx]
    return rows


def row_bits(rows, n_bins):
    """uint64[n, W] -> bool[n, n_bins]"""
    return np.unpackbits(np.ascontiguousarray(rows).view(np.uint8), axis=1, bitorder="little")[:, :n_bins].astype(bool)


def decode_slots(slots, side, n_bins):
    """the list table as the kernel reads it -> (bool[n, n_bins] of the listed bins, overflow rows followed into `side`; the rows that are
    overflow slots).  Asserts the layout of rb_lists.h on the way: ascending bins, then sentinels only; an overflow slot is the mark, two
    index entries and sentinels, and the side indices are each used once."""
    n, cap = slots.shape
    listed = slots < OVERFLOW_MARK
    over = slots[:, 0] == OVERFLOW_MARK
    plain = ~over
    assert not (slots[plain] == OVERFLOW_MARK).any()
    lp, sp = listed[plain], slots[plain].astype(np.int64)
    assert not (lp[:, 1:] & ~lp[:, :-1]).any()                            # no bin behind a sentinel
    assert ((sp[:, 1:] > sp[:, :-1]) | ~lp[:, 1:]).all()                  # ascending, so distinct
    assert (sp[lp] < n_bins).all()
    bits = np.zeros((n, n_bins), dtype=bool)
    rr, cc = np.nonzero(listed & plain[:, None])
    bits[rr, slots[rr, cc]] = True
    if over.any():
        assert (slots[over, 3:] == SENTINEL).all()
        idx = slots[over, 1].astype(np.int64) | (slots[over, 2].astype(np.int64) << 16)
        assert sorted(idx.tolist()) == list(range(len(side))), (sorted(idx.tolist())[:8], len(side))
        bits[over] = row_bits(side[idx], n_bins)
        assert not (np.ascontiguousarray(side).view(np.uint8).reshape(len(side), -1)[:, (n_bins + 7) // 8:]).any()  # pad words list nothing
    else:
        assert len(side) == 0
    return bits, over


def kmer_rank(s):
    r = 0
    for c in s:
        r = r * 4 + "ACGT".index(c)
    return r


class Crafted:
    """A filter of n_bins bins at design load (fill_synth's words, handed in) in which five chosen 7-mers have rows of exactly 0,
    cap - 1, cap, cap + 1 and n_bins set bits (cap = 64 x lines, the slot's capacity): the three blocks of each are rewritten to one
    pattern.  SAT = n_bins - 1 is then set in every block but the three of the empty row, so it counts every k-mer of a read but those."""
    KMERS = ("ACGTACG", "GATTACA", "CCGGTTA", "TGCATGC", "AACCGGT")

    def __init__(self, n_bins, lines, words, n_bits):
        self.n_bins, self.lines, self.cap = n_bins, lines, 64 * lines
        self.W = (n_bins + 63) // 64
        self.o = po.OracleIBF.wrap(n_bins, H_FUNCS, K, n_bits, words)
        assert self.o.n_blocks == CRAFT_BLOCKS
        w = words[:CRAFT_BLOCKS * self.W].reshape(CRAFT_BLOCKS, self.W)
        self.sat = n_bins - 1
        self.want = (0, self.cap - 1, self.cap, self.cap + 1, n_bins)
        blocks = [[self.o.block_index(po.kmer_value(po.encode(s), K), h) for h in range(H_FUNCS)] for s in self.KMERS]
        assert len({b for bs in blocks for b in bs}) == 15, blocks  # fifteen different blocks
        rng = np.random.default_rng(n_bins + lines)
        w[:, self.sat // 64] |= np.uint64(1) << np.uint64(self.sat % 64)
        for bs, m in zip(blocks, self.want):
            bits = np.zeros(self.W * 64, dtype=np.uint8)
            if m:
                others = rng.choice(n_bins - 1, size=m - 1, replace=False)
                bits[others] = 1
                bits[self.sat] = 1
            pattern = np.packbits(bits, bitorder="little").view(np.uint64)
            for b in bs:
                w[b] = pattern
        self.ranks = [kmer_rank(s) for s in self.KMERS]
        self.o = po.OracleIBF.wrap(n_bins, H_FUNCS, K, n_bits, words)  # (the view the tests compare with: the words as they are now)

    def reads(self):
        rc = lambda s: s[::-1].translate(str.maketrans("ACGT", "TGCA"))
        ks = list(self.KMERS)
        out = ks + [rc(s) for s in ks]
        out += [a + b for a in ks for b in ks if a != b]
        out += ["".join(ks) * 3, rc("".join(ks) * 3), "".join(ks[1:]) * 11, (ks[4] + ks[0]) * 40, ks[0] * 9]
        return out


# Reads that hit NOTHING, on either strand: the blocks of a few 7-mers and of their reverse complements are cleared, so their rows are
# empty slots -- sentinels from the first entry to the last -- and a read made of them alone has a true maximum of 0 with n > 0.  Only such
# a read shows an entry that is no bin being counted where the add itself goes nowhere: every other read's maximum is 1 or more anyway.
SILENT_KMERS = ("AAAAAAA", "ACGTACG")


def revcomp(s):
    return s[::-1].translate(str.maketrans("ACGT", "TGCA"))


def silence(n_bins, n_blocks, words, n_bits):
    """clears the blocks of SILENT_KMERS and their reverse complements in `words` -> the oracle's view of the words as they are then"""
    o = po.OracleIBF.wrap(n_bins, H_FUNCS, K, n_bits, words)
    W = (n_bins + 63) // 64
    w = words[:n_blocks * W].reshape(n_blocks, W)
    for s in SILENT_KMERS:
        for t in (s, revcomp(s)):
            for h in range(H_FUNCS):
                w[o.block_index(po.kmer_value(po.encode(t), K), h)] = 0
    return po.OracleIBF.wrap(n_bins, H_FUNCS, K, n_bits, words)


def silent_reads():
    """one k-mer, a tile of 64, a tile and one, several tiles, the reverse strand's view of them, and the other silent k-mer both ways"""
    return ["A" * K, "A" * (K + 63), "A" * (K + 64), "A" * 200, "T" * 100, SILENT_KMERS[1], revcomp(SILENT_KMERS[1])]

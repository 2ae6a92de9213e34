"""Fixtures of tests/test_gpu_list_scan.py: the list kernel counts with adds that return nothing and finds a strand's maximum by
scanning the counters, so the fixtures put the maximum where a scan can lose it, fill the spare dwords with junk, put the forward
maximum on either side of every point where the second strand's stop rule can fire, and put overflow slots at chosen places of a group
of eight slots.  Host arithmetic on the oracle's words only: the GPU tests upload the same words, and tests/test_list_scan_cpu.py
asserts on the oracle alone that the fixtures are what they claim."""
import numpy as np

from oracle import pyoracle as po
from tests import helpers as H
from tests import row_lists_rig as LR

K = LR.K
N_BLOCKS = 1021
rc = LR.revcomp

# With 1021 blocks three k-mers in a thousand have two equal block numbers; their rows, the AND of two blocks, decide the slot size
# (tests/row_lists_rig.py).  Bit loads that put those rows (load^2 x n_bins bins) well inside one, two and four lines:
LOADS = {(2112, 1): 0.120, (2112, 2): 0.210, (2112, 4): 0.295,
         (4090, 1): 0.088, (4090, 2): 0.152, (4090, 4): 0.213,
         (8192, 1): 0.062, (8192, 2): 0.107, (8192, 4): 0.150}
GEOMETRIES = sorted(LOADS)


def n_bits(n_bins, n_blocks=N_BLOCKS):
    return ((n_bins + 63) // 64) * 64 * n_blocks


def random_fill(words, n_bins, n_blocks, load, seed):
    W = (n_bins + 63) // 64
    bits = np.random.default_rng(seed).random((n_blocks, W * 64)) < load
    bits[:, n_bins:] = False
    words[:n_blocks * W].reshape(n_blocks, W)[:] = np.packbits(bits, axis=1, bitorder="little").view(np.uint64)


def wrap(n_bins, words, n_blocks=N_BLOCKS):
    return po.OracleIBF.wrap(n_bins, LR.H_FUNCS, K, n_bits(n_bins, n_blocks), words)


def scan_bins(n_bins):
    """where a scan of 16-byte pieces (eight bins each, lane l takes pieces l, l + 64, ...) can lose a maximum: the two halves of the
    first and of the last counter dword, the first and the last bin of the pieces of lane 0, lane 1 and lane 63, of lane 0's second
    piece and of the last piece that holds a bin, and one bin in the middle"""
    last_piece = 8 * ((n_bins - 1) // 8)
    bins = [0, 1, 7, 8, 15, 504, 511, 512, 519, last_piece, min(last_piece + 7, n_bins - 1), n_bins - 2, n_bins - 1, n_bins // 2 + 3]
    return sorted(set(bins))


class Planted:
    """a filter of the given geometry and slot size with one read of 70 to 200 k-mers planted per bin of scan_bins()"""

    def __init__(self, n_bins, lines, words):
        self.n_bins, self.lines = n_bins, lines
        random_fill(words, n_bins, N_BLOCKS, LOADS[(n_bins, lines)], seed=n_bins + lines)
        rng = np.random.default_rng(n_bins * 8 + lines)
        self.o = wrap(n_bins, words)
        self.bins = scan_bins(n_bins)
        self.kmers = [int(x) for x in np.linspace(70, 200, len(self.bins)).astype(int)]
        self.plants = [H.random_dna(rng, n + K - 1) for n in self.kmers]
        for seq, b in zip(self.plants, self.bins):
            self.o.insert(po.encode(seq), b)
        self.noise = [H.random_dna(rng, n + K - 1) for n in TAILS]

    def reads(self):
        """every planted read, and its reverse complement (the maximum is then the second strand's)"""
        return self.plants + [rc(s) for s in self.plants]

    def tail_reads(self):
        """strands of TAILS k-mers: the head of a planted read (all of its k-mers count in the read's bin), its reverse complement, noise"""
        heads = [self.plants[i % len(self.plants)][:n + K - 1] for i, n in enumerate(TAILS)]
        return heads + [rc(s) for s in heads] + self.noise


TAILS = (1, 7, 8, 9, 63, 64, 65, 71)


class Sparse:
    """the same random fill with the blocks of LR.SILENT_KMERS cleared and nothing planted: reads that hit little or nothing, while
    nearly every entry of every slot is a sentinel and goes to the spare dwords"""

    def __init__(self, n_bins, lines, words):
        self.n_bins, self.lines = n_bins, lines
        random_fill(words, n_bins, N_BLOCKS, LOADS[(n_bins, lines)], seed=n_bins + lines)
        self.o = LR.silence(n_bins, N_BLOCKS, words, n_bits(n_bins))
        rng = np.random.default_rng(n_bins * 8 + lines + 1)
        self.negatives = [H.random_dna(rng, int(n) + K - 1) for n in (70, 128, 129, 200, 300, 640)]

    def reads(self):
        return self.negatives + LR.silent_reads()


def distinct_read(rng, length, used):
    """a random read none of whose 7-mers, on either strand, is in `used` or occurs twice (there are only 4^7 of them: reads drawn
    freely share plenty, and a planted k-mer must count where it stands and nowhere else) -> the read; its k-mers are added to `used`"""
    while True:
        read, mine = H.random_dna(rng, K - 1), set()
        while len(read) < length:
            ways = [c for c in "ACGT" if not {read[-(K - 1):] + c, rc(read[-(K - 1):] + c)} & (used | mine)]
            if not ways:
                break  # a dead end: once more from the start
            read += ways[int(rng.integers(len(ways)))]
            mine |= {read[-K:], rc(read[-K:])}
        if len(read) == length:
            used |= mine
            return read


class Stops:
    """Reads of N = 200 k-mers on a filter that holds nothing else.  The first `best` k-mers of a read are planted in a bin of its own,
    so the forward strand counts exactly `best`, for best = N - mt + off, mt in (64, 128, 192), off in (-1, 0, 1): the second strand's
    stop rule, so_far(mt) + (N - mt) <= best, can fire at tile edge mt only when off >= 0, and only with so_far(mt) <= off.  Each case
    comes twice: with a second strand that counts nothing, and with one that counts REV k-mers -- the reverse complement of k-mers
    10 to 10 + REV of the read, planted in another bin."""
    N, N_BINS, N_BLOCKS, REV = 200, 2112, LR.SPARE_BLOCKS, 3
    CASES = [(mt, off, rev) for mt in (64, 128, 192) for off in (-1, 0, 1) for rev in (0, 3)]

    def __init__(self, words):
        self.o = wrap(self.N_BINS, words, self.N_BLOCKS)
        rng = np.random.default_rng(200)
        self.items, used = [], set()
        for i, (mt, off, rev) in enumerate(self.CASES):
            read = distinct_read(rng, self.N + K - 1, used)
            best = self.N - mt + off
            self.o.insert(po.encode(read[:best + K - 1]), 40 + 100 * i)
            if rev:
                self.o.insert(po.encode(rc(read[10:10 + rev + K - 1])), 41 + 100 * i)
            self.items.append(read)

    def reads(self):
        return list(self.items)

    def forward(self, read):
        return int(self.o.count(po.encode(read)).max())

    def so_far(self, read, mt):
        """what the second strand has counted after the read's first mt k-mers"""
        return int(self.o.count(po.encode(rc(read[:mt + K - 1]))).max()) if mt else 0

    def reverse_stop(self, read):
        """the first tile edge at which nothing to come can pass the forward maximum, else the strand's end"""
        n, best = len(read) - K + 1, self.forward(read)
        if best >= n:
            return 0
        for mt in range(0, n, 64):
            if self.so_far(read, mt) + (n - mt) <= best:
                return mt
        return n


class CraftedGroups(LR.Crafted):
    """LR.Crafted, with bin 0 in the row of cap + 1 bins (a set bit of the three blocks' pattern is moved there if need be): the row's
    overflow slot is mark, index low, index high, and an index half that is counted as a bin lands in bin 0 (the high half: the side
    table is small) or in bin `index`.  The k-mer alone counts every bin of its row once; counted entries make bin 0 two or more."""
    OVER = LR.Crafted.KMERS[3]  # "TGCATGC": TGCATGCATGC holds it twice, four k-mers apart

    def __init__(self, n_bins, lines, words, n_bits_):
        super().__init__(n_bins, lines, words, n_bits_)
        w = words[:LR.CRAFT_BLOCKS * self.W].reshape(LR.CRAFT_BLOCKS, self.W)
        blocks = [self.o.block_index(po.kmer_value(po.encode(self.OVER), K), h) for h in range(LR.H_FUNCS)]
        if not int(w[blocks[0], 0]) & 1:
            row = LR.row_bits(w[blocks[0]][None, :], n_bins)[0]
            moved = int(np.nonzero(row)[0][0])
            assert moved != self.sat
            for b in blocks:
                w[b, moved // 64] &= ~(np.uint64(1) << np.uint64(moved % 64))
                w[b, 0] |= np.uint64(1)
        self.o = po.OracleIBF.wrap(n_bins, LR.H_FUNCS, K, n_bits_, words)

    # k-mer positions of the overflow slot within a read: first, last and a middle slot of a group of eight, two in one group, the
    # first and the last slot of a tile, in the second tile, and in a tail tile's last, partly filled group
    PLACES = ((8,), (15,), (11,), (9, 13), (0,), (63,), (64 + 19,), (128 + 2,), (24, 28))

    def group_reads(self):
        rng = np.random.default_rng(self.n_bins)
        out = [self.OVER, rc(self.OVER)]
        for places in self.PLACES:
            read = list(H.random_dna(rng, max(places) + K + int(rng.integers(1, 40))))
            for p in places:
                read[p:p + K] = self.OVER
            out.append("".join(read))
        return out + [rc(r) for r in out[2:]]

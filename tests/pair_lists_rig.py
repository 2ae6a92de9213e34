"""Fixtures of the pair-table tests (tests/test_gpu_pair_lists.py), kept apart so that what is a property of the FIXTURES -- the
populations of the crafted pairs, the caps of the census on config 3's geometry -- is asserted on the oracle alone where there is no GPU
(tests/test_pair_lists_cpu.py).  Host arithmetic only: the GPU tests upload the same words."""
import numpy as np

from oracle import pyoracle as po
from tests import row_lists_rig as LR

H_FUNCS = 3
SENTINEL, DENSE_MARK, TAIL_MARK = 0xFFFF, 0xFFFE, 0xFFFD  # readbouncer_amd/csrc/rb_pair_lists.h
CANON, POSITIONAL, REST, REST_INDEXED, TAIL_HALVES = 256, 64, 64, 62, 64
CAPACITY, TAIL_CAPACITY = 192, 254
PLAIN, TAIL, DENSE = 0, 1, 2
TAIL_SHARE, DENSE_SHARE = 32, 1024  # the census's caps: one sampled pair in ...
SPARE_BLOCKS, CRAFT_BLOCKS = LR.SPARE_BLOCKS, LR.CRAFT_BLOCKS


def revcomp(s):
    return s[::-1].translate(str.maketrans("ACGT", "TGCA"))


def rc_ranks(k):
    """-> int64[4^k]: the rank of the reverse complement of the k-mer of rank r"""
    r = np.arange(4 ** k, dtype=np.int64)
    out = np.zeros_like(r)
    for i in range(k):
        out = out * 4 + (3 - ((r >> (2 * i)) & 3))
    return out


def rest_of(nA, nB):
    return np.maximum(np.asarray(nA) - POSITIONAL, 0) + np.maximum(np.asarray(nB) - POSITIONAL, 0)


def kind_of(nA, nB):
    rest = rest_of(nA, nB)
    return np.where(rest <= REST, PLAIN, np.where(rest <= REST_INDEXED + TAIL_HALVES, TAIL, DENSE))


def expected_pairs(o, k, n_blocks, n_bins):
    """-> (bool[4^k, n_bins] of row(x), bool[4^k, n_bins] of row(rc(x))) from the oracle's blocks"""
    a = LR.row_bits(LR.expected_rows(o, k, H_FUNCS, n_blocks), n_bins)
    return a, a[rc_ranks(k)]


def cnt_dwords(n_bins):
    return (n_bins + 255) & ~255


def decode_tail(line, n_bins):
    """one tail line (uint32[32]) -> ([bins of list A], [bins of list B]); asserts line 2's format: A's entries, then B's, then spares"""
    halves = np.stack([line & 0xFFFF, line >> 16], axis=1).reshape(-1).astype(np.int64)
    A, B, stage = [], [], 1
    for q, h in enumerate(halves):
        assert not (h & 2), (q, hex(h))
        if (h >> 2) >= cnt_dwords(n_bins):
            assert h == (cnt_dwords(n_bins) + q) * 4, (q, hex(h))
            stage = 0
            continue
        what = 2 if (h & 1) else 1
        assert stage and not (stage == 2 and what == 1) and (h >> 2) < n_bins, (q, hex(h))
        stage = what
        (B if what == 2 else A).append(int(h >> 2))
    return A, B


def decode_slots(slots, tails, side, n_bins, whole=True):
    """the pair table as the kernel reads it -> (bool[n, n_bins] list A, bool[n, n_bins] list B, int[n] kind), tail lines and dense rows
    followed.  Asserts the canonical layout on the way: ascending bins, one sentinel between the lists, sentinels to entry 252, marks and
    indices in entries 253-255 only, every tail line and every dense row pair named exactly once."""
    n = len(slots)
    assert slots.shape == (n, CANON)
    A = np.zeros((n, n_bins), dtype=bool)
    B = np.zeros((n, n_bins), dtype=bool)
    kind = np.where(slots[:, 255] == SENTINEL, PLAIN, np.where(slots[:, 255] == TAIL_MARK, TAIL, DENSE))
    assert np.isin(slots[:, 255], (SENTINEL, TAIL_MARK, DENSE_MARK)).all()
    assert (slots[kind == PLAIN][:, 253:255] == SENTINEL).all()
    body = slots[:, :253].astype(np.int64)
    used_tails, used_rows = [], []
    for r in range(n):
        ends = np.nonzero(body[r] == SENTINEL)[0]
        nA = int(ends[0])
        a = body[r, :nA]
        rest = body[r, nA + 1:]
        nB = int(np.nonzero(rest == SENTINEL)[0][0])
        b = rest[:nB]
        assert (rest[nB:] == SENTINEL).all(), r
        assert (np.diff(a) > 0).all() and (np.diff(b) > 0).all() and (a < n_bins).all() and (b < n_bins).all(), r
        A[r, a] = True
        B[r, b] = True
        index = int(slots[r, 253]) | (int(slots[r, 254]) << 16)
        if kind[r] == TAIL:
            assert rest_of(nA, nB) == REST_INDEXED, (r, nA, nB)  # a tail slot's line 2 is full
            ta, tb = decode_tail(tails[index], n_bins)
            assert not A[r, ta].any() and not B[r, tb].any() and (not ta or not len(a) or min(ta) > a[-1]) and (not tb or not len(b) or min(tb) > b[-1]), r
            A[r, ta] = True
            B[r, tb] = True
            used_tails.append(index)
        elif kind[r] == DENSE:
            assert nA == 0 and nB == 0, r
            A[r] = LR.row_bits(side[index:index + 1], n_bins)[0]
            B[r] = LR.row_bits(side[index + 1:index + 2], n_bins)[0]
            used_rows.append(index)
    if whole:  # (a prefix of a table names some of the tail lines and dense rows only)
        assert sorted(used_tails) == list(range(len(tails))), (len(used_tails), len(tails))
        assert sorted(used_rows) == list(range(0, len(side), 2)), (len(used_rows), len(side))
    else:
        assert len(set(used_tails)) == len(used_tails) and len(set(used_rows)) == len(used_rows) and not any(i & 1 for i in used_rows)
    return A, B, kind


class CraftedPairs:
    """A filter of n_bins bins at design load (fill_synth's words, handed in) in which chosen k-mers x have rows of exactly nA bins and
    their reverse complements rows of exactly nB bins: the three blocks of each are rewritten to one pattern.  PAIRS names the cases:
    nothing at all; capacity - 1, capacity and capacity + 1 (the first tail); 254 and 255 (the first dense row pair); one list of 128
    with a short other, and the mirror, which stay plain.  Every pair is in the table twice, under x and under rc(x)."""
    K = 7
    KMERS = ("ACGTACG", "GATTACA", "CCGGTTA", "TGCATGC", "AACCGGT", "CTTGACC", "GGATCTA", "TCAGTCA")
    PAIRS = ((0, 0), (96, 95), (96, 96), (97, 96), (127, 127), (128, 127), (128, 10), (10, 128))

    def __init__(self, n_bins, words, n_bits):
        k = self.K
        self.n_bins, self.W = n_bins, (n_bins + 63) // 64
        o = po.OracleIBF.wrap(n_bins, H_FUNCS, k, n_bits, words)
        assert o.n_blocks == CRAFT_BLOCKS
        w = words[:CRAFT_BLOCKS * self.W].reshape(CRAFT_BLOCKS, self.W)
        both = [s for x in self.KMERS for s in (x, revcomp(x))]
        blocks = [[o.block_index(po.kmer_value(po.encode(s), k), h) for h in range(H_FUNCS)] for s in both]
        assert len({b for bs in blocks for b in bs}) == 3 * len(both), blocks  # all different: no palindrome, no shared block
        rng = np.random.default_rng(n_bins)
        for i, (nA, nB) in enumerate(self.PAIRS):
            for bs, m in ((blocks[2 * i], nA), (blocks[2 * i + 1], nB)):
                bits = np.zeros(self.W * 64, dtype=np.uint8)
                bits[rng.choice(n_bins, size=m, replace=False)] = 1
                for b in bs:
                    w[b] = np.packbits(bits, bitorder="little").view(np.uint64)
        self.ranks = [LR.kmer_rank(s) for s in self.KMERS]
        self.rc_ranks = [LR.kmer_rank(revcomp(s)) for s in self.KMERS]
        self.o = po.OracleIBF.wrap(n_bins, H_FUNCS, k, n_bits, words)  # the words as they are now

    def kinds(self):
        return [int(kind_of(a, b)) for a, b in self.PAIRS]

    def reads(self):
        ks = list(self.KMERS)
        tail, tail2, dense = ks[3], ks[4], ks[5]
        out = ks + [revcomp(s) for s in ks]
        out += [a + b for a in ks for b in ks if a != b]
        # a tail slot first and last of a group of eight (k-mers 0 and 7), two in one group, a dense and a tail slot in one group, and
        # the same deep inside longer reads (other tiles, other waves of the workgroup)
        out += [tail + tail2, tail + tail, dense + tail, tail + dense + tail2, "".join(ks) * 3, revcomp("".join(ks) * 3), (tail + ks[0]) * 40, (ks[6] + ks[7]) * 30]
        out += ["ACGT" * 90 + tail + dense, tail2 * 60]
        return out


def census_shares(n_bins, p, pairs, seed):
    """the shares of `pairs` simulated pairs, nA and nB independent Binomial(n_bins, p), that need a tail or more / dense rows"""
    rng = np.random.default_rng(seed)
    nA, nB = rng.binomial(n_bins, p, pairs), rng.binomial(n_bins, p, pairs)
    k = kind_of(nA, nB)
    return float((k != PLAIN).mean()), float((k == DENSE).mean())

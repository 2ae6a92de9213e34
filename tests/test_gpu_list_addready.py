"""The resident ("add-ready") form of the list table (readbouncer_amd/csrc/rb_lists.h): the device keeps every slot half as a ready LDS
byte offset, even bins in low halves and odd bins in high halves, and a group of eight slots without a flag is counted with two vector
instructions per dword; rows whose even or odd bins alone exceed half a slot carry swapped halves, overflow slots a flag, and both take
the careful path of list_batch.  None of that may change a result.  Five crafted rows -- all even, all odd, exactly cap bins with
unbalanced parity, cap + 1 bins (an overflow slot) and none -- belong to the five 7-mers of ONE 11-mer, so they sit next to each other in
one group of eight wherever a read holds it.  The count kernel's raw maxima, locate and hits from the list table, and the downloaded
table are compared with the oracle bit for bit at one, two and four lines per slot.  k = 7: tables of 4^7 slots."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import pyoracle as po
from readbouncer_amd import capi
from tests import helpers as H
from tests import list_scan_rig as SR
from tests import row_lists_rig as LR
from tests import test_gpu_list_scan as LS
from tests import test_gpu_pass_lists as GP
from tests import test_gpu_row_lists as LT
from tests import test_gpu_row_table as RT

K = LR.K
rc = LR.revcomp
GEOMETRIES = ((8192, 2), (2112, 1), (8192, 4))  # the last at a bit load of 0.15: the census sends it to four lines


class Rows:
    """A filter at SR.LOADS' bit load in which the five 7-mers of STRETCH have rows of chosen bins: the three blocks of each are
    rewritten to one pattern.
      even   : cap / 2 + 9 even bins -- more than the low halves hold: swapped halves, and no odd bin at all
      odd    : cap - 1 odd bins
      tilted : exactly cap bins, 70 : 58 even to odd in proportion; every odd bin is the upper neighbour of an even one, and the even
               bins without a neighbour are the lowest of the row -- so whichever even bins the builder swaps, one that is added with the
               wrong constant lands on a bin of the row and doubles it
      over   : cap + 1 bins: an overflow slot
      none   : no bin"""
    NAMES = ("even", "odd", "tilted", "over", "none")

    def __init__(self, n_bins, lines, words):
        self.n_bins, self.lines, self.cap = n_bins, lines, 64 * lines
        SR.random_fill(words, n_bins, SR.N_BLOCKS, SR.LOADS[(n_bins, lines)], seed=n_bins + lines)
        o = SR.wrap(n_bins, words)
        W = (n_bins + 63) // 64
        w = words[:SR.N_BLOCKS * W].reshape(SR.N_BLOCKS, W)
        rng = np.random.default_rng(7 * n_bins + lines)
        while True:  # an 11-mer whose five k-mers and their reverse complements have thirty different blocks
            s = H.random_dna(rng, K + 4)
            kmers = [s[i:i + K] for i in range(5)]
            blocks = [[o.block_index(po.kmer_value(po.encode(t), K), h) for h in range(LR.H_FUNCS)] for t in kmers + [rc(t) for t in kmers]]
            if len({b for bs in blocks for b in bs}) == 30:
                break
        self.STRETCH, self.kmers = s, dict(zip(self.NAMES, kmers))
        cap, half = self.cap, self.cap // 2
        n_even = cap * 70 // 128
        lone = 2 * np.arange(n_even - (cap - n_even))                                     # bins 0, 2, ...: the first word(s)
        pairs = 2 * rng.choice(np.arange(64, n_bins // 2 - 1), size=cap - n_even, replace=False)
        self.bins = dict(even=2 * rng.choice(n_bins // 2, size=half + 9, replace=False),
                         odd=2 * rng.choice(n_bins // 2, size=cap - 1, replace=False) + 1,
                         tilted=np.concatenate([lone, pairs, pairs + 1]),
                         over=rng.choice(n_bins, size=cap + 1, replace=False),
                         none=np.zeros(0, dtype=np.int64))
        for name, bs in zip(self.NAMES, blocks):
            bits = np.zeros(W * 64, dtype=np.uint8)
            bits[self.bins[name]] = 1
            assert int(bits.sum()) == len(self.bins[name]) and int(bits[n_bins:].sum()) == 0
            for b in bs:
                w[b] = np.packbits(bits, bitorder="little").view(np.uint64)
        self.ranks = {name: LR.kmer_rank(t) for name, t in self.kmers.items()}
        self.o = SR.wrap(n_bins, words)

    def reads(self):
        rng = np.random.default_rng(self.n_bins)
        S = self.STRETCH

        def around(n_kmers, places):
            read = list(H.random_dna(rng, n_kmers + K - 1))
            for p in places:
                read[p:p + len(S)] = S
            return "".join(read)

        out = [S] + list(self.kmers.values())                                          # one group; one k-mer
        out += [around(63, (8,)), around(64, (56,)), around(65, (58,)), around(65, (0, 40))]  # 63, 64 and 65 k-mers
        out += [around(70, (62,))]                                                      # the stretch across a tile's edge
        out += [around(200, (3, 64 + 40, 128 + 17)), around(321, (61, 180, 310))]       # several tiles
        out += [rc(r) for r in out]
        return out + [self.kmers["tilted"] * 200, rc(self.kmers["tilted"] * 200)]       # far above anything a stray add could produce


@pytest.fixture(scope="module", params=GEOMETRIES, ids=lambda g: "%d-%d" % g)
def rows(request):
    n_bins, lines = request.param
    d, f = LS.resident(lambda words, info: Rows(n_bins, lines, words), n_bins, SR.N_BLOCKS, lines)
    yield d, f
    d.free()


def test_download_is_the_canonical_form_of_the_expected_rows(rows):
    d, f = rows
    info = d.list_table_info()
    assert info["lines"] == f.lines
    slots, side = d.list_table_download()
    want = LR.row_bits(LR.expected_rows(f.o, K, LR.H_FUNCS, SR.N_BLOCKS), f.n_bins)
    pop = want.sum(axis=1)
    for name in f.NAMES:
        assert pop[f.ranks[name]] == len(f.bins[name]) and np.array_equal(np.nonzero(want[f.ranks[name]])[0], np.sort(f.bins[name])), name
    over = pop > f.cap
    assert over[f.ranks["over"]] and not over[f.ranks["tilted"]] and info["side_rows"] == int(over.sum())
    canon = np.full((4 ** K, f.cap), LR.SENTINEL, dtype=np.uint16)  # ascending bins, then 0xFFFF to the end
    for r in np.nonzero(~over)[0]:
        canon[r, :pop[r]] = np.nonzero(want[r])[0]
    assert np.array_equal(slots[~over], canon[~over])
    assert (slots[over, 0] == LR.OVERFLOW_MARK).all() and (slots[over, 3:] == LR.SENTINEL).all()  # the mark, two index entries
    idx = slots[over, 1].astype(np.int64) | (slots[over, 2].astype(np.int64) << 16)
    assert sorted(idx.tolist()) == list(range(len(side)))
    assert np.array_equal(LR.row_bits(side[idx], f.n_bins), want[over])
    got, got_over = LR.decode_slots(slots, side, f.n_bins)  # (the existing reader of the table agrees)
    assert np.array_equal(got, want) and np.array_equal(got_over, over)
    # a prefix that ends inside a slot: converted on the host, the same entries
    n = 5 * f.cap + 3
    part = np.zeros(n, dtype=np.uint16)
    assert capi.lib().rb_dibf_list_table_download(d.h, capi._ptr(part), n, None, 0) == 0
    assert np.array_equal(part, slots.reshape(-1)[:n])


def test_count_kernel_equals_the_oracle(rows):
    d, f = rows
    reads = f.reads()
    batch = H.pack_reads(reads)
    expected = RT.reference(f.o, batch)
    n_t = 200 * K - K + 1
    assert expected[0][-2, 0] >= 200 and expected[0][-2, 0] < 400 and int(batch[2][-1]) - K + 1 == n_t
    for nt in (0, 1):
        eng = LT.lists_engine(d, nt)
        for prune in (1, 0):
            eng.set_bound_pruning(prune)
            LT.check(eng, batch, expected, ("add-ready", f.n_bins, f.lines, nt, prune), LT.LISTS_KERNEL, repeats=1)
        eng.destroy()


def test_locate_and_hits_from_the_list_table_equal_the_oracle(rows):
    """hits at min_count 1 with room for every bin: every counter of both strands, not the maximum alone"""
    d, f = rows
    eng = GP.lists_engine([d])
    for nt in (0, 1):
        eng.set_nt_threshold(0 if nt else GP.NT_DEFAULT)
        GP.run_both(eng, [f.o], f.reads(), [f.lines], ("add-ready", f.n_bins, f.lines, nt))
    eng.destroy()

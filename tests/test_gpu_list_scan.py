"""ibf_count_lists_kernel counts with LDS adds that return nothing and finds a strand's maximum by scanning the counters (rb_lists.hip):
entries that are no bin go to spare dwords behind the counters, the second strand's stop rule scans at a tile edge only where it can
fire, overflow slots are found per group of eight slots, and full tiles take a path of their own.  None of that may change a result:
every case here runs under RB_ROW_TABLE_LISTS with the plan naming the list kernel and is compared bit for bit with the oracle.  The
fixtures are tests/list_scan_rig.py's; what they claim of themselves is asserted without a GPU in tests/test_list_scan_cpu.py."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import helpers as H
from tests import list_scan_rig as SR
from tests import row_lists_rig as LR
from tests import test_gpu_row_lists as LT
from tests import test_gpu_row_table as RT

K = SR.K
LISTS_KERNEL = LT.LISTS_KERNEL


def resident(make, n_bins, n_blocks, lines, seed=None):
    """-> (the resident filter, the fixture `make(words, info)` built on its words before the upload); the list table is built and
    has `lines` lines per slot"""
    made = {}

    def edit(w, host):
        made["f"] = make(host.words(), host.info)

    d, owner = LT.uploaded(n_bins, n_blocks, K, edit, seed=seed)
    made["f"]._owner = owner  # (keeps the words the fixture's oracle looks at)
    info = d.list_table_build()
    assert info["refused"] == 0 and info["lines"] == lines, info
    return d, made["f"]


def both_ways(d, f, reads, label):
    """the reads under LISTS, temporal and not, bound on and off, against the fixture's oracle"""
    batch = H.pack_reads(reads)
    expected = RT.reference(f.o, batch)
    for nt in (0, 1):
        eng = LT.lists_engine(d, nt)
        for prune in (1, 0):
            eng.set_bound_pruning(prune)
            p = LT.check(eng, batch, expected, (label, nt, prune), LISTS_KERNEL, repeats=1)
            assert p["nontemporal"] == nt
        eng.destroy()
    return expected


@pytest.mark.parametrize("n_bins,lines", SR.GEOMETRIES)
def test_where_the_maximum_sits_and_tail_tiles(n_bins, lines):
    """one read planted per bin at the edges of the counters and of a lane's 16-byte scan pieces, on either strand, at 2112, 4090 and
    8192 bins (a rounded-up cnt_dwords, a last piece that is half pad) and at one, two and four lines; then strands of 1 to 71 k-mers,
    where the last group of eight slots is partly or wholly beyond the strand (at four lines: half-tiles of 32)"""
    d, f = resident(lambda words, info: SR.Planted(n_bins, lines, words), n_bins, SR.N_BLOCKS, lines)
    reads = f.reads()
    expected = both_ways(d, f, reads, "planted")
    assert expected[0][:len(f.bins), 0].tolist() == f.kmers and expected[0][len(f.bins):, 0].tolist() == f.kmers
    tails = f.tail_reads()
    expected = both_ways(d, f, tails, "tails")
    assert expected[0][:2 * len(SR.TAILS), 0].tolist() == list(SR.TAILS) * 2
    d.free()


@pytest.mark.parametrize("n_bins,lines", SR.GEOMETRIES)
def test_spares_never_leak(n_bins, lines):
    """reads that hit little or nothing on a sparse filter: nearly every entry of every slot is a sentinel, so the junk in the spare
    dwords is far beyond every true count, and the silent reads (LR.silent_reads) must still count 0"""
    d, f = resident(lambda words, info: SR.Sparse(n_bins, lines, words), n_bins, SR.N_BLOCKS, lines)
    slots, _ = d.list_table_download()
    assert (slots == LR.SENTINEL).mean() > 0.5
    reads = f.reads()
    expected = both_ways(d, f, reads, "sparse")
    assert not expected[0][len(f.negatives):].any()
    d.free()


def test_exact_stops():
    """the forward maximum one below, at and one above n - mt for every tile edge mt of a strand of 200 k-mers, with a second strand
    that has counted nothing or three by then: the trace's reverse stop is the first edge where so_far + (n - mt) <= best, else n,
    and the maxima are the same with the bound off"""
    torch = pytest.importorskip("torch")
    S = SR.Stops
    d, f = resident(lambda words, info: S(words), S.N_BINS, S.N_BLOCKS, 1)
    reads = f.reads()
    batch = H.pack_reads(reads)
    expected = RT.reference(f.o, batch)
    want = [f.reverse_stop(r) for r in reads]
    assert expected[0][:, 0].tolist() == [S.N - mt + off for mt, off, _ in S.CASES] and set(want) == {64, 128, 192, S.N}
    for nt in (0, 1):
        eng = LT.lists_engine(d, nt)
        eng.set_bound_pruning(0)
        LT.check(eng, batch, expected, ("stops, no bound", nt), LISTS_KERNEL, repeats=1)
        eng.set_bound_pruning(1)
        t = torch.zeros(len(reads), dtype=torch.int64, device="cuda:0")
        torch.cuda.synchronize()
        eng.set_prune_trace(t.data_ptr())
        LT.check(eng, batch, expected, ("stops, bound", nt), LISTS_KERNEL, repeats=1)
        torch.cuda.synchronize()
        eng.set_prune_trace(None)
        r = t.cpu().numpy().view(np.uint64)
        stop_fwd = ((r >> np.uint64(16)) & np.uint64(0xFFFF)).astype(np.int64).tolist()
        stop_rev = ((r >> np.uint64(32)) & np.uint64(0xFFFF)).astype(np.int64).tolist()
        assert stop_fwd == [S.N] * len(reads)
        assert stop_rev == want, (nt, list(zip(S.CASES, stop_rev, want)))
        eng.destroy()
    d.free()


@pytest.mark.parametrize("n_bins,lines", ((2112, 1), (8192, 2)))
def test_overflow_slot_inside_a_group(n_bins, lines):
    """LR.Crafted's row of cap + 1 bins as the first, the last and a middle slot of a group of eight, twice in one group, at the edges
    of a tile and in a tail tile, next to ordinary slots; and alone, where its index entries, counted as bins, would double bin 0"""
    d, c = resident(lambda words, info: SR.CraftedGroups(n_bins, lines, words, info["n_bits"]), n_bins, LR.CRAFT_BLOCKS, lines, seed=5)
    slots, side = d.list_table_download()
    rank = LR.kmer_rank(c.OVER)
    assert slots[rank, 0] == LR.OVERFLOW_MARK and (slots[rank, 3:] == LR.SENTINEL).all()
    reads = c.group_reads()
    expected = both_ways(d, c, reads, "groups")
    assert expected[0][0, 0] == 1
    d.free()

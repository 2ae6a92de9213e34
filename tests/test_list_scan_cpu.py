"""The fixtures of tests/test_gpu_list_scan.py (tests/list_scan_rig.py), checked on the oracle alone: the slot size every filter is
meant to take, where the planted maxima sit, that the sparse filters' reads count little or nothing, that every case of the stop
fixture occurs, and that the overflow k-mer stands where the reads claim."""
import numpy as np
import pytest

from oracle import pyoracle as po
from tests import list_scan_rig as SR
from tests import row_lists_rig as LR
from tests.test_row_lists_cpu import census

K = SR.K


def host_words(n_bins, n_blocks=SR.N_BLOCKS):
    o = po.OracleIBF(n_bins, LR.H_FUNCS, K, SR.n_bits(n_bins, n_blocks))
    return o, o.words()


@pytest.mark.parametrize("n_bins,lines", SR.GEOMETRIES)
def test_planted_and_sparse_filters_take_the_slot_size_they_claim(n_bins, lines):
    owner, words = host_words(n_bins)
    p = SR.Planted(n_bins, lines, words)
    got, over, _ = census(p.o, K, SR.N_BLOCKS, n_bins)
    assert got == lines, (over,)
    assert {0, 1, n_bins - 2, n_bins - 1} <= set(p.bins) and all(b < n_bins for b in p.bins)
    assert any(b % 8 == 0 for b in p.bins) and any(b % 8 == 7 for b in p.bins) and any(b >= 512 for b in p.bins)
    for seq, b, n in zip(p.plants, p.bins, p.kmers):
        c = p.o.count(po.encode(seq))
        assert 70 <= n <= 200 and int(c[b]) == n == len(seq) - K + 1 and int((c == n).sum()) == 1, (b, n)  # the maximum sits in its bin alone
    assert [len(r) - K + 1 for r in p.tail_reads()[:len(SR.TAILS)]] == list(SR.TAILS)
    owner2, words2 = host_words(n_bins)
    s = SR.Sparse(n_bins, lines, words2)
    got, over, _ = census(s.o, K, SR.N_BLOCKS, n_bins)
    assert got == lines, (over,)
    for r in LR.silent_reads():
        assert int(s.o.count(po.encode(r)).max()) == 0 and int(s.o.count(po.encode(LR.revcomp(r))).max()) == 0
    for r in s.negatives:  # far below what a lane's spare dword collects: a sentinel for nearly every entry of every slot
        assert int(s.o.count(po.encode(r)).max()) < (len(r) - K + 1) // 2


def test_every_case_of_the_stop_fixture_occurs():
    owner, words = host_words(SR.Stops.N_BINS, SR.Stops.N_BLOCKS)
    s = SR.Stops(words)
    n = s.N
    stops = []
    for (mt, off, rev), read in zip(s.CASES, s.reads()):
        assert len(read) - K + 1 == n and s.forward(read) == n - mt + off, (mt, off, rev)
        assert [s.so_far(read, e) for e in (64, 128, 192)] == [rev] * 3, (mt, off, rev)
        # the rule fires at the edge mt itself exactly when the strand has counted no more than `off` by then
        want = mt if 0 <= off and rev <= off else (mt + 64 if mt + 64 < n else n)
        assert s.reverse_stop(read) == want, (mt, off, rev, s.reverse_stop(read))
        stops.append(want)
    assert set(stops) == {64, 128, 192, n}
    assert len({(mt, off) for mt, off, _ in s.CASES}) == 9


@pytest.mark.parametrize("n_bins,lines", ((2112, 1), (8192, 2)))
def test_the_overflow_kmer_stands_where_the_group_reads_claim(n_bins, lines):
    o = po.OracleIBF(n_bins, LR.H_FUNCS, K, SR.n_bits(n_bins, LR.CRAFT_BLOCKS))
    o.fill_synth(5)
    words = o.words()
    c = SR.CraftedGroups(n_bins, lines, words, SR.n_bits(n_bins, LR.CRAFT_BLOCKS))
    got, over, pc = census(c.o, K, LR.CRAFT_BLOCKS, n_bins)
    assert got == lines and [int(pc[r]) for r in c.ranks] == list(c.want)
    row = c.o.count(po.encode(c.OVER))
    assert int(row.sum()) == c.cap + 1 and row[0] == 1 and row[c.sat] == 1 and int(row.max()) == 1
    reads = c.group_reads()
    assert reads[0] == c.OVER and len(set(reads)) == len(reads)
    for places, read in zip(c.PLACES, reads[2:]):
        at = [i for i in range(len(read) - K + 1) if read[i:i + K] == c.OVER]
        assert set(places) <= set(at), (places, at)
    assert any(len([p for p in places if p // 8 == places[0] // 8]) == 2 for places in c.PLACES)
    assert {p % 8 for places in c.PLACES for p in places} >= {0, 7, 3}

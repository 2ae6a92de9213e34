"""What tests/test_gpu_pass_lists_edges.py relies on, checked on the oracle alone: every filter of tests/pass_lists_edges_rig.py takes the
slot size it claims (and is refused the smaller one), the bins set in every block count a strand's every k-mer -- 65 535 on the longest
strand the list form serves -- on both strands, the neighbour of the saturated low half lies just below it, the threshold 65 535 picks
exactly the saturated bins, every record list fits the cap the GPU tests use, and the filters of different k are what the mixed engine
needs."""
import functools

import numpy as np
import pytest

from oracle import pyoracle as po
from tests import list_scan_rig as SR
from tests import pass_lists_edges_rig as ER
from tests import pass_lists_rig as PL
from tests import row_lists_rig as LR
from tests.hits_rules import reduce_hits
from tests.locate_rules import reduce_locate
from tests.test_row_lists_cpu import census

K = ER.K


@functools.lru_cache(maxsize=None)
def edges(n_bins, lines):
    words = np.zeros(SR.n_bits(n_bins) // 64 + 8, dtype=np.uint64)  # (the payload's closing words)
    return ER.Edges(n_bins, lines, words)


@pytest.mark.parametrize("n_bins,lines", ER.GEOMETRIES)
def test_edge_filters_take_the_slot_size_they_claim(n_bins, lines):
    f = edges(n_bins, lines)
    got, over, pc = census(f.raw, K, SR.N_BLOCKS, n_bins)
    assert got == lines, over
    if lines > 1:
        assert over[lines.bit_length() - 2] > len(pc) >> 10, over  # the smaller slot size is refused
    assert over[lines.bit_length() - 1] >= 1                       # and some rows overflow this one: the strands pass overflow slots
    assert int(pc.min()) >= len(f.sat)                             # the saturated bins are in every row


def test_the_planted_bins_are_where_the_scan_can_go_wrong():
    assert ER.EVEN_SAT % 2 == 0 and ER.EVEN_SAT % 8 in (2, 4) and ER.LOW_EVEN % 2 == 0 and abs(ER.LOW_EVEN - ER.EVEN_SAT) > 512
    for n_bins, _ in ER.GEOMETRIES:
        if n_bins % 2:
            assert ER.pair_bins(n_bins) == (n_bins - 1,) and (n_bins - 1) % 2 == 0  # the last bin is a low half; its high half is pad
        else:
            a, b = ER.pair_bins(n_bins)
            assert (a, b) == (n_bins - 2, n_bins - 1) and a % 2 == 0 and a // 2 == b // 2  # the two halves of one dword
        assert max(ER.EVEN_SAT + 1, ER.LOW_EVEN) < n_bins - 2
    reads = ER.reads()
    assert [len(r) - K + 1 for r in reads] == list(ER.BIG) + [ER.MAX_KMERS] + list(ER.SHORT)
    assert ER.BIG[-1] == ER.MAX_KMERS == 0xFFFF and len(ER.over_read()) - K + 1 == 0x10000
    assert all(set(r) <= set("ACGT") for r in reads)


@pytest.mark.parametrize("n_bins,lines", ER.GEOMETRIES)
def test_saturated_bins_count_every_kmer_on_both_strands(n_bins, lines):
    f = edges(n_bins, lines)
    cap = 2 * n_bins
    for read in ER.reads():
        n = len(read) - K + 1
        o = po.encode(read)
        fwd, rev = f.o.count(o), f.o.count(po.revcomp(o))
        for c in (fwd, rev):
            assert [int(c[b]) for b in f.sat] == [n] * len(f.sat), (n, [int(c[b]) for b in f.sat])
            if n >= 1000:
                assert 0.9 * n < int(c[ER.EVEN_SAT + 1]) < n, (n, int(c[ER.EVEN_SAT + 1]))
                assert 0.05 * n < int(c[ER.LOW_EVEN]) < 0.25 * n
            others = np.delete(c.astype(np.int64), list(f.sat))
            assert int(others.max()) < n or n < 1000  # the maximum is the saturated bins', the lowest of them first
        m, b, s, _ = reduce_locate(fwd, rev, 1)
        assert (m, s) == (n, 0) and (b == f.sat[0] or n < 1000)
        at_top = reduce_hits(fwd, rev, ER.MAX_KMERS)
        if n == ER.MAX_KMERS:
            assert at_top == [(b, s, n) for b in f.sat for s in (0, 1)]
        else:
            assert at_top == []
        for t in (1, po.threshold(len(read), K, PL.R, PL.CONF)):
            assert len(reduce_hits(fwd, rev, t)) <= cap
    # one k-mer more: the saturated bins wrap to 0 and the neighbour of EVEN_SAT holds the maximum
    o = po.encode(ER.over_read())
    fwd, rev = f.o.count(o), f.o.count(po.revcomp(o))
    assert [int(fwd[b]) for b in f.sat] == [0] * len(f.sat) == [int(rev[b]) for b in f.sat]
    m, b, s, _ = reduce_locate(fwd, rev, 1)
    assert b == ER.EVEN_SAT + 1 and 0.9 * 65536 < m < 65536


def test_zero_threshold_reads_hit_every_bin():
    reads, n_zero, _ = PL.threshold_reads()
    assert n_zero == 2
    for n_bins, lines in ((2112, 1), ER.ODD):
        f = edges(n_bins, lines)
        for read in reads[:n_zero]:
            o = po.encode(read)
            assert len(reduce_hits(f.o.count(o), f.o.count(po.revcomp(o)), po.threshold(len(read), K, PL.R, PL.CONF))) == 2 * n_bins


def mixed():
    n5, blocks5 = ER.K5_GEOMETRY[:2]
    n7 = ER.K7_GEOMETRY[0]
    words5 = np.zeros(SR.n_bits(n5, blocks5) // 64 + 8, dtype=np.uint64)
    words7 = np.zeros(SR.n_bits(n7) // 64 + 8, dtype=np.uint64)
    return ER.MixedK(words5, words7, ER.make_narrow())


def test_mixed_k_fixture():
    m = mixed()
    n5, blocks5 = ER.K5_GEOMETRY[:2]
    got5, over5, _ = census(m.o5, ER.K5, blocks5, n5)
    got7, over7, _ = census(m.o7, K, SR.N_BLOCKS, ER.K7_GEOMETRY[0])
    assert (got5, got7) == (m.lines5, m.lines7), (over5, over7)
    assert (m.o5.kmer_size, m.o7.kmer_size, m.narrow.kmer_size) == (5, 7, 7)
    assert [len(r) for r in m.reads] == list(ER.MIXED_LENGTHS) + [70] and m.reads[-1].count("N") == 1
    for r in m.reads[1:3]:  # too short for the engine, countable by the k = 5 filter: planted, so that counting them would show
        c = m.o5.count(po.encode(r))
        assert K > len(r) >= ER.K5 and int(c[ER.BIN_5MERS]) == len(r) - ER.K5 + 1
    for o in m.filters():
        long = m.reads[-2]
        assert int(o.count(po.encode(long))[ER.BIN_LONG]) == len(long) - o.kmer_size + 1


@pytest.mark.parametrize("k", (5, 13))
def test_strand_reads(k):
    reads = ER.strand_reads(k)
    half = len(reads) // 2
    assert [len(r) - k + 1 for r in reads[:5]] == [1, 63, 64, 65, 129]
    assert set(reads[5]) == {"A"} and set(reads[6]) == {"T"} and len(reads[5]) - k + 1 > 64
    assert reads[half:] == [LR.revcomp(r) for r in reads[:half]]

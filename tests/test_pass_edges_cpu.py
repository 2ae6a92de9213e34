"""The cases of tests/pass_edges.py are what they claim to be -- on the oracle alone, no GPU.

tests/test_gpu_pass_edges.py compares the query passes with the oracle on these cases bit for bit; what makes that comparison worth
something is asserted here: the counts sit ON the edges of the counters (1023 with all ten planes set, 1024, the uint16_t wrap), the
maximum moves off the bin that matched everything once that bin wraps, the strands differ, the prefix rows fall across the wrap.

THE THRESHOLDS.  At 65 536 bases and at 65 536 + L0 bases (L0: a length whose threshold is 0) the reference computes
uint16_t(readlen) - k + 1 - ci.second with ci.second from the WHOLE length (src/IBF/IBFClassify.cpp:154-162), and the result is cut to
sixteen bits anyway: the cut of the length changes nothing, the threshold is the plain n - ci.second (15 959 and 15 991 at k = 13), and
neither a wrapped threshold nor a threshold of 0 exists at a length that S (70 100 bases) can give.  Both reads stay in the batch, and
what is asserted of them is what holds and what the passes meet there: that plain value, with SAT -- which matched every k-mer --
BELOW it after its wrap.  The threshold of 0 comes with the read of L0 bases that every batch carries (every bin is a hit on both
strands, in a batch of sixteen planes too), the wrapped threshold with k = 31, where the reads of the ten-plane batch have one above
65 000 and nothing is a hit."""
import numpy as np
import pytest

from oracle import pyoracle as po
from tests import pass_edges as PE
from tests import prefix_rules as PR

NAMES = sorted(PE.ALL)


def read_with(name, which, kmers):
    return PE.batch(which, PE.ALL[name][3])[1].index(kmers)


@pytest.mark.parametrize("name", NAMES)
def test_counts_sit_on_the_counter_edges(name):
    n_bins, _, h, k = PE.ALL[name]
    b = PE.bins_of(name)
    for which in PE.BATCHES:
        reads, kmers = PE.batch(which, k)
        cv = PE.counts(name, which)
        assert [c is None for c in cv] == [len(r) < k for r in reads]
        for c, n in zip(cv, kmers):
            if n is not None:  # SAT counts every k-mer on both strands, modulo 2^16
                assert int(c[0][b["SAT"]]) == n % 65536 and int(c[1][b["SAT"]]) == n % 65536, (name, which, n)
        top = max(int(max(c[0].max(), c[1].max())) for c in cv if c is not None)
        longest = max(n for n in kmers if n is not None)
        if which == "TEN":
            assert top == 1023 and longest == 1023 and max(len(r) for r in reads) == 1023 + k - 1
        elif which == "SWITCH":
            assert top == 1024 and longest == 1024 and max(len(r) for r in reads) == 1024 + k - 1
        else:
            assert longest == 70000 and top == 65535
    cv = PE.counts(name, "BIG")
    # at 65 536 k-mers SAT reads 0 and the maximum is NEAR's, on either strand below 65 536
    fwd, rev = cv[read_with(name, "BIG", 65536)]
    both = np.maximum(fwd, rev)
    assert int(both[b["SAT"]]) == 0 and int(np.argmax(both)) == b["NEAR"] and 60000 < int(both.max()) < 65536
    # at 70 000 NEAR has wrapped as well, to below HALF: the maximum belongs to a bin that matched a part of the read
    fwd, rev = cv[read_with(name, "BIG", 70000)]
    assert max(int(fwd[b["NEAR"]]), int(rev[b["NEAR"]])) < min(int(fwd[b["HALF"]]), int(rev[b["HALF"]]))
    assert int(fwd[b["SAT"]]) == 4464 and int(np.argmax(np.maximum(fwd, rev))) not in (b["SAT"], b["NEAR"])
    # REV: the reverse strand leads by 10 000 and more; the reverse complement of a read swaps the two
    for n in (65536, 70000):
        fwd, rev = cv[read_with(name, "BIG", n)]
        assert int(rev[b["REV"]]) - int(fwd[b["REV"]]) >= 10000, (name, n, int(fwd[b["REV"]]), int(rev[b["REV"]]))
    i, j = read_with(name, "BIG", 65537), len(PE.BIG) + 2
    assert PE.batch("BIG", k)[0][j] == PE.revcomp_str(PE.batch("BIG", k)[0][i])
    assert np.array_equal(cv[i][0], cv[j][1]) and np.array_equal(cv[i][1], cv[j][0])
    # the empty bins are empty
    planted = np.zeros(n_bins, bool)
    planted[list(b.values())] = True
    assert not fwd[~planted].any() and not rev[~planted].any()
    # the N rule matters to the reads with N
    n_read = len(PE.BIG) + 3
    assert "N" in PE.batch("BIG", k)[0][n_read]
    assert not np.array_equal(PE.counts(name, "BIG", 4)[n_read][1], cv[n_read][1])


@pytest.mark.parametrize("name", NAMES)
def test_thresholds_at_and_beyond_65536_bases(name):
    _, _, h, k = PE.ALL[name]
    b = PE.bins_of(name)
    reads, kmers = PE.batch("BIG", k)
    cv = PE.counts(name, "BIG")
    L0 = PE.zero_threshold_length(k)
    for i, L in ((len(PE.BIG), 65536), (len(PE.BIG) + 1, 65536 + (L0 or 130))):
        assert len(reads[i]) == L and kmers[i] == L - k + 1
        t = po.threshold(L, k, PE.R, PE.CONF)
        assert t == (L - k + 1 - po.calculate_ci(PE.R, k, L, PE.CONF)[1]) % 65536 and 0 < t < 32768  # (see the module's docstring)
        sat, near = int(cv[i][0][b["SAT"]]), int(cv[i][0][b["NEAR"]])
        assert sat == (L - k + 1) % 65536 and near >= t
        if L > 65536 + k:
            assert sat < t  # the bin that matched every k-mer is no hit: its count wrapped to below the threshold
    if k == 13:  # t == 0 in every batch, among reads of sixteen planes too
        assert L0 and po.threshold(L0, k, PE.R, PE.CONF) == 0
        for which in PE.BATCHES:
            assert PE.batch(which, k)[0].count(PE.sequence()[:L0]) == 1
    else:  # wrapped thresholds: the short reads of k = 31
        assert all(po.threshold(len(r), k, PE.R, PE.CONF) > 65000 for r in PE.batch("TEN", k)[0] if len(r) >= k)


@pytest.mark.parametrize("name", NAMES)
def test_hit_lists_fit_their_cap_and_reach_it(name):
    """with max_hits = 2 x n_bins no expected list is truncated, so truncation can hide nothing; the t == 0 read fills it"""
    n_bins, _, _, k = PE.ALL[name]
    cap = 2 * n_bins
    for which in PE.BATCHES:
        for mc in (0, 1, 65535):
            _, exp_n, _, status = PE.hits_expectation(name, which, 3, mc, cap, 0xAB)
            assert int(exp_n.max()) <= cap and (status == PE.RB_ERR_SHORT_READ).sum() == 3
            if mc == 0 and k == 13:
                assert int(exp_n.max()) == cap
            if mc == 65535:  # only SAT at exactly 65 535 k-mers, on both strands
                assert int(exp_n.sum()) == (2 if which == "BIG" else 0)


@pytest.mark.parametrize("name", ["lg0", "lg3", "w129", "lg3_h2", "w129_h4", "lg0_k31"])
def test_prefix_rows_fall_across_the_wrap(name):
    reads, cps, exp = PE.prefix_expectation(name, "WRAP")
    k = PE.ALL[name][3]
    assert len(reads[0]) == 70000 + k - 1 and len(reads[1]) == 32768 + k - 1 and cps[-1] == 80000
    m = exp["max_count"][0, :, 0].astype(np.int64)
    assert m[:4].tolist() == [1023, 1024, 32768, 65535] and m[4] < m[3] and m[6] < m[5] < 65535  # not monotone
    assert exp["max_count"][1, :, 0].tolist() == [1023, 1024] + [32768] * 6  # the shorter read repeats its last maximum
    assert exp["prefix_len"][0].tolist() == list(cps[:-1]) + [len(reads[0])] and (exp["status"] == PR.RB_OK).all()
    # the rows stitched from single checkpoints are prefix_rules.expected_batch's
    whole = PR.expected_batch(reads[1:], cps[:3], [PE.make_filter(name)], [], PR.MODE_CHECK_UNBLOCK, r=PE.R, conf=PE.CONF)
    for key in ("max_count", "decision", "best_target", "status", "prefix_len", "first_decided"):
        assert np.array_equal(whole[key], exp[key][1:, :3] if key != "first_decided" else exp[key][1:]), key


def test_dense_checkpoints_surround_the_wrap():
    cps = PE.wrap_checkpoints(13, dense=True)
    assert len(cps) == 64 and cps[0] == 65400 + 12 and cps[-1] == 65600 + 12 and list(cps) == sorted(set(cps))
    assert sum(c - 12 < 65536 for c in cps) > 20 and sum(c - 12 > 65536 for c in cps) > 15


def test_the_hits_layout_is_that_of_hits_rules():
    """hits_expectation lays the cached count vectors out as hits_rules.expected_arrays lays out counts of its own"""
    from tests.hits_rules import expected_arrays
    name, which = "lg1", "SWITCH"
    f = PE.make_filter(name)
    reads = PE.batch(which, f.kmer_size)[0]
    st = PE.status_of(reads, f.kmer_size)
    for mc, cap in ((0, 2 * f.n_bins), (1, 3), (1024, 5)):
        a = expected_arrays([f], reads, st == PE.RB_OK, cap, min_count=mc, r=PE.R, conf=PE.CONF, sentinel=0xAB)
        b = PE.hits_expectation(name, which, 3, mc, cap, 0xAB)
        assert a[0].tobytes() == b[0].tobytes() and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and np.array_equal(st, b[3])

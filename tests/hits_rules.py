"""The hits pass's rules (include/readbouncer_amd.h, rb_hits_out) restated in numpy over the per-bin count vectors of the two strands
-- the reduction the GPU tests apply to the oracle's `OracleIBF.count()` vectors, checked on hand-written vectors in
test_hits_cpu.py.  Test infrastructure: may use the oracle."""
import numpy as np

from oracle import pyoracle as po

HIT = np.dtype([("bin", "<u4"), ("count", "<u2"), ("strand", "u1"), ("reserved", "u1")])


def reduce_hits(fwd, rev, t):
    """fwd / rev: uint16 count per bin of the read and of its reverse complement; t: the threshold as the uint16 it is compared as.
    -> every (bin, strand, count) with count >= t, in rising (bin, strand) order"""
    fwd = np.asarray(fwd, dtype=np.uint16)
    rev = np.asarray(rev, dtype=np.uint16)
    assert fwd.shape == rev.shape and fwd.ndim == 1
    if not 0 <= t <= 0xFFFF:
        return []
    both = np.stack([fwd, rev], axis=1)  # [bin, strand]: C order is (bin, strand) order
    b, s = np.nonzero(both >= np.uint16(t))
    return [(int(x), int(y), int(both[x, y])) for x, y in zip(b, s)]


def distinct_bins(records):
    return len({b for b, _, _ in records})


def oracle_hits(filters, read, min_count=0, r=0.1, conf=0.95):
    """one read (ASCII str) against a list of OracleIBF -> per filter the full hit list, and the threshold used per filter
    (min_count > 0 replaces the decision threshold).  The caller applies the status rules (short read, chunking)."""
    o = po.encode(read)
    rc = po.revcomp(o)
    rows, thr = [], []
    for f in filters:
        t = min_count if min_count else po.threshold(len(o), f.kmer_size, r, conf)
        rows.append(reduce_hits(f.count(o), f.count(rc), t))
        thr.append(t)
    return rows, thr


def expected_arrays(filters, reads, ok, cap, min_count=0, r=0.1, conf=0.95, sentinel=0xAB):
    """what a call must leave behind for these reads (ok[i]: the item's status is RB_OK): the record buffer [n, nf, cap] over a
    sentinel fill, n_hits [n, nf], the profile (one entry per bin of every filter) and the full lists [i][j]"""
    n, nf = len(reads), len(filters)
    hits = np.frombuffer(bytes([sentinel]) * (n * nf * cap * 8), dtype=HIT).reshape(n, nf, cap).copy()
    n_hits = np.zeros((n, nf), np.uint32)
    starts = np.concatenate([[0], np.cumsum([f.n_bins for f in filters])]).astype(np.int64)
    profile = np.zeros(int(starts[-1]), np.uint64)
    lists = []
    for i, read in enumerate(reads):
        if not ok[i]:
            lists.append([[] for _ in filters])
            continue
        rows, _ = oracle_hits(filters, read, min_count, r, conf)
        lists.append(rows)
        for j, rec in enumerate(rows):
            n_hits[i, j] = len(rec)
            for q, (b, s, c) in enumerate(rec[:cap]):
                hits[i, j, q] = (b, c, s, 0)
            for b in {b for b, _, _ in rec}:
                profile[starts[j] + b] += 1
    return hits, n_hits, profile, lists

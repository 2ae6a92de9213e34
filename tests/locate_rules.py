"""The locate pass's rules (include/readbouncer_amd.h, rb_locate_out) restated in numpy over the per-bin count vectors of the two
strands -- the reduction the GPU tests apply to the oracle's `OracleIBF.count()` vectors, checked on hand-written vectors in
test_locate_cpu.py.  Test infrastructure: may use the oracle."""
import numpy as np

from oracle import pyoracle as po


def reduce_locate(fwd, rev, t):
    """fwd / rev: uint16 count per bin of the read and of its reverse complement; t: the uint16 threshold.
    -> (max_count, best_bin, best_strand, hit_bins)"""
    fwd = np.asarray(fwd, dtype=np.uint16)
    rev = np.asarray(rev, dtype=np.uint16)
    assert fwd.shape == rev.shape and fwd.ndim == 1
    both = np.maximum(fwd, rev)
    m = int(both.max()) if both.size else 0
    hits = int(np.count_nonzero((fwd >= np.uint16(t)) | (rev >= np.uint16(t)))) if 0 <= t <= 0xFFFF else 0
    if m == 0:
        return 0, -1, 0, hits
    b = int(np.flatnonzero(both == m)[0])  # the lowest bin at the maximum
    return m, b, 0 if int(fwd[b]) == m else 1, hits


def oracle_locate(filters, read, r=0.1, conf=0.95):
    """one read (ASCII str) against a list of OracleIBF -> per filter (max_count, best_bin, best_strand, hit_bins), and the threshold
    used per filter.  The caller applies the status rules (short read, chunking)."""
    o = po.encode(read)
    rc = po.revcomp(o)
    rows, thr = [], []
    for f in filters:
        t = po.threshold(len(o), f.kmer_size, r, conf)
        rows.append(reduce_locate(f.count(o), f.count(rc), t))
        thr.append(t)
    return rows, thr


def places_at_max(fwd, rev):
    """number of (bin, strand) places that hold the maximum (0 when the maximum is 0)"""
    m = max(int(np.max(fwd)), int(np.max(rev)))
    return 0 if m == 0 else int(np.count_nonzero(np.asarray(fwd) == m)) + int(np.count_nonzero(np.asarray(rev) == m))

"""The spans pass's rules (include/readbouncer_amd.h, rb_span / rb_spans_out) restated in numpy.  Everything comes from the oracle as
it stands: position p of a read is a strand-0 hit of a bin iff `OracleIBF.count()` of the k bases [p, p + k) alone has a 1 there, and
a strand-1 hit iff the count of `revcomp()` of those k bases has -- so the per-position sums are the two count vectors of the whole
read (checked in test_spans_cpu.py).  Records and mask words follow from the per-position booleans.  Test infrastructure: may use the
oracle."""
import numpy as np

from oracle import pyoracle as po

SPAN = np.dtype([(n, "<u4") for n in ("count", "first", "last", "run_start", "run_len", "covered")])
QUERY = np.dtype([("item", "<u4"), ("bin", "<u4")])
NONE = 0xFFFFFFFF
RB_OK, RB_ERR_INVALID_ARG = 0, 8


def position_hits(f, read, bins):
    """read: ASCII str; bins: bin numbers of filter f -> bool [2, len(bins), n_kmers]: [s, i, p] = position p is a hit of bins[i] on
    strand s, under the oracle's current N rule (po.set_revcomp_of_n)"""
    o = po.encode(read)
    k = f.kmer_size
    n = max(len(o) - k + 1, 0)
    bins = np.asarray(bins, dtype=np.int64)
    out = np.zeros((2, len(bins), n), dtype=bool)
    for p in range(n):
        w = o[p:p + k].copy()
        out[0, :, p] = f.count(w)[bins] == 1
        out[1, :, p] = f.count(po.revcomp(w))[bins] == 1
    return out


def record(hits, k):
    """hits: bool per position -> (count, first, last, run_start, run_len, covered) as rb_span defines them"""
    hits = np.asarray(hits, dtype=bool)
    idx = np.flatnonzero(hits)
    if len(idx) == 0:
        return (0, NONE, NONE, NONE, 0, 0)
    breaks = np.flatnonzero(np.diff(idx) != 1)
    starts = np.concatenate([[0], breaks + 1])
    ends = np.concatenate([breaks, [len(idx) - 1]])
    lens = ends - starts + 1
    j = int(np.argmax(lens))  # the first of equally long runs: the lowest
    cov = np.zeros(len(hits) + k - 1, dtype=bool)
    for s, e in zip(starts, ends):
        cov[idx[s]:idx[e] + k] = True
    return (len(idx), int(idx[0]), int(idx[-1]), int(idx[starts[j]]), int(lens[j]), int(cov.sum()))


def mask_words(hits, n_words):
    """hits: bool per position -> u64 [n_words]: bit p & 63 of word p >> 6; positions at or beyond 64 n_words are left out"""
    hits = np.asarray(hits, dtype=bool)
    bits = np.zeros(64 * n_words, dtype=bool)
    m = min(len(hits), len(bits))
    bits[:m] = hits[:m]
    return np.packbits(bits, bitorder="little").view("<u8").astype(np.uint64) if n_words else np.zeros(0, np.uint64)


def as_queries(pairs):
    q = np.zeros(len(pairs), dtype=QUERY)
    if len(pairs):
        a = np.asarray(pairs, dtype=np.uint32).reshape(-1, 2)
        q["item"], q["bin"] = a[:, 0], a[:, 1]
    return q


def expected_arrays(f, items, item_status, queries, n_mask_words):
    """what a call must leave behind: items = the bases of every work item (ASCII str, already chunked), item_status = u8 per item
    by the locate pass's rules, queries = QUERY records -> spans [nq, 2], mask [nq, 2, n_mask_words], n_kmers [nq], status [nq]"""
    nq = len(queries)
    spans = np.zeros((nq, 2), dtype=SPAN)
    for name in ("first", "last", "run_start"):
        spans[name] = NONE
    mask = np.zeros((nq, 2, n_mask_words), dtype=np.uint64)
    n_kmers = np.zeros(nq, dtype=np.uint32)
    status = np.zeros(nq, dtype=np.uint8)
    by_item = {}
    for qi, (item, b) in enumerate(zip(queries["item"].tolist(), queries["bin"].tolist())):
        if item >= len(items) or b >= f.n_bins:
            status[qi] = RB_ERR_INVALID_ARG
        elif item_status[item] != RB_OK:
            status[qi] = item_status[item]
        else:
            by_item.setdefault(item, []).append((qi, b))
    for item, lst in by_item.items():
        hits = position_hits(f, items[item], sorted({b for _, b in lst}))
        col = {b: i for i, b in enumerate(sorted({b for _, b in lst}))}
        for qi, b in lst:
            n_kmers[qi] = hits.shape[2]
            for s in range(2):
                h = hits[s, col[b]]
                spans[qi, s] = record(h, f.kmer_size)
                mask[qi, s] = mask_words(h, n_mask_words)
    return spans, mask, n_kmers, status

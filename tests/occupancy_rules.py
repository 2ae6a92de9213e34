"""Per-bin occupancy of an IBF from its HOST image, in numpy: the yardstick of rb_dibf_bin_occupancy (never the code under test).
The file layout stores block b as the W = ceil(n_bins / 64) words [b * W, (b + 1) * W); bin j of block b is bit j % 64 of word
b * W + j // 64.  Bits at or beyond n_bins in the last word column, and every word behind the blocks (tail, metadata), are not bins."""
import numpy as np


def bin_occupancy(words, n_bins, n_blocks):
    """words: uint64 array holding at least n_blocks * W words in file layout -> uint64 [n_bins], blocks whose bit for the bin is set"""
    W = (n_bins + 63) // 64
    m = np.ascontiguousarray(words[:n_blocks * W], dtype=np.uint64).reshape(n_blocks, W)
    out = np.zeros(W * 64, dtype=np.uint64)
    for c in range(W):  # column by column: one [n_blocks, 64] bit matrix at a time
        col = np.ascontiguousarray(m[:, c]).astype("<u8")
        bits = np.unpackbits(col.view(np.uint8).reshape(n_blocks, 8), axis=1, bitorder="little")
        out[c * 64:(c + 1) * 64] = bits.sum(axis=0, dtype=np.uint64)
    return out[:n_bins]


def summary(bits, n_blocks, n_hash, max_fp=0.01):
    """the integer figures of rb_bin_occupancy_summary, and the doubles computed the way the header states them"""
    bits = np.asarray(bits, dtype=np.uint64)
    ne = np.flatnonzero(bits)
    s = {"n_bins": len(bits), "n_blocks": n_blocks, "n_hash": n_hash, "bits_total": int(bits.sum(dtype=np.uint64)),
         "empty_bins": int(len(bits) - len(ne)), "max_bits": 0, "max_bin": 0, "min_bits": 0, "min_bin": 0,
         "mean_load": 0.0, "max_load": 0.0, "mean_fpr": 0.0, "max_fpr": 0.0, "bins_over_max_fp": 0}
    if len(ne):
        load = bits[ne].astype(np.float64) / float(n_blocks)
        fpr = load ** float(n_hash)
        s.update(max_bits=int(bits.max()), max_bin=int(np.argmax(bits)), min_bits=int(bits[ne].min()), min_bin=int(ne[np.argmin(bits[ne])]),
                 mean_load=float(s["bits_total"]) / float(n_blocks) / len(ne), max_load=float(bits.max()) / float(n_blocks),
                 mean_fpr=float(np.sum(fpr.astype(np.longdouble)) / len(ne)), max_fpr=(float(bits.max()) / float(n_blocks)) ** float(n_hash),
                 bins_over_max_fp=int(np.count_nonzero(fpr > max_fp)))
    return s

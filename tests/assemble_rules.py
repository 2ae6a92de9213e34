"""Assembling a filter from bins of others, restated in numpy from HOST images: the yardstick of rb_dibf_assemble / rb_dibf_select_bins
(never the code under test), and the plans the tests put through it.

The file layout stores block b of a filter as the W = ceil(n_bins / 64) words [b * W, (b + 1) * W); bin j of block b is bit j % 64 of
word b * W + j // 64.  A plan is a list with one list of (filter, bin) pairs per out bin.  The model
  1. unpacks each source's words into an [n_blocks, n_bins] bit matrix,
  2. ORs the columns each out bin's list names,
  3. packs little-endian into n_blocks x ceil(n_out / 64) words,
  4. appends the zero tail and metadata words up to (n_bits + 256 + 63) / 64 (a host image carries its metadata only in a file)."""
import numpy as np


def unpack(words, n_bins, n_blocks):
    """uint64 words in file layout (at least n_blocks * W of them) -> bool [n_blocks, n_bins]"""
    W = (n_bins + 63) // 64
    m = np.ascontiguousarray(words[:n_blocks * W], dtype="<u8").reshape(n_blocks, W)
    bits = np.unpackbits(m.view(np.uint8).reshape(n_blocks, W * 8), axis=1, bitorder="little")
    return bits[:, :n_bins].astype(bool)


def pack(bits):
    """bool [n_blocks, n_bins] -> uint64 [n_blocks * W] in file layout, bits at or beyond n_bins zero"""
    n_blocks, n_bins = bits.shape
    W = (n_bins + 63) // 64
    full = np.zeros((n_blocks, W * 64), dtype=np.uint8)
    full[:, :n_bins] = bits
    return np.packbits(full, axis=1, bitorder="little").view("<u8").reshape(-1).astype(np.uint64)


def n_words(n_out, n_blocks):
    """payload words of the assembled filter's host image, tail and metadata included"""
    n_bits = n_blocks * ((n_out + 63) // 64) * 64
    return (n_bits + 256 + 63) // 64


def assemble_bits(matrices, plan):
    """matrices: one bool [n_blocks, n_bins_s] per source -> bool [n_blocks, len(plan)]"""
    n_blocks = matrices[0].shape[0]
    out = np.zeros((n_blocks, len(plan)), dtype=bool)
    for j, refs in enumerate(plan):
        for f, b in refs:
            out[:, j] |= matrices[f][:, b]
    return out


def assemble_words(sources, plan):
    """sources: [(words, n_bins, n_blocks)], all of one n_blocks -> uint64 [n_words] of the assembled filter's host image"""
    n_blocks = sources[0][2]
    assert all(s[2] == n_blocks for s in sources) and len(plan) > 0
    payload = pack(assemble_bits([unpack(*s) for s in sources], plan))
    out = np.zeros(n_words(len(plan), n_blocks), dtype=np.uint64)
    out[:len(payload)] = payload
    return out


# ---- plans: n = bins of source 0 (sizes = bins of every source where several are used) ----------------------------------------------
def identity(n):
    return [[(0, b)] for b in range(n)]


def reversed_order(n):
    return [[(0, n - 1 - b)] for b in range(n)]


def drop_every_third(n):
    return [[(0, b)] for b in range(n) if b % 3 != 2]


def empty_first(n, k=3):
    return [[] for _ in range(k)] + identity(n)


def empty_middle(n, k=3):
    p = identity(n)
    return p[:n // 2] + [[] for _ in range(k)] + p[n // 2:]


def empty_last(n, k=3):
    return identity(n) + [[] for _ in range(k)]


def all_empty(n):
    return [[] for _ in range(n)]


def duplicated_refs(n):
    """every list names its bin twice and its neighbour once: a repeated ref is allowed and changes nothing"""
    return [[(0, b), (0, b), (0, (b + 1) % n), (0, b)] for b in range(n)]


def groups_of(n, g):
    return [[(0, b) for b in range(j, min(j + g, n))] for j in range(0, n, g)]


def all_into_one(n):
    return [[(0, b) for b in range(n)]]


def interleaved_join(sizes):
    """out bins take bins of the sources in turn (source 0 bin 0, source 1 bin 0, ...) until every source has given all of its bins"""
    plan = []
    for b in range(max(sizes)):
        for f, n in enumerate(sizes):
            if b < n:
                plan.append([(f, b)])
    return plan


def truncated(plan, n_out):
    """the first n_out out bins of a plan, padded with empty bins when it is shorter"""
    return [list(l) for l in plan[:n_out]] + [[] for _ in range(max(0, n_out - len(plan)))]


SINGLE_SOURCE = {
    "identity": identity,
    "reversed": reversed_order,
    "drop_every_third": drop_every_third,
    "empty_first": empty_first,
    "empty_middle": empty_middle,
    "empty_last": empty_last,
    "all_empty": all_empty,
    "duplicated_refs": duplicated_refs,
    "groups_of_3": lambda n: groups_of(n, 3),
    "groups_of_8": lambda n: groups_of(n, 8),
    "all_into_one": all_into_one,
}


# ---- oracle-built sources and the oracle-side rebuild (test infrastructure: the oracle is the yardstick) --------------------------------
def oracle_source(seed, n_bins, n_blocks, h=3, k=13, seq_len=120):
    """an oracle filter with a sequence of its own in every bin -> (OracleIBF, [ascii sequence per bin])"""
    from oracle import pyoracle as po
    from tests import helpers as H
    rng = np.random.default_rng(seed)
    f = po.OracleIBF(n_bins, h, k, 64 * ((n_bins + 63) // 64) * n_blocks)
    assert f.n_blocks == n_blocks
    seqs = [H.random_dna(rng, seq_len) for _ in range(n_bins)]
    for b, s in enumerate(seqs):
        f.insert(po.encode(s), b)
    return f, seqs


def oracle_rebuild(seq_lists, plan, n_blocks, h=3, k=13):
    """what the builder writes: each ref's own sequence inserted into the out bin it is routed to, at the same n_blocks -> OracleIBF"""
    from oracle import pyoracle as po
    n_out = len(plan)
    f = po.OracleIBF(n_out, h, k, 64 * ((n_out + 63) // 64) * n_blocks)
    assert f.n_blocks == n_blocks
    for j, refs in enumerate(plan):
        for src, b in refs:
            f.insert(po.encode(seq_lists[src][b]), j)
    return f


def source_triple(f):
    return (f.words(), f.n_bins, f.n_blocks)

"""Cases that put the query passes (locate, hits, spans, prefixes) at the edges of their counters: the builder, on the oracle alone.

A filter here is made by the oracle on the host with bits written straight into `OracleIBF.words()` ([n_blocks, W]), so that the count of
a bin on ANY read is known by construction and reaches the top plane of ten (1023), the switch to sixteen (1024) and the uint16_t wrap
(65535, 65536 -> 0, 65537 -> 1, 70000 -> 4464):
  SAT   n_bins - 1, its bit set in every block: the count is the read's k-mer count on both strands, modulo 65 536.  The last valid bit
        before the pad bits;
  NEAR  bin 5 at bit load 0.99: about 0.97 n with three hash functions -- the maximum where SAT has wrapped, below HALF once it has
        wrapped itself;
  HALF  a bin of a middle word column (of the second slice's one column on w129) at load 0.8; LOW at load 0.5;
  REV   gets insert() of the reverse complement of the first 40 012 bases of S: high on strand 1 only.
Every other bin is empty.  S is one random sequence of 70 100 bases and every read a prefix of it (plus the reverse complement of one,
one with 1 % N and the three reads shorter than k per batch).

THE BLOCK COUNTS.  REV needs its 40 000 k-mers to leave the bin well below saturation: with m k-mers inserted into B blocks by h hash
functions the bit load is L = 1 - exp(-h m / B), a read's forward count of the bin is about n L^h and its reverse count exceeds that by
m (1 - L^h).  Below B = 50 000 blocks that difference cannot reach the 10 000 that test_pass_edges_cpu.py asks for (at B = 1021 the bin
is full and both strands count n), so the filters have 65 521 (prime: Barrett reduction) or 65 536 (a mask) blocks.  The widest is
68 MB on the host; the oracle takes a fraction of a second per read and strand.

Expectations are cached per (geometry, batch, N rule) and come from the rule modules (locate_rules, hits_rules, prefix_rules,
spans_rules) over the oracle's count vectors.  Test infrastructure: may use the oracle; nothing here looks at the product."""
import functools
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from oracle import pyoracle as po
from tests import prefix_rules as PR
from tests.hits_rules import HIT, reduce_hits
from tests.locate_rules import reduce_locate

R, CONF = 0.1, 0.95
RB_OK, RB_ERR_SHORT_READ = PR.RB_OK, PR.RB_ERR_SHORT_READ
THREADS = 16

# name -> (n_bins, n_blocks, n_hash, k)
GEOMETRIES = {
    "lg0": (56, 65521, 3, 13),          # LG 0
    "lg1": (100, 65536, 3, 13),         # LG 1
    "lg2": (243, 65521, 3, 13),         # LG 2
    "lg3": (300, 65536, 3, 13),         # LG 3, with idle lanes
    "lg4": (1000, 65521, 3, 13),        # LG 4
    "lg5": (2040, 65536, 3, 13),        # LG 5
    "lg6": (4090, 65521, 3, 13),        # LG 6, one word per lane
    "w129": (8200, 65521, 3, 13),       # two words per lane, two slices, the second holding one column
    "lg3_h2": (300, 65521, 2, 13),      # run-time hash
    "w129_h4": (8200, 65536, 4, 13),    # run-time hash
    "lg0_k31": (56, 65521, 3, 31),      # k = 31
}
# the run-time hash build of the geometries that have none above: the smallest filter of each block shape
HASH_EXTRA = {
    "lg0_h2": (56, 65536, 2, 13), "lg1_h4": (100, 65521, 4, 13), "lg2_h2": (243, 65536, 2, 13), "lg4_h4": (1000, 65536, 4, 13),
    "lg5_h2": (2040, 65521, 2, 13), "lg6_h4": (4090, 65536, 4, 13),
}
ALL = dict(GEOMETRIES, **HASH_EXTRA)
NEAR, LOW, REV = 5, 9, 12
REV_BASES = 40012
S_LEN = 70100
TEN = (511, 512, 513, 1023)                           # k-mers of the reads of the ten-plane batch
BIG = (32767, 32768, 65535, 65536, 65537, 70000)      # ... of the batch up to and across the uint16_t wrap


def revcomp_str(s):
    return s[::-1].translate(str.maketrans("ACGT", "TGCA"))


@functools.lru_cache(maxsize=None)
def sequence():
    rng = np.random.default_rng(70100)
    return "".join(np.array(list("ACGT"))[rng.integers(0, 4, size=S_LEN)])


def bins_of(name):
    """the planted bins of a geometry: dict SAT / NEAR / HALF / LOW / REV -> bin number"""
    n_bins = ALL[name][0]
    W = (n_bins + 63) // 64
    return {"SAT": n_bins - 1, "NEAR": NEAR, "HALF": 64 * (W // 2 if W <= 128 else 128) + 3, "LOW": LOW, "REV": REV}


@functools.lru_cache(maxsize=None)
def make_filter(name):
    n_bins, n_blocks, h, k = ALL[name]
    W = (n_bins + 63) // 64
    f = po.OracleIBF(n_bins, h, k, 64 * W * n_blocks)
    assert f.n_blocks == n_blocks and f.bin_width == W
    b = bins_of(name)
    assert len(set(b.values())) == 5 and max(b.values()) < n_bins
    f.insert(po.encode(revcomp_str(sequence()[:REV_BASES])), b["REV"])
    w = f.words()[:n_blocks * W].reshape(n_blocks, W)
    rng = np.random.default_rng(sum(name.encode()))
    for key, load in (("SAT", 2.0), ("NEAR", 0.99), ("HALF", 0.8), ("LOW", 0.5)):
        col, bit = divmod(b[key], 64)
        w[:, col] |= (rng.random(n_blocks) < load).astype(np.uint64) << np.uint64(bit)
    return f


def zero_threshold_length(k):
    """L0: the largest length below 400 whose oracle threshold is 0; None where there is none (k = 31: a threshold below 0, which the
    reference's int16_t -> uint16_t conversion turns into one above 65 000)"""
    zero = [L for L in range(k, 400) if po.threshold(L, k, R, CONF) == 0]
    return zero[-1] if zero else None


def with_n(s, seed):
    a = np.frombuffer(s.encode(), dtype=np.uint8).copy()
    a[np.random.default_rng(seed).random(len(a)) < 0.01] = ord("N")
    return a.tobytes().decode()


@functools.lru_cache(maxsize=None)
def batch(which, k):
    """-> (reads, kmers): kmers[i] = the k-mer count of read i where the read is a planned prefix of S, else None"""
    S = sequence()
    short = ["ACGT", "A" * (k - 1), ""]
    pre = lambda n: S[:n + k - 1]
    L0 = zero_threshold_length(k)
    zero = [S[:L0]] if L0 else []  # t == 0: every bin is a hit on both strands, whatever the planes of the batch
    if which in ("TEN", "SWITCH"):
        ns = TEN + ((1024,) if which == "SWITCH" else ())
        reads = [pre(n) for n in ns] + [revcomp_str(pre(1023)), with_n(pre(900), 1)] + zero + short
        return tuple(reads), tuple(ns) + (None,) * (len(reads) - len(ns))
    assert which == "BIG"
    L0 = L0 or 130
    reads = [pre(n) for n in BIG] + [S[:65536], S[:65536 + L0], revcomp_str(pre(65537)), with_n(pre(66000), 2)] + zero + short
    return tuple(reads), tuple(BIG) + (65536 - k + 1, 65536 + L0 - k + 1) + (None,) * (len(reads) - len(BIG) - 2)


BATCHES = ("TEN", "SWITCH", "BIG")


def status_of(reads, k):
    return np.array([RB_OK if len(r) >= k else RB_ERR_SHORT_READ for r in reads], np.uint8)


def _map(fn, items):
    with ThreadPoolExecutor(THREADS) as ex:  # (the oracle's calls release the interpreter lock)
        return list(ex.map(fn, items))


@functools.lru_cache(maxsize=None)
def counts(name, which, n_rule=3):
    """the oracle's two count vectors of every read of the batch: [(fwd, rev) or None for a read shorter than k]; shared, read-only"""
    f = make_filter(name)
    reads, _ = batch(which, f.kmer_size)
    prev = po.set_revcomp_of_n(n_rule)
    try:
        def one(r):
            if len(r) < f.kmer_size:
                return None
            o = po.encode(r)
            return f.count(o), f.count(po.revcomp(o))
        return tuple(_map(one, reads))
    finally:
        po.set_revcomp_of_n(prev)


def thresholds(name, which):
    k = ALL[name][3]
    return [po.threshold(len(r), k, R, CONF) for r in batch(which, k)[0]]


@functools.lru_cache(maxsize=None)
def locate_expectation(name, which, n_rule=3):
    """dict of arrays like Engine.locate for a one-filter engine, through locate_rules.reduce_locate"""
    cv, thr = counts(name, which, n_rule), thresholds(name, which)
    n = len(cv)
    out = {"max_count": np.zeros((n, 1), np.uint16), "best_bin": np.full((n, 1), -1, np.int32), "best_strand": np.zeros((n, 1), np.uint8),
           "hit_bins": np.zeros((n, 1), np.uint32), "status": np.zeros(n, np.uint8)}
    for i, c in enumerate(cv):
        if c is None:
            out["status"][i] = RB_ERR_SHORT_READ
            continue
        out["max_count"][i, 0], out["best_bin"][i, 0], out["best_strand"][i, 0], out["hit_bins"][i, 0] = reduce_locate(c[0], c[1], thr[i])
    return out


def hits_expectation(name, which, n_rule, min_count, cap, sentinel, ids=None):
    """what a hits call must leave behind, as hits_rules.expected_arrays lays it out, through hits_rules.reduce_hits over the cached
    count vectors -> (hits [n, 1, cap] over the sentinel, n_hits [n, 1], profile [n_bins], status [n])"""
    cv, thr = counts(name, which, n_rule), thresholds(name, which)
    sel = range(len(cv)) if ids is None else [int(i) for i in ids]
    n, n_bins = len(sel), ALL[name][0]
    hits = np.frombuffer(bytes([sentinel]) * (n * cap * 8), dtype=HIT).reshape(n, 1, cap).copy()
    n_hits = np.zeros((n, 1), np.uint32)
    profile = np.zeros(n_bins, np.uint64)
    status = np.zeros(n, np.uint8)
    for row, i in enumerate(sel):
        if cv[i] is None:
            status[row] = RB_ERR_SHORT_READ
            continue
        rec = reduce_hits(cv[i][0], cv[i][1], min_count if min_count else thr[i])
        n_hits[row, 0] = len(rec)
        if rec[:cap]:
            a = np.array(rec[:cap], dtype=np.int64)
            hits["bin"][row, 0, :len(a)], hits["strand"][row, 0, :len(a)], hits["count"][row, 0, :len(a)] = a[:, 0], a[:, 1], a[:, 2]
            hits["reserved"][row, 0, :len(a)] = 0
        profile[np.array(sorted({b for b, _, _ in rec}), dtype=np.int64)] += 1
    return hits, n_hits, profile, status


def prefix_rows(f, reads, checkpoints, mode, n_rule=3, **kw):
    """prefix_rules.expected_batch with the (read, checkpoint) rows computed side by side: every row is expected_rows of ONE
    checkpoint, first_decided is prefix_rules.first_decided over a read's rows"""
    prev = po.set_revcomp_of_n(n_rule)
    try:
        jobs = [(i, p) for i in range(len(reads)) for p in range(len(checkpoints))]
        rows = _map(lambda j: PR.expected_rows(reads[j[0]], (checkpoints[j[1]],), [f], [], mode, r=R, conf=CONF, **kw), jobs)
    finally:
        po.set_revcomp_of_n(prev)
    n, P = len(reads), len(checkpoints)
    out = {key: np.stack([rows[i * P + p][key][0] for i in range(n) for p in range(P)]).reshape((n, P) + rows[0][key].shape[1:])
           for key in ("max_count", "decision", "best_target", "status", "prefix_len", "ok")}
    out["first_decided"] = np.array([PR.first_decided(out["decision"][i], out["status"][i]) for i in range(n)], dtype=np.uint32)
    return out


def kmer_checkpoints(kmers, k):
    return tuple(n + k - 1 for n in kmers)


# checkpoints (k-mers) of the three prefix cases; the last one of each lies beyond every read of its batch
TEN_CPS = (511, 512, 513, 1023, 1500)
SWITCH_CPS = (511, 512, 513, 1023, 1024, 1500)
WRAP_CPS = (1023, 1024, 32768, 65535, 65536, 65537, 70000)  # + 80 000 bases
WRAP_READS = (5, 1)  # of BIG: the 70000-k-mer read and the 32768-k-mer read


def wrap_checkpoints(k, dense=False):
    if dense:  # 64 checkpoints over 65 400 .. 65 600 k-mers: every lane of the wave holds one around the wrap
        return tuple(int(x) + k - 1 for x in np.unique(np.linspace(65400, 65600, 64).astype(np.int64)))
    return kmer_checkpoints(WRAP_CPS, k) + (80000,)


@functools.lru_cache(maxsize=None)
def prefix_expectation(name, case, mode=PR.MODE_CHECK_UNBLOCK, n_rule=3):
    """case: "TEN", "SWITCH", "WRAP" or "DENSE" -> (reads, checkpoints, expected arrays); shared, read-only"""
    f = make_filter(name)
    k = f.kmer_size
    if case in ("TEN", "SWITCH"):
        reads = batch(case, k)[0]
        cps = kmer_checkpoints(TEN_CPS if case == "TEN" else SWITCH_CPS, k)
    else:
        big = batch("BIG", k)[0]
        reads = tuple(big[i] for i in WRAP_READS)
        cps = wrap_checkpoints(k, dense=case == "DENSE")
    return reads, cps, prefix_rows(f, reads, cps, mode, n_rule)

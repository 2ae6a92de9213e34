"""What the resume pass (rb_resume_batch / rb_resume_batch_device / rb_resume_counts) must return, from the oracle alone.

A slot's HISTORY is the chunks committed to it since its last RB_RESUME_FIRST.  The row of a feed is the oracle's answer for the
concatenation history + chunk as ONE read -- prefix_rules.expected_rows(concat, [len(concat)], ...) states it for all three modes,
max_len = max_total_len included -- and the slot's counters are f.count(encode(concat)) and f.count(revcomp(encode(concat))), zero
while the concatenation is shorter than k.  An item the call refuses (a slot number at or beyond n_slots, a chunk longer than
max_chunk_len, a total beyond max_total_len: RB_ERR_INVALID_ARG; chunk_start beyond the read: RB_ERR_BAD_CHUNK) has decision 0,
best_target -1, total_len 0 and leaves its slot as it was.  `Model` keeps the histories as a caller would.  Nothing here looks at the
product."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from oracle import pyoracle as po
from tests import prefix_rules as PR

FIRST, PEEK = 1, 2  # RB_RESUME_FIRST, RB_RESUME_PEEK (include/readbouncer_amd.h)
RB_OK, RB_ERR_SHORT_READ, RB_ERR_BAD_CHUNK, RB_ERR_INVALID_ARG = PR.RB_OK, PR.RB_ERR_SHORT_READ, PR.RB_ERR_BAD_CHUNK, PR.RB_ERR_INVALID_ARG
KEYS = ("max_count", "decision", "best_target", "status", "total_len")
THREADS = 16


def stitched(seen, chunk, k):
    """what a feed counts: the last k - 1 bases seen so far + the new chunk"""
    return (seen[-(k - 1):] if k > 1 else "") + chunk


def expected_row(concat, deplete, target, mode, r=0.1, conf=0.95, max_total_len=None):
    """-> dict of one row: max_count u16[nf], decision, best_target, status, total_len, ok"""
    rows = PR.expected_rows(concat, [len(concat)], deplete, target, mode, r=r, conf=conf, max_len=max_total_len)
    out = {key: rows[key][0] for key in ("max_count", "decision", "best_target", "status", "ok")}
    out["total_len"] = np.uint32(len(concat))
    return out


def refused_row(nf, status):
    return {"max_count": np.zeros(nf, np.uint16), "decision": np.uint8(0), "best_target": np.int32(-1), "status": np.uint8(status),
            "total_len": np.uint32(0), "ok": np.bool_(False)}


def expected_counts(concat, f):
    """-> u16 [2, n_bins]: seqan::count of the concatenation and of its reverse complement"""
    if len(concat) < f.kmer_size:
        return np.zeros((2, f.n_bins), np.uint16)
    o = po.encode(concat)
    return np.stack([f.count(o), f.count(po.revcomp(o))]).astype(np.uint16)


class Model:
    """the slots as their caller knows them: slot -> concatenation of the chunks committed since the last FIRST"""

    def __init__(self, n_slots, max_chunk_len, max_total_len):
        self.n_slots, self.max_chunk_len, self.max_total_len = n_slots, max_chunk_len, max_total_len
        self.seen = {}

    def verdict(self, slot, chunk, flags):
        """-> (status the call gives the item before it counts, the concatenation the row stands for)"""
        if slot >= self.n_slots or len(chunk) > self.max_chunk_len:
            return RB_ERR_INVALID_ARG, None
        concat = ("" if flags & FIRST else self.seen.get(slot, "")) + chunk
        if len(concat) > self.max_total_len:
            return RB_ERR_INVALID_ARG, None
        return RB_OK, concat

    def feed(self, items, deplete, target, mode, r=0.1, conf=0.95, bad_chunk=()):
        """items: [(slot, chunk, flags)]; bad_chunk: indices whose descriptor names a chunk_start beyond the read.  -> the rows stacked
        like Resume.feed, plus ok; commits what the call commits"""
        nf = len(deplete) + len(target)
        plan = [(RB_ERR_BAD_CHUNK, None) if i in bad_chunk else self.verdict(*it) for i, it in enumerate(items)]

        def row(p):
            return refused_row(nf, p[0]) if p[1] is None else expected_row(p[1], deplete, target, mode, r, conf, self.max_total_len)
        with ThreadPoolExecutor(THREADS) as ex:  # (the oracle's calls release the interpreter lock)
            rows = list(ex.map(row, plan))
        for (slot, _, flags), (_, concat) in zip(items, plan):
            if concat is not None and not flags & PEEK:
                self.seen[slot] = concat
        return {key: np.stack([x[key] for x in rows]) for key in KEYS + ("ok",)}

    def counts(self, slot, f):
        return expected_counts(self.seen.get(slot, ""), f)

    def total(self, slot):
        return len(self.seen.get(slot, ""))


def assert_same(got, exp, what):
    """every output bit for bit; max_count wherever the row's status is RB_OK"""
    for key in ("status", "total_len", "decision", "best_target"):
        if not np.array_equal(got[key], exp[key]):
            bad = np.argwhere(got[key] != exp[key])[:5]
            raise AssertionError("%s: %s differs at %s: got %s, expected %s" % (what, key, bad.tolist(), got[key][tuple(bad.T)].tolist(),
                                                                               exp[key][tuple(bad.T)].tolist()))
    g, e = got["max_count"][exp["ok"]], exp["max_count"][exp["ok"]]
    if not np.array_equal(g, e):
        bad = np.argwhere(g != e)[:5]
        raise AssertionError("%s: max_count differs at (ok row, filter) %s: got %s, expected %s" % (what, bad.tolist(), g[tuple(bad.T)].tolist(),
                                                                                                  e[tuple(bad.T)].tolist()))


def assert_counts(got, exp, what):
    if not np.array_equal(got, exp):
        bad = np.argwhere(got != exp)[:8]
        raise AssertionError("%s: counts differ at (strand, bin) %s: got %s, expected %s" % (what, bad.tolist(), got[tuple(bad.T)].tolist(),
                                                                                           exp[tuple(bad.T)].tolist()))

"""What the prefix pass (rb_prefix_batch / rb_prefix_batch_device) must return, from the oracle alone.

Row (read, checkpoint c) is the oracle's answer for the ASCII prefix read[:c]: per filter max(count(o).max(), count(revcomp(o)).max()),
and the decision of the mode -- po.check_unblock, po.classify_any over deplete + target, or po.classify_read_chunks with ONE chunk of
chunk_length = c (of the whole prefix where the read ends before c: the device call looks at min(c, length) bases, where the
reference's file loop would skip the read as too short) -- with the status that call returns.  best_target is
Read::classify(TargetFilters) on the prefix (po.classify_best), -1 when that raises or there is no target filter, as everywhere in
the suite (tests/decide_cells.py).  Nothing here looks at the product."""
import numpy as np

from oracle import pyoracle as po

MODE_CHECK_UNBLOCK, MODE_CLASSIFY_CHUNK, MODE_CLASSIFY_ANY = 0, 1, 2
RB_OK, RB_ERR_SHORT_READ, RB_ERR_BAD_CHUNK, RB_ERR_INVALID_ARG = 0, 2, 6, 8  # include/readbouncer_amd.h


def first_decided(decision, status):
    """lowest p with status RB_OK and decision != 0; len(decision) when there is none"""
    for p, (d, s) in enumerate(zip(decision, status)):
        if s == RB_OK and d != 0:
            return p
    return len(decision)


def expected_rows(read, checkpoints, deplete, target, mode, r=0.1, conf=0.95, chunk_start=0, chunk_length=0, max_len=None):
    """-> dict: max_count u16[P, nf], decision u8[P], best_target i32[P], status u8[P], prefix_len u32[P], first_decided int, and
    ok bool[P] = rows whose max_count the header promises (status RB_OK).  chunk_start / chunk_length / max_len as in rb_batch_desc."""
    filters = list(deplete) + list(target)
    P, nf = len(checkpoints), len(filters)
    out = {"max_count": np.zeros((P, nf), np.uint16), "decision": np.zeros(P, np.uint8), "best_target": np.full(P, -1, np.int32),
           "status": np.zeros(P, np.uint8), "prefix_len": np.zeros(P, np.uint32)}
    bad = chunk_start > len(read)
    body = "" if bad else (read[chunk_start:chunk_start + chunk_length] if chunk_length else read[chunk_start:])
    for p, c in enumerate(checkpoints):
        prefix = body[:c]
        out["prefix_len"][p] = len(prefix)
        if bad:
            out["status"][p] = RB_ERR_BAD_CHUNK
            continue
        if max_len is not None and len(prefix) > max_len:
            out["status"][p] = RB_ERR_INVALID_ARG
            continue
        o = po.encode(prefix)
        rc = po.revcomp(o)
        for j, f in enumerate(filters):
            fwd, rev = f.count(o), f.count(rc)
            out["max_count"][p, j] = max(int(fwd.max()), int(rev.max()))
        if target:
            st, b = po.classify_best(list(target), o, r, conf)
            out["best_target"][p] = b if st == po.OK else -1
        if mode == MODE_CHECK_UNBLOCK:
            st, d = po.check_unblock(list(deplete), list(target), o, r, conf)
        elif mode == MODE_CLASSIFY_ANY:
            st, found = po.classify_any(filters, o, r, conf)
            d = 1 if found else 0
        else:
            res = po.classify_read_chunks(list(deplete), list(target), prefix, len(prefix), 1, r, conf)
            st, d = res["status"], 1 if res["classified"] else 0
        out["status"][p] = st
        out["decision"][p] = d if st == po.OK else 0
    out["first_decided"] = first_decided(out["decision"], out["status"])
    out["ok"] = out["status"] == RB_OK
    return out


def expected_batch(reads, checkpoints, deplete, target, mode, **kw):
    """the rows of every read stacked like Engine.prefixes: [n, P, ...] and first_decided [n]"""
    rows = [expected_rows(rd, checkpoints, deplete, target, mode, **kw) for rd in reads]
    out = {key: np.stack([x[key] for x in rows]) for key in ("max_count", "decision", "best_target", "status", "prefix_len", "ok")}
    out["first_decided"] = np.array([x["first_decided"] for x in rows], dtype=np.uint32)
    return out


def assert_same(got, exp, what):
    """every output bit for bit; max_count wherever the row's status is RB_OK"""
    for key in ("status", "prefix_len", "decision", "best_target", "first_decided"):
        if not np.array_equal(got[key], exp[key]):
            bad = np.argwhere(got[key] != exp[key])[:5]
            raise AssertionError("%s: %s differs at %s: got %s, expected %s" % (what, key, bad.tolist(), got[key][tuple(bad.T)].tolist(),
                                                                               exp[key][tuple(bad.T)].tolist()))
    g, e = got["max_count"][exp["ok"]], exp["max_count"][exp["ok"]]
    if not np.array_equal(g, e):
        bad = np.argwhere(g != e)[:5]
        raise AssertionError("%s: max_count differs at (ok row, filter) %s: got %s, expected %s" % (what, bad.tolist(), g[tuple(bad.T)].tolist(),
                                                                                                  e[tuple(bad.T)].tolist()))

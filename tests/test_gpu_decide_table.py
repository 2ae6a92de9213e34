"""The decision kernel against the oracle over its whole decision table (tests/decide_cells.py: cells, filter sets, designed reads).
`decide_one` (readbouncer_amd/csrc/rb_kernels.hip) runs in K2, in the latency kernel's fold and behind rb_decide_device /
rb_decide_device_parts; every path gets the designed reads, and the expected decision, status and best target always come from the
oracle on the reads (batch_check_unblock, classify_read_chunks with one chunk covering the read, classify_any, classify_best).
Exact equality everywhere.  The filters are built on the device and seen by the oracle through download().

Paths, as the ledger names them:  a  rb_decide_device on the ORACLE's raw maxima (no count kernel involved: a failure is K2's);
b  rb_decide_device_parts on splits of those maxima;  d  the throughput form end to end (more than 2 048 reads);  e  the latency
form and its fold (1, 7, 64 reads);  f  the host call on the whole set.  (c: the status arms.)  test_every_decision_cell_was_reached
asserts that each of a, b, d, e, f compared reads in every REQUIRED cell."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import pyoracle as po
from readbouncer_amd import capi
from tests import decide_cells as DC

_LEDGER = {}  # path -> {cell: reads compared}
SETS = sorted(DC.FILTER_SETS)
assert (capi.RB_MODE_CHECK_UNBLOCK, capi.RB_MODE_CLASSIFY_CHUNK, capi.RB_MODE_CLASSIFY_ANY) == DC.MODES


class Ctx:
    """one filter set on the device, its designed reads, and what the oracle says about them (computed once, never changed)"""

    def __init__(self, name):
        import torch
        self.torch, self.dev = torch, torch.device("cuda:0")
        self.name = name
        self.ks, self.nd, self.nt = DC.set_ks(name)
        self.nf = self.nd + self.nt
        refs, _ = DC.references(name)
        self.filters, self.views, self._keep = [], [], []
        for (nb, h, k, bits), ref in zip(DC.geometry(name), refs):
            d = capi.DeviceIBF.create(0, nb, h, k, bits)
            d.add_sequence(ref, DC.FRAG)
            host = d.download()
            i = host.info
            self.views.append(po.OracleIBF.wrap(i["n_bins"], i["n_hash"], i["kmer_size"], i["n_bits"], host.words()))
            self.filters.append(d)
            self._keep.append(host)
        self.odep, self.otgt = self.views[:self.nd], self.views[self.nd:]
        self.eng = capi.Engine(0, self.filters[:self.nd], self.filters[self.nd:])
        self.reads = list(DC.designed_reads(name))
        self.n = len(self.reads)
        self.buf, self.offs, self.lens = DC.pack(self.reads)
        self.encoded = [po.encode(r) for r in self.reads]
        self.raw = np.ascontiguousarray(DC.oracle_raw(self.views, self.buf, self.offs, self.lens))
        self.max_len = int(self.lens.max())
        self.t_buf, self.t_offs, self.t_lens = self.up(self.buf), self.up(self.offs), self.up(self.lens)
        self.t_raw = self.up(self.raw)

    def up(self, a):
        a = np.ascontiguousarray(a)
        signed = {np.dtype(np.uint16): np.int16, np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}.get(a.dtype)
        return self.torch.from_numpy(a.view(signed) if signed else a).to(self.dev)

    @functools.lru_cache(maxsize=None)
    def expect(self, r, mode):
        dec, st, best = DC.oracle_expect(self.odep, self.otgt, self.reads, self.encoded, self.buf, self.offs, self.lens, r, mode)
        for a in (dec, st, best):
            a.setflags(write=False)
        return dec, st, best

    @functools.lru_cache(maxsize=None)
    def cells(self, r, mode):
        return tuple(DC.cells_of_batch(self.raw, self.lens, self.ks, r, mode, self.nd, self.nt))

    def poisoned(self, n):
        t = self.torch
        return (t.full((n,), -9, dtype=t.int32, device=self.dev), t.full((n,), 9, dtype=t.uint8, device=self.dev),
                t.full((n,), 9, dtype=t.uint8, device=self.dev))

    def check(self, got_best, got_dec, got_st, r, mode, where, idx=None, path=None):
        """got_*: numpy arrays (None: not returned) for reads idx (default: all, in order)"""
        dec, st, best = self.expect(r, mode)
        idx = np.arange(self.n) if idx is None else np.asarray(idx)
        for what, got, want in (("decision", got_dec, dec), ("status", got_st, st), ("best_target", got_best, best)):
            if got is None:
                continue
            bad = np.nonzero(got != want[idx])[0]
            assert len(bad) == 0, "%s %s: %s differs from the oracle for %d reads, first %s" % (
                self.name, where, what, len(bad),
                [(int(idx[i]), int(self.lens[idx[i]]), self.raw[idx[i]].tolist(), int(got[i]), int(want[idx[i]]),
                  DC.describe(self.cells(r, mode)[idx[i]])) for i in bad[:4]])
        if path is not None and got_dec is not None and got_st is not None:
            cells = self.cells(r, mode)
            DC.ledger_add(_LEDGER, path, [cells[i] for i in idx])


@functools.lru_cache(maxsize=None)
def ctx(name):
    pytest.importorskip("torch")
    return Ctx(name)


def decide(c, t_table, r, mode, n_parts=1, stride=0, outs=(True, True, True), max_len=None):
    """K2 alone on a table of maxima -> (best, decision, status) as numpy, None where the output was passed as NULL"""
    t_best, t_dec, t_st = c.poisoned(c.n)
    ptr = [t.data_ptr() if on else None for t, on in zip((t_best, t_dec, t_st), outs)]
    c.torch.cuda.synchronize()
    kw = dict(error_rate=r, mode=mode, d_best=ptr[0], d_decision=ptr[1], d_status=ptr[2])
    ml = c.max_len if max_len is None else max_len
    if n_parts == 1 and stride == 0:
        c.eng.decide_device(t_table.data_ptr(), c.t_lens.data_ptr(), c.n, ml, **kw)
    else:
        c.eng.decide_device_parts(t_table.data_ptr(), n_parts, stride, c.t_lens.data_ptr(), c.n, ml, **kw)
    c.torch.cuda.synchronize()
    got = [t.cpu().numpy() for t in (t_best, t_dec, t_st)]
    for g, on, poison in zip(got, outs, (-9, 9, 9)):
        if not on:
            assert (g == poison).all(), "an output passed as NULL was written"
    return [g if on else None for g, on in zip(got, outs)]


@pytest.mark.parametrize("name", SETS)
def test_decide_device_on_the_oracles_maxima(name):
    """path a"""
    c = ctx(name)
    for r in DC.RATES:
        for mode in DC.MODES:
            best, dec, st = decide(c, c.t_raw, r, mode)
            c.check(best, dec, st, r, mode, "rb_decide_device r=%g mode=%d" % (r, mode), path="a")
    # every optional output as NULL, one at a time: the others are what they were
    for mode in DC.MODES:
        for off in range(3):
            outs = tuple(i != off for i in range(3))
            best, dec, st = decide(c, c.t_raw, 0.1, mode, outs=outs)
            c.check(best, dec, st, 0.1, mode, "rb_decide_device with output %d NULL, mode=%d" % (off, mode))


@pytest.mark.parametrize("name", SETS)
def test_decide_device_parts_on_splits_of_the_oracles_maxima(name):
    """path b: every (read, filter) maximum sits in one part chosen at random, the other parts hold values from [0, max] (zero and
    equality included); with a padded stride the gap between the parts is 0xFFFF, which must never be read as a count"""
    c = ctx(name)
    rng = np.random.default_rng(SETS.index(name) + 77)
    cells = c.n * c.nf
    for n_parts in (2, 3, 4):
        for stride in (cells, cells + 37):
            table = np.full(n_parts * stride, 0xFFFF, dtype=np.uint16)
            owner = rng.integers(0, n_parts, size=(c.n, c.nf))
            for q in range(n_parts):
                part = rng.integers(0, c.raw.astype(np.int64) + 1).astype(np.uint16)
                part[owner == q] = c.raw[owner == q]
                table[q * stride:q * stride + cells] = part.reshape(-1)
            assert np.array_equal(np.max([table[q * stride:q * stride + cells] for q in range(n_parts)], axis=0), c.raw.reshape(-1))
            t_table = c.up(table)
            for r in DC.RATES:
                for mode in DC.MODES:
                    best, dec, st = decide(c, t_table, r, mode, n_parts, stride)
                    c.check(best, dec, st, r, mode, "rb_decide_device_parts n_parts=%d stride=%d r=%g mode=%d" % (n_parts, stride, r, mode), path="b")
            best, dec, st = decide(c, t_table, 0.1, capi.RB_MODE_CHECK_UNBLOCK, n_parts, stride, outs=(False, True, False))
            c.check(best, dec, st, 0.1, capi.RB_MODE_CHECK_UNBLOCK, "rb_decide_device_parts with NULL outputs")
    # overlapping parts are refused
    t_table = c.up(np.zeros(2 * cells, dtype=np.uint16))
    with pytest.raises(capi.RBError) as ei:
        c.eng.decide_device_parts(t_table.data_ptr(), 2, cells - 1, c.t_lens.data_ptr(), c.n, c.max_len)
    assert ei.value.status == capi.RB_ERR_INVALID_ARG
    with pytest.raises(capi.RBError) as ei:
        c.eng.decide_device_parts(t_table.data_ptr(), 0, cells, c.t_lens.data_ptr(), c.n, c.max_len)
    assert ei.value.status == capi.RB_ERR_INVALID_ARG


@pytest.mark.parametrize("name", ["d1", "d1t1", "d2t2", "d13t15t13"])
def test_status_arms(name):
    """path c: an understated max_len marks the longer reads alone (RB_ERR_INVALID_ARG, decision 0, best -1); a chunk start beyond a
    read marks it RB_ERR_BAD_CHUNK through on-GPU chunking while the others decide on their remaining bases"""
    c = ctx(name)
    understated = int(np.sort(c.lens)[-6]) - 1
    too_long = c.lens > understated
    assert 0 < too_long.sum() < c.n // 2
    for mode in DC.MODES:
        best, dec, st = decide(c, c.t_raw, 0.1, mode, max_len=understated)
        assert (st[too_long] == capi.RB_ERR_INVALID_ARG).all() and (dec[too_long] == 0).all() and (best[too_long] == -1).all()
        ok = np.nonzero(~too_long)[0]
        c.check(best[ok], dec[ok], st[ok], 0.1, mode, "rb_decide_device with max_len understated", idx=ok)
    start = 100
    bad = c.lens < start
    tails = [rd[start:] for rd in c.reads]
    tb, to, tl = DC.pack(tails)
    enc = [po.encode(t) for t in tails]
    assert bad.sum() > 10 and (~bad).sum() > 10
    for mode in DC.MODES:
        e_dec, e_st, e_best = DC.oracle_expect(c.odep, c.otgt, tails, enc, tb, to, tl, 0.1, mode)
        t_best, t_dec, t_st = c.poisoned(c.n)
        c.torch.cuda.synchronize()
        c.eng.classify_device_ex(c.t_buf.data_ptr(), c.t_offs.data_ptr(), c.t_lens.data_ptr(), c.n, c.max_len, chunk_start=start,
                                 mode=mode, d_best=t_best.data_ptr(), d_decision=t_dec.data_ptr(), d_status=t_st.data_ptr())
        c.torch.cuda.synchronize()
        best, dec, st = t_best.cpu().numpy(), t_dec.cpu().numpy(), t_st.cpu().numpy()
        assert (st[bad] == capi.RB_ERR_BAD_CHUNK).all() and (dec[bad] == 0).all() and (best[bad] == -1).all(), mode
        assert np.array_equal(dec[~bad], e_dec[~bad]) and np.array_equal(st[~bad], e_st[~bad]) and np.array_equal(best[~bad], e_best[~bad]), mode


@pytest.mark.parametrize("name", SETS)
def test_throughput_form_end_to_end(name):
    """path d: rb_classify_batch_device with more than 2 048 reads (the set repeated), every mode, the raw maxima asked for and not,
    the early-decision mode on and off"""
    c = ctx(name)
    reps = 2049 // c.n + 1
    n = reps * c.n
    assert n > 2048
    buf, offs, lens = DC.pack(c.reads * reps)
    t_buf, t_offs, t_lens = c.up(buf), c.up(offs), c.up(lens)
    idx = np.tile(np.arange(c.n), reps)
    try:
        for early in (0, 1):
            c.eng.set_early_decision(early)
            for r in DC.RATES:
                for mode in DC.MODES:
                    for with_max in (True, False):
                        t_best, t_dec, t_st = c.poisoned(n)
                        t_mc = c.torch.zeros((n, c.nf), dtype=c.torch.int16, device=c.dev)
                        c.torch.cuda.synchronize()
                        c.eng.classify_device(t_buf.data_ptr(), t_offs.data_ptr(), t_lens.data_ptr(), n, c.max_len, error_rate=r, mode=mode,
                                              d_maxcount=t_mc.data_ptr() if with_max else None, d_best=t_best.data_ptr(),
                                              d_decision=t_dec.data_ptr(), d_status=t_st.data_ptr())
                        c.torch.cuda.synchronize()
                        where = "rb_classify_batch_device early=%d r=%g mode=%d maxima=%s" % (early, r, mode, with_max)
                        if with_max:
                            assert np.array_equal(t_mc.cpu().numpy().view(np.uint16), c.raw[idx]), where
                        c.check(t_best.cpu().numpy(), t_dec.cpu().numpy(), t_st.cpu().numpy(), r, mode, where, idx=idx,
                                path="d" if early == 0 and with_max else None)
    finally:
        c.eng.set_early_decision(0)


@pytest.mark.parametrize("name", SETS)
def test_latency_form_and_fold(name):
    """path e: rb_classify_batch with micro-batches -- 64 reads for every set (latency kernel, then K2; a one-filter engine folds the
    decision into the latency kernel), and for the one-filter engines also 7 reads and ONE read (the folded decision and its
    completion word)"""
    c = ctx(name)
    sizes = (1, 7, 64) if c.nf == 1 else (64,)
    try:
        for size in sizes:
            c.eng.set_completion_word(size == 1)
            for r in DC.RATES:
                for mode in DC.MODES:
                    lo = hi = 0
                    while hi < c.n:
                        lo, hi = hi, min(c.n, hi + size)
                        while hi < c.n and c.lens[lo:hi].max() == 0:  # (a call of empty reads only is not part of this table)
                            hi += 1
                        mc, best, dec, st = c.eng.classify(c.buf, c.offs[lo:hi], c.lens[lo:hi], error_rate=r, mode=mode)
                        assert np.array_equal(mc, c.raw[lo:hi])
                        c.check(best, dec, st, r, mode, "rb_classify_batch of %d reads r=%g mode=%d" % (size, r, mode), idx=np.arange(lo, hi),
                                path="e" if size == 64 else None)
    finally:
        c.eng.set_completion_word(False)


@pytest.mark.parametrize("name", SETS)
def test_host_call_on_the_whole_set(name):
    """path f: rb_classify_batch on the whole set in one call, every mode -- the set repeated until the call carries more than 8 MiB of
    reads and offsets, which is where the host call leaves the pinned micro-batch path for the large one"""
    c = ctx(name)
    total = int(c.lens.sum())
    reps = (8 << 20) // (total + 16 * c.n) + 2
    buf = np.tile(c.buf[:total], reps)
    lens = np.tile(c.lens, reps)
    offs = np.zeros(len(lens), dtype=np.uint64)
    offs[1:] = np.cumsum(lens[:-1], dtype=np.uint64)
    assert int(lens.sum()) + 16 * len(lens) > (8 << 20)
    idx = np.tile(np.arange(c.n), reps)
    raw = c.raw[idx]
    for r in DC.RATES:
        for mode in DC.MODES:
            mc, best, dec, st = c.eng.classify(buf, offs, lens, error_rate=r, mode=mode)
            assert np.array_equal(mc, raw)
            c.check(best, dec, st, r, mode, "rb_classify_batch of %d reads r=%g mode=%d" % (len(lens), r, mode), idx=idx, path="f")
    dec, st = c.eng.decide(buf, offs, lens, error_rate=0.1)
    c.check(None, dec, st, 0.1, capi.RB_MODE_CHECK_UNBLOCK, "rb_classify_batch without maxima and best target", idx=idx)


def test_every_decision_cell_was_reached():
    """every REQUIRED cell (tests/decide_cells.py) was compared with the oracle, three reads or more, on each of the paths; fails (never
    skips) when the tests that fill the ledger did not run"""
    required = DC.REQUIRED
    for path in "abdef":
        assert path in _LEDGER, "the tests of path %s did not run" % path
        missing = DC.ledger_missing(_LEDGER, path, required)
        assert not missing, "path %s: %d of %d required cells compared fewer than %d reads:\n%s" % (
            path, len(missing), len(required), DC.MIN_READS_PER_CELL, "\n".join("%3d  %s" % (k, DC.describe(x)) for x, k in missing))
        assert not set(_LEDGER[path]) & set(DC.IMPOSSIBLE)

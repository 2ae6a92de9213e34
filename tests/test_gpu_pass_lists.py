"""Locate and hits from a filter's list table (rb_engine_set_pass_lists; rb_pass_lists.hip, ibf_locate_lists_kernel and
ibf_hits_lists_kernel) against the oracle, bit for bit, through the C ABI and the existing reductions (tests/locate_rules.py,
tests/hits_rules.py).  Every case asserts that Engine.plan_pass names the list form at the fixture's slot size -- a call that silently ran
the plain form would prove nothing -- and that the same call under RB_PASS_LISTS_OFF on the same engine returns the same bytes.  The
fixtures are tests/list_scan_rig.py's, tests/row_lists_rig.py's and tests/pass_lists_rig.py's (k = 7: tables of 4^7 slots); what the
new ones claim of themselves is asserted without a GPU in tests/test_pass_lists_cpu.py.  No tolerance, no assertion on elapsed time."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import pyoracle as po
from readbouncer_amd import capi
from tests import helpers as H
from tests import list_scan_rig as SR
from tests import pass_lists_rig as PL
from tests import row_lists_rig as LR
from tests import test_gpu_hits as GH
from tests import test_gpu_list_scan as LS
from tests import test_gpu_locate as GL
from tests import test_gpu_row_table as RT
from tests.hits_rules import expected_arrays

K, R, CONF = PL.K, PL.R, PL.CONF
OFF, CURRENT, BUILD = capi.RB_PASS_LISTS_OFF, capi.RB_PASS_LISTS_CURRENT, capi.RB_PASS_LISTS_BUILD
NT_DEFAULT = 512 << 20


def lists_engine(devs, mode=CURRENT):
    eng = capi.Engine(0, list(devs), [])
    eng.set_pass_lists(mode)
    return eng


def plan_lines(eng, max_len, nf=1):
    return [eng.plan_pass(j, max_len)["list_lines"] for j in range(nf)]


def same_bytes(a, b, what):
    for key in a:
        if a[key] is not None and isinstance(a[key], np.ndarray):
            assert a[key].tobytes() == b[key].tobytes(), (what, key)


def run_both(eng, filters, reads, lines, label, min_count=1, cap=None, mode=CURRENT, ids=None):
    """locate and hits of `reads` on the list form (the plan says so: `lines` per filter) against the oracle, then the same calls
    with the setting off: the same bytes -> (locate's expectation, the expected n_hits)"""
    nf = len(filters)
    cap = cap or 2 * max(f.n_bins for f in filters)
    buf, offs, lens = H.pack_reads(list(reads))
    max_len = int(lens.max())
    exp, _, _ = GL.oracle_rows(filters, reads, R, CONF)
    ok = exp["status"] == capi.RB_OK
    exp_hits, exp_n, exp_prof, _ = expected_arrays(filters, reads, ok, cap, min_count=min_count, r=R, conf=CONF, sentinel=GH.SENT)
    assert int(exp_n.max()) <= cap
    if ids is not None:
        sel = np.array(ids, dtype=np.int64)
        exp = {key: v[sel] for key, v in exp.items()}
        starts = np.concatenate([[0], np.cumsum([f.n_bins for f in filters])])
        exp_prof = np.zeros_like(exp_prof)
        for i in sel:
            for j in range(nf):
                for b in {int(h["bin"]) for h in exp_hits[i, j, :exp_n[i, j]]}:
                    exp_prof[starts[j] + b] += 1
        exp_hits, exp_n = exp_hits[sel], exp_n[sel]
    n = len(exp["status"])
    rid = None if ids is None else np.array(ids, dtype=np.uint32)
    got = {}
    for setting in (mode, OFF):
        eng.set_pass_lists(setting)
        assert plan_lines(eng, max_len, nf) == (list(lines) if setting != OFF else [0] * nf), (label, setting)
        loc = eng.locate(buf, offs, lens, read_ids=rid, error_rate=R, significance=CONF)
        GL.assert_same(loc, exp, "%s locate, setting %d" % (label, setting))
        prof = np.zeros(len(exp_prof), np.uint64)
        hit = eng.hits(buf, offs, lens, read_ids=rid, error_rate=R, significance=CONF, min_count=min_count, max_hits=cap, bin_reads=prof,
                       hits=GH.sentinel_hits(n, nf, cap))
        GH.check(hit, exp_hits, exp_n, exp["status"], "%s hits, setting %d" % (label, setting))
        assert np.array_equal(prof, exp_prof), (label, setting)
        got[setting] = (loc, hit, prof)
    eng.set_pass_lists(mode)
    same_bytes(got[mode][0], got[OFF][0], label)
    same_bytes(got[mode][1], got[OFF][1], label)
    assert got[mode][2].tobytes() == got[OFF][2].tobytes()
    return exp, exp_n


# ------------------------------------------------------------------------------------------------ 1. where the maximum sits
@pytest.mark.parametrize("n_bins,lines", SR.GEOMETRIES)
def test_where_the_maximum_sits(n_bins, lines):
    """SR.Planted: a read per bin at the edges of the counters and of a lane's scan pieces, on either strand, and strands of 1 to 71
    k-mers; hits at min_count 1 with room for every bin is seqan::count in sparse form -- every counter of both strands, and nothing
    from the pad counters or the spare dwords -- temporal and non-temporal"""
    d, f = LS.resident(lambda words, info: SR.Planted(n_bins, lines, words), n_bins, SR.N_BLOCKS, lines)
    eng = lists_engine([d])
    reads = f.reads() + f.tail_reads()
    for nt in (0, 1):
        eng.set_nt_threshold(0 if nt else NT_DEFAULT)
        exp, _ = run_both(eng, [f.o], reads, [lines], ("planted", n_bins, lines, nt))
    assert exp["best_bin"][:len(f.bins), 0].tolist() == f.bins and exp["best_strand"][:len(f.bins), 0].tolist() == [0] * len(f.bins)
    assert exp["best_strand"][len(f.bins):2 * len(f.bins), 0].tolist() == [1] * len(f.bins)
    eng.destroy()
    d.free()


# ------------------------------------------------------------------------------------------------ 2. ties and strands
@pytest.mark.parametrize("n_bins,lines", PL.TIE_GEOMETRIES)
def test_ties_and_strands(n_bins, lines):
    d, f = LS.resident(lambda words, info: PL.Ties(n_bins, lines, words), n_bins, SR.N_BLOCKS, lines)
    eng = lists_engine([d])
    reads = f.reads()
    exp, exp_n = run_both(eng, [f.o], reads, [lines], ("ties", n_bins), min_count=PL.N_KMERS)
    assert list(zip(exp["best_bin"][:, 0].tolist(), exp["best_strand"][:, 0].tolist())) == f.want()
    assert exp["max_count"][:, 0].tolist() == [PL.N_KMERS] * len(reads)
    same = reads.index(f.same)  # one hit bin, two records
    assert int(exp_n[same, 0]) == 2
    eng.destroy()
    d.free()


# ------------------------------------------------------------------------------------------------ 3. thresholds
@pytest.mark.parametrize("n_bins,lines", ((PL.OddBins.N_BINS, PL.OddBins.LINES), (2112, 1)))
def test_threshold_zero_and_wrapped(n_bins, lines):
    """t == 0 counts every existing bin -- exactly n_bins at an odd bin count, whose last counter dword is half pad (4091), and at a
    rounded-up cnt_dwords (2112) -- and a wrapped t none"""
    reads, n_zero, n_wrapped = PL.threshold_reads()
    assert n_zero and n_wrapped  # lengths of both kinds exist below 400 at k = 7, r = 0.1 (tests/test_pass_lists_cpu.py)
    make = (lambda words, info: PL.OddBins(words)) if n_bins % 2 else (lambda words, info: SR.Sparse(n_bins, lines, words))
    d, f = LS.resident(make, n_bins, SR.N_BLOCKS, lines)
    eng = lists_engine([d])
    exp, exp_n = run_both(eng, [f.o], reads, [lines], ("thresholds", n_bins), min_count=0)
    assert exp["hit_bins"][:n_zero, 0].tolist() == [n_bins] * n_zero and exp_n[:n_zero, 0].tolist() == [2 * n_bins] * n_zero
    assert not exp["hit_bins"][n_zero:n_zero + n_wrapped].any() and not exp_n[n_zero:n_zero + n_wrapped].any()
    eng.destroy()
    d.free()


# ------------------------------------------------------------------------------------------------ 4. caps
def test_caps_and_optional_outputs():
    n_bins, lines = 2112, 1
    d, f = LS.resident(lambda words, info: SR.Planted(n_bins, lines, words), n_bins, SR.N_BLOCKS, lines)
    eng = lists_engine([d])
    reads = f.reads()[:6]
    buf, offs, lens = H.pack_reads(reads)
    assert plan_lines(eng, int(lens.max())) == [lines]
    ok = np.ones(len(reads), bool)
    st = np.zeros(len(reads), np.uint8)
    _, full_n, exp_prof, lists = expected_arrays([f.o], reads, ok, 1, min_count=1, r=R, conf=CONF, sentinel=GH.SENT)
    n_hits = int(full_n[0, 0])
    assert n_hits > 3
    for cap in (1, n_hits - 1, n_hits, n_hits + 5):
        exp_hits, exp_n, _, _ = expected_arrays([f.o], reads, ok, cap, min_count=1, r=R, conf=CONF, sentinel=GH.SENT)
        got = eng.hits(buf, offs, lens, error_rate=R, significance=CONF, min_count=1, max_hits=cap, hits=GH.sentinel_hits(len(reads), 1, cap))
        GH.check(got, exp_hits, exp_n, st, "cap %d" % cap)  # whole buffers over the sentinel: order, truncation, untouched slots
        assert np.array_equal(exp_n, full_n)
    # no record buffer (max_hits 0 and any), and the profile alone, accumulating over two calls
    for cap in (0, 7):
        got = eng.hits(buf, offs, lens, error_rate=R, significance=CONF, min_count=1, max_hits=cap)
        assert np.array_equal(got["n_hits"], full_n)
    prof = np.zeros(n_bins, np.uint64)
    for _ in range(2):
        eng.hits(buf, offs, lens, error_rate=R, significance=CONF, min_count=1, max_hits=0, bin_reads=prof)
    assert np.array_equal(prof, 2 * exp_prof)
    eng.destroy()
    d.free()


# ------------------------------------------------------------------------------------------------ 5. nothing hit
@pytest.mark.parametrize("n_bins,lines", ((2112, 1), (4090, 2), (8192, 4)))
def test_nothing_hit(n_bins, lines):
    d, f = LS.resident(lambda words, info: SR.Sparse(n_bins, lines, words), n_bins, SR.N_BLOCKS, lines)
    eng = lists_engine([d])
    reads = f.reads()
    exp, exp_n = run_both(eng, [f.o], reads, [lines], ("sparse", n_bins))
    silent = slice(len(f.negatives), len(reads))
    assert not exp["max_count"][silent].any() and (exp["best_bin"][silent] == -1).all() and not exp["best_strand"][silent].any()
    assert not exp_n[silent].any()
    eng.destroy()
    d.free()


# ------------------------------------------------------------------------------------------------ 6. overflow slots
@pytest.mark.parametrize("n_bins,lines", ((2112, 1), (8192, 2)))
def test_overflow_slots(n_bins, lines):
    d, c = LS.resident(lambda words, info: SR.CraftedGroups(n_bins, lines, words, info["n_bits"]), n_bins, LR.CRAFT_BLOCKS, lines, seed=5)
    eng = lists_engine([d])
    run_both(eng, [c.o], c.group_reads(), [lines], ("groups", n_bins))
    eng.destroy()
    d.free()


# ------------------------------------------------------------------------------------------------ 7. who takes which item
def chunk_expectation(o, reads, start, length, max_len, cap):
    """rb_locate_out / rb_hits_out for the chunk [start, start + length) of every read (length 0: to the end)"""
    chunks = [(r[start:start + length] if length else r[start:]) for r in reads]
    exp, _, _ = GL.oracle_rows([o], chunks, R, CONF)
    for i, r in enumerate(reads):
        bad = capi.RB_ERR_BAD_CHUNK if start > len(r) else (capi.RB_ERR_INVALID_ARG if len(chunks[i]) > max_len else None)
        if bad is not None:
            exp["status"][i] = bad
            exp["max_count"][i], exp["best_bin"][i], exp["best_strand"][i], exp["hit_bins"][i] = 0, -1, 0, 0
    hits = expected_arrays([o], chunks, exp["status"] == capi.RB_OK, cap, min_count=1, r=R, conf=CONF, sentinel=GH.SENT)
    return exp, hits


def test_who_takes_which_item():
    """one batch interleaves N-free reads with reads that hold an N, a short and a too long one; as ASCII and as packed 2-bit + N mask,
    whole and chunked (a chunk that begins beyond a read; a window that cuts the N out, so that the item becomes the list kernel's),
    with read_ids (a permuted subset with a repeat), through the host and the device forms"""
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda:0")
    n_bins, lines = 2112, 1
    d, f = LS.resident(lambda words, info: SR.Planted(n_bins, lines, words), n_bins, SR.N_BLOCKS, lines)
    reads, kinds = PL.mixed_batch()
    reads = reads + [f.plants[0], LR.revcomp(f.plants[3])]
    n, cap = len(reads), 2 * n_bins
    eng = lists_engine([d])
    # host forms: every read whole (the long one is within the batch's own max_len there), and a selection
    run_both(eng, [f.o], reads, [lines], "mixed, host")
    run_both(eng, [f.o], reads, [lines], "mixed, host ids", ids=[7, 2, 2, n - 1, 0, 9, 5])
    # device forms
    buf, offs, lens = H.pack_reads(reads)
    packed, p_offs, nmask, n_offs = capi.pack_reads(buf, offs, lens)
    t = {k: torch.from_numpy(np.ascontiguousarray(a)).to(dev) for k, a in (("seq", buf), ("off", offs.view(np.int64)), ("len", lens.view(np.int32)),
         ("p", packed), ("po", p_offs.view(np.int64)), ("nm", nmask), ("no", n_offs.view(np.int64)))}
    ids = np.array([7, 2, 2, n - 1, 0, 9, 5], dtype=np.uint32)
    t["ids"] = torch.from_numpy(ids.view(np.int32)).to(dev)

    def run(setting, packed_form, start, length, with_ids):
        eng.set_pass_lists(setting)
        m = len(ids) if with_ids else n
        o = {"max_count": torch.full((m, 1), 77, dtype=torch.int16, device=dev), "best_bin": torch.full((m, 1), 77, dtype=torch.int32, device=dev),
             "best_strand": torch.full((m, 1), 77, dtype=torch.uint8, device=dev), "hit_bins": torch.full((m, 1), 77, dtype=torch.int32, device=dev),
             "status": torch.full((m,), 77, dtype=torch.uint8, device=dev), "hits": torch.full((m, 1, cap, 8), GH.SENT, dtype=torch.uint8, device=dev),
             "n_hits": torch.full((m, 1), 77, dtype=torch.int32, device=dev), "hstatus": torch.full((m,), 77, dtype=torch.uint8, device=dev),
             "prof": torch.zeros(n_bins, dtype=torch.int64, device=dev)}
        torch.cuda.synchronize()
        src = dict(d_nmask=t["nm"].data_ptr(), d_nmask_offsets=t["no"].data_ptr()) if packed_form else {}
        seq, off = (t["p"], t["po"]) if packed_form else (t["seq"], t["off"])
        kw = dict(chunk_start=start, chunk_length=length, d_read_ids=t["ids"].data_ptr() if with_ids else None, error_rate=R, significance=CONF, **src)
        eng.locate_device(seq.data_ptr(), off.data_ptr(), t["len"].data_ptr(), m, PL.MAX_LEN, d_max_count=o["max_count"].data_ptr(),
                          d_best_bin=o["best_bin"].data_ptr(), d_best_strand=o["best_strand"].data_ptr(), d_hit_bins=o["hit_bins"].data_ptr(),
                          d_status=o["status"].data_ptr(), **kw)
        eng.hits_device(seq.data_ptr(), off.data_ptr(), t["len"].data_ptr(), m, PL.MAX_LEN, min_count=1, max_hits=cap, d_hits=o["hits"].data_ptr(),
                        d_n_hits=o["n_hits"].data_ptr(), d_status=o["hstatus"].data_ptr(), d_bin_reads=o["prof"].data_ptr(), **kw)
        torch.cuda.synchronize()
        return {k: v.cpu().numpy() for k, v in o.items()}

    assert plan_lines(eng, PL.MAX_LEN) == [lines]
    for start, length in ((0, 0), (1, 148), (120, 0), (101, 100)):  # whole; the N at 0 and at 149 cut out; beyond the short reads; the N at 100 cut out
        exp, (exp_hits, exp_n, exp_prof, _) = chunk_expectation(f.o, reads, start, length, PL.MAX_LEN, cap)
        assert (exp["status"] == capi.RB_OK).sum() >= 5
        for packed_form in (False, True):
            for with_ids in (False, True):
                sel = ids.astype(np.int64) if with_ids else np.arange(n)
                got = {s: run(s, packed_form, start, length, with_ids) for s in (CURRENT, OFF)}
                what = ("device", start, length, packed_form, with_ids)
                for s in (CURRENT, OFF):
                    g = got[s]
                    loc = {"max_count": g["max_count"].view(np.uint16), "best_bin": g["best_bin"], "best_strand": g["best_strand"],
                           "hit_bins": g["hit_bins"].view(np.uint32), "status": g["status"]}
                    GL.assert_same(loc, {k: v[sel] for k, v in exp.items()}, what + (s,))
                    hit = {"hits": g["hits"].view(GH.HIT).reshape(len(sel), 1, cap), "n_hits": g["n_hits"].view(np.uint32), "status": g["hstatus"]}
                    GH.check(hit, exp_hits[sel], exp_n[sel], exp["status"][sel], what + (s,))
                assert all(got[CURRENT][k].tobytes() == got[OFF][k].tobytes() for k in got[OFF]), what
    eng.destroy()
    d.free()


# ------------------------------------------------------------------------------------------------ 8. engines of several filters
def test_engines_of_several_filters():
    """a list-served filter, a narrow one of a few words per block, and a second list-served one of another slot size: list_lines is per
    filter, the outputs are per filter, and the profile is the filters' bins one after the other"""
    d1, f1 = LS.resident(lambda words, info: SR.Planted(2112, 1, words), 2112, SR.N_BLOCKS, 1)
    d3, f3 = LS.resident(lambda words, info: SR.Planted(4090, 2, words), 4090, SR.N_BLOCKS, 2)
    narrow = po.OracleIBF(200, 3, K, 64 * 4 * 1021)
    rng = np.random.default_rng(3)
    planted = H.random_dna(rng, 300)
    narrow.insert(po.encode(planted), 77)
    d2 = GL.upload(narrow)
    eng = lists_engine([d1, d2, d3])
    reads = f1.reads()[:8] + f3.reads()[:8] + [planted[20:200], "ACGT", "ACGTNACGTACGTAACCGGTT" * 4]
    run_both(eng, [f1.o, narrow, f3.o], reads, [1, 0, 2], "three filters")
    eng.destroy()
    for d in (d1, d2, d3):
        d.free()


# ------------------------------------------------------------------------------------------------ 9. the setting
def test_the_setting():
    n_bins, lines = 2112, 1
    made = {}

    def edit(w, host):
        made["f"] = SR.Planted(n_bins, lines, host.words())

    d, owner = LS.LT.uploaded(n_bins, SR.N_BLOCKS, K, edit)
    f = made["f"]
    eng = capi.Engine(0, [d], [])
    reads = f.reads()[:10] + ["ACGTNACGTACGTAACCGGTT" * 4]
    buf, offs, lens = H.pack_reads(reads)
    max_len = int(lens.max())
    exp, _, _ = GL.oracle_rows([f.o], reads, R, CONF)

    def locate_is(want_lines, expectation, what):
        assert plan_lines(eng, max_len) == [want_lines], what
        GL.assert_same(eng.locate(buf, offs, lens, error_rate=R, significance=CONF), expectation, what)

    # CURRENT without a table: the plain form, and the call builds none
    eng.set_pass_lists(CURRENT)
    eng.set_row_table(capi.RB_ROW_TABLE_OFF)  # (the classify path builds no table either)
    locate_is(0, exp, "current, no table")
    assert d.list_table_info()["bytes"] == 0 and d.list_table_info()["builds"] == 0
    # BUILD builds one
    eng.set_pass_lists(BUILD)
    assert plan_lines(eng, max_len) == [0]
    GL.assert_same(eng.locate(buf, offs, lens, error_rate=R, significance=CONF), exp, "build")
    info = d.list_table_info()
    assert info["lines"] == lines and info["builds"] == 1 and plan_lines(eng, max_len) == [lines]
    # OFF: the plain form even with a current table
    eng.set_pass_lists(OFF)
    locate_is(0, exp, "off, table present")
    # the bits move on: CURRENT reports 0 and the results follow the new bits; BUILD rebuilds
    eng.set_pass_lists(CURRENT)
    locate_is(lines, exp, "current")
    moved = reads[0]
    d.insert(moved, [0], [len(moved)], [100])
    f.o.insert(po.encode(moved), 100)
    exp2, _, _ = GL.oracle_rows([f.o], reads, R, CONF)
    assert not np.array_equal(exp2["hit_bins"], exp["hit_bins"])  # (a second bin holds every k-mer of the read)
    locate_is(0, exp2, "current, stale table")
    eng.set_pass_lists(BUILD)
    GL.assert_same(eng.locate(buf, offs, lens, error_rate=R, significance=CONF), exp2, "rebuild")
    assert d.list_table_info()["builds"] == 2 and plan_lines(eng, max_len) == [lines]
    cap = 2 * n_bins
    st = exp2["status"]
    exp_hits, exp_n, _, _ = expected_arrays([f.o], reads, st == capi.RB_OK, cap, min_count=1, r=R, conf=CONF, sentinel=GH.SENT)
    GH.check(eng.hits(buf, offs, lens, error_rate=R, significance=CONF, min_count=1, max_hits=cap, hits=GH.sentinel_hits(len(reads), 1, cap)),
             exp_hits, exp_n, st, "hits after the rebuild")
    # a refused table: max_bytes too small -> the plain form, RB_OK
    d.list_table_drop()
    eng.set_row_table(capi.RB_ROW_TABLE_OFF, max_bytes=4096)
    GL.assert_same(eng.locate(buf, offs, lens, error_rate=R, significance=CONF), exp2, "refused")
    assert d.list_table_info()["bytes"] == 0 and d.list_table_info()["refused"] == capi.RB_LIST_REFUSED_MAX_BYTES and plan_lines(eng, max_len) == [0]
    eng.destroy()
    # classify before and after the passes: the same bytes
    eng = capi.Engine(0, [d], [])
    before = eng.classify(buf, offs, lens, error_rate=R, significance=CONF)
    eng.set_pass_lists(BUILD)
    eng.set_row_table(capi.RB_ROW_TABLE_OFF, max_bytes=96 << 30)
    eng.locate(buf, offs, lens, error_rate=R, significance=CONF)
    eng.hits(buf, offs, lens, error_rate=R, significance=CONF, min_count=1, max_hits=4)
    after = eng.classify(buf, offs, lens, error_rate=R, significance=CONF)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(before, after))
    eng.destroy()
    d.free()

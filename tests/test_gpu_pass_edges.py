"""The query passes (rb_locate_batch, rb_hits_batch, rb_spans_batch, rb_prefix_batch and their _device forms) against the oracle with
bin counts ON the edges of the bit-sliced counters, through the C ABI, bit for bit.

The cases are those of tests/pass_edges.py (asserted on the oracle alone in tests/test_pass_edges_cpu.py): a bin that counts every
k-mer of any read (1023: all ten planes set; 1024: the switch to sixteen; 65535, 65536 -> 0, 65537 -> 1 and 70000 -> 4464: the
uint16_t wrap the boundary header promises), a bin just below it that takes over the maximum when the first wraps and wraps itself
later, a bin on the reverse strand only, thresholds placed on those counts.  Every build of a pass -- lanes per block, words per lane,
counter planes, hash form, non-temporal twin -- has a filter here, every launch records what Engine.plan_pass reported for it, and a
closing test asserts that every build the launchers can select was reached by a launch that matched the oracle.  Expectations come
from locate_rules, hits_rules, prefix_rules and spans_rules.  No tolerance, no assertion on elapsed time."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from readbouncer_amd import capi
from tests import helpers as H
from tests import pass_edges as PE
from tests import prefix_rules as PR
from tests import spans_rules as SR
from tests.hits_rules import HIT, expected_arrays as hits_expected_arrays
from tests.test_gpu_hits import SENT, check as check_hits, sentinel_hits, upload
from tests.test_gpu_locate import assert_same as assert_same_locate, oracle_rows as locate_oracle_rows
from tests.test_gpu_prefix import device_buffers as prefix_device_buffers, to_host as prefix_to_host
from tests.test_gpu_spans import check as check_spans

R, CONF = PE.R, PE.CONF
MODES = (capi.RB_MODE_CHECK_UNBLOCK, capi.RB_MODE_CLASSIFY_CHUNK, capi.RB_MODE_CLASSIFY_ANY)
NT_DEFAULT = 512 << 20
# kernel geometries (log2 lanes per block, words per lane), as rb_kernels.hip dispatch_lg_wpl selects them
GEOMS = ((0, 1), (1, 1), (2, 1), (3, 1), (4, 1), (5, 1), (6, 1), (6, 2))
# what plain_geometry (rb_engine.hip) gives the filters of pass_edges.ALL: (lg, wpl, column slices)
SHAPE = {"lg0": (0, 1, 1), "lg1": (1, 1, 1), "lg2": (2, 1, 1), "lg3": (3, 1, 1), "lg4": (4, 1, 1), "lg5": (5, 1, 1), "lg6": (6, 1, 1),
         "w129": (6, 2, 2), "lg3_h2": (3, 1, 1), "w129_h4": (6, 2, 2), "lg0_k31": (0, 1, 1), "lg0_h2": (0, 1, 1), "lg1_h4": (1, 1, 1),
         "lg2_h2": (2, 1, 1), "lg4_h4": (4, 1, 1), "lg5_h2": (5, 1, 1), "lg6_h4": (6, 1, 1)}
NAMES = sorted(PE.ALL)
SPANS_NAMES = ("lg0", "w129", "lg3_h2", "w129_h4", "lg0_k31")  # one wave per query whatever the block shape: both hash forms, k = 31
# spans: the work items of the BIG batch a part queries (a position costs the oracle two count() calls, a second or two per read of
# 65 537 k-mers: the batch goes in two parts) -- up to the wrap and one past it; 70000 k-mers, 65 536 (+ L0) bases and the rest
SPANS_PARTS = {"TEN": None, "BIG_A": (0, 1, 2, 3, 4), "BIG_B": (5, 6, 7, 8, 9, 10, 11, 12, 13)}
DEVICE_NAMES = ("lg2", "w129")


def build_label(pass_name, p):
    return "%s<LG=%d,WPL=%d,NP=%d,%s,NT=%d>" % (pass_name, p["lanes_per_block_log2"], p["words_per_lane"], p["counter_planes"],
                                                  "h=3" if p["hash_functions"] == 3 else "generic", p["nontemporal"])


def spans_label(p):
    return "spans<%s,NT=%d>" % ("h=3" if p["hash_functions"] == 3 else "generic", p["spans_nontemporal"])


def expected_builds():
    out = set()
    for pass_name in ("locate", "hits", "prefix"):
        for lg, wpl in GEOMS:
            for planes, hashes in ((10, 3), (16, 3), (16, 0)):
                for nt in ((0, 1) if lg == 6 else (0,)):
                    out.add(build_label(pass_name, {"lanes_per_block_log2": lg, "words_per_lane": wpl, "counter_planes": planes,
                                                    "hash_functions": hashes, "nontemporal": nt}))
    for hashes in (3, 0):
        for nt in (0, 1):
            out.add(spans_label({"hash_functions": hashes, "spans_nontemporal": nt}))
    return out


EXPECTED_BUILDS = expected_builds()
_reached = {}   # build -> cases it ran and matched the oracle on
_tests_run = set()


class Rig:
    """one filter of pass_edges on the device behind an engine of its own; classify before and after the passes must be the same bytes"""

    def __init__(self, name):
        self.name = name
        self.f = PE.make_filter(name)
        self.k = self.f.kmer_size
        self.bins = PE.bins_of(name)
        self.dev = upload(self.f)
        self.eng = capi.Engine(0, [self.dev], [])
        self.probe = H.pack_reads(list(PE.batch("SWITCH", self.k)[0]))
        self.before = self.eng.classify(*self.probe, error_rate=R, significance=CONF)

    def plan(self, max_len, nt=False):
        p = self.eng.plan_pass(0, max_len)
        lg, wpl, slices = SHAPE[self.name]
        assert (p["lanes_per_block_log2"], p["words_per_lane"], p["column_slices"]) == (lg, wpl, slices), (self.name, p)
        assert p["hash_functions"] == (3 if self.f.n_hash == 3 else 0) and p["spans_nontemporal"] == int(nt), (self.name, p)
        assert p["nontemporal"] == int(nt and lg == 6), (self.name, p)
        kmers = max(max_len - self.k + 1, 0)
        assert p["counter_planes"] == (10 if kmers <= 1023 and self.f.n_hash == 3 else 16), (self.name, max_len, p)
        return p

    def nontemporal(self, on):
        self.eng.set_nt_threshold(0 if on else NT_DEFAULT)

    def close(self):
        after = self.eng.classify(*self.probe, error_rate=R, significance=CONF)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(self.before, after)), self.name
        self.eng.destroy()
        self.dev.free()


def reached(label, case):
    assert label in EXPECTED_BUILDS, label
    _reached.setdefault(label, set()).add(case)


def max_len_of(reads):
    return max(len(r) for r in reads)


# ---------------------------------------------------------------------------------------------------------------- locate
@pytest.mark.parametrize("name", NAMES)
def test_locate_at_the_counter_edges(name):
    rig = Rig(name)
    try:
        for which in PE.BATCHES:
            reads = PE.batch(which, rig.k)[0]
            buf, offs, lens = H.pack_reads(list(reads))
            for rule in (3, 4):
                exp = PE.locate_expectation(name, which, rule)
                rig.eng.set_revcomp_of_n(rule)
                for nt in (False, True):
                    rig.nontemporal(nt)
                    p = rig.plan(max_len_of(reads), nt)
                    got = rig.eng.locate(buf, offs, lens, error_rate=R, significance=CONF)
                    assert_same_locate(got, exp, "%s %s rule %d nt %d" % (name, which, rule, nt))
                    reached(build_label("locate", p), which)
            rig.eng.set_revcomp_of_n(3)
            rig.nontemporal(False)
        # what the batches are for, on the product's own numbers: the maximum moved off the bin that matched everything
        big = PE.batch("BIG", rig.k)[1]
        got = rig.eng.locate(*H.pack_reads(list(PE.batch("BIG", rig.k)[0])), error_rate=R, significance=CONF)
        assert int(got["best_bin"][big.index(65535), 0]) == rig.bins["SAT"] and int(got["max_count"][big.index(65535), 0]) == 65535
        assert int(got["best_bin"][big.index(65536), 0]) == rig.bins["NEAR"] and int(got["best_bin"][big.index(70000), 0]) == rig.bins["REV"]
        assert int(got["best_strand"][big.index(70000), 0]) == 1
    finally:
        rig.close()
    _tests_run.add(("locate", name))


# ------------------------------------------------------------------------------------------------------------------ hits
def edge_read(which):
    return {"TEN": 1023, "SWITCH": 1024, "BIG": 65536}[which]


def hits_min_counts(name, which):
    """0: the decision's t (t == 0 and, for k = 31, the wrapped t among them); 1: every nonzero entry; then the threshold ON a count:
    c and c + 1 with c the oracle's count of NEAR on the batch's edge read, SAT's own count and one more, 65535 in the BIG batch"""
    k = PE.ALL[name][3]
    i = PE.batch(which, k)[1].index(edge_read(which))
    c = int(PE.counts(name, which)[i][0][PE.bins_of(name)["NEAR"]])
    assert 0 < c < 65535
    return [0, 1, c, c + 1] + {"TEN": [1023, 1024], "SWITCH": [1024, 1025], "BIG": [65535]}[which]


@pytest.mark.parametrize("name", NAMES)
def test_hits_at_the_counter_edges(name):
    rig = Rig(name)
    cap = 2 * rig.f.n_bins
    try:
        for which in PE.BATCHES:
            reads = PE.batch(which, rig.k)[0]
            buf, offs, lens = H.pack_reads(list(reads))
            n = len(reads)
            for nt in (False, True):
                rig.nontemporal(nt)
                p = rig.plan(max_len_of(reads), nt)
                mcs = hits_min_counts(name, which)
                for mc in (mcs if not nt else mcs[:3]):
                    exp_hits, exp_n, exp_prof, st = PE.hits_expectation(name, which, 3, mc, cap, SENT)
                    assert int(exp_n.max()) <= cap
                    prof = np.zeros(rig.f.n_bins, np.uint64)
                    got = rig.eng.hits(buf, offs, lens, error_rate=R, significance=CONF, min_count=mc, max_hits=cap, bin_reads=prof,
                                       hits=sentinel_hits(n, 1, cap))
                    check_hits(got, exp_hits, exp_n, st, "%s %s min_count %d nt %d" % (name, which, mc, nt))
                    assert np.array_equal(prof, exp_prof), (name, which, mc)
                reached(build_label("hits", p), which)
            rig.nontemporal(False)
        # the other N rule, in full
        rig.eng.set_revcomp_of_n(4)
        reads = PE.batch("BIG", rig.k)[0]
        exp_hits, exp_n, _, st = PE.hits_expectation(name, "BIG", 4, 1, cap, SENT)
        got = rig.eng.hits(*H.pack_reads(list(reads)), error_rate=R, significance=CONF, min_count=1, max_hits=cap, hits=sentinel_hits(len(reads), 1, cap))
        check_hits(got, exp_hits, exp_n, st, name + " BIG, N stays N")
        rig.eng.set_revcomp_of_n(3)
    finally:
        rig.close()
    _tests_run.add(("hits", name))


# -------------------------------------------------------------------------------------------------------------- prefixes
def run_prefixes(rig, reads, cps, mode=capi.RB_MODE_CHECK_UNBLOCK):
    buf, offs, lens = H.pack_reads(list(reads))
    return rig.eng.prefixes(buf, offs, lens, cps, error_rate=R, significance=CONF, mode=mode)


@pytest.mark.parametrize("name", NAMES)
def test_prefixes_at_the_counter_edges(name):
    rig = Rig(name)
    try:
        cases = [("TEN", (capi.RB_MODE_CHECK_UNBLOCK,)), ("SWITCH", (capi.RB_MODE_CHECK_UNBLOCK,)), ("WRAP", MODES)]
        if name in ("lg3", "w129"):
            cases.append(("DENSE", (capi.RB_MODE_CHECK_UNBLOCK,)))
        for case, modes in cases:
            for mode in modes:
                reads, cps, exp = PE.prefix_expectation(name, case, mode)
                for nt in (False, True):
                    rig.nontemporal(nt)
                    p = rig.plan(min(max_len_of(reads), cps[-1]), nt)  # (no row is longer than the last checkpoint: rb_engine.hip, rb_prefix_batch_device)
                    PR.assert_same(run_prefixes(rig, reads, cps, mode), exp, "%s %s mode %d nt %d" % (name, case, mode, nt))
                    reached(build_label("prefix", p), case)
                rig.nontemporal(False)
                assert exp["first_decided"].shape == (len(reads),)
    finally:
        rig.close()
    _tests_run.add(("prefix", name))


# ----------------------------------------------------------------------------------------------------------------- spans
def spans_items(name, part):
    k = PE.ALL[name][3]
    if part == "TEN":
        reads = PE.batch("TEN", k)[0]
        return "TEN", reads, list(range(len(reads)))
    reads = PE.batch("BIG", k)[0]
    return "BIG", reads, [i for i in SPANS_PARTS[part] if i < len(reads)]


_spans_cache = {}


def spans_expectation(name, part, mw):
    key = (name, part, mw)
    if key not in _spans_cache:
        f = PE.make_filter(name)
        b = PE.bins_of(name)
        _, reads, items = spans_items(name, part)
        q = SR.as_queries([(i, b[x]) for i in items for x in ("SAT", "NEAR", "REV")])
        _spans_cache[key] = (q, SR.expected_arrays(f, list(reads), PE.status_of(reads, f.kmer_size), q, mw))
    return _spans_cache[key]


@pytest.mark.parametrize("part", sorted(SPANS_PARTS))
@pytest.mark.parametrize("name", SPANS_NAMES)
def test_spans_at_the_counter_edges(name, part):
    rig = Rig(name)
    mw = 3  # far fewer words than the reads have positions: what lies beyond is left out of the mask ONLY
    try:
        which, reads, items = spans_items(name, part)
        q, exp = spans_expectation(name, part, mw)
        spans, mask, n_kmers, status = exp
        buf, offs, lens = H.pack_reads(list(reads))
        cv = PE.counts(name, which)
        for nt in (False, True):
            rig.nontemporal(nt)
            p = rig.plan(max_len_of(reads), nt)
            got = rig.eng.spans(buf, offs, lens, 0, q, mask_words=mw, mask=np.full((len(q), 2, mw), 0xABABABABABABABAB, dtype=np.uint64))
            check_spans(got, exp, "%s %s nt %d" % (name, part, nt))
            reached(spans_label(p), part)
        rig.nontemporal(False)
        # count is exact; its low 16 bits are the oracle's uint16_t entry -- and the hits record's count of the same (bin, strand)
        cap = 2 * rig.f.n_bins
        hit = rig.eng.hits(buf, offs, lens, error_rate=R, significance=CONF, min_count=1, max_hits=cap, hits=sentinel_hits(len(reads), 1, cap))
        for qi, (item, b) in enumerate(zip(q["item"].tolist(), q["bin"].tolist())):
            if status[qi] != capi.RB_OK:
                continue
            rec = hit["hits"][item, 0, :int(hit["n_hits"][item, 0])]
            for s in range(2):
                c = int(got["spans"][qi, s]["count"])
                assert c & 0xFFFF == int(cv[item][s][b]), (name, part, item, b, s)
                mine = rec[(rec["bin"] == b) & (rec["strand"] == s)]
                assert (int(mine["count"][0]) if len(mine) else 0) == c & 0xFFFF, (name, part, item, b, s)
        if part == "BIG_A":  # SAT on the read of 65 537 k-mers: every position, one run, every base
            n = 65537
            qi = [i for i, (item, b) in enumerate(zip(q["item"].tolist(), q["bin"].tolist())) if item == 4 and b == rig.bins["SAT"]][0]
            assert int(n_kmers[qi]) == n
            for s in range(2):
                r = got["spans"][qi, s]
                assert (int(r["count"]), int(r["first"]), int(r["last"]), int(r["run_start"]), int(r["run_len"]), int(r["covered"])) == \
                    (n, 0, n - 1, 0, n, len(reads[4])), (name, s, r)
    finally:
        rig.close()
    _tests_run.add(("spans", name, part))


# ---------------------------------------------------------------------------------------------------------- device forms
DEVICE_IDS = (4, 5, 4, 8, 9, 10, 11)  # of BIG: 65537 and 70000 k-mers, the first again, the reverse complement, the one with N, t == 0, "ACGT"
CHUNK_START = 3                       # not a multiple of 4: a chunk starts inside a byte of the 2-bit source


class DeviceBatch:
    def __init__(self, torch, rig):
        self.torch, self.dev = torch, torch.device("cuda:0")
        reads = PE.batch("BIG", rig.k)[0]
        self.buf, self.offs, self.lens = H.pack_reads(list(reads))
        packed, p_offs, nmask, n_offs = capi.pack_reads(self.buf, self.offs, self.lens)
        self.keep = [torch.from_numpy(np.ascontiguousarray(a)).to(self.dev) for a in (packed, p_offs.view(np.int64), nmask, n_offs.view(np.int64),
                                                                                      self.lens.view(np.int32), np.array(DEVICE_IDS, np.int32))]
        t_p, t_po, t_nm, t_no, t_len, t_ids = self.keep
        self.max_len = int(self.lens.max())
        self.args = (t_p.data_ptr(), t_po.data_ptr(), t_len.data_ptr(), len(DEVICE_IDS), self.max_len)
        self.kw = dict(d_nmask=t_nm.data_ptr(), d_nmask_offsets=t_no.data_ptr(), chunk_start=CHUNK_START, d_read_ids=t_ids.data_ptr())
        self.chunks = [reads[i][CHUNK_START:] for i in DEVICE_IDS]
        self.status = PE.status_of(self.chunks, rig.k)
        assert (self.status != capi.RB_OK).any() and any("N" in c for c in self.chunks)


@pytest.mark.parametrize("pass_name", ["locate", "hits", "prefix", "spans"])
@pytest.mark.parametrize("name", DEVICE_NAMES)
def test_device_forms_packed_chunked_with_read_ids(name, pass_name):
    torch = pytest.importorskip("torch")
    rig = Rig(name)
    try:
        d = DeviceBatch(torch, rig)
        dev, n = d.dev, len(DEVICE_IDS)
        p = rig.plan(d.max_len)
        full = lambda shape, dtype: torch.full(shape, 77, dtype=dtype, device=dev)
        if pass_name == "locate":
            exp, _, _ = locate_oracle_rows([rig.f], d.chunks)
            o = {"max_count": full((n, 1), torch.int16), "best_bin": full((n, 1), torch.int32), "best_strand": full((n, 1), torch.uint8),
                 "hit_bins": full((n, 1), torch.int32), "status": full((n,), torch.uint8)}
            torch.cuda.synchronize()
            rig.eng.locate_device(*d.args, error_rate=R, significance=CONF, d_max_count=o["max_count"].data_ptr(), d_best_bin=o["best_bin"].data_ptr(),
                                  d_best_strand=o["best_strand"].data_ptr(), d_hit_bins=o["hit_bins"].data_ptr(), d_status=o["status"].data_ptr(), **d.kw)
            torch.cuda.synchronize()
            got = {"max_count": o["max_count"].cpu().numpy().view(np.uint16), "best_bin": o["best_bin"].cpu().numpy(), "best_strand": o["best_strand"].cpu().numpy(),
                   "hit_bins": o["hit_bins"].cpu().numpy().view(np.uint32), "status": o["status"].cpu().numpy()}
            assert_same_locate(got, exp, name + " device form")
            assert int(exp["max_count"][0, 0]) == 65537 - CHUNK_START and int(exp["best_bin"][1, 0]) == rig.bins["REV"]
            reached(build_label("locate", p), "device")
        elif pass_name == "hits":
            cap = 2 * rig.f.n_bins
            for mc in (0, 65537 - CHUNK_START):
                exp_hits, exp_n, exp_prof, _ = hits_expected_arrays([rig.f], d.chunks, d.status == capi.RB_OK, cap, min_count=mc, r=R, conf=CONF, sentinel=SENT)
                assert int(exp_n.max()) <= cap and exp_n.any()
                o = {"hits": torch.full((n * cap * 8,), SENT, dtype=torch.uint8, device=dev), "n_hits": full((n, 1), torch.int32),
                     "status": full((n,), torch.uint8), "bin_reads": torch.zeros(rig.f.n_bins, dtype=torch.int64, device=dev)}
                torch.cuda.synchronize()
                rig.eng.hits_device(*d.args, error_rate=R, significance=CONF, min_count=mc, max_hits=cap, d_hits=o["hits"].data_ptr(),
                                    d_n_hits=o["n_hits"].data_ptr(), d_status=o["status"].data_ptr(), d_bin_reads=o["bin_reads"].data_ptr(), **d.kw)
                torch.cuda.synchronize()
                got = {"hits": o["hits"].cpu().numpy().view(HIT).reshape(n, 1, cap), "n_hits": o["n_hits"].cpu().numpy().view(np.uint32),
                       "status": o["status"].cpu().numpy()}
                check_hits(got, exp_hits, exp_n, d.status, "%s device form, min_count %d" % (name, mc))
                assert np.array_equal(o["bin_reads"].cpu().numpy().view(np.uint64), exp_prof), (name, mc)
            reached(build_label("hits", p), "device")
        elif pass_name == "prefix":
            cps = PE.wrap_checkpoints(rig.k)
            exp = PE.prefix_rows(rig.f, d.chunks, cps, capi.RB_MODE_CHECK_UNBLOCK, chunk_start=0)
            o = prefix_device_buffers(torch, dev, n, len(cps), 1)
            torch.cuda.synchronize()
            rig.eng.prefixes_device(*d.args, cps, error_rate=R, significance=CONF, d_max_count=o["max_count"].data_ptr(), d_decision=o["decision"].data_ptr(),
                                    d_best_target=o["best_target"].data_ptr(), d_status=o["status"].data_ptr(), d_prefix_len=o["prefix_len"].data_ptr(),
                                    d_first_decided=o["first_decided"].data_ptr(), **d.kw)
            torch.cuda.synchronize()
            PR.assert_same(prefix_to_host(o), exp, name + " device form")
            assert int(exp["max_count"][0, -1, 0]) == 65537 - CHUNK_START and exp["max_count"][1, -1, 0] < exp["max_count"][1, 3, 0]  # the chunk's own counts
            reached(build_label("prefix", rig.plan(min(d.max_len, cps[-1]))), "device")
        else:
            mw = 2
            q = SR.as_queries([(0, rig.bins["SAT"]), (0, rig.bins["NEAR"]), (3, rig.bins["REV"]), (5, rig.bins["SAT"]), (6, rig.bins["SAT"])])
            nq = len(q)
            exp = SR.expected_arrays(rig.f, d.chunks, d.status, q, mw)
            t_q = torch.from_numpy(q.view(np.int32).reshape(-1, 2).copy()).to(dev)
            o = {"spans": torch.full((nq * 2 * 6,), 0x5A5A5A5A, dtype=torch.int32, device=dev),
                 "mask": torch.full((nq * 2 * mw,), -0x5454545454545455, dtype=torch.int64, device=dev),
                 "n_kmers": full((nq,), torch.int32), "status": full((nq,), torch.uint8)}
            torch.cuda.synchronize()
            rig.eng.spans_device(*d.args, 0, t_q.data_ptr(), nq, mask_words=mw, d_spans=o["spans"].data_ptr(), d_mask=o["mask"].data_ptr(),
                                 d_n_kmers=o["n_kmers"].data_ptr(), d_status=o["status"].data_ptr(), **d.kw)
            torch.cuda.synchronize()
            got = {"spans": o["spans"].cpu().numpy().view(SR.SPAN).reshape(nq, 2), "mask": o["mask"].cpu().numpy().view(np.uint64).reshape(nq, 2, mw),
                   "n_kmers": o["n_kmers"].cpu().numpy().view(np.uint32), "status": o["status"].cpu().numpy()}
            check_spans(got, exp, name + " device form")
            assert int(exp[0][0, 0]["count"]) == 65537 - CHUNK_START and exp[3][4] == capi.RB_ERR_SHORT_READ
            reached(spans_label(p), "device")
    finally:
        rig.close()
    _tests_run.add(("device", name, pass_name))


ALL_TESTS = ({(p, n) for p in ("locate", "hits", "prefix") for n in NAMES} | {("spans", n, part) for n in SPANS_NAMES for part in SPANS_PARTS} |
             {("device", n, p) for n in DEVICE_NAMES for p in ("locate", "hits", "prefix", "spans")})


def test_every_pass_build_was_reached():
    """Coverage of the matrix above.  EXPECTED_BUILDS is every instantiation the launchers of rb_kernels.hip can select: launch_plain_pass
    (locate, hits and prefixes alike) goes through dispatch_planes_hash -- ten planes only with the three compile-time hash functions,
    sixteen with them or with the run-time hash count -- and dispatch_lg_wpl -- the eight geometries --, and takes the non-temporal twin
    `if constexpr (L == 6)` only: 8 x 3 + 2 x 3 builds per pass, the count commit 7af8428 gives; launch_ibf_spans picks h = 3 or the
    run-time h and launch_spans_nt the twin: 4 builds.  Every one of them matched the oracle at least once, the ten-plane builds on the
    batch whose maximum is 1023, the sixteen-plane builds on the batch of 1024 and on the one across the uint16_t wrap.  A change of
    plain_geometry that stops routing a case to a build makes this fail instead of silently testing less."""
    if _tests_run != ALL_TESTS:
        pytest.skip("runs after the whole matrix of this file")
    missing = EXPECTED_BUILDS - set(_reached)
    assert not missing, ("builds never reached", sorted(missing), "reached", sorted(_reached))
    assert len(EXPECTED_BUILDS) == 3 * 30 + 4
    for b in sorted(EXPECTED_BUILDS):
        if b.startswith("spans"):
            want = {"TEN", "BIG_A", "BIG_B"}
        elif b.startswith("prefix"):
            want = {"TEN"} if "NP=10" in b else {"SWITCH", "WRAP"}
        else:
            want = {"TEN"} if "NP=10" in b else {"SWITCH", "BIG"}
        assert want <= _reached[b], (b, "cases never counted", sorted(want - _reached[b]))
    print("reached builds:\n  " + "\n  ".join("%s: %s" % (b, sorted(v)) for b, v in sorted(_reached.items())))

"""The hits pass (rb_hits_batch / rb_hits_batch_device) against the oracle, bit for bit, through the C ABI.

The oracle side of every case is `OracleIBF.count()` on the read and on `revcomp()` of it, reduced by tests/hits_rules.py (checked on
hand-written vectors in test_hits_cpu.py).  Record buffers go in filled with a sentinel and are compared WHOLE against the expected
buffer over the same sentinel, so order, truncation and "slots beyond the list are not written" are one comparison.  A test that
compares whole lists first asserts, from the oracle, that no list exceeds its cap.  No assertion on elapsed time."""
import functools

import numpy as np
import pytest

from oracle import pyoracle as po
from readbouncer_amd import capi, synth
from tests import helpers as H
from tests.hits_rules import HIT, distinct_bins, expected_arrays

# name -> (n_bins, n_blocks, n_hash, k): W = ceil(n_bins / 64) word columns -- every (lanes per block, words per lane) build
GEOMETRIES = {
    "w1": (64, 4096, 3, 13), "w2": (100, 4099, 3, 13), "w4": (243, 4096, 3, 13), "w8": (500, 4099, 3, 13), "w16": (1000, 4096, 3, 13),
    "w32": (2040, 4099, 3, 13), "w64": (4090, 4096, 3, 13), "w128": (8190, 4099, 3, 13), "w144": (9200, 4096, 3, 13),
    "w485": (31000, 4099, 3, 13), "w5_h2": (300, 4096, 2, 13),
}
R, CONF, SENT = 0.1, 0.95, 0xAB
FRAG = 700


def revcomp_str(s):
    return s[::-1].translate(str.maketrans("ACGT", "TGCA"))


@functools.lru_cache(maxsize=None)
def make_case(name, n_reads=36, frag=FRAG, lo=60, hi=500):
    """filter (oracle) + reads: fragments planted in several bins, one fragment in three bins, one with its reverse complement in the
    same bin (a read of it hits that bin on both strands), reads with runs of N, random reads, reads shorter than k"""
    n_bins, n_blocks, h, k = GEOMETRIES[name]
    W = (n_bins + 63) // 64
    rng = np.random.default_rng(sum(name.encode()) + frag)
    f = po.OracleIBF(n_bins, h, k, 64 * W * n_blocks)
    three, same = (0, n_bins // 2, n_bins - 1), min(20, n_bins - 2)
    free = [b for b in range(n_bins) if b not in three and b != same]
    bins = sorted(rng.choice(free, size=min(12, len(free)), replace=False).tolist())
    frags = [H.random_dna(rng, frag) for _ in bins]
    for b, s in zip(bins, frags):
        f.insert(po.encode(s), b)
    t1, t2 = H.random_dna(rng, frag), H.random_dna(rng, frag)
    for b in three:
        f.insert(po.encode(t1), b)
    f.insert(po.encode(t2), same)
    f.insert(po.encode(revcomp_str(t2)), same)
    reads = []
    for i in range(n_reads):
        L = int(rng.integers(lo, hi + 1))
        src = (frags + [t1, t2])[i % (len(frags) + 2)] if i % 4 else None
        if src is None:
            r = H.random_dna(rng, L)
        else:
            s = int(rng.integers(0, len(src) - L + 1))
            r = H.mutate(rng, src[s:s + L], float(rng.uniform(0.0, 0.12)))
        if i % 5 == 0:  # a run of N and single Ns
            a = np.frombuffer(r.encode(), dtype=np.uint8).copy()
            p = int(rng.integers(0, L - 8))
            a[p:p + 8] = ord("N")
            a[rng.random(L) < 0.01] = ord("N")
            r = a.tobytes().decode()
        reads.append(r)
    reads += [t2[100:100 + hi // 2], t1[50:50 + hi // 2], "ACGT", "A" * (k - 1), ""]
    return f, tuple(reads)


def upload(f):
    host = capi.HostIBF.create(f.n_bins, f.n_hash, f.kmer_size, f.n_bits)
    w = f.words()
    host.words()[:len(w)] = w
    return capi.DeviceIBF.upload(0, host)


def sentinel_hits(n, nf, cap):
    return np.frombuffer(bytes([SENT]) * (n * nf * cap * 8), dtype=HIT).reshape(n, nf, cap).copy()


def run_hits(eng, reads, cap, min_count=0, ids=None, profile=None):
    buf, offs, lens = H.pack_reads(list(reads))
    n = len(reads) if ids is None else len(ids)
    nf = eng.nd + eng.nt
    return eng.hits(buf, offs, lens, read_ids=ids, error_rate=R, significance=CONF, min_count=min_count, max_hits=cap, bin_reads=profile,
                    hits=sentinel_hits(n, nf, cap) if cap else None)


def check(got, exp_hits, exp_n, exp_status, what):
    assert np.array_equal(got["status"], exp_status), (what, got["status"].tolist(), exp_status.tolist())
    if not np.array_equal(got["n_hits"], exp_n):
        bad = np.argwhere(got["n_hits"] != exp_n)[:5]
        raise AssertionError("%s: n_hits differs at %s: got %s, expected %s" % (what, bad.tolist(), got["n_hits"][tuple(bad.T)].tolist(), exp_n[tuple(bad.T)].tolist()))
    if exp_hits is not None and got["hits"].tobytes() != exp_hits.tobytes():
        bad = np.argwhere(got["hits"] != exp_hits)[:5]
        raise AssertionError("%s: records differ at %s: got %s, expected %s" % (what, bad.tolist(), got["hits"][tuple(bad.T)].tolist(), exp_hits[tuple(bad.T)].tolist()))


def status_of(reads, kmax):
    return np.array([capi.RB_OK if len(r) >= kmax else capi.RB_ERR_SHORT_READ for r in reads], np.uint8)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(GEOMETRIES))
def test_full_count_vectors(name):
    """min_count = 1 with a cap of 2 x n_bins: the list is every nonzero entry of the oracle's two vectors, under both N rules"""
    f, reads = make_case(name)
    cap = 2 * f.n_bins
    eng = capi.Engine(0, [upload(f)], [])
    for rule in (3, 4):
        prev = po.set_revcomp_of_n(rule)
        try:
            st = status_of(reads, f.kmer_size)
            exp_hits, exp_n, exp_prof, lists = expected_arrays([f], reads, st == capi.RB_OK, cap, min_count=1, sentinel=SENT)
        finally:
            po.set_revcomp_of_n(prev)
        assert int(exp_n.max()) <= cap  # no truncation can hide a mismatch
        both = [i for i, l in enumerate(lists) if {(b, s) for b, s, _ in l[0]} >= {(min(20, f.n_bins - 2), 0), (min(20, f.n_bins - 2), 1)}]
        assert both and int(exp_n.max()) >= 6, (name, exp_n.max())  # a bin on both strands; several bins in one list
        eng.set_revcomp_of_n(rule)
        prof = np.zeros(f.n_bins, np.uint64)
        got = run_hits(eng, reads, cap, min_count=1, profile=prof)
        check(got, exp_hits, exp_n, st, "%s rule %d" % (name, rule))
        assert np.array_equal(prof, exp_prof), name
        # the non-temporal twins of the whole-wave builds (the engine picks them by table size: here by a threshold of 0)
        eng.set_nt_threshold(0)
        check(run_hits(eng, reads, cap, min_count=1), exp_hits, exp_n, st, "%s rule %d, non-temporal" % (name, rule))
        eng.set_nt_threshold(512 << 20)
    eng.destroy()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["w1", "w4", "w16", "w144", "w485", "w5_h2"])
def test_decision_threshold_and_consistency_with_locate(name):
    """min_count = 0: t is the decision stage's; lengths with t == 0 (every bin on both strands) and with a wrapped t are among the reads"""
    f, reads = make_case(name)
    k = f.kmer_size
    zero = [L for L in range(k, 400) if po.threshold(L, k, R, CONF) == 0]
    wrapped = [L for L in range(k, 400) if po.threshold(L, k, R, CONF) > 60000]
    rng = np.random.default_rng(4)
    assert zero and wrapped
    reads = list(reads) + [H.random_dna(rng, zero[-1]), H.random_dna(rng, wrapped[0])]
    cap = 2 * f.n_bins
    st = status_of(reads, k)
    exp_hits, exp_n, exp_prof, lists = expected_arrays([f], reads, st == capi.RB_OK, cap, sentinel=SENT)
    assert int(exp_n.max()) == cap and (exp_n[st == capi.RB_OK] == 0).any() and ((exp_n > 0) & (exp_n < 8)).any()
    eng = capi.Engine(0, [upload(f)], [])
    got = run_hits(eng, reads, cap)
    check(got, exp_hits, exp_n, st, name)
    buf, offs, lens = H.pack_reads(reads)
    loc = eng.locate(buf, offs, lens, error_rate=R, significance=CONF)
    for i in range(len(reads)):
        n = int(got["n_hits"][i, 0])
        rec = got["hits"][i, 0, :n]
        assert len(np.unique(rec["bin"])) == int(loc["hit_bins"][i, 0]), (name, i)
        t = po.threshold(len(reads[i]), k, R, CONF) if st[i] == capi.RB_OK else 0
        if st[i] == capi.RB_OK and int(loc["max_count"][i, 0]) >= t:
            assert n > 0 and int(rec["count"].max()) == int(loc["max_count"][i, 0]), (name, i)
    eng.destroy()


@pytest.mark.gpu
def test_reads_of_more_than_1023_kmers():
    """the 16-plane builds, at the decision threshold and in full"""
    f, reads = make_case("w4", n_reads=16, frag=2400, lo=1100, hi=1500)
    assert max(len(r) for r in reads) - 13 + 1 > 1023
    cap = 2 * f.n_bins
    st = status_of(reads, f.kmer_size)
    eng = capi.Engine(0, [upload(f)], [])
    for mc in (0, 1):
        exp_hits, exp_n, _, _ = expected_arrays([f], reads, st == capi.RB_OK, cap, min_count=mc, sentinel=SENT)
        assert int(exp_n.max()) <= cap and int(exp_hits["count"][exp_hits["reserved"] == 0].max()) > 1023
        check(run_hits(eng, reads, cap, min_count=mc), exp_hits, exp_n, st, "long reads, min_count %d" % mc)
    eng.destroy()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["w2", "w144"])
def test_truncation_keeps_the_first_records_and_leaves_the_rest_alone(name):
    f, reads = make_case(name)
    st = status_of(reads, f.kmer_size)
    eng = capi.Engine(0, [upload(f)], [])
    profiles = []
    for cap in (0, 1, 2, 3):
        exp_hits, exp_n, exp_prof, _ = expected_arrays([f], reads, st == capi.RB_OK, cap, min_count=1, sentinel=SENT)
        assert int(np.count_nonzero(exp_n > 3)) >= 10  # more hits than any of the caps
        prof = np.zeros(f.n_bins, np.uint64)
        got = run_hits(eng, reads, cap, min_count=1, profile=prof)
        check(got, exp_hits if cap else None, exp_n, st, "%s cap %d" % (name, cap))
        assert np.array_equal(prof, exp_prof)
        profiles.append(prof)
    assert all(np.array_equal(p, profiles[0]) for p in profiles)
    eng.destroy()


def four_filter_engine():
    names = ["w2", "w144", "w1", "w5_h2"]  # two deplete + two target filters of different geometry
    cases = [make_case(n) for n in names]
    filters = [c[0] for c in cases]
    reads = []
    for c in cases:
        reads += list(c[1][:14]) + list(c[1][-5:])
    return filters, reads, [upload(f) for f in filters]


@pytest.mark.gpu
def test_several_filters_engine_settings_ids_profile_and_determinism():
    filters, reads, devs = four_filter_engine()
    kmax = max(f.kmer_size for f in filters)
    st = status_of(reads, kmax)
    cap = 40
    exp_hits, exp_n, exp_prof, _ = expected_arrays(filters, reads, st == capi.RB_OK, cap, sentinel=SENT)
    assert (st != capi.RB_OK).any() and exp_n.any(axis=0).all()
    buf, offs, lens = H.pack_reads(reads)
    eng = capi.Engine(0, devs[:2], devs[2:])
    before = eng.classify(buf, offs, lens, error_rate=R, significance=CONF)
    prof = np.zeros(sum(f.n_bins for f in filters), np.uint64)
    first = run_hits(eng, reads, cap, profile=prof)
    check(first, exp_hits, exp_n, st, "four filters")
    assert np.array_equal(prof, exp_prof)
    # the profile accumulates over calls; two calls return byte-identical buffers
    second = run_hits(eng, reads, cap, profile=prof)
    assert np.array_equal(prof, 2 * exp_prof)
    for key in ("hits", "n_hits", "status"):
        assert first[key].tobytes() == second[key].tobytes(), key
    # the classify path is what it was
    after = eng.classify(buf, offs, lens, error_rate=R, significance=CONF)
    assert all(np.array_equal(a, b) for a, b in zip(before, after))
    # the engine's settings do not reach the pass
    for what, change in (("early decision", lambda e: e.set_early_decision(1)), ("no pruning", lambda e: e.set_bound_pruning(0)),
                         ("merge always", lambda e: e.set_merge(2)), ("merge never", lambda e: e.set_merge(0)),
                         ("phased", lambda e: e.set_phased(0, 1 << 40, 300, 0, 1)), ("not phased", lambda e: e.set_phased(0, 0, 0, 0, 0))):
        change(eng)
        eng.classify(buf, offs, lens, error_rate=R, significance=CONF)  # (lets the setting take effect on the classify path)
        check(run_hits(eng, reads, cap), exp_hits, exp_n, st, what)
    # host read ids: one, repeated, all, none
    n = len(reads)
    for ids in ([5], [3, 3, 7, 3, n - 1, 0], list(range(n)), []):
        sel = np.array(ids, dtype=np.int64)
        got = run_hits(eng, reads, cap, ids=np.array(ids, dtype=np.uint32))
        check(got, exp_hits[sel], exp_n[sel], st[sel], "ids %s" % ids[:6])
    # a column-sharded engine refuses
    eng.set_column_shard(0, 2)
    with pytest.raises(capi.RBError) as ei:
        run_hits(eng, reads, cap)
    assert ei.value.status == capi.RB_ERR_INVALID_ARG
    eng.set_column_shard(0, 1)
    check(run_hits(eng, reads, cap), exp_hits, exp_n, st, "after the shard is lifted")
    eng.destroy()


@pytest.mark.gpu
def test_device_form_packed_chunked_ids_statuses_and_stream():
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda:0")
    f, reads = make_case("w144")
    reads = list(reads)
    k = f.kmer_size
    eng = capi.Engine(0, [upload(f)], [])
    buf, offs, lens = H.pack_reads(reads)
    n, cap = len(reads), 24
    t_seq, t_off, t_len = (torch.from_numpy(a).to(dev) for a in (buf, offs.view(np.int64), lens.view(np.int32)))

    def run(n_items, max_len, **kw):
        o = {"hits": torch.full((max(n_items, 1) * cap * 8,), SENT, dtype=torch.uint8, device=dev),
             "n_hits": torch.full((max(n_items, 1), 1), 77, dtype=torch.int32, device=dev),
             "status": torch.full((max(n_items, 1),), 77, dtype=torch.uint8, device=dev), "bin_reads": torch.zeros(f.n_bins, dtype=torch.int64, device=dev)}
        torch.cuda.synchronize()
        seq = kw.pop("d_seqs", t_seq.data_ptr())
        off = kw.pop("d_offsets", t_off.data_ptr())
        eng.hits_device(seq, off, t_len.data_ptr(), n_items, max_len, error_rate=R, significance=CONF, max_hits=cap, d_hits=o["hits"].data_ptr(),
                        d_n_hits=o["n_hits"].data_ptr(), d_status=o["status"].data_ptr(), d_bin_reads=o["bin_reads"].data_ptr(), **kw)
        torch.cuda.synchronize()
        return {"hits": o["hits"].cpu().numpy().view(HIT).reshape(-1, 1, cap)[:n_items], "n_hits": o["n_hits"].cpu().numpy().view(np.uint32)[:n_items],
                "status": o["status"].cpu().numpy()[:n_items], "bin_reads": o["bin_reads"].cpu().numpy().view(np.uint64)}

    def expect(items, status):
        h, c, p, _ = expected_arrays([f], items, status == capi.RB_OK, cap, sentinel=SENT)
        return h, c, p

    def same(got, items, status, what):
        h, c, p = expect(items, status)
        check(got, h, c, status, what)
        assert np.array_equal(got["bin_reads"], p), what

    max_len = int(lens.max())
    st = status_of(reads, k)
    same(run(n, max_len), reads, st, "device form")
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        got = run(n, max_len, stream=s.cuda_stream)
    same(got, reads, st, "caller's stream")
    # an understated max_len: the longer reads are refused per item -- no hits, no record written, no profile contribution
    cut = int(np.sort(lens)[n // 2])
    st_cut = st.copy()
    st_cut[lens > cut] = capi.RB_ERR_INVALID_ARG
    assert (lens > cut).any()
    same(run(n, cut), reads, st_cut, "understated max_len")
    # read ids on the device
    ids = np.array([4, 4, 0, n - 1, 17, 4], dtype=np.uint32)
    t_ids = torch.from_numpy(ids.view(np.int32)).to(dev)
    same(run(len(ids), max_len, d_read_ids=t_ids.data_ptr()), [reads[i] for i in ids], st[ids.astype(np.int64)], "device ids")
    # chunks; a chunk that starts beyond the read is RB_ERR_BAD_CHUNK
    for start, length in ((100, 200), (0, 150), (300, 0)):
        chunks = [r[start:start + length] if length else r[start:] for r in reads]
        st_c = status_of(chunks, k)
        for i, r in enumerate(reads):
            if start > len(r):
                st_c[i] = capi.RB_ERR_BAD_CHUNK
        assert (st_c == capi.RB_OK).any() and ((st_c == capi.RB_ERR_BAD_CHUNK).any() or start == 0)
        same(run(n, max_len, chunk_start=start, chunk_length=length), chunks, st_c, "chunk %d+%d" % (start, length))
    # packed 2-bit reads with an N bitmap, whole and chunked
    packed, p_offs, nmask, n_offs = capi.pack_reads(buf, offs, lens)
    t_p, t_po, t_nm, t_no = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (packed, p_offs.view(np.int64), nmask, n_offs.view(np.int64)))
    pk = dict(d_seqs=t_p.data_ptr(), d_offsets=t_po.data_ptr(), d_nmask=t_nm.data_ptr(), d_nmask_offsets=t_no.data_ptr())
    same(run(n, max_len, **pk), reads, st, "packed")
    chunks = [r[64:64 + 180] for r in reads]
    st_c = status_of(chunks, k)
    for i, r in enumerate(reads):
        if 64 > len(r):
            st_c[i] = capi.RB_ERR_BAD_CHUNK
    same(run(n, max_len, chunk_start=64, chunk_length=180, **pk), chunks, st_c, "packed chunk")
    # n_hits alone with max_hits == 0; no output at all is refused
    only = torch.full((n, 1), -5, dtype=torch.int32, device=dev)
    eng.hits_device(t_seq.data_ptr(), t_off.data_ptr(), t_len.data_ptr(), n, max_len, error_rate=R, significance=CONF, max_hits=0, d_n_hits=only.data_ptr())
    assert np.array_equal(only.cpu().numpy().view(np.uint32), expect(reads, st)[1])
    with pytest.raises(capi.RBError) as ei:
        eng.hits_device(t_seq.data_ptr(), t_off.data_ptr(), t_len.data_ptr(), n, max_len, d_status=only.data_ptr())
    assert ei.value.status == capi.RB_ERR_INVALID_ARG
    eng.destroy()


def sub_batch_items(n_bins, cap):
    """work items per sub-batch of rb_hits_batch, from the budget the boundary header states: workspace (S x 2 x cap records and
    S x 2 counters per item, S = the most column slices of any filter) plus staged outputs (nf x cap records, nf counters, a status
    byte and a read id per item) at or below 256 MiB, one item at a time where a single item needs more"""
    W = max((b + 63) // 64 for b in n_bins)
    S = (W + 127) // 128 if W > 64 else 1
    per_item = S * 2 * (cap * 8 + 4) + len(n_bins) * (cap * 8 + 4) + 1 + 4
    return max(1, (256 << 20) // per_item)


@pytest.mark.gpu
def test_host_call_in_several_sub_batches():
    """a cap large enough that the host call cannot take its items in one piece: with and without read ids, over a sentinel buffer,
    with a profile; and a cap so large that every item goes alone"""
    f, reads = make_case("w485")
    reads = list(reads)
    st = status_of(reads, f.kmer_size)
    cap = 2 * f.n_bins
    per = sub_batch_items([f.n_bins], cap)
    exp_hits, exp_n, exp_prof, _ = expected_arrays([f], reads, st == capi.RB_OK, cap, min_count=1, sentinel=SENT)
    assert int(exp_n.max()) <= cap
    eng = capi.Engine(0, [upload(f)], [])
    # read ids: every read three times and then some, in an order that is not the reads'
    ids = np.concatenate([np.arange(len(reads))[::-1], np.arange(len(reads)), np.arange(len(reads))[::2], np.arange(len(reads))]).astype(np.uint32)
    assert len(ids) > 2 * per and len(ids) % per != 0  # three sub-batches or more, the last one short
    sel = ids.astype(np.int64)
    prof = np.zeros(f.n_bins, np.uint64)
    got = run_hits(eng, reads, cap, min_count=1, ids=ids, profile=prof)
    check(got, exp_hits[sel], exp_n[sel], st[sel], "sub-batches, read ids")
    want_prof = np.zeros(f.n_bins, np.uint64)
    for i in sel:
        if exp_n[i, 0]:
            want_prof[np.unique(exp_hits[i, 0, :exp_n[i, 0]]["bin"])] += 1
    assert np.array_equal(prof, want_prof)
    # without ids: the reads themselves, four times over
    many = [reads[i] for i in np.concatenate([np.arange(len(reads))] * 4)]
    assert len(many) > 2 * per and len(many) % per != 0
    rep4 = np.concatenate([np.arange(len(reads))] * 4)
    prof = np.zeros(f.n_bins, np.uint64)
    got = run_hits(eng, many, cap, min_count=1, profile=prof)
    check(got, exp_hits[rep4], exp_n[rep4], st[rep4], "sub-batches, no ids")
    assert np.array_equal(prof, 4 * exp_prof)
    # one item alone needs more than the budget
    huge = 4_000_000
    assert sub_batch_items([f.n_bins], huge) == 1 and (256 << 20) // (9 * (huge * 8 + 4) + 5) == 0
    few = reads[:2] + [reads[-1]] + [reads[5]]
    st_few = status_of(few, f.kmer_size)
    h, c, p, _ = expected_arrays([f], few, st_few == capi.RB_OK, huge, sentinel=SENT)
    prof = np.zeros(f.n_bins, np.uint64)
    got = run_hits(eng, few, huge, profile=prof)
    check(got, h, c, st_few, "one item per sub-batch")
    assert np.array_equal(prof, p) and c.any() and (st_few != capi.RB_OK).any()
    eng.destroy()


@pytest.mark.gpu
def test_scale_on_the_8_gib_filter_sample_through_the_oracle_rest_against_locate():
    """config 3's filter (8 GiB, 128 word columns: the non-temporal 16-byte-lane build, as the engine picks it) and 200 000 reads, which
    the host call takes in several sub-batches: a seeded sample of 2 000 goes through the oracle, every read is cross-checked against the
    locate pass"""
    dep, ref = synth.build_device_filter(0, synth.WORKLOADS["c3"], fill_seed=4, plant_seed=40)
    n, cap = 200_000, 128
    buf, offs, lens = synth.make_reads(79, n, 360, ref)
    eng = capi.Engine(0, [dep], [])
    n_bins = int(dep.info["n_bins"])
    assert n > 2 * sub_batch_items([n_bins], cap)  # several sub-batches
    prof = np.zeros(n_bins, np.uint64)
    got = eng.hits(buf, offs, lens, error_rate=R, significance=CONF, max_hits=cap, bin_reads=prof, hits=sentinel_hits(n, 1, cap))
    loc = eng.locate(buf, offs, lens, error_rate=R, significance=CONF)
    nh = got["n_hits"][:, 0].astype(np.int64)
    assert not got["status"].any() and int(np.count_nonzero(nh)) > n // 4 and int(np.count_nonzero(nh == 0)) > n // 4
    assert int(nh.max()) <= cap  # every list is whole
    rec = got["hits"][:, 0, :]
    valid = np.arange(cap)[None, :] < nh[:, None]
    assert (rec["reserved"][valid] == 0).all() and (np.ascontiguousarray(rec).view(np.uint8).reshape(n, cap, 8)[~valid] == SENT).all()
    new_bin = valid.copy()
    new_bin[:, 1:] &= rec["bin"][:, 1:] != rec["bin"][:, :-1]  # lists rise in (bin, strand): a bin is new where it differs from the one before
    assert np.array_equal(new_bin.sum(axis=1), loc["hit_bins"][:, 0].astype(np.int64))
    top = np.where(valid, rec["count"], 0).max(axis=1)
    has = nh > 0
    assert np.array_equal(top[has], loc["max_count"][has, 0])
    key = rec["bin"].astype(np.int64) * 2 + rec["strand"]
    assert (np.diff(key, axis=1)[valid[:, 1:]] > 0).all()
    assert int(prof.sum()) == int(new_bin.sum()) and np.array_equal(prof, np.bincount(rec["bin"][new_bin], minlength=n_bins).astype(np.uint64))
    # the sample through the oracle
    host = dep.download()
    orc = po.OracleIBF.wrap(host.info["n_bins"], 3, 13, host.info["n_bits"], host.words())
    sample = np.sort(np.random.default_rng(5).choice(n, size=2000, replace=False))
    sub = [buf[int(offs[i]):int(offs[i]) + int(lens[i])].tobytes().decode() for i in sample]
    exp_hits, exp_n, _, _ = expected_arrays([orc], sub, np.ones(len(sub), bool), cap, sentinel=SENT)
    assert int(exp_n.max()) <= cap and int(np.count_nonzero(exp_n)) > 400
    check({"hits": got["hits"][sample], "n_hits": got["n_hits"][sample], "status": got["status"][sample]}, exp_hits, exp_n,
          np.zeros(len(sub), np.uint8), "sample")
    eng.destroy()
    dep.free()

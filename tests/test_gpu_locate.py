"""The locate pass (rb_locate_batch / rb_locate_batch_device) against the oracle, bit for bit, through the C ABI.

The oracle side of every case is `OracleIBF.count()` on the read and on `revcomp()` of it, reduced in numpy by the rules of the
boundary header (tests/locate_rules.py, itself checked on hand-written vectors in test_locate_cpu.py), and `pyoracle.threshold()`
for t.  Filters are made by the ORACLE on the host and uploaded, so that every condition a case depends on -- enough reads on
either side of the threshold, planted ties really being ties -- is asserted on the oracle's numbers before the GPU is looked at
(test_case_conditions_hold_on_the_oracle checks the same without a GPU).  No assertion on elapsed time."""
import functools

import numpy as np
import pytest

from oracle import pyoracle as po
from readbouncer_amd import capi
from tests import helpers as H
from tests.locate_rules import places_at_max, reduce_locate

# name -> (n_bins, n_blocks, n_hash, k): W = ceil(n_bins / 64) word columns; block counts are powers of two (mask) or not (Barrett)
GEOMETRIES = {
    "w1": (64, 16384, 3, 13),
    "w2": (100, 16411, 3, 13),
    "w4": (243, 16384, 3, 13),
    "w5": (300, 16411, 3, 13),
    "w5_h2": (300, 16384, 2, 13),      # run-time hash path
    "w16": (1000, 16384, 3, 13),
    "w37_k15": (2340, 16411, 3, 15),
    "w128": (8190, 16384, 3, 13),
    "w129": (8200, 16411, 3, 13),      # two column slices, the second holds one column
    "w485": (31000, 16411, 3, 13),     # four slices of 16-byte lanes, odd column count
}
LONG = {"w5_long": (300, 131101, 3, 13)}  # reads of more than 1 023 k-mers: fragments of 2 400 bp, so more blocks for the same load
FRAG = 800
R, CONF = 0.1, 0.95


def revcomp_str(s):
    return s[::-1].translate(str.maketrans("ACGT", "TGCA"))


@functools.lru_cache(maxsize=None)
def make_case(name, n_reads=300, long_reads=False):
    """filter (oracle) + reads + the indices of the planted-tie reads: everything but the GPU"""
    n_bins, n_blocks, h, k = (LONG if long_reads else GEOMETRIES)[name]
    W = (n_bins + 63) // 64
    seed = sum(name.encode()) + (1000 if long_reads else 0)
    rng = np.random.default_rng(seed)
    f = po.OracleIBF(n_bins, h, k, 64 * W * n_blocks)
    frag = 2400 if long_reads else FRAG
    tie3, tie_same, tie_low = (7, 40, n_bins - 1), 20, (3, n_bins - 2)  # (bins of the same fragment), (fragment + its reverse complement), (rev bin, fwd bin)
    taken = set(tie3) | {tie_same} | set(tie_low)
    free = [b for b in range(n_bins) if b not in taken]
    bins = sorted(rng.choice(free, size=min(24, len(free)), replace=False).tolist())
    frags = [H.random_dna(rng, frag) for _ in bins]
    for b, s in zip(bins, frags):
        f.insert(po.encode(s), b)
    t1, t2, t3 = (H.random_dna(rng, frag) for _ in range(3))
    for b in tie3:
        f.insert(po.encode(t1), b)
    f.insert(po.encode(t2), tie_same)
    f.insert(po.encode(revcomp_str(t2)), tie_same)
    f.insert(po.encode(t3), tie_low[1])
    f.insert(po.encode(revcomp_str(t3)), tie_low[0])
    lo, hi = (1100, 1500) if long_reads else (120, 600)
    reads = []
    for i in range(n_reads):
        L = int(rng.integers(lo, hi + 1))
        if i % 2 == 0:
            src = frags[int(rng.integers(0, len(frags)))]
            s = int(rng.integers(0, len(src) - L + 1))
            r = H.mutate(rng, src[s:s + L], float(rng.uniform(0.05, 0.15)))
            if i % 8 == 0:  # some Ns
                a = np.frombuffer(r.encode(), dtype=np.uint8).copy()
                a[rng.random(L) < 0.01] = ord("N")
                r = a.tobytes().decode()
        else:
            r = H.random_dna(rng, L)
        reads.append(r)
    planted = {}
    for key, src in (("three_bins", t1), ("both_strands", t2), ("rev_lower", t3)):
        for _ in range(3):
            L = int(rng.integers(lo, hi + 1))
            s = int(rng.integers(0, len(src) - L + 1))
            planted.setdefault(key, []).append(len(reads))
            reads.append(src[s:s + L])
    reads += ["ACGT", "A" * (k - 1), ""]  # shorter than k
    want = {"three_bins": (7, 0), "both_strands": (tie_same, 0), "rev_lower": (tie_low[0], 1)}
    return f, tuple(reads), planted, want


def oracle_rows(filters, reads, r=R, conf=CONF):
    """expected outputs for whole reads: dict of arrays like Engine.locate, plus the thresholds [n, nf]"""
    n, nf = len(reads), len(filters)
    kmax = max(f.kmer_size for f in filters)
    out = {"max_count": np.zeros((n, nf), np.uint16), "best_bin": np.full((n, nf), -1, np.int32), "best_strand": np.zeros((n, nf), np.uint8),
           "hit_bins": np.zeros((n, nf), np.uint32), "status": np.zeros(n, np.uint8)}
    thr = np.zeros((n, nf), np.int64)
    places = np.zeros((n, nf), np.int64)
    for i, read in enumerate(reads):
        if len(read) < kmax:
            out["status"][i] = capi.RB_ERR_SHORT_READ
            continue
        o = po.encode(read)
        rc = po.revcomp(o)
        for j, f in enumerate(filters):
            t = po.threshold(len(o), f.kmer_size, r, conf)
            fwd, rev = f.count(o), f.count(rc)
            m, b, s, hits = reduce_locate(fwd, rev, t)
            out["max_count"][i, j], out["best_bin"][i, j], out["best_strand"][i, j], out["hit_bins"][i, j] = m, b, s, hits
            thr[i, j] = t
            places[i, j] = places_at_max(fwd, rev)
    return out, thr, places


def check_conditions(name, exp, thr, places, planted, want, n_body):
    m, t = exp["max_count"][:n_body, 0].astype(np.int64), thr[:n_body, 0]
    above = int(np.count_nonzero((m >= t) & (t >= 1)))
    below = int(np.count_nonzero(m < t))
    assert 3 * above >= n_body and 3 * below >= n_body, (name, above, below, n_body)
    for key, idx in planted.items():
        for i in idx:
            assert places[i, 0] >= 2, (name, key, i, places[i, 0])
            assert (int(exp["best_bin"][i, 0]), int(exp["best_strand"][i, 0])) == want[key], (name, key, i)


@functools.lru_cache(maxsize=None)
def case_with_expectation(name, n_rule=3, long_reads=False):
    f, reads, planted, want = make_case(name, 300 if not long_reads else 60, long_reads)
    prev = po.set_revcomp_of_n(n_rule)
    try:
        exp, thr, places = oracle_rows([f], reads)
    finally:
        po.set_revcomp_of_n(prev)
    n_body = len(reads) - 3 - sum(len(v) for v in planted.values())
    check_conditions(name, exp, thr, places, planted, want, n_body)
    return f, reads, exp


@pytest.mark.parametrize("name", ["w1", "w5", "w129"])
def test_case_conditions_hold_on_the_oracle(name):
    """runs without a GPU: the seeds give every geometry both sides of the threshold and real ties (three of the geometries here, all
    of them again -- the same assertion -- before the GPU is looked at below)"""
    case_with_expectation(name)


def upload(f):
    host = capi.HostIBF.create(f.n_bins, f.n_hash, f.kmer_size, f.n_bits)
    w = f.words()
    host.words()[:len(w)] = w
    return capi.DeviceIBF.upload(0, host)


def assert_same(got, exp, what):
    for key in ("status", "max_count", "best_bin", "best_strand", "hit_bins"):
        if not np.array_equal(got[key], exp[key]):
            bad = np.argwhere(got[key] != exp[key])[:5]
            raise AssertionError("%s: %s differs at %s: got %s, expected %s" % (what, key, bad.tolist(), got[key][tuple(bad.T)].tolist(),
                                                                               exp[key][tuple(bad.T)].tolist()))


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(GEOMETRIES))
def test_locate_matches_oracle(name):
    f, reads, exp = case_with_expectation(name)
    d = upload(f)
    eng = capi.Engine(0, [d], [])
    buf, offs, lens = H.pack_reads(list(reads))
    got = eng.locate(buf, offs, lens, error_rate=R, significance=CONF)
    assert_same(got, exp, name)
    # the raw maximum of the classify path (engine at its defaults: pruning on, the planner's forms) -- not through the oracle
    maxcount, _, _, _ = eng.classify(buf, offs, lens, error_rate=R, significance=CONF)
    assert np.array_equal(maxcount, got["max_count"]), name
    # the other N rule
    f4, reads4, exp4 = case_with_expectation(name, 4)
    eng.set_revcomp_of_n(4)
    assert_same(eng.locate(buf, offs, lens, error_rate=R, significance=CONF), exp4, name + " (N stays N)")
    eng.destroy()


@pytest.mark.gpu
def test_locate_reads_of_more_than_1023_kmers():
    """the 16-plane builds"""
    f, reads, exp = case_with_expectation("w5_long", 3, True)
    assert max(len(r) for r in reads) - 13 + 1 > 1023
    d = upload(f)
    eng = capi.Engine(0, [d], [])
    buf, offs, lens = H.pack_reads(list(reads))
    got = eng.locate(buf, offs, lens, error_rate=R, significance=CONF)
    assert_same(got, exp, "long reads")
    maxcount, _, _, _ = eng.classify(buf, offs, lens, error_rate=R, significance=CONF)
    assert np.array_equal(maxcount, got["max_count"])
    eng.destroy()


@pytest.mark.gpu
def test_locate_on_an_empty_filter():
    k = 13
    f = po.OracleIBF(100, 3, k, 128 * 4099)
    zero = [L for L in range(k, 400) if po.threshold(L, k, R, CONF) == 0]
    some = [L for L in range(k, 400) if 1 <= po.threshold(L, k, R, CONF) < 60000]
    assert zero and some  # lengths on both sides of t == 0
    rng = np.random.default_rng(9)
    reads = [H.random_dna(rng, L) for L in (zero[0], zero[-1], some[0], some[-1], 250)]
    exp, thr, _ = oracle_rows([f], reads)
    assert sorted(set(exp["hit_bins"][:, 0].tolist())) == [0, 100] and not exp["max_count"].any() and (exp["best_bin"] == -1).all()
    eng = capi.Engine(0, [upload(f)], [])
    buf, offs, lens = H.pack_reads(reads)
    assert_same(eng.locate(buf, offs, lens, error_rate=R, significance=CONF), exp, "empty filter")
    eng.destroy()


def four_filter_engine():
    names = ["w2", "w129", "w1", "w37_k15"]  # two deplete + two target filters of different geometry (and k)
    cases = [make_case(n) for n in names]
    filters = [c[0] for c in cases]
    reads = []
    for c in cases:
        reads += list(c[1][:40]) + list(c[1][-12:])
    devs = [upload(f) for f in filters]
    return filters, reads, devs


@pytest.mark.gpu
def test_locate_several_filters_and_engine_settings():
    """output column order (deplete filters first), and the engine's settings do not reach the locate pass"""
    filters, reads, devs = four_filter_engine()
    exp, _, _ = oracle_rows(filters, reads)
    assert (exp["status"] == capi.RB_ERR_SHORT_READ).any() and (exp["status"] == capi.RB_OK).any()
    buf, offs, lens = H.pack_reads(reads)
    eng = capi.Engine(0, devs[:2], devs[2:])
    base = eng.locate(buf, offs, lens, error_rate=R, significance=CONF)
    assert_same(base, exp, "four filters")
    for what, change in (("early decision", lambda e: e.set_early_decision(1)), ("no pruning", lambda e: e.set_bound_pruning(0)),
                         ("merge always", lambda e: e.set_merge(2)), ("merge never", lambda e: e.set_merge(0))):
        change(eng)
        eng.classify(buf, offs, lens, error_rate=R, significance=CONF)  # (lets the setting take effect on the classify path)
        assert_same(eng.locate(buf, offs, lens, error_rate=R, significance=CONF), exp, what)
    # a selection of reads, by id: one, repeated, all, none
    n = len(reads)
    for ids in ([5], [3, 3, 7, 3, n - 1, 0], list(range(n)), []):
        got = eng.locate(buf, offs, lens, read_ids=np.array(ids, dtype=np.uint32), error_rate=R, significance=CONF)
        sel = {k: v[np.array(ids, dtype=np.int64)] for k, v in exp.items()}
        assert_same(got, sel, "ids %s" % ids[:6])
    # a column-sharded engine refuses
    eng.set_column_shard(0, 2)
    with pytest.raises(capi.RBError) as ei:
        eng.locate(buf, offs, lens)
    assert ei.value.status == capi.RB_ERR_INVALID_ARG
    eng.set_column_shard(0, 1)
    assert_same(eng.locate(buf, offs, lens, error_rate=R, significance=CONF), exp, "after the shard is lifted")
    eng.destroy()


@pytest.mark.gpu
def test_locate_device_form_packed_chunked_subsets_and_stream():
    torch = pytest.importorskip("torch")
    dev = torch.device("cuda:0")
    f, reads, _, _ = make_case("w129")
    reads = list(reads[:60]) + list(reads[-12:])
    k = f.kmer_size
    eng = capi.Engine(0, [upload(f)], [])
    buf, offs, lens = H.pack_reads(reads)
    n = len(reads)
    t_seq, t_off, t_len = (torch.from_numpy(a).to(dev) for a in (buf, offs.view(np.int64), lens.view(np.int32)))

    def run(n_items, max_len, **kw):
        o = {"max_count": torch.full((max(n_items, 1), 1), 77, dtype=torch.int16, device=dev), "best_bin": torch.full((max(n_items, 1), 1), 77, dtype=torch.int32, device=dev),
             "best_strand": torch.full((max(n_items, 1), 1), 77, dtype=torch.uint8, device=dev), "hit_bins": torch.full((max(n_items, 1), 1), 77, dtype=torch.int32, device=dev),
             "status": torch.full((max(n_items, 1),), 77, dtype=torch.uint8, device=dev)}
        torch.cuda.synchronize()
        seq = kw.pop("d_seqs", t_seq.data_ptr())
        off = kw.pop("d_offsets", t_off.data_ptr())
        eng.locate_device(seq, off, t_len.data_ptr(), n_items, max_len, error_rate=R, significance=CONF, d_max_count=o["max_count"].data_ptr(),
                          d_best_bin=o["best_bin"].data_ptr(), d_best_strand=o["best_strand"].data_ptr(), d_hit_bins=o["hit_bins"].data_ptr(),
                          d_status=o["status"].data_ptr(), **kw)
        torch.cuda.synchronize()
        return {"max_count": o["max_count"].cpu().numpy().view(np.uint16)[:n_items], "best_bin": o["best_bin"].cpu().numpy()[:n_items],
                "best_strand": o["best_strand"].cpu().numpy()[:n_items], "hit_bins": o["hit_bins"].cpu().numpy().view(np.uint32)[:n_items],
                "status": o["status"].cpu().numpy()[:n_items]}

    max_len = int(lens.max())
    exp, _, _ = oracle_rows([f], reads)
    assert_same(run(n, max_len), exp, "device form")
    # a caller's stream
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        got = run(n, max_len, stream=s.cuda_stream)
    assert_same(got, exp, "caller's stream")
    # an understated max_len: the longer reads are refused per item, the others are located
    cut = int(np.sort(lens)[n // 2])
    exp_cut = {key: v.copy() for key, v in exp.items()}
    over = lens > cut
    assert over.any() and (~over).any()
    exp_cut["status"][over] = capi.RB_ERR_INVALID_ARG
    exp_cut["max_count"][over] = 0
    exp_cut["best_bin"][over] = -1
    exp_cut["best_strand"][over] = 0
    exp_cut["hit_bins"][over] = 0
    assert_same(run(n, cut), exp_cut, "understated max_len")
    # read ids on the device
    ids = np.array([4, 4, 0, n - 1, 17, 4], dtype=np.uint32)
    t_ids = torch.from_numpy(ids.view(np.int32)).to(dev)
    assert_same(run(len(ids), max_len, d_read_ids=t_ids.data_ptr()), {key: v[ids.astype(np.int64)] for key, v in exp.items()}, "device ids")
    # chunks: bases [start, start + length) of every read; a chunk that starts beyond the read is RB_ERR_BAD_CHUNK
    for start, length in ((100, 200), (0, 150), (300, 0)):
        chunks = [r[start:start + length] if length else r[start:] for r in reads]
        exp_c, _, _ = oracle_rows([f], chunks)
        for i, r in enumerate(reads):
            if start > len(r):
                exp_c["status"][i] = capi.RB_ERR_BAD_CHUNK
        assert (exp_c["status"] == capi.RB_OK).any()
        assert_same(run(n, max_len, chunk_start=start, chunk_length=length), exp_c, "chunk %d+%d" % (start, length))
    # packed 2-bit reads with an N bitmap
    packed, p_offs, nmask, n_offs = capi.pack_reads(buf, offs, lens)
    t_p, t_po, t_nm, t_no = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (packed, p_offs.view(np.int64), nmask, n_offs.view(np.int64)))
    assert_same(run(n, max_len, d_seqs=t_p.data_ptr(), d_offsets=t_po.data_ptr(), d_nmask=t_nm.data_ptr(), d_nmask_offsets=t_no.data_ptr()), exp, "packed")
    exp_c, _, _ = oracle_rows([f], [r[64:64 + 180] for r in reads])
    for i, r in enumerate(reads):
        if 64 > len(r):
            exp_c["status"][i] = capi.RB_ERR_BAD_CHUNK
    assert_same(run(n, max_len, d_seqs=t_p.data_ptr(), d_offsets=t_po.data_ptr(), d_nmask=t_nm.data_ptr(), d_nmask_offsets=t_no.data_ptr(), chunk_start=64,
                    chunk_length=180), exp_c, "packed chunk")
    # not every output is needed; none is refused
    only = torch.full((n, 1), -5, dtype=torch.int32, device=dev)
    eng.locate_device(t_seq.data_ptr(), t_off.data_ptr(), t_len.data_ptr(), n, max_len, error_rate=R, significance=CONF, d_best_bin=only.data_ptr())
    assert np.array_equal(only.cpu().numpy(), exp["best_bin"])
    with pytest.raises(capi.RBError) as ei:
        eng.locate_device(t_seq.data_ptr(), t_off.data_ptr(), t_len.data_ptr(), n, max_len)
    assert ei.value.status == capi.RB_ERR_INVALID_ARG
    eng.destroy()


@pytest.mark.gpu
def test_cli_report_bins_and_bin_map(tmp_path):
    """build --write-bin-map, classify with and without --report-bins: without the flag nothing new is written and the FASTA outputs
    are the same bytes; with it, classified_bins.tsv holds the oracle's line for every classified read, record id included"""
    import hashlib
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cli = os.path.join(root, "readbouncer_amd", "readbouncer_amd_cli")

    def run(*args):
        p = subprocess.run([cli] + list(args), capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
        return p.stdout

    def config(path, usage, out, **ibf):
        lines = ['usage = "%s"' % usage, "output_directory = '%s'" % out, "log_directory = '%s/logs'" % out, "", "[IBF]"]
        for key, v in ibf.items():
            lines.append("%s = [%s]" % (key, ", ".join("'%s'" % x for x in v)) if isinstance(v, list) else "%s = %s" % (key, v))
        path.write_text("\n".join(lines) + "\n")

    rng = np.random.default_rng(23)
    chr_a = H.random_dna(rng, 5300)
    chr_b = H.random_dna(rng, 1500) + "N" * 40 + H.random_dna(rng, 2200)  # cutOutNNNs shifts what follows the run of N
    (tmp_path / "tgt.fasta").write_text(">chrA first record\n%s\n>chrB\n%s\n" % (chr_a, chr_b))
    out_b = tmp_path / "built"
    config(tmp_path / "b.toml", "build", out_b, kmer_size=13, fragment_size=1000, target_files=[tmp_path / "tgt.fasta"])
    run("--config", str(tmp_path / "b.toml"), "--write-bin-map")
    # the bin map: the fragments of each record after cutOutNNNs, bins numbered through
    rows = [l.split("\t") for l in (out_b / "tgt.bins.tsv").read_text().splitlines() if not l.startswith("#")]
    assert rows[0] == ["bin", "record_id", "start", "end"] and "cutOutNNNs" in (out_b / "tgt.bins.tsv").read_text().splitlines()[0]
    want_map = []
    for rid, seq in (("chrA", chr_a), ("chrB", chr_b)):
        s, e = capi.fragment_bounds(len(po.cut_out_nnns(seq)), 1000, 13)
        want_map += [(rid, int(a), int(b)) for a, b in zip(s, e)]
    assert [(r[1], int(r[2]), int(r[3])) for r in rows[1:]] == want_map and [int(r[0]) for r in rows[1:]] == list(range(len(want_map)))
    oracle = po.OracleIBF.load(str(out_b / "tgt.ibf"))
    assert oracle.n_bins == len(want_map) and len(want_map) >= 9

    reads = []
    for i in range(400):
        L = int(rng.integers(300, 700))
        if i % 3 == 0:
            s = H.random_dna(rng, L)
        elif i % 3 == 1:
            g = chr_a if i % 2 else chr_b.replace("N", "")
            p = int(rng.integers(0, len(g) - L))
            s = H.mutate(rng, g[p:p + L], 0.06)
            if i % 4 == 0:
                s = revcomp_str(s)
        else:  # random first chunk, reference after it: classified by the second chunk
            p = int(rng.integers(0, len(chr_a) - L))
            s = H.random_dna(rng, 250) + chr_a[p:p + L - 250]
        reads.append(("r%d" % i, s))
    fq = tmp_path / "reads.fastq"
    with open(fq, "w") as fh:
        for n, s in reads:
            fh.write("@%s some comment\n%s\n+\n%s\n" % (n, s, "I" * len(s)))
    outs = {}
    for tag, extra in (("plain", []), ("bins", ["--report-bins", "--bin-map", str(out_b / "tgt.bins.tsv")])):
        out = tmp_path / ("out_" + tag)
        config(tmp_path / (tag + ".toml"), "classify", out, kmer_size=13, fragment_size=1000, target_files=[out_b / "tgt.ibf"], read_files=[fq],
               chunk_length=250, max_chunks=2)
        run("--config", str(tmp_path / (tag + ".toml")), "--segment-bytes", "20000", *extra)
        outs[tag] = {p.name: hashlib.sha256(p.read_bytes()).hexdigest() for p in sorted(out.iterdir()) if p.is_file()}
    assert "classified_bins.tsv" not in outs["plain"]
    assert set(outs["bins"]) == set(outs["plain"]) | {"classified_bins.tsv"}
    for name in outs["plain"]:
        if name.endswith(".fasta"):
            assert outs["plain"][name] == outs["bins"][name], name
    want = ["read_id\tfilter\tbest_bin\tstrand\tmax_count\tthreshold\thit_bins\tchunk\trecord_id"]
    chunks_seen = set()
    for n, s in reads:
        for c in range(2):
            chunk = s[c * 250:(c + 1) * 250]
            o = po.encode(chunk)
            t = po.threshold(len(o), 13, 0.1, 0.95)
            m, b, strand, hits = reduce_locate(oracle.count(o), oracle.count(po.revcomp(o)), t)
            if m > 0 and m >= t:
                want.append("%s\ttgt\t%d\t%s\t%d\t%d\t%d\t%d\t%s" % (n, b, "-" if strand else "+", m, t, hits, c, want_map[b][0]))
                chunks_seen.add((c, strand))
                break
    assert chunks_seen >= {(0, 0), (0, 1), (1, 0)} and len(want) > 200  # both chunks and both strands are reported
    assert (tmp_path / "out_bins" / "classified_bins.tsv").read_text().splitlines() == want

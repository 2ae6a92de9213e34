"""The kernels that WRITE filters, bit for bit against the oracle: the insert kernel (K4, behind rb_dibf_insert and
rb_dibf_add_sequence), the re-stride kernel (upload, download, resize_bins), fill_synth and compare_bits.

The count tests cannot see most of what goes wrong here: a raw maximum is a max over bins, so a k-mer written into the wrong bin
changes no count, and a stray bit in a padding word or past n_bins in the last column changes one only if some read hashes there.
So every filter built on the GPU is compared as an image with the oracle's own build (never with a download of the GPU image):
the payload words, the stored .ibf file byte for byte, and compare(d, d)["file_bits"] -- the popcount of the whole padded HBM image,
padding words included -- against the popcount of the oracle's payload.  A last test asserts that every stride class, h, k class,
block-count form, alphabet class and fragment edge of the matrix was reached."""
import os
import subprocess
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import pyoracle as po
from readbouncer_amd import capi
from tests import helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "readbouncer_amd", "readbouncer_amd_cli")

_reached = {}     # axis -> values a passing check went through
_tests_run = set()


def _reach(axis, *values):
    _reached.setdefault(axis, set()).update(values)


def hbm_stride(W):
    """rb_engine.hip, hbm_stride"""
    if W % 16 == 0:
        return W
    if W < 16:
        s = 1
        while s < W:
            s <<= 1
        return s
    return (W + 15) // 16 * 16


def popcount(words):
    return int(np.bitwise_count(np.ascontiguousarray(words, dtype=np.uint64)).sum(dtype=np.uint64))


def blocks_form(n_blocks):
    if n_blocks == 1:
        return "1"
    if n_blocks & (n_blocks - 1) == 0:
        return "pow2"
    if all(n_blocks % p for p in range(2, int(n_blocks ** 0.5) + 1)):
        return "prime"
    return "odd" if n_blocks % 2 else "even"


def geometry_axes(o):
    """record the geometry of an insert image that matched"""
    _reach("W", o.bin_width)
    _reach("stride", (o.bin_width, hbm_stride(o.bin_width)))
    _reach("bins%64", "zero" if o.n_bins % 64 == 0 else "non-zero")
    _reach("h", o.n_hash)
    _reach("k", o.kmer_size)
    _reach("n_blocks", blocks_form(o.n_blocks))
    if o.n_bits > o.n_blocks * o.bin_width * 64:
        _reach("n_blocks", "tail")


def check_image(d, o, tmp_path, nonempty=True):
    """d (GPU) against o (oracle build): payload words, the stored files, and no bit in the padded image outside the payload"""
    assert (d.info["n_bins"], d.info["n_hash"], d.info["kmer_size"], d.info["n_bits"]) == (o.n_bins, o.n_hash, o.kmer_size, o.n_bits)
    host = d.download()
    nw = o.n_bits // 64
    got, want = host.words()[:nw], o.words()[:nw]
    if not np.array_equal(got, want):
        bad = np.flatnonzero(got != want)
        w = int(bad[0])
        raise AssertionError("image differs in %d words; first: word %d (block %d, column %d) gpu %#x oracle %#x"
                             % (len(bad), w, w // o.bin_width, w % o.bin_width, int(got[w]), int(want[w])))
    gp, op = str(tmp_path / "gpu.ibf"), str(tmp_path / "oracle.ibf")
    host.store(gp)
    o.store(op)
    with open(gp, "rb") as a, open(op, "rb") as b:
        assert a.read() == b.read(), "stored files differ"
    payload = popcount(o.words()[:o.n_blocks * o.bin_width])
    c = d.compare(d)
    assert c["file_bits"] == c["rebuilt_bits"] == payload, ("bits of the padded HBM image outside the payload", c, payload)
    assert c["new_bits"] == 0 and c["payload_bits"] == o.n_blocks * o.n_bins
    if nonempty:
        assert payload > 0
    return payload


# ---- inputs ---------------------------------------------------------------------------------------------------------
ALPHABET = {
    "upper": b"ACGT",
    "lower": b"acgt",
    "mixed": b"AcGtaCgT",
    "U": b"ACGUu",
    "IUPAC": b"RYKMSWBDHVrykmswbdhv",
    "non-letter": b"-*.0@[`{\x00\x7f\x80\xc1\xe1\xff",
}


def alphabet_seq(rng, n):
    """n bytes made of stretches of every alphabet class, with N and n runs between them"""
    out, classes = [], list(ALPHABET)
    while sum(map(len, out)) < n:
        cls = classes[int(rng.integers(len(classes)))]
        if cls in ("upper", "lower", "mixed"):
            L = int(rng.integers(20, 400))
        else:  # rare classes stay short so that most k-mers carry no N
            L = int(rng.integers(1, 4))
            out.append(bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), size=int(rng.integers(30, 120)))))
        alpha = np.frombuffer(ALPHABET[cls], np.uint8)
        out.append(bytes(rng.choice(alpha, size=L)))
        r = rng.random()
        if r < 0.08:
            out.append(b"N" * int(rng.integers(1, 60)))
        elif r < 0.16:
            out.append(b"n" * int(rng.integers(1, 60)))
    s = b"".join(out)[:n]
    _reach("alphabet", *ALPHABET, "N-run", "n-run")
    return s


def edge_fragments(rng, L, k, n_bins, n_random):
    """(starts, ends, bins, edges): the fragment edges of K4's prefix search and of the reference's fragmenter, then random ones"""
    fr, edges = [], set()

    def pos(length):
        return int(rng.integers(0, L - length))

    s = pos(600)
    fr += [(s, s + 600, n_bins - 1)]; edges.add("last bin")
    fr += [(pos(0), None, int(rng.integers(n_bins))) for _ in range(3)]; edges.add("zero-length")
    fr += [(pos(k - 1), None, n_bins + 7)]; edges.add("shorter than k, bin >= n_bins")
    s = pos(k)
    fr += [(s, s + k, int(rng.integers(n_bins)))]; edges.add("exactly k")
    s = pos(900)
    fr += [(s, s + 500, 0), (s + 200, s + 900, min(1, n_bins - 1))]; edges.add("overlapping")
    s = pos(300)
    b = int(rng.integers(n_bins))
    fr += [(s, s + 300, b), (s, s + 300, b)]; edges.add("repeated")
    # k-mer-less fragments packed between long ones: the prefix table holds runs of equal entries there
    for _ in range(4):
        s = pos(700)
        fr += [(s, s + 700, int(rng.integers(n_bins)))]
        for _ in range(int(rng.integers(1, 5))):
            t = pos(k)
            fr += [(t, t + int(rng.integers(0, k)), int(rng.integers(n_bins + 100)))]
    edges.add("k-mer-less between long")
    for _ in range(n_random):
        ln = int(rng.integers(0, 3 * k))
        s = pos(ln)
        fr += [(s, s + ln, int(rng.integers(n_bins)))]
    starts = np.array([a for a, _, _ in fr], dtype=np.uint64)
    ends = np.array([a if e is None else e for a, e, _ in fr], dtype=np.uint64)
    bins = np.array([b for _, _, b in fr], dtype=np.uint64)
    assert not np.all(np.diff(bins.astype(np.int64)) >= 0)
    edges.add("bins out of order")
    return starts, ends, bins, edges


def insert_both(d, o, seq, starts, ends, bins):
    d.insert(seq, starts, ends, bins)
    ords = po.encode(seq)
    for s, e, b in zip(starts.tolist(), ends.tolist(), bins.tolist()):
        o.insert(ords[s:e], b)


def add_sequence_both(d, o, seq, fragment_length, first_bin, overlap):
    nb = d.add_sequence(seq, fragment_length, first_bin, overlap)
    assert nb == o.add_sequence(po.encode(seq), fragment_length, first_bin, overlap)
    return nb


# ---- 1-2. the insert image matrix --------------------------------------------------------------------------------------
# (n_bins, n_blocks, tail bits past the last block, h, k): every width class W in {1,2,3,4,5,8,9,16,17,33,130} (and so every stride
# class of hbm_stride), n_bins % 64 zero and not, n_blocks of 1, powers of two (pow2_mask), odd and prime (Barrett), every h and k
INSERT_MATRIX = [
    (64, 1, 0, 1, 5),
    (37, 65536, 41, 3, 32),
    (100, 2, 0, 2, 13),
    (128, 3003, 64, 4, 5),
    (150, 1024, 0, 3, 19),
    (256, 65536, 0, 4, 21),
    (300, 4099, 100, 5, 27),
    (512, 3003, 0, 8, 28),
    (550, 1, 300, 3, 31),
    (1024, 2, 0, 5, 32),
    (1039, 1024, 17, 1, 21),
    (2112, 4099, 0, 2, 28),
    (8300, 1021, 5000, 8, 13),
    (200, 7919, 0, 3, 19),
]
BIG_CALL = {(150, 1024, 0, 3, 19), (2112, 4099, 0, 2, 28)}  # these also take one call of >= 100 000 fragments


@pytest.mark.parametrize("n_bins,n_blocks,tail,h,k", INSERT_MATRIX)
def test_insert_image_matches_oracle(tmp_path, n_bins, n_blocks, tail, h, k):
    W = (n_bins + 63) // 64
    n_bits = n_blocks * W * 64 + tail
    rng = np.random.default_rng(n_bins * 7 + n_blocks + k)
    d = capi.DeviceIBF.create(0, n_bins, h, k, n_bits)
    o = po.OracleIBF(n_bins, h, k, n_bits)
    assert (o.n_blocks, o.bin_width) == (n_blocks, W) == (d.info["n_blocks"], d.info["bin_width"])
    # explicit fragment lists over a sequence of every alphabet class; several calls OR into the one filter
    seq = alphabet_seq(rng, 40000)
    text = bytes(c for c in seq if c < 0x80).decode()  # (the Python bindings of cutOutNNNs take text)
    assert capi.cut_out_nnns(text) == po.cut_out_nnns(text)
    for _ in range(2):
        starts, ends, bins, edges = edge_fragments(rng, len(seq), k, n_bins, 300)
        insert_both(d, o, seq, starts, ends, bins)
    _reach("fragments", *edges, "several calls")
    # the reference's fragmenter: every overlap rule, first_bin > 0, the last fragment in bin n_bins - 1
    F = max(2 * k, 60)
    for overlap in (0, 1, k - 1, 1500):
        part = alphabet_seq(rng, int(rng.integers(3 * F, 6 * F)))
        n_frag = len(capi.fragment_bounds(len(part), F, k, overlap)[0])
        assert n_frag < n_bins
        first = n_bins - n_frag if overlap == 1500 else int(rng.integers(1, n_bins - n_frag + 1))
        add_sequence_both(d, o, part, F, first, overlap)
        _reach("add_sequence overlap", {0: "0", 1: "1", k - 1: "k-1", 1500: "1500"}[overlap])
        _reach("fragments", "first_bin > 0")
    if (n_bins, n_blocks, tail, h, k) in BIG_CALL:
        big = alphabet_seq(rng, 800000)
        n = 120000
        ln = rng.integers(0, 3 * k, size=n)
        ln[rng.random(n) < 0.3] = 0
        starts = rng.integers(0, len(big) - 3 * k, size=n).astype(np.uint64)
        ends = starts + ln.astype(np.uint64)
        bins = rng.integers(0, n_bins, size=n).astype(np.uint64)
        insert_both(d, o, big, starts, ends, bins)
        _reach("fragments", ">= 100000 fragments in one call")
    check_image(d, o, tmp_path)
    geometry_axes(o)
    _tests_run.add(("insert", n_bins, n_blocks))


# ---- 3. fill_synth at every stride class -------------------------------------------------------------------------------
FILL_MATRIX = [(64, 3001), (37, 4096), (128, 1001), (150, 999), (256, 1024), (300, 777), (512, 513), (550, 211), (1024, 129),
               (1039, 131), (2112, 67), (8300, 9)]


@pytest.mark.parametrize("n_bins,n_blocks", FILL_MATRIX)
def test_fill_synth_image_matches_oracle(tmp_path, n_bins, n_blocks):
    W = (n_bins + 63) // 64
    n_bits = n_blocks * W * 64 + 77
    d = capi.DeviceIBF.create(0, n_bins, 3, 13, n_bits)
    o = po.OracleIBF(n_bins, 3, 13, n_bits)
    seed = 1000 + n_bins
    d.fill_synth(seed)
    o.fill_synth(seed)
    check_image(d, o, tmp_path)
    _reach("fill_synth W", W)
    _tests_run.add(("fill", n_bins))


# ---- 4. re-stride paths --------------------------------------------------------------------------------------------------
RESIZES = [(64, 65, 2003), (192, 256, 1024), (256, 257, 1001), (1024, 1025, 257), (2000, 4200, 131)]


@pytest.mark.parametrize("old_bins,new_bins,n_blocks", RESIZES)
def test_resize_bins_then_update_matches_oracle(tmp_path, old_bins, new_bins, n_blocks):
    k, F = 15, 100
    rng = np.random.default_rng(old_bins + new_bins)
    W = (old_bins + 63) // 64
    n_bits = n_blocks * W * 64
    d = capi.DeviceIBF.create(0, old_bins, 3, k, n_bits)
    o = po.OracleIBF(old_bins, 3, k, n_bits)
    starts, ends, bins, _ = edge_fragments(rng, 200000, k, old_bins, 2000)
    seq = alphabet_seq(rng, 200000)
    insert_both(d, o, seq, starts, ends, bins)
    d2, o2 = d.resize_bins(new_bins), o.resize_bins(new_bins)
    d.free()
    assert d2.device_stride() == hbm_stride(o2.bin_width)
    # update_filter: the new bins from old_bins to the last one, in order
    extra = new_bins - old_bins
    if extra:
        part = H.random_dna(rng, (extra - 1) * F + F // 2).encode()
        nb = add_sequence_both(d2, o2, part, F, old_bins, 1500)
        assert nb == new_bins
    check_image(d2, o2, tmp_path)
    _reach("resize", (hbm_stride(W), hbm_stride(o2.bin_width)))
    _tests_run.add(("resize", old_bins, new_bins))


ROUNDTRIP_BINS = [64, 100, 150, 256, 300, 512, 550, 1024, 1039, 2112, 8300]


@pytest.mark.parametrize("n_bins", ROUNDTRIP_BINS)
def test_file_upload_open_and_clone_keep_the_bits(tmp_path, n_bins):
    """an oracle-built file through HostIBF.open -> upload -> download -> store, and through DeviceIBF.open -> clone_to -> download"""
    rng = np.random.default_rng(n_bins)
    W = (n_bins + 63) // 64
    n_blocks = 1031 if W < 40 else 97
    n_bits = n_blocks * W * 64 + 13
    o = po.OracleIBF(n_bins, 3, 13, n_bits)
    seq = alphabet_seq(rng, 100000)
    starts, ends, bins, _ = edge_fragments(rng, len(seq), 13, n_bins, 1500)
    ords = po.encode(seq)
    for s, e, b in zip(starts.tolist(), ends.tolist(), bins.tolist()):
        o.insert(ords[s:e], b)
    path = str(tmp_path / "file.ibf")
    o.store(path)
    d1 = capi.DeviceIBF.upload(0, capi.HostIBF.open(path))
    d2 = capi.DeviceIBF.open(0, path)
    d3 = d2.clone_to(0)
    for d in (d1, d2, d3):  # (check_image stores the download and compares it with the oracle's file, byte for byte)
        assert d.device_stride() == hbm_stride(W)
        check_image(d, o, tmp_path)
    _reach("roundtrip W", W)
    _tests_run.add(("roundtrip", n_bins))


# ---- 5. rb_dibf_compare against numpy --------------------------------------------------------------------------------
COMPARES = [(64, 37, "below 64 words"), (150, 1001, "not a multiple of 256 words"), (64, (1 << 21) + 4099, "past the grid-stride cap")]


@pytest.mark.parametrize("n_bins,n_blocks,size", COMPARES)
def test_compare_counts_match_numpy(tmp_path, n_bins, n_blocks, size):
    k, h = 19, 3
    rng = np.random.default_rng(n_blocks)
    W = (n_bins + 63) // 64
    n_bits = n_blocks * W * 64
    n_x = 40 if n_blocks < 64 else min(700000, n_blocks * 2)
    x, y = H.random_dna(rng, n_x).encode(), H.random_dna(rng, n_x // 2).encode()
    F = max(n_x // 30, 2 * k)
    a, b = capi.DeviceIBF.create(0, n_bins, h, k, n_bits), capi.DeviceIBF.create(0, n_bins, h, k, n_bits)
    oa, ob = po.OracleIBF(n_bins, h, k, n_bits), po.OracleIBF(n_bins, h, k, n_bits)
    nb = add_sequence_both(a, oa, x, F, 0, 1500)
    add_sequence_both(b, ob, x, F, 0, 1500)
    add_sequence_both(b, ob, y, F, nb, 1500)
    check_image(a, oa, tmp_path)
    check_image(b, ob, tmp_path)
    used = n_blocks * W
    wa, wb = oa.words()[:used], ob.words()[:used]
    want = {"file_bits": popcount(wa), "rebuilt_bits": popcount(wb), "new_bits": popcount(wb & ~wa), "payload_bits": n_blocks * n_bins}
    assert want["new_bits"] > 0
    if n_blocks * hbm_stride(W) > 8192 * 256:
        assert popcount(wa[8192 * 256:]) > 0  # words only the second pass of the grid-stride loop reaches
    assert a.compare(b) == want
    back = dict(want, file_bits=want["rebuilt_bits"], rebuilt_bits=want["file_bits"], new_bits=popcount(wa & ~wb))
    assert b.compare(a) == back and back["new_bits"] == 0
    _reach("compare", size)
    _tests_run.add(("compare", n_blocks))


# ---- 6. bit indices above 2^32 ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_blocks", [1 << 31, (1 << 32) - 1])
def test_large_block_indices(n_blocks):
    import torch

    n_bins, h, k = 64, 3, 21
    table = n_blocks * 8
    free, _ = torch.cuda.mem_get_info(0)
    if free < 1.25 * table:
        pytest.skip("needs %.1f GiB of free HBM, %.1f GiB free" % (1.25 * table / 2**30, free / 2**30))
    rng = np.random.default_rng(n_blocks)
    capi.set_placement_tries(1)
    try:
        d = capi.DeviceIBF.create(0, n_bins, h, k, n_blocks * 64)
    finally:
        capi.set_placement_tries(5)  # (the library's default)
    try:
        assert d.info["n_blocks"] == n_blocks
        # only block_index is called on this oracle: its calloc'd words are never touched
        o = po.OracleIBF(n_bins, h, k, n_blocks * 64)
        ref = H.random_dna(rng, 400000)
        n_frag, flen = 3000, 60
        starts = rng.integers(0, len(ref) - flen, size=n_frag).astype(np.uint64)
        ends = starts + flen
        bins = (np.arange(n_frag) * 7 % n_bins).astype(np.uint64)
        bins[:64] = np.arange(64)
        d.insert(ref.encode(), starts, ends, bins)
        ords = po.encode(ref)
        expected = set()
        for s, b in zip(starts.tolist(), bins.tolist()):
            for p in range(s, s + flen - k + 1):
                v = po.kmer_value(ords[p:p + k], k)
                for i in range(h):
                    expected.add(o.block_index(v, i) * 64 + b)
        del o
        assert max(expected) >= 1 << 36
        c = d.compare(d)
        assert c["file_bits"] == len(expected) and c["payload_bits"] == n_blocks * n_bins, (c, len(expected))
        reads = [ref[int(s):int(s) + flen] for s in starts[:200]] + [H.random_dna(rng, 200) for _ in range(200)]
        buf, offs, lens = H.pack_reads(reads)
        want = np.array([flen - k + 1] * 200 + [0] * 200)
        eng = capi.Engine(0, [d], [])
        for form, threshold in (("latency", 4096), ("throughput", 0)):
            eng.set_split_threshold(threshold)
            p = eng.plan(0, len(reads), int(lens.max()))
            assert (p["kernel"] == "ibf_count_max_split_kernel") == (form == "latency"), (form, p)
            maxcount = eng.classify(buf, offs, lens)[0]
            assert np.array_equal(maxcount[:, 0], want), form
        eng.destroy()
    finally:
        d.free()
    _reach("large", blocks_form(n_blocks))
    _tests_run.add(("large", n_blocks))


# ---- 7. unsupported geometries are refused before anything is allocated ---------------------------------------------------
def _refused(fn):
    import torch

    free0, _ = torch.cuda.mem_get_info(0)
    t0 = time.perf_counter()
    with pytest.raises(capi.RBError) as e:
        fn()
    dt = time.perf_counter() - t0
    free1, _ = torch.cuda.mem_get_info(0)
    assert e.value.status == capi.RB_ERR_UNSUPPORTED, str(e.value)
    assert dt < 0.5, ("refused only after %.2f s" % dt)
    assert abs(free1 - free0) < 256 << 20
    return str(e.value)


def test_unsupported_geometry_is_refused_before_allocation(tmp_path):
    capi.DeviceIBF.create(0, 64, 3, 13, 64 * 64).free()  # (device initialised before anything is timed)
    assert "2^32-1 blocks" in _refused(lambda: capi.DeviceIBF.create(0, 64, 3, 13, (1 << 32) * 64))
    assert "2^32-1 blocks" in _refused(lambda: capi.DeviceIBF.create(0, 64, 3, 13, (1 << 40) * 64))
    assert "hash functions" in _refused(lambda: capi.DeviceIBF.create(0, 64, 9, 13, 64 * 64 * 1000))
    assert "k-mer size" in _refused(lambda: capi.DeviceIBF.create(0, 64, 3, 33, 64 * 64 * 1000))
    for h, k in ((9, 13), (3, 33)):
        host = capi.HostIBF.create(100, h, k, 128 * 50)
        _refused(lambda: capi.DeviceIBF.upload(0, host))
        path = str(tmp_path / ("h%d_k%d.ibf" % (h, k)))
        po.OracleIBF(100, h, k, 128 * 50).store(path)
        _refused(lambda: capi.DeviceIBF.open(0, path))
    d = capi.DeviceIBF.create(0, 64, 3, 13, 64 * 64)
    assert "too many bins" in _refused(lambda: d.resize_bins(1 << 31))
    _tests_run.add(("refused",))


# ---- 8. the CLI's build of an awkward FASTA ---------------------------------------------------------------------------------
def test_cli_build_of_an_awkward_fasta(tmp_path):
    rng = np.random.default_rng(808)
    k, F = 13, 1000
    soft = list(H.random_dna(rng, 60000))
    for s in rng.integers(0, 59000, size=40).tolist():
        soft[s:s + 400] = [c.lower() for c in soft[s:s + 400]]
    for s in rng.integers(0, 59000, size=15).tolist():
        r = int(rng.integers(1, 30))
        soft[s:s + r] = ["n"] * r
    soft = "".join(soft)
    soft = soft[:30000] + "N" * 25 + soft[30000:]
    seqs = [H.random_dna(rng, 10),                             # shorter than k: not a reference record
            "N" * 50,                                          # all N: one bin, no fragment
            H.random_dna(rng, 40000) + "NNNN",                 # ends in N
            soft,                                              # soft-masked, n runs
            H.random_dna(rng, 40500, with_n=0.001)]
    fasta = tmp_path / "awkward.fasta"
    with open(fasta, "wb") as fh:
        for i, s in enumerate(seqs):
            fh.write(b">rec%d description\r\n" % i)
            for j in range(0, len(s), 61):
                fh.write(s[j:j + 61].encode() + b"\r\n")
    o = H.build_filter_like_reference(seqs, k=k, fragment_length=F)
    assert 128 < o.n_bins <= 192 and o.bin_width == 3 and hbm_stride(o.bin_width) == 4
    out = tmp_path / "out"
    cfg = tmp_path / "build.toml"
    cfg.write_text('usage = "build"\noutput_directory = \'%s\'\nlog_directory = \'%s/logs\'\n\n[IBF]\nkmer_size = %d\n'
                   'fragment_size = %d\ntarget_files = [\'%s\']\n' % (out, out, k, F, fasta))
    p = subprocess.run([CLI, "--config", str(cfg), "--placement-tries", "1"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout, p.stderr)
    op = tmp_path / "oracle.ibf"
    o.store(str(op))
    assert (out / "awkward.ibf").read_bytes() == op.read_bytes()
    p = subprocess.run([CLI, "--verify-ibf", str(out / "awkward.ibf"), "--reference", str(fasta), "--fragment-size", str(F)],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "VERIFY OK" in p.stdout and " new_bits=0 " in p.stdout, (p.stdout, p.stderr)
    _tests_run.add(("cli",))


# ---- 9. coverage of the matrix ------------------------------------------------------------------------------------------------
EXPECTED = {
    "W": {1, 2, 3, 4, 5, 8, 9, 16, 17, 33, 130},
    "stride": {(W, hbm_stride(W)) for W in (1, 2, 3, 4, 5, 8, 9, 16, 17, 33, 130)},
    "bins%64": {"zero", "non-zero"},
    "h": {1, 2, 3, 4, 5, 8},
    "k": {5, 13, 19, 21, 27, 28, 31, 32},
    "n_blocks": {"1", "pow2", "odd", "prime", "tail"},
    "alphabet": set(ALPHABET) | {"N-run", "n-run"},
    "fragments": {"last bin", "zero-length", "shorter than k, bin >= n_bins", "exactly k", "overlapping", "repeated",
                  "k-mer-less between long", "bins out of order", "several calls", "first_bin > 0", ">= 100000 fragments in one call"},
    "add_sequence overlap": {"0", "1", "k-1", "1500"},
    "fill_synth W": {1, 2, 3, 4, 5, 8, 9, 16, 17, 33, 130},
    "resize": {(1, 2), (4, 4), (4, 8), (16, 32), (32, 80)},
    "roundtrip W": {1, 2, 3, 4, 5, 8, 9, 16, 17, 33, 130},
    "compare": {"below 64 words", "not a multiple of 256 words", "past the grid-stride cap"},
}
ALL_TESTS = ({("insert", b, n) for b, n, _, _, _ in INSERT_MATRIX} | {("fill", b) for b, _ in FILL_MATRIX}
             | {("resize", a, b) for a, b, _ in RESIZES} | {("roundtrip", b) for b in ROUNDTRIP_BINS}
             | {("compare", n) for _, n, _ in COMPARES} | {("refused",), ("cli",)})


def test_every_builder_case_was_reached():
    """the matrix above was not quietly shrunk: every stride class, h, k, block-count form, alphabet class and fragment edge
    went through a check that passed (the large-index cases are reported by their own tests: they skip on a card without the HBM)"""
    if not ALL_TESTS <= _tests_run:
        pytest.skip("runs after the whole matrix of this file")
    for axis, want in EXPECTED.items():
        got = _reached.get(axis, set())
        assert want <= got, (axis, "never reached", sorted(map(str, want - got)))
    print("reached: " + "; ".join("%s: %s" % (a, sorted(map(str, v))) for a, v in sorted(_reached.items())))

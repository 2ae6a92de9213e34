"""rb_dibf_assemble / rb_dibf_select_bins on the GPU, through the C ABI.  No assertion on elapsed time.

The yardstick is never the kernel under test: the expected words come from the numpy model of tests/assemble_rules.py over the sources'
HOST images (itself held against an oracle rebuild in test_assemble_cpu.py), the expected hits from the oracle's count vectors on the
oracle-side rebuild, the expected occupancy from the model's column sums.  All comparisons are exact."""
import ctypes as C

import numpy as np
import pytest

from readbouncer_amd import capi
from tests import assemble_rules as R
from tests import helpers as H
from tests.hits_rules import expected_arrays
from tests.occupancy_rules import bin_occupancy

pytestmark = pytest.mark.gpu

SHAPES = {64: 1, 70: 2, 130: 4, 600: 16, 1100: 32, 8192: 128}  # bins -> stride in HBM (W = 1, 2, 3, 10, 18, 128)
N_BLOCKS = (1, 257, 4099)
# rb_set_assemble_grid: the built-in rule; a single workgroup; chunks of 1 block and of 5 blocks (many chunks per workgroup, a short last
# chunk, steps cut short by the chunk's end), with one workgroup and with the built-in number
GRIDS = ((0, 0), (1, 0), (1, 1), (1, 5), (0, 1), (0, 5))
K, HASHES = 13, 3

_cache = {}


def source(n_bins, n_blocks, seed=0):
    """-> (OracleIBF, sequences per bin, host words (a copy), DeviceIBF)"""
    key = (n_bins, n_blocks, seed)
    if key not in _cache:
        f, seqs = R.oracle_source(7919 * seed + 31 * n_bins + n_blocks, n_bins, n_blocks, HASHES, K)
        dev = upload(f.words(), n_bins, n_blocks)
        assert dev.device_stride() == SHAPES[n_bins] and dev.info["n_blocks"] == n_blocks
        _cache[key] = (f, seqs, f.words().copy(), dev)
    return _cache[key]


def upload(words, n_bins, n_blocks):
    host = capi.HostIBF.create(n_bins, HASHES, K, 64 * ((n_bins + 63) // 64) * n_blocks)
    assert host.info["n_words"] == len(words)
    host.words()[:] = words
    return capi.DeviceIBF.upload(0, host)


def words_of(dev):
    """the downloaded host image's words, copied (HostIBF.words() is a view that dies with the image)"""
    host = dev.download()
    return host.words().copy()


def reads_for(seq_lists, plan, rng):
    """64 reads: half cut from sequences the plan routes somewhere (or from any sequence when it routes none) and mutated, half random"""
    refs = [r for l in plan for r in l] or [(0, 0)]
    reads = []
    for i in range(64):
        L = int(rng.integers(K, 100))
        if i % 2:
            reads.append(H.random_dna(rng, L))
        else:
            f, b = refs[int(rng.integers(0, len(refs)))]
            s = seq_lists[f][b]
            a = int(rng.integers(0, len(s) - L + 1))
            reads.append(H.mutate(rng, s[a:a + L], 0.05))
    return reads


def check_case(sources, plan, grids=GRIDS, seed=1):
    """sources: [source(...)] of one n_blocks; plan: list of lists of (filter, bin).  Every check the issue lists per case."""
    n_blocks = sources[0][0].n_blocks
    n_out = len(plan)
    devs = [s[3] for s in sources]
    want = R.assemble_words([(s[2], s[0].n_bins, n_blocks) for s in sources], plan)
    out = None
    try:
        for grid in grids:
            capi.set_assemble_grid(*grid)
            if out is not None:
                out.free()
            out = capi.DeviceIBF.assemble(devs, plan)
            info = out.info
            assert info["n_bins"] == n_out and info["n_blocks"] == n_blocks and info["n_hash"] == HASHES and info["kmer_size"] == K
            assert info["n_bits"] == n_blocks * ((n_out + 63) // 64) * 64 and info["n_words"] == len(want)
            got = words_of(out)
            assert got.shape == want.shape and np.array_equal(got, want), (grid, int(np.flatnonzero(got != want)[0]))
    finally:
        capi.set_assemble_grid(0, 0)
    # the padded image as it lies: against an upload of the model's image, both ways
    model = upload(want, n_out, n_blocks)
    for a, b in ((out, model), (model, out)):
        c = a.compare(b)
        assert c["file_bits"] == c["rebuilt_bits"] and c["new_bits"] == 0, c
    # the sources are as they were; a second assemble gives the same words
    for s in sources:
        assert np.array_equal(words_of(s[3]), s[2])
    again = capi.DeviceIBF.assemble(devs, capi.assemble_plan(plan))  # (the CSR form)
    assert np.array_equal(words_of(again), want)
    again.free()
    # select_bins is the one-source, at-most-one-ref case
    if len(sources) == 1 and all(len(l) <= 1 for l in plan):
        sel = devs[0].select_bins([l[0][1] if l else None for l in plan])
        assert sel.info == out.info and np.array_equal(words_of(sel), want)
        sel.free()
    # per-bin occupancy of the result: the model's column sums
    assert np.array_equal(out.bin_occupancy(), bin_occupancy(want, n_out, n_blocks))
    # an engine over the assembled filter against the oracle's counts on the oracle-side rebuild
    seq_lists = [s[1] for s in sources]
    rebuilt = R.oracle_rebuild(seq_lists, plan, n_blocks, HASHES, K)
    assert np.array_equal(rebuilt.words(), want)
    reads = reads_for(seq_lists, plan, np.random.default_rng(seed))
    buf, offs, lens = H.pack_reads(reads)
    cap = 2 * n_out
    exp_hits, exp_n, _, _ = expected_arrays([rebuilt], reads, [True] * len(reads), cap, min_count=1, sentinel=0)
    eng = capi.Engine(0, [out], [])
    res = eng.hits(buf, offs, lens, min_count=1, max_hits=cap)
    eng.destroy()
    assert not res["status"].any() and np.array_equal(res["n_hits"], exp_n)
    assert np.array_equal(res["hits"], exp_hits.astype(capi.HIT_DTYPE))
    return out, want


@pytest.mark.parametrize("n_blocks", N_BLOCKS)
@pytest.mark.parametrize("n_bins", [64, 70, 130, 600, 1100])
@pytest.mark.parametrize("name", sorted(R.SINGLE_SOURCE))
def test_every_generator(name, n_bins, n_blocks):
    src = source(n_bins, n_blocks)
    plan = R.SINGLE_SOURCE[name](n_bins)
    out, want = check_case([src], plan)
    if name == "identity":
        assert np.array_equal(want, src[2]) and out.device_stride() == src[3].device_stride()
    if name == "all_empty":
        assert not want.any()


@pytest.mark.parametrize("n_blocks", N_BLOCKS)
def test_interleaved_join_of_three_sources_of_different_widths(n_blocks):
    sizes = [130, 70, 600]  # strides 4, 2 and 16 into one of 16
    srcs = [source(n, n_blocks, seed=i + 1) for i, n in enumerate(sizes)]
    out, _ = check_case(srcs, R.interleaved_join(sizes))
    assert out.info["n_bins"] == 800 and out.device_stride() == 16
    # ... and a join that names the sources unevenly, repeats refs across filters and leaves bins empty
    plan = [[] if j % 7 == 0 else [(0, j), (1, j % 70), (0, j), (2, 599 - j)] for j in range(74)] + [[(0, b) for b in range(130)]]
    check_case(srcs, plan, grids=((0, 0), (1, 5)))


@pytest.mark.parametrize("n_out", [1, 63, 64, 65, 128, 129])
def test_out_bin_counts_around_a_word(n_out):
    src = source(130, 257)
    out, _ = check_case([src], R.truncated(R.reversed_order(130), n_out))
    assert out.device_stride() == {1: 1, 63: 1, 64: 1, 65: 2, 128: 2, 129: 4}[n_out]


@pytest.mark.parametrize("n_blocks", [257, 4099])
def test_one_list_of_700_refs_is_beyond_any_held_length(n_blocks):
    src = source(1100, n_blocks)
    long_list = [(0, b) for b in range(150, 850)]
    plan = R.identity(70)
    plan[33] = long_list
    plan[64] = [(0, 9)] * 9  # one ref beyond the held length, all the same
    out, want = check_case([src], plan)
    col = R.unpack(want, 70, n_blocks)[:, 33]
    assert col.sum() == np.bitwise_or.reduce(R.unpack(src[2], 1100, n_blocks)[:, 150:850], axis=1).sum() > 0


def test_groups_of_8_on_the_8192_bin_shape():
    src = source(8192, 67)
    out, _ = check_case([src], R.groups_of(8192, 8))
    assert out.info["n_bins"] == 1024 and out.device_stride() == 16
    # both tiles of a 128-word output: the identity and the reversal of all 8 192 bins, the words alone
    for plan in (R.identity(8192), R.reversed_order(8192)):
        want = R.assemble_words([(src[2], 8192, 67)], plan)
        for grid in ((0, 0), (1, 5)):
            capi.set_assemble_grid(*grid)
            try:
                got = capi.DeviceIBF.assemble([src[3]], plan)
            finally:
                capi.set_assemble_grid(0, 0)
            assert got.device_stride() == 128 and np.array_equal(words_of(got), want)


def test_rejected_plans_return_invalid_arg_and_a_valid_call_still_works():
    L = capi.lib()
    a, b = source(130, 257), source(70, 257, seed=1)
    other_blocks = source(70, 4099)
    other_k = capi.DeviceIBF.create(0, 70, HASHES, 15, 64 * 2 * 257)
    other_h = capi.DeviceIBF.create(0, 70, 2, K, 64 * 2 * 257)
    good_off, good_refs = capi.assemble_plan([[(0, 1)], [(1, 2), (0, 129)], []])

    def call(srcs, offsets, refs, n_out, n_srcs=None, out=True):
        h = C.c_void_p()
        off = None if offsets is None else np.ascontiguousarray(offsets, dtype=np.uint64)
        rf = None if refs is None else np.ascontiguousarray(refs, dtype=capi.BIN_REF_DTYPE)
        st = L.rb_dibf_assemble(None if srcs is None else capi._handle_array(srcs), len(srcs or []) if n_srcs is None else n_srcs,
                                capi._ptr(off), capi._ptr(rf), n_out, C.byref(h) if out else None)
        msg = L.rb_last_error().decode()
        if st == capi.RB_OK:
            return st, msg, capi.DeviceIBF(h)
        assert not h.value
        return st, msg, None

    def refs_of(*pairs):
        return np.array(list(pairs), dtype=capi.BIN_REF_DTYPE)

    two = [a[3], b[3]]
    rejected = [
        ("null sources", call(None, good_off, good_refs, 3, n_srcs=2), "null"),
        ("null offsets", call(two, None, good_refs, 3), "null"),
        ("null refs", call(two, good_off, None, 3), "null"),
        ("null out", call(two, good_off, good_refs, 3, out=False), "null"),
        ("no sources", call(two, good_off, good_refs, 3, n_srcs=0), "0 sources"),
        ("nine sources", call([a[3]] * 9, good_off, good_refs, 3), "9 sources"),
        ("no out bins", call(two, good_off, good_refs, 0), "n_out_bins"),
        ("other n_blocks", call([a[3], other_blocks[3]], good_off, good_refs, 3), "source 1"),
        ("other kmer_size", call([a[3], other_k], good_off, good_refs, 3), "source 1"),
        ("other n_hash", call([a[3], b[3], other_h], good_off, good_refs, 3), "source 2"),
        ("offsets[0] != 0", call(two, [1, 1, 3, 3], good_refs, 3), "offsets[0]"),
        ("descending offsets", call(two, [0, 2, 1, 3], good_refs, 3), "out bin 1"),
        ("filter out of range", call(two, good_off, refs_of((0, 1), (2, 2), (0, 129)), 3), "out bin 1 names filter 2"),
        ("bin at n_bins", call(two, good_off, refs_of((0, 1), (1, 70), (0, 129)), 3), "out bin 1 names bin 70 of source 1"),
        ("bin beyond n_bins", call(two, good_off, refs_of((0, 130), (1, 2), (0, 129)), 3), "out bin 0 names bin 130 of source 0"),
    ]
    for what, (st, msg, _), needle in rejected:
        assert st == capi.RB_ERR_INVALID_ARG, (what, st, msg)
        assert needle in msg, (what, msg)
    for bins, needle in (([0, 130], "out bin 1 names bin 130"), ([], "n_out_bins")):
        arr = np.array(bins, dtype=np.uint64)
        h = C.c_void_p()
        assert L.rb_dibf_select_bins(a[3].h, capi._ptr(arr) if len(arr) else capi._ptr(np.zeros(1, np.uint64)), len(arr), C.byref(h)) == capi.RB_ERR_INVALID_ARG
        assert needle in L.rb_last_error().decode() and not h.value
    # a valid call straight afterwards
    st, _, out = call(two, good_off, good_refs, 3)
    assert st == capi.RB_OK
    want = R.assemble_words([(a[2], 130, 257), (b[2], 70, 257)], [[(0, 1)], [(1, 2), (0, 129)], []])
    assert np.array_equal(words_of(out), want)
    assert capi.assemble_last_seconds() > 0.0


def test_a_tile_whose_lists_span_more_than_the_staged_image_is_unsupported():
    """4 096 consecutive out bins whose lists together span more than 60 KiB (7 680 words) of one block of the sources are refused with
    RB_ERR_UNSUPPORTED before anything is launched (include/readbouncer_amd.h); the same bins in separate tiles, or a span just inside
    the limit, assemble to the model's words"""
    n_bins, n_blocks = 500000, 3  # W = 7 813 words
    src = capi.DeviceIBF.create(0, n_bins, HASHES, K, 64 * ((n_bins + 63) // 64) * n_blocks)
    rng = np.random.default_rng(5)
    picks = [0, 63, 64 * 7678 + 5, 64 * 7679 + 1, n_bins - 1]
    for b in picks:
        src.insert(H.random_dna(rng, 90), [0], [90], [b])
    words = words_of(src)
    assert all(R.unpack(words, n_bins, n_blocks)[:, b].any() for b in picks)
    L = capi.lib()

    def status(plan):
        off, refs = capi.assemble_plan(plan)
        h = C.c_void_p()
        st = L.rb_dibf_assemble(capi._handle_array([src]), 1, capi._ptr(off), capi._ptr(refs), len(plan), C.byref(h))
        return st, L.rb_last_error().decode(), (capi.DeviceIBF(h) if st == capi.RB_OK else None)

    st, msg, _ = status([[(0, 0)], [(0, n_bins - 1)]])  # words 0 and 7 812 in one tile: 7 813 + 1 staged words
    assert st == capi.RB_ERR_UNSUPPORTED and "out bins 0 to 1" in msg and "61440" in msg, (st, msg)
    st, msg, _ = status([[(0, 0), (0, 64 * 7679 + 1)]])  # words 0 .. 7 679: 7 680 + the zero word
    assert st == capi.RB_ERR_UNSUPPORTED, (st, msg)
    for plan in ([[(0, 63), (0, 64 * 7678 + 5)], []],                           # words 0 .. 7 678: 7 679 + the zero word, the widest that fits
                 [[(0, 0)]] + [[] for _ in range(4095)] + [[(0, n_bins - 1)]]):  # the refused pair, one tile apart
        st, msg, out = status(plan)
        assert st == capi.RB_OK, (st, msg)
        assert np.array_equal(words_of(out), R.assemble_words([(words, n_bins, n_blocks)], plan))
        out.free()

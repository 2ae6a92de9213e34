"""rb_dibf_bin_occupancy / rb_dibf_bin_occupancy_device on the GPU, through the C ABI.  No assertion on elapsed time.

The yardstick is never the kernel under test: expected counts come from the HOST image of the same filter (made by the oracle, or
downloaded from a GPU-built one) reduced in numpy by tests/occupancy_rules.py (itself checked on hand-written vectors in
test_bin_occupancy_cpu.py), from closed forms for patterns written through the device pointer, or from a torch reduction over the same
device words.  All integer comparisons are exact."""
import math
import os
import subprocess

import numpy as np
import pytest

from oracle import pyoracle as po
from readbouncer_amd import capi, synth
from tests import helpers as H
from tests.occupancy_rules import bin_occupancy, summary

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "readbouncer_amd", "readbouncer_amd_cli")
# name -> (n_bins, n_blocks, n_hash, k).  The ten geometries the locate tests use (strides 1, 2, 4, 8, 16, 48, 128, 144, 496; mask and
# Barrett block counts; n_bins not a multiple of 64), a 600-bin filter (W = 10 -> stride 16) and a one-word filter with a prime block count
GEOMETRIES = {
    "w1": (64, 16384, 3, 13),
    "w2": (100, 16411, 3, 13),
    "w4": (243, 16384, 3, 13),
    "w5": (300, 16411, 3, 13),
    "w5_h2": (300, 16384, 2, 13),
    "w16": (1000, 16384, 3, 13),
    "w37_k15": (2340, 16411, 3, 15),
    "w128": (8190, 16384, 3, 13),
    "w129": (8200, 16411, 3, 13),      # two column slices, the second holds one column
    "w485": (31000, 16411, 3, 13),     # four slices, odd column count
    "w10": (600, 16411, 3, 13),
    "w1_prime": (64, 16411, 3, 13),
}
PLANES = 12  # kOccPlanes of rb_kernels.hip: a lane's counters hold 2^12 - 1 rows between two flushes
FLUSH = 1 << PLANES
CHUNK_CAP, WAVES = 4080, 16  # kOccMaxChunkRows, kOccWaves: the most wave rows a wave walks between two flushes; waves per workgroup


def oracle_filter(name, n_fragments=24):
    n_bins, n_blocks, h, k = GEOMETRIES[name]
    W = (n_bins + 63) // 64
    rng = np.random.default_rng(sum(name.encode()) + 77)
    f = po.OracleIBF(n_bins, h, k, 64 * W * n_blocks)
    bins = sorted(rng.choice(n_bins, size=min(n_fragments, n_bins // 2), replace=False).tolist())
    for b in bins:
        f.insert(po.encode(H.random_dna(rng, int(rng.integers(300, 1200)))), b)
    return f, bins


def host_counts(host):
    return bin_occupancy(host.words(), host.info["n_bins"], host.info["n_blocks"])


def device_counts(dev):
    """host form, device form into a torch buffer on the default stream and on a stream of the caller: all three must agree"""
    import torch
    got = dev.bin_occupancy()
    n = dev.info["n_bins"]
    for stream in (None, torch.cuda.Stream()):
        t = torch.full((n,), -1, dtype=torch.int64, device="cuda:0")
        torch.cuda.synchronize()
        dev.bin_occupancy_device(t.data_ptr(), None if stream is None else stream.cuda_stream)
        if stream is not None:
            stream.synchronize()
        assert np.array_equal(t.cpu().numpy().view(np.uint64), got)
    return got


def check_summary(bits, info, max_fp=0.01):
    got, want = capi.bin_occupancy_summary(bits, info["n_blocks"], info["n_hash"], max_fp), summary(bits, info["n_blocks"], info["n_hash"], max_fp)
    for key, v in want.items():
        assert math.isclose(got[key], v, rel_tol=1e-12, abs_tol=0.0) if isinstance(v, float) else got[key] == v, (key, got[key], v)
    return got


def words_view(dev):
    """the filter's own device image as a torch tensor [n_blocks, stride] of int64 (writes go through rb_dibf_device_words)"""
    import torch

    class View:
        def __init__(self, ptr, n):
            self.__cuda_array_interface__ = {"shape": (n,), "typestr": "<i8", "data": (ptr, False), "version": 2}
    n_blocks, stride = dev.info["n_blocks"], dev.device_stride()
    t = torch.as_tensor(View(dev.device_words(), n_blocks * stride), device="cuda:0")
    assert t.data_ptr() == dev.device_words()
    return t.view(n_blocks, stride)


@pytest.mark.parametrize("name", sorted(GEOMETRIES))
def test_counts_equal_the_host_image(name):
    f, bins = oracle_filter(name)
    n_bins, n_blocks, h, k = GEOMETRIES[name]
    host = capi.HostIBF.create(n_bins, h, k, 64 * ((n_bins + 63) // 64) * n_blocks)
    w = f.words()
    host.words()[:len(w)] = w
    want = host_counts(host)
    assert np.count_nonzero(want) == len(bins) and (want[bins] > 0).all() and np.count_nonzero(want == 0) >= n_bins // 2
    dev = capi.DeviceIBF.upload(0, host)
    got = device_counts(dev)
    assert got.dtype == np.uint64 and np.array_equal(got, want)
    assert int(got.sum()) == dev.compare(dev)["file_bits"]  # a second, independent kernel
    s = check_summary(got, dev.info)
    assert s["empty_bins"] == n_bins - len(bins) and s["max_bin"] == int(np.argmax(want)) and s["bits_total"] == int(want.sum())


@pytest.mark.parametrize("name", ["w1", "w5", "w10", "w37_k15", "w128", "w485"])
def test_gpu_built_filters_and_resize(name):
    n_bins, n_blocks, h, k = GEOMETRIES[name]
    W = (n_bins + 63) // 64
    rng = np.random.default_rng(sum(name.encode()) + 5)
    dev = capi.DeviceIBF.create(0, n_bins, h, k, 64 * W * n_blocks)
    nxt = dev.add_sequence(H.random_dna(rng, 9000), 800, 0)
    nxt = dev.add_sequence(H.random_dna(rng, 700), 800, nxt + 3)
    assert 12 <= nxt <= n_bins
    want = host_counts(dev.download())
    got = device_counts(dev)
    assert np.array_equal(got, want) and np.count_nonzero(got) == nxt - 3
    assert int(got.sum()) == dev.compare(dev)["file_bits"]
    check_summary(got, dev.info)
    wider = dev.resize_bins(W * 64 + 17)  # one more word column: new bins report 0, old bins unchanged
    got_w = device_counts(wider)
    assert len(got_w) == W * 64 + 17 and np.array_equal(got_w[:n_bins], want) and not got_w[n_bins:].any()
    assert np.array_equal(got_w, host_counts(wider.download()))


@pytest.mark.parametrize("name", ["w5", "w37_k15", "w485"])
def test_pad_words_and_tail_bits_are_not_counted(name):
    f, _ = oracle_filter(name)
    n_bins, n_blocks, h, k = GEOMETRIES[name]
    W = (n_bins + 63) // 64
    host = capi.HostIBF.create(n_bins, h, k, 64 * W * n_blocks)
    w = f.words()
    host.words()[:len(w)] = w
    want = host_counts(host)
    dev = capi.DeviceIBF.upload(0, host)
    stride = dev.device_stride()
    assert stride > W and n_bins % 64 != 0
    import torch
    v = words_view(dev)  # inside the filter's own allocation: n_blocks * stride words
    v[:, W:] = -1
    v[:, W - 1] |= torch.tensor(-1 << (n_bins % 64), dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    capi._check(capi.lib().rb_dibf_touch(dev.h), "rb_dibf_touch")
    assert int(v[5, W].item()) == -1 and np.array_equal(device_counts(dev), want)


@pytest.mark.parametrize("name,n_blocks", [(g, n) for g in ("w1", "w128") for n in (FLUSH - 1, FLUSH, FLUSH + 1)] +
                         [("w1", 67108859), ("w128", 65537)])  # 2^26 - 5 and 2^16 + 1 are primes
def test_planes_do_not_wrap(name, n_blocks):
    """more blocks than 2^planes; a bin set in every block, one in none, one in every second block: closed-form counts.  (With the
    built-in grid a wave walks at most 256 rows of these tables per chunk: the lane-private planes near their limit, and several chunks
    per wave, are driven by test_full_length_chunks_and_several_per_wave below.)"""
    check_closed_form(name, n_blocks)


def check_closed_form(name, n_blocks):
    import torch
    n_bins = GEOMETRIES[name][0]
    W = (n_bins + 63) // 64
    dev = capi.DeviceIBF.create(0, n_bins, 3, 13, 64 * W * n_blocks)
    assert dev.info["n_blocks"] == n_blocks
    every, none, second, every_low = n_bins - 1, 1, 35, 2  # (every_low: a bin of the first column slice set in every block, too)
    v = words_view(dev)
    v[:, (n_bins - 1) // 64] |= torch.tensor(-(1 << 63) if every % 64 == 63 else 1 << (every % 64), dtype=torch.int64, device="cuda:0")
    v[0::2, 0] |= 1 << second
    v[:, 0] |= 1 << every_low
    torch.cuda.synchronize()
    capi._check(capi.lib().rb_dibf_touch(dev.h), "rb_dibf_touch")
    got = device_counts(dev)
    want = np.zeros(n_bins, dtype=np.uint64)
    want[every], want[every_low], want[second] = n_blocks, n_blocks, (n_blocks + 1) // 2
    assert got[none] == 0 and np.array_equal(got, want), (got[every], got[every_low], got[second], n_blocks)
    s = check_summary(got, dev.info)
    assert s["max_bin"] == every_low and s["max_load"] == 1.0 and s["min_bin"] == second and s["empty_bins"] == n_bins - 3


# One workgroup per column slice (rb_set_bin_occupancy_grid(1, 0)): 16 waves share the wave rows of a slice, so a table of
# 16 * CHUNK_CAP * iters wave rows makes every wave walk `iters` chunks of exactly CHUNK_CAP rows -- what a 16 GiB table does by itself
# on a whole GPU.  A bin set in every block then stands at 4 080 = 0xFF0 in a lane's planes before each flush (planes 4 to 11 set; one
# dropped plane, or a cap above 2^12 - 1, changes the count), and the flush-clear-continue sequence runs.  Wave rows hold 64 >> lg blocks:
#   w1       one-word blocks, 64 per wave row; iters 2, the last chunk short by a few blocks (the one-row-at-a-time tail)
#   w128     one block per wave row; iters 2, chunks exactly at the cap
#   w37_k15  stride 48: 24 of every 32 lanes hold columns, the others skip their chunks; 2 blocks per wave row; iters 3
#   w129     stride 144: the second slice (16 words, 8 blocks per wave row) has an eighth of the rows, so most of its waves find no chunk
#            at all and the others none in the second round; iters 2
@pytest.mark.parametrize("name,n_blocks,iters", [("w1", 64 * WAVES * CHUNK_CAP * 2 - 3, 2), ("w128", WAVES * CHUNK_CAP * 2, 2),
                                                 ("w37_k15", 2 * WAVES * CHUNK_CAP * 3 - 1, 3), ("w129", WAVES * CHUNK_CAP * 2, 2)])
def test_full_length_chunks_and_several_per_wave(name, n_blocks, iters):
    # the launcher's rule (rb_kernels.hip, launch_bin_occupancy), restated to make sure the case is what it says
    stride = {"w1": 1, "w128": 128, "w37_k15": 48, "w129": 144}[name]
    rows = -(-n_blocks // {"w1": 64, "w37_k15": 2}.get(name, 1))
    per_wave = -(-rows // WAVES)
    assert -(-per_wave // CHUNK_CAP) == iters and -(-(-(-per_wave // iters)) // 16) * 16 == CHUNK_CAP, (per_wave, iters)
    capi.set_bin_occupancy_grid(1, 0)
    try:
        check_closed_form(name, n_blocks)
    finally:
        capi.set_bin_occupancy_grid(0, 0)
    check_closed_form(name, n_blocks)  # and the built-in grid on the same table


def torch_sync():
    import torch
    torch.cuda.synchronize()


def torch_column_counts(dev, col):
    """bits of word column `col` by an independent reduction on the device: ((words >> j) & 1).sum() per bin"""
    import torch
    v = words_view(dev)[:, col]
    return np.array([int(((v >> j) & 1).sum().item()) for j in range(64)], dtype=np.uint64)


@pytest.mark.parametrize("n_bins", [8192, 64])
def test_design_load_fill_equals_a_torch_reduction(n_bins):
    W = n_bins // 64
    dev = capi.DeviceIBF.create(0, n_bins, 3, 13, 1 << 31)  # 256 MiB
    dev.fill_synth(21)
    got = device_counts(dev)
    for c in range(W):
        assert np.array_equal(got[c * 64:(c + 1) * 64], torch_column_counts(dev, c)), c
    assert int(got.sum()) == dev.compare(dev)["file_bits"]


def test_full_size_filter():
    """config 3's filter (8 GiB, 2^23 blocks of 128 words) under the synthetic fill.  Every bit of the fill is set independently with
    the probability the AND / OR tree of rbspec::synth_word gives: eight uniform bits combined as ((((((r7|r6)|r5)&r4)|r3)|r2)&r1)&r0, i.e.
    0.5 -> 0.75 -> 0.875 -> 0.4375 -> 0.71875 -> 0.859375 -> 0.4296875 -> p = 55 / 256 = 0.21484375, the eight-bit fraction below the
    design load 0.01^(1/3) = 0.21544.  (The issue names 0.01^(1/3) itself as p; the fill's own probability differs from it by 4.3 of the
    standard deviations below, so the bound is taken around 55 / 256 -- derived from the tree, not measured.)  A bin's load is a mean of
    2^23 such bits: sd = sqrt(p (1 - p) / 2^23) = 1.4e-4, and every bin must lie within 6 sd."""
    w = synth.WORKLOADS["c3"]
    dev = capi.DeviceIBF.create(0, w["n_bins"], w["h"], w["k"], synth.filter_bits(w))
    dev.fill_synth(4)
    n_blocks = dev.info["n_blocks"]
    assert n_blocks == 1 << 23 and dev.device_stride() == 128
    got = device_counts(dev)
    assert int(got.sum()) == dev.compare(dev)["file_bits"]
    for c in (0, 127, 41, 90):
        assert np.array_equal(got[c * 64:(c + 1) * 64], torch_column_counts(dev, c)), c
    p = 55.0 / 256.0
    sd = math.sqrt(p * (1.0 - p) / n_blocks)
    load = got.astype(np.float64) / n_blocks
    print("full size: load min %.6f max %.6f, p %.6f, sd %.3g, worst %.2f sd" % (load.min(), load.max(), p, sd, np.abs(load - p).max() / sd))
    assert np.abs(load - p).max() <= 6.0 * sd
    assert check_summary(got, dev.info)["empty_bins"] == 0
    # a bin set in EVERY block: each wave's chunk is 2 048 rows here, so the lane-private counters reach 2 048 (plane 11)
    words_view(dev)[:, 1] |= 1 << 13
    torch_sync()
    capi._check(capi.lib().rb_dibf_touch(dev.h), "rb_dibf_touch")
    full = dev.bin_occupancy()
    assert full[77] == n_blocks and np.array_equal(np.delete(full, 77), np.delete(got, 77))


def run_cli(*args, expect=0):
    p = subprocess.run([CLI] + [str(a) for a in args], capture_output=True, text=True, timeout=600)
    assert p.returncode == expect, (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
    return p.stdout


def read_tsv(path):
    rows = [l.split("\t") for l in path.read_text().splitlines()]
    return rows[0], rows[1:]


def test_cli_filter_stats(tmp_path):
    rng = np.random.default_rng(31)
    recs = [("chrA", H.random_dna(rng, 5300)), ("chrB", H.random_dna(rng, 1500) + "N" * 40 + H.random_dna(rng, 2200)), ("chrC", H.random_dna(rng, 700))]
    (tmp_path / "tgt.fasta").write_text("".join(">%s some text\n%s\n" % r for r in recs))
    out = tmp_path / "built"

    def config(path, out_dir):
        path.write_text("usage = \"build\"\noutput_directory = '%s'\nlog_directory = '%s/logs'\n\n[IBF]\nkmer_size = 13\nfragment_size = 1000\n"
                        "target_files = ['%s']\n" % (out_dir, out_dir, tmp_path / "tgt.fasta"))
    config(tmp_path / "b.toml", out)
    # (--max-fp 0.05: a bin built at the design load sits AT 0.01, on either side of it by chance)
    text = run_cli("--config", tmp_path / "b.toml", "--filter-stats", "--write-bin-map", "--max-fp", "0.05")
    assert "FILTER_STATS" in text and "bins_over_max_fp=0" in text
    built = (out / "tgt.binstats.tsv").read_bytes()
    text = run_cli("--filter-stats", out / "tgt.ibf", "--bin-map", out / "tgt.bins.tsv", "--max-fp", "0.05")
    assert "FILTER_STATS" in text and "fullest_bin=" in text and "chunk_length=360 threshold=%d " % capi.threshold(360, 13) in text
    assert (out / "tgt.binstats.tsv").read_bytes() == built  # the table in HBM at build time and the stored file give the same report
    head, rows = read_tsv(out / "tgt.binstats.tsv")
    assert head == ["bin", "bits", "load", "fpr", "est_kmers", "record_id", "start", "end"]
    dev = capi.DeviceIBF.open(0, str(out / "tgt.ibf"))
    bits = dev.bin_occupancy()
    load, fpr, est = capi.bin_occupancy_derive(bits, dev.info["n_blocks"], dev.info["n_hash"])
    assert [int(r[0]) for r in rows] == list(range(len(bits))) and np.array_equal(np.array([int(r[1]) for r in rows], dtype=np.uint64), bits)
    for col, want in ((2, load), (3, fpr), (4, est)):
        assert np.array_equal(np.array([float(r[col]) for r in rows]), want)  # printed with 17 digits: they read back exactly
    _, map_rows = read_tsv(out / "tgt.bins.tsv")
    map_rows = [r for r in map_rows if not r[0].startswith("#") and r[0] != "bin"]
    assert [r[5:] for r in rows] == [r[1:] for r in map_rows] and {r[5] for r in rows} == {"chrA", "chrB", "chrC"}
    assert np.array_equal(bits, host_counts(capi.HostIBF.open(str(out / "tgt.ibf")))) and bits.all()
    # without a bin map: the five columns alone
    run_cli("--filter-stats", out / "tgt.ibf", "--max-fp", "0.05")
    head, rows5 = read_tsv(out / "tgt.binstats.tsv")
    assert head == ["bin", "bits", "load", "fpr", "est_kmers"] and rows5 == [r[:5] for r in rows]
    # build without the flag writes no report
    config(tmp_path / "c.toml", tmp_path / "plain")
    assert "FILTER_STATS" not in run_cli("--config", tmp_path / "c.toml")
    plain = sorted(x.name for x in (tmp_path / "plain").iterdir() if x.is_file())
    assert "tgt.ibf" in plain and not [n for n in plain if n.endswith(".tsv")], plain  # (the build's own configLog.toml is there as ever)
    # one bin deliberately overfilled: ten fragments into bin 0 of a filter sized like the one above
    over = capi.DeviceIBF.create(0, dev.info["n_bins"], 3, 13, dev.info["n_bits"])
    for b in range(dev.info["n_bins"]):
        over.insert(H.random_dna(rng, 1000), [0], [1000], [b])
    for _ in range(9):
        over.insert(H.random_dna(rng, 1000), [0], [1000], [0])
    over.download().store(str(tmp_path / "over.ibf"))
    text = run_cli("--filter-stats", tmp_path / "over.ibf", "--max-fp", "0.05", expect=3)
    assert "fullest_bin=0 " in text and "bins_over_max_fp=1\n" in text
    assert int(read_tsv(tmp_path / "over.binstats.tsv")[1][0][1]) == int(over.bin_occupancy()[0])

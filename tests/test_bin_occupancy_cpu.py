"""Per-bin occupancy without a GPU: the numpy yardstick on hand-written vectors, the two host helpers of the C ABI against numpy, the
declarations, the CLI's behaviour on a box without a device, and the register budget of the kernel builds.

Integers are compared exactly.  The derived doubles are compared with numpy's `load ** h` and `-(m / h) * log1p(-load)` at a relative
tolerance of 1e-12: both sides are a handful of libm calls on identical inputs, each correct to about an ulp (2.2e-16), so 1e-12 leaves
three orders of margin and still catches a wrong formula."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

from oracle import pyoracle as po
from readbouncer_amd import capi
from tests import helpers as H
from tests.kernel_build import resources
from tests.occupancy_rules import bin_occupancy, summary

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "readbouncer_amd", "readbouncer_amd_cli")
RTOL = 1e-12


def test_occupancy_rules_on_hand_vectors():
    """3 blocks x 70 bins (W = 2), written out bit by bit; the tail bits of the last column (bins 70-127) are set and ignored"""
    n_bins, n_blocks, W = 70, 3, 2
    mat = np.zeros((n_blocks, 128), dtype=np.uint8)
    mat[0, [0, 1, 63, 64, 69]] = 1
    mat[1, [1, 63, 69]] = 1
    mat[2, [1, 2, 64, 69]] = 1
    mat[:, 70:] = 1  # not bins
    words = np.zeros(n_blocks * W + 5, dtype=np.uint64)
    for b in range(n_blocks):
        for j in range(128):
            if mat[b, j]:
                words[b * W + j // 64] |= np.uint64(1) << np.uint64(j % 64)
    words[n_blocks * W:] = np.uint64(0xFFFFFFFFFFFFFFFF)  # words behind the blocks are not bins either
    got = bin_occupancy(words, n_bins, n_blocks)
    want = np.zeros(n_bins, dtype=np.uint64)
    want[[0, 2]] = 1
    want[1] = 3
    want[63] = 2
    want[64] = 2
    want[69] = 3
    assert got.dtype == np.uint64 and np.array_equal(got, want)
    assert np.array_equal(bin_occupancy(np.array([0b101, 0b100, 0b111], dtype=np.uint64), 3, 3), np.array([2, 1, 3], dtype=np.uint64))
    s = summary(want, n_blocks, 3, 0.5)
    assert (s["bits_total"], s["empty_bins"], s["max_bits"], s["max_bin"], s["min_bits"], s["min_bin"]) == (12, 64, 3, 1, 1, 0)
    assert s["bins_over_max_fp"] == 2  # load 1 -> fpr 1; load 2/3 -> 0.296 is not over 0.5


def check_against_numpy(bits, n_blocks, h, max_fp=0.01):
    bits = np.asarray(bits, dtype=np.uint64)
    load, fpr, est = capi.bin_occupancy_derive(bits, n_blocks, h)
    want_load = bits.astype(np.float64) / float(n_blocks)
    with np.errstate(divide="ignore"):
        want_est = -(float(n_blocks) / float(h)) * np.log1p(-want_load)
    assert np.array_equal(load, want_load)
    np.testing.assert_allclose(fpr, want_load ** float(h), rtol=RTOL, atol=0)
    np.testing.assert_allclose(est, want_est, rtol=RTOL, atol=0)
    got, want = capi.bin_occupancy_summary(bits, n_blocks, h, max_fp), summary(bits, n_blocks, h, max_fp)
    for key, v in want.items():
        if isinstance(v, float):
            assert math.isclose(got[key], v, rel_tol=RTOL, abs_tol=0.0), (key, got[key], v)
        else:
            assert got[key] == v, (key, got[key], v)
    return got, (load, fpr, est)


@pytest.mark.parametrize("h", [1, 2, 3, 4, 5])
@pytest.mark.parametrize("n_bins", [1, 9000])
def test_host_helpers_against_numpy(n_bins, h):
    rng = np.random.default_rng(100 * h + n_bins)
    n_blocks = 16411
    bits = rng.integers(0, n_blocks + 1, size=n_bins).astype(np.uint64)
    bits[rng.random(n_bins) < 0.2] = 0
    check_against_numpy(bits, n_blocks, h)
    bits[:] = np.minimum(bits, np.uint64(n_blocks // 4))  # loads up to 0.25 against max_fp = 0.125^h: some bins over it, some under
    got, _ = check_against_numpy(bits, n_blocks, h, 0.125 ** h)
    assert n_bins == 1 or 0 < got["bins_over_max_fp"] < n_bins - got["empty_bins"]


def test_host_helpers_edges():
    # all empty
    got, (load, fpr, est) = check_against_numpy(np.zeros(130, dtype=np.uint64), 4096, 3)
    assert (got["empty_bins"], got["max_bits"], got["max_bin"], got["min_bits"], got["min_bin"], got["bins_over_max_fp"]) == (130, 0, 0, 0, 0, 0)
    assert got["mean_load"] == 0.0 and got["max_fpr"] == 0.0 and not load.any() and not fpr.any() and not est.any()
    # one bin full: load 1, fpr 1, est_kmers +inf
    bits = np.zeros(70, dtype=np.uint64)
    bits[33] = 4096
    got, (load, fpr, est) = check_against_numpy(bits, 4096, 3)
    assert load[33] == 1.0 and fpr[33] == 1.0 and est[33] == np.inf and got["max_bin"] == 33 and got["min_bin"] == 33 and got["max_fpr"] == 1.0
    # ties for the fullest and for the emptiest non-empty bin go to the lowest index
    bits = np.array([0, 7, 9, 3, 9, 0, 3, 5], dtype=np.uint64)
    got, _ = check_against_numpy(bits, 10, 2)
    assert (got["max_bits"], got["max_bin"], got["min_bits"], got["min_bin"], got["empty_bins"], got["bits_total"]) == (9, 2, 3, 3, 2, 36)
    # strictly greater than max_fp: load 0.5, h 3 gives fpr == 0.125 exactly
    bits = np.array([8, 8, 9, 7], dtype=np.uint64)
    got, (_, fpr, _) = check_against_numpy(bits, 16, 3, 0.125)
    assert fpr[0] == 0.125 and got["bins_over_max_fp"] == 1
    # any output of derive may be left out
    L = capi.lib()
    load = np.zeros(4)
    assert L.rb_bin_occupancy_derive(bits.ctypes.data, 4, 16, 3, load.ctypes.data, None, None) == capi.RB_OK and load[2] == 9 / 16


def test_host_helpers_refuse_degenerate_geometry():
    bits = np.ones(4, dtype=np.uint64)
    for n_blocks, h in ((0, 3), (16, 0)):
        with pytest.raises(capi.RBError) as e:
            capi.bin_occupancy_summary(bits, n_blocks, h)
        assert e.value.status == capi.RB_ERR_INVALID_ARG
        with pytest.raises(capi.RBError) as e:
            capi.bin_occupancy_derive(bits, n_blocks, h)
        assert e.value.status == capi.RB_ERR_INVALID_ARG


NEW_CALLS = ("rb_dibf_bin_occupancy", "rb_dibf_bin_occupancy_device", "rb_bin_occupancy_summarize", "rb_bin_occupancy_derive")


def test_new_calls_sit_in_the_boundary_header_with_a_reference_citation():
    main = open(os.path.join(ROOT, "include", "readbouncer_amd.h")).read()
    tuning = open(os.path.join(ROOT, "include", "readbouncer_amd_tuning.h")).read()
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read().split("### 1b.")[0]
    for name in NEW_CALLS:
        assert re.search(r"RB_API int %s\(" % name, main) and not re.search(r"RB_API[^;(]*\b%s\s*\(" % name, tuning)
        assert name in capi.SIGNATURES and name in integration
        # the comment block that ends at the declaration names where the reference holds the matter (file:line)
        head = main[:main.index("RB_API int %s(" % name)]
        comment = head[head.rindex("/*"):]
        assert re.search(r"(IBFConfig\.hpp|IBFBuild\.cpp|IBF\.hpp):\d+", comment), name
    # the section as a whole states the two reference-derived facts it uses
    sect = main[main.index("how full is each bin"):main.index("rb_bin_occupancy_derive(")]
    assert "IBFConfig.hpp:77" in sect and "IBFBuild.cpp:404-413" in sect
    assert hasattr(capi.DeviceIBF, "bin_occupancy") and hasattr(capi.DeviceIBF, "bin_occupancy_device")
    hpp = open(os.path.join(ROOT, "include", "readbouncer_amd.hpp")).read()
    assert "bin_occupancy(" in hpp and "rb_bin_occupancy_summary" in hpp


# (RB_ERR_NO_DEVICE from the two rb_dibf_* calls cannot be shown without a GPU: they take a device filter, and no such handle can be
# made without a device -- rb_dibf_create / _open refuse first, which the CLI test below sees through `--filter-stats`.)


def test_cli_names_the_flags_and_needs_a_device(tmp_path):
    p = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0
    for flag in ("--filter-stats", "--bin-map", "--max-fp", "--chunk-length", "binstats.tsv"):
        assert flag in p.stdout, flag
    if capi.device_count() > 0:
        return  # with a GPU the report itself is checked in tests/test_gpu_bin_occupancy.py
    rng = np.random.default_rng(5)
    f = po.OracleIBF(100, 3, 13, 128 * 4099)
    for b in range(0, 100, 9):
        f.insert(po.encode(H.random_dna(rng, 700)), b)
    f.store(str(tmp_path / "small.ibf"))
    p = subprocess.run([CLI, "--filter-stats", str(tmp_path / "small.ibf")], capture_output=True, text=True, timeout=120)
    assert p.returncode != 0 and p.returncode != 3
    assert re.search(r"no (HIP|gfx950) device", p.stderr), p.stderr
    assert sorted(x.name for x in tmp_path.iterdir()) == ["small.ibf"]


# ---- kernel resources at build time (the route of tests/test_kernel_resources.py) --------------------------------------------------
# ibf_bin_occupancy_kernel<words per lane, non-temporal> -> waves per SIMD.  Workgroups of 16 waves: four per SIMD, one workgroup per CU,
# which is what the launcher sizes its grid for; a build that needs more than 128 registers would not launch at all.
OCCUPANCY_EXPECT = {"<1,0>": 4, "<1,1>": 4, "<2,0>": 4, "<2,1>": 4}


def test_occupancy_kernel_builds_keep_their_waves_and_do_not_spill():
    found = {k[len("ibf_bin_occupancy_kernel"):]: v for k, v in resources("rb_kernels.hip").items() if k.startswith("ibf_bin_occupancy_kernel<")}
    assert sorted(found) == sorted(OCCUPANCY_EXPECT), sorted(found)
    for k, waves in OCCUPANCY_EXPECT.items():
        assert found[k]["occ"] >= waves and found[k]["scratch"] == 0 and found[k]["vgpr"] <= 128, (k, found[k])

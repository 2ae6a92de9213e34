"""CPU-side checks of the prefix pass (rb_prefix_batch / rb_prefix_batch_device): the calls are declared, exported, bound and
documented; malformed arguments are refused with a text that names the fault and well-formed calls fail loudly without a GPU; the CLI
names and parses its flags; the rules of tests/prefix_rules.py do what the header says on hand-written rows; the conditions the GPU
cases depend on hold on the oracle; and every build of ibf_prefix_kernel keeps the register class of the ibf_locate_kernel build of
the same template arguments."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from readbouncer_amd import capi
from tests import prefix_rules as PR
from tests.kernel_build import builds, resources
from tests.test_gpu_locate import make_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("rb_prefix_batch_device", "rb_prefix_batch")
CHECKPOINTS = (77, 140, 141, 204, 268, 360, 500, 640)


def test_calls_are_declared_exported_bound_and_documented():
    header = open(os.path.join(ROOT, "include", "readbouncer_amd.h")).read()
    tuning = open(os.path.join(ROOT, "include", "readbouncer_amd_tuning.h")).read()
    declared = set(re.findall(r"RB_API[^;(]*?\b(rb_[a-z0-9_]+)\s*\(", header))
    out = subprocess.check_output(["nm", "-D", "--defined-only", capi.LIB_PATH], text=True)
    exported = set(re.findall(r" T (rb_[a-z0-9_]+)", out))
    one = open(os.path.join(ROOT, "INTEGRATION.md")).read().split("### 1b.")[0]
    for name in CALLS:
        assert name in declared and name in exported and name in capi.SIGNATURES and name in one, name
        assert name not in tuning
        assert getattr(capi.lib(), name) is not None
    line = [l for l in one.splitlines() if "rb_prefix_batch_device" in l]
    assert len(line) == 1 and "adaptive_sampling.hpp:280-331" in line[0] and "classify.hpp:262-299" in line[0]
    assert "adaptive_sampling.hpp:280-331" in header and "classify.hpp:262-299" in header
    body = re.search(r"typedef struct rb_prefix_out \{(.*?)\} rb_prefix_out;", header, re.S).group(1)
    assert re.findall(r"void \*(\w+);", body) == [n for n, _ in capi.PrefixOut._fields_] == \
        ["max_count", "decision", "best_target", "status", "prefix_len", "first_decided"]
    assert int(re.search(r"#define RB_PREFIX_MAX (\d+)", header).group(1)) == capi.RB_PREFIX_MAX == 64
    assert hasattr(capi.Engine, "prefixes") and hasattr(capi.Engine, "prefixes_device")


def test_calls_refuse_malformed_arguments_and_fail_loudly_without_a_gpu():
    L = capi.lib()
    keep = {"mc": np.zeros(64, np.uint16), "d": np.zeros(64, np.uint8), "b": np.zeros(64, np.int32), "st": np.zeros(64, np.uint8),
            "pl": np.zeros(64, np.uint32), "fd": np.zeros(1, np.uint32), "seq": np.frombuffer(b"ACGTACGTACGTACGTACGT", dtype=np.uint8).copy(),
            "off": np.zeros(1, np.uint64), "len": np.array([20], np.uint32)}
    out = capi.PrefixOut(*[keep[k].ctypes.data for k in ("mc", "d", "b", "st", "pl", "fd")])
    none = capi.PrefixOut(None, None, None, None, None, None)
    desc = capi.BatchDesc(keep["seq"].ctypes.data, keep["off"].ctypes.data, keep["len"].ctypes.data, 1, 20, None, None, 0, 0, None)

    def cps(*v):
        keep["cps"] = np.array(v, dtype=np.uint32)
        return keep["cps"].ctypes.data, len(v)

    def host(o, lens_n, mode=capi.RB_MODE_CHECK_UNBLOCK):
        return L.rb_prefix_batch(None, keep["seq"].ctypes.data, keep["off"].ctypes.data, keep["len"].ctypes.data, 1, None, 0, lens_n[0], lens_n[1],
                                 0.1, 0.95, mode, o)

    def dev(d, o, lens_n, mode=capi.RB_MODE_CHECK_UNBLOCK):
        return L.rb_prefix_batch_device(None, d, lens_n[0], lens_n[1], 0.1, 0.95, mode, o, None)

    def refused(rc, text):
        msg = L.rb_last_error().decode()
        assert rc == capi.RB_ERR_INVALID_ARG and text in msg, (rc, text, msg)

    good = cps(5, 10)
    # null arguments
    refused(dev(None, C.byref(out), good), "null descriptor")
    refused(dev(C.byref(desc), None, good), "null output struct")
    refused(host(None, good), "null output struct")
    refused(dev(C.byref(desc), C.byref(out), (None, 2)), "null checkpoint list")
    refused(host(C.byref(out), (None, 2)), "null checkpoint list")
    # the number of checkpoints
    refused(dev(C.byref(desc), C.byref(out), (good[0], 0)), "n_prefixes")
    refused(host(C.byref(out), (good[0], 0)), "n_prefixes")
    many = cps(*range(1, 66))
    refused(dev(C.byref(desc), C.byref(out), many), "n_prefixes")
    refused(host(C.byref(out), many), "n_prefixes")
    # their values
    for bad, text in (((0, 5), "checkpoint of 0"), ((5, 0), "checkpoint of 0"), ((5, 5), "strictly rising"), ((5, 9, 7), "strictly rising")):
        v = cps(*bad)
        refused(dev(C.byref(desc), C.byref(out), v), text)
        refused(host(C.byref(out), v), text)
    good = cps(5, 10)
    # no output, an unknown mode
    refused(dev(C.byref(desc), C.byref(none), good), "no output")
    refused(host(C.byref(none), good), "no output")
    refused(dev(C.byref(desc), C.byref(out), good, 7), "unknown mode")
    refused(host(C.byref(out), good, 7), "unknown mode")
    # well-formed calls, P = 64 included: without a GPU they say so, with one the NULL engine is refused
    want = capi.RB_ERR_NO_DEVICE if capi.device_count() <= 0 else capi.RB_ERR_INVALID_ARG
    only = capi.PrefixOut(None, None, None, None, None, keep["fd"].ctypes.data)
    for v in (good, cps(*range(1, 65))):
        for mode in (capi.RB_MODE_CHECK_UNBLOCK, capi.RB_MODE_CLASSIFY_CHUNK, capi.RB_MODE_CLASSIFY_ANY):
            assert dev(C.byref(desc), C.byref(out), v, mode) == want and host(C.byref(out), v, mode) == want
        assert dev(C.byref(desc), C.byref(only), v) == want and host(C.byref(only), v) == want
    if capi.device_count() <= 0:
        assert "no gfx950" in L.rb_last_error().decode().lower() or "device" in L.rb_last_error().decode().lower()


def test_cli_names_and_parses_the_flags():
    cli = os.path.join(os.path.dirname(capi.LIB_PATH), "readbouncer_amd_cli")
    p = subprocess.run([cli, "--help"], capture_output=True, text=True, timeout=60)
    for flag in ("--report-prefixes", "--prefix-lens", "--prefix-step", "--prefix-count", "classified_prefixes.tsv", "prefix_summary.tsv"):
        assert flag in p.stdout + p.stderr, flag
    bad_lists = (["--prefix-lens"], ["--prefix-lens", "0,5"], ["--prefix-lens", "5,5"], ["--prefix-lens", "9,7"], ["--prefix-lens", "12x"],
                 ["--prefix-lens", "5,,7"], ["--prefix-lens", "5,"], ["--prefix-lens", "--report-prefixes"],
                 ["--prefix-lens", ",".join(str(i) for i in range(1, 66))])
    for bad in bad_lists:
        p = subprocess.run([cli] + bad, capture_output=True, text=True, timeout=60)
        assert p.returncode == 1 and "--prefix-lens" in p.stderr, bad
    for bad in (["--prefix-step"], ["--prefix-step", "0"], ["--prefix-step", "-3"], ["--prefix-step", "4x"], ["--prefix-count", "0"], ["--prefix-count", "65"]):
        p = subprocess.run([cli] + bad, capture_output=True, text=True, timeout=60)
        assert p.returncode == 1 and bad[0] in p.stderr, bad
    # one way of naming the checkpoints, not both -- in either order
    for both in (["--prefix-lens", "140,204", "--prefix-step", "100"], ["--prefix-step", "100", "--prefix-lens", "140,204"],
                 ["--prefix-count", "3", "--prefix-lens", "140,204"], ["--prefix-lens", "140,204", "--prefix-count", "3"]):
        p = subprocess.run([cli, "--report-prefixes"] + both + ["--help"], capture_output=True, text=True, timeout=60)
        assert p.returncode == 1 and "--prefix-lens" in p.stderr and "--prefix-step" in p.stderr, both
    # the report without checkpoints
    p = subprocess.run([cli, "--report-prefixes"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 1 and "--prefix-lens" in p.stderr and "--prefix-step" in p.stderr
    # good values are taken (and with them their arguments: --help after them is still seen)
    for good in (["--prefix-lens", "140,204,360"], ["--prefix-lens", "7"], ["--prefix-step", "360"], ["--prefix-step", "100", "--prefix-count", "64"]):
        p = subprocess.run([cli, "--report-prefixes"] + good + ["--help"], capture_output=True, text=True, timeout=60)
        assert p.returncode == 0 and "--report-prefixes" in p.stdout, good


def test_rules_on_hand_written_rows():
    ok = PR.RB_OK
    # a decision that goes 1 -> 0 -> 1: the first one counts
    assert PR.first_decided([0, 1, 0, 1], [ok] * 4) == 1
    assert PR.first_decided([2, 0, 0], [ok] * 3) == 0
    # all zero: P
    assert PR.first_decided([0, 0, 0], [ok] * 3) == 3 and PR.first_decided([], []) == 0
    # a status that is not RB_OK in the first row: that row decides nothing, whatever it holds
    assert PR.first_decided([0, 0, 1], [PR.RB_ERR_SHORT_READ, ok, ok]) == 2
    assert PR.first_decided([1, 1], [PR.RB_ERR_SHORT_READ, ok]) == 1
    assert PR.first_decided([1, 0], [PR.RB_ERR_BAD_CHUNK, PR.RB_ERR_BAD_CHUNK]) == 2
    # the status codes are the header's
    assert (PR.RB_OK, PR.RB_ERR_SHORT_READ, PR.RB_ERR_BAD_CHUNK, PR.RB_ERR_INVALID_ARG) == \
        (capi.RB_OK, capi.RB_ERR_SHORT_READ, capi.RB_ERR_BAD_CHUNK, capi.RB_ERR_INVALID_ARG)
    assert (PR.MODE_CHECK_UNBLOCK, PR.MODE_CLASSIFY_CHUNK, PR.MODE_CLASSIFY_ANY) == \
        (capi.RB_MODE_CHECK_UNBLOCK, capi.RB_MODE_CLASSIFY_CHUNK, capi.RB_MODE_CLASSIFY_ANY)


def test_rows_of_a_short_read_a_chunk_and_a_bound():
    """the rules on one filter of the GPU cases: below k, at or beyond the end, chunk_start, an understated max_len"""
    f, reads, _, _ = make_case("w5")
    k = f.kmer_size
    read = reads[0]
    assert len(read) > 120
    rows = PR.expected_rows(read, (5, k, k + 1, 10000), [f], [], PR.MODE_CHECK_UNBLOCK)
    assert rows["prefix_len"].tolist() == [5, k, k + 1, len(read)] and rows["status"].tolist() == [PR.RB_ERR_SHORT_READ, 0, 0, 0]
    assert rows["max_count"][0, 0] == 0 and rows["max_count"][1, 0] <= 1 and rows["max_count"][2, 0] <= 2
    whole = PR.expected_rows(read, (len(read), len(read) + 1), [f], [], PR.MODE_CHECK_UNBLOCK)
    assert whole["max_count"][0, 0] == whole["max_count"][1, 0] == rows["max_count"][3, 0] and whole["prefix_len"].tolist() == [len(read)] * 2
    # counted from chunk_start, clipped by the descriptor's chunk_length, refused beyond max_len
    part = PR.expected_rows(read, (40, 100), [f], [], PR.MODE_CHECK_UNBLOCK, chunk_start=50, chunk_length=60)
    same = PR.expected_rows(read[50:110], (40, 100), [f], [], PR.MODE_CHECK_UNBLOCK)
    assert part["prefix_len"].tolist() == [40, 60] and all(np.array_equal(part[key], same[key]) for key in part)
    cut = PR.expected_rows(read, (40, 100), [f], [], PR.MODE_CHECK_UNBLOCK, max_len=99)
    assert cut["status"].tolist() == [0, PR.RB_ERR_INVALID_ARG] and cut["decision"][1] == 0 and cut["first_decided"] in (0, 2)
    gone = PR.expected_rows(read[:30], (40,), [f], [], PR.MODE_CHECK_UNBLOCK, chunk_start=31)
    assert gone["status"].tolist() == [PR.RB_ERR_BAD_CHUNK] and gone["first_decided"] == 1


@pytest.mark.parametrize("name", ["w5", "w129"])
def test_case_conditions_hold_on_the_oracle(name):
    """what the GPU cases depend on, on the oracle's numbers: deplete-only check_unblock at k = 13, r = 0.1 is NOT monotone in the prefix
    length.  The threshold is 65531 (the uint16_t wrap), 2, 2, 11, 21, 38, 64, 91 at the checkpoints: nobody is decided at 77, nearly
    everybody at 140, and more than a hundred reads fall back to "wait" by 204."""
    from oracle import pyoracle as po
    f, reads, _, _ = make_case(name)
    k = f.kmer_size
    assert [po.threshold(c, k, 0.1, 0.95) for c in CHECKPOINTS] == [65531, 2, 2, 11, 21, 38, 64, 91]
    exp = PR.expected_batch(reads, CHECKPOINTS, [f], [], PR.MODE_CHECK_UNBLOCK)
    d, st = exp["decision"], exp["status"]
    decided = [int(np.count_nonzero(d[:, p])) for p in range(len(CHECKPOINTS))]
    steps_back = int(np.count_nonzero(((d[:, :-1] == 1) & (d[:, 1:] == 0)).any(axis=1)))
    differ = int(np.count_nonzero(d[:, 1:] != d[:, :-1]))
    print(name, "reads", len(reads), "decided", decided, "rows that differ from the row before", differ, "reads with a 1 -> 0 step", steps_back)
    assert decided[0] == 0
    assert decided[1] >= 250
    assert all(100 <= n <= 220 for n in decided[3:]), decided
    assert steps_back >= 100
    lens = np.array([len(r) for r in reads])
    assert (lens < CHECKPOINTS[-1]).any() and (lens < k).any()
    assert (st[lens < k] == PR.RB_ERR_SHORT_READ).all() and (st[lens >= CHECKPOINTS[-1]][:, 1:] == PR.RB_OK).all()
    assert (exp["first_decided"] == 1).sum() == decided[1] and (exp["first_decided"] == 0).sum() == 0


def test_prefix_builds_keep_the_locate_builds_register_class():
    """compiled like tests/test_hits_cpu.py does: every ibf_prefix_kernel build has no scratch, and its waves per SIMD are no lower than
    those of the ibf_locate_kernel build of the same template arguments, read from the same compile"""
    found = resources("rb_kernels.hip")
    prefix, locate = builds(found, "ibf_prefix_kernel"), builds(found, "ibf_locate_kernel")
    # the (LG, WPL) x {10 planes, 16 planes, 16 planes with run-time hashes} cases, non-temporal twins where locate has them
    assert set(prefix) == set(locate) and len(prefix) == 8 * 3 + 2 * 3, (sorted(prefix), sorted(locate))
    for a, v in sorted(prefix.items()):
        print(a, "prefix", v, "locate", locate[a])
        assert v["scratch"] == 0, (a, v)
        assert v["occ"] >= 3 and v["occ"] >= locate[a]["occ"], (a, v, locate[a])

"""CPU-side checks of the hits pass (rb_hits_batch / rb_hits_batch_device): the calls are declared, exported, bound and documented;
rb_hit is the 8 bytes the header says; without a GPU the calls fail loudly and with malformed arguments they refuse; the CLI names
and parses its flags; the numpy restatement of the rules does what the header says on hand-written vectors; and every build of
ibf_hits_kernel keeps the register class of the ibf_locate_kernel build it was made from."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from readbouncer_amd import capi
from tests.kernel_build import builds, resources
from tests.hits_rules import HIT, distinct_bins, reduce_hits
from tests.locate_rules import reduce_locate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("rb_hits_batch_device", "rb_hits_batch")


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
    assert "IBFClassify.cpp:16-38" in header and "97-98" in header and "149-150" in header
    body = re.search(r"typedef struct rb_hits_out \{(.*?)\} rb_hits_out;", header, re.S).group(1)
    assert re.findall(r"void \*(\w+);", body) == [n for n, _ in capi.HitsOut._fields_] == ["hits", "n_hits", "status", "bin_reads"]


def test_rb_hit_is_eight_bytes_with_the_documented_offsets(tmp_path):
    assert C.sizeof(capi.Hit) == 8
    assert [(n, getattr(capi.Hit, n).offset, getattr(capi.Hit, n).size) for n, _ in capi.Hit._fields_] == \
        [("bin", 0, 4), ("count", 4, 2), ("strand", 6, 1), ("reserved", 7, 1)]
    assert capi.HIT_DTYPE == HIT and HIT.itemsize == 8 and [HIT.fields[n][1] for n in HIT.names] == [0, 4, 6, 7]
    # ... and the C compiler agrees, in C99
    src = tmp_path / "hit.c"
    src.write_text(r'''
#include <stddef.h>
#include "readbouncer_amd.h"
int main(void)
{
    rb_hits_out out;
    rb_batch_desc desc;
    uint32_t n[1];
    out.hits = 0; out.n_hits = n; out.status = 0; out.bin_reads = 0;
    desc.d_seqs = 0; desc.d_offsets = 0; desc.d_lens = 0; desc.n_items = 0; desc.max_len = 0; desc.d_nmask = 0;
    desc.d_nmask_offsets = 0; desc.chunk_start = 0; desc.chunk_length = 0; desc.d_read_ids = 0;
    if (sizeof(rb_hit) != 8 || offsetof(rb_hit, bin) != 0 || offsetof(rb_hit, count) != 4 || offsetof(rb_hit, strand) != 6 ||
        offsetof(rb_hit, reserved) != 7) return 2;
    /* NULL engine: refused, whatever the machine */
    return rb_hits_batch_device(0, &desc, 0.1, 0.95, 0, 0, &out, 0) == RB_OK || rb_hits_batch(0, "", 0, 0, 0, 0, 0, 0.1, 0.95, 0, 0, &out) == RB_OK;
}
''')
    exe = tmp_path / "hit"
    lib_dir = os.path.dirname(capi.LIB_PATH)
    subprocess.check_call(["cc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src),
                           "-o", str(exe), "-L", lib_dir, "-lreadbouncer_amd", "-Wl,-rpath," + lib_dir])
    assert subprocess.run([str(exe)], timeout=120).returncode == 0


def test_calls_refuse_malformed_arguments_and_fail_loudly_without_a_gpu():
    L = capi.lib()
    keep = {"h": np.zeros(4, HIT), "n": np.zeros(1, np.uint32), "st": np.zeros(1, np.uint8), "br": np.zeros(64, np.uint64),
            "seq": np.frombuffer(b"ACGTACGTACGTACGTACGT", dtype=np.uint8).copy(), "off": np.zeros(1, np.uint64), "len": np.array([20], np.uint32)}
    out = capi.HitsOut(keep["h"].ctypes.data, keep["n"].ctypes.data, keep["st"].ctypes.data, keep["br"].ctypes.data)
    desc = capi.BatchDesc(keep["seq"].ctypes.data, keep["off"].ctypes.data, keep["len"].ctypes.data, 1, 20, None, None, 0, 0, None)
    host = lambda e, o, cap=4: L.rb_hits_batch(e, keep["seq"].ctypes.data, keep["off"].ctypes.data, keep["len"].ctypes.data, 1, None, 0, 0.1, 0.95, 0, cap, o)
    dev = lambda e, d, o, cap=4: L.rb_hits_batch_device(e, d, 0.1, 0.95, 0, cap, o, None)
    only_status = capi.HitsOut(None, None, keep["st"].ctypes.data, None)
    assert dev(None, None, C.byref(out)) == capi.RB_ERR_INVALID_ARG
    assert dev(None, C.byref(desc), None) == capi.RB_ERR_INVALID_ARG
    assert dev(None, C.byref(desc), C.byref(only_status)) == capi.RB_ERR_INVALID_ARG
    assert host(None, None) == capi.RB_ERR_INVALID_ARG
    assert host(None, C.byref(only_status)) == capi.RB_ERR_INVALID_ARG
    # a record buffer with room for no record
    assert dev(None, C.byref(desc), C.byref(out), 0) == capi.RB_ERR_INVALID_ARG
    assert host(None, C.byref(out), 0) == capi.RB_ERR_INVALID_ARG
    # well-formed calls (max_hits == 0 with n_hits alone is one): without a GPU they say so, with one the NULL engine is refused
    want = capi.RB_ERR_NO_DEVICE if capi.device_count() <= 0 else capi.RB_ERR_INVALID_ARG
    counts = capi.HitsOut(None, keep["n"].ctypes.data, None, None)
    assert dev(None, C.byref(desc), C.byref(out)) == want and host(None, C.byref(out)) == want
    assert dev(None, C.byref(desc), C.byref(counts), 0) == want and host(None, C.byref(counts), 0) == want


def test_cli_names_and_parses_the_flags():
    cli = os.path.join(os.path.dirname(capi.LIB_PATH), "readbouncer_amd_cli")
    p = subprocess.run([cli, "--help"], capture_output=True, text=True, timeout=60)
    for flag in ("--report-hits", "--max-hits", "classified_hits.tsv", "bin_profile.tsv"):
        assert flag in p.stdout + p.stderr, flag
    for bad in (["--max-hits"], ["--max-hits", "0"], ["--max-hits", "-3"], ["--max-hits", "12x"], ["--max-hits", "--report-hits"]):
        p = subprocess.run([cli] + bad, capture_output=True, text=True, timeout=60)
        assert p.returncode == 1 and "--max-hits" in p.stderr, bad
    # a good value is taken (and with it its argument: --help after it is still seen)
    p = subprocess.run([cli, "--report-hits", "--max-hits", "7", "--help"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0 and "--report-hits" in p.stdout


def u16(*v):
    return np.array(v, dtype=np.uint16)


def test_rules_on_hand_written_vectors():
    # one hit per strand, rising bins; the strand of an equal bin: forward first
    assert reduce_hits(u16(0, 5, 2), u16(1, 1, 7), 3) == [(1, 0, 5), (2, 1, 7)]
    assert reduce_hits(u16(0, 0, 6), u16(0, 0, 6), 1) == [(2, 0, 6), (2, 1, 6)]
    # ties are all listed; a bin on both strands is two records and one distinct bin
    rec = reduce_hits(u16(4, 4, 0, 9), u16(4, 0, 0, 3), 4)
    assert rec == [(0, 0, 4), (0, 1, 4), (1, 0, 4), (3, 0, 9)] and distinct_bins(rec) == 3
    assert distinct_bins(rec) == reduce_locate(u16(4, 4, 0, 9), u16(4, 0, 0, 3), 4)[3]
    # t == 0: every bin on both strands, zero counts included
    assert reduce_hits(u16(0, 3), u16(0, 0), 0) == [(0, 0, 0), (0, 1, 0), (1, 0, 3), (1, 1, 0)]
    # a wrapped t lists nothing ... unless a wrapped COUNT is up there as well (uint16_t compare)
    assert reduce_hits(u16(0, 3, 900), u16(1000, 0, 0), 65531) == []
    assert reduce_hits(u16(65535, 3), u16(0, 0), 65531) == [(0, 0, 65535)]
    # min_count = 1: the nonzero entries of both vectors, i.e. seqan::count in sparse form
    assert reduce_hits(u16(0, 2, 0, 1), u16(5, 0, 0, 1), 1) == [(0, 1, 5), (1, 0, 2), (3, 0, 1), (3, 1, 1)]
    # truncation keeps the first records of that order
    assert reduce_hits(u16(1, 1, 1), u16(1, 1, 1), 1)[:3] == [(0, 0, 1), (0, 1, 1), (1, 0, 1)]
    # no bins at all, a single bin
    assert reduce_hits(u16(), u16(), 0) == [] and reduce_hits(u16(2), u16(3), 3) == [(0, 1, 3)]


def test_rules_against_a_plain_loop_and_the_locate_rules():
    rng = np.random.default_rng(5)
    for _ in range(300):
        nb = int(rng.integers(1, 200))
        hi = int(rng.choice([1, 2, 4, 50]))
        fwd = rng.integers(0, hi + 1, size=nb).astype(np.uint16)
        rev = rng.integers(0, hi + 1, size=nb).astype(np.uint16)
        t = int(rng.choice([0, 1, 2, hi, hi + 1, 65530]))
        want = [(b, s, int(v[b])) for b in range(nb) for s, v in ((0, fwd), (1, rev)) if int(v[b]) >= t]
        got = reduce_hits(fwd, rev, t)
        assert got == want and got == sorted(got)
        m, _, _, hit_bins = reduce_locate(fwd, rev, t)
        assert distinct_bins(got) == hit_bins
        if m >= t:
            assert max(c for _, _, c in got) == m


def test_hits_builds_keep_the_locate_builds_register_class():
    """compiled like test_kernel_resources.py does: every ibf_hits_kernel build has no scratch, and its waves per SIMD are no lower than
    those of the ibf_locate_kernel build of the same template arguments, read from the same compile"""
    found = resources("rb_kernels.hip")
    hits, locate = builds(found, "ibf_hits_kernel"), builds(found, "ibf_locate_kernel")
    # the (LG, WPL) x {10 planes, 16 planes, 16 planes with run-time hashes} cases, non-temporal twins where locate has them
    assert set(hits) == set(locate) and len(hits) == 8 * 3 + 2 * 3, (sorted(hits), sorted(locate))
    for a, v in sorted(hits.items()):
        print(a, "hits", v, "locate", locate[a])
        assert v["scratch"] == 0, (a, v)
        assert v["occ"] >= locate[a]["occ"], (a, v, locate[a])

"""CPU-side checks of the locate pass (rb_locate_batch / rb_locate_batch_device): the two calls are declared, exported, bound and
documented; the boundary header is still C99; without a GPU they fail loudly and with NULL arguments they refuse; the CLI names
its flags; and the numpy restatement of the rules that the GPU tests reduce the oracle's count vectors with does what the header
says on hand-written vectors (every tie case, M == 0, t == 0, a wrapped t)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from readbouncer_amd import capi
from tests.locate_rules import places_at_max, reduce_locate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("rb_locate_batch_device", "rb_locate_batch")


def test_calls_are_declared_exported_bound_and_documented():
    header = open(os.path.join(ROOT, "include", "readbouncer_amd.h")).read()
    declared = set(re.findall(r"RB_API[^;(]*?\b(rb_[a-z0-9_]+)\s*\(", header))
    out = subprocess.check_output(["nm", "-D", "--defined-only", capi.LIB_PATH], text=True)
    exported = set(re.findall(r" T (rb_[a-z0-9_]+)", out))
    one = open(os.path.join(ROOT, "INTEGRATION.md")).read().split("### 1b.")[0]
    for name in CALLS:
        assert name in declared and name in exported and name in capi.SIGNATURES and name in one, name
        assert getattr(capi.lib(), name) is not None
    # the header says what the calls extend and that the reference has no such call
    assert "IBFClassify.cpp:149-150" in header and ":48-71" in header and ":16-38" in header
    assert "The reference has no such call" in header
    assert ctypes_layout_matches_header(header)


def ctypes_layout_matches_header(header):
    body = re.search(r"typedef struct rb_locate_out \{(.*?)\} rb_locate_out;", header, re.S).group(1)
    members = re.findall(r"void \*(\w+);", body)
    return members == [n for n, _ in capi.LocateOut._fields_] == ["max_count", "best_bin", "best_strand", "hit_bins", "status"]


def test_header_is_c99_with_a_filled_locate_out(tmp_path):
    src = tmp_path / "loc.c"
    src.write_text(r'''
#include "readbouncer_amd.h"
int main(void)
{
    uint16_t m[2]; int32_t b[2]; uint8_t s[2]; uint32_t h[2]; uint8_t st[1];
    rb_locate_out out;
    rb_batch_desc desc;
    out.max_count = m; out.best_bin = b; out.best_strand = s; out.hit_bins = h; out.status = st;
    desc.d_seqs = 0; desc.d_offsets = 0; desc.d_lens = 0; desc.n_items = 0; desc.max_len = 0; desc.d_nmask = 0;
    desc.d_nmask_offsets = 0; desc.chunk_start = 0; desc.chunk_length = 0; desc.d_read_ids = 0;
    /* NULL engine: refused, whatever the machine */
    return rb_locate_batch_device(0, &desc, 0.1, 0.95, &out, 0) == RB_OK || rb_locate_batch(0, "", 0, 0, 0, 0, 0, 0.1, 0.95, &out) == RB_OK;
}
''')
    exe = tmp_path / "loc"
    lib_dir = os.path.dirname(capi.LIB_PATH)
    subprocess.check_call(["cc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src),
                           "-o", str(exe), "-L", lib_dir, "-lreadbouncer_amd", "-Wl,-rpath," + lib_dir])
    assert subprocess.run([str(exe)], timeout=120).returncode == 0


def _well_formed():
    keep = {"m": np.zeros(1, np.uint16), "b": np.zeros(1, np.int32), "s": np.zeros(1, np.uint8), "h": np.zeros(1, np.uint32),
            "st": np.zeros(1, np.uint8), "seq": np.frombuffer(b"ACGTACGTACGTACGTACGT", dtype=np.uint8).copy(),
            "off": np.zeros(1, np.uint64), "len": np.array([20], np.uint32)}
    out = capi.LocateOut(keep["m"].ctypes.data, keep["b"].ctypes.data, keep["s"].ctypes.data, keep["h"].ctypes.data, keep["st"].ctypes.data)
    # (host addresses in a descriptor: never dereferenced, the calls below are refused before any GPU work)
    desc = capi.BatchDesc(keep["seq"].ctypes.data, keep["off"].ctypes.data, keep["len"].ctypes.data, 1, 20, None, None, 0, 0, None)
    return keep, out, desc


def test_calls_refuse_null_arguments_and_fail_loudly_without_a_gpu():
    L = capi.lib()
    keep, out, desc = _well_formed()
    host = lambda e, o: L.rb_locate_batch(e, keep["seq"].ctypes.data, keep["off"].ctypes.data, keep["len"].ctypes.data, 1, None, 0, 0.1, 0.95, o)
    dev = lambda e, d, o: L.rb_locate_batch_device(e, d, 0.1, 0.95, o, None)
    empty = capi.LocateOut(None, None, None, None, None)
    # argument shape is checked before anything else: NULL descriptor, NULL output struct, an output struct with no output
    assert dev(None, None, C.byref(out)) == capi.RB_ERR_INVALID_ARG
    assert dev(None, C.byref(desc), None) == capi.RB_ERR_INVALID_ARG
    assert dev(None, C.byref(desc), C.byref(empty)) == capi.RB_ERR_INVALID_ARG
    assert host(None, None) == capi.RB_ERR_INVALID_ARG
    assert host(None, C.byref(empty)) == capi.RB_ERR_INVALID_ARG
    # a well-formed call: without a GPU it says so (no CPU fallback), with one the NULL engine is refused
    want = capi.RB_ERR_NO_DEVICE if capi.device_count() <= 0 else capi.RB_ERR_INVALID_ARG
    assert dev(None, C.byref(desc), C.byref(out)) == want
    assert host(None, C.byref(out)) == want
    assert "engine" in L.rb_last_error().decode() or want == capi.RB_ERR_NO_DEVICE


def test_cli_help_names_the_flags():
    cli = os.path.join(os.path.dirname(capi.LIB_PATH), "readbouncer_amd_cli")
    p = subprocess.run([cli, "--help"], capture_output=True, text=True, timeout=60)
    text = p.stdout + p.stderr
    for flag in ("--report-bins", "--write-bin-map", "--bin-map"):
        assert flag in text, flag


def u16(*v):
    return np.array(v, dtype=np.uint16)


def test_rules_on_hand_written_vectors():
    # one bin at the maximum, forward / reverse
    assert reduce_locate(u16(0, 5, 2), u16(1, 1, 1), 3) == (5, 1, 0, 1)
    assert reduce_locate(u16(0, 1, 2), u16(1, 7, 1), 3) == (7, 1, 1, 1)
    # the same maximum in several bins of one strand: the lowest bin
    assert reduce_locate(u16(0, 9, 0, 9, 9), u16(0, 0, 0, 0, 0), 9) == (9, 1, 0, 3)
    # forward and reverse tie in ONE bin: strand 0
    assert reduce_locate(u16(0, 0, 6), u16(0, 0, 6), 1) == (6, 2, 0, 1)
    # reverse reaches the maximum in a LOWER bin than forward: that bin, strand 1
    assert reduce_locate(u16(0, 0, 0, 6), u16(0, 6, 0, 0), 6) == (6, 1, 1, 2)
    # forward lower than reverse: forward's bin
    assert reduce_locate(u16(6, 0, 0, 0), u16(0, 6, 0, 6), 6) == (6, 0, 0, 3)
    # the tie in a bin where forward is NOT at the maximum but the bin is the lowest: strand 1 there, even though forward ties later
    assert reduce_locate(u16(2, 0, 8), u16(8, 0, 0), 8) == (8, 0, 1, 2)
    # a bin that hits on both strands counts once
    assert reduce_locate(u16(4, 4), u16(4, 0), 4)[3] == 2
    # M == 0: no bin, strand 0; t == 0 counts every bin, any other t none
    assert reduce_locate(u16(0, 0, 0), u16(0, 0, 0), 0) == (0, -1, 0, 3)
    assert reduce_locate(u16(0, 0, 0), u16(0, 0, 0), 1) == (0, -1, 0, 0)
    # t == 0 with counts: still every bin
    assert reduce_locate(u16(0, 3, 0), u16(0, 0, 0), 0) == (3, 1, 0, 3)
    # a wrapped threshold (a negative int16 arrives as 65 5xx): no bin hits, the maximum and its bin are reported all the same
    assert reduce_locate(u16(0, 3, 900), u16(1000, 0, 0), 65531) == (1000, 0, 1, 0)
    # ... unless a wrapped COUNT is up there as well (uint16_t compare, as the reference's)
    assert reduce_locate(u16(65535, 3), u16(0, 0), 65531) == (65535, 0, 0, 1)
    # last bin, and a single-bin filter
    assert reduce_locate(u16(0, 0, 0, 1), u16(0, 0, 0, 0), 1) == (1, 3, 0, 1)
    assert reduce_locate(u16(2), u16(3), 3) == (3, 0, 1, 1)
    # places at the maximum (the condition of the planted-tie cases)
    assert places_at_max(u16(0, 6, 6), u16(6, 0, 0)) == 3 and places_at_max(u16(0, 0), u16(0, 0)) == 0
    assert places_at_max(u16(1, 2), u16(0, 1)) == 1


def test_rules_against_a_plain_loop():
    """the vectorised reduction against the header's wording spelled out bin by bin, on random vectors with many ties"""
    rng = np.random.default_rng(3)
    for _ in range(400):
        nb = int(rng.integers(1, 200))
        hi = int(rng.choice([1, 2, 4, 50]))
        fwd = rng.integers(0, hi + 1, size=nb).astype(np.uint16)
        rev = rng.integers(0, hi + 1, size=nb).astype(np.uint16)
        t = int(rng.choice([0, 1, 2, hi, hi + 1, 65530]))
        m = max(int(fwd.max()), int(rev.max()))
        best, strand = -1, 0
        if m > 0:
            for b in range(nb):
                if max(int(fwd[b]), int(rev[b])) == m:
                    best, strand = b, (0 if int(fwd[b]) == m else 1)
                    break
        hits = sum(1 for b in range(nb) if int(fwd[b]) >= t or int(rev[b]) >= t)
        assert reduce_locate(fwd, rev, t) == (m, best, strand, hits)

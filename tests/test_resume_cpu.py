"""CPU-side checks of the resume pass (rb_resume_create / _destroy / _bytes / _batch_device / _batch / _counts): the calls are declared,
exported, bound and documented; rb_resume_out matches the header; malformed arguments are refused with a text that names the fault and
well-formed calls fail loudly without a GPU; the stitching identity the pass rests on holds on the oracle; the rules of
tests/resume_rules.py do what the header says; and every build of ibf_resume_kernel keeps the register class of the sixteen-plane
ibf_locate_kernel build of the same template arguments."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from oracle import pyoracle as po
from readbouncer_amd import capi
from tests import helpers as H
from tests.kernel_build import builds, resources
from tests import resume_rules as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("rb_resume_create", "rb_resume_destroy", "rb_resume_bytes", "rb_resume_batch_device", "rb_resume_batch", "rb_resume_counts")
MEMBERS = ["max_count", "decision", "best_target", "status", "total_len"]
PR_MODE = capi.RB_MODE_CHECK_UNBLOCK


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
    line = [l for l in one.splitlines() if "rb_resume_batch_device" in l]
    assert len(line) == 1 and "adaptive_sampling.hpp:280-331" in line[0]
    body = re.search(r"typedef struct rb_resume_out \{(.*?)\} rb_resume_out;", header, re.S).group(1)
    assert re.findall(r"void \*(\w+);", body) == [n for n, _ in capi.ResumeOut._fields_] == MEMBERS
    assert int(re.search(r"#define RB_RESUME_FIRST (\d+)u", header).group(1)) == capi.RB_RESUME_FIRST == RR.FIRST == 1
    assert int(re.search(r"#define RB_RESUME_PEEK +(\d+)u", header).group(1)) == capi.RB_RESUME_PEEK == RR.PEEK == 2
    assert hasattr(capi.Engine, "resume")
    for attr in ("feed", "feed_device", "counts", "bytes", "destroy"):
        assert hasattr(capi.Resume, attr), attr
    mirror = open(os.path.join(ROOT, "include", "readbouncer_amd.hpp")).read()
    for name in CALLS:
        assert name in mirror, name


def test_struct_layout_matches_the_header(tmp_path):
    """sizes and offsets of rb_resume_out as a C compiler lays the header's struct out, against the ctypes mirror"""
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "readbouncer_amd.h"\nint main(void) {\n'
                   '    printf("%zu", sizeof(rb_resume_out));\n' +
                   "".join('    printf(" %%zu", offsetof(rb_resume_out, %s));\n' % m for m in MEMBERS) +
                   '    printf(" %u %u\\n", RB_RESUME_FIRST, RB_RESUME_PEEK);\n    return 0;\n}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["cc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    want = [C.sizeof(capi.ResumeOut)] + [getattr(capi.ResumeOut, m).offset for m in MEMBERS] + [capi.RB_RESUME_FIRST, capi.RB_RESUME_PEEK]
    assert got == want, (got, want)


def test_calls_refuse_malformed_arguments_and_fail_loudly_without_a_gpu():
    L = capi.lib()
    keep = {"mc": np.zeros(8, np.uint16), "d": np.zeros(8, np.uint8), "b": np.zeros(8, np.int32), "st": np.zeros(8, np.uint8),
            "tl": np.zeros(8, np.uint32), "seq": np.frombuffer(b"ACGTACGTACGTACGTACGT", dtype=np.uint8).copy(),
            "off": np.zeros(1, np.uint64), "len": np.array([20], np.uint32), "slot": np.zeros(1, np.uint32), "cnt": np.zeros(256, np.uint16)}
    out = capi.ResumeOut(*[keep[k].ctypes.data for k in ("mc", "d", "b", "st", "tl")])
    none = capi.ResumeOut(None, None, None, None, None)
    desc = capi.BatchDesc(keep["seq"].ctypes.data, keep["off"].ctypes.data, keep["len"].ctypes.data, 1, 20, None, None, 0, 0, None)
    slot = keep["slot"].ctypes.data

    def host(o, mode=capi.RB_MODE_CHECK_UNBLOCK):
        return L.rb_resume_batch(None, keep["seq"].ctypes.data, keep["off"].ctypes.data, keep["len"].ctypes.data, 1, slot, None, 0.1, 0.95, mode, o)

    def dev(d, o, mode=capi.RB_MODE_CHECK_UNBLOCK):
        return L.rb_resume_batch_device(None, d, slot, None, 0.1, 0.95, mode, o, None)

    def refused(rc, text):
        msg = L.rb_last_error().decode()
        assert rc == capi.RB_ERR_INVALID_ARG and text in msg, (rc, text, msg)

    # null arguments, no output, an unknown mode
    refused(dev(None, C.byref(out)), "null descriptor")
    refused(dev(C.byref(desc), None), "null output struct")
    refused(host(None), "null output struct")
    refused(dev(C.byref(desc), C.byref(none)), "no output")
    refused(host(C.byref(none)), "no output")
    refused(dev(C.byref(desc), C.byref(out), 7), "unknown mode")
    refused(host(C.byref(out), 7), "unknown mode")
    # the sizes of a set
    h = C.c_void_p()
    refused(L.rb_resume_create(None, 4, 360, 1500, None), "null out")
    refused(L.rb_resume_create(None, 0, 360, 1500, C.byref(h)), "at least one slot")
    refused(L.rb_resume_create(None, 4, 0, 1500, C.byref(h)), "max_chunk_len")
    refused(L.rb_resume_create(None, 4, 1501, 1500, C.byref(h)), "max_chunk_len")
    assert not h.value
    # NULL handles do nothing and hold nothing
    L.rb_resume_destroy(None)
    assert L.rb_resume_bytes(None) == 0
    # well-formed calls: without a GPU they say so, with one the NULL engine / NULL handle is refused
    want = capi.RB_ERR_NO_DEVICE if capi.device_count() <= 0 else capi.RB_ERR_INVALID_ARG
    only = capi.ResumeOut(None, None, None, None, keep["tl"].ctypes.data)
    for mode in (capi.RB_MODE_CHECK_UNBLOCK, capi.RB_MODE_CLASSIFY_CHUNK, capi.RB_MODE_CLASSIFY_ANY):
        assert dev(C.byref(desc), C.byref(out), mode) == want and host(C.byref(out), mode) == want
    assert dev(C.byref(desc), C.byref(only)) == want and host(C.byref(only)) == want
    assert L.rb_resume_create(None, 4, 360, 1500, C.byref(h)) == want and not h.value
    assert L.rb_resume_create(None, 4, 1500, 1500, C.byref(h)) == want and not h.value
    total = C.c_uint32(0)
    assert L.rb_resume_counts(None, 0, 0, keep["cnt"].ctypes.data, C.addressof(total)) == want
    if capi.device_count() <= 0:
        assert "device" in L.rb_last_error().decode().lower()


def schedule(k):
    return (k - 1, 1, 1, 0, 5, 360, 3, k - 2, 512, 700)


@pytest.mark.parametrize("geometry", [(100, 3, 13), (300, 2, 13), (56, 3, 31)])
@pytest.mark.parametrize("n_rule", [3, 4])
def test_stitching_identity_on_the_oracle(geometry, n_rule):
    """the counters of a grown prefix are the counters of the shorter one plus count() of "the last k - 1 bases seen + the new chunk",
    on both strands and for every bin, after every chunk with at least k bases seen"""
    n_bins, h, k = geometry
    rng = np.random.default_rng(n_bins + h + k)
    read = H.random_dna(rng, 3000, with_n=0.02)
    assert 30 <= read.count("N") <= 100
    W = (n_bins + 63) // 64
    f = po.OracleIBF(n_bins, h, k, 64 * W * 4099)
    assert f.n_blocks == 4099
    # bins that hold stretches of the read on either strand, on top of a random background: counts that differ from bin to bin
    w = f.words()[:4099 * W].reshape(4099, W)
    w |= (rng.integers(0, 1 << 63, size=w.shape, dtype=np.uint64) & rng.integers(0, 1 << 63, size=w.shape, dtype=np.uint64))
    if n_bins % 64:
        w[:, W - 1] &= np.uint64((1 << (n_bins % 64)) - 1)
    for b, (lo, hi) in enumerate(((0, 900), (700, 2100), (1500, 3000))):
        f.insert(po.encode(read[lo:hi]), 3 + 7 * b)
    f.insert(po.revcomp(po.encode(read[200:2500])), n_bins - 1)
    prev = po.set_revcomp_of_n(n_rule)
    try:
        seen = ""
        fwd, rev = np.zeros(n_bins, np.uint16), np.zeros(n_bins, np.uint16)
        checked = 0
        for c in schedule(k):
            chunk = read[len(seen):len(seen) + c]
            assert len(chunk) == c
            st = RR.stitched(seen, chunk, k)
            if len(st) >= k:
                o = po.encode(st)
                fwd = fwd + f.count(o)
                rev = rev + f.count(po.revcomp(o))
            seen += chunk
            exp = RR.expected_counts(seen, f)
            assert np.array_equal(fwd, exp[0]) and np.array_equal(rev, exp[1]), (geometry, n_rule, len(seen))
            if len(seen) >= k:
                checked += 1
                whole = po.encode(seen)
                assert np.array_equal(exp[0], f.count(whole)) and np.array_equal(exp[1], f.count(po.revcomp(whole)))
        assert checked == len(schedule(k)) - 1 and int(fwd.max()) > 500 and len(set(fwd.tolist())) > 5 and not np.array_equal(fwd, rev)
    finally:
        po.set_revcomp_of_n(prev)


def test_rules_model_commits_what_the_header_says():
    f = po.OracleIBF(70, 3, 13, 128 * 1009)
    rng = np.random.default_rng(3)
    read = H.random_dna(rng, 400)
    f.insert(po.encode(read), 7)
    m = RR.Model(4, 100, 250)
    a = m.feed([(0, read[:12], RR.FIRST), (1, read[:100], RR.FIRST), (4, read[:5], 0), (2, read[:101], 0)], [f], [], PR_MODE)
    assert a["status"].tolist() == [RR.RB_ERR_SHORT_READ, RR.RB_OK, RR.RB_ERR_INVALID_ARG, RR.RB_ERR_INVALID_ARG]
    assert a["total_len"].tolist() == [12, 100, 0, 0] and int(a["max_count"][1, 0]) == 88 and m.total(0) == 12 and m.total(2) == 0
    # PEEK answers and leaves the slot; the same chunk without it gives the same row and commits
    p = m.feed([(0, read[12:60], RR.PEEK)], [f], [], PR_MODE)
    assert m.total(0) == 12 and int(p["total_len"][0]) == 60 and int(p["max_count"][0, 0]) == 48
    q = m.feed([(0, read[12:60], 0)], [f], [], PR_MODE)
    assert all(np.array_equal(p[key], q[key]) for key in RR.KEYS) and m.total(0) == 60
    assert np.array_equal(m.counts(0, f), RR.expected_counts(read[:60], f)) and int(m.counts(0, f)[0, 7]) == 48
    # a total beyond max_total_len, a bad chunk: refused, the slot as it was; FIRST drops what the slot held
    r = m.feed([(1, read[100:200], 0), (0, "", 0)], [f], [], PR_MODE, bad_chunk=(1,))
    assert r["status"].tolist() == [RR.RB_OK, RR.RB_ERR_BAD_CHUNK] and m.total(1) == 200 and m.total(0) == 60
    r = m.feed([(1, read[200:260], 0)], [f], [], PR_MODE)
    assert r["status"].tolist() == [RR.RB_ERR_INVALID_ARG] and r["decision"].tolist() == [0] and r["best_target"].tolist() == [-1] and m.total(1) == 200
    r = m.feed([(1, read[300:320], RR.FIRST)], [f], [], PR_MODE)
    assert r["total_len"].tolist() == [20] and m.total(1) == 20 and int(r["max_count"][0, 0]) == 8
    # an empty chunk repeats the row
    again = m.feed([(1, "", 0)], [f], [], PR_MODE)
    assert all(np.array_equal(r[key], again[key]) for key in RR.KEYS)
    assert (RR.RB_OK, RR.RB_ERR_SHORT_READ, RR.RB_ERR_BAD_CHUNK, RR.RB_ERR_INVALID_ARG) == \
        (capi.RB_OK, capi.RB_ERR_SHORT_READ, capi.RB_ERR_BAD_CHUNK, capi.RB_ERR_INVALID_ARG)



def test_resume_builds_keep_the_locate_builds_register_class():
    """compiled like tests/test_hits_cpu.py does, once: every ibf_resume_kernel build has no scratch, its waves per SIMD are no lower
    than those of the ibf_locate_kernel build of the same template arguments, and the set of builds is locate's sixteen-plane set"""
    found = resources("rb_kernels.hip")
    resume = builds(found, "ibf_resume_kernel")
    locate = {a: v for a, v in builds(found, "ibf_locate_kernel").items() if a[2] == 16}
    # the (LG, WPL) x {h = 3, run-time hashes} cases on sixteen planes, non-temporal twins where locate has them
    assert set(resume) == set(locate) and len(resume) == 8 * 2 + 2 * 2, (sorted(resume), sorted(locate))
    assert all(a[2] == 16 for a in resume)
    for a, v in sorted(resume.items()):
        print(a, "resume", v, "locate", locate[a])
        assert v["scratch"] == 0, (a, v)
        assert v["occ"] >= locate[a]["occ"], (a, v, locate[a])

"""What tests/test_gpu_pass_lists.py relies on, checked without a GPU: the fixtures of tests/pass_lists_rig.py are what they claim (on the
oracle alone), the LDS arithmetic of rb_lists.h leaves the list forms of locate and hits the count kernel's nine workgroups per CU, the
new symbol and constants exist where they belong, and the six builds of each new kernel exist, use no scratch memory and declare no
static LDS (read from the code object's metadata)."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from oracle import pyoracle as po
from readbouncer_amd import capi
from tests import kernel_build as KB
from tests import list_scan_rig as SR
from tests import pass_lists_rig as PL
from tests import test_capi_cpu as CC
from tests.locate_rules import reduce_locate
from tests.hits_rules import reduce_hits

ROOT = KB.ROOT
K = PL.K


# ---------------------------------------------------------------- the fixtures
@pytest.mark.parametrize("n_bins,lines", PL.TIE_GEOMETRIES)
def test_ties_are_ties(n_bins, lines):
    words = np.zeros(SR.n_bits(n_bins) // 64 + 8, dtype=np.uint64)  # (the payload's closing words)
    f = PL.Ties(n_bins, lines, words)
    n = PL.N_KMERS
    pairs = PL.seam_pairs(n_bins)
    assert [a // 8 != b // 8 for a, b in pairs[:2]] == [True, True] and pairs[1][0] // 512 != pairs[1][1] // 512 and pairs[2] == (n_bins - 2, n_bins - 1)
    for read, want in zip(f.reads(), f.want()):
        o = po.encode(read)
        fwd, rev = f.o.count(o), f.o.count(po.revcomp(o))
        m, b, s, _ = reduce_locate(fwd, rev, 1)
        assert (m, b, s) == (n,) + want, (read[:10], m, b, s, want)
        assert int((fwd == n).sum()) + int((rev == n).sum()) == 2  # two places hold the maximum, no more
    o = po.encode(f.same)
    fwd, rev = f.o.count(o), f.o.count(po.revcomp(o))
    assert int(fwd[f.SAME]) == n == int(rev[f.SAME])
    assert reduce_hits(fwd, rev, n) == [(f.SAME, 0, n), (f.SAME, 1, n)]  # one bin, two records
    o = po.encode(f.rev_lower)
    assert int(f.o.count(po.revcomp(o))[f.REV_LOWER[0]]) == n == int(f.o.count(o)[f.REV_LOWER[1]]) and f.REV_LOWER[0] < f.REV_LOWER[1]
    o = po.encode(f.fwd_lower)
    assert int(f.o.count(o)[f.FWD_LOWER[0]]) == n == int(f.o.count(po.revcomp(o))[f.FWD_LOWER[1]]) and f.FWD_LOWER[0] < f.FWD_LOWER[1]


def test_threshold_lengths_exist():
    zero, wrapped = PL.threshold_lengths()
    assert zero and wrapped, (zero, wrapped)  # both kinds exist among the lengths 7 .. 400 at r = 0.1, significance 0.95
    assert all(po.threshold(L, K, PL.R, PL.CONF) == 0 for L in zero)
    assert all(60000 < (po.threshold(L, K, PL.R, PL.CONF) & 0xFFFF) <= 0xFFFF for L in wrapped)
    reads, n_zero, n_wrapped = PL.threshold_reads()
    assert (n_zero, n_wrapped) == (2, 2) and [len(r) for r in reads] == [zero[0], zero[-1], wrapped[0], wrapped[-1], 250]


def test_mixed_batch_has_each_kind():
    reads, kinds = PL.mixed_batch()
    assert set(kinds) == {"free", "n_first", "n_last", "n_mid", "short", "long"}
    for r, kind in zip(reads, kinds):
        if kind == "free":
            assert set(r) <= set("ACGT") and K <= len(r) <= PL.MAX_LEN
        elif kind == "short":
            assert len(r) < K
        elif kind == "long":
            assert len(r) > PL.MAX_LEN and set(r) <= set("ACGT")
        else:
            at = {"n_first": 0, "n_last": len(r) - 1, "n_mid": 100}[kind]
            assert r.count("N") == 1 and r[at] == "N" and K <= len(r) <= PL.MAX_LEN
    assert 64 <= reads[kinds.index("n_mid")].index("N") < 128  # a middle tile
    assert [k for k in kinds[::2]] == ["free"] * 6  # interleaved


# ---------------------------------------------------------------- the LDS arithmetic of rb_lists.h
@pytest.mark.parametrize("sanitize", (False, True))
def test_pass_lds_bytes(tmp_path, sanitize):
    exe = str(tmp_path / "test_pass_lists")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall"] + flags + [os.path.join(ROOT, "tests", "cpp", "test_pass_lists.cpp"), "-o", exe])
    geometries = sorted({n for n, _ in SR.GEOMETRIES} | {n for n, _ in PL.TIE_GEOMETRIES} | {PL.OddBins.N_BINS})
    run = subprocess.run([exe] + [str(n) for n in geometries], capture_output=True, text=True)
    assert run.returncode == 0 and "failures: 0" in run.stdout, run.stdout + run.stderr
    got = {int(a): (int(b), int(c), int(d)) for a, b, c, d in re.findall(r"pass_lds n_bins (\d+) bytes (\d+) resident (\d+) count_resident (\d+)", run.stdout)}
    assert got[8192][1] == 9 and got[8192][2] == 9
    for n in geometries:
        assert got[n][0] <= 64 * 1024, (n, got[n])


# ---------------------------------------------------------------- the public surface
def test_symbol_and_constants():
    assert "rb_engine_set_pass_lists" in CC.declared_symbols(CC.HEADERS[1:]) and "rb_engine_set_pass_lists" not in CC.declared_symbols(CC.HEADERS[:1])
    assert (capi.RB_PASS_LISTS_OFF, capi.RB_PASS_LISTS_CURRENT, capi.RB_PASS_LISTS_BUILD) == (0, 1, 2)
    header = open(os.path.join(ROOT, "include", "readbouncer_amd_tuning.h")).read()
    for name, value in (("RB_PASS_LISTS_OFF", 0), ("RB_PASS_LISTS_CURRENT", 1), ("RB_PASS_LISTS_BUILD", 2)):
        assert re.search(r"#define %s %d\b" % (name, value), header)
    fields = [name for name, _ in capi.PassPlan._fields_]
    assert fields[-1] == "list_lines" and "reserved0" not in fields and len(fields) == 8  # the struct keeps its size
    assert hasattr(capi.Engine, "set_pass_lists")
    assert "rb_engine_set_pass_lists" in open(os.path.join(ROOT, "readbouncer_amd", "capi.py")).read()


# ---------------------------------------------------------------- the kernels, from the code object's metadata
def code_object_kernels(tmp_path, unit):
    """{kernel symbol: (private segment bytes, static group segment bytes)} of a kernel unit compiled for gfx950, from the notes of the
    code object"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        pytest.skip("no hipcc on this box: the resources are pinned where the library is built")
    readelf = os.path.join(os.path.dirname(os.path.realpath(hipcc)), "..", "llvm", "bin", "llvm-readelf")
    if not os.path.exists(readelf):
        readelf = shutil.which("llvm-readelf") or "/opt/rocm/llvm/bin/llvm-readelf"
    co = str(tmp_path / (unit + ".co"))
    flags = [f for f in KB.FLAGS if not f.startswith("-Rpass")]
    p = subprocess.run([hipcc] + flags + ["--cuda-device-only", "--no-gpu-bundle-output", "-c", os.path.join(KB.CSRC, unit), "-o", co], capture_output=True, text=True,
                       timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    notes = subprocess.run([readelf, "--notes", co], capture_output=True, text=True, check=True).stdout
    out = {}
    for entry in re.split(r"\n\s+- \.", "\n" + notes.split("amdhsa.kernels:")[1].split("amdhsa.target:")[0]):
        name = re.search(r"\.name:\s+(\S+)", entry) or re.search(r"^name:\s+(\S+)", entry)
        priv = re.search(r"private_segment_fixed_size:\s+(\d+)", entry)
        group = re.search(r"group_segment_fixed_size:\s+(\d+)", entry)
        if name and priv and group:
            out[name.group(1)] = (int(priv.group(1)), int(group.group(1)))
    return out


def test_new_kernels_exist_without_scratch_or_static_lds(tmp_path):
    found = code_object_kernels(tmp_path, "rb_pass_lists.hip")
    for kernel in ("ibf_locate_lists_kernel", "ibf_hits_lists_kernel"):
        builds = {m.groups(): v for name, v in found.items() for m in [re.search(r"%sILi(\d)ELb([01])EE" % kernel, name)] if m}
        assert sorted(builds) == [(l, nt) for l in "124" for nt in "01"], (kernel, sorted(found))
        for key, (scratch, static_lds) in builds.items():
            assert scratch == 0 and static_lds == 0, (kernel, key, scratch, static_lds)  # (their LDS is the launch's: rblist::pass_lds_bytes)
    assert [v for name, v in found.items() if "pass_lists_prep_kernel" in name] == [(0, 0)]
    assert len(found) == 13  # the unit holds these kernels and no other
    # rb_lists.hip, whose device code the unit shares through rb_lists_device.h, declares what it declared: the table builder's slot
    # images, nothing in the count kernel, and no kernel more
    lists = code_object_kernels(tmp_path, "rb_lists.hip")
    assert [v for name, v in lists.items() if "ibf_list_table_kernel" in name] == [(0, 2048)]
    assert {v for name, v in lists.items() if "ibf_count_lists_kernel" in name} == {(0, 0)} and len(lists) == 7

"""CPU-side checks of rb_dibf_assemble / rb_dibf_select_bins: the numpy model of tests/assemble_rules.py equals an oracle rebuild for every
plan generator (the exactness argument: a block number depends on the k-mer, the hash number and n_blocks only); rb_bin_ref is the 8
bytes the header says; assemble_plan normalises both plan forms; the calls are declared, exported, bound and documented and the header
still compiles as pedantic C99; without a GPU the calls refuse malformed plans on the host and say that there is no device otherwise;
and both builds of ibf_assemble_kernel compile for gfx950 without scratch at the waves per SIMD DESIGN 4.9 states."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from readbouncer_amd import capi
from tests import assemble_rules as R
from tests.kernel_build import builds, resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("rb_dibf_assemble", "rb_dibf_select_bins")
SHAPES = [64, 70, 130, 600, 1100]  # bins: W = 1, 2, 3, 10, 18
N_BLOCKS = 257
# DESIGN 4.9, "Resources": waves per SIMD of the builds <non-temporal>
DESIGN_WAVES = {(0,): 4, (1,): 4}

_sources = {}


def source(n_bins, seed=0):
    key = (n_bins, seed)
    if key not in _sources:
        _sources[key] = R.oracle_source(1000 * seed + n_bins, n_bins, N_BLOCKS)
    return _sources[key]


def check_against_rebuild(filters, seq_lists, plan):
    got = R.assemble_words([R.source_triple(f) for f in filters], plan)
    rebuilt = R.oracle_rebuild(seq_lists, plan, N_BLOCKS)  # (words() is a view: the filter stays alive while it is read)
    want = rebuilt.words()
    assert len(got) == R.n_words(len(plan), N_BLOCKS) == len(want)
    assert np.array_equal(got, want)
    assert not got[-4:].any()  # the tail / metadata words
    return got


@pytest.mark.parametrize("n_bins", SHAPES)
@pytest.mark.parametrize("name", sorted(R.SINGLE_SOURCE))
def test_model_equals_an_oracle_rebuild(name, n_bins):
    f, seqs = source(n_bins)
    plan = R.SINGLE_SOURCE[name](n_bins)
    got = check_against_rebuild([f], [seqs], plan)
    if name == "identity":
        assert np.array_equal(got, f.words())
    if name == "all_empty":
        assert not got.any()


def test_model_equals_an_oracle_rebuild_for_a_join_of_three():
    sizes = [130, 70, 600]
    fs = [source(n, seed=i + 1) for i, n in enumerate(sizes)]
    plan = R.interleaved_join(sizes)
    assert len(plan) == sum(sizes) and plan[:4] == [[(0, 0)], [(1, 0)], [(2, 0)], [(0, 1)]]
    check_against_rebuild([f for f, _ in fs], [s for _, s in fs], plan)
    # the plan of the issue's own check: 130 and 70 bins into 75, with empty, duplicated, cross-filter and 130-to-1 lists
    plan = [[] if j % 7 == 0 else [(0, j), (1, j % 70), (0, j)] for j in range(74)] + [[(0, b) for b in range(130)]]
    check_against_rebuild([fs[0][0], fs[1][0]], [fs[0][1], fs[1][1]], plan)


def test_pack_and_unpack_on_hand_written_words():
    w = np.array([1, 1 << 63, (1 << 5) | 2, 0, 3, 1], dtype=np.uint64)  # two blocks of three words: 130 bins
    m = R.unpack(w, 130, 2)
    assert m.shape == (2, 130) and np.flatnonzero(m[0]).tolist() == [0, 127, 129] and np.flatnonzero(m[1]).tolist() == [64, 65, 128]
    assert np.array_equal(R.pack(m), np.array([1, 1 << 63, 2, 0, 3, 1], dtype=np.uint64))  # bit 133 is no bin: dropped
    out = R.assemble_words([(w, 130, 2)], [[(0, 129), (0, 64)], [], [(0, 0)]])
    assert out.tolist() == [1 | 4, 1, 0, 0, 0, 0] and len(out) == R.n_words(3, 2) == 6


def test_rb_bin_ref_is_8_bytes():
    assert C.sizeof(capi.BinRef) == 8 and capi.BIN_REF_DTYPE.itemsize == 8
    assert [(n, getattr(capi.BinRef, n).offset) for n, _ in capi.BinRef._fields_] == [("filter", 0), ("bin", 4)]
    assert [capi.BIN_REF_DTYPE.fields[n][1] for n in capi.BIN_REF_DTYPE.names] == [0, 4]
    assert capi.RB_BIN_NONE == 2**64 - 1 and capi.RB_ASSEMBLE_MAX_SOURCES == 8


def test_assemble_plan_normalises_both_forms():
    lists = [[(0, 5)], [], [(1, 2), (0, 7), (1, 2)], []]
    off, refs = capi.assemble_plan(lists)
    assert off.dtype == np.uint64 and off.tolist() == [0, 1, 1, 4, 4]
    assert refs.dtype == capi.BIN_REF_DTYPE and refs.tolist() == [(0, 5), (1, 2), (0, 7), (1, 2)]
    for form in ((off, refs), (off.astype(np.int64), np.array([[0, 5], [1, 2], [0, 7], [1, 2]])), (off, refs.tolist())):
        o2, r2 = capi.assemble_plan(form)
        assert o2.dtype == np.uint64 and r2.dtype == capi.BIN_REF_DTYPE and o2.flags["C_CONTIGUOUS"] and r2.flags["C_CONTIGUOUS"]
        assert np.array_equal(o2, off) and np.array_equal(r2, refs)
    o0, r0 = capi.assemble_plan([[], []])
    assert o0.tolist() == [0, 0, 0] and len(r0) == 0
    with pytest.raises(ValueError):
        capi.assemble_plan((np.array([0, 3], np.uint64), refs[:2]))
    with pytest.raises(ValueError):
        capi.assemble_plan([[(0, 2**32)]])
    # the generators give what their names say
    assert R.groups_of(10, 4) == [[(0, 0), (0, 1), (0, 2), (0, 3)], [(0, 4), (0, 5), (0, 6), (0, 7)], [(0, 8), (0, 9)]]
    assert R.drop_every_third(7) == [[(0, 0)], [(0, 1)], [(0, 3)], [(0, 4)], [(0, 6)]]
    assert R.empty_middle(4, 1) == [[(0, 0)], [(0, 1)], [], [(0, 2)], [(0, 3)]] and R.reversed_order(3) == [[(0, 2)], [(0, 1)], [(0, 0)]]
    assert R.interleaved_join([2, 1, 3]) == [[(0, 0)], [(1, 0)], [(2, 0)], [(0, 1)], [(2, 1)], [(2, 2)]]
    assert R.truncated(R.identity(3), 5) == [[(0, 0)], [(0, 1)], [(0, 2)], [], []] and len(R.all_into_one(9)[0]) == 9


def test_calls_are_declared_exported_bound_and_documented():
    header = open(os.path.join(ROOT, "include", "readbouncer_amd.h")).read()
    tuning = open(os.path.join(ROOT, "include", "readbouncer_amd_tuning.h")).read()
    declared = set(re.findall(r"RB_API[^;(]*?\b(rb_[a-z0-9_]+)\s*\(", header))
    tuned = set(re.findall(r"RB_API[^;(]*?\b(rb_[a-z0-9_]+)\s*\(", tuning))
    out = subprocess.check_output(["nm", "-D", "--defined-only", capi.LIB_PATH], text=True)
    exported = set(re.findall(r" T (rb_[a-z0-9_]+)", out))
    for name in CALLS:
        assert name in declared and name in exported and name in capi.SIGNATURES and name not in tuned, name
    for name in ("rb_set_assemble_grid", "rb_assemble_last_seconds"):
        assert name in tuned and name in exported and name in capi.SIGNATURES and name not in declared, name
    assert "#define RB_ASSEMBLE_MAX_SOURCES 8" in header and "#define RB_BIN_NONE UINT64_MAX" in header
    assert "IBFBuild.cpp:223-321" in header.split("---- assemble:")[1].split("rb_dibf_insert")[0]
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "### 4.9" in design and "ibf_assemble_kernel" in design
    assert "assemble_cost.py" in open(os.path.join(ROOT, "profiles", "README.md")).read()
    assert "rb_dibf_assemble" in open(os.path.join(ROOT, "README.md")).read()
    assert "rb_dibf_assemble" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    hpp = open(os.path.join(ROOT, "include", "readbouncer_amd.hpp")).read()
    assert "rb_dibf_assemble" in hpp and "throw_status" in hpp


def test_header_compiles_as_pedantic_c99_and_the_calls_vet_their_arguments(tmp_path):
    src = tmp_path / "asm.c"
    src.write_text(r'''
#include <stddef.h>
#include "readbouncer_amd.h"
#include "readbouncer_amd_tuning.h"
int main(void)
{
    rb_bin_ref refs[2];
    uint64_t offsets[2];
    uint64_t bins[1];
    rb_dibf *out = 0;
    const rb_dibf *none[1];
    none[0] = 0;
    refs[0].filter = 0; refs[0].bin = 1; refs[1] = refs[0];
    offsets[0] = 0; offsets[1] = 2;
    bins[0] = RB_BIN_NONE;
    if (sizeof(rb_bin_ref) != 8 || offsetof(rb_bin_ref, filter) != 0 || offsetof(rb_bin_ref, bin) != 4) return 2;
    if (RB_ASSEMBLE_MAX_SOURCES != 8 || bins[0] != 0xFFFFFFFFFFFFFFFFull) return 3;
    rb_set_assemble_grid(0, 0);
    if (rb_assemble_last_seconds() != 0.0) return 4;
    /* null arguments, no sources, too many, no out bins, a null source: refused on the host, whatever the machine */
    if (rb_dibf_assemble(0, 1, offsets, refs, 1, &out) != RB_ERR_INVALID_ARG) return 5;
    if (rb_dibf_assemble(none, 1, 0, refs, 1, &out) != RB_ERR_INVALID_ARG) return 6;
    if (rb_dibf_assemble(none, 1, offsets, refs, 1, 0) != RB_ERR_INVALID_ARG) return 7;
    if (rb_dibf_assemble(none, 0, offsets, refs, 1, &out) != RB_ERR_INVALID_ARG) return 8;
    if (rb_dibf_assemble(none, 9, offsets, refs, 1, &out) != RB_ERR_INVALID_ARG) return 9;
    if (rb_dibf_assemble(none, 1, offsets, refs, 0, &out) != RB_ERR_INVALID_ARG) return 10;
    if (rb_dibf_assemble(none, 1, offsets, refs, 1, &out) != RB_ERR_INVALID_ARG) return 11;
    if (rb_dibf_select_bins(0, bins, 1, &out) != RB_ERR_INVALID_ARG) return 12;
    return out != 0;
}
''')
    exe = tmp_path / "asm"
    lib_dir = os.path.dirname(capi.LIB_PATH)
    subprocess.check_call(["cc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src),
                           "-o", str(exe), "-L", lib_dir, "-lreadbouncer_amd", "-Wl,-rpath," + lib_dir])
    assert subprocess.run([str(exe)], timeout=120).returncode == 0
    # the message names what is at fault
    L = capi.lib()
    h = C.c_void_p()
    off = np.array([0, 1], np.uint64)
    ref = np.zeros(1, capi.BIN_REF_DTYPE)
    assert L.rb_dibf_assemble(capi._handle_array([]), 9, off.ctypes.data, ref.ctypes.data, 1, C.byref(h)) == capi.RB_ERR_INVALID_ARG
    assert "9 sources" in L.rb_last_error().decode()


def test_cli_names_the_flags():
    cli = os.path.join(os.path.dirname(capi.LIB_PATH), "readbouncer_amd_cli")
    p = subprocess.run([cli, "--help"], capture_output=True, text=True, timeout=60)
    for word in ("--edit-ibf", "--with", "--plan", "--merge-every", "--drop-records", "EDIT_IBF"):
        assert word in p.stdout + p.stderr, word
    # exactly one of --plan / --merge-every / --drop-records; --output is needed
    p = subprocess.run([cli, "--edit-ibf", "a.ibf", "--output", "o.ibf"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 1 and "--plan" in p.stderr
    p = subprocess.run([cli, "--edit-ibf", "a.ibf", "--merge-every", "2", "--plan", "p.tsv", "--output", "o.ibf"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 1 and "one of" in p.stderr
    p = subprocess.run([cli, "--edit-ibf", "a.ibf", "--merge-every", "2"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 1 and "--output" in p.stderr
    # ... and without --edit-ibf its flags are refused, not ignored
    for flags in (["--output", "o.ibf"], ["--plan", "p.tsv"], ["--merge-every", "2"], ["--with", "b.ibf"], ["--drop-records", "x"]):
        p = subprocess.run([cli] + flags, capture_output=True, text=True, timeout=60)
        assert p.returncode == 1 and "--edit-ibf" in p.stderr, flags


def test_assemble_builds_compile_without_scratch_at_the_stated_waves():
    """compiled like test_kernel_resources.py does: both ibf_assemble_kernel builds have no scratch, and their waves per SIMD, from the
    compiler's own remarks, are what DESIGN 4.9 states"""
    found = builds(resources("rb_kernels.hip"), "ibf_assemble_kernel")
    assert set(found) == set(DESIGN_WAVES), sorted(found)
    design = open(os.path.join(ROOT, "DESIGN.md")).read().split("### 4.9")[1]
    for a, v in sorted(found.items()):
        print(a, v)
        assert v["scratch"] == 0, (a, v)
        assert v["occ"] == DESIGN_WAVES[a], (a, v)
    assert all("%d waves per SIMD" % w in design for w in set(DESIGN_WAVES.values()))

"""What tests/test_gpu_resume_lists.py relies on, checked without a GPU: the merge arithmetic of rb_resume_planes.h against plain uint16_t
arithmetic (a stand-alone program, plain and under the address and undefined-behaviour sanitizers), the fixtures of
tests/resume_lists_rig.py on the oracle alone, the new symbols where they belong, the builds of the new kernel from the code object's
metadata (no scratch, no static LDS: its LDS is the launch's, rblist::count_lds_bytes), and that rb_kernels.hip is as it was."""
import os
import re
import subprocess

import numpy as np
import pytest

from oracle import pyoracle as po
from readbouncer_amd import capi
from tests import kernel_build as KB
from tests import list_scan_rig as SR
from tests import pass_edges as PE
from tests import pass_lists_edges_rig as ER
from tests import resume_lists_rig as RL
from tests import resume_rules as RR
from tests import test_capi_cpu as CC
from tests.test_pass_lists_cpu import code_object_kernels

ROOT = KB.ROOT
K = SR.K


# ---------------------------------------------------------------- the merge arithmetic and the LDS bytes
@pytest.mark.parametrize("sanitize", (False, True))
def test_transpose_and_ripple_add(tmp_path, sanitize):
    exe = str(tmp_path / "test_resume_lists")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall"] + flags + [os.path.join(ROOT, "tests", "cpp", "test_resume_lists.cpp"), "-o", exe])
    geometries = sorted({n for n, _ in SR.GEOMETRIES} | {n for n, _ in RL.WRAP_GEOMETRIES})
    run = subprocess.run([exe] + [str(n) for n in geometries], capture_output=True, text=True)
    assert run.returncode == 0 and "failures: 0" in run.stdout, run.stdout + run.stderr
    got = {int(a): (int(b), int(c)) for a, b, c in re.findall(r"resume_lds n_bins (\d+) bytes (\d+) resident (\d+)", run.stdout)}
    assert sorted(got) == geometries and got[8192] == (16768, 9)  # nine workgroups per CU, as the count kernel
    # ... and that is what the launch asks for, with no hit mask behind it
    unit = open(os.path.join(KB.CSRC, "rb_resume_lists.hip")).read()
    assert re.search(r"const size_t lds = rblist::count_lds_bytes\(a\.f\.n_bins\);", unit) and "pass_lds_bytes" not in unit


# ---------------------------------------------------------------- the fixtures
def test_the_schedule_covers_what_it_names():
    sched = RL.schedule(K)
    assert sched == (6, 1, 1, 0, 5, 70, 3, 5, 200) and sum(sched) == RL.MAX_TOTAL and max(sched) == RL.MAX_CHUNK
    assert sched[0] < K and sched[3] == 0  # below k, an empty chunk
    assert sum(sched[:3]) == K + 1         # the first k-mer appears one base at a time across two seams
    assert (sched[5] + K - 1) - K + 1 == 70 > 64 and (sched[8] + K - 1) - K + 1 == 200 > 3 * 64  # full tiles and a part tile
    words = np.zeros(SR.n_bits(2112) // 64 + 8, dtype=np.uint64)
    f = SR.Planted(2112, 1, words)
    reads = RL.schedule_reads(f)
    assert len(reads) == 2 * len(f.bins) + 6 and all(len(r) >= RL.MAX_TOTAL for r in reads[-6:]) and all(set(r) <= RL.ACGT for r in reads)
    assert min(len(r) for r in reads) < sum(sched[:6])  # some run out: empty chunks later on


def test_the_wrap_fixture_walks_the_totals_across_the_wrap():
    n_bins, lines = ER.ODD
    words = np.zeros(SR.n_bits(n_bins) // 64 + 8, dtype=np.uint64)
    f = ER.Edges(n_bins, lines, words)
    ends = RL.wrap_ends(K)
    assert [e - K + 1 for e in ends] == list(RL.WRAP_TOTALS) == [32767, 65534, 65535, 65536, 65537, 70000]
    chunks = [b - a for a, b in zip((0,) + ends, ends)]
    assert max(chunks) == 32767 + K - 1 and max(chunks) + 31 - K + 1 < 65536  # every feed's delta fits the 16-bit counters
    fwd, rev = RL.wrap_reads(K)
    assert len(fwd) == ends[-1] == len(rev) and set(fwd) <= RL.ACGT and rev == SR.rc(fwd)
    assert n_bins % 2 == 1 and f.sat == (ER.EVEN_SAT, n_bins - 1) and ER.EVEN_SAT % 2 == 0
    for e, sat in zip(ends, RL.WRAP_SAT):
        c = f.o.count(po.encode(fwd[:e])).astype(np.uint16)
        assert sat == (e - K + 1) % 65536 and [int(c[b]) for b in f.sat] == [sat] * len(f.sat), (e, sat)
    # on the last feed the neighbour of EVEN_SAT crosses 2^16 by itself: a carry out of EVEN_SAT would show here
    for read in (fwd, rev):
        before = f.o.count(po.encode(read[:ends[-2]])).astype(np.int64)
        after = f.o.count(po.encode(read)).astype(np.int64)
        full = int(after[ER.EVEN_SAT + 1]) if int(after[ER.EVEN_SAT + 1]) > 65535 else None
        c16 = after.astype(np.uint16)
        assert 0 < int(c16[ER.EVEN_SAT + 1]) < RL.WRAP_TOTALS[-1] - 65536 + 1, (int(c16[ER.EVEN_SAT + 1]), full)
        assert int(before.astype(np.uint16)[ER.EVEN_SAT + 1]) > 60000  # ... from just below it


def test_the_mixed_feeds_hold_each_kind():
    words = np.zeros(SR.n_bits(4090) // 64 + 8, dtype=np.uint64)
    f = SR.Planted(4090, 2, words)
    first, second, third, kinds = RL.mixed_feeds(f)
    assert set(kinds) == {"free", "n_first", "n_last", "n_mid", "bad_slot", "too_long", "short"} and kinds[::2] == ["free"] * 6
    model = RR.Model(RL.MIX_SLOTS, RL.MIX_MAX_CHUNK, 2000)
    at = kinds.index
    # the first feed: an N in the chunk's first, last and a middle base (the second tile), the refusals, a string shorter than k
    chunk = {k: first[at(k)][1] for k in kinds}
    assert chunk["n_first"][0] == "N" == chunk["n_last"][-1] and chunk["n_mid"].index("N") == 70 and all(chunk[k].count("N") == 1 for k in ("n_first", "n_last", "n_mid"))
    assert first[at("bad_slot")][0] >= RL.MIX_SLOTS and len(chunk["too_long"]) == RL.MIX_MAX_CHUNK + 1 and len(chunk["short"]) == K - 2
    assert all(fl == RR.FIRST for _, _, fl in first) and all(fl == 0 for _, _, fl in second + third)
    taken = RL.taken_items(model, first, K)
    assert taken == [k in ("free", "short") for k in kinds]
    exp = model.feed(first, [f.o], [], capi.RB_MODE_CHECK_UNBLOCK)
    assert [int(s) for s in exp["status"][[at("bad_slot"), at("too_long")]]] == [capi.RB_ERR_INVALID_ARG] * 2
    assert int(exp["status"][at("short")]) == capi.RB_ERR_SHORT_READ
    # the second: N-free chunks everywhere, but the tail of the slot fed "....N" carries the N
    assert all(set(c) <= RL.ACGT for _, c, _ in second + third)
    assert "N" in RR.stitched(model.seen[at("n_last")], second[at("n_last")][1], K) and "N" not in RR.stitched(model.seen[at("n_first")], second[at("n_first")][1], K)
    taken = RL.taken_items(model, second, K)
    assert taken == [k not in ("n_last", "bad_slot", "too_long") for k in kinds]
    model.feed(second, [f.o], [], capi.RB_MODE_CHECK_UNBLOCK)
    # the third: that slot is back
    taken = RL.taken_items(model, third, K)
    assert taken == [k not in ("bad_slot", "too_long") for k in kinds]


# ---------------------------------------------------------------- the public surface
def test_symbols_and_the_plan_struct():
    tuning, boundary = CC.declared_symbols(CC.HEADERS[1:]), CC.declared_symbols(CC.HEADERS[:1])
    for name in ("rb_resume_set_lists", "rb_resume_plan"):
        assert name in tuning and name not in boundary
        assert name in open(os.path.join(ROOT, "readbouncer_amd", "capi.py")).read()
    assert [name for name, _ in capi.ResumePlan._fields_] == ["lanes_per_block_log2", "words_per_lane", "column_slices", "nontemporal", "list_lines"]
    assert hasattr(capi.Resume, "set_lists") and hasattr(capi.Resume, "plan")
    hpp = open(os.path.join(ROOT, "include", "readbouncer_amd.hpp")).read()
    assert "void set_lists(int mode)" in hpp and "rb_resume_plan_info plan(size_t filter) const" in hpp
    header = open(os.path.join(ROOT, "include", "readbouncer_amd_tuning.h")).read()
    assert "Spans, prefixes and resume are not affected" in header  # rb_engine_set_pass_lists keeps its promise


# ---------------------------------------------------------------- the kernels, from the code object's metadata
def test_new_kernels_exist_without_scratch_or_static_lds(tmp_path):
    found = code_object_kernels(tmp_path, "rb_resume_lists.hip")
    builds = {m.groups(): v for name, v in found.items() for m in [re.search(r"ibf_resume_lists_kernelILi(\d)ELb([01])EE", name)] if m}
    assert sorted(builds) == [(l, nt) for l in "124" for nt in "01"], sorted(found)
    for key, (scratch, static_lds) in builds.items():
        assert scratch == 0 and static_lds == 0, (key, scratch, static_lds)  # (their LDS is the launch's: rblist::count_lds_bytes)
    assert [v for name, v in found.items() if "resume_lists_prep_kernel" in name] == [(0, 0)]
    assert len(found) == 7  # the unit holds these kernels and no other


def test_rb_kernels_is_as_it_was():
    """the plain kernel serves the list form's call unchanged: rb_kernels.hip knows nothing of it, its resume builds are the twenty there
    were (tests/test_kernel_units_cpu.py pins every build's resources), and the per-kernel comparison of the device assembly with the
    parent commit's is on record"""
    text = open(os.path.join(KB.CSRC, "rb_kernels.hip")).read()
    assert "resume_lists" not in text and "plain_ctl" not in text and "rb_resume_planes" not in text
    table = KB.resources("rb_kernels.hip")
    assert len(KB.builds(table, "ibf_resume_kernel")) == 20 and all(v["scratch"] == 0 for v in KB.builds(table, "ibf_resume_kernel").values())
    note = open(os.path.join(ROOT, "profiles", "resume", "isa_identity_lists.txt")).read()
    assert re.search(r"compared (\d+), identical \1, different 0", note) and "only before: 0; only after: 0" in note

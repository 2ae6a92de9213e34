"""What the list-table tests rest on, checked without a GPU: the slot layout of readbouncer_amd/csrc/rb_lists.h (a stand-alone C++
program, plain and under the address and undefined-behaviour sanitizers), the resources of the kernels of rb_lists.hip at build time
(hipcc -Rpass-analysis=kernel-resource-usage), and -- on the oracle alone -- that the fixtures of tests/row_lists_rig.py and
tests/test_gpu_row_lists.py have the row populations and the census outcomes they claim."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from oracle import pyoracle as po
from tests import row_lists_rig as LR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "readbouncer_amd", "csrc")
K = LR.K


# ---------------------------------------------------------------- the slot layout
@pytest.mark.parametrize("sanitize", (False, True))
def test_slot_layout(tmp_path, sanitize):
    exe = str(tmp_path / "test_lists")
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall"] + flags + [os.path.join(ROOT, "tests", "cpp", "test_lists.cpp"), "-o", exe])
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and "failures: 0" in run.stdout, run.stdout + run.stderr


# ---------------------------------------------------------------- resources of the unit (tests/kernel_build.py's way, for rb_lists.hip)
FLAGS = ["-O3", "-std=c++17", "-fPIC", "-fvisibility=hidden", "-ffp-contract=off", "--offload-arch=gfx950", "-Rpass-analysis=kernel-resource-usage"]
REMARKS = (("occ", r"Occupancy \[waves/SIMD\]: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"), ("vgpr", r" VGPRs: (\d+)"),
           ("lds", r"LDS Size \[bytes/block\]: (\d+)"))
LDS_PER_CU = 160 * 1024


def parse(remarks):
    found, cur = {}, None
    for line in remarks.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            base = re.match(r"_ZN2rb\d+(\w+?_kernel)(?=[IE]|$)", m.group(1))
            args = re.search(r"_kernelI((?:L[ib]\d+E)+)E", m.group(1))
            cur = base.group(1) + ("<" + ",".join(re.findall(r"L[ib](\d+)E", args.group(1))) + ">" if args else "") if base else None
            if cur:
                assert cur not in found, cur
                found[cur] = {}
            continue
        if cur:
            for key, pat in REMARKS:
                m = re.search(pat, line)
                if m:
                    found[cur][key] = int(m.group(1))
    return found


def launch_lds(tmp_path):
    """{n_bins: (bytes of dynamic LDS launch_lists_nt asks for, workgroups a CU then holds)}, from rblist::count_lds_bytes itself: the
    stand-alone program prints what the header's functions -- the ones the launcher calls -- give"""
    exe = str(tmp_path / "test_lists_lds")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", os.path.join(ROOT, "tests", "cpp", "test_lists.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout
    return {int(a): (int(b), int(c)) for a, b, c in re.findall(r"count_lds n_bins (\d+) bytes (\d+) resident (\d+)", out)}


def test_list_kernels_resources(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        pytest.skip("no hipcc on this box: the resources are pinned where the library is built")
    p = subprocess.run([hipcc] + FLAGS + ["-c", os.path.join(CSRC, "rb_lists.hip"), "-o", str(tmp_path / "rb_lists.o")], capture_output=True,
                       text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    found = parse(p.stderr)
    lds = launch_lds(tmp_path)
    src = open(os.path.join(CSRC, "rb_lists.hip")).read()
    assert "lds = rblist::count_lds_bytes(a.f.n_bins)" in src and "rblist::count_cnt_dwords(a.f.n_bins)" in src  # the launcher asks the header
    want = {"ibf_count_lists_kernel<%d,%d>" % (lines, nt) for lines in (1, 2, 4) for nt in (0, 1)} | {"ibf_list_table_kernel"}
    assert set(found) == want, sorted(set(found) ^ want)
    assert not {k: v for k, v in found.items() if v["scratch"]}, found
    for name, r in found.items():
        if name.startswith("ibf_count_lists_kernel"):
            # one wave per workgroup, counters in dynamic LDS: nine workgroups of 8192 bins, eighteen of 4096 are to be resident per CU
            assert r["lds"] == 0
            for n_bins, (lds_bytes, resident) in lds.items():
                assert resident >= 1 and lds_bytes * resident <= LDS_PER_CU < lds_bytes * (resident + 1), (n_bins, lds_bytes, resident)
            assert r["occ"] * 4 >= lds[8192][1] == 9, (name, r)  # the registers allow the waves per CU that the LDS of an 8192-bin filter allows
        else:
            assert r["lds"] * (r["occ"] * 4 // 4) <= LDS_PER_CU, (name, r)  # four waves per workgroup
    assert {8192, 4096, 4090, 2112} <= set(lds)


# ---------------------------------------------------------------- the fixtures, on the oracle alone
def census(o, k, n_blocks, n_bins):
    pc = LR.row_bits(LR.expected_rows(o, k, 3, n_blocks), n_bins).sum(axis=1)
    over = [int((pc > (64 << i)).sum()) for i in range(3)]
    allowed = len(pc) >> 10
    lines = next((1 << i for i in range(3) if over[i] <= allowed), 0)  # rblist::choose_lines
    return lines, over, pc


def synth(seed, n_bins, n_blocks, k=K):
    o = po.OracleIBF(n_bins, 3, k, ((n_bins + 63) // 64) * 64 * n_blocks)
    o.fill_synth(seed)
    return o


def random_filter(load, seed, n_bins, n_blocks=1021, k=K):
    W = (n_bins + 63) // 64
    o = po.OracleIBF(n_bins, 3, k, W * 64 * n_blocks)
    bits = np.random.default_rng(seed).random((n_blocks, W * 64)) < load
    bits[:, n_bins:] = False
    o.words()[:n_blocks * W].reshape(n_blocks, W)[:] = np.packbits(bits, axis=1, bitorder="little").view(np.uint64)
    return o


@pytest.mark.parametrize("n_bins,lines", ((2112, 1), (8192, 2)))  # (33 words at design load: 21 bins per row)
def test_crafted_rows_have_the_populations_they_claim(n_bins, lines):
    o = synth(5, n_bins, LR.CRAFT_BLOCKS)
    words = o.words()
    c = LR.Crafted(n_bins, lines, words, ((n_bins + 63) // 64) * 64 * LR.CRAFT_BLOCKS)
    assert c.want == (0, 64 * lines - 1, 64 * lines, 64 * lines + 1, n_bins)
    got_lines, over, pc = census(c.o, K, LR.CRAFT_BLOCKS, n_bins)
    assert got_lines == lines, over                      # the rewritten blocks leave the census where the fill puts it
    assert [int(pc[r]) for r in c.ranks] == list(c.want)
    w = words[:LR.CRAFT_BLOCKS * c.W].reshape(LR.CRAFT_BLOCKS, c.W)
    sat = (w[:, c.sat // 64] >> np.uint64(c.sat % 64)) & np.uint64(1)
    assert int(sat.sum()) == LR.CRAFT_BLOCKS - 3         # SAT in every block but the empty row's three
    reads = c.reads()
    assert len(set(reads)) == len(reads) and all(set(r) <= set("ACGT") for r in reads)
    # the chosen k-mers alone: the empty row counts nothing, the others count SAT once
    assert [int(c.o.count(po.encode(s)).max()) for s in c.KMERS] == [0, 1, 1, 1, 1]


@pytest.mark.parametrize("n_bins,n_blocks,load,lines", ((2112, LR.CRAFT_BLOCKS, None, 1), (8192, LR.CRAFT_BLOCKS, None, 2), (8192, 1021, 0.15, 4)))
def test_silent_reads_hit_nothing_on_either_strand(n_bins, n_blocks, load, lines):
    filled = synth(5, n_bins, n_blocks) if load is None else random_filter(load, 15, n_bins, n_blocks)  # (owns the words `o` looks at)
    o = LR.silence(n_bins, n_blocks, filled.words(), ((n_bins + 63) // 64) * 64 * n_blocks)
    got_lines, over, pc = census(o, K, n_blocks, n_bins)
    assert got_lines == lines, over
    for s in LR.SILENT_KMERS:
        assert pc[LR.kmer_rank(s)] == 0 and pc[LR.kmer_rank(LR.revcomp(s))] == 0
    for r in LR.silent_reads():
        assert len(r) >= K and int(o.count(po.encode(r)).max()) == 0 and int(o.count(po.encode(LR.revcomp(r))).max()) == 0, r


@pytest.mark.parametrize("what,lines,min_over", (
    (("synth", 703, 4096, 1021, 7), 4, 1), (("synth", 703, 4096, 1024, 7), 4, 1), (("synth", 503, 4096, 1021, 5), 4, 1),
    (("synth", 503, 4096, 1024, 5), 4, 1), (("random", 0.15, 15, 8192, 1021, 7), 4, 1), (("random", 0.15, 15, 8192, 1024, 7), 4, 1),
    (("random", 0.15, 15, 8192, 1021, 5), 4, 1), (("random", 0.15, 15, 8192, 1024, 5), 4, 1),
    (("synth", 9, 4096, LR.SPARE_BLOCKS, 7), 1, 1), (("synth", 9, 8192, LR.SPARE_BLOCKS, 7), 2, 1),
    (("random", 0.17, 8192, 8192, 1021, 7), 4, 2), (("random", 0.24, 4090, 4090, 1021, 7), 4, 1), (("random", 0.6, 60, 8192, 1021, 7), 0, 0)))
def test_census_of_the_gpu_fixtures(what, lines, min_over):
    """the slot size the GPU tests expect of each filter they build, and that rows overflow it where they say some do"""
    if what[0] == "synth":
        _, seed, n_bins, n_blocks, k = what
        o = synth(seed, n_bins, n_blocks, k)
    else:
        _, load, seed, n_bins, n_blocks, k = what
        o = random_filter(load, seed, n_bins, n_blocks, k)
    got, over, pc = census(o, k, n_blocks, n_bins)
    assert got == lines, (what, over)
    if lines:
        assert min_over <= over[lines.bit_length() - 1] <= len(pc) >> 10, (what, over)

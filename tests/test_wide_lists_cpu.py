"""What the wide-list-table tests rest on, checked without a GPU: the slot layout of readbouncer_amd/csrc/rb_wide_lists.h (a stand-alone
C++ program, plain and under the address and undefined-behaviour sanitizers), the resources of the kernels of rb_wide_lists.hip at build
time (hipcc -Rpass-analysis=kernel-resource-usage), and -- on the oracle alone -- that the fixtures of tests/wide_lists_rig.py contain
what tests/test_gpu_wide_lists.py claims of them: the census verdicts, maxima at the named bins, rows at cap and cap + 1, N-carrying
k-mers that count, strands of 1 to 4 x 64 + 7 k-mers."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from oracle import pyoracle as po
from tests import wide_lists_rig as WR
from tests.test_row_lists_cpu import FLAGS, LDS_PER_CU, parse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "readbouncer_amd", "csrc")
K = WR.K


# ---------------------------------------------------------------- the slot layout
def build_layout_program(tmp_path, sanitize):
    exe = str(tmp_path / ("test_wide_lists" + ("_san" if sanitize else "")))
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall"] + flags + [os.path.join(ROOT, "tests", "cpp", "test_wide_lists.cpp"), "-o", exe])
    return exe


@pytest.mark.parametrize("sanitize", (False, True))
def test_slot_layout(tmp_path, sanitize):
    run = subprocess.run([build_layout_program(tmp_path, sanitize)], capture_output=True, text=True)
    assert run.returncode == 0 and "failures: 0" in run.stdout, run.stdout + run.stderr


def test_the_list_table_header_keeps_its_limits():
    """the wide table is a second object: rb_lists.h still ends at 8192 bins and four lines, and the wide header begins behind it"""
    src = open(os.path.join(CSRC, "rb_lists.h")).read()
    assert "constexpr uint32_t kMaxBins = 8192;" in src and "lines == 1 || lines == 2 || lines == 4" in src
    wide = open(os.path.join(CSRC, "rb_wide_lists.h")).read()
    assert "kWideMinBins = rblist::kMaxBins + 1" in wide and "hip_runtime" not in wide


# ---------------------------------------------------------------- resources of the unit
def test_wide_kernels_resources(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.exists(hipcc) or shutil.which(hipcc)):
        pytest.skip("no hipcc on this box: the resources are pinned where the library is built")
    p = subprocess.run([hipcc] + FLAGS + ["-c", os.path.join(CSRC, "rb_wide_lists.hip"), "-o", str(tmp_path / "rb_wide_lists.o")],
                       capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    found = parse(p.stderr)
    want = {"ibf_count_wide_lists_kernel<%d,%d,4>" % (lines, nt) for lines in WR.WIDE_LINES for nt in (0, 1)} | {"ibf_wide_list_table_kernel"}
    assert set(found) == want, sorted(set(found) ^ want)
    assert not {k: v for k, v in found.items() if v["scratch"]}, found
    out = subprocess.run([build_layout_program(tmp_path, False)], capture_output=True, text=True, check=True).stdout
    lds = {int(a): (int(b), int(c)) for a, b, c in re.findall(r"wide_count_lds n_bins (\d+) bytes (\d+) resident (\d+)", out)}
    assert {8193, 8256, 31000, 32256} <= set(lds) and lds[32256] == (65344, 2) and lds[31000][1] == 2
    src = open(os.path.join(CSRC, "rb_wide_lists.hip")).read()
    assert "lds = rbwide::count_lds_bytes(a.f.n_bins, NW)" in src  # the launcher asks the header
    for name, r in found.items():
        if name.startswith("ibf_count_wide_lists_kernel"):
            assert r["lds"] == 0  # dynamic: counters, spares, stages, partial maxima
            for n_bins, (lds_bytes, resident) in lds.items():
                assert lds_bytes <= 64 * 1024 and lds_bytes * resident <= LDS_PER_CU < lds_bytes * (resident + 1)
                # four waves per workgroup, four SIMDs per CU: a workgroup is one wave per SIMD.  From 16 300 bins on the LDS holds
                # at most four workgroups, and the registers allow every such geometry what the LDS allows (below that -- 8193 bins:
                # eight workgroups by LDS -- the registers of the four- and six-line builds stop at five to seven)
                if resident <= 4:
                    assert r["occ"] >= resident, (name, r, n_bins)
            assert r["occ"] >= 5, (name, r)
        else:
            assert r["lds"] == 4 * 8 * 128  # a slot image of eight lines per wave


# ---------------------------------------------------------------- the fixtures, on the oracle alone
@pytest.mark.parametrize("name", list(WR.FILTERS))
def test_census_of_the_table_fixtures(name):
    n_bins, k, load, seed, lines = WR.FILTERS[name]
    o = WR.table_fixture(name)
    assert (o.n_bins, o.kmer_size, o.n_blocks, o.bin_width) == (n_bins, k, WR.N_BLOCKS, (n_bins + 63) // 64)
    pc = WR.populations(WR.expected_rows(o))
    got, over = WR.census(pc)
    assert got == lines, (name, over)
    if lines:
        assert 1 <= over[WR.WIDE_LINES.index(lines)] <= len(pc) >> 10  # some rows overflow the chosen slot, no more than allowed
        if lines > 4:
            assert over[WR.WIDE_LINES.index(lines) - 1] > len(pc) >> 10  # ... and too many the next smaller one
    else:
        assert over[-1] > len(pc) >> 10
    if name == "over":
        assert over[-1] >= 3  # more rows than the side table of two that the GPU test allows


def test_every_slot_size_is_chosen_and_one_filter_is_refused():
    assert {f[4] for f in WR.FILTERS.values()} == {0, 4, 6, 8}
    assert {f[0] for f in WR.FILTERS.values()} >= {8193, 8256, 31000, 32256}
    assert {f[3] for f in WR.COUNT_FIXTURES.values()} == {4, 6, 8} and {f[0] for f in WR.COUNT_FIXTURES.values()} == {8193, 31000, 32256}


@pytest.mark.parametrize("name", list(WR.COUNT_FIXTURES))
def test_count_fixture_holds_what_it_claims(name):
    c = WR.count_fixture(name)
    n_bins = c.n_bins
    rows = WR.expected_rows(c.o)
    pc = WR.populations(rows)
    assert WR.census(pc)[0] == c.lines == WR.COUNT_FIXTURES[name][3]
    # rows at cap + 1 (an overflow slot), cap / 2 + 40 of one parity (swapped halves) and exactly cap
    assert [int(pc[r]) for r in c.ranks] == list(c.want) == [c.cap + 1, c.cap // 2 + 40, c.cap // 2 + 40, c.cap]
    bits = WR.row_bits(rows[c.ranks], n_bins)
    assert not bits[1, 1::2].any() and not bits[2, 0::2].any()  # all even, all odd: more than half a slot of one parity
    assert pc[WR.kmer_rank(WR.SILENT)] == 0 and pc[WR.kmer_rank(WR.revcomp(WR.SILENT))] == 0
    assert pc[WR.kmer_rank(WR.HOMOPOLYMER)] == 1 and rows[WR.kmer_rank(WR.HOMOPOLYMER), 0] == 1 << 5
    # maxima at the named bins
    want_bins = WR.best_bins(n_bins)
    assert [b for _, b in c.plants] == want_bins
    assert {0, 8191, 8192, n_bins - 1} <= set(want_bins) and (n_bins == 8193 or 8193 in want_bins)
    if n_bins % 2 == 0:
        assert {n_bins - 2, n_bins - 1} <= set(want_bins)  # both halves of the last counter dword
    else:
        assert (n_bins - 1) % 2 == 0                       # the last bin of an odd bin count: a low half with no partner
    for read, b in c.planted_reads():
        enc = po.encode(read)
        fwd, rev = c.o.count(enc), c.o.count(po.encode(WR.revcomp(read)))
        both = np.maximum(fwd, rev)
        n = len(read) - K + 1
        assert int(both.argmax()) == b and n - 12 <= int(both.max()) == c.o.raw_max(enc) <= n, (b, int(both.max()), n)
        assert int(np.sort(both)[-2]) < int(both.max())  # the maximum is that bin's alone
    # strands of every length from 1 to 4 x 64 + 7 k-mers
    assert [len(r) - K + 1 for r in c.length_reads()] == list(range(1, 4 * 64 + 8))
    # hits in the tiles of one wave alone: the planted stretch covers k-mers 64 w .. 64 w + 63, silence around it
    seq, b = c.plants[1]
    for wave in range(WR.WAVES):
        read = c.one_wave_reads()[2 * wave]
        assert read[64 * wave:64 * wave + 64 + K - 1] == seq[:64 + K - 1] and len(read) - K + 1 > 64 * 2 * WR.WAVES
        assert set(read[:64 * wave]) <= {"A"} and set(read[64 * wave + 64 + K - 1:]) == {"A"}
        fwd = c.o.count(po.encode(read))
        assert int(fwd.argmax()) == b and 64 - 8 <= int(fwd.max()) <= 64 + 2 * (K - 1)
    # N-carrying k-mers that count: the N sequence's own k-mers are in bin 77, the K of them that hold the N included
    enc = po.encode(c.n_seq)
    n = len(c.n_seq) - K + 1
    at = c.n_seq.index("N")
    whole = int(c.o.count(enc)[c.n_bin])
    n_free = int(c.o.count(po.encode(c.n_seq[:at]))[c.n_bin]) + int(c.o.count(po.encode(c.n_seq[at + 1:]))[c.n_bin])
    assert n - 12 <= whole <= n and whole == c.o.raw_max(enc) and n_free <= n - K and whole - n_free >= K - 3
    reads = c.n_reads()
    assert sum("N" in r for r in reads) == len(reads) // 2 and all(("N" in r) == (i % 2 == 0) for i, r in enumerate(reads))
    assert any(r.startswith("N") for r in reads) and any(r.endswith("N") for r in reads) and any("N" in r[5:-5] for r in reads)
    # a read of C counts bin 5 once per k-mer and nothing else on that strand
    fwd = c.o.count(po.encode("C" * 300))
    assert int(fwd[5]) == 300 - K + 1 and int(fwd.sum()) == 300 - K + 1
    # the crafted k-mers sit at the first, a middle and the last place of a group of eight, in several batches and tiles
    flagged = c.flagged_reads()
    places = {r.find(s) % 8 for r in flagged for s in WR.CRAFTED if s in r}
    assert {0, 3, 7} <= places
    assert len(c.all_reads()) < 400

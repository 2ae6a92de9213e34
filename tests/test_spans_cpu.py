"""CPU-side checks of the spans pass (rb_spans_batch / rb_spans_batch_device): the calls are declared, exported, bound and documented;
rb_span and rb_span_query are the bytes the header says; without a GPU the calls fail loudly and with malformed arguments they
refuse; the CLI names and parses its flag; the numpy restatement of the rules does what the header says on hand-written masks and
agrees with the oracle's full count vectors; and every build of ibf_spans_kernel compiles for gfx950 without scratch at no fewer
waves per SIMD than DESIGN 4.8 states."""
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
from tests.spans_rules import NONE, QUERY, SPAN, as_queries, expected_arrays, mask_words, position_hits, record

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = ("rb_spans_batch_device", "rb_spans_batch")
# DESIGN 4.8, "Resources": waves per SIMD of the builds <h at compile time (0: run-time), non-temporal>
DESIGN_WAVES = {(3, 0): 4, (3, 1): 4, (0, 0): 7, (0, 1): 7}


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
    section = header.split("---- spans:")[1].split("bin-sharded operation")[0]
    assert "IBFClassify.cpp:97-98" in section and "149-150" in section  # what the reference computes and discards, file:line
    body = re.search(r"typedef struct rb_spans_out \{(.*?)\} rb_spans_out;", header, re.S).group(1)
    assert re.findall(r"void \*(\w+);", body) == [n for n, _ in capi.SpansOut._fields_] == ["spans", "mask", "n_kmers", "status"]
    body = re.search(r"typedef struct rb_span \{(.*?)\} rb_span;", header, re.S).group(1)
    assert re.findall(r"uint32_t (\w+);", body) == [n for n, _ in capi.Span._fields_] == list(SPAN.names)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "4.8" in design and "ibf_spans_kernel" in design
    assert "spans_cost.py" in open(os.path.join(ROOT, "profiles", "README.md")).read()
    assert "rb_spans_batch" in open(os.path.join(ROOT, "README.md")).read()


def test_rb_span_is_24_bytes_and_rb_span_query_8_with_the_documented_offsets(tmp_path):
    assert C.sizeof(capi.Span) == 24 and C.sizeof(capi.SpanQuery) == 8
    assert [(n, getattr(capi.Span, n).offset, getattr(capi.Span, n).size) for n, _ in capi.Span._fields_] == \
        [("count", 0, 4), ("first", 4, 4), ("last", 8, 4), ("run_start", 12, 4), ("run_len", 16, 4), ("covered", 20, 4)]
    assert [(n, getattr(capi.SpanQuery, n).offset) for n, _ in capi.SpanQuery._fields_] == [("item", 0), ("bin", 4)]
    assert capi.SPAN_DTYPE == SPAN and SPAN.itemsize == 24 and [SPAN.fields[n][1] for n in SPAN.names] == [0, 4, 8, 12, 16, 20]
    assert capi.SPAN_QUERY_DTYPE == QUERY and QUERY.itemsize == 8 and [QUERY.fields[n][1] for n in QUERY.names] == [0, 4]
    # ... and the C compiler agrees, in C99
    src = tmp_path / "span.c"
    src.write_text(r'''
#include <stddef.h>
#include "readbouncer_amd.h"
int main(void)
{
    rb_spans_out out;
    rb_batch_desc desc;
    rb_span_query q[1];
    uint32_t n[1];
    out.spans = 0; out.mask = 0; out.n_kmers = n; out.status = 0;
    q[0].item = 0; q[0].bin = 0;
    desc.d_seqs = 0; desc.d_offsets = 0; desc.d_lens = 0; desc.n_items = 0; desc.max_len = 0; desc.d_nmask = 0;
    desc.d_nmask_offsets = 0; desc.chunk_start = 0; desc.chunk_length = 0; desc.d_read_ids = 0;
    if (sizeof(rb_span) != 24 || offsetof(rb_span, count) != 0 || offsetof(rb_span, first) != 4 || offsetof(rb_span, last) != 8 ||
        offsetof(rb_span, run_start) != 12 || offsetof(rb_span, run_len) != 16 || offsetof(rb_span, covered) != 20) return 2;
    if (sizeof(rb_span_query) != 8 || offsetof(rb_span_query, item) != 0 || offsetof(rb_span_query, bin) != 4) return 3;
    /* NULL engine: refused, whatever the machine */
    return rb_spans_batch_device(0, &desc, 0, q, 1, 0, &out, 0) == RB_OK || rb_spans_batch(0, "", 0, 0, 0, 0, 0, 0, q, 1, 0, &out) == RB_OK;
}
''')
    exe = tmp_path / "span"
    lib_dir = os.path.dirname(capi.LIB_PATH)
    subprocess.check_call(["cc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), str(src),
                           "-o", str(exe), "-L", lib_dir, "-lreadbouncer_amd", "-Wl,-rpath," + lib_dir])
    assert subprocess.run([str(exe)], timeout=120).returncode == 0


def test_calls_refuse_malformed_arguments_and_fail_loudly_without_a_gpu():
    L = capi.lib()
    keep = {"sp": np.zeros((1, 2), SPAN), "m": np.zeros((1, 2, 2), np.uint64), "n": np.zeros(1, np.uint32), "st": np.zeros(1, np.uint8),
            "q": as_queries([(0, 0)]), "seq": np.frombuffer(b"ACGTACGTACGTACGTACGT", dtype=np.uint8).copy(), "off": np.zeros(1, np.uint64),
            "len": np.array([20], np.uint32)}
    out = capi.SpansOut(keep["sp"].ctypes.data, keep["m"].ctypes.data, keep["n"].ctypes.data, keep["st"].ctypes.data)
    nothing = capi.SpansOut(None, None, None, None)
    desc = capi.BatchDesc(keep["seq"].ctypes.data, keep["off"].ctypes.data, keep["len"].ctypes.data, 1, 20, None, None, 0, 0, None)
    host = lambda e, o, mw=2: L.rb_spans_batch(e, keep["seq"].ctypes.data, keep["off"].ctypes.data, keep["len"].ctypes.data, 1, None, 0, 0,
                                               keep["q"].ctypes.data, 1, mw, o)
    dev = lambda e, d, o, mw=2: L.rb_spans_batch_device(e, d, 0, keep["q"].ctypes.data, 1, mw, o, None)
    assert dev(None, None, C.byref(out)) == capi.RB_ERR_INVALID_ARG
    assert dev(None, C.byref(desc), None) == capi.RB_ERR_INVALID_ARG
    assert dev(None, C.byref(desc), C.byref(nothing)) == capi.RB_ERR_INVALID_ARG
    assert host(None, None) == capi.RB_ERR_INVALID_ARG
    assert host(None, C.byref(nothing)) == capi.RB_ERR_INVALID_ARG
    # well-formed calls (mask_words == 0 with the status alone is one): without a GPU they say so, with one the NULL engine is refused
    want = capi.RB_ERR_NO_DEVICE if capi.device_count() <= 0 else capi.RB_ERR_INVALID_ARG
    only_status = capi.SpansOut(None, None, None, keep["st"].ctypes.data)
    assert dev(None, C.byref(desc), C.byref(out)) == want and host(None, C.byref(out)) == want
    assert dev(None, C.byref(desc), C.byref(only_status), 0) == want and host(None, C.byref(only_status), 0) == want


def test_cli_names_and_parses_the_flag():
    cli = os.path.join(os.path.dirname(capi.LIB_PATH), "readbouncer_amd_cli")
    p = subprocess.run([cli, "--help"], capture_output=True, text=True, timeout=60)
    for word in ("--report-spans", "classified_spans.tsv", "run_start", "covered"):
        assert word in p.stdout + p.stderr, word
    # the flag is taken, alone and beside its siblings (--help after it is still seen)
    for flags in (["--report-spans"], ["--report-bins", "--report-spans", "--report-hits", "--max-hits", "7"]):
        p = subprocess.run([cli] + flags + ["--help"], capture_output=True, text=True, timeout=60)
        assert p.returncode == 0 and "--report-spans" in p.stdout, flags
    # ... and it takes no argument: a word after it is not swallowed
    p = subprocess.run([cli, "--report-spans", "--max-hits"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 1 and "--max-hits" in p.stderr


def bits(n, *ones):
    h = np.zeros(n, dtype=bool)
    for o in ones:
        if isinstance(o, tuple):
            h[o[0]:o[1]] = True
        else:
            h[o] = True
    return h


def test_rules_on_hand_written_masks():
    k = 13
    # empty
    assert record(bits(200), k) == (0, NONE, NONE, NONE, 0, 0)
    assert not mask_words(bits(200), 4).any()
    # one bit: a run of one, k bases covered
    assert record(bits(200, 70), k) == (1, 70, 70, 70, 1, k)
    assert mask_words(bits(200, 70), 4).tolist() == [0, 1 << 6, 0, 0]
    # all ones: one run of n positions covers all n + k - 1 bases
    assert record(bits(129, (0, 129)), k) == (129, 0, 128, 0, 129, 129 + k - 1)
    assert mask_words(bits(129, (0, 129)), 3).tolist() == [2**64 - 1, 2**64 - 1, 1]
    # the cap leaves positions out of the mask only; words beyond n_kmers are zero
    assert mask_words(bits(129, (0, 129)), 2).tolist() == [2**64 - 1, 2**64 - 1]
    assert mask_words(bits(129, (0, 129)), 5).tolist() == [2**64 - 1, 2**64 - 1, 1, 0, 0]
    assert mask_words(bits(129, (0, 129)), 0).tolist() == []
    # a run across bit 63 / 64
    assert record(bits(200, (60, 70)), k) == (10, 60, 69, 60, 10, 10 + k - 1)
    assert mask_words(bits(200, (60, 70)), 2).tolist() == [0xF << 60, 0x3F]
    # two equal runs: the lowest wins; a longer one later wins over both
    assert record(bits(300, (10, 15), (100, 105)), k)[3:5] == (10, 5)
    assert record(bits(300, (10, 15), (100, 105), (200, 206)), k)[3:5] == (200, 6)
    assert record(bits(300, (62, 66), (126, 130)), k)[3:5] == (62, 4)  # both across a word boundary
    # covered: hits k - 1 apart share one base, hits k apart share none, closer ones overlap
    assert record(bits(100, 20, 20 + k - 1), k)[5] == 2 * k - 1
    assert record(bits(100, 20, 20 + k), k)[5] == 2 * k
    assert record(bits(100, 20, 20 + k + 5), k)[5] == 2 * k
    assert record(bits(100, 20, 23), k)[5] == k + 3
    # ... also where the two hits sit in different words, and at the last position (the bases reach the read's end)
    assert record(bits(100, 60, 60 + k - 1), k)[5] == 2 * k - 1 and record(bits(100, 60, 60 + k), k)[5] == 2 * k
    assert record(bits(100, 99), k) == (1, 99, 99, 99, 1, k)
    assert record(bits(64, 63), 31)[5] == 31 and record(bits(1, 0), 1) == (1, 0, 0, 0, 1, 1)


def random_filter(rng, n_bins, n_blocks, h, k, frag=300, planted=6):
    W = (n_bins + 63) // 64
    f = po.OracleIBF(n_bins, h, k, 64 * W * n_blocks)
    frags = []
    for b in rng.choice(n_bins, size=planted, replace=False).tolist():
        s = H.random_dna(rng, frag)
        f.insert(po.encode(s), b)
        frags.append((b, s))
    return f, frags


@pytest.mark.parametrize("k", [13, 20, 27])
def test_rules_against_the_oracles_full_count_vectors(k):
    """the sum identity: the hit positions of every bin number fwd[bin] and rev[bin] of the whole read, under both N rules, for reads
    with N; and the records the rules derive are consistent with those vectors"""
    rng = np.random.default_rng(k)
    f, frags = random_filter(rng, 70, 257, 3, k)
    reads = []
    for i, (b, s) in enumerate(frags):
        L = int(rng.integers(k, 200))
        a = int(rng.integers(0, len(s) - L + 1))
        r = H.mutate(rng, s[a:a + L], 0.05)
        if i % 2:
            r = r[:L // 3] + "N" + r[L // 3 + 1:L // 2] + "NNNN" + r[L // 2 + 4:]
        reads.append(r[:L])
    reads += [H.random_dna(rng, 150, with_n=0.03), "ACGT"[:k - 1], frags[0][1][:k]]
    all_bins = np.arange(f.n_bins)
    for rule in (3, 4):
        prev = po.set_revcomp_of_n(rule)
        try:
            for r in reads:
                o = po.encode(r)
                hits = position_hits(f, r, all_bins)
                assert hits.shape == (2, f.n_bins, max(len(r) - k + 1, 0))
                assert np.array_equal(hits[0].sum(axis=1), f.count(o)) and np.array_equal(hits[1].sum(axis=1), f.count(po.revcomp(o)))
                for b in all_bins[hits.any(axis=(0, 2))].tolist():
                    for s in range(2):
                        c, first, last, rs, rl, cov = record(hits[s, b], k)
                        assert c == int(hits[s, b].sum())
                        if c:
                            assert hits[s, b, first] and hits[s, b, last] and hits[s, b, rs:rs + rl].all() and 1 <= rl <= c
                            assert last - first + 1 >= c and k + c - 1 <= cov <= min(len(r), c * k)
        finally:
            po.set_revcomp_of_n(prev)
    # a read cut from a planted fragment hits its bin at every position
    assert position_hits(f, frags[0][1][:100], [frags[0][0]])[0].all()


def test_expected_arrays_apply_the_status_rules():
    rng = np.random.default_rng(2)
    f, frags = random_filter(rng, 100, 257, 3, 13)
    b0, s0 = frags[0]
    items = [s0[:80], "ACGT", s0[100:180]]
    st = np.array([0, capi.RB_ERR_SHORT_READ, capi.RB_ERR_BAD_CHUNK], np.uint8)
    q = as_queries([(0, b0), (1, b0), (2, b0), (3, b0), (0, 100), (0, (b0 + 1) % 100)])
    spans, mask, nk, status = expected_arrays(f, items, st, q, 3)
    assert status.tolist() == [0, capi.RB_ERR_SHORT_READ, capi.RB_ERR_BAD_CHUNK, capi.RB_ERR_INVALID_ARG, capi.RB_ERR_INVALID_ARG, 0]
    assert nk.tolist() == [68, 0, 0, 0, 0, 68]
    assert tuple(spans[0, 0]) == (68, 0, 67, 0, 68, 80) and mask[0, 0].tolist() == [2**64 - 1, 0xF, 0]
    for i in (1, 2, 3, 4):
        assert tuple(spans[i, 0]) == tuple(spans[i, 1]) == (0, NONE, NONE, NONE, 0, 0) and not mask[i].any()


def test_spans_builds_compile_without_scratch_at_the_stated_waves():
    """compiled like test_kernel_resources.py does: every ibf_spans_kernel build has no scratch, and its waves per SIMD, from the
    compiler's own remarks, are no lower than the figure DESIGN 4.8 states"""
    found = builds(resources("rb_kernels.hip"), "ibf_spans_kernel")
    assert set(found) == set(DESIGN_WAVES), sorted(found)
    design = open(os.path.join(ROOT, "DESIGN.md")).read().split("### 4.8")[1]
    for a, v in sorted(found.items()):
        print(a, v)
        assert v["scratch"] == 0, (a, v)
        assert v["occ"] >= DESIGN_WAVES[a], (a, v)
    assert all("%d waves per SIMD" % w in design for w in set(DESIGN_WAVES.values()))

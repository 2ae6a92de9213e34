"""What tests/test_gpu_prefix_lists.py relies on, checked without a GPU: the fixtures of tests/prefix_lists_rig.py are what they claim (on
the oracle alone), the rig's model of the take rule produces every kind of item, the three new symbols are declared in the tuning header
only and bound in capi.py, rb_pass_plan keeps its eight fields, and the new unit's code object holds exactly the six builds of
ibf_prefix_lists_kernel and the prep kernel, each without scratch memory and without static LDS (read from the code object's metadata)."""
import os
import re

import numpy as np

from oracle import pyoracle as po
from readbouncer_amd import capi
from tests import kernel_build as KB
from tests import list_scan_rig as SR
from tests import pass_lists_edges_rig as ER
from tests import prefix_lists_rig as XL
from tests import prefix_rules as PR
from tests import test_capi_cpu as CC
from tests.test_pass_lists_cpu import code_object_kernels

ROOT = KB.ROOT
K = XL.K


# ---------------------------------------------------------------- the fixtures
def test_seam_checkpoints_are_one_kmer_apart_across_the_seams():
    for lines in (1, 2, 4):
        cps = XL.seam_checkpoints(lines)
        kmers = [max(0, c - K + 1) for c in cps]
        assert list(cps) == sorted(set(cps)) and len(cps) <= 64
        assert cps[0] == K - 1 and cps[1] == K and kmers[:2] == [0, 1]  # one below k, exactly k
        assert {63, 64, 65} <= set(kmers) and {127, 128, 129} <= set(kmers)  # a tile's seam
        assert ({31, 32, 33} <= set(kmers)) == (lines == 4)  # a batch of 32 four-line slots
        assert sum(n > 200 for n in kmers) == 2  # two beyond every read
        assert any(a % 64 and b - a > 1 for a, b in zip(kmers, kmers[1:]))  # a range that begins inside a tile and holds several k-mers
    assert len(XL.ONE_CHECKPOINT) == 1 and len(XL.SIXTY_FOUR) == 64  # RB_PREFIX_MAX
    assert XL.SIXTY_FOUR[0] == K - 1 and XL.SIXTY_FOUR[-1] == K - 1 + 189 and list(XL.SIXTY_FOUR) == sorted(set(XL.SIXTY_FOUR))
    words = np.zeros(SR.n_bits(2112) // 64 + 8, dtype=np.uint64)
    f = SR.Planted(2112, 1, words)
    reads = XL.seam_reads(f)
    n = [len(r) - K + 1 for r in reads]
    assert max(n) == 200 and min(n) == 1 and {63, 64, 65} <= set(n) and all(set(r) <= XL.ACGT for r in reads)


def test_the_maximum_moves_between_strands_and_bins():
    for n_bins, lines in ((2112, 1), ER.ODD):
        words = np.zeros(SR.n_bits(n_bins) // 64 + 8, dtype=np.uint64)
        f = XL.Moves(n_bins, lines, words)
        scanned = set(SR.scan_bins(n_bins))
        assert all(a in scanned and b in scanned for a, b in f.pairs), f.pairs
        assert (0, 1) in f.pairs and (1, 0) in f.pairs and (504, 511) in f.pairs
        assert ((n_bins - 2, n_bins - 1) in f.pairs) if n_bins % 2 == 0 else ((n_bins - 1, 8) in f.pairs and (n_bins - 1) % 2 == 0)  # the pad half
        kmers = [c - K + 1 for c in XL.MOVE_CHECKPOINTS]
        assert XL.HEAD + XL.TAIL_FROM - 1 in kmers and XL.HEAD + XL.TAIL_FROM + 1 in kmers and XL.HEAD in kmers
        # (the pairs share bins, so a planted bin also counts k-mers it was not given: the counts below are bounds, the places exact)
        for (a, b), whole, tail in zip(f.pairs, f.whole, f.tail):
            for n, (fm, fb, rm, rb) in zip(kmers, XL.strand_maxima(f.o, whole, XL.MOVE_CHECKPOINTS)):
                assert fm >= min(n, XL.HEAD) and (rm, rb) == (n, b) and (fm < rm or n <= XL.HEAD), (a, b, n, fm, fb, rm, rb)
            won = {}
            for n, (fm, fb, rm, rb) in zip(kmers, XL.strand_maxima(f.o, tail, XL.MOVE_CHECKPOINTS)):
                assert fm >= min(n, XL.HEAD) and rm >= n - XL.TAIL_FROM, (a, b, n, fm, rm)
                won[n] = (0, fb) if fm > rm else (1, rb) if rm > fm else None
            # strand 0 and bin A hold the maximum alone at 40 and 60 k-mers, strand 1 and bin B at the last checkpoint
            assert won[40] == (0, a) == won[XL.HEAD] and won[XL.MOVE_KMERS] == (1, b), (a, b, won)


def test_the_counter_edge_stands_at_fffe_and_ffff():
    n_bins, lines = 2112, 1
    words = np.zeros(SR.n_bits(n_bins) // 64 + 8, dtype=np.uint64)
    f = ER.Edges(n_bins, lines, words)
    read = XL.edge_read()
    assert len(read) - K + 1 == XL.MAX_KMERS == 65535 and [c - K + 1 for c in XL.EDGE_CHECKPOINTS] == [0xFFFE, 0xFFFF]
    assert [c - K + 1 for c in XL.OVER_CHECKPOINTS] == [65535, 65536] and len(ER.over_read()) == XL.OVER_CHECKPOINTS[-1]
    for c, want in zip(XL.EDGE_CHECKPOINTS, (0xFFFE, 0xFFFF)):
        fwd = f.raw.count(po.encode(read[:c]))
        assert [int(fwd[b]) for b in f.sat] == [want] * len(f.sat) and int(fwd.max()) == want


def test_the_take_rule_produces_every_kind():
    seen = set()
    tiny = po.OracleIBF(64, 3, K, 64 * 64)
    for start, bound in ((0, XL.WIDE_BOUND), (XL.ODD_START, XL.WIDE_BOUND), (XL.ODD_START, XL.UNDERSTATED)):
        reads, kinds = XL.mixed_items(start)
        assert set(kinds) == set(XL.KINDS) and kinds[1::2] == ["free_short"] * len(XL.KINDS)
        body = {kind: r[start:] for r, kind in zip(reads[::2], kinds[::2])}
        assert len(body["free_short"]) < XL.C_LAST < len(body["free_long"]) and set(body["free_short"] + body["free_long"]) <= XL.ACGT
        assert body["n_before_last"].index("N") == XL.C_LAST - 1 and body["n_at_last"].index("N") == XL.C_LAST and body["n_first"][0] == "N"
        assert all(body[kind].count("N") == 1 for kind in ("n_before_last", "n_at_last", "n_first"))
        assert len(body["short"]) == K - 1 and body["empty"] == "" and XL.UNDERSTATED < len(body["under"]) == XL.UNDER_LEN <= XL.C_LAST
        beyond = reads[2 * XL.KINDS.index("beyond")]
        assert (len(beyond) < start) if start else beyond == ""
        got = [XL.takes(r, XL.C_LAST, chunk_start=start, max_len=bound) for r in reads]
        assert got == [XL.want_taken(kind, start, bound) for kind in kinds], (start, bound, got)
        assert XL.taken_counts(reads, XL.C_LAST, chunk_start=start, max_len=bound) == (sum(got), len(got) - sum(got)) and 0 < sum(got) < len(got)
        seen |= {(kind, t) for kind, t in zip(kinds, got)}
        # the oracle's rows of the items the rule leaves for their status: the kinds the plain form answers with a refusal
        exp = PR.expected_batch(reads, XL.MIXED_CHECKPOINTS, [tiny], [], PR.MODE_CLASSIFY_ANY, chunk_start=start, max_len=min(bound, XL.C_LAST))
        assert (exp["status"][kinds.index("beyond")] == PR.RB_ERR_BAD_CHUNK).all() == (start > 0)
        assert (exp["status"][kinds.index("under")] == PR.RB_ERR_INVALID_ARG).any() == (bound == XL.UNDERSTATED)
    # an N behind the last checkpoint does not send a long read away; one at c_last - 1 does; an understated bound does
    assert {("n_at_last", True), ("n_before_last", False), ("under", False), ("under", True), ("free_long", True), ("short", True),
            ("empty", True), ("beyond", False), ("n_first", False)} <= seen
    assert XL.MIXED_CHECKPOINTS[-1] == XL.C_LAST and XL.ODD_START % 2 == 1


# ---------------------------------------------------------------- the public surface
def test_symbols_and_structs():
    tuning, boundary = CC.declared_symbols(CC.HEADERS[1:]), CC.declared_symbols(CC.HEADERS[:1])
    source = open(os.path.join(ROOT, "readbouncer_amd", "capi.py")).read()
    for name in ("rb_engine_set_prefix_lists", "rb_engine_plan_prefix", "rb_engine_prefix_lists_items"):
        assert name in tuning and name not in boundary
        assert name in capi.SIGNATURES and name in source
    assert [name for name, _ in capi.PrefixPlan._fields_] == ["lanes_per_block_log2", "words_per_lane", "column_slices", "counter_planes", "nontemporal",
                                                               "hash_functions", "list_lines"]
    fields = [name for name, _ in capi.PassPlan._fields_]
    assert len(fields) == 8 and fields[-1] == "list_lines"  # rb_pass_plan is as it was
    for method in ("set_prefix_lists", "plan_prefix", "prefix_lists_items"):
        assert hasattr(capi.Engine, method)
    header = open(os.path.join(ROOT, "include", "readbouncer_amd_tuning.h")).read()
    assert re.search(r"typedef struct rb_prefix_plan_info \{[^}]*list_lines;\s*\} rb_prefix_plan_info;", header)
    assert "rb_engine_set_pass_lists does not reach the prefix pass" in header
    main = open(os.path.join(ROOT, "readbouncer_amd", "host", "rb_main.cpp")).read()
    assert "--prefix-lists off|current|build" in main and "int prefix_lists = RB_PASS_LISTS_OFF;" in main


# ---------------------------------------------------------------- the kernels, from the code object's metadata
def test_new_kernels_exist_without_scratch_or_static_lds(tmp_path):
    found = code_object_kernels(tmp_path, "rb_prefix_lists.hip")
    builds = {m.groups(): v for name, v in found.items() for m in [re.search(r"ibf_prefix_lists_kernelILi(\d)ELb([01])EE", name)] if m}
    assert sorted(builds) == [(l, nt) for l in "124" for nt in "01"], sorted(found)
    for key, (scratch, static_lds) in builds.items():
        assert scratch == 0 and static_lds == 0, (key, scratch, static_lds)  # (their LDS is the launch's: rblist::count_lds_bytes)
    assert [v for name, v in found.items() if "prefix_lists_prep_kernel" in name] == [(0, 0)]
    assert len(found) == 7  # the unit holds these kernels and no other
    unit = open(os.path.join(KB.CSRC, "rb_prefix_lists.hip")).read()
    assert re.search(r"const size_t lds = rblist::count_lds_bytes\(a\.f\.n_bins\);", unit) and "pass_lds_bytes" not in unit  # no hit mask
    assert "rb_prefix_lists.o" in open(os.path.join(KB.CSRC, "Makefile")).read()
    # rb_pass_lists.hip, whose header the unit shares, holds the kernels it held
    assert len(code_object_kernels(tmp_path, "rb_pass_lists.hip")) == 13
    assert "prefix_lists" not in open(os.path.join(KB.CSRC, "rb_kernels.hip")).read()

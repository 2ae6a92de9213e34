"""The pair table at the k production runs (tests/test_gpu_pair_lists.py stays at k = 5, 6 and 7): 4^13 slots of three lines, 24 GiB,
under RB_ROW_TABLE_PAIRS.  Only this size reaches the strided loop of ibf_pair_table_kernel (more slots than its 2^22 waves), a census
that samples (every 1024th pair), slot byte offsets beyond 2^32 in the builder, in the count kernel's gather address and in the re-read of
a tail or dense slot's index, tail and side arrays at their 4^13 capacities, and ranks 0 and 4^13 - 1 (A^13 and T^13: the pair that is
dense in every filter).  The fixture is tests/row_rig.py's WideCase on a filter of 16 381 blocks, whose k-mers with two coinciding blocks
(three in 16 381) give dense slots and whose fullest pairs take tail lines, so every kind of slot is in the table; the head of the table
is decoded against the oracle, and reads made of the head's tail and dense k-mers -- and of their reverse complements, whose slots lie
all over the table -- are counted bit for bit against the oracle beside the case's own batch."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import pyoracle as po
from readbouncer_amd import capi
from tests import helpers as H
from tests import pair_lists_rig as PR
from tests import row_lists_rig as LR
from tests import row_rig as RR
from tests import test_gpu_pair_lists as TP
from tests import test_gpu_row_table as RT

K, N_BINS, HEAD = 13, 8192, 4096


def kmer_of(rank):
    return "".join("ACGT"[(rank >> (2 * (K - 1 - i))) & 3] for i in range(K))


def test_slots_beyond_32_bit_offsets_with_every_kind_of_slot():
    torch = pytest.importorskip("torch")
    table = 4 ** K * 384
    free = torch.cuda.mem_get_info(0)[0]
    if free < 2 * table + (4 << 30):  # (the library refuses a table above half of the free memory)
        pytest.skip("a pair table of 24 GiB needs 52 GiB free, the device has %.1f" % (free / 2.0 ** 30))
    case = RR.WideCase(K, N_BINS)
    case.ranks_cover()
    d, o = RT.device_filter(N_BINS, LR.SPARE_BLOCKS, 3, K, seed=7, plant=case.plant)
    try:
        batch = H.pack_reads(case.reads)
        refs = {n_rule: RT.reference(o, batch, n_rule) for n_rule in (3, 4)}
        for ref in refs.values():
            case.fixture_holds(ref[0][:, 0])
        eng = RT.engine(d, TP.PAIRS)
        for nt in (0, 1):
            eng.set_nt_threshold(0 if nt else RT.NT_NEVER)
            for n_rule, ref in refs.items():
                eng.set_revcomp_of_n(n_rule)
                p = TP.check(eng, batch, ref, ("pairs", nt, n_rule), repeats=1)
                assert p["nontemporal"] == nt and p["row_table_bytes"] == table
        info = d.pair_table_info()
        print("pair table at k = 13:", {k: info[k] for k in ("bytes", "tail_bytes", "side_bytes", "tail_rows", "side_rows", "build_ms", "alloc_s", "census_over", "census_one_line")})
        assert info["builds"] == 1 and info["refused"] == 0 and info["rows"] == 4 ** K and info["lines"] == 3 and info["bytes"] == table, info
        assert info["census_rows"] == 65536 and info["census_over"][0] <= 2048 + 2 and info["census_over"][1] <= 64 + 2
        assert info["census_one_line"] > 32768 and info["census_over"][2] <= 64  # 81 bins per row: the list table would take two lines
        assert 0 < info["tail_rows"] <= info["tail_capacity"] == 4 ** K // 16 + 64
        assert 0 < info["side_rows"] <= info["side_capacity"] == 2 * (4 ** K // 512 + 64) and info["side_rows"] % 2 == 0
        # the head of the table against the AND of the oracle's blocks for x and rc(x), tail lines and dense rows followed
        slots = np.zeros(HEAD * PR.CANON, dtype=np.uint16)
        tails = np.zeros(info["tail_rows"] * 32, dtype=np.uint32)
        side = np.zeros(info["side_rows"] * info["stride_words"], dtype=np.uint64)
        assert capi.lib().rb_dibf_pair_table_download(d.h, slots.ctypes.data, len(slots), tails.ctypes.data, len(tails), side.ctypes.data, len(side)) == 0
        slots, tails, side = slots.reshape(HEAD, PR.CANON), tails.reshape(-1, 32), side.reshape(info["side_rows"], -1)
        W = N_BINS // 64
        blocks = o.words()[:LR.SPARE_BLOCKS * W].reshape(LR.SPARE_BLOCKS, W)

        def rows_of(kmers):
            rows = np.full((len(kmers), W), ~np.uint64(0), dtype=np.uint64)
            for hash_no in range(3):
                idx = np.array([o.block_index(po.kmer_value(po.encode(s), K), hash_no) for s in kmers], dtype=np.int64)
                rows &= blocks[idx]
            return LR.row_bits(rows, N_BINS)

        head = [kmer_of(r) for r in range(HEAD)]
        wantA, wantB = rows_of(head), rows_of([PR.revcomp(s) for s in head])
        A, B, kind = PR.decode_slots(slots, tails, side[:, :W], N_BINS, whole=False)
        assert np.array_equal(A, wantA) and np.array_equal(B, wantB)
        assert np.array_equal(kind, PR.kind_of(wantA.sum(axis=1), wantB.sum(axis=1)))
        assert kind[0] == PR.DENSE and (kind == PR.TAIL).any() and (kind == PR.PLAIN).any()  # A^13 / T^13, and every kind of slot
        # reads of the head's tail and dense k-mers and of their reverse complements (slots far beyond 2^32 bytes): alone, first and last
        # of a group of eight, and many in a row over several tiles and waves
        tail_k = [head[r] for r in np.nonzero(kind == PR.TAIL)[0][:12]]
        dense_k = [head[r] for r in np.nonzero(kind == PR.DENSE)[0][:4]]
        special = tail_k + dense_k
        far = [PR.revcomp(s) for s in special]
        assert max(LR.kmer_rank(s) for s in far) * 384 > 2 ** 32
        reads = special + far + [a + b for a, b in zip(special, far)] + ["".join(special), "".join(far), "".join(far + special) * 3]
        extra = H.pack_reads(reads)
        ref = RT.reference(o, extra)
        for nt in (0, 1):
            eng.set_nt_threshold(0 if nt else RT.NT_NEVER)
            eng.set_revcomp_of_n(3)
            TP.check(eng, extra, ref, ("tail and dense slots at k = 13", nt), repeats=1)
        assert d.pair_table_info()["builds"] == 1
        eng.destroy()
        torch.cuda.synchronize()
        with_table = torch.cuda.mem_get_info(0)[0]
    finally:
        d.free()
    assert torch.cuda.mem_get_info(0)[0] >= with_table + table  # the table went with the filter

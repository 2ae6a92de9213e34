"""The list table at the k production runs (tests/test_gpu_row_lists.py stays at k = 5 and 7): 4^13 slots of two lines, 16 GiB, under
RB_ROW_TABLE_LISTS.  Only this size reaches the strided loop of ibf_list_table_kernel (more slots than its 2^22 waves), a census that
samples (every 1024th row), slot byte offsets beyond 2^32 in the builder and in the count kernel's gather address, and ranks 0 and
4^13 - 1.  The fixture is tests/row_rig.py's WideCase on a filter of 16 381 blocks (with 1021, three rows in a thousand are the AND of
two blocks only and no slot size is allowed that many overflows: tests/row_lists_rig.py); a small batch, bit for bit against the oracle.
The same table then serves locate and hits (RB_PASS_LISTS_CURRENT): list_count_strand, the strand loop of their kernels, loads a tile's
bases with lanes 0 to 11 of its second load at k = 13 and forms ranks of 26 bits -- the case's reads and strands of 1, 63, 64, 65 and 129
k-mers, all-A and all-T, on either strand, through tests/test_gpu_pass_lists.py's run_both."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from readbouncer_amd import capi
from tests import helpers as H
from tests import pass_lists_edges_rig as ER
from tests import row_lists_rig as LR
from tests import row_rig as RR
from tests import test_gpu_pass_lists as GP
from tests import test_gpu_row_lists as TL
from tests import test_gpu_row_table as RT

K, N_BINS, HEAD = 13, 8192, 4096


def test_slots_beyond_32_bit_offsets():
    torch = pytest.importorskip("torch")
    table = 4 ** K * 256
    free = torch.cuda.mem_get_info(0)[0]
    if free < 2 * table + (2 << 30):  # (the library refuses a table above half of the free memory)
        pytest.skip("a list table of 16 GiB needs 34 GiB free, the device has %.1f" % (free / 2.0 ** 30))
    case = RR.WideCase(K, N_BINS)
    case.ranks_cover()
    d, o = RT.device_filter(N_BINS, LR.SPARE_BLOCKS, 3, K, seed=7, plant=case.plant)
    try:
        batch = H.pack_reads(case.reads)
        refs = {n_rule: RT.reference(o, batch, n_rule) for n_rule in (3, 4)}
        for ref in refs.values():
            case.fixture_holds(ref[0][:, 0])
        eng = RT.engine(d, TL.LISTS)
        for nt in (0, 1):
            eng.set_nt_threshold(0 if nt else RT.NT_NEVER)
            for n_rule, ref in refs.items():
                eng.set_revcomp_of_n(n_rule)
                p = TL.check(eng, batch, ref, ("lists", nt, n_rule), TL.LISTS_KERNEL, repeats=1)
                assert p["nontemporal"] == nt and p["row_table_bytes"] == table
        info = d.list_table_info()
        assert info["builds"] == 1 and info["refused"] == 0 and info["rows"] == 4 ** K and info["lines"] == 2 and info["bytes"] == table, info
        assert info["census_rows"] == 65536 and info["census_over"][0] > 32768 and info["census_over"][1] <= 64  # 81 bins per row
        assert 0 < info["side_rows"] <= info["side_capacity"] == 4 ** K // 512 + 64
        # locate and hits from the table that is there now: every counter of both strands (min_count 1, room for every bin)
        pe = GP.lists_engine([d])
        cached = ER.CachedCounts(o)
        reads = list(case.reads) + ER.strand_reads(K)
        for nt in (0, 1):
            pe.set_nt_threshold(0 if nt else RT.NT_NEVER)
            GP.run_both(pe, [cached], reads, [2], ("k = 13, locate and hits", nt))
        pe.destroy()
        assert d.list_table_info()["builds"] == 1
        # the head of the table against the AND of the oracle's blocks, overflow slots followed into the side table; the tail is what
        # the all-T read gathered
        slots = np.zeros(HEAD * 128, dtype=np.uint16)
        side = np.zeros(info["side_rows"] * info["stride_words"], dtype=np.uint64)
        assert capi.lib().rb_dibf_list_table_download(d.h, slots.ctypes.data, len(slots), side.ctypes.data, len(side)) == 0
        slots, side = slots.reshape(HEAD, 128), side.reshape(info["side_rows"], -1)
        W = N_BINS // 64
        blocks = o.words()[:LR.SPARE_BLOCKS * W].reshape(LR.SPARE_BLOCKS, W)
        r = np.arange(HEAD)
        digits = np.stack([(r >> (2 * (K - 1 - i))) & 3 for i in range(K)], axis=1).astype(np.uint8)
        from oracle import pyoracle as po
        expected = np.full((HEAD, W), ~np.uint64(0), dtype=np.uint64)
        for hash_no in range(3):
            idx = np.array([o.block_index(po.kmer_value(np.ascontiguousarray(digits[i]), K), hash_no) for i in range(HEAD)], dtype=np.int64)
            expected &= blocks[idx]
        want = LR.row_bits(expected, N_BINS)
        over = slots[:, 0] == LR.OVERFLOW_MARK
        assert np.array_equal(over, want.sum(axis=1) > 128)
        got = np.zeros_like(want)
        rr, cc = np.nonzero((slots < LR.OVERFLOW_MARK) & ~over[:, None])
        got[rr, slots[rr, cc]] = True
        if over.any():
            idx = slots[over, 1].astype(np.int64) | (slots[over, 2].astype(np.int64) << 16)
            assert (idx < info["side_rows"]).all() and len(set(idx.tolist())) == len(idx)
            got[over] = LR.row_bits(side[idx][:, :W], N_BINS)
        assert np.array_equal(got, want)
        eng.destroy()
        torch.cuda.synchronize()
        with_table = torch.cuda.mem_get_info(0)[0]
    finally:
        d.free()
    assert torch.cuda.mem_get_info(0)[0] >= with_table + table  # the table went with the filter

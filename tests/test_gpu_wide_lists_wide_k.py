"""The wide list table at the k production runs (tests/test_gpu_wide_lists.py stays at k = 5 and 7): 4^13 slots of four lines, 32 GiB,
on a filter of 8193 bins (129 words) and 16 381 blocks.  Only this size reaches the strided loop of ibf_wide_list_table_kernel (more
slots than its 2^22 waves), a census that samples (every 1024th row), slot byte offsets beyond 2^32 and 2^34 in the builder and in the
count kernel's gather address, and ranks 0 and 4^13 - 1.  The fixture is tests/row_rig.py's WideCase; a small batch, bit for bit against
the oracle, and the head of the table against the AND of the oracle's blocks."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from readbouncer_amd import capi
from tests import helpers as H
from tests import row_lists_rig as LR
from tests import row_rig as RR
from tests import test_gpu_row_table as RT
from tests import test_gpu_wide_lists as TW
from tests import wide_lists_rig as WR

K, N_BINS, HEAD, LINES = 13, 8193, 4096, 4


def test_slots_beyond_32_bit_offsets():
    torch = pytest.importorskip("torch")
    table = 4 ** K * LINES * 128
    free = torch.cuda.mem_get_info(0)[0]
    if free < 2 * table + (2 << 30):  # (the library refuses a table above half of the free memory)
        pytest.skip("a wide list table of 32 GiB needs 66 GiB free, the device has %.1f" % (free / 2.0 ** 30))
    case = RR.WideCase(K, N_BINS)
    case.ranks_cover()
    d, o = RT.device_filter(N_BINS, LR.SPARE_BLOCKS, 3, K, seed=7, plant=case.plant)
    try:
        batch = H.pack_reads(case.reads)
        refs = {n_rule: RT.reference(o, batch, n_rule) for n_rule in (3, 4)}
        for ref in refs.values():
            case.fixture_holds(ref[0][:, 0])
        info = d.wide_list_table_build()
        assert info["builds"] == 1 and info["refused"] == 0 and info["rows"] == 4 ** K and info["lines"] == LINES and info["bytes"] == table, info
        assert info["census_rows"] == 65536 and info["census_over"][0] <= 64  # 81 bins per row; the two-block rows are three in 16 381
        assert 0 < info["side_rows"] <= info["side_capacity"] == 4 ** K // 512 + 64
        eng = TW.engine([d], TW.CURRENT)
        for nt in (0, 1):
            eng.set_nt_threshold(0 if nt else RT.NT_NEVER)
            for n_rule, ref in refs.items():
                eng.set_revcomp_of_n(n_rule)
                p = TW.check(eng, batch, ref, ("wide", nt, n_rule), TW.WIDE_KERNEL, repeats=1)
                assert p["nontemporal"] == nt and p["row_table_bytes"] == table
        assert d.wide_list_table_info()["builds"] == 1
        # the head of the table against the AND of the oracle's blocks, overflow slots followed into the side table; the tail is what
        # the all-T read gathered
        cap = 64 * LINES
        slots = np.zeros(HEAD * cap, dtype=np.uint16)
        side = np.zeros(info["side_rows"] * info["stride_words"], dtype=np.uint64)
        assert capi.lib().rb_dibf_wide_list_table_download(d.h, slots.ctypes.data, len(slots), side.ctypes.data, len(side)) == 0
        slots, side = slots.reshape(HEAD, cap), side.reshape(info["side_rows"], -1)
        W = (N_BINS + 63) // 64
        blocks = o.words()[:LR.SPARE_BLOCKS * W].reshape(LR.SPARE_BLOCKS, W)
        r = np.arange(HEAD)
        digits = np.stack([(r >> (2 * (K - 1 - i))) & 3 for i in range(K)], axis=1).astype(np.uint8)
        from oracle import pyoracle as po
        expected = np.full((HEAD, W), ~np.uint64(0), dtype=np.uint64)
        for hash_no in range(3):
            idx = np.array([o.block_index(po.kmer_value(np.ascontiguousarray(digits[i]), K), hash_no) for i in range(HEAD)], dtype=np.int64)
            expected &= blocks[idx]
        want = WR.row_bits(expected, N_BINS)
        over = slots[:, 0] == WR.OVERFLOW_MARK
        assert np.array_equal(over, want.sum(axis=1) > cap)
        got = np.zeros_like(want)
        rr, cc = np.nonzero((slots < WR.OVERFLOW_MARK) & ~over[:, None])
        got[rr, slots[rr, cc]] = True
        if over.any():
            idx = slots[over, 1].astype(np.int64) | (slots[over, 2].astype(np.int64) << 16)
            assert (idx < info["side_rows"]).all() and len(set(idx.tolist())) == len(idx)
            got[over] = WR.row_bits(side[idx][:, :W], N_BINS)
        assert np.array_equal(got, want)
        eng.destroy()
        torch.cuda.synchronize()
        with_table = torch.cuda.mem_get_info(0)[0]
    finally:
        d.free()
    assert torch.cuda.mem_get_info(0)[0] >= with_table + table  # the table went with the filter

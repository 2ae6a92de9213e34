"""The row table at the k production runs (tests/test_gpu_row_table.py stays at k = 5 and 7, tables of at most 16 MiB): 4^12 and 4^13
rows.  Only these sizes reach the strided loop of ibf_row_table_kernel (more rows than its 2^22 waves), row byte offsets beyond 2^32
and row word offsets beyond 2^31 and 2^32 -- a dropped 64-bit cast in the builder or in count_strand's gather address lands in a lower
row and nothing smaller notices.  The filters are tiny (1021 blocks); the tables are 8, 32 and 64 GiB, built on the GPU in tens of
milliseconds and freed with their filter before the next case.  Bit for bit against the oracle; the fixture (tests/row_rig.py, WideCase)
is checked on the oracle first: the batch gathers rank 0, rank 4^k - 1 and every quarter of the table, and a planted read stands far
above the floor a wrong row would drop it to."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import pyoracle as po
from readbouncer_amd import capi
from tests import helpers as H
from tests import row_rig as RR
from tests import test_gpu_row_table as RT

HEAD_ROWS = 4096


def head_of_the_table(d, n_rows, stride):
    out = np.zeros(n_rows * stride, dtype=np.uint64)
    st = capi.lib().rb_dibf_row_table_download(d.h, out.ctypes.data, len(out))
    assert st == 0, st
    return out.reshape(n_rows, stride)


@pytest.mark.parametrize("k,n_bins", RR.WIDE_CASES)
def test_rows_beyond_32_bit_offsets(k, n_bins):
    torch = pytest.importorskip("torch")
    W = n_bins // 64
    table = 4 ** k * W * 8
    free = torch.cuda.mem_get_info(0)[0]
    if free < 2 * table + (1 << 30):  # (the library refuses a table above half of the free memory)
        pytest.skip("a table of %d GiB needs %d GiB free, the device has %.1f" % (table >> 30, (2 * table + (1 << 30)) >> 30, free / 2.0 ** 30))
    case = RR.WideCase(k, n_bins)
    case.ranks_cover()
    d, o = RT.device_filter(n_bins, RR.N_BLOCKS, 3, k, seed=7, plant=case.plant)
    try:
        batch = H.pack_reads(case.reads)
        refs = {n_rule: RT.reference(o, batch, n_rule) for n_rule in (3, 4)}
        for ref in refs.values():
            case.fixture_holds(ref[0][:, 0])
        off, force = RT.engine(d, RT.OFF), RT.engine(d, RT.FORCE)
        for nt in (0, 1):
            for eng in (off, force):
                eng.set_nt_threshold(0 if nt else RT.NT_NEVER)
            for n_rule, ref in refs.items():
                off.set_revcomp_of_n(n_rule), force.set_revcomp_of_n(n_rule)
                RT.check(off, batch, ref, ("off", k, n_bins, nt, n_rule), RT.PLAIN_KERNEL, masks=(15,))
                RT.check(force, batch, ref, ("force", k, n_bins, nt, n_rule), RT.ROWS_KERNEL, masks=(0, 15))
                assert force.plan(0, len(batch[2]), RR.WIDE_L)["nontemporal"] == nt
        info = d.row_table_info()
        stride = d.device_stride()
        assert info["builds"] == 1 and info["refused"] == 0 and info["rows"] == 4 ** k and info["bytes"] == 4 ** k * stride * 8 == table
        # the head of the table against the AND of the oracle's blocks (row r: the k-mer whose base-4 digits are r); its tail is what the
        # reads above gathered
        rows = head_of_the_table(d, HEAD_ROWS, stride)
        blocks = o.words()[:RR.N_BLOCKS * W].reshape(RR.N_BLOCKS, W)
        r = np.arange(HEAD_ROWS)
        digits = np.stack([(r >> (2 * (k - 1 - i))) & 3 for i in range(k)], axis=1).astype(np.uint8)
        expected = np.full((HEAD_ROWS, W), ~np.uint64(0), dtype=np.uint64)
        for hash_no in range(3):
            idx = np.array([o.block_index(po.kmer_value(np.ascontiguousarray(digits[i]), k), hash_no) for i in range(HEAD_ROWS)], dtype=np.int64)
            expected &= blocks[idx]
        assert np.array_equal(rows[:, :W], expected)
        off.destroy(), force.destroy()
        torch.cuda.synchronize()
        with_table = torch.cuda.mem_get_info(0)[0]
    finally:
        d.free()
    assert torch.cuda.mem_get_info(0)[0] >= with_table + table  # the table went with the filter: the next case has the memory

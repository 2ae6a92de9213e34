"""The wide forms of locate and hits at the k production runs (tests/test_gpu_wide_pass_lists.py stays at k = 7): 4^13 slots of four
lines, 32 GiB, on a filter of 8193 bins -- slot byte offsets beyond 2^32 and 2^34 in the gather address of the pass kernels, ranks 0 and
4^13 - 1.  Built as tests/test_gpu_wide_lists_wide_k.py builds it (tests/row_rig.py's WideCase); a handful of reads through locate and
hits, the wide form against the plain form: the same bytes, and locate's maxima the oracle's."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from readbouncer_amd import capi
from tests import helpers as H
from tests import row_lists_rig as LR
from tests import row_rig as RR
from tests import test_gpu_hits as GH
from tests import test_gpu_row_table as RT

K, N_BINS, LINES, CAP = 13, 8193, 4, 64
OFF, CURRENT = capi.RB_PASS_LISTS_OFF, capi.RB_PASS_LISTS_CURRENT


def test_pass_kernels_beyond_32_bit_offsets():
    torch = pytest.importorskip("torch")
    table = 4 ** K * LINES * 128
    free = torch.cuda.mem_get_info(0)[0]
    if free < 2 * table + (2 << 30):  # (the library refuses a table above half of the free memory)
        pytest.skip("a wide list table of 32 GiB needs 66 GiB free, the device has %.1f" % (free / 2.0 ** 30))
    case = RR.WideCase(K, N_BINS)
    case.ranks_cover()
    d, o = RT.device_filter(N_BINS, LR.SPARE_BLOCKS, 3, K, seed=7, plant=case.plant)
    try:
        buf, offs, lens = H.pack_reads(case.reads)
        ref = RT.reference(o, (buf, offs, lens))
        info = d.wide_list_table_build()
        assert info["builds"] == 1 and info["refused"] == 0 and info["lines"] == LINES and info["bytes"] == table, info
        eng = capi.Engine(0, [d], [])
        n, max_len = len(lens), int(lens.max())
        for nt in (0, 1):
            eng.set_nt_threshold(0 if nt else RT.NT_NEVER)
            got = {}
            for setting in (CURRENT, OFF):
                eng.set_wide_pass_lists(setting)
                assert eng.wide_pass_lines(0, max_len) == (LINES if setting == CURRENT else 0)
                loc = eng.locate(buf, offs, lens)
                prof = np.zeros(N_BINS, np.uint64)
                hit = eng.hits(buf, offs, lens, min_count=1, max_hits=CAP, bin_reads=prof, hits=GH.sentinel_hits(n, 1, CAP))
                got[setting] = (loc, hit, prof)
            ok = got[CURRENT][0]["status"] == capi.RB_OK
            assert np.array_equal(got[CURRENT][0]["max_count"][ok, 0], ref[0][ok, 0])  # the oracle's raw maxima
            for a, b in zip(got[CURRENT][:2], got[OFF][:2]):
                for key in a:
                    if isinstance(a[key], np.ndarray):
                        assert a[key].tobytes() == b[key].tobytes(), (nt, key)
            assert got[CURRENT][2].tobytes() == got[OFF][2].tobytes() and got[CURRENT][2].any()
        assert d.wide_list_table_info()["builds"] == 1
        eng.destroy()
    finally:
        d.free()

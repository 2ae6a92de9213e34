"""The wide form of the prefix pass at the k production runs (tests/test_gpu_wide_prefix_lists.py stays at k = 7): 4^13 slots of four
lines, 32 GiB, on a filter of 8193 bins -- slot byte offsets beyond 2^32 and 2^34 in the gather address of the ranged count, ranks 0 and
4^13 - 1.  Built as tests/test_gpu_wide_pass_lists_wide_k.py builds it (tests/row_rig.py's WideCase); a handful of reads through
Engine.prefixes, the wide form against the oracle's rows (tests/prefix_rules.py) and against the plain form: the same bytes."""
import pytest

pytestmark = pytest.mark.gpu

from readbouncer_amd import capi
from tests import helpers as H
from tests import prefix_rules as PR
from tests import row_lists_rig as LR
from tests import row_rig as RR
from tests import test_gpu_row_table as RT

K, N_BINS, LINES = 13, 8193, 4
OFF, CURRENT = capi.RB_PASS_LISTS_OFF, capi.RB_PASS_LISTS_CURRENT
KEYS = ("max_count", "decision", "best_target", "status", "prefix_len", "first_decided")


def test_prefix_kernel_beyond_32_bit_offsets():
    torch = pytest.importorskip("torch")
    table = 4 ** K * LINES * 128
    free = torch.cuda.mem_get_info(0)[0]
    if free < 2 * table + (2 << 30):  # (the library refuses a table above half of the free memory)
        pytest.skip("a wide list table of 32 GiB needs 66 GiB free, the device has %.1f" % (free / 2.0 ** 30))
    case = RR.WideCase(K, N_BINS)
    case.ranks_cover()
    d, o = RT.device_filter(N_BINS, LR.SPARE_BLOCKS, 3, K, seed=7, plant=case.plant)
    try:
        reads = list(case.reads)[:12]
        buf, offs, lens = H.pack_reads(reads)
        max_len = int(lens.max())
        cps = (K - 1, K, K + 63, K + 64, K + 100, max(K + 101, max_len // 2), max_len + 5)
        exp = PR.expected_batch(reads, cps, [o], [], PR.MODE_CHECK_UNBLOCK)
        info = d.wide_list_table_build()
        assert info["builds"] == 1 and info["refused"] == 0 and info["lines"] == LINES and info["bytes"] == table, info
        eng = capi.Engine(0, [d], [])
        for nt in (0, 1):
            eng.set_nt_threshold(0 if nt else RT.NT_NEVER)
            got = {}
            for setting in (CURRENT, OFF):
                eng.set_wide_prefix_lists(setting)
                assert eng.wide_prefix_lines(0, max_len, cps[-1]) == (LINES if setting == CURRENT else 0)
                eng.wide_prefix_lists_items(reset=True)
                got[setting] = eng.prefixes(buf, offs, lens, cps)
                PR.assert_same(got[setting], exp, (nt, setting))
                assert eng.wide_prefix_lists_items() == ((len(reads), 0) if setting == CURRENT else (0, 0))
            for key in KEYS:
                assert got[CURRENT][key].tobytes() == got[OFF][key].tobytes(), (nt, key)
            assert int(got[CURRENT]["max_count"].max()) > 0
        assert d.wide_list_table_info()["builds"] == 1
        eng.destroy()
    finally:
        d.free()

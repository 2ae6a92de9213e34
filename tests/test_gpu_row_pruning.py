"""The pruning paths the row form keeps (ibf_count_rows_kernel: the bound, the sub-tile checks, the strand lead, the probe parked in
LDS), on the fixtures that were built to make each of them tight -- tests/test_gpu_bound_pruning.py and test_gpu_strand_lead.py run
them on the three-hash kernel only -- and with the trace read under the row form.  k = 11 keeps the table of the 8192-bin filter at
4 GiB; the sparse filter (131 071 blocks) keeps chance hits at 0, and tests/test_row_engines_cpu.py holds the seeds at which every read
comes out at the maximum it was built for at this k.  Results bit for bit against the oracle and against pruning off, masks 0 - 3 and
15, repeats equal; every (read, slice) record written once and none behind the call's; no certificate tried; probe and lead as the
fixture names them; and, the reads being N-free, the stops of both strands equal to those of the three-hash kernel under the same mask
without certificate and lead line -- the parts the row build says it keeps unchanged."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from readbouncer_amd import capi
from tests import helpers as H
from tests import row_rig as RR
from tests import test_gpu_bound_pruning as BP
from tests import test_gpu_row_table as RT
from tests import test_gpu_strand_lead as SL

K = RR.PRUNE_K
TILE = SL.TILE
MASKS = (0, 1, 2, 3, 15)
SENTINEL = 0x5A5A5A5A5A5A5A5A
SLACK = 64  # records behind the call's that must keep the sentinel


@pytest.fixture(scope="module")
def rig():
    torch = pytest.importorskip("torch")
    table = 4 ** K * 128 * 8
    free = torch.cuda.mem_get_info(0)[0]
    assert free >= 2 * table + (1 << 30), "a row table of 4 GiB needs 9 GiB free, the device has %.1f" % (free / 2.0 ** 30)
    plants = RR.pruning_plants()
    d = BP.make_filter(8192, k=K)
    for plant in plants.values():
        plant.insert_into(d)
    rows, plain = RT.engine(d, RT.FORCE), RT.engine(d, RT.OFF)
    yield torch, d, plants, rows, plain
    rows.destroy(), plain.destroy(), d.free()


class SentinelTrace:
    """the kernel's records in a buffer longer than the call, filled with a value no record has"""

    def __init__(self, torch, eng, n):
        self.torch, self.eng, self.n = torch, eng, n
        self.t = torch.full((n + SLACK,), SENTINEL, dtype=torch.int64, device="cuda:0")
        torch.cuda.synchronize()
        eng.set_prune_trace(self.t.data_ptr())

    def take(self, label):
        self.torch.cuda.synchronize()
        r = self.t.cpu().numpy().view(np.uint64).copy()
        self.t.fill_(SENTINEL)
        self.torch.cuda.synchronize()
        assert (r[self.n:] == np.uint64(SENTINEL)).all(), (label, "a record behind the call's")
        r = r[:self.n]
        assert (r != np.uint64(SENTINEL)).all(), (label, "records not written", np.nonzero(r == np.uint64(SENTINEL))[0][:8].tolist())
        f = lambda sh, m: ((r >> np.uint64(sh)) & np.uint64(m)).astype(np.int64)
        t = dict(lead=f(0, 1), probed=f(1, 1), tried=f(2, 1), held=f(3, 1), line=f(4, 7), written=f(15, 1), stop_fwd=f(16, 0xFFFF),
                 stop_rev=f(32, 0xFFFF), rest=f(48, 0xFFFF))
        assert t["written"].all() and not t["rest"].any(), label
        return t

    def close(self):
        self.eng.set_prune_trace(None)


def run(eng, batch, ref, label):
    mc, _, dec, st = eng.classify(*batch)
    bad = np.nonzero((mc != ref[0]).any(axis=1))[0]
    assert len(bad) == 0, (label, [(int(i), int(batch[2][i]), mc[i].tolist(), ref[0][i].tolist()) for i in bad[:6]])
    assert np.array_equal(dec, ref[1]) and np.array_equal(st, ref[2]), (label, "decision/status")
    return mc, dec, st


@pytest.mark.parametrize("name", ("cross", "edges", "lead"))
def test_pruning_fixtures_on_the_row_form(rig, name):
    torch, d, plants, rows, plain = rig
    plant = plants[name]
    batch = H.pack_reads(plant.reads)
    lens = batch[2]
    n = lens.astype(np.int64) - K + 1
    assert not any(set(r) - set("ACGT") for r in plant.reads)  # N-free: every read is the row build's
    ref = SL.oracle_results(batch, [d], [])
    BP.fixture_holds(plant, ref[0][:, 0], name)
    for eng, kernel in ((rows, RT.ROWS_KERNEL), (plain, RT.PLAIN_KERNEL)):
        p = eng.plan(0, len(lens), int(lens.max()))
        assert p["kernel"] == kernel and p["lanes_per_block_log2"] == 6 and p["words_per_lane"] == 2 and p["column_slices"] == 1, p
        assert p["counter_planes"] == 10
    # parity: oracle == pruning off == every mask, every repeat
    rows.set_bound_pruning(0)
    off = run(rows, batch, ref, (name, "pruning off"))
    rows.set_bound_pruning(1)
    for mask in MASKS:
        rows.set_prune_parts(mask)
        for rep in range(2):
            out = run(rows, batch, ref, (name, mask, rep))
            assert all(np.array_equal(a, b) for a, b in zip(out, off)), (name, mask, rep, "differs from pruning off")
    assert d.row_table_info()["builds"] == 1
    # the trace
    tr_rows, tr_plain = SentinelTrace(torch, rows, len(lens)), SentinelTrace(torch, plain, len(lens))
    lead = getattr(plant, "lead", [None] * len(lens))
    try:
        for mask in MASKS:
            rows.set_prune_parts(mask)
            run(rows, batch, ref, (name, mask, "traced"))
            t = tr_rows.take((name, mask))
            assert not t["tried"].any() and not t["held"].any() and not t["line"].any(), (name, mask)  # nothing to certify
            probes = bool(mask & SL.LEAD)
            assert np.array_equal(t["probed"], ((n > TILE) & probes).astype(np.int64)), (name, mask)
            for i, want in enumerate(lead):
                if probes and want is not None:
                    assert t["probed"][i] == 1 and t["lead"][i] == want, (name, mask, i, int(n[i]), want, {k: int(v[i]) for k, v in t.items()})
                if not probes or n[i] <= TILE:
                    assert t["lead"][i] == 0, (name, mask, i)
            if probes:  # a leader that reached n drops the other strand behind its probe
                for i in range(len(lens)):
                    if plant.want[i] == n[i] and n[i] > TILE:
                        trailing = t["stop_rev"][i] if t["lead"][i] == 0 else t["stop_fwd"][i]
                        assert trailing == TILE, (name, mask, i, int(trailing))
            if mask & SL.SUB:
                assert ((t["stop_rev"] % 8 == 0) | (t["stop_rev"] == n)).all() and ((t["stop_fwd"] % 8 == 0) | (t["stop_fwd"] == n)).all()
            else:
                assert ((t["stop_rev"] % TILE == 0) | (t["stop_rev"] == n)).all() and ((t["stop_fwd"] % TILE == 0) | (t["stop_fwd"] == n)).all()
            # the three-hash kernel with the sub-tile checks and the lead of this mask, no certificate, no lead line: the same stops
            plain.set_prune_parts(mask & 3)
            run(plain, batch, ref, (name, mask, "three-hash"))
            p = tr_plain.take((name, mask, "three-hash"))
            assert not p["tried"].any() and not p["line"].any()
            for key in ("probed", "lead", "stop_fwd", "stop_rev"):
                bad = np.nonzero(t[key] != p[key])[0]
                assert len(bad) == 0, (name, mask, key, [(int(i), int(n[i]), int(t[key][i]), int(p[key][i])) for i in bad[:8]])
    finally:
        tr_rows.close(), tr_plain.close()
        rows.set_prune_parts(15), plain.set_prune_parts(15)


def test_sub_tile_stops_fall_inside_a_tile(rig):
    torch, d, plants, rows, _ = rig
    plant = plants["edges"]
    batch = H.pack_reads(plant.reads)
    n = batch[2].astype(np.int64) - K + 1
    tr = SentinelTrace(torch, rows, len(n))
    try:
        rows.set_prune_parts(SL.SUB)
        rows.classify(*batch)
        t = tr.take("sub")
        inside = ((t["stop_rev"] % TILE != 0) & (t["stop_rev"] < n)) | ((t["stop_fwd"] % TILE != 0) & (t["stop_fwd"] < n))
        assert inside.any(), "no strand was left inside a tile"
    finally:
        tr.close()
        rows.set_prune_parts(15)

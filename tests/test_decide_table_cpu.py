"""The decision table on the oracle alone (no GPU): tests/decide_cells.py enumerates the cells of check_unblock / classify_reads /
Read::classify(vector<TIbf>&), and the designed reads must land in every REQUIRED cell at least three times when the ORACLE counts
them in filters the ORACLE built.  This is what keeps tests/test_gpu_decide_table.py honest: the same reads, filters and cells are
used there, so a cell the GPU half never compares is a failure here first."""
import numpy as np
import pytest

from oracle import pyoracle as po
from tests import decide_cells as DC

_LEDGER = {}     # "oracle" -> {cell: reads}
_DECISIONS = {}  # mode -> set of (decision, status)
_RAN = set()


def test_required_and_impossible_are_the_cross_product():
    required, impossible = DC.REQUIRED, DC.IMPOSSIBLE
    full = set(DC.all_cells())
    assert len(full) == 3 * 2 ** 13
    assert set(required) | set(impossible) == full
    assert not set(required) & set(impossible)
    assert len(required) == len(set(required)) and len(required) % 3 == 0
    assert all(isinstance(why, str) and why and "\n" not in why for why in impossible.values())
    # the cells the issue names are among the required ones: D1>0, T1>0, D2>0, T2==0; a tie in either group; a filter skipped by its
    # own k; the zero and the wrapped threshold; D2>0 with D1==0 (the threshold at r - 0.02 is BELOW the one at r where r's has wrapped)
    bits = [c[1:] for c in required if c[0] == DC.MODE_CHECK_UNBLOCK]
    f = {n: i for i, n in enumerate(DC.FIELDS[1:])}
    assert any(b[f["D1>0"]] and b[f["T1>0"]] and b[f["D2>0"]] and not b[f["T2>0"]] for b in bits)
    assert any(b[f["D1>0"]] and b[f["T1>0"]] and not b[f["D2>0"]] and b[f["T2>0"]] for b in bits)
    assert any(b[f["D2>0"]] and not b[f["D1>0"]] for b in bits)
    for name in ("tie_d", "tie_t", "skipped", "thr0", "wrapped", "short_d", "short_t"):
        assert any(b[f[name]] for b in bits), name
    assert any(b[f["short_t"]] and b[f["T1>0"]] for b in bits)  # best_target is -1 although a later target filter matches


def test_the_d2_without_d1_cells_follow_from_the_oracles_thresholds():
    """D2>0 with D1==0 needs a length whose threshold at r - 0.02 is below the one at r: the oracle has such lengths (r's threshold is a
    wrapped negative while the other is not yet), so these cells are REQUIRED, not IMPOSSIBLE."""
    below = [(k, r, L) for k in (13, 15) for r in DC.RATES for L in DC.LENGTHS if DC.threshold(L, k, r - 0.02) < DC.threshold(L, k, r)]
    assert below
    assert DC.threshold(35, 13, 0.1) == 65529  # the reference's KAT
    assert [L for L in range(100, 140) if DC.threshold(L, 13, 0.1) == 0] == list(range(123, 131))


@pytest.mark.parametrize("name", sorted(DC.FILTER_SETS))
def test_designed_reads_through_the_oracle(name):
    ks, nd, nt = DC.set_ks(name)
    odep, otgt = DC.build_oracle_filters(name)
    reads = DC.designed_reads(name)
    assert all(len(r) <= DC.HALF for r in reads)
    buf, offs, lens = DC.pack(reads)
    encoded = [po.encode(r) for r in reads]
    raw = DC.oracle_raw(odep + otgt, buf, offs, lens)
    for r in DC.RATES:
        for mode in DC.MODES:
            cells = DC.cells_of_batch(raw, lens, ks, r, mode, nd, nt)
            DC.ledger_add(_LEDGER, "oracle", cells)
            dec, st, best = DC.oracle_expect(odep, otgt, reads, encoded, buf, offs, lens, r, mode)
            _DECISIONS.setdefault(mode, set()).update(zip(dec.tolist(), st.tolist()))
            assert ((best >= -1) & (best < max(nt, 1))).all()
    _RAN.add(name)


def test_every_required_cell_is_reached_on_the_oracle():
    assert _RAN == set(DC.FILTER_SETS), "the tests that fill the ledger did not all run"
    missing = DC.ledger_missing(_LEDGER, "oracle", DC.REQUIRED)
    assert not missing, "%d of %d required cells have fewer than %d reads:\n%s" % (
        len(missing), len(DC.REQUIRED), DC.MIN_READS_PER_CELL, "\n".join("%3d  %s" % (n, DC.describe(c)) for c, n in missing))
    assert not set(_LEDGER["oracle"]) & set(DC.IMPOSSIBLE), [DC.describe(c) for c in set(_LEDGER["oracle"]) & set(DC.IMPOSSIBLE)]


def test_the_designed_decisions_are_not_degenerate():
    assert _RAN == set(DC.FILTER_SETS), "the tests that fill the ledger did not all run"
    want = {DC.MODE_CHECK_UNBLOCK: {0, 1, 2}, DC.MODE_CLASSIFY_CHUNK: {0, 1}, DC.MODE_CLASSIFY_ANY: {0, 1}}
    for mode, decisions in want.items():
        assert {d for d, s in _DECISIONS[mode] if s == po.OK} == decisions, mode
        assert {s for _, s in _DECISIONS[mode]} == {po.OK, po.ERR_SHORT_READ}, mode
        assert all(d == 0 for d, s in _DECISIONS[mode] if s != po.OK)

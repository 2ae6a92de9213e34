"""What the GPU tests of the row table assume of their fixtures (tests/row_rig.py), asserted on the oracle alone: a fixture that has gone
stale fails here, on a machine without a GPU, and not as a puzzling kernel failure.
  - the five-filter rig: check_unblock answers unblock, keep and wait; best_target takes every value from -1 to 3; two row-counted
    targets tie and the first wins; the other two modes answer both ways;
  - the wide-k batches: ranks 0 and 4^k - 1, every quarter of the table, both sides of 2^22 rows at k = 12; planted reads stand far
    above the floor of the random ones;
  - the pruning plants at k = 11: every read comes out at the maximum it was built for (chance repeats of a k-mer inside a read are
    what a smaller k adds)."""
import numpy as np
import pytest

from oracle import pyoracle as po
from tests import helpers as H
from tests import row_rig as RR
from tests import test_gpu_bound_pruning as BP


@pytest.mark.parametrize("lens", ((40, 70, 71, 354), (354, 1100)))
def test_the_rig_covers_every_decision_and_best_target(lens):
    rig = RR.Rig()
    views = rig.oracle_filters()
    reads = rig.reads(lens)
    batch = H.pack_reads(reads)
    for n_rule in (3, 4):
        RR.rig_covers(rig, reads, {mode: RR.oracle_reference(views, reads, batch, n_rule, mode) for mode in RR.MODES})


def test_rule_b_separates_k5_from_k7():
    L = 360
    need5, need7 = RR.rule_b_need(5, 3, L), RR.rule_b_need(7, 3, L)
    assert need5 + 1 < need7 - 1  # a batch between the two exists
    assert RR.rule_b_need(RR.K, 3, L) == -(-(4 ** RR.K * 4) // (2 * (L - RR.K + 1) * 2))  # as test_auto_mode_policy computes it


@pytest.mark.parametrize("k,n_bins", RR.WIDE_CASES)
def test_wide_k_batches_reach_both_ends_of_the_table(k, n_bins):
    case = RR.WideCase(k, n_bins)
    assert 90 <= len(case.reads) <= 120
    below_top = case.ranks_cover()
    words = (n_bins // 64) * below_top  # word offset of the highest row short of the last one
    assert words * 8 > 2 ** 32
    if k == 13:
        assert words > (2 ** 31 if n_bins == 4096 else 2 ** 32)
    o = case.oracle_filter()
    buf, offs, lens = H.pack_reads(case.reads)
    for n_rule in (3, 4):
        prev = po.set_revcomp_of_n(n_rule)
        try:
            floor = case.fixture_holds(po.batch_raw_max(o, buf, offs, lens, 8))
        finally:
            po.set_revcomp_of_n(prev)
        assert floor <= 25


def test_pruning_fixtures_hold_at_k11():
    plants = RR.pruning_plants()
    o = RR.pruning_oracle_filter(plants)
    for name, plant in plants.items():
        assert plant.k == RR.PRUNE_K
        buf, offs, lens = H.pack_reads(plant.reads)
        BP.fixture_holds(plant, po.batch_raw_max(o, buf, offs, lens, 8), name)

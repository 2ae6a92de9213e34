"""The arithmetic of the row table (rb_dibf_row_table_build, ibf_count_rows_kernel) that needs no GPU: the row of a k-mer is its base-4
rank, the table is built from the base-5 value the oracle hashes, the auto mode's batch rule at config 3's shape, and the one-gather state
of the CPU model (profiles/prune_model.py)."""
import importlib.util
import os

import numpy as np
import pytest

from oracle import pyoracle as po

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("prune_model_rows", os.path.join(ROOT, "profiles", "prune_model.py"))
model = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(model)


def rank_of(ords):
    """the row of an N-free k-mer: its Dna5 ordinals as base-4 digits, first base most significant (count_strand, ROWS)"""
    r = 0
    for o in ords:
        r = (r << 2) | (int(o) & 3)
    return r


def value_of_rank(r, k):
    """the base-5 value the table kernel forms for row r (ibf_row_table_kernel)"""
    v = 0
    for i in range(k):
        v = v * 5 + ((r >> (2 * (k - 1 - i))) & 3)
    return v


@pytest.mark.parametrize("k", (1, 5, 13))
def test_rank_and_base5_value_name_the_same_kmer(k):
    rng = np.random.default_rng(k)
    ranks = set(range(4 ** k)) if k <= 5 else {0, 4 ** k - 1} | {int(x) for x in rng.integers(0, 4 ** k, size=2000)}
    f = po.OracleIBF(64, 3, k, 64 * 1021)
    for r in ranks:
        ords = np.array([(r >> (2 * (k - 1 - i))) & 3 for i in range(k)], dtype=np.uint8)
        assert rank_of(ords) == r < 4 ** k
        v = po.kmer_value(ords, k)  # what the oracle hashes for these bases
        assert value_of_rank(r, k) == v
        # ... and the reverse complement of an N-free k-mer is another N-free k-mer: it has a row of its own
        rc = po.revcomp(ords)
        assert rc.max() <= 3 and rank_of(rc) == sum((3 - int(o)) << (2 * i) for i, o in enumerate(ords))
        assert 0 <= f.block_index(v, 0) < 1021
    # the mapping is one to one: distinct ranks, distinct values
    some = sorted(ranks)[:4096]
    assert len({value_of_rank(r, k) for r in some}) == len(some)


def test_batch_rule_at_config_3():
    """rule (b): items x 2 x k-mers x (h - 1) >= 4^k x (h + 1) block transfers"""
    k, h, L = 13, 3, 360
    kmers = L - k + 1
    need = -(-(4 ** k * (h + 1)) // (2 * kmers * (h - 1)))
    assert kmers == 348 and need == 192842  # about 193 000 reads of 360 bp
    assert (need - 1) * 2 * kmers * (h - 1) < 4 ** k * (h + 1) <= need * 2 * kmers * (h - 1)
    assert 4 ** k * 1024 == 64 << 30  # config 3's rows of 1 KiB: 64 GiB


def test_model_rows_state_is_a_third_of_parts_12_and_exact():
    """one gather per k-mer under the sub-tile checks and the strand lead: the same passes over the same counts, a third of the lines"""
    rng = np.random.default_rng(5)
    for kind in ((None, 0.0), (0, 0.075), (1, 0.075), (1, 0.16)):
        r = model.read_lines(rng, kind)  # (asserts the maxima of the rows state against parts 1 and 2 itself)
        assert r["rows"] * model.H == r["12"], r
        assert r["rows"] < r["1234"] and r["max_1234"] == r["true_max"]


def test_model_today_state_calibrates_within_its_gate():
    """The extended model's `today` state against its measurement (15 698.1 TCC_EA0_RDREQ per read): within 0.2 %, the gate behind every
    figure the model predicts -- the rows state among them.  Through the model's own read_lines / run_strand, with the counts drawn per
    tile (a pass without sub-tile checks looks at tile boundaries only; Binomial(64, d^3) per bin and tile is what 64 draws per k-mer
    add up to).  Sample size: the per-read standard deviations of today's state are 0 (negatives), about 1 270 / 640 (positives
    forward / reverse) and 590 / 280 (the threshold-adjacent tenth); with the bench mix's weights the mean of n reads per kind has a
    standard error of 320 / sqrt(n) lines, 6.4 at n = 2 500, so the gate of 31.4 lines is 4.9 standard errors wide and a model that
    sits where the 500-read run of the full sampler put it (-0.05 %, 8 lines) passes with room for 3.6 of them."""
    today, off = model.calibration(per_kind=2500, seed=1)
    print("today's state: model %.1f, measured %.1f, %+.3f %%" % (today, model.MEASURED_TODAY, 100 * off))
    assert abs(off) <= model.GATE == 0.002, (today, off)
    # the per-tile draws and the per-k-mer draws are one model: same states where both exist, same deterministic negatives
    rng = np.random.default_rng(11)
    full = model.read_lines(rng, (None, 0.0))
    fast = model.read_lines(rng, (None, 0.0), only_today=True)
    assert full["today"] == fast["today"] == full["none"] == 16704
    pos_full = np.mean([model.read_lines(rng, (0, 0.075))["today"] for _ in range(12)])
    pos_fast = np.mean([model.read_lines(rng, (0, 0.075), only_today=True)["today"] for _ in range(600)])
    assert abs(pos_full - pos_fast) <= 4 * 1270 / np.sqrt(12), (pos_full, pos_fast)  # (the 12 full reads set the error: 4 of their standard errors)

"""Seeded differential fuzzing of the HIP path against the oracle over random filter geometries (bins, blocks,
k, h), read lengths and alphabets -- the corner cases nobody thought of listing."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import pyoracle as po
from readbouncer_amd import capi
from tests import helpers as H


# RB_FUZZ_SEEDS=<n> widens the sweep for an offline soak (profiles/r01/deep_parity.txt)
# n_rule: what the reverse strand holds for an N of the read -- 3 (T; ModComplementDna over a Dna5String, the default)
# or 4 (N).  Both candidates of that recalled SeqAn fact are fuzzed, kernels and oracle under the same rule.
@pytest.mark.parametrize("n_rule", [3, 4])
@pytest.mark.parametrize("seed", range(int(os.environ.get("RB_FUZZ_SEEDS", "24"))))
def test_random_geometry(seed, n_rule):
    prev = po.set_revcomp_of_n(n_rule)
    try:
        _random_geometry(seed, n_rule)
    finally:
        po.set_revcomp_of_n(prev)


def _random_geometry(seed, n_rule):
    rng = np.random.default_rng(1000 + seed)
    n_bins = int(rng.choice([1, 2, 63, 64, 65, 127, 128, 129, int(rng.integers(1, 9000)), int(rng.integers(1, 700))]))
    k = int(rng.choice([3, 5, 8, 11, 13, 15, 19, 27, 28, 32, int(rng.integers(3, 33))]))
    h = int(rng.choice([1, 2, 3, 3, 3, 4, 5, 8]))
    W = (n_bins + 63) // 64
    n_blocks = int(rng.choice([1, 2, 3, 64, 1000, 1024, int(rng.integers(1, 4000))]))
    if W * n_blocks > 4_000_000:
        n_blocks = max(1, 4_000_000 // W)
    n_bits = n_blocks * W * 64 + int(rng.integers(0, 64 * W))
    d = capi.DeviceIBF.create(0, n_bins, h, k, n_bits)
    if rng.random() < 0.5:
        d.fill_synth(int(rng.integers(1, 1 << 30)))
    ref = H.random_dna(rng, 5000, with_n=0.01)
    frag = int(rng.integers(max(k, 20), 2000))
    nfrag_bins = min(n_bins, 5000 // frag + 2)
    starts = (np.arange(nfrag_bins) * frag).astype(np.uint64)
    ends = np.minimum(starts + np.uint64(frag + k - 1), np.uint64(5000)).astype(np.uint64)
    ok = starts < 5000
    d.insert(ref, starts[ok], ends[ok], rng.integers(0, n_bins, size=int(ok.sum())).astype(np.uint64))
    host = d.download()
    o = po.OracleIBF.wrap(n_bins, h, k, n_bits, host.words())
    reads = []
    for i in range(60):
        L = int(rng.choice([0, 1, k - 1, k, k + 1, 63 + k, 64 + k, 65 + k, int(rng.integers(1, 700)), int(rng.integers(1, 1300))]))
        L = max(0, L)
        if i % 3 == 0:
            r = H.random_dna(rng, L, with_n=0.05)
        else:
            s = int(rng.integers(0, max(1, 5000 - L)))
            r = H.mutate(rng, ref[s:s + L], float(rng.choice([0.0, 0.05, 0.2])))
        if i % 7 == 0:
            r = r.lower()
        reads.append(r)
    buf, offs, lens = H.pack_reads(reads)
    exp_max = po.batch_raw_max(o, buf, offs, lens, 4)
    r_err = float(rng.choice([0.1, 0.05, 0.14]))
    exp_dec, exp_st = po.batch_check_unblock([o], [], buf, offs, lens, r=r_err, n_threads=4)
    eng = capi.Engine(0, [d], [])
    eng.set_revcomp_of_n(n_rule)
    for split in (2048, 0):
        eng.set_split_threshold(split)
        mc, _, dec, st = eng.classify(buf, offs, lens, error_rate=r_err)
        assert np.array_equal(mc[:, 0], exp_max), (n_bins, k, h, n_blocks, split)
        assert np.array_equal(dec, exp_dec) and np.array_equal(st, exp_st), (n_bins, k, h, n_blocks, split)
    # the opt-in early-decision mode on the throughput form (a call that asks for decisions only): same decisions, whatever the geometry
    # (builds without an early twin -- h != 3 -- count on as before)
    eng.set_early_decision(1)
    dec, st = eng.decide(buf, offs, lens, error_rate=r_err)
    eng.set_early_decision(0)
    assert np.array_equal(dec, exp_dec) and np.array_equal(st, exp_st), (n_bins, k, h, n_blocks, "early")
    # throughput form with clock-phased gathers (forced; serves blocks of one and two words with three hash functions)
    eng.set_phased(0, 1 << 40, int(rng.choice([0, 100, 1500])), int(rng.choice([1, 30])), 1)
    eng.set_phase_slices(1, int(rng.choice([2, 5, 8, 32])))  # as many slices as that, however small the table
    mc, _, dec, st = eng.classify(buf, offs, lens, error_rate=r_err)
    assert np.array_equal(mc[:, 0], exp_max), (n_bins, k, h, n_blocks, "phased")
    assert np.array_equal(dec, exp_dec) and np.array_equal(st, exp_st), (n_bins, k, h, n_blocks, "phased")
    eng.set_phased(0, 0, 0, 0, 0)
    # latency form with several workgroups per read (wide filters), on the batch and on a few reads of it (more parts)
    eng.set_split_threshold(2048)
    eng.set_split_parts(int(rng.choice([2, 3, 8, 16])), int(rng.choice([1, 2, 4, 8])))
    for n_sub in (len(reads), 7, 2):
        mc = eng.classify(buf, offs[:n_sub], lens[:n_sub], error_rate=r_err)[0]
        assert np.array_equal(mc[:, 0], exp_max[:n_sub]), (n_bins, k, h, n_blocks, "parts", n_sub)


SHORT_KERNELS = ("ibf_count_max_phased_kernel", "ibf_count_max_phased_multi_kernel")


# the same seeds and knob as test_random_geometry, on geometries that plan the short-read builds: every read of a batch has at most
# 256, 384 or 512 k-mers, the filter is narrow (1-256 bins, or a merged group of 2-4 narrow filters), three hash functions
@pytest.mark.parametrize("n_rule", [3, 4])
@pytest.mark.parametrize("seed", range(int(os.environ.get("RB_FUZZ_SEEDS", "24"))))
def test_random_short_read_geometry(seed, n_rule):
    prev = po.set_revcomp_of_n(n_rule)
    try:
        _random_short_read_geometry(seed, n_rule)
    finally:
        po.set_revcomp_of_n(prev)


def _random_short_read_geometry(seed, n_rule):
    rng = np.random.default_rng(5000 + seed)
    k = int(rng.integers(1, 33))
    n_blocks = int(rng.choice([1, 2, 3, 7, 64, 1021, 4096, 8191, int(rng.integers(1, 20000))]))
    if rng.random() < 0.3:
        # (more than 64 bins together: a merged copy of one word would take the merged kernel, not a short build)
        widths = [int(rng.integers(1, 65)) for _ in range(int(rng.integers(2, 5)))]
        while sum(widths) <= 64:
            widths[int(np.argmin(widths))] = 64
    else:
        widths = [int(rng.choice([1, 40, 64, 65, 100, 128, 129, 192, 193, 256, int(rng.integers(1, 257))]))]
    ref = H.random_dna(rng, 5000, with_n=0.01)
    filters, views, keep = [], [], []
    for i, bins in enumerate(widths):
        W = (bins + 63) // 64
        d = capi.DeviceIBF.create(0, bins, 3, k, n_blocks * W * 64 + int(rng.integers(0, 64 * W)))
        if rng.random() < 0.7:
            d.fill_synth(int(rng.integers(1, 1 << 30)))
        lo = int(rng.integers(0, 4000))
        d.add_sequence(ref[lo:lo + 1000], int(rng.integers(max(k, 20, 1000 // bins + 1), 1200)), 0, int(rng.integers(0, 300)))
        host = d.download()
        keep.append(host)
        views.append(po.OracleIBF.wrap(bins, 3, k, host.info["n_bits"], host.words()))
        filters.append(d)
    cap = int(rng.choice([256, 384, 512]))
    reads = []
    for i in range(int(rng.integers(1, 90))):
        L = int(rng.choice([0, 1, max(0, k - 1), k, k + 1, cap + k - 1, cap + k - 2, int(rng.integers(1, cap + k))]))
        if i % 3 == 0:
            r = H.random_dna(rng, L, with_n=0.05)
        else:
            s = int(rng.integers(0, max(1, 5000 - L)))
            r = H.mutate(rng, ref[s:s + L], float(rng.choice([0.0, 0.05, 0.2])))
            if i % 3 == 2:
                r = "".join("ACGTN"[x] for x in po.revcomp(po.encode(r)))
        if i % 7 == 0:
            r = r.lower()
        reads.append(r)
    buf, offs, lens = H.pack_reads(reads)
    assert int(lens.max()) - k + 1 <= cap  # every read within the cap: the short-read builds are what gets planned
    nd = 1 if (len(widths) == 1 and rng.random() < 0.5) else 0
    eng = capi.Engine(0, filters[:nd], filters[nd:])
    eng.set_merge(2)
    eng.set_revcomp_of_n(n_rule)
    eng.set_split_threshold(0)
    r_err = float(rng.choice([0.1, 0.05, 0.14]))
    exp_max = np.stack([po.batch_raw_max(v, buf, offs, lens, 4) for v in views], axis=1)
    exp_dec, exp_st = po.batch_check_unblock(views[:nd], views[nd:], buf, offs, lens, r=r_err, n_threads=4)
    for launch in range(3):
        ticks = int(rng.integers(1, 2001))
        skew = int(rng.integers(0, 4))
        rpw = int(rng.choice([0, 1, 2, 17, 18]))
        cut = int(rng.integers(0, 3))
        eng.set_phased(0, 1 << 40, ticks, 0, 1)
        eng.set_phase_xcd_skew(skew)
        eng.set_reads_per_wave(rpw)
        if cut == 0:
            eng.set_phase_equal_slices(0)
            eng.set_phase_slices(0, 32)  # the rule
            how = "rule"
        elif cut == 1:
            eng.set_phase_equal_slices(0)
            how = int(rng.integers(1, 24))
            eng.set_phase_slices(how, int(rng.choice([1, 3, 8, 32])))
        else:
            eng.set_phase_slices(0, 32)
            how = "equal %d" % int(rng.integers(2, 32))
            eng.set_phase_equal_slices(int(how.split()[1]))
        where = (widths, n_blocks, k, cap, ticks, skew, rpw, how)
        for fi in range(len(filters)):
            p = eng.plan(fi, len(lens), int(lens.max()))
            assert p["kernel"] in SHORT_KERNELS, (where, p)
        mc, _, dec, st = eng.classify(buf, offs, lens, error_rate=r_err)
        bad = np.nonzero((mc != exp_max).any(axis=1))[0]
        assert len(bad) == 0, (where, [(int(i), int(lens[i]), mc[i].tolist(), exp_max[i].tolist()) for i in bad[:5]])
        assert np.array_equal(dec, exp_dec) and np.array_equal(st, exp_st), where
    eng.destroy()
    for d in filters:
        d.free()

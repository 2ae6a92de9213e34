"""The same launch, again and again: the clock-phased count kernels choose the order in which they walk a table's slices by the wall
clock (s_memrealtime), so their results must not depend on when a wave runs.  For every LDS-offset shape, one register build and the
plain kernel on a wide filter: a batch of 32 768 reads resident on the device, the first launch against the oracle, then 200 launches
under a random window, XCD skew mode and slice cut each, every one compared in full with the first.

Stream discipline: torch zeroes the outputs on its own stream and the engine launches on its stream; torch.cuda.synchronize() between
the two (and after the engine) keeps the zeroing from racing the kernels -- the harness race of profiles/soak_determinism.py."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import pyoracle as po
from readbouncer_amd import capi
from tests import helpers as H

N_READS = 32768
LAUNCHES = 200
K = 13
TABLE_BYTES = 4 << 20  # several slices of the phased walk, few enough blocks for a quick oracle

# name: (bins of the deplete filters, bins of the (merged) targets, read length, reads per wave, kernel, phase shape name / build)
SHAPES = {
    "one-word, four tiles (LDS offsets)": ((64,), (), 250, 1, "ibf_count_max_phased_multi_kernel", "four tiles, one-word"),
    "one-word, six tiles (LDS offsets)": ((64,), (), 360, 1, "ibf_count_max_phased_multi_kernel", "six tiles, one-word"),
    "two-word, R = 1 (LDS offsets)": ((128,), (), 250, 1, "ibf_count_max_phased_multi_kernel", "four tiles, two-word"),
    "two-word, R = 2 (LDS offsets)": ((128,), (), 250, 2, "ibf_count_max_phased_multi_kernel", "four tiles, two-word"),
    "two-word, six tiles (LDS offsets)": ((128,), (), 360, 1, "ibf_count_max_phased_multi_kernel", "six tiles, two-word"),
    "merged pair, OR form (LDS offsets)": ((), (60, 50), 250, 1, "ibf_count_max_phased_multi_kernel", "four tiles, two-word"),
    "four-word, six tiles (LDS offsets)": ((256,), (), 360, 1, "ibf_count_max_phased_multi_kernel", "wide, rounds of three tiles (four-word build)"),
    "two-word, register build": ((128,), (), 250, 0, "ibf_count_max_phased_kernel", "four tiles, two-word"),
    "wide filter, plain kernel": ((1024,), (), 360, 1, "ibf_count_max_kernel", ""),
}


def _batch(rng, ref, L):
    """N_READS reads of up to L bases, L apart in one buffer: positives of both strands at error rates around the threshold's, random reads"""
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    ref_a = np.frombuffer(ref.encode(), dtype=np.uint8)
    starts = rng.integers(0, len(ref_a) - L, size=N_READS)
    R = ref_a[starts[:, None] + np.arange(L)[None, :]].copy()
    rate = rng.choice([0.0, 0.04, 0.07, 0.08, 0.09, 0.1, 0.12, 0.3], size=N_READS)[:, None]
    m = rng.random((N_READS, L)) < rate
    R[m] = acgt[rng.integers(0, 4, size=int(m.sum()))]
    rand = rng.random(N_READS) < 0.25
    R[rand] = acgt[rng.integers(0, 4, size=(int(rand.sum()), L))]
    comp = np.zeros(256, dtype=np.uint8)
    comp[list(b"ACGT")] = list(b"TGCA")
    flip = rng.random(N_READS) < 0.5
    R[flip] = comp[R[flip][:, ::-1]]
    nm = rng.random((N_READS, L)) < 0.002
    R[nm] = ord("N")
    lens = (L - rng.integers(0, 25, size=N_READS)).astype(np.uint32)
    offs = (np.arange(N_READS, dtype=np.uint64) * np.uint64(L))
    return R.reshape(-1), offs, lens


@pytest.mark.parametrize("name", list(SHAPES))
def test_repeated_launches_are_identical(name):
    torch = pytest.importorskip("torch")
    dep_bins, tgt_bins, L, rpw, kernel, shape = SHAPES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    ref = H.random_dna(rng, 60000)
    filters, views, keep = [], [], []
    for i, bins in enumerate(dep_bins + tgt_bins):
        W = (bins + 63) // 64
        stride = 1 << (W - 1).bit_length()
        n_blocks = TABLE_BYTES // (8 * stride) - 3 if not tgt_bins else TABLE_BYTES // 16 - 3  # (a merged pair: a two-word copy)
        d = capi.DeviceIBF.create(0, bins, 3, K, W * 64 * n_blocks)
        d.fill_synth(40 + i)
        d.add_sequence(ref[20000 * i:20000 * i + 30000], 30000 // bins + 1, 0, 200)
        host = d.download()
        keep.append(host)
        views.append(po.OracleIBF.wrap(bins, 3, K, host.info["n_bits"], host.words()))
        filters.append(d)
    nd = len(dep_bins)
    eng = capi.Engine(0, filters[:nd], filters[nd:])
    eng.set_merge(2)
    eng.set_split_threshold(0)
    eng.set_reads_per_wave(rpw)
    eng.set_phased(0, 1 << 40, 300, 0, 1)
    buf, offs, lens = _batch(rng, ref, L)
    nf = len(filters)
    p = eng.plan(0, N_READS, L)
    assert p["kernel"] == kernel and p["phase_shape_name"] == shape, (name, p)
    assert p["reserved0"] == (rpw if kernel == "ibf_count_max_phased_multi_kernel" else 0), (name, p)
    assert p["merged_members"] == len(tgt_bins) and (p["phased"] == 1) == bool(shape), (name, p)

    # the first launch against the oracle, on the whole batch; it holds reads within one k-mer of their threshold
    exp_mc = np.stack([po.batch_raw_max(v, buf, offs, lens, 16) for v in views], axis=1)
    exp_dec, exp_st = po.batch_check_unblock(views[:nd], views[nd:], buf, offs, lens, n_threads=16)
    thr_of = {int(n): po.threshold(int(n), K) for n in np.unique(lens)}
    thr = np.array([thr_of[int(n)] for n in lens], dtype=np.int64)
    assert (np.abs(exp_mc.astype(np.int64) - thr[:, None]) <= 1).sum() >= 20 and len(set(exp_dec.tolist())) >= 2
    dev = torch.device("cuda:0")
    t_buf, t_offs, t_lens = (torch.from_numpy(a.view(dt)).to(dev) for a, dt in ((buf, np.uint8), (offs, np.int64), (lens, np.int32)))
    mc = torch.zeros((N_READS, nf), dtype=torch.int16, device=dev)
    dec = torch.zeros(N_READS, dtype=torch.uint8, device=dev)
    st = torch.zeros(N_READS, dtype=torch.uint8, device=dev)

    def launch():
        mc.zero_()
        dec.zero_()
        st.zero_()
        torch.cuda.synchronize()  # the zeroing (torch's stream) is done before the engine's stream starts
        eng.classify_device(t_buf.data_ptr(), t_offs.data_ptr(), t_lens.data_ptr(), N_READS, L, d_maxcount=mc.data_ptr(),
                            d_decision=dec.data_ptr(), d_status=st.data_ptr())
        torch.cuda.synchronize()

    launch()
    got = mc.cpu().numpy().view(np.uint16)
    bad = np.nonzero((got != exp_mc).any(axis=1))[0]
    assert len(bad) == 0, (name, len(bad), [(int(i), got[i].tolist(), exp_mc[i].tolist()) for i in bad[:5]])
    assert np.array_equal(dec.cpu().numpy(), exp_dec) and np.array_equal(st.cpu().numpy(), exp_st), name
    first_mc, first_dec = mc.clone(), dec.clone()

    for i in range(LAUNCHES):
        ticks, skew = int(rng.integers(1, 2001)), int(rng.integers(0, 4))
        eng.set_phased(0, 1 << 40, ticks, 0, 1)
        eng.set_phase_xcd_skew(skew)
        cut = int(rng.integers(0, 3))
        if cut == 0:
            eng.set_phase_equal_slices(0)
            eng.set_phase_slices(0, 32)
            how = "rule"
        elif cut == 1:
            eng.set_phase_equal_slices(0)
            how = "2^%d bytes" % int(rng.integers(12, 23))
            eng.set_phase_slices(int(how[2:].split()[0]), 32)
        else:
            eng.set_phase_slices(0, 32)
            how = "%d equal" % int(rng.integers(2, 32))
            eng.set_phase_equal_slices(int(how.split()[0]))
        launch()
        if not (torch.equal(mc, first_mc) and torch.equal(dec, first_dec)):
            rows = ((mc != first_mc).any(dim=1) | (dec != first_dec)).nonzero().flatten()
            first = [(int(r), mc[r].tolist(), int(dec[r]), first_mc[r].tolist(), int(first_dec[r])) for r in rows[:5].tolist()]
            pytest.fail("%s: launch %d (window %d ticks, XCD skew %d, slices: %s) differs from the first in %d rows; "
                        "first (read, maxima, decision, expected maxima, expected decision): %s"
                        % (name, i + 1, ticks, skew, how, int(rows.numel()), first))
    eng.destroy()
    for d in filters:
        d.free()

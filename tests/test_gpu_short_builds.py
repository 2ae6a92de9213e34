"""The short-read builds of the phased count kernel against the oracle, at every k-mer size class and both N rules.

For narrow filters (one to four words per block) and batches whose longest read has at most 256 / 384 / 512 k-mers the engine takes
one of the one-lane short builds (ibf_count_max_phased_kernel: four tiles, six tiles, rounds, the wide builds) or, by default, one of the
LDS-offset builds (ibf_count_max_phased_multi_kernel<R, INV, T, NW>).  These compute k-mer values from staged base triples for k <= 13
and by 64-bit Horner above, in staging areas sized for a fixed number of bases.  Here every such build sees k from 3 to 32 -- triples
with k % 3 = 0, 1, 2, the last triple k (13), the first Horner k (14), the base-5 wrap above 27, the engine's maximum -- on batches whose
longest read sits exactly at a build boundary and one past it, and every launch is compared bit for bit with the oracle.  At the end
the test asserts that every build the launchers can select was reached, so that a planner change cannot make it test less unnoticed."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import pyoracle as po
from readbouncer_amd import capi
from tests import helpers as H

KS = (3, 8, 11, 12, 13, 14, 15, 19, 27, 28, 31, 32)
# what the reverse strand holds for an N of the read: 3 for half of the k values, 4 for the other half, both for 13 and 14
N_RULES = {3: (3,), 8: (4,), 11: (3,), 12: (4,), 13: (3, 4), 14: (3, 4), 15: (4,), 19: (3,), 27: (4,), 28: (3,), 31: (4,), 32: (3,)}
CASES = [(k, rule) for k in KS for rule in N_RULES[k]]
# longest read of a batch in k-mers: at the capacity of the four-tile, six-tile and rounds builds, and one past each
KMER_CAPS = (256, 257, 384, 385, 512, 513)
# reads per wave: 0 = the register builds, 1 / 2 = the LDS-offset builds (+ 16: the AND form on merged copies too)
READS_PER_WAVE = (0, 1, 2, 17, 18)
# filters on their own (bins, blocks): one, two, three (stride 4) and four words per block; Barrett and mask modulus
ALONE = ((40, 8111), (64, 8192), (100, 8209), (128, 4096), (130, 8219), (192, 4099), (200, 8231), (256, 8237))
# merged groups of narrow targets (members' bins, blocks): a two-, a three- and a four-word merged copy
GROUPS = (((60, 50), 8243), ((100, 60, 30), 8269), ((122, 43, 29, 49), 4093))

# every build of ibf_count_max_phased_multi_kernel<R, INV, T, NW> the launchers (rb_kernels.hip, launch_phased / dispatch_phased) can
# select, and every shape of the one-lane short builds of ibf_count_max_phased_kernel
EXPECTED_BUILDS = {
    "multi<R=1,AND,T=4,NW=1>", "multi<R=1,AND,T=6,NW=1>",
    "multi<R=1,AND,T=4,NW=2>", "multi<R=1,OR,T=4,NW=2>", "multi<R=2,AND,T=4,NW=2>", "multi<R=2,OR,T=4,NW=2>",
    "multi<R=1,AND,T=6,NW=2>", "multi<R=1,OR,T=6,NW=2>",
    "multi<R=1,AND,T=4,NW=4>", "multi<R=1,OR,T=4,NW=4>", "multi<R=1,AND,T=6,NW=4>", "multi<R=1,OR,T=6,NW=4>",
    "phased<four tiles, one-word>", "phased<six tiles, one-word>", "phased<rounds of three tiles, one-word>",
    "phased<four tiles, two-word>", "phased<six tiles, two-word>", "phased<rounds of four tiles, two-word>",
    "phased<wide, four tiles (four-word build)>", "phased<wide, four tiles (three-word build)>",
    "phased<wide, rounds of three tiles (four-word build)>", "phased<wide, rounds of three tiles (three-word build)>",
}

_reached = {}       # build -> set of (k, N rule) it ran at
_plans = set()      # the raw plan tuples behind them
_packed_done = set()
_cases_run = set()


def build_of(plan, reads_per_wave):
    """The kernel instantiation a plan stands for.  The plan tuple is (kernel, phase_shape_name, reserved0 = reads per wave of the
    multi build, block_words, stride_words, merged_members); the OR form is the merged copy's complemented twin, taken unless
    reads_per_wave carries + 16.  R, T and NW follow the launchers: six tiles and blocks of one, three or four words carry one read."""
    kernel, shape, r, words, stride, merged = plan
    if kernel == "ibf_count_max_phased_multi_kernel":
        nw = 1 if words == 1 else 2 if words == 2 else 4
        t = 4 if "four tiles" in shape else 6
        rr = r if (nw == 2 and t == 4) else 1
        form = "OR" if (merged and reads_per_wave < 16) else "AND"
        return "multi<R=%d,%s,T=%d,NW=%d>" % (rr, form, t, nw)
    if kernel == "ibf_count_max_phased_kernel":
        return "phased<%s>" % shape
    return kernel


def plan_tuple(eng, fi, n_reads, max_len):
    p = eng.plan(fi, n_reads, max_len)
    return (p["kernel"], p["phase_shape_name"], p["reserved0"], p["block_words"], p["stride_words"], p["merged_members"])


def make_filter(ref, bins, n_blocks, k, seed, lo):
    W = (bins + 63) // 64
    d = capi.DeviceIBF.create(0, bins, 3, k, W * 64 * n_blocks + (seed * 7) % (64 * W))
    assert d.info["n_blocks"] == n_blocks
    d.fill_synth(seed)
    d.add_sequence(ref[lo:lo + 8000], 8000 // min(bins, 40) + 1, 0, 200)
    host = d.download()
    return d, po.OracleIBF.wrap(host.info["n_bins"], 3, k, host.info["n_bits"], host.words()), host


def rc(s):
    return "".join("ACGTN"[x] for x in po.revcomp(po.encode(s)))


def short_batch(rng, ref, k, cap):
    """A batch whose longest read has exactly `cap` k-mers, with the edge reads every build must get right."""
    L = cap + k - 1
    reads = ["", "A", H.random_dna(rng, k - 1), ref[500:500 + k], "N" * L, ref[1000:1000 + L], rc(ref[9000:9000 + L]),
             ref[17000:17000 + L].lower(), H.mutate(rng, ref[25000:25000 + L], 0.03).lower()]
    for i in range(40):
        n = int(rng.integers(max(1, k - 1), L + 1))
        s = int(rng.integers(0, len(ref) - n))
        kind = i % 5
        if kind == 0:
            r = H.random_dna(rng, n, with_n=0.03)
        elif kind == 1:
            r = H.mutate(rng, ref[s:s + n], float(rng.choice([0.0, 0.02, 0.06])))
        elif kind == 2:
            r = rc(H.mutate(rng, ref[s:s + n], float(rng.choice([0.0, 0.02, 0.06]))))
        elif kind == 3:
            # the reverse strand of a reverse-complemented positive holds the reference's T where the read's A became N: under the
            # N rule 3 those k-mers hit, under 4 they miss -- counts that depend on the rule
            a = np.frombuffer(rc(ref[s:s + n]).encode(), dtype=np.uint8).copy()
            m = (a == ord("A")) & (rng.random(n) < 0.08)
            a[m] = ord("N")
            r = a.tobytes().decode()
        else:
            r = H.mutate(rng, ref[s:s + n], 0.04)
            if n > 2:
                p = int(rng.integers(0, n - 1))
                r = r[:p] + "n" + r[p + 1:].lower()
        reads.append(r)
    if len(reads) % 2 == 0:  # the last wave of a two-reads-per-wave build has one read too few
        reads.append(ref[30000:30000 + L])
    assert max(len(r) for r in reads) == L and len(reads) % 2 == 1
    return reads


def slice_setting(eng, i):
    """Window and slice cut for launch i: slices of 2^n bytes as small as max_slices allows, or equal slices."""
    ticks = (1, 150, 300, 2000, 700)[(i + i // 5) % 5]
    eng.set_phased(0, 1 << 40, ticks, 0, 1)
    if i % 3 == 2:
        eng.set_phase_slices(0, 32)
        eng.set_phase_equal_slices((3, 7, 31)[(i // 3) % 3])
    else:
        eng.set_phase_equal_slices(0)
        eng.set_phase_slices(1, (8, 32, 1, 3)[i % 4])


@pytest.mark.parametrize("k,n_rule", CASES)
def test_short_builds_match_oracle(k, n_rule):
    torch = pytest.importorskip("torch")
    prev = po.set_revcomp_of_n(n_rule)
    try:
        _short_builds(torch, k, n_rule)
    finally:
        po.set_revcomp_of_n(prev)
    _cases_run.add((k, n_rule))


def _short_builds(torch, k, n_rule):
    rng = np.random.default_rng(100 * k + n_rule)
    ref = H.random_dna(rng, 40000)
    alone = [make_filter(ref, b, nb, k, 11 + i, (i * 4000) % 30000) for i, (b, nb) in enumerate(ALONE)]
    grouped = []
    for gi, (members, nb) in enumerate(GROUPS):
        for j, b in enumerate(members):
            grouped.append(make_filter(ref, b, nb, k, 50 + 10 * gi + j, (gi * 9000 + j * 3000) % 30000))
    # engine A: the filters on their own, half deplete, half target (decisions depend on k through the thresholds)
    eng_a = capi.Engine(0, [x[0] for x in alone[:4]], [x[0] for x in alone[4:]])
    # engine B: the merged groups (set_merge(2): every group of one hash geometry is merged)
    eng_b = capi.Engine(0, [], [x[0] for x in grouped])
    eng_b.set_merge(2)
    engines = ((eng_a, [x[1] for x in alone], 4), (eng_b, [x[1] for x in grouped], 0))
    for eng, _, _ in engines:
        eng.set_revcomp_of_n(n_rule)
        eng.set_split_threshold(0)
    dev = torch.device("cuda:0")
    launch = 0
    for cap in KMER_CAPS:
        reads = short_batch(rng, ref, k, cap)
        buf, offs, lens = H.pack_reads(reads)
        L = int(lens.max())
        packed, p_off, nmask, n_off = capi.pack_reads(buf, offs, lens)
        for eng, views, nd in engines:
            exp = np.stack([po.batch_raw_max(v, buf, offs, lens, 8) for v in views], axis=1)
            exp_dec, exp_st = po.batch_check_unblock(views[:nd], views[nd:], buf, offs, lens, n_threads=8)
            assert exp.max() > 50, "the planted reads do not hit"
            for rpw in READS_PER_WAVE:
                eng.set_reads_per_wave(rpw)
                slice_setting(eng, launch)
                launch += 1
                plans = [plan_tuple(eng, fi, len(lens), L) for fi in range(len(views))]
                builds = [build_of(p, rpw) for p in plans]
                mc, _, dec, st = eng.classify(buf, offs, lens)
                where = (k, n_rule, cap, rpw, launch, builds)
                bad = np.nonzero((mc != exp).any(axis=1))[0]
                assert len(bad) == 0, (where, [(int(i), int(lens[i]), mc[i].tolist(), exp[i].tolist()) for i in bad[:5]])
                assert np.array_equal(dec, exp_dec) and np.array_equal(st, exp_st), where
                for p, b in zip(plans, builds):
                    _plans.add(p)
                    _reached.setdefault(b, set()).add((k, n_rule))
                # packed 2-bit + N input through the same builds, once per build
                if any(b not in _packed_done for b in builds):
                    t = lambda a, dt: torch.from_numpy(a.view(dt)).to(dev)
                    t_pk, t_po, t_nm, t_no, t_lens = t(packed, np.uint8), t(p_off, np.int64), t(nmask, np.uint8), t(n_off, np.int64), t(lens, np.int32)
                    t_mc = torch.zeros((len(lens), len(views)), dtype=torch.int16, device=dev)
                    torch.cuda.synchronize()
                    eng.classify_device_ex(t_pk.data_ptr(), t_po.data_ptr(), t_lens.data_ptr(), len(lens), L, d_nmask=t_nm.data_ptr(),
                                           d_nmask_offsets=t_no.data_ptr(), d_maxcount=t_mc.data_ptr())
                    torch.cuda.synchronize()
                    got = t_mc.cpu().numpy().view(np.uint16)
                    assert np.array_equal(got, exp), (where, "packed input")
                    _packed_done.update(builds)
    assert eng_b.merge_info()[0] == len(GROUPS)
    for eng, _, _ in engines:
        eng.destroy()
    for d, _, _ in alone + grouped:
        d.free()


def test_every_short_build_was_reached():
    """Coverage of the matrix above: every build in EXPECTED_BUILDS ran (and matched) at least once, and each of them also took packed
    input.  A planner change that stops routing a batch to a build makes this fail instead of silently testing less."""
    if _cases_run != set(CASES):
        pytest.skip("runs after the whole matrix of test_short_builds_match_oracle")
    reached = {b: sorted(v) for b, v in _reached.items()}
    missing = EXPECTED_BUILDS - set(reached)
    assert not missing, ("builds never reached", sorted(missing), "reached", reached, sorted(_plans))
    assert EXPECTED_BUILDS <= _packed_done, ("builds never given packed input", sorted(EXPECTED_BUILDS - _packed_done))
    # the multi builds ran at every k and both N rules (the k-mer values of both code paths, triples and Horner)
    for b in EXPECTED_BUILDS:
        ks = {k for k, _ in _reached[b]}
        assert ks == set(KS), (b, sorted(set(KS) - ks))
    print("reached builds:\n  " + "\n  ".join(sorted(reached)))


# Packed block numbers of the LDS-offset builds (rb_device.h, kPackMaxBlocks / kPackMaxBlocks1): the largest tables they take, and the
# first block count the planner refuses them -- those fall back to the register builds and still count exactly.
PACK_MAX, PACK_MAX1 = (1 << 21) - 2, (1 << 22) - 2
LIMIT_TABLES = [((128,), PACK_MAX), ((256,), PACK_MAX), ((130,), PACK_MAX), ((64,), PACK_MAX1),
                ((128,), PACK_MAX + 1), ((256,), PACK_MAX + 1), ((64,), PACK_MAX1 + 1)]


def _looked_up_blocks(view, reads, k):
    """(block numbers of every forward k-mer of the reads, those of the third hash function) as the oracle computes them"""
    blocks, third = [], []
    for r in reads:
        o = po.encode(r)
        for p in range(len(o) - k + 1):
            v = po.kmer_value(o[p:p + k], k)
            for h in range(3):
                b = view.block_index(v, h)
                blocks.append(b)
                if h == 2:
                    third.append(b)
    return np.array(blocks, dtype=np.uint64), np.array(third, dtype=np.uint64)


def _sentinel_reads(rng, view, k, n_blocks, want, test):
    """random k-mers whose block numbers satisfy test(block numbers of the three hashes) -- planted where random reads do not reach"""
    out = []
    while len(out) < want:
        s = H.random_dna(rng, 64 + k)
        o = po.encode(s)
        for p in range(64):
            v = po.kmer_value(o[p:p + k], k)
            if test([view.block_index(v, h) for h in range(3)]):
                out.append(s[p:p + k])
                break
    return out


@pytest.mark.parametrize("k", [13, 14, 27])
@pytest.mark.parametrize("widths,n_blocks", LIMIT_TABLES)
def test_packed_block_number_limits(widths, n_blocks, k):
    """Tables at the top of the packed range (2^21 - 2 blocks of two, three and four words: 32 / 64 / 64 MiB; 2^22 - 2 one-word blocks)
    through the LDS-offset builds, and one block more through the register builds the planner falls back to.  The batch really looks
    up block numbers within 64 of the table's end, and on one-word tables third-hash numbers of 2^20 and more (non-zero spill bits)."""
    bins = widths[0]
    limit = PACK_MAX1 if bins <= 64 else PACK_MAX
    rng = np.random.default_rng(n_blocks + 7 * k + bins)
    ref = H.random_dna(rng, 40000)
    d, view, _host = make_filter(ref, bins, n_blocks, k, 5 + k, 1000)
    eng = capi.Engine(0, [d], [])
    eng.set_split_threshold(0)
    eng.set_phased(0, 1 << 40, 300, 0, 1)
    eng.set_phase_slices(1, 32)
    top = lambda bs: max(bs) >= n_blocks - 64
    spill = lambda bs: bs[2] >= (1 << 20)
    for cap in (256, 384):
        reads = short_batch(rng, ref, k, cap)
        sentinels = _sentinel_reads(rng, view, k, n_blocks, 4, top)
        if bins <= 64:
            sentinels += _sentinel_reads(rng, view, k, n_blocks, 4, spill)
        # each sentinel k-mer inside a read of the batch, and once inserted into a bin so that it is a hit there
        reads += [H.random_dna(rng, 20) + s + H.random_dna(rng, 30) for s in sentinels]
        d.insert("".join(sentinels), np.arange(len(sentinels), dtype=np.uint64) * k, np.arange(1, len(sentinels) + 1, dtype=np.uint64) * k,
                 np.full(len(sentinels), 3, dtype=np.uint64))
        host = d.download()
        view = po.OracleIBF.wrap(host.info["n_bins"], 3, k, host.info["n_bits"], host.words())
        blocks, third = _looked_up_blocks(view, reads[-len(sentinels):], k)
        assert (blocks >= n_blocks - 64).any() and blocks.max() < n_blocks
        if bins <= 64:
            assert (third >= (1 << 20)).any()
        buf, offs, lens = H.pack_reads(reads)
        exp = po.batch_raw_max(view, buf, offs, lens, 8)
        exp_dec, exp_st = po.batch_check_unblock([view], [], buf, offs, lens, n_threads=8)
        for rpw in (1, 2, 0):
            eng.set_reads_per_wave(rpw)
            p = eng.plan(0, len(lens), int(lens.max()))
            if rpw and n_blocks <= limit:
                assert p["kernel"] == "ibf_count_max_phased_multi_kernel", p
            else:  # beyond the packed range: the register build of the same shape
                assert p["kernel"] == "ibf_count_max_phased_kernel" and p["phase_shape_name"], p
            mc, _, dec, st = eng.classify(buf, offs, lens)
            bad = np.nonzero(mc[:, 0] != exp)[0]
            assert len(bad) == 0, (widths, n_blocks, k, cap, rpw, [(int(i), int(mc[i, 0]), int(exp[i])) for i in bad[:5]])
            assert np.array_equal(dec, exp_dec) and np.array_equal(st, exp_st), (widths, n_blocks, k, cap, rpw)
    eng.destroy()
    d.free()

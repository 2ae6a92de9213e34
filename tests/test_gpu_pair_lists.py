"""The pair table of a resident filter (rb_dibf_pair_table_build) and the pair form of the plain count kernel
(ibf_count_pair_lists_kernel, RB_ROW_TABLE_PAIRS): per N-free k-mer x ONE slot of three lines with the bins of row(x) and of row(rc(x)),
counted into one LDS dword per bin -- low half forward strand, high half reverse strand.  None of that may change a result.  Every slot,
decoded as the kernel reads it (tail lines and dense rows followed), is compared with the AND of the oracle's blocks for x and rc(x);
classify calls under PAIRS are compared bit for bit -- raw maxima, decisions, status -- with the oracle; policy and lifecycle are read
through rb_engine_plan and rb_dibf_pair_table_info.  k = 5, 6 and 7 keep the tables at 4^5 - 4^7 slots."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import pyoracle as po
from readbouncer_amd import capi
from tests import helpers as H
from tests import pair_lists_rig as PR
from tests import row_lists_rig as LR
from tests import test_gpu_row_lists as RL
from tests import test_gpu_row_table as RT

PAIRS_KERNEL, LISTS_KERNEL, ROWS_KERNEL, PLAIN_KERNEL = "ibf_count_pair_lists_kernel", RL.LISTS_KERNEL, RT.ROWS_KERNEL, RT.PLAIN_KERNEL
OFF, AUTO, LISTS, PAIRS = capi.RB_ROW_TABLE_OFF, capi.RB_ROW_TABLE_AUTO, capi.RB_ROW_TABLE_LISTS, capi.RB_ROW_TABLE_PAIRS
rc = PR.revcomp
# 8192 bins at design load want blocks to spare: with about a thousand, six pairs in a thousand hold a row of two coinciding blocks (378
# bins: dense rows), six times the census's cap -- and at k = 5 the cap is ONE of the 1024 slots, which a single such pair passes (it
# has two slots): 65 521 blocks leave 0.05 such pairs to expect.  At 4090 bins such a row is 189 bins, at the edge of slot + tail, and
# 16 381 blocks keep them few; at 2112 bins it is 97 bins and fits the slot, so a thousand blocks serve.
GEOMETRIES = ((8192, PR.CRAFT_BLOCKS), (4090, PR.SPARE_BLOCKS), (2112, 1021))


def check(eng, batch, ref, label, want_kernel=PAIRS_KERNEL, repeats=2):
    buf, offs, lens = batch
    p = eng.plan(0, len(lens), int(lens.max()))
    assert p["kernel"] == want_kernel, (label, p)
    if want_kernel == PAIRS_KERNEL:
        assert p["row_table_bytes"] > 0 and p["column_slices"] == 1
    for rep in range(repeats):
        mc, _, dec, st = eng.classify(buf, offs, lens)
        bad = np.nonzero((mc != ref[0]).any(axis=1))[0]
        assert len(bad) == 0, (label, rep, [(int(i), int(lens[i]), mc[i].tolist(), ref[0][i].tolist()) for i in bad[:6]])
        assert np.array_equal(dec, ref[1]) and np.array_equal(st, ref[2]), (label, rep, "decision/status")
    return p


def pairs_engine(d, nt=0, mode=PAIRS):
    return RT.engine(d, mode, nt)


# ---------------------------------------------------------------- the table itself, slot by slot
def slots_equal_pairs(d, o, k, n_blocks, n_bins):
    info = d.pair_table_build()
    assert info["refused"] == 0 and info["rows"] == 4 ** k and info["lines"] == 3, (info["refused"], info["census_rows"], info["census_over"])
    assert info["bytes"] == 4 ** k * 384 and info["side_rows"] <= info["side_capacity"] and info["tail_rows"] <= info["tail_capacity"]
    slots, tails, side = d.pair_table_download()
    assert len(tails) == info["tail_rows"] and len(side) == info["side_rows"]
    wantA, wantB = PR.expected_pairs(o, k, n_blocks, n_bins)
    A, B, kind = PR.decode_slots(slots, tails, side, n_bins)
    assert np.array_equal(A, wantA) and np.array_equal(B, wantB)
    assert np.array_equal(kind, PR.kind_of(wantA.sum(axis=1), wantB.sum(axis=1)))  # a pair leaves the slot exactly when it does not fit
    assert info["census_rows"] == min(4 ** k, 65536)
    assert info["census_over"][0] == int((kind != PR.PLAIN).sum()) and info["census_over"][1] == int((kind == PR.DENSE).sum())
    return info, kind


@pytest.mark.parametrize("n_bins,n_blocks", GEOMETRIES)
@pytest.mark.parametrize("k", (5, 6, 7))
def test_slots_are_the_pairs_of_the_oracles_rows(k, n_bins, n_blocks):
    """k = 6: sixty-four palindromic k-mers, whose slot holds the same list twice"""
    d, o = RT.device_filter(n_bins, n_blocks, 3, k, seed=k * 100 + 3)
    info, kind = slots_equal_pairs(d, o, k, n_blocks, n_bins)
    if k == 6:
        slots, _, _ = d.pair_table_download()
        pal = np.nonzero(PR.rc_ranks(k) == np.arange(4 ** k))[0]
        assert len(pal) == 64
        for r in pal[kind[pal] == PR.PLAIN]:
            nA = int(np.nonzero(slots[r] == PR.SENTINEL)[0][0])
            assert np.array_equal(slots[r, :nA], slots[r, nA + 1:2 * nA + 1])
    d.free()


# ---------------------------------------------------------------- classify: pairs == the oracle
@pytest.fixture(scope="module")
def planted():
    rng = np.random.default_rng(79)
    return rng, H.random_dna(rng, 6000)


@pytest.mark.parametrize("nt", (0, 1))
@pytest.mark.parametrize("n_bins,n_blocks", GEOMETRIES + ((4091, PR.SPARE_BLOCKS),))
@pytest.mark.parametrize("k", (5, 6, 7))
def test_classify_pairs_equal_the_oracle(planted, k, n_bins, n_blocks, nt):
    """bin 0, a middle bin and the last bin (of an odd bin count at 4091) are planted; N at the first base, in the middle, at the last
    base, on the reverse strand, everywhere (read_shapes): the twin's reads; reads on either strand, so that the maximum lies on the
    reverse strand alone for some"""
    rng, ref = planted
    plant = [(ref[i * 2000:(i + 1) * 2000], b) for i, b in enumerate((0, n_bins // 2 + 5, n_bins - 1))]
    d, o = RT.device_filter(n_bins, n_blocks, 3, k, seed=9, plant=plant)
    reads = RT.read_shapes(rng, ref, (40, 70, 71, 354, 1100)) + [rc(ref[4100:4460]), rc(ref[100:460]), ref[2100:2460]]
    batch = H.pack_reads(reads)
    eng = pairs_engine(d, nt)
    for n_rule in (3, 4):
        expected = RT.reference(o, batch, n_rule)
        eng.set_revcomp_of_n(n_rule)
        for prune in (1, 0):  # accepted, and changes nothing
            eng.set_bound_pruning(prune)
            p = check(eng, batch, expected, ("pairs", k, n_bins, n_rule, prune))
        assert p["nontemporal"] == nt
    info = d.pair_table_info()
    assert info["builds"] == 1 and info["lines"] == 3, info
    eng.destroy(), d.free()


def test_strands_of_1_to_71_kmers(planted):
    rng, ref = planted
    k = 7
    d, o = RT.device_filter(8192, PR.SPARE_BLOCKS, 3, k, seed=12, plant=[(ref[:2000], 8191), (ref[2000:4000], 0)])
    reads = [ref[300:300 + k - 1 + n] for n in range(1, 72)] + [rc(ref[2300:2300 + k - 1 + n]) for n in range(1, 72)] + [ref[:k - 1], "A"]
    batch = H.pack_reads(reads)
    eng = pairs_engine(d)
    check(eng, batch, RT.reference(o, batch), "1..71")
    eng.destroy(), d.free()


# ---------------------------------------------------------------- crafted pairs: the edges of a slot, of slot + tail, and balance
@pytest.fixture(scope="module")
def crafted():
    made = {}

    def edit(w, host):
        made["c"] = PR.CraftedPairs(8192, host.words(), host.info["n_bits"])

    d, _ = RL.uploaded(8192, PR.CRAFT_BLOCKS, PR.CraftedPairs.K, edit, seed=5)
    yield d, made["c"]
    d.free()


def test_crafted_pairs_at_the_edges_of_slot_tail_and_dense_rows(crafted):
    d, c = crafted
    info = d.pair_table_build()
    assert info["refused"] == 0, info
    slots, tails, side = d.pair_table_download()
    A, B, kind = PR.decode_slots(slots, tails, side, 8192)
    for r, rr, (nA, nB), want in zip(c.ranks, c.rc_ranks, c.PAIRS, c.kinds()):
        assert (A[r].sum(), B[r].sum(), kind[r]) == (nA, nB, want), (r, nA, nB)
        assert (A[rr].sum(), B[rr].sum(), kind[rr]) == (nB, nA, want), (rr, nA, nB)  # the pair's second slot, under rc(x)
    assert c.kinds() == [PR.PLAIN, PR.PLAIN, PR.PLAIN, PR.TAIL, PR.TAIL, PR.DENSE, PR.PLAIN, PR.PLAIN]
    assert info["tail_rows"] >= 4 and info["side_rows"] >= 4  # two tail pairs and one dense pair, each under x and under rc(x)
    batch = H.pack_reads(c.reads())
    expected = RT.reference(c.o, batch)
    for nt in (0, 1):
        eng = pairs_engine(d, nt)
        check(eng, batch, expected, ("crafted", nt))
        eng.destroy()


def test_one_long_list_beside_a_short_one_stays_on_the_hot_path():
    """nA = 128 with nB = 10, the mirror, and the full slot 96 + 96 alone in a filter with blocks to spare: no tail line, no dense row"""
    made = {}

    class Balanced(PR.CraftedPairs):
        KMERS = PR.CraftedPairs.KMERS[:3]
        PAIRS = ((128, 10), (10, 128), (96, 96))

    def edit(w, host):
        made["c"] = Balanced(8192, host.words(), host.info["n_bits"])

    d, _ = RL.uploaded(8192, PR.CRAFT_BLOCKS, Balanced.K, edit, seed=6)
    c = made["c"]
    info = d.pair_table_build()
    slots, tails, side = d.pair_table_download()
    A, B, kind = PR.decode_slots(slots, tails, side, 8192)
    assert [int(kind[r]) for r in c.ranks + c.rc_ranks] == [PR.PLAIN] * 6
    wantA, wantB = PR.expected_pairs(c.o, c.K, PR.CRAFT_BLOCKS, 8192)
    flagged = int((PR.kind_of(wantA.sum(axis=1), wantB.sum(axis=1)) != PR.PLAIN).sum())
    assert info["tail_rows"] + info["side_rows"] // 2 == flagged  # the info call's counters: the crafted slots are not among them
    ks = list(c.KMERS)
    batch = H.pack_reads(ks + [rc(s) for s in ks] + [a + b for a in ks for b in ks if a != b] + ["".join(ks) * 20])
    eng = pairs_engine(d)
    check(eng, batch, RT.reference(c.o, batch), "balanced")
    eng.destroy(), d.free()


def test_reads_silent_on_both_strands():
    made = {}

    def edit(w, host):
        made["o"] = LR.silence(8192, PR.SPARE_BLOCKS, host.words(), host.info["n_bits"])

    d, _ = RL.uploaded(8192, PR.SPARE_BLOCKS, LR.K, edit, seed=7)
    batch = H.pack_reads(LR.silent_reads())
    expected = RT.reference(made["o"], batch)
    assert not expected[0].any()
    eng = pairs_engine(d)
    check(eng, batch, expected, "silent")
    eng.destroy(), d.free()


# ---------------------------------------------------------------- counter edges: both halves of one dword at 0xFFFF
def test_one_bin_at_0xffff_on_both_strands_and_the_max_len_boundary():
    """SAT (set in every block) counts every k-mer of a read on both strands: at 65 535 k-mers both halves of its dword are 0xFFFF and
    its neighbours' dwords 0 -- a carry would show in one of them.  One base more and the pair form does not serve."""
    k, n_bins, n_blocks = 7, 2112, 1021
    sat = 1001

    def edit(w, host):
        w[:] = 0
        w[:, sat // 64] = np.uint64(1) << np.uint64(sat % 64)

    d, o = RL.uploaded(n_bins, n_blocks, k, edit)
    rng = np.random.default_rng(3)
    long_read = H.random_dna(rng, k + 65534)
    eng = pairs_engine(d)
    batch = H.pack_reads([long_read, long_read[:k + 65533], long_read[:1000]])
    expected = RT.reference(o, batch)
    assert expected[0][:, 0].tolist() == [65535, 65534, 1000 - k + 1]
    check(eng, batch, expected, "0xFFFF", repeats=1)
    slots, tails, side = d.pair_table_download()
    A, B, kind = PR.decode_slots(slots, tails, side, n_bins)
    assert A.sum(axis=1).tolist() == [1] * 4 ** k and B[:, sat].all() and not kind.any()
    over = H.pack_reads([long_read + "A"])
    assert eng.plan(0, 1, k + 65535)["kernel"] != PAIRS_KERNEL
    mc, _, _, _ = eng.classify(*over)
    assert int(mc[0, 0]) == po.batch_raw_max(o, *over, 8)[0]
    eng.destroy(), d.free()


# ---------------------------------------------------------------- engines, lifecycle, policy
def test_two_filter_engine_with_a_narrow_filter_beside(planted):
    rng, ref = planted
    k = 7
    d, o = RT.device_filter(8192, PR.SPARE_BLOCKS, 3, k, seed=13, plant=[(ref[:2000], 5)])
    narrow, on = RT.device_filter(128, 4093, 3, k, seed=14, plant=[(ref[2000:4000], 100)])
    eng = capi.Engine(0, [d, narrow], [])
    eng.set_split_threshold(0)
    eng.set_row_table(PAIRS)
    batch = H.pack_reads(RT.read_shapes(rng, ref, (70, 354)))
    buf, offs, lens = batch
    assert eng.plan(0, len(lens), int(lens.max()))["kernel"] == PAIRS_KERNEL
    assert eng.plan(1, len(lens), int(lens.max()))["kernel"] != PAIRS_KERNEL
    mc, _, dec, st = eng.classify(buf, offs, lens)
    assert np.array_equal(mc[:, 0], po.batch_raw_max(o, buf, offs, lens, 8)) and np.array_equal(mc[:, 1], po.batch_raw_max(on, buf, offs, lens, 8))
    wdec, wst = po.batch_check_unblock([o, on], [], buf, offs, lens, n_threads=8)
    assert np.array_equal(dec, wdec) and np.array_equal(st, wst)
    eng.destroy(), d.free(), narrow.free()


def test_an_insert_drops_the_table_and_the_next_call_rebuilds_it(planted):
    rng, ref = planted
    d, o = RT.device_filter(8192, PR.SPARE_BLOCKS, 3, 7, seed=15)
    read = ref[2500:2854]
    batch = H.pack_reads([read, rc(read), ref[100:460]])
    eng = pairs_engine(d)
    check(eng, batch, RT.reference(o, batch), "before")
    assert d.pair_table_info()["builds"] == 1
    d.insert(ref[2000:4000], [0], [2000], [4242])
    info = d.pair_table_info()
    assert info["bytes"] == 0 and info["builds"] == 1, info
    expected = RT.reference(RT.oracle_view(d), batch)
    assert expected[0][0, 0] == len(read) - 7 + 1
    check(eng, batch, expected, "after")
    assert d.pair_table_info()["builds"] == 2
    eng.destroy(), d.free()


def test_refusals_are_remembered_per_version_of_the_bits(planted):
    """a filter at a bit load of 0.5: every pair needs dense rows, the census refuses, the call takes the list rule (refused as well:
    the row kernel), and no later call asks again until the bits change"""
    rng, ref = planted
    d, o = RL.uploaded(4096, 1021, 7, RL.random_load(0.5, seed=1))
    eng = pairs_engine(d)
    batch = H.pack_reads([ref[100:460], rc(ref[500:860])])
    expected = RT.reference(o, batch)
    assert eng.plan(0, 2, 360)["kernel"] == PAIRS_KERNEL  # before the census
    buf, offs, lens = batch
    for rep in range(2):
        mc, _, dec, st = eng.classify(buf, offs, lens)
        assert np.array_equal(mc, expected[0]) and np.array_equal(dec, expected[1]) and np.array_equal(st, expected[2])
        info = d.pair_table_info()
        assert info["refused"] == capi.RB_LIST_REFUSED_DENSITY and info["builds"] == 0 and info["bytes"] == 0, info
        assert info["census_over"][1] > info["census_rows"] // 1024
        assert eng.plan(0, 2, 360)["kernel"] != PAIRS_KERNEL
    d.insert(ref[:100], [0], [100], [1])
    assert eng.plan(0, 2, 360)["kernel"] == PAIRS_KERNEL  # new bits: the question is open again
    eng.destroy(), d.free()


def test_a_traced_call_plans_the_list_kernel(planted):
    torch = pytest.importorskip("torch")
    rng, ref = planted
    d, o = RT.device_filter(8192, PR.SPARE_BLOCKS, 3, 7, seed=16)
    eng = pairs_engine(d)
    assert eng.plan(0, 4, 360)["kernel"] == PAIRS_KERNEL
    trace = torch.zeros(64, dtype=torch.int64, device="cuda")
    eng.set_prune_trace(trace.data_ptr())
    assert eng.plan(0, 4, 360)["kernel"] == LISTS_KERNEL
    batch = H.pack_reads([ref[100:460], rc(ref[500:860])])
    check(eng, batch, RT.reference(o, batch), "traced", LISTS_KERNEL, repeats=1)
    assert d.pair_table_info()["builds"] == 0 and d.list_table_info()["builds"] == 1
    eng.set_prune_trace(0)
    assert eng.plan(0, 4, 360)["kernel"] == PAIRS_KERNEL
    eng.destroy(), d.free()


def test_auto_takes_the_pair_table_from_pair_min_bytes_on(planted):
    """the same small filter under AUTO: with the default of 1 GiB its pair table (6 MiB) is too small and the list kernel is planned;
    with pair_min_bytes 0 the pair kernel, and the call builds the pair table and no list table"""
    rng, ref = planted
    k, L = 7, 360
    d, o = RT.device_filter(8192, PR.SPARE_BLOCKS, 3, k, seed=17, plant=[(ref[:2000], 9)])
    eng = RT.engine(d, AUTO)
    eng.set_list_min_dense_bytes(0)
    n = 2000  # repays either build: 51 reads repay the pair table's, 33 the list table's
    assert eng.plan(0, n, L)["kernel"] == LISTS_KERNEL
    eng.set_pair_min_bytes(0)
    assert eng.plan(0, n, L)["kernel"] == PAIRS_KERNEL
    assert eng.plan(0, 10, L)["kernel"] == PLAIN_KERNEL  # a batch that repays nothing
    reads = [ref[i:i + L] for i in range(0, 4000, 40)] + [rc(ref[i:i + L]) for i in range(0, 4000, 40)]
    reads = (reads * (n // len(reads) + 1))[:n]
    batch = H.pack_reads(reads)
    buf, offs, lens = batch
    mc, _, dec, st = eng.classify(buf, offs, lens)
    want = po.batch_raw_max(o, *H.pack_reads(reads[:200]), 8)
    assert np.array_equal(mc[:200, 0], want) and np.array_equal(mc[200:400, 0], want)
    pi, li = d.pair_table_info(), d.list_table_info()
    assert pi["builds"] == 1 and li["builds"] == 0 and pi["census_one_line"] > pi["census_rows"] // 1024 >= pi["census_over"][2], (pi, li)
    eng.destroy(), d.free()

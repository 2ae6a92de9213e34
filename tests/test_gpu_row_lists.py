"""The list table of a resident filter (rb_dibf_list_table_build) and the list form of the plain count kernel (ibf_count_lists_kernel,
RB_ROW_TABLE_LISTS): per N-free k-mer the sorted bin numbers of its row -- the AND of its h blocks -- in a slot of 1, 2 or 4 lines,
gathered instead of the row's 8 lines and counted with one LDS add per listed bin.  None of that may change a result.  Every slot,
decoded as the kernel reads it (overflow slots followed into the side table), is compared with the AND of the oracle's blocks; classify
calls under LISTS are compared bit for bit -- raw maxima, decisions, status -- with the oracle and with the modes OFF and FORCE; policy
and lifecycle are read through rb_engine_plan and rb_dibf_list_table_info.  k = 5 and 7 keep the tables at 4^5 - 4^7 slots."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import pyoracle as po
from readbouncer_amd import capi
from tests import helpers as H
from tests import pass_edges as PE
from tests import row_lists_rig as LR
from tests import row_rig as RR
from tests import test_gpu_row_table as RT

LISTS_KERNEL, ROWS_KERNEL, PLAIN_KERNEL = "ibf_count_lists_kernel", RT.ROWS_KERNEL, RT.PLAIN_KERNEL
OFF, AUTO, FORCE, LISTS = capi.RB_ROW_TABLE_OFF, capi.RB_ROW_TABLE_AUTO, capi.RB_ROW_TABLE_FORCE, capi.RB_ROW_TABLE_LISTS
K = LR.K
rc = PE.revcomp_str


def uploaded(n_bins, n_blocks, k, edit, seed=None, h=3):
    """a resident filter whose words `edit(words[n_blocks, W], info)` has written on the host (after fill_synth(seed) when given)"""
    W = (n_bins + 63) // 64
    d = capi.DeviceIBF.create(0, n_bins, h, k, W * 64 * n_blocks)
    if seed is not None:
        d.fill_synth(seed)
    host = d.download()
    edit(host.words()[:n_blocks * W].reshape(n_blocks, W), host)
    d.free()
    d = capi.DeviceIBF.upload(0, host)
    o = po.OracleIBF.wrap(n_bins, h, k, host.info["n_bits"], host.words())
    o._host = host
    return d, o


def random_load(load, seed):
    def edit(w, host):
        rng = np.random.default_rng(seed)
        bits = rng.random((w.shape[0], w.shape[1] * 64)) < load
        bits[:, host.info["n_bins"]:] = False
        w[:] = np.packbits(bits, axis=1, bitorder="little").view(np.uint64)
    return edit


def check(eng, batch, ref, label, want_kernel, repeats=2):
    buf, offs, lens = batch
    p = eng.plan(0, len(lens), int(lens.max()))
    assert p["kernel"] == want_kernel, (label, p)
    if want_kernel == LISTS_KERNEL:
        assert p["row_table_bytes"] > 0 and p["column_slices"] == 1
    for rep in range(repeats):
        mc, _, dec, st = eng.classify(buf, offs, lens)
        bad = np.nonzero((mc != ref[0]).any(axis=1))[0]
        assert len(bad) == 0, (label, rep, [(int(i), int(lens[i]), mc[i].tolist(), ref[0][i].tolist()) for i in bad[:6]])
        assert np.array_equal(dec, ref[1]) and np.array_equal(st, ref[2]), (label, rep, "decision/status")
    return p


def lists_engine(d, nt=0, mode=LISTS):
    return RT.engine(d, mode, nt)


# ---------------------------------------------------------------- the table itself, slot by slot
def slots_equal_rows(d, o, k, n_blocks, n_bins, want_lines=None):
    info = d.list_table_build()
    assert info["refused"] == 0 and info["rows"] == 4 ** k and info["lines"] in (1, 2, 4), info
    assert info["bytes"] == 4 ** k * info["lines"] * 128 and info["side_rows"] <= info["side_capacity"]
    if want_lines:
        assert info["lines"] == want_lines, info
    slots, side = d.list_table_download()
    assert slots.shape == (4 ** k, 64 * info["lines"]) and side.shape[0] == info["side_rows"]
    want = LR.row_bits(LR.expected_rows(o, k, 3, n_blocks), n_bins)
    got, over = LR.decode_slots(slots, side, n_bins)
    assert np.array_equal(got, want)
    assert np.array_equal(over, want.sum(axis=1) > 64 * info["lines"])  # a row overflows exactly when it does not fit
    assert info["census_rows"] == min(4 ** k, 65536)
    for i in range(3):
        assert info["census_over"][i] == int((want.sum(axis=1) > (64 << i)).sum())  # (every row was looked at)
    return info, int(over.sum())


@pytest.mark.parametrize("n_bins", (4096, 8192))
@pytest.mark.parametrize("n_blocks", (1024, 1021))
@pytest.mark.parametrize("k", (5, 7))
def test_slots_are_the_and_of_the_oracles_blocks(k, n_blocks, n_bins):
    """With about a thousand blocks, three k-mers in a thousand have two of their three block numbers equal: their rows are the AND of
    two blocks (d^2 of the bins, not d^3), far more than one row in 1024, so THEY set the slot size -- four lines -- and the filter
    must be sparse enough for them to fit it: 4096 bins at design load (189 bins in such a row), 8192 bins at a bit load of 0.15 (184).
    The rows whose three block numbers coincide overflow four lines as well and go to the side table."""
    if n_bins == 4096:
        d, o = RT.device_filter(n_bins, n_blocks, 3, k, seed=k * 100 + 3)
    else:
        d, o = uploaded(n_bins, n_blocks, k, random_load(0.15, seed=15))
    info, n_over = slots_equal_rows(d, o, k, n_blocks, n_bins, want_lines=4)
    assert n_over >= 1
    d.free()


@pytest.mark.parametrize("n_bins,lines", ((4096, 1), (8192, 2)))
def test_slots_at_design_load_with_blocks_to_spare(n_bins, lines):
    """16 381 blocks (LR.SPARE_BLOCKS): the rows of coinciding block numbers are three in 16 384 and no longer decide; 40 / 81 bins per row take one / two lines"""
    d, o = RT.device_filter(n_bins, LR.SPARE_BLOCKS, 3, K, seed=9)
    info, n_over = slots_equal_rows(d, o, K, LR.SPARE_BLOCKS, n_bins, want_lines=lines)
    assert 1 <= n_over <= 16
    d.free()


@pytest.mark.parametrize("n_bins", (4090, 8192))
def test_slots_of_a_denser_filter_and_its_overflow_rows(n_bins):
    """bit load 0.17 (0.24 at 4090 bins, whose last word has pad bits): the two-block rows lie around 236 bins and some pass 256"""
    d, o = uploaded(n_bins, 1021, K, random_load(0.17 if n_bins == 8192 else 0.24, seed=n_bins))
    info, n_over = slots_equal_rows(d, o, K, 1021, n_bins, want_lines=4)
    assert info["side_rows"] == n_over >= 1
    d.free()


# ---------------------------------------------------------------- classify: lists == force == off == oracle
@pytest.fixture(scope="module")
def planted():
    rng = np.random.default_rng(78)
    return rng, H.random_dna(rng, 6000)


@pytest.mark.parametrize("nt", (0, 1))
@pytest.mark.parametrize("n_bins,n_blocks,load,lines", ((4096, LR.SPARE_BLOCKS, None, 1), (8192, LR.SPARE_BLOCKS, None, 2), (4090, 1021, None, 4),
                                                        (8192, 1021, 0.17, 4)))
def test_classify_lists_equal_force_off_and_the_oracle(planted, n_bins, n_blocks, load, lines, nt):
    rng, ref = planted
    plant = [(ref[i * 2000:(i + 1) * 2000], b) for i, b in enumerate((3, n_bins // 2 + 5, n_bins - 1))]
    if load is None:
        d, o = RT.device_filter(n_bins, n_blocks, 3, K, seed=9, plant=plant)
    else:
        d, _ = uploaded(n_bins, n_blocks, K, random_load(load, seed=n_bins))
        for seq, b in plant:
            d.insert(seq, [0], [len(seq)], [b])
        o = RT.oracle_view(d)
    # N at the first base, in the middle, at the last base, on the reverse strand, everywhere (read_shapes): the twin's reads
    batch = H.pack_reads(RT.read_shapes(rng, ref, (40, 70, 71, 354, 1100)))
    engines = {mode: RT.engine(d, mode, nt) for mode in (OFF, FORCE, LISTS)}
    for n_rule in (3, 4):
        expected = RT.reference(o, batch, n_rule)
        for eng in engines.values():
            eng.set_revcomp_of_n(n_rule)
        check(engines[OFF], batch, expected, ("off", n_bins, n_rule), PLAIN_KERNEL, repeats=1)
        check(engines[FORCE], batch, expected, ("force", n_bins, n_rule), ROWS_KERNEL, repeats=1)
        for prune in (1, 0):
            engines[LISTS].set_bound_pruning(prune)
            p = check(engines[LISTS], batch, expected, ("lists", n_bins, n_rule, prune), LISTS_KERNEL)
        assert p["nontemporal"] == nt
    info = d.list_table_info()
    assert info["lines"] == lines and info["builds"] == 1, info  # with p["nontemporal"] above: the parameters ARE the six list builds
    for eng in engines.values():
        eng.destroy()
    d.free()


def test_reads_with_n_are_written_by_the_twin_only(planted):
    """a batch of reads with an N alone, on a filter whose LIST table is rubbish for them anyway (k-mers with an N have no slot): the
    result is the oracle's, under both N rules"""
    rng, ref = planted
    d, o = RT.device_filter(8192, LR.SPARE_BLOCKS, 3, K, seed=21, plant=[(ref[:2000], 77)])
    pos = ref[100:454]
    reads = ["N" + pos[1:], pos[:-1] + "N", pos[:177] + "N" + pos[178:], rc("N" + pos[1:]), "N" * 354, pos[:6] + "N" + pos[7:], "N" + pos[1:K]]
    batch = H.pack_reads(reads)
    eng = lists_engine(d)
    for n_rule in (3, 4):
        eng.set_revcomp_of_n(n_rule)
        check(eng, batch, RT.reference(o, batch, n_rule), ("N only", n_rule), LISTS_KERNEL)
    eng.destroy(), d.free()


# ---------------------------------------------------------------- crafted rows: 0, cap - 1, cap, cap + 1 and every bin
@pytest.mark.parametrize("n_bins,lines", ((2112, 1), (8192, 2)))  # (33 words at design load: 21 bins per row)
def test_crafted_rows_at_the_edges_of_a_slot(n_bins, lines):
    made = {}

    def edit(w, host):
        made["c"] = LR.Crafted(n_bins, lines, host.words(), host.info["n_bits"])

    d, _ = uploaded(n_bins, LR.CRAFT_BLOCKS, K, edit, seed=5)
    c = made["c"]
    info = d.list_table_build()
    assert info["refused"] == 0 and info["lines"] == lines, info
    slots, side = d.list_table_download()
    got, over = LR.decode_slots(slots, side, n_bins)
    for rank, m in zip(c.ranks, c.want):
        assert got[rank].sum() == m and over[rank] == (m > c.cap), (rank, m)
        assert (slots[rank, 0] == LR.OVERFLOW_MARK) if m > c.cap else ((slots[rank] < LR.OVERFLOW_MARK).sum() == m)
    batch = H.pack_reads(c.reads())
    expected = RT.reference(c.o, batch)
    assert expected[0][:5, 0].tolist() == [1, 1, 1, 1, 1]  # the chosen k-mers alone: SAT (the empty row's on its reverse strand only)
    for nt in (0, 1):
        eng = lists_engine(d, nt)
        check(eng, batch, expected, ("crafted", n_bins, nt), LISTS_KERNEL)
        eng.destroy()
    eng = lists_engine(d, mode=FORCE)
    check(eng, batch, expected, ("crafted, dense rows", n_bins), ROWS_KERNEL, repeats=1)
    eng.destroy(), d.free()


@pytest.mark.parametrize("n_bins,n_blocks,load,lines", ((2112, LR.CRAFT_BLOCKS, None, 1), (8192, LR.CRAFT_BLOCKS, None, 2), (8192, 1021, 0.15, 4)))
def test_reads_that_hit_nothing_count_zero(n_bins, n_blocks, load, lines):
    """reads of k-mers whose rows are empty on BOTH strands (LR.silence) in a filter with no saturated bin: the maximum is 0 with n > 0,
    so a slot's sentinels must add nothing to it -- no other read can tell, since any hit at all already makes the maximum 1"""
    made = {}

    def edit(w, host):
        if load is not None:
            random_load(load, seed=15)(w, host)
        made["o"] = LR.silence(n_bins, n_blocks, host.words(), host.info["n_bits"])

    d, owner = uploaded(n_bins, n_blocks, K, edit, seed=5 if load is None else None)  # (`owner` keeps the words that `o` looks at)
    o = made["o"]
    info = d.list_table_build()
    assert info["refused"] == 0 and info["lines"] == lines, info
    slots, _ = d.list_table_download()
    for s in LR.SILENT_KMERS:
        assert (slots[LR.kmer_rank(s)] == LR.SENTINEL).all() and (slots[LR.kmer_rank(LR.revcomp(s))] == LR.SENTINEL).all()
    batch = H.pack_reads(LR.silent_reads())
    expected = RT.reference(o, batch)
    assert not expected[0].any() and int(batch[2].min()) >= K  # nothing is hit, and every read has a k-mer
    for nt in (0, 1):
        eng = lists_engine(d, nt)
        for prune in (1, 0):
            eng.set_bound_pruning(prune)
            check(eng, batch, expected, ("silent", n_bins, nt, prune), LISTS_KERNEL, repeats=1)
        eng.destroy()
    d.free()


# ---------------------------------------------------------------- counter edges (the constructions of tests/pass_edges.py at k = 7)
def edge_filter(n_bins):
    def edit(w, host):
        rng = np.random.default_rng(n_bins)
        for b, load in ((n_bins - 1, 2.0), (PE.NEAR, 0.99), (PE.LOW, 0.5)):
            w[:, b // 64] |= (rng.random(w.shape[0]) < load).astype(np.uint64) << np.uint64(b % 64)
    return uploaded(n_bins, 1021, K, edit)


@pytest.mark.parametrize("n_bins", (4090, 8192))
def test_counter_edges_under_lists(n_bins):
    """SAT counts every k-mer on both strands: 1023 / 1024 is where the twin's planes switch and means nothing to 16-bit counters; a batch
    that declares 65 536 k-mers or more is beyond them and takes the dense row form"""
    d, o = edge_filter(n_bins)
    engines = [lists_engine(d, nt) for nt in (0, 1)]
    for which in PE.BATCHES:
        reads, kmers = PE.batch(which, K)
        batch = H.pack_reads(list(reads))
        expected = RT.reference(o, batch)
        for n, got in zip(kmers, expected[0][:, 0]):
            if n is not None and n < 65536:
                assert got == n  # SAT
        want = LISTS_KERNEL if int(batch[2].max()) - K + 1 < 65536 else ROWS_KERNEL
        assert want == (ROWS_KERNEL if which == "BIG" else LISTS_KERNEL)
        for nt, eng in enumerate(engines):
            check(eng, batch, expected, (n_bins, which, nt), want, repeats=1)
    # the boundary itself, one read per call: 65 535 k-mers is the last strand the lists count, 65 536 goes to the dense rows
    S = PE.sequence()
    for n, want in ((65535, LISTS_KERNEL), (65536, ROWS_KERNEL)):
        batch = H.pack_reads([S[:n + K - 1]])
        expected = RT.reference(o, batch)
        assert (expected[0][0, 0] == n) == (n == 65535)  # SAT; at 65 536 it has wrapped to 0 and NEAR is the maximum
        check(engines[0], batch, expected, (n_bins, n), want, repeats=1)
    for eng in engines:
        eng.destroy()
    d.free()


# ---------------------------------------------------------------- pruning and strand order
def test_pruning_fixtures_and_where_the_strands_stop():
    """the crossover and tile-edge plants of tests/row_rig.py at k = 7 on a sparse filter (one line per slot): results with the bound on
    and off, and the trace of the list kernel -- a second strand that is skipped, one that stops on a tile edge short of its end, one
    that is counted to the end because it is the positive one"""
    torch = pytest.importorskip("torch")
    plants = RR.pruning_plants(k=K)
    d = RR.BP.make_filter(8192, k=K)
    for name in ("cross", "edges"):
        plants[name].insert_into(d)
    # three reads of 256 k-mers on a stretch of their own: all of it (the forward strand reaches n), its reverse complement (the reverse
    # strand is the positive one), and 200 k-mers of it before a random tail (the reverse strand, a handful of chance hits, cannot pass
    # 200 once 196 or fewer k-mers are left: it stops at k-mer 64, a tile edge)
    rng = np.random.default_rng(256)
    own = H.random_dna(rng, 256 + K - 1)
    d.insert(own, [0], [len(own)], [4321])
    mine = [own, rc(own), own[:200 + K - 1] + H.random_dna(rng, 56)]
    o = RT.oracle_view(d)
    eng = lists_engine(d)
    seen = dict(skipped=0, tile_edge=0, reverse_wins=0)
    for name in ("cross", "edges"):
        reads = mine + list(plants[name].items)
        reads += [rc(r) for r in reads[3:43]]
        batch = H.pack_reads(reads)
        expected = RT.reference(o, batch)
        eng.set_bound_pruning(0)
        check(eng, batch, expected, (name, "no bound"), LISTS_KERNEL, repeats=1)
        eng.set_bound_pruning(1)
        t = torch.zeros(len(reads), dtype=torch.int64, device="cuda:0")
        torch.cuda.synchronize()
        eng.set_prune_trace(t.data_ptr())
        check(eng, batch, expected, (name, "bound"), LISTS_KERNEL, repeats=1)
        torch.cuda.synchronize()
        eng.set_prune_trace(None)
        r = t.cpu().numpy().view(np.uint64)
        n = np.maximum(batch[2].astype(np.int64) - K + 1, 0)
        stop_fwd, stop_rev = ((r >> np.uint64(16)) & np.uint64(0xFFFF)).astype(np.int64), ((r >> np.uint64(32)) & np.uint64(0xFFFF)).astype(np.int64)
        assert ((r >> np.uint64(15)) & np.uint64(1)).all() and np.array_equal(stop_fwd, n)  # the first strand is always counted whole
        assert ((stop_rev % 64 == 0) | (stop_rev == n)).all()                               # a stop is a tile edge
        fwd = np.array([int(o.count(po.encode(x)).max()) if len(x) >= K else 0 for x in reads])
        assert np.array_equal(stop_rev[(fwd >= n) & (n > 0)], np.zeros(int(((fwd >= n) & (n > 0)).sum())))  # reached n: no second strand
        assert stop_rev[0] == 0 and stop_rev[1] == 256 and fwd[1] < 128 and expected[0][1, 0] == 256 and fwd[2] >= 200 and stop_rev[2] == 64, (
            stop_rev[:3].tolist(), fwd[:3].tolist())
        seen["skipped"] += int(((fwd >= n) & (n > 0)).sum())
        seen["tile_edge"] += int(((stop_rev > 0) & (stop_rev < n)).sum())
        seen["reverse_wins"] += int(((expected[0][:, 0] > fwd) & (stop_rev == n)).sum())
    assert min(seen.values()) > 0, seen
    eng.destroy(), d.free()


# ---------------------------------------------------------------- policy, refusals, lifecycle
def test_auto_keeps_the_row_form_below_the_size_rule_and_takes_lists_above(planted):
    rng, ref = planted
    d, o = RT.device_filter(8192, LR.SPARE_BLOCKS, 3, K, seed=13, plant=[(ref[:2000], 9)])
    L = 360
    eng = capi.Engine(0, [d], [])  # auto is the default
    eng.set_split_threshold(0)
    need_rows = RR.rule_b_need(K, 3, L)
    assert eng.plan(0, need_rows, L)["kernel"] == ROWS_KERNEL and eng.plan(0, 1 << 24, L)["kernel"] == ROWS_KERNEL  # 16 MiB of dense rows: cache-served
    eng.set_list_min_dense_bytes(0)
    # rule (c) in lines: items x 2 x k-mers x (8 h - 4) >= 4^k x (8 h + 4)
    need = -(-(4 ** K * 28) // (2 * (L - K + 1) * 20))
    assert need < need_rows
    assert eng.plan(0, need - 1, L)["kernel"] == PLAIN_KERNEL and eng.plan(0, need, L)["kernel"] == LISTS_KERNEL
    big = H.pack_reads([H.random_dna(rng, L) for _ in range(need)] + [ref[100:100 + L], "N" + ref[101:100 + L]])
    ref_big = RT.reference(o, big)
    check(eng, big, ref_big, "auto, lists", LISTS_KERNEL)
    assert d.list_table_info()["builds"] == 1 and d.row_table_info()["builds"] == 0
    small = H.pack_reads([ref[100:100 + L]])
    check(eng, small, RT.reference(o, small), "auto, a current list table has nothing to repay", LISTS_KERNEL, repeats=1)
    eng.set_early_decision(1)
    assert eng.plan(0, need, L)["kernel"] == PLAIN_KERNEL
    eng.set_early_decision(0)
    eng.set_list_min_dense_bytes(512 << 20)
    # (the size rule again: lists are out, and this batch is below the row table's rule (b))
    check(eng, big, ref_big, "auto, the size rule back", PLAIN_KERNEL, repeats=1)
    assert eng.plan(0, need_rows, L)["kernel"] == ROWS_KERNEL
    # the three modes give the same outputs
    outs = []
    for mode in (OFF, FORCE, LISTS):
        eng.set_row_table(mode)
        outs.append(eng.classify(*big))
    for other in outs[1:]:
        assert all(np.array_equal(a, b) for a, b in zip(outs[0], other))
    eng.destroy(), d.free()


def test_a_dense_filter_is_refused_and_falls_back(planted):
    rng, ref = planted
    d, o = uploaded(8192, 1021, K, random_load(0.6, seed=60))  # 0.6^3 x 8192 = 1770 bins per row
    info = d.list_table_build()
    assert info["refused"] == capi.RB_LIST_REFUSED_DENSITY and info["bytes"] == 0 and info["builds"] == 0, info
    assert info["census_over"][2] > info["census_rows"] >> 10
    batch = H.pack_reads(RT.read_shapes(rng, ref, (70, 354)))
    expected = RT.reference(o, batch)
    eng = lists_engine(d)
    check(eng, batch, expected, "lists refused: dense rows", ROWS_KERNEL)  # (the plan knows the refusal of these bits)
    assert d.list_table_info()["builds"] == 0 and d.row_table_info()["builds"] == 1
    eng.set_row_table(AUTO)
    eng.set_list_min_dense_bytes(0)
    assert eng.plan(0, 1 << 24, 354)["kernel"] == ROWS_KERNEL  # a batch that would repay either table: the refused one is not planned
    check(eng, batch, expected, "auto after the refusal, a small batch", PLAIN_KERNEL, repeats=1)
    eng.destroy(), d.free()


def test_a_refusal_for_want_of_room_stands_and_the_plan_says_what_the_call_does(planted):
    """two-line slots of 4^7 rows are 4 MiB and a side table: an engine that allows tables 3 MiB -- room for one-line slots, which is all
    the policy can know before the census -- is refused after it, and from then on neither the call nor the plan asks again until the
    engine allows more or the table is dropped"""
    rng, ref = planted
    d, o = RT.device_filter(8192, LR.SPARE_BLOCKS, 3, K, seed=13, plant=[(ref[:2000], 9)])
    batch = H.pack_reads(RT.read_shapes(rng, ref, (70, 354)))
    expected = RT.reference(o, batch)
    eng = capi.Engine(0, [d], [])
    eng.set_split_threshold(0)
    eng.set_row_table(LISTS, 3 << 20)
    n, L = len(batch[2]), int(batch[2].max())
    assert eng.plan(0, n, L)["kernel"] == LISTS_KERNEL  # nothing is known of the bits yet
    mc, _, dec, st = eng.classify(*batch)
    assert np.array_equal(mc, expected[0]) and np.array_equal(dec, expected[1]) and np.array_equal(st, expected[2])
    info = d.list_table_info()
    assert info["refused"] == capi.RB_LIST_REFUSED_MAX_BYTES and info["builds"] == 0 and info["census_over"][0] > info["census_rows"] >> 10 >= info["census_over"][1], info
    check(eng, batch, expected, "refused for its size: 16 MiB of dense rows are beyond 3 MiB as well", PLAIN_KERNEL)
    assert d.list_table_info()["refused"] == capi.RB_LIST_REFUSED_MAX_BYTES and d.row_table_info()["builds"] == 0
    d.list_table_drop()
    assert d.list_table_info()["refused"] == capi.RB_LIST_REFUSED_NONE and eng.plan(0, n, L)["kernel"] == LISTS_KERNEL  # dropped: may ask again
    eng.classify(*batch)  # asks again, and is refused again
    assert d.list_table_info()["refused"] == capi.RB_LIST_REFUSED_MAX_BYTES and eng.plan(0, n, L)["kernel"] == PLAIN_KERNEL
    eng.set_row_table(LISTS, 8 << 20)  # room for the lists, still none for the dense rows
    check(eng, batch, expected, "more room", LISTS_KERNEL)
    assert d.list_table_info()["builds"] == 1 and d.list_table_info()["lines"] == 2
    eng.destroy(), d.free()


def test_a_full_side_table_refuses_the_build():
    d, o = uploaded(8192, 1021, K, random_load(0.17, seed=8192))  # (the filter of the overflow test: a few rows beyond four lines)
    try:
        capi.set_list_side_capacity(1)
        info = d.list_table_build()
        assert info["refused"] == capi.RB_LIST_REFUSED_SIDE_FULL and info["bytes"] == 0, info
        capi.set_list_side_capacity(0)
        info = d.list_table_build()
        assert info["refused"] == 0 and 1 < info["side_rows"] <= info["side_capacity"] == 4 ** K // 512 + 64, info
    finally:
        capi.set_list_side_capacity(0)
    d.free()
    k14 = capi.DeviceIBF.create(0, 8192, 3, 14, 128 * 64 * 1021)
    assert k14.list_table_build()["refused"] == capi.RB_LIST_REFUSED_K
    k14.free()
    for bins in (2048, 8200):
        f = capi.DeviceIBF.create(0, bins, 3, K, ((bins + 63) // 64) * 64 * 1021)
        assert f.list_table_build()["refused"] == capi.RB_LIST_REFUSED_GEOMETRY
        e = lists_engine(f)
        if bins == 8200:
            assert e.plan(0, 1 << 20, 360)["kernel"] == ROWS_KERNEL  # two column slices: the dense rows
        e.destroy(), f.free()


def test_an_insert_drops_the_table_and_the_next_call_rebuilds_it(planted):
    torch = pytest.importorskip("torch")
    rng, ref = planted
    d, o = RT.device_filter(4096, LR.SPARE_BLOCKS, 3, K, seed=11)
    read = ref[2500:2854]
    batch = H.pack_reads([read, H.random_dna(rng, 354), rc(read)])
    e1, e2 = lists_engine(d), lists_engine(d)
    before = RT.reference(o, batch)
    check(e1, batch, before, "before the insert", LISTS_KERNEL, repeats=1)
    check(e2, batch, before, "second engine", LISTS_KERNEL, repeats=1)
    assert d.list_table_info()["builds"] == 1  # two engines, one table
    d.insert(read, [0], [len(read)], [1234])
    assert d.list_table_info()["bytes"] == 0 and d.list_table_info()["builds"] == 1
    after = RT.reference(RT.oracle_view(d), batch)
    assert after[0][0, 0] == len(read) - K + 1 > before[0][0, 0]
    check(e2, batch, after, "after the insert", LISTS_KERNEL, repeats=1)
    assert d.list_table_info()["builds"] == 2 and d.list_table_info()["bytes"] == 4 ** K * 128
    check(e1, batch, after, "after the insert, first engine", LISTS_KERNEL, repeats=1)
    assert d.list_table_info()["builds"] == 2
    d.list_table_drop()
    assert d.list_table_info()["bytes"] == 0
    e1.destroy(), e2.destroy()
    d.list_table_build()
    torch.cuda.synchronize()
    free_with = torch.cuda.mem_get_info(0)[0]
    d.free()
    assert torch.cuda.mem_get_info(0)[0] >= free_with + 4 ** K * 128  # the table went with the filter


def test_a_list_counted_filter_beside_a_narrow_one(planted):
    rng, ref = planted
    wide, ow = RT.device_filter(8192, LR.SPARE_BLOCKS, 3, K, seed=31, plant=[(ref[:2000], 8191)])
    narrow, on = RT.device_filter(300, 1021, 3, K, seed=32, plant=[(ref[2000:4000], 7)])
    reads = RT.read_shapes(rng, ref, (70, 354))
    batch = H.pack_reads(reads)
    eng = capi.Engine(0, [wide], [narrow])
    eng.set_split_threshold(0)
    eng.set_row_table(LISTS)
    assert eng.plan(0, len(reads), 354)["kernel"] == LISTS_KERNEL and eng.plan(1, len(reads), 354)["row_table_bytes"] == 0
    raw = np.stack([po.batch_raw_max(ow, *batch, 8), po.batch_raw_max(on, *batch, 8)], axis=1)
    dec, st = po.batch_check_unblock([ow], [on], *batch, n_threads=8)
    for rep in range(2):
        mc, _, got_dec, got_st = eng.classify(*batch)
        assert np.array_equal(mc, raw) and np.array_equal(got_dec, dec) and np.array_equal(got_st, st), rep
    assert wide.list_table_info()["builds"] == 1 and narrow.list_table_info()["builds"] == 0
    eng.destroy(), wide.free(), narrow.free()

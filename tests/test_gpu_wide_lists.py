"""The WIDE list table of a resident filter (rb_dibf_wide_list_table_build) and the wide list form of the plain count kernel
(ibf_count_wide_lists_kernel, rb_engine_set_wide_lists): filters of 8193 to 32 256 bins counted from slots of 4, 6 or 8 lines, one
workgroup of four waves per read.  None of that may change a result.  Every slot of the downloaded table is compared with the AND of
the oracle's blocks; classify calls under BUILD are compared bit for bit -- raw maxima, decisions, status -- with the oracle; policy and
lifecycle are read through rb_engine_plan and rb_dibf_wide_list_table_info.  The fixtures are tests/wide_lists_rig.py's, whose claims
tests/test_wide_lists_cpu.py checks on the oracle alone.  k = 5 and 7 keep the tables at 4^5 - 4^7 slots, the filters at a few MB."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import pyoracle as po
from readbouncer_amd import capi
from tests import helpers as H
from tests import test_gpu_row_table as RT
from tests import wide_lists_rig as WR

WIDE_KERNEL, LISTS_KERNEL = "ibf_count_wide_lists_kernel", "ibf_count_lists_kernel"
OFF, CURRENT, BUILD = capi.RB_PASS_LISTS_OFF, capi.RB_PASS_LISTS_CURRENT, capi.RB_PASS_LISTS_BUILD
K = WR.K
REACHED = set()  # (lines, non-temporal) of the wide launches the tests made: the closing test wants all six builds


def upload(o):
    """the oracle's words as a resident filter"""
    W, n_blocks = o.bin_width, o.n_blocks
    d = capi.DeviceIBF.create(0, o.n_bins, o.n_hash, o.kmer_size, W * 64 * n_blocks)
    host = d.download()
    host.words()[:n_blocks * W] = o.words()[:n_blocks * W]
    d.free()
    return capi.DeviceIBF.upload(0, host)


def engine(filters, mode, nt=0):
    eng = capi.Engine(0, list(filters), [])
    eng.set_split_threshold(0)  # small batches in the throughput form
    eng.set_nt_threshold(0 if nt else RT.NT_NEVER)
    if mode is not None:
        eng.set_wide_lists(mode)
    return eng


def check(eng, batch, ref, label, want_kernel=None, fi=0, repeats=2):
    buf, offs, lens = batch
    p = eng.plan(fi, len(lens), int(lens.max()))
    if want_kernel:
        assert p["kernel"] == want_kernel, (label, p)
    if p["kernel"] == WIDE_KERNEL:
        assert p["row_table_bytes"] > 0 and p["column_slices"] == 1
    for rep in range(repeats):
        mc, _, dec, st = eng.classify(buf, offs, lens)
        bad = np.nonzero(mc[:, fi] != ref[0][:, 0])[0]
        assert len(bad) == 0, (label, rep, [(int(i), int(lens[i]), int(mc[i, fi]), int(ref[0][i, 0])) for i in bad[:8]])
        if mc.shape[1] == 1:
            assert np.array_equal(dec, ref[1]) and np.array_equal(st, ref[2]), (label, rep, "decision/status")
    return p


# ---------------------------------------------------------------- the table itself, slot by slot
@pytest.mark.parametrize("name", [n for n, f in WR.FILTERS.items() if f[4]])
def test_slots_are_the_and_of_the_oracles_blocks(name):
    n_bins, k, _, _, lines = WR.FILTERS[name]
    o = WR.table_fixture(name)
    d = upload(o)
    info = d.wide_list_table_build()
    assert info["refused"] == 0 and info["rows"] == 4 ** k and info["lines"] == lines and info["builds"] == 1, info
    assert info["bytes"] == 4 ** k * lines * 128 and info["side_rows"] <= info["side_capacity"] == 4 ** k // 512 + 64
    assert d.list_table_build()["refused"] == capi.RB_LIST_REFUSED_GEOMETRY  # the list table still refuses what the wide one serves
    slots, side = d.wide_list_table_download()
    assert slots.shape == (4 ** k, 64 * lines) and side.shape[0] == info["side_rows"]
    rows = WR.expected_rows(o)
    pc = WR.populations(rows)
    over = WR.slots_match_rows(slots, side, rows, n_bins)
    assert np.array_equal(over, pc > 64 * lines) and int(over.sum()) == info["side_rows"] >= 1  # a row overflows exactly when it does not fit
    assert info["census_rows"] == 4 ** k and info["census_over"] == WR.census(pc)[1]
    if name == "over":
        assert info["side_rows"] >= 3
    d.wide_list_table_drop()
    assert d.wide_list_table_info()["bytes"] == 0
    d.free()


def test_refusals_of_the_wide_build():
    d = upload(WR.table_fixture("dense"))
    info = d.wide_list_table_build()
    assert info["refused"] == capi.RB_LIST_REFUSED_DENSITY and info["bytes"] == 0 and info["builds"] == 0, info
    eng = engine([d], BUILD)
    assert eng.plan(0, 4096, 400)["kernel"] != WIDE_KERNEL  # remembered for these bits
    for bad in (3, -1):
        with pytest.raises(Exception):
            eng.set_wide_lists(bad)
    eng.destroy(), d.free()
    for n_bins, k, h, why in ((32257, 5, 3, capi.RB_LIST_REFUSED_GEOMETRY), (8192, 5, 3, capi.RB_LIST_REFUSED_GEOMETRY),
                              (8200, 5, 2, capi.RB_LIST_REFUSED_GEOMETRY), (8200, 14, 3, capi.RB_LIST_REFUSED_K)):
        d = capi.DeviceIBF.create(0, n_bins, h, k, ((n_bins + 63) // 64) * 64 * 64)
        info = d.wide_list_table_build()
        assert info["refused"] == why and info["bytes"] == 0, (n_bins, k, h, info)
        eng = engine([d], BUILD)
        assert eng.plan(0, 4096, 400)["kernel"] != WIDE_KERNEL
        eng.destroy(), d.free()


# ---------------------------------------------------------------- counts: planted bins, the tile deal, flagged slots, N
@pytest.fixture(scope="module", params=list(WR.COUNT_FIXTURES))
def counted(request):
    c = WR.count_fixture(request.param)
    d = upload(c.o)
    batch = H.pack_reads(c.all_reads())
    refs = {n_rule: RT.reference(c.o, batch, n_rule) for n_rule in (3, 4)}
    yield c, d, batch, refs
    d.free()


@pytest.mark.parametrize("nt", (0, 1))
def test_counts_equal_the_oracle(counted, nt):
    """every read of the fixture -- planted reads peaking at the first bin, 8191, 8192, 8193, both halves of the last counter dword and
    the last bin, on both strands; strands of 1 to 4 x 64 + 7 k-mers; hits in the tiles of one wave alone; crafted overflow and
    swapped-half slots at every place of a group; N at the first, a middle and the last base mixed with N-free reads -- in ONE batch,
    under both N rules, with and without the strand skip"""
    c, d, batch, refs = counted
    off, on = engine([d], OFF, nt), engine([d], BUILD, nt)
    parent = engine([d], None, nt)
    n, max_len = len(batch[2]), int(batch[2].max())
    assert off.plan(0, n, max_len) == parent.plan(0, n, max_len) and off.plan(0, n, max_len)["kernel"] != WIDE_KERNEL
    for n_rule in (3, 4):
        for eng in (off, on):
            eng.set_revcomp_of_n(n_rule)
        check(off, batch, refs[n_rule], ("off", c.n_bins, n_rule), repeats=1)
        if nt == 0 and n_rule == 3:
            assert d.wide_list_table_info()["builds"] == 0  # OFF builds nothing
        for prune in (1, 0):
            on.set_bound_pruning(prune)
            p = check(on, batch, refs[n_rule], ("build", c.n_bins, n_rule, prune, nt), WIDE_KERNEL)
            assert p["nontemporal"] == nt
    info = d.wide_list_table_info()
    assert info["lines"] == c.lines and info["builds"] == 1 and info["side_rows"] >= 1, info  # one table for every engine and call
    REACHED.add((info["lines"], nt))
    # the planted reads do peak where the fixture says, with (nearly) every k-mer
    planted = c.planted_reads()
    assert all(int(refs[3][0][i, 0]) >= len(r) - K + 1 - 12 for i, (r, _) in enumerate(planted))
    for eng in (off, on, parent):
        eng.destroy()


def test_a_counter_at_0xffff_and_a_strand_too_long_for_the_wide_form():
    c = WR.count_fixture("c8193")
    d = upload(c.o)
    eng, off = engine([d], BUILD), engine([d], OFF)
    d.wide_list_table_build()
    full = H.pack_reads(["C" * (65535 + K - 1), "G" * (65535 + K - 1), "C" * 500])
    ref = RT.reference(c.o, full)
    assert ref[0][:, 0].tolist() == [65535, 65535, 500 - K + 1]  # bin 5 once per k-mer: its counter ends at 0xFFFF
    check(eng, full, ref, "65535 k-mers", WIDE_KERNEL, repeats=1)
    p, q = eng.plan(0, 2, 65536 + K - 1), off.plan(0, 2, 65536 + K - 1)
    assert p == q and p["kernel"] != WIDE_KERNEL  # 65 536 k-mers: the plain form
    eng.destroy(), off.destroy(), d.free()


# ---------------------------------------------------------------- policy and lifecycle
@pytest.fixture(scope="module")
def small():
    c = WR.count_fixture("c8193")
    rng = np.random.default_rng(41)  # (48 random reads of 400 bases: with them the batch alone repays a table of 4^7 slots)
    batch = H.pack_reads([r for r, _ in c.planted_reads()] + c.n_reads() + c.flagged_reads()[:12] + [WR.random_dna(rng, 400) for _ in range(48)])
    return c, batch, RT.reference(c.o, batch)


def test_off_and_current_never_build_and_build_builds_once(small):
    c, batch, ref = small
    d = upload(c.o)
    n, max_len = len(batch[2]), int(batch[2].max())
    parent, off, cur, bld, bld2 = (engine([d], m) for m in (None, OFF, CURRENT, BUILD, BUILD))
    want = parent.plan(0, n, max_len)
    for eng, label in ((off, "off"), (cur, "current, no table")):
        assert eng.plan(0, n, max_len) == want
        check(eng, batch, ref, label, want["kernel"])
    assert d.wide_list_table_info()["builds"] == 0 and d.wide_list_table_info()["bytes"] == 0
    check(bld, batch, ref, "build", WIDE_KERNEL)
    check(bld2, batch, ref, "a second engine", WIDE_KERNEL)
    check(cur, batch, ref, "current, with the table", WIDE_KERNEL)
    check(off, batch, ref, "off, with the table", want["kernel"])
    info = d.wide_list_table_info()
    assert info["builds"] == 1 and info["lines"] == 4 and info["refused"] == 0 and info["build_ms"] > 0, info
    # a change of the bits drops the table; CURRENT goes back to the plain kernel, BUILD builds again
    read = WR.random_dna(np.random.default_rng(5), 300)
    d.insert(read, [0], [len(read)], [8190])
    assert d.wide_list_table_info()["bytes"] == 0 and d.wide_list_table_info()["builds"] == 1
    rng = np.random.default_rng(43)
    batch2 = H.pack_reads([read, WR.revcomp(read)] + c.n_reads() + [WR.random_dna(rng, 400) for _ in range(48)])
    after = RT.reference(RT.oracle_view(d), batch2)
    assert after[0][0, 0] == len(read) - K + 1
    check(cur, batch2, after, "current, after the insert", parent.plan(0, len(batch2[2]), int(batch2[2].max()))["kernel"])
    assert d.wide_list_table_info()["builds"] == 1
    check(bld, batch2, after, "build, after the insert", WIDE_KERNEL)
    assert d.wide_list_table_info()["builds"] == 2
    for eng in (parent, off, cur, bld, bld2):
        eng.destroy()
    d.free()


def test_an_insert_drops_the_table_and_the_next_call_rebuilds_it(small):
    """the list table's test of this name (tests/test_gpu_row_lists.py), for the wide table: both go through one drop and one build"""
    c, batch, ref = small
    d = upload(c.o)
    bld, cur = engine([d], BUILD), engine([d], CURRENT)
    check(bld, batch, ref, "before the insert", WIDE_KERNEL, repeats=1)
    info = d.wide_list_table_info()
    assert info["builds"] == 1 and info["bytes"] == 4 ** K * info["lines"] * 128 and info["refused"] == capi.RB_LIST_REFUSED_NONE, info
    read = WR.random_dna(np.random.default_rng(6), 300)
    d.insert(read, [0], [len(read)], [8191])
    info = d.wide_list_table_info()
    assert info["bytes"] == 0 and info["rows"] == 0 and info["builds"] == 1, info  # the table went with the bits it was built from
    rng = np.random.default_rng(44)
    batch2 = H.pack_reads([read, WR.revcomp(read)] + c.n_reads() + [WR.random_dna(rng, 400) for _ in range(48)])
    after = RT.reference(RT.oracle_view(d), batch2)
    assert after[0][0, 0] == after[0][1, 0] == len(read) - K + 1  # the changed filter: every k-mer of the inserted sequence, on both strands
    n2, max_len2 = len(batch2[2]), int(batch2[2].max())
    plain = engine([d], OFF)
    want = plain.plan(0, n2, max_len2)["kernel"]
    plain.destroy()
    assert want != WIDE_KERNEL
    check(cur, batch2, after, "current, after the insert", want, repeats=1)  # CURRENT takes the plain kernel and builds nothing
    info = d.wide_list_table_info()
    assert info["builds"] == 1 and info["bytes"] == 0, info
    check(bld, batch2, after, "build, after the insert", WIDE_KERNEL, repeats=1)
    info = d.wide_list_table_info()
    assert info["builds"] == 2 and info["refused"] == capi.RB_LIST_REFUSED_NONE and info["bytes"] == 4 ** K * info["lines"] * 128, info
    check(cur, batch2, after, "current, with the new table", WIDE_KERNEL, repeats=1)
    assert d.wide_list_table_info()["builds"] == 2
    bld.destroy(), cur.destroy(), d.free()


def test_a_batch_that_does_not_repay_the_build_and_a_trace_take_the_plain_kernel(small):
    torch = pytest.importorskip("torch")
    c, batch, ref = small
    d = upload(c.o)
    eng = engine([d], BUILD)
    n, max_len = len(batch[2]), int(batch[2].max())
    off = engine([d], OFF)
    assert eng.plan(0, 2, 40) == off.plan(0, 2, 40) and eng.plan(0, 2, 40)["kernel"] != WIDE_KERNEL  # 2 reads of 34 k-mers against 4^7 slots
    off.destroy()
    one = H.pack_reads([c.plants[0][0][:40], c.plants[1][0][:40]])
    check(eng, one, RT.reference(c.o, one), "too small a batch", repeats=1)
    assert d.wide_list_table_info()["builds"] == 0
    t = torch.zeros(16 * n, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    eng.set_prune_trace(t.data_ptr())
    assert check(eng, batch, ref, "trace", repeats=1)["kernel"] != WIDE_KERNEL
    torch.cuda.synchronize()
    assert d.wide_list_table_info()["builds"] == 0 and int((t != 0).sum()) >= n  # the plain kernel wrote its records
    eng.set_prune_trace(None)
    check(eng, batch, ref, "no trace", WIDE_KERNEL, repeats=1)
    eng.destroy(), d.free()


def test_a_full_side_table_refuses():
    o = WR.table_fixture("over")
    d = upload(o)
    rng = np.random.default_rng(3)
    batch = H.pack_reads([WR.random_dna(rng, 300) for _ in range(64)])
    ref = RT.reference(o, batch)
    eng = engine([d], BUILD)
    n, max_len = len(batch[2]), 300
    off = engine([d], OFF)
    plain = off.plan(0, n, max_len)["kernel"]
    off.destroy()
    capi.lib().rb_set_wide_list_side_capacity(2)
    try:
        check(eng, batch, ref, "side table of two rows", repeats=1)
        info = d.wide_list_table_info()
        assert info["refused"] == capi.RB_LIST_REFUSED_SIDE_FULL and info["bytes"] == 0 and info["builds"] == 0, info
        assert eng.plan(0, n, max_len)["kernel"] == plain  # remembered for these bits
    finally:
        capi.lib().rb_set_wide_list_side_capacity(0)
    check(eng, batch, ref, "still refused", plain, repeats=1)
    assert d.wide_list_table_info()["builds"] == 0
    d.wide_list_table_drop()  # lifts the refusal
    check(eng, batch, ref, "asked again", WIDE_KERNEL, repeats=1)
    info = d.wide_list_table_info()
    assert info["builds"] == 1 and info["side_rows"] >= 3 and info["lines"] == 8, info
    REACHED.add((info["lines"], 0))
    eng.destroy(), d.free()


def test_a_max_bytes_refusal_is_remembered_and_lifted(small):
    c = WR.count_fixture("c32256")  # eight lines: 16 MiB of slots at k = 7, where four lines would be 8 MiB
    d = upload(c.o)
    batch = H.pack_reads([r for r, _ in c.planted_reads()] * 8)
    ref = RT.reference(c.o, batch)
    eng, off = engine([d], BUILD), engine([d], OFF)
    n, max_len = len(batch[2]), int(batch[2].max())
    off.set_row_table(capi.RB_ROW_TABLE_OFF)
    plain = off.plan(0, n, max_len)["kernel"]
    off.destroy()
    eng.set_row_table(capi.RB_ROW_TABLE_OFF, 10 << 20)
    assert eng.plan(0, n, max_len)["kernel"] == WIDE_KERNEL  # before the census nothing says the table will not fit
    check(eng, batch, ref, "10 MiB allowed", repeats=1)
    info = d.wide_list_table_info()
    assert info["refused"] == capi.RB_LIST_REFUSED_MAX_BYTES and info["builds"] == 0 and info["census_rows"] == 4 ** K, info
    assert eng.plan(0, n, max_len)["kernel"] == plain
    eng.set_row_table(capi.RB_ROW_TABLE_OFF, 4 << 20)  # not even the smallest slot size
    assert eng.plan(0, n, max_len)["kernel"] == plain
    eng.set_row_table(capi.RB_ROW_TABLE_OFF, 1 << 30)  # the caller allows more: asked again
    check(eng, batch, ref, "1 GiB allowed", WIDE_KERNEL, repeats=1)
    assert d.wide_list_table_info()["builds"] == 1 and d.wide_list_table_info()["lines"] == 8
    eng.destroy(), d.free()


@pytest.mark.parametrize("mode", (OFF, CURRENT, BUILD))
def test_an_engine_serves_each_filter_from_its_own_form(small, mode):
    """a wide filter, an 8192-bin filter with a list table and a narrow filter in one engine"""
    c, batch, ref = small
    rng = np.random.default_rng(17)
    wide = upload(c.o)
    lst, o_lst = RT.device_filter(8192, 16381, 3, K, seed=9, plant=[(c.plants[0][0], 100)])
    narrow, o_nar = RT.device_filter(200, 4099, 3, K, seed=4, plant=[(c.plants[1][0], 7)])
    eng = capi.Engine(0, [wide, lst, narrow], [])
    eng.set_split_threshold(0)
    eng.set_row_table(capi.RB_ROW_TABLE_LISTS)
    base = capi.Engine(0, [wide, lst, narrow], [])
    base.set_split_threshold(0)
    base.set_row_table(capi.RB_ROW_TABLE_LISTS)
    eng.set_wide_lists(mode)
    if mode == CURRENT:
        wide.wide_list_table_build()
    n, max_len = len(batch[2]), int(batch[2].max())
    plans = [eng.plan(fi, n, max_len)["kernel"] for fi in range(3)]
    parents = [base.plan(fi, n, max_len)["kernel"] for fi in range(3)]
    assert plans[0] == (parents[0] if mode == OFF else WIDE_KERNEL) and parents[0] != WIDE_KERNEL
    assert plans[1] == parents[1] == LISTS_KERNEL and plans[2] == parents[2] and plans[2] not in (WIDE_KERNEL, LISTS_KERNEL)
    refs = [ref, RT.reference(o_lst, batch), RT.reference(o_nar, batch)]
    for rep in range(2):
        mc = eng.classify(*batch)[0]
        for fi in range(3):
            assert np.array_equal(mc[:, fi], refs[fi][0][:, 0]), (mode, rep, fi)
    assert wide.wide_list_table_info()["builds"] == (0 if mode == OFF else 1)
    assert lst.list_table_info()["builds"] == 1 and lst.wide_list_table_info()["builds"] == 0
    eng.destroy(), base.destroy()
    for d in (wide, lst, narrow):
        d.free()


def test_every_slot_size_and_both_builds_were_reached():
    assert REACHED == {(lines, nt) for lines in WR.WIDE_LINES for nt in (0, 1)}, sorted(REACHED)

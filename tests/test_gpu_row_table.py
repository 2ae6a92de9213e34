"""The row table of a resident filter (rb_dibf_row_table_build) and the row form of the plain count kernel (ibf_count_rows_kernel,
rb_engine_set_row_table): one precomputed row per N-free k-mer -- the AND of its h blocks -- gathered once per k-mer instead of h blocks.
None of that may change a result.  The table is compared row by row with the AND of the filter's downloaded blocks at the oracle's block
numbers; classify calls with the row form forced are compared bit for bit -- raw maxima, decisions, status -- with the oracle and with
the row form off; the lifecycle (drop on change, shared by engines, freed with the filter) and the policy of the auto mode are read
through rb_engine_plan and rb_dibf_row_table_info.  Small k keeps every table at 4^5 - 4^7 rows (at most 16 MiB)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import pyoracle as po
from readbouncer_amd import capi
from tests import helpers as H
from tests import pass_edges as PE

ROWS_KERNEL, PLAIN_KERNEL = "ibf_count_rows_kernel", "ibf_count_max_kernel"
OFF, AUTO, FORCE = capi.RB_ROW_TABLE_OFF, capi.RB_ROW_TABLE_AUTO, capi.RB_ROW_TABLE_FORCE
# every row build the launcher can select: (words per lane, counter planes, non-temporal).  The row launches are non-temporal when the ROW
# TABLE is beyond rb_engine_set_nt_threshold: 0 puts every table beyond it, NT_NEVER none
REACHED = set()
ROW_BUILDS = {(wpl, planes, nt) for wpl in (1, 2) for planes in (10, 16) for nt in (0, 1)}
NT_NEVER = 1 << 62


def rc(s):
    return PE.revcomp_str(s)


def device_filter(n_bins, n_blocks, h, k, seed, plant=None):
    """a resident filter at design load with `plant` = [(sequence, bin)] inserted, and the oracle's view of its downloaded bits"""
    W = (n_bins + 63) // 64
    d = capi.DeviceIBF.create(0, n_bins, h, k, W * 64 * n_blocks)
    d.fill_synth(seed)
    for seq, b in plant or []:
        d.insert(seq, [0], [len(seq)], [b])
    return d, oracle_view(d)


def oracle_view(d):
    host = d.download()
    i = host.info
    o = po.OracleIBF.wrap(i["n_bins"], i["n_hash"], i["kmer_size"], i["n_bits"], host.words())
    o._host = host
    return o


def reference(o, batch, n_rule=3):
    buf, offs, lens = batch
    prev = po.set_revcomp_of_n(n_rule)
    try:
        dec, st = po.batch_check_unblock([o], [], buf, offs, lens, n_threads=8)
        return po.batch_raw_max(o, buf, offs, lens, 8).reshape(-1, 1), dec, st
    finally:
        po.set_revcomp_of_n(prev)


def engine(d, mode, nt=0):
    eng = capi.Engine(0, [d], [])
    eng.set_split_threshold(0)  # small batches in the throughput form
    eng.set_row_table(mode)
    eng.set_nt_threshold(0 if nt else NT_NEVER)
    return eng


def check(eng, batch, ref, label, want_kernel, masks=(0, 7, 15)):
    buf, offs, lens = batch
    p = eng.plan(0, len(lens), int(lens.max()))
    assert p["kernel"] == want_kernel, (label, p)
    assert (p["row_table_bytes"] > 0) == (want_kernel == ROWS_KERNEL), (label, p)
    if want_kernel == ROWS_KERNEL:
        assert p["lanes_per_block_log2"] == 6
        REACHED.add((p["words_per_lane"], p["counter_planes"], p["nontemporal"]))
    for mask in masks:
        eng.set_prune_parts(mask)
        for rep in range(2):
            mc, _, dec, st = eng.classify(buf, offs, lens)
            bad = np.nonzero((mc != ref[0]).any(axis=1))[0]
            assert len(bad) == 0, (label, mask, rep, [(int(i), int(lens[i]), mc[i].tolist(), ref[0][i].tolist()) for i in bad[:6]])
            assert np.array_equal(dec, ref[1]) and np.array_equal(st, ref[2]), (label, mask, rep, "decision/status")
    eng.set_prune_parts(15)


# ---------------------------------------------------------------- the table itself
@pytest.mark.parametrize("n_bins", (4096, 8192))
@pytest.mark.parametrize("n_blocks", (1024, 1021))
@pytest.mark.parametrize("h", (2, 3, 4))
@pytest.mark.parametrize("k", (5, 7))
def test_rows_are_the_and_of_the_oracles_blocks(k, h, n_blocks, n_bins):
    d, o = device_filter(n_bins, n_blocks, h, k, seed=k * 100 + h)
    info = d.row_table_build()
    W = o.bin_width
    assert info["refused"] == 0 and info["rows"] == 4 ** k and info["bytes"] == info["want_bytes"] == 4 ** k * W * 8 and info["builds"] == 1
    rows = d.row_table_download()
    assert rows.shape == (4 ** k, W)
    blocks = o.words()[:n_blocks * W].reshape(n_blocks, W)
    r = np.arange(4 ** k)
    digits = np.stack([(r >> (2 * (k - 1 - i))) & 3 for i in range(k)], axis=1).astype(np.uint8)  # first base most significant
    expected = np.full((4 ** k, W), ~np.uint64(0), dtype=np.uint64)
    for hash_no in range(h):
        idx = np.array([o.block_index(po.kmer_value(np.ascontiguousarray(digits[i]), k), hash_no) for i in range(4 ** k)], dtype=np.int64)
        expected &= blocks[idx]
    assert np.array_equal(rows, expected)
    d.free()


# ---------------------------------------------------------------- classify: force == off == oracle
K = 7


@pytest.fixture(scope="module")
def planted():
    rng = np.random.default_rng(77)
    return rng, H.random_dna(rng, 6000)


def read_shapes(rng, ref, lens):
    """per length: a random read, a planted one with 5 % errors on either strand, a threshold-adjacent one (20 %), and the N cases"""
    reads = []
    for L in lens:
        s = int(rng.integers(0, len(ref) - L))
        pos = ref[s:s + L]
        reads += [H.random_dna(rng, L), H.mutate(rng, pos, 0.05), rc(H.mutate(rng, pos, 0.05)), H.mutate(rng, pos, 0.2), rc(H.mutate(rng, pos, 0.2)),
                  "N" + pos[1:], pos[:L // 2] + "N" + pos[L // 2 + 1:], pos[:-1] + "N", rc("N" + pos[1:]), "N" * L, H.random_dna(rng, L, with_n=0.02)]
    return reads + ["ACGT", "A" * (K - 1), ""]


@pytest.mark.parametrize("nt", (0, 1))
@pytest.mark.parametrize("n_bins", (4096, 8192, 8200))
@pytest.mark.parametrize("lens,planes", (((40, 70, 71, 354), 10), ((354, 1100), 16)))
def test_classify_forced_rows_equal_off_and_the_oracle(planted, n_bins, lens, planes, nt):
    rng, ref = planted
    plant = [(ref[i * 2000:(i + 1) * 2000], b) for i, b in enumerate((3, n_bins // 2 + 5, n_bins - 1))]
    d, o = device_filter(n_bins, 1021, 3, K, seed=9, plant=plant)
    batch = H.pack_reads(read_shapes(rng, ref, lens))
    eng_off, eng_on = engine(d, OFF, nt), engine(d, FORCE, nt)
    for n_rule in (3, 4):  # what the reverse strand holds for an N of the read
        expected = reference(o, batch, n_rule)
        for eng in (eng_off, eng_on):
            eng.set_revcomp_of_n(n_rule)
        check(eng_off, batch, expected, ("off", n_bins, lens, n_rule), PLAIN_KERNEL, masks=(15,))
        check(eng_on, batch, expected, ("force", n_bins, lens, n_rule), ROWS_KERNEL)
    p = eng_on.plan(0, len(batch[2]), int(batch[2].max()))
    assert p["counter_planes"] == planes and p["column_slices"] == (2 if n_bins == 8200 else 1) and p["nontemporal"] == nt
    assert d.row_table_info()["builds"] == 1  # one table, built by the first forced call, used by all
    eng_off.destroy(), eng_on.destroy(), d.free()


def test_packed_input_chunks_and_ids(planted):
    torch = pytest.importorskip("torch")
    rng, ref = planted
    d, o = device_filter(8192, 1021, 3, K, seed=10, plant=[(ref[:2000], 100)])
    reads = read_shapes(rng, ref, (200, 354))
    buf, offs, lens = H.pack_reads(reads)
    packed, p_offs, nmask, n_offs = capi.pack_reads(buf, offs, lens)
    dev = torch.device("cuda:0")
    t = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (packed, p_offs.view(np.int64), lens.view(np.int32), nmask, n_offs.view(np.int64))]
    ids = np.array([i for i in range(len(reads)) if i % 3 != 1][::-1], dtype=np.uint32)
    t_ids = torch.from_numpy(ids.view(np.int32)).to(dev)
    start, length = 33, 150
    items = [reads[i][start:start + length] for i in ids]
    expected = reference(o, H.pack_reads(items))
    keep = [i for i, r in enumerate(items) if len(reads[ids[i]]) > start]  # (a chunk beyond the read's end has a status of its own)
    assert len(keep) >= len(items) - 3
    outs = {}
    for mode in (OFF, FORCE):
        eng = engine(d, mode)
        t_max = torch.zeros((len(ids), 1), dtype=torch.int16, device=dev)
        t_dec = torch.zeros(len(ids), dtype=torch.uint8, device=dev)
        t_st = torch.zeros(len(ids), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        eng.classify_device_ex(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), len(ids), int(lens.max()), t[3].data_ptr(), t[4].data_ptr(),
                               chunk_start=start, chunk_length=length, d_read_ids=t_ids.data_ptr(), d_maxcount=t_max.data_ptr(),
                               d_decision=t_dec.data_ptr(), d_status=t_st.data_ptr())
        torch.cuda.synchronize()
        p = eng.plan(0, len(ids), int(lens.max()))
        assert p["kernel"] == (ROWS_KERNEL if mode == FORCE else PLAIN_KERNEL)
        outs[mode] = (t_max.cpu().numpy().view(np.uint16), t_dec.cpu().numpy(), t_st.cpu().numpy())
        eng.destroy()
    assert all(np.array_equal(a, b) for a, b in zip(outs[OFF], outs[FORCE]))
    assert np.array_equal(outs[FORCE][0][keep], expected[0][keep]) and np.array_equal(outs[FORCE][1][keep], expected[1][keep])
    d.free()


# ---------------------------------------------------------------- lifecycle
def test_a_change_of_the_bits_drops_the_table_and_engines_share_it(planted):
    rng, ref = planted
    d, o = device_filter(4096, 1021, 3, K, seed=11)
    read = ref[2500:2854]
    batch = H.pack_reads([read, H.random_dna(rng, 354), rc(read)])
    e1, e2 = engine(d, FORCE), engine(d, FORCE)
    before = reference(o, batch)
    check(e1, batch, before, "before the insert", ROWS_KERNEL, masks=(15,))
    check(e2, batch, before, "second engine", ROWS_KERNEL, masks=(15,))
    info = d.row_table_info()
    assert info["builds"] == 1 and info["bytes"] == 4 ** K * 64 * 8  # two engines, one table
    d.insert(read, [0], [len(read)], [1234])
    assert d.row_table_info()["bytes"] == 0 and d.row_table_info()["builds"] == 1  # dropped with the change
    after = reference(oracle_view(d), batch)
    assert after[0][0, 0] == len(read) - K + 1 > before[0][0, 0]  # the insert changed the read's maximum
    check(e2, batch, after, "after the insert", ROWS_KERNEL, masks=(15,))
    assert d.row_table_info()["builds"] == 2 and d.row_table_info()["bytes"] > 0  # rebuilt by the call that needed it
    check(e1, batch, after, "after the insert, first engine", ROWS_KERNEL, masks=(15,))
    assert d.row_table_info()["builds"] == 2
    d.row_table_drop()
    assert d.row_table_info()["bytes"] == 0
    d.fill_synth(12)
    e1.set_row_table(OFF)
    check(e1, batch, reference(oracle_view(d), batch), "off after a refill", PLAIN_KERNEL, masks=(15,))
    assert d.row_table_info()["bytes"] == 0 and d.row_table_info()["builds"] == 2
    e1.destroy(), e2.destroy()
    torch = pytest.importorskip("torch")
    d.row_table_build()
    torch.cuda.synchronize()
    free_with = torch.cuda.mem_get_info(0)[0]
    d.free()
    assert torch.cuda.mem_get_info(0)[0] >= free_with + 4 ** K * 64 * 8  # the table went with the filter


# ---------------------------------------------------------------- policy of the auto mode
def kernel_of(eng, n_reads, max_len):
    return eng.plan(0, n_reads, max_len)["kernel"]


def test_auto_mode_policy(planted):
    rng, ref = planted
    L = 360
    kmers = L - K + 1
    need = -(-(4 ** K * 4) // (2 * kmers * 2))  # rule (b): items x 2 x k-mers x (h - 1) >= 4^k x (h + 1)
    d, o = device_filter(8192, 1021, 3, K, seed=13)
    eng = capi.Engine(0, [d], [])  # auto is the default
    eng.set_split_threshold(0)
    assert kernel_of(eng, need - 1, L) == PLAIN_KERNEL and kernel_of(eng, need, L) == ROWS_KERNEL
    small = H.pack_reads([H.random_dna(rng, L) for _ in range(need - 1)])
    check(eng, small, reference(o, small), "below rule (b)", PLAIN_KERNEL, masks=(15,))
    assert d.row_table_info()["builds"] == 0
    big = H.pack_reads([H.random_dna(rng, L) for _ in range(need)] + [ref[100:100 + L]])
    ref_big = reference(o, big)
    # what keeps a qualifying batch on today's kernel: early decision, a max_bytes below the table, a column shard
    eng.set_early_decision(1)
    assert kernel_of(eng, need, L) == PLAIN_KERNEL
    eng.set_early_decision(0)
    eng.set_row_table(AUTO, 4 ** K * 128 * 8 - 1)
    check(eng, big, ref_big, "max_bytes below the table", PLAIN_KERNEL, masks=(15,))
    assert d.row_table_info()["builds"] == 0
    eng.set_row_table(AUTO, 96 << 30)
    check(eng, big, ref_big, "above rule (b)", ROWS_KERNEL, masks=(15,))
    info = d.row_table_info()
    assert info["builds"] == 1 and info["bytes"] == 4 ** K * 128 * 8 and info["build_ms"] > 0
    eng.set_row_table(OFF)
    check(eng, big, ref_big, "off", PLAIN_KERNEL, masks=(15,))
    eng.destroy(), d.free()
    # k = 14 has no table; a run-time hash count has no row build
    for k, h in ((14, 3), (K, 2), (K, 4)):
        f = capi.DeviceIBF.create(0, 8192, h, k, 128 * 64 * 1021)
        e = capi.Engine(0, [f], [])
        e.set_split_threshold(0)
        assert kernel_of(e, 1 << 24, L) == PLAIN_KERNEL, (k, h)
        e.set_row_table(FORCE)
        assert kernel_of(e, 1 << 24, L) == PLAIN_KERNEL, (k, h)
        if k == 14:
            assert f.row_table_build()["refused"] == capi.RB_ROW_REFUSED_K
        e.destroy(), f.free()
    narrow = capi.DeviceIBF.create(0, 2048, 3, K, 32 * 64 * 1021)
    assert narrow.row_table_build()["refused"] == capi.RB_ROW_REFUSED_NARROW
    narrow.free()


def test_column_sharded_engine_keeps_the_plain_kernel():
    d = capi.DeviceIBF.create(0, 8192 * 2, 3, K, 256 * 64 * 1021)
    eng = capi.Engine(0, [d], [])
    eng.set_split_threshold(0)
    eng.set_row_table(FORCE)
    assert kernel_of(eng, 1 << 20, 360) == ROWS_KERNEL
    eng.set_column_shard(0, 2)
    assert kernel_of(eng, 1 << 20, 360) == PLAIN_KERNEL
    eng.destroy(), d.free()


# ---------------------------------------------------------------- counter edges (the constructions of tests/pass_edges.py at k = 7)
@pytest.mark.parametrize("n_bins", (4090, 8200))
def test_counter_edges_on_the_row_builds(n_bins):
    """SAT (the last bin, set in every block) counts every k-mer of a read on both strands: 1023 fills the ten planes, 1024 switches to
    sixteen, 65 536 and more wrap a uint16_t; NEAR (bit load 0.99) is the maximum where SAT has wrapped"""
    n_blocks, W = 1021, (n_bins + 63) // 64
    d = capi.DeviceIBF.create(0, n_bins, 3, K, W * 64 * n_blocks)
    host = d.download()
    w = host.words()[:n_blocks * W].reshape(n_blocks, W)
    rng = np.random.default_rng(n_bins)
    for b, load in ((n_bins - 1, 2.0), (PE.NEAR, 0.99), (PE.LOW, 0.5)):
        w[:, b // 64] |= (rng.random(n_blocks) < load).astype(np.uint64) << np.uint64(b % 64)
    d.free()
    d = capi.DeviceIBF.upload(0, host)
    o = po.OracleIBF.wrap(n_bins, 3, K, host.info["n_bits"], host.words())
    engines = [engine(d, FORCE, nt) for nt in (0, 1)]
    for which in PE.BATCHES:
        reads, kmers = PE.batch(which, K)
        batch = H.pack_reads(list(reads))
        expected = reference(o, batch)
        for n, got in zip(kmers, expected[0][:, 0]):
            if n is not None and n < 65536:
                assert got == n  # SAT
        for nt, eng in enumerate(engines):
            check(eng, batch, expected, (n_bins, which, nt), ROWS_KERNEL, masks=(0, 15))
    for eng in engines:
        eng.destroy()
    d.free()


def test_every_row_build_was_reached():
    assert REACHED == ROW_BUILDS, sorted(ROW_BUILDS - REACHED)

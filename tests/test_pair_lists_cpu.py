"""The pair table checked without a GPU: readbouncer_amd/csrc/rb_pair_lists.h through a stand-alone C++ program, plain and under the
address and undefined-behaviour sanitizers (encode / decode round trips, every offset inside counters or spares, the census's verdicts,
a host emulation of the add path against plain counting); the fixtures of tests/test_gpu_pair_lists.py asserted on the oracle alone, so
that every branch those tests name is provably reached; and the census's caps on config 3's geometry at design load."""
import os
import subprocess

import numpy as np
import pytest

from oracle import pyoracle as po
from tests import pair_lists_rig as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "readbouncer_amd", "csrc")


def build_program(tmp_path, sanitize):
    exe = str(tmp_path / ("test_pair_lists" + ("_san" if sanitize else "")))
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall"] + flags + [os.path.join(ROOT, "tests", "cpp", "test_pair_lists.cpp"), "-o", exe])
    return exe


@pytest.mark.parametrize("sanitize", (False, True))
def test_layout_round_trips_offsets_census_and_add_path(tmp_path, sanitize):
    run = subprocess.run([build_program(tmp_path, sanitize)], capture_output=True, text=True)
    assert run.returncode == 0 and "all passed" in run.stdout, run.stdout + run.stderr


def test_the_header_is_free_of_hip_and_the_unit_is_built():
    header = open(os.path.join(CSRC, "rb_pair_lists.h")).read()
    assert "hip_runtime" not in header and "rb_device.h" not in header
    makefile = open(os.path.join(CSRC, "Makefile")).read()
    assert "rb_pair_lists.o" in makefile and "rb_pair_lists.h" in makefile


def test_the_constants_of_the_rig_are_the_headers():
    header = open(os.path.join(CSRC, "rb_pair_lists.h")).read()
    for text in ("kPairCanonEntries = 256", "kPairPositional = 64;", "kPairRest = 64;", "kPairRestIndexed = kPairRest - 2;", "kPairTailHalves = 64;",
                 "kPairTailMark = 0xFFFDu", "kPairTailShare = 5;", "kPairDenseShare = 10;"):
        assert text in header, text
    assert (PR.CANON, PR.POSITIONAL, PR.REST, PR.REST_INDEXED, PR.TAIL_HALVES, PR.TAIL_MARK) == (256, 64, 64, 62, 64, 0xFFFD)
    assert (PR.TAIL_SHARE, PR.DENSE_SHARE) == (1 << 5, 1 << 10) and (PR.CAPACITY, PR.TAIL_CAPACITY) == (192, 254)


def test_the_crafted_pairs_reach_every_kind_of_slot():
    """on the oracle alone: the crafted k-mers and their reverse complements have exactly the populations the GPU test names -- nothing,
    capacity - 1, capacity, capacity + 1 (the first tail), 254 (the last tail), 255 (the first dense pair), 128 beside 10 and its mirror"""
    n_bins, k = 8192, PR.CraftedPairs.K
    W = n_bins // 64
    n_bits = W * 64 * PR.CRAFT_BLOCKS
    words = np.zeros(PR.CRAFT_BLOCKS * W + 8, dtype=np.uint64)  # (the crafted blocks are rewritten whole: what the others hold does not matter; 8 pad words)
    c = PR.CraftedPairs(n_bins, words, n_bits)
    assert [a + b for a, b in c.PAIRS] == [0, PR.CAPACITY - 1, PR.CAPACITY, PR.CAPACITY + 1, PR.TAIL_CAPACITY, PR.TAIL_CAPACITY + 1, 138, 138]
    assert c.kinds() == [PR.PLAIN, PR.PLAIN, PR.PLAIN, PR.TAIL, PR.TAIL, PR.DENSE, PR.PLAIN, PR.PLAIN]
    blocks = c.o.words()[:PR.CRAFT_BLOCKS * W].reshape(PR.CRAFT_BLOCKS, W)
    for x, (nA, nB) in zip(c.KMERS, c.PAIRS):
        for s, want in ((x, nA), (PR.revcomp(x), nB)):
            row = np.full(W, ~np.uint64(0), dtype=np.uint64)
            for h in range(PR.H_FUNCS):
                row &= blocks[c.o.block_index(po.kmer_value(po.encode(s), k), h)]
            assert int(np.unpackbits(row.view(np.uint8)).sum()) == want, (s, want)
    reads = c.reads()
    tail, tail2, dense = c.KMERS[3], c.KMERS[4], c.KMERS[5]
    assert tail + tail2 in reads and tail + tail in reads and dense + tail in reads  # k-mers 0 and 7: first and last of one group of eight
    assert len(set(c.ranks + c.rc_ranks)) == 16  # no palindrome among them (k is odd), no k-mer the reverse complement of another


def test_palindromes_exist_at_even_k_only():
    for k, want in ((5, 0), (6, 64), (7, 0)):
        assert int((PR.rc_ranks(k) == np.arange(4 ** k)).sum()) == want
    assert np.array_equal(PR.rc_ranks(6)[PR.rc_ranks(6)], np.arange(4 ** 6))


def test_config_3_at_design_load_stays_inside_both_caps():
    """config 3: 8192 bins, h = 3, bit load 55/256, so a row holds Binomial(8192, (55/256)^3) bins -- 81 +- 9 -- and the rows of x and
    rc(x) are independent (different blocks).  4 M simulated pairs: the share that needs a tail stays below 1 in 32 -- it is about 1 in
    106 -- and none needs dense rows, where 1 in 1024 is allowed (the k-mers with coinciding blocks are a handful in 4^13 at 8 M blocks)."""
    p = (55 / 256) ** 3
    assert abs(8192 * p - 81.2) < 0.5
    tail, dense = PR.census_shares(8192, p, 4_000_000, seed=3)
    assert 0.005 < tail < 1 / PR.TAIL_SHARE / 2 and dense < 1 / PR.DENSE_SHARE / 100, (tail, dense)
    # and the list table's census chooses two lines there, which is when RB_ROW_TABLE_AUTO considers the pair table at all
    rng = np.random.default_rng(4)
    n = rng.binomial(8192, p, 1_000_000)
    assert (n > 64).mean() > 1 / 1024 > (n > 128).mean()


@pytest.mark.parametrize("k", (5, 6, 7, 13))
def test_the_kmer_of_value_0_hashes_to_block_0_under_every_hash_function(k):
    """why the census allows two dense slots beyond its cap (rbpair::kPairAlwaysDense): A^k has the value 0, every hash of 0 is block 0,
    so its row is a whole block -- a fifth of the bins at design load -- in every filter, and it has two slots, its own and T^k's"""
    for n_bins, n_blocks in ((8192, PR.SPARE_BLOCKS), (8192, 1021), (2112, 1021), (4090, 65521)):
        W = (n_bins + 63) // 64
        o = po.OracleIBF(n_bins, PR.H_FUNCS, k, W * 64 * n_blocks)
        assert po.kmer_value(po.encode("A" * k), k) == 0
        assert [o.block_index(0, h) for h in range(PR.H_FUNCS)] == [0] * PR.H_FUNCS
        assert po.kmer_value(po.encode("T" * k), k) != 0

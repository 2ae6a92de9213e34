// test_pair_lists.cpp -- the pair table's slot layout (readbouncer_amd/csrc/rb_pair_lists.h) on a CPU: encode / decode round trips over
// every kind of slot, every offset a slot or tail line holds lies inside the counters or the spares, the census's verdicts, and a host
// emulation of the count kernel's add path -- lines 0-1 positional, line 2 and the tail line by their list bit, an index dword replaced
// by spares -- against plain counting of both lists.  A stand-alone program: build it plain and with -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../../readbouncer_amd/csrc/rb_pair_lists.h"

using namespace rbpair;

static int g_fail = 0;
#define CHECK(c)                                                  \
    do {                                                          \
        if (!(c)) {                                               \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
            ++g_fail;                                             \
        }                                                         \
    } while (0)

static std::vector<uint16_t> random_list(std::mt19937 &rng, uint32_t n, uint32_t n_bins)
{
    std::vector<uint8_t> in(n_bins, 0);
    uint32_t have = 0;
    while (have < n) {
        const uint32_t b = rng() % n_bins;
        if (!in[b]) in[b] = 1, ++have;
    }
    std::vector<uint16_t> out;
    for (uint32_t b = 0; b < n_bins; ++b)
        if (in[b]) out.push_back((uint16_t)b);
    return out;
}

// the kernel's add path on the host: counters of one dword per bin behind them the spares, as count_lds_bytes lays them out
struct Lds {
    std::vector<uint32_t> dw;
    uint32_t limit;
    bool ok = true;
    explicit Lds(uint32_t n_bins) : dw(cnt_dwords(n_bins) + kPairSpareDwords, 0), limit((cnt_dwords(n_bins) + kPairSpareDwords) * 4u) {}
    void add(uint32_t offset, uint32_t value)
    {
        if ((offset & 3u) || offset >= limit) {  // every offset lies inside the counters or the spares, on a dword
            ok = false;
            return;
        }
        dw[offset / 4] += value;
    }
    void add_positional(uint32_t v) { add(v & 0xFFFFu, 1u), add(v >> 16, 0x10000u); }
    void add_rest(uint32_t v)
    {
        add(v & kPairOffset, (v & kPairListB) * 0xFFFFu + 1u);
        add((v >> 16) & kPairOffset, ((v >> 16) & kPairListB) * 0xFFFFu + 1u);
    }
};

static void count_slot(Lds &lds, const uint32_t *slot, const std::vector<uint32_t> &tails, const std::vector<uint16_t> &A, const std::vector<uint16_t> &B,
                       uint32_t n_bins)
{
    for (uint32_t d = 0; d < kPairPositional; ++d) lds.add_positional(slot[d]);
    bool indexed = false;
    for (uint32_t i = 0; i < kPairRest / 2; ++i) {
        uint32_t w = slot[kPairPositional + i];
        if (w & kPairIndex) {  // only the last dword ever is
            CHECK(i == kPairRest / 2 - 1);
            indexed = true;
            w = spare_of_half(n_bins, 2 * i) | (spare_of_half(n_bins, 2 * i + 1) << 16);
        }
        lds.add_rest(w);
    }
    if (!indexed) return;
    const uint32_t last = slot[kPairIndexDword], idx = index_of(last);
    if (last & kPairDense) {  // the dense rows: here the lists themselves
        for (uint16_t b : A) lds.add(b * 4u, 1u);
        for (uint16_t b : B) lds.add(b * 4u, 0x10000u);
    } else {
        for (uint32_t i = 0; i < kPairTailDwords; ++i) lds.add_rest(tails[(size_t)idx * kPairTailDwords + i]);
    }
}

static void round_trip(std::mt19937 &rng, uint32_t nA, uint32_t nB, uint32_t n_bins, bool same = false)
{
    const std::vector<uint16_t> A = random_list(rng, nA, n_bins), B = same ? A : random_list(rng, nB, n_bins);
    const uint32_t index = rng() % 5;
    uint32_t slot[kPairDwords];
    std::vector<uint32_t> tails((index + 1) * kPairTailDwords, 0xDEADBEEFu);
    const PairKind kind = encode_pair(A.data(), nA, B.data(), nB, n_bins, index, slot, tails.data() + (size_t)index * kPairTailDwords);
    CHECK(kind == kind_of(nA, nB));
    std::vector<uint16_t> a(kPairMaxBins), b(kPairMaxBins);
    uint32_t na = 0, nb = 0, got_index = ~0u;
    const int dk = decode_pair(slot, n_bins, a.data(), &na, b.data(), &nb, &got_index);
    CHECK(dk == (int)kind);
    if (kind != kPlain) CHECK(got_index == index);
    if (kind == kTail) CHECK(decode_rest(tails.data() + (size_t)index * kPairTailDwords, kPairTailHalves, n_bins, a.data(), &na, b.data(), &nb));
    if (kind != kDenseRows) {
        CHECK(na == nA && nb == nB);
        CHECK((!nA || !memcmp(a.data(), A.data(), 2 * nA)) && (!nB || !memcmp(b.data(), B.data(), 2 * nB)));
    } else {
        CHECK(na == 0 && nb == 0);
    }
    // the canonical form and back
    uint16_t canon[kPairCanonEntries];
    CHECK(decode_resident(slot, n_bins, canon) == (int)kind);
    uint32_t ca = 0, cb = 0, cindex = ~0u;
    CHECK(decode_canonical(canon, n_bins, a.data(), &ca, b.data(), &cb, &cindex) == (int)kind);
    if (kind == kPlain) CHECK(ca == nA && cb == nB);
    if (kind != kPlain) CHECK(cindex == index);
    // the add path against plain counting
    Lds lds(n_bins);
    count_slot(lds, slot, tails, A, B, n_bins);
    CHECK(lds.ok);
    std::vector<uint32_t> want(cnt_dwords(n_bins), 0);
    for (uint16_t x : A) want[x] += 1u;
    for (uint16_t x : B) want[x] += 0x10000u;
    CHECK(!memcmp(want.data(), lds.dw.data(), want.size() * 4));
    // what no builder writes
    uint32_t bad[kPairDwords];
    memcpy(bad, slot, sizeof bad);
    bad[3] |= 1u;  // a flag in a positional half
    CHECK(decode_pair(bad, n_bins, a.data(), &na, b.data(), &nb, &got_index) == -2);
    memcpy(bad, slot, sizeof bad);
    put_half(bad, 2 * 70, (cnt_dwords(n_bins) + 63u) * 4u);  // the spare of another position, in line 2
    CHECK(decode_pair(bad, n_bins, a.data(), &na, b.data(), &nb, &got_index) == -2);
    if (nA >= 2 && kind != kDenseRows) {
        memcpy(bad, slot, sizeof bad);
        put_half(bad, 2, get_half(bad, 0));  // A[1] = A[0]: not ascending
        CHECK(decode_pair(bad, n_bins, a.data(), &na, b.data(), &nb, &got_index) == -2);
    }
    if (n_bins < cnt_dwords(n_bins)) {
        memcpy(bad, slot, sizeof bad);
        put_half(bad, 0, n_bins * 4u);  // a counter behind the last bin
        CHECK(decode_pair(bad, n_bins, a.data(), &na, b.data(), &nb, &got_index) == -2);
    }
}

int main()
{
    std::mt19937 rng(12345);
    static_assert(kind_of(96, 96) == kPlain && kind_of(97, 96) == kTail && kind_of(127, 127) == kTail && kind_of(128, 127) == kDenseRows, "the edges");
    static_assert(kind_of(128, 10) == kPlain && kind_of(10, 128) == kPlain && kind_of(128, 64) == kPlain && kind_of(129, 0) == kTail, "balance");
    static_assert(kind_of(0, 0) == kPlain && kind_of(190, 0) == kTail && kind_of(191, 0) == kDenseRows, "one list alone");
    static_assert(index_of(index_dword(0x2ABCDEF, true)) == 0x2ABCDEF && (index_dword(5, false) & kPairIndex) && !(index_dword(5, false) & kPairDense), "index");
    const uint32_t edges[][2] = {{0, 0},   {1, 0},    {0, 1},    {64, 64}, {65, 64},  {96, 95},  {96, 96},  {97, 96},  {96, 97},  {127, 127},
                                 {128, 127}, {128, 10}, {10, 128}, {128, 64}, {129, 0}, {190, 0}, {191, 0}, {0, 190}, {126, 64}, {64, 126},
                                 {300, 5},   {81, 81},  {100, 100}, {63, 130}};
    for (uint32_t n_bins : {8192u, 4090u, 4091u, 2112u})
        for (const auto &e : edges) round_trip(rng, e[0], e[1], n_bins);
    for (int i = 0; i < 400; ++i) round_trip(rng, rng() % 140, rng() % 140, 8192);
    for (uint32_t n : {0u, 40u, 81u, 96u, 97u, 127u, 128u}) round_trip(rng, n, n, 8192, true);  // a palindromic x: A = B, both counted
    // the census's verdicts
    {
        const uint64_t sampled = 65536;
        uint64_t over[3] = {0, 0, 0};
        CHECK(choose_lines(over, sampled) == kPairLines);
        over[0] = (sampled >> kPairTailShare) + kPairAlwaysDense;
        over[1] = (sampled >> kPairDenseShare) + kPairAlwaysDense;
        CHECK(choose_lines(over, sampled) == kPairLines);
        over[0] += 1;
        CHECK(choose_lines(over, sampled) == 0);
        over[0] -= 1, over[1] += 1;
        CHECK(choose_lines(over, sampled) == 0);
        const uint64_t small[3] = {2, 2, 0};  // k = 5: A^k and T^k alone
        CHECK(choose_lines(small, 1024) == kPairLines);
        CHECK(tail_capacity(1ull << 26) == (1ull << 22) + 64 && side_capacity(1ull << 26) == 2 * ((1ull << 17) + 64));
        CHECK(count_lds_bytes(8192) == 33024 + 4 * 128 + 64 && count_resident_workgroups(8192) == 4);
    }
    printf(g_fail ? "test_pair_lists: %d FAILED\n" : "test_pair_lists: all passed\n", g_fail);
    return g_fail ? 1 : 0;
}

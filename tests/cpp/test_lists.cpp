// test_lists.cpp -- the slot layout of the list table (readbouncer_amd/csrc/rb_lists.h) on a CPU: seeded dense rows go into a slot and
// come back as the same bins, rows of exactly capacity - 1, capacity, capacity + 1 and every bin included; an overflow slot names its
// side index and lists nothing; slots the builder never writes are told apart; the census picks the smallest slot size that at most one
// sampled row in 1024 overflows.  Built plain by tests/test_row_lists_cpu.py and with -fsanitize=address,undefined as well.
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "../../readbouncer_amd/csrc/rb_lists.h"

static int failures = 0;
#define CHECK(c)                                                                 \
    do {                                                                         \
        if (!(c)) { ++failures; std::fprintf(stderr, "%s:%d CHECK(%s) failed\n", __FILE__, __LINE__, #c); } \
    } while (0)

using namespace rblist;

static std::vector<uint64_t> row_with(std::mt19937_64 &rng, uint32_t n_words, uint32_t n_bins, uint32_t set)
{
    std::vector<uint32_t> bins(n_bins);
    for (uint32_t i = 0; i < n_bins; ++i) bins[i] = i;
    for (uint32_t i = 0; i < set; ++i) std::swap(bins[i], bins[i + rng() % (n_bins - i)]);
    std::vector<uint64_t> row(n_words, 0);
    for (uint32_t i = 0; i < set; ++i) row[bins[i] / 64] |= 1ull << (bins[i] % 64);
    return row;
}

static void round_trips()
{
    std::mt19937_64 rng(20261020);
    const uint32_t bins_of[4] = {8192, 4096, 4090, 2049};
    for (uint32_t lines : {1u, 2u, 4u}) {
        const uint32_t cap = slot_entries(lines);
        CHECK(cap == 64 * lines && slot_bytes(lines) == 128ull * lines && lines_valid(lines));
        for (uint32_t n_bins : bins_of) {
            const uint32_t n_words = (n_bins + 63) / 64;
            std::vector<uint32_t> sets = {0, 1, cap - 1, cap, cap + 1, n_bins};
            for (int i = 0; i < 40; ++i) sets.push_back((uint32_t)(rng() % (2 * cap)));
            for (uint32_t set : sets) {
                std::vector<uint64_t> row = row_with(rng, n_words, n_bins, set);
                row[n_words - 1] |= (n_bins % 64) ? ~0ull << (n_bins % 64) : 0;  // pad bits list nothing
                std::vector<uint16_t> slot(cap), bins(cap);
                const uint32_t side = (uint32_t)(rng() % (1u << 20));
                uint32_t got_side = ~0u;
                const bool fits = encode_slot(row.data(), n_words, n_bins, lines, side, slot.data());
                CHECK(fits == (set <= cap));
                const int n = decode_slot(slot.data(), lines, bins.data(), &got_side);
                if (!fits) {
                    CHECK(n == -1 && got_side == side && slot[0] == kOverflowMark);
                    continue;
                }
                CHECK(n == (int)set);
                std::vector<uint64_t> back(n_words, 0);
                for (int i = 0; i < n; ++i) back[bins[i] / 64] |= 1ull << (bins[i] % 64);
                if (n_bins % 64) row[n_words - 1] &= (1ull << (n_bins % 64)) - 1;
                CHECK(back == row);
                for (uint32_t i = set; i < cap; ++i) CHECK(slot[i] == kSentinel);
            }
        }
    }
    CHECK(!lines_valid(0) && !lines_valid(3) && !lines_valid(8));
}

static void malformed()
{
    std::vector<uint16_t> slot(128, kSentinel), bins(128);
    uint32_t side = 0;
    CHECK(decode_slot(slot.data(), 2, bins.data(), &side) == 0);
    slot[0] = 5, slot[1] = 5;
    CHECK(decode_slot(slot.data(), 2, bins.data(), &side) == -2);  // not ascending
    slot[1] = kSentinel, slot[2] = 9;
    CHECK(decode_slot(slot.data(), 2, bins.data(), &side) == -2);  // a bin behind a sentinel
    slot[2] = kSentinel, slot[0] = (uint16_t)kMaxBins;
    CHECK(decode_slot(slot.data(), 2, bins.data(), &side) == -2);  // no such bin
    slot[0] = 3, slot[1] = kOverflowMark;
    CHECK(decode_slot(slot.data(), 2, bins.data(), &side) == -2);  // the mark is the first entry or nothing
    slot[0] = kOverflowMark, slot[1] = 0x1234, slot[2] = 0x0005;
    CHECK(decode_slot(slot.data(), 2, bins.data(), &side) == -1 && side == 0x51234u);
    slot[7] = 1;
    CHECK(decode_slot(slot.data(), 2, bins.data(), &side) == -2);
    CHECK(kMaxBins <= kOverflowMark && kOverflowMark < kSentinel);
}

static void census()
{
    const uint64_t none[3] = {0, 0, 0}, a[3] = {64, 0, 0}, b[3] = {65, 64, 0}, c[3] = {65536, 65, 64}, d[3] = {65536, 65536, 65};
    CHECK(choose_lines(none, 65536) == 1 && choose_lines(a, 65536) == 1 && choose_lines(b, 65536) == 2 && choose_lines(c, 65536) == 4);
    CHECK(choose_lines(d, 65536) == 0);
    const uint64_t one[3] = {1, 1, 1};
    CHECK(choose_lines(one, 1024) == 1 && choose_lines(one, 1023) == 0);  // a sample below 1024 rows allows no overflow at all
    CHECK(side_capacity(1ull << 26) == (1ull << 17) + 64 && side_capacity(1024) == 66 && side_capacity(16384) == 96);
}

// what a wave of the count kernel keeps in LDS: room for every counter half, the spares and the staged bases, and what a CU then holds.
// The lines it prints are what tests/test_row_lists_cpu.py sets beside the compiler's resource remarks.
static void count_lds()
{
    for (uint32_t n_bins : {2049u, 2112u, 4090u, 4096u, 8191u, 8192u}) {
        const uint32_t dwords = count_cnt_dwords(n_bins), bytes = count_lds_bytes(n_bins);
        CHECK(dwords % 256 == 0 && 2 * dwords >= n_bins && 2 * dwords < n_bins + 512);  // a counter half for every bin, rounded up to 1 KiB
        CHECK(bytes == dwords * 4 + kCountSpareDwords * 4 + kCountStageBytes);
        CHECK(kCountSpareDwords >= 64);                   // a spare dword for every lane of the wave
        CHECK(kCountStageBytes >= 64 + 13 - 1);           // a tile's bases at k <= 13
        CHECK(bytes % 16 == 0);                           // the counters and spares are cleared sixteen bytes at a time
        CHECK(count_resident_workgroups(n_bins) * bytes <= kLdsPerCuBytes);
        std::printf("count_lds n_bins %u bytes %u resident %u\n", n_bins, bytes, count_resident_workgroups(n_bins));
    }
    CHECK(kLdsPerCuBytes == 160 * 1024);
    CHECK(count_lds_bytes(8192) == 16768 && count_resident_workgroups(8192) == 9);
    CHECK(count_lds_bytes(4096) == 8576 && count_lds_bytes(4090) == 8576 && count_resident_workgroups(4096) == 19);
    CHECK(count_lds_bytes(kMaxBins) <= 64 * 1024);        // what one workgroup may ask for
}

int main()
{
    round_trips();
    malformed();
    census();
    count_lds();
    std::printf("failures: %d\n", failures);
    return failures ? 1 : 0;
}

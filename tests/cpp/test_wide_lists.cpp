// test_wide_lists.cpp -- the slot layout of a filter's WIDE list table (readbouncer_amd/csrc/rb_wide_lists.h) on a CPU: the arithmetic
// of kWideMaxBins, the LDS bytes and resident workgroups; canonical -> resident -> canonical at every offered slot size for rows that are
// empty, random, all even, all odd, exactly cap, cap + 1 (overflow) and parity-tilted (swapped halves); where every offset points; a host
// emulation of what wide_batch (rb_wide_lists.hip) does with a slot, whose counters must be the row's bits; and the malformed slots that
// decode_resident must refuse.  Built plain and with -fsanitize=address,undefined by tests/test_wide_lists_cpu.py.
#include <cstdint>
#include <cstdio>
#include <random>
#include <set>
#include <vector>

#include "../../readbouncer_amd/csrc/rb_wide_lists.h"

static int failures = 0;
#define CHECK(c)                                                                 \
    do {                                                                         \
        if (!(c)) { ++failures; std::fprintf(stderr, "%s:%d CHECK(%s) failed\n", __FILE__, __LINE__, #c); } \
    } while (0)

using namespace rbwide;

static const uint32_t kBins[] = {8193u, 8256u, 31000u, 32256u};

static void arithmetic()
{
    CHECK(kWideMaxBins == 32256 && kWideMinBins == 8193 && kWideMaxWords == 504 && kWideMaxCntDwords == 16128);
    CHECK((kWideMaxCntDwords + kWideSpareDwords) * 4 == 64768 && 64768 <= 65536);  // counters and spares end within 64 KiB
    CHECK(cnt_dwords(32256) == 16128 && cnt_dwords(32257) == 16384);               // one more bin, one more KiB: offsets no longer fit
    CHECK((cnt_dwords(32257) + kWideSpareDwords) * 4 > kResidentOffset + 4);
    CHECK(bins_served(8193) && bins_served(32256) && !bins_served(8192) && !bins_served(32257) && !bins_served(0));
    CHECK(lines_valid(4) && lines_valid(6) && lines_valid(8) && !lines_valid(0) && !lines_valid(1) && !lines_valid(2) && !lines_valid(5) && !lines_valid(16));
    CHECK(cnt_dwords(8193) == 4352 && cnt_dwords(8256) == 4352 && cnt_dwords(31000) == 15616);
    // LDS: counters, 64 spares, a stage per wave, the partial maxima
    CHECK(count_lds_bytes(32256, 4) == 64512 + 256 + 512 + 64 && count_lds_bytes(32256, 4) <= 65536);
    CHECK(count_lds_bytes(31000, 4) == 62464 + 256 + 512 + 64);
    CHECK(count_lds_bytes(32256, 1) == 64512 + 256 + 128 + 64);
    for (uint32_t n_bins : kBins) {
        const uint32_t b = count_lds_bytes(n_bins), r = count_resident_workgroups(n_bins);
        CHECK(r >= 2 && b * r <= rblist::kLdsPerCuBytes && b * (r + 1) > rblist::kLdsPerCuBytes);
        std::printf("wide_count_lds n_bins %u bytes %u resident %u\n", n_bins, b, r);
    }
    CHECK(count_resident_workgroups(32256) == 2 && count_resident_workgroups(31000) == 2 && count_resident_workgroups(8193) == 8);
    for (uint32_t lines : kWideLines) {
        CHECK(slot_entries(lines) == 64 * lines && slot_dwords(lines) == 32 * lines && slot_bytes(lines) == 128ull * lines);
        CHECK(lane_dwords(lines) * 64 == slot_dwords(lines));  // a whole number of dwords per lane: one load
    }
    CHECK((1ull << 26) * slot_bytes(8) == 64ull << 30 && (1ull << 26) * slot_bytes(6) == 48ull << 30);  // beyond 2^32 and 2^35
    // the census rule: the smallest slot that at most one sampled row in 1024 overflows
    const uint64_t none[3] = {0, 0, 0}, first[3] = {65, 64, 0}, second[3] = {9000, 65, 64}, dense[3] = {9000, 9000, 65};
    CHECK(choose_lines(none, 65536) == 4 && choose_lines(first, 65536) == 6 && choose_lines(second, 65536) == 8 && choose_lines(dense, 65536) == 0);
    const uint64_t small[3] = {2, 1, 0};
    CHECK(choose_lines(small, 1024) == 6 && choose_lines(small, 2048) == 4);
}

// `set` bins of which `even` are even (even > set: no matter which), as a dense row
static std::vector<uint64_t> row_with(std::mt19937_64 &rng, uint32_t n_words, uint32_t n_bins, uint32_t set, uint32_t even)
{
    std::vector<uint32_t> pool[2];
    for (uint32_t i = 0; i < n_bins; ++i) pool[i & 1].push_back(i);
    std::vector<uint64_t> row(n_words, 0);
    auto take = [&](std::vector<uint32_t> &from) {
        const size_t at = rng() % from.size();
        row[from[at] / 64] |= 1ull << (from[at] % 64);
        from[at] = from.back();
        from.pop_back();
    };
    for (uint32_t i = 0; i < set; ++i) {
        if (even <= set) take(pool[i < even ? 0 : 1]);
        else take(pool[(pool[0].empty() || (!pool[1].empty() && (rng() & 1))) ? 1 : 0]);
    }
    return row;
}

// What a wave does with one slot (wide_batch), on counters laid out as count_lds_bytes says: lane l holds dwords DW l .. DW l + DW - 1
static void emulate(const uint32_t *slot, uint32_t lines, uint32_t n_bins, const uint64_t *dense, std::vector<uint32_t> &lds)
{
    const uint32_t half = slot_entries(lines) / 2, cnt = cnt_dwords(n_bins), dw = lane_dwords(lines);
    std::vector<uint32_t> v(slot, slot + half);
    uint32_t fold = 0;
    for (uint32_t d = 0; d < half; ++d) fold |= v[d];
    auto add = [&](uint32_t off, uint32_t what) {
        CHECK(off % 4 == 0 && off + 4 <= (cnt + kWideSpareDwords) * 4);
        if (off + 4 <= lds.size() * 4) lds[off / 4] += what;
    };
    if (fold & kResidentFlags) {  // the careful path
        if (v[0] & kResidentOverflow) {
            for (uint32_t d = 0; d < half; ++d) v[d] = ((cnt + d / dw) * 4u) * 0x10001u;
            for (uint32_t bin = 0; bin < n_bins; ++bin)
                if ((dense[bin / 64] >> (bin % 64)) & 1ull) lds[bin >> 1] += 1u << (16 * (bin & 1));
        } else {
            for (uint32_t d = 0; d < half; ++d) {
                const uint32_t spare_off = (cnt + d / dw) * 4u;
                if (v[d] & kResidentSwapped) {
                    add(v[d] & kResidentOffset, 0x10000u);
                    v[d] = (v[d] & 0xFFFF0000u) | spare_off;
                }
                if (v[d] & (kResidentSwapped << 16)) {
                    add((v[d] >> 16) & kResidentOffset, 1u);
                    v[d] = (v[d] & 0x0000FFFFu) | (spare_off << 16);
                }
            }
        }
    }
    for (uint32_t d = 0; d < half; ++d) {  // the two-instruction path: no flag may be left
        CHECK(!(v[d] & kResidentFlags));
        add(v[d] & 0xFFFFu, 1u);
        add(v[d] >> 16, 0x10000u);
    }
}

static void one_row(const std::vector<uint64_t> &row, uint32_t n_words, uint32_t n_bins, uint32_t lines, uint32_t side)
{
    const uint32_t cap = slot_entries(lines), half = cap / 2, cnt = cnt_dwords(n_bins);
    uint32_t n_par[2] = {0, 0};
    for (uint32_t bin = 0; bin < n_bins; ++bin)
        if ((row[bin / 64] >> (bin % 64)) & 1ull) ++n_par[bin & 1];
    const uint32_t set = n_par[0] + n_par[1];
    std::vector<uint16_t> canon(cap), back(cap, 7), bins(cap);
    std::vector<uint32_t> res(half, 0);
    const bool fits = encode_slot(row.data(), n_words, n_bins, lines, side, canon.data());
    CHECK(fits == (set <= cap));
    uint32_t side_back = ~0u;
    CHECK(decode_slot(canon.data(), lines, n_bins, bins.data(), &side_back) == (fits ? (int)set : -1));
    if (!fits) CHECK(side_back == side);
    CHECK(encode_resident(canon.data(), lines, n_bins, res.data()));
    // ---- round trip
    const int n = decode_resident(res.data(), lines, n_bins, back.data());
    CHECK(n == (fits ? (int)set : -1));
    CHECK(back == canon);
    // ---- offsets, spares and the flag word
    uint32_t fold = 0;
    for (uint32_t d = 0; d < half; ++d) {
        if (!fits && d == 1) continue;  // the side index, whole
        fold |= res[d];
        for (uint32_t pos = 0; pos < 2; ++pos) {
            const uint32_t h = (res[d] >> (16 * pos)) & 0xFFFFu, off = h & kResidentOffset;
            CHECK(off % 4 == 0 && off + 4 <= (cnt + kWideSpareDwords) * 4 && off + 4 <= 65536);
            if (off / 4 >= cnt) CHECK(off / 4 == resident_spare_dword(n_bins, lines, d) && !(h & kResidentSwapped));
            else CHECK(fits && off / 4 * 2 + (pos ^ (h & kResidentSwapped)) < n_bins);
        }
    }
    if (!fits) CHECK(res[1] == side && (res[0] & kResidentFlags) == kResidentOverflow);
    CHECK(((fold & kResidentFlags) == 0) == (fits && n_par[0] <= half && n_par[1] <= half));  // zero exactly when balanced and fitting
    // ---- what the kernel's adds make of it, three times over: every listed bin counts 3, every other bin 0
    std::vector<uint32_t> lds(count_lds_bytes(n_bins) / 4, 0);
    for (int rep = 0; rep < 3; ++rep) emulate(res.data(), lines, n_bins, row.data(), lds);
    bool same = true;
    for (uint32_t bin = 0; bin < 2 * cnt; ++bin) {
        const uint32_t got = (lds[bin >> 1] >> (16 * (bin & 1))) & 0xFFFFu;
        const bool is_set = bin < n_bins && ((row[bin / 64] >> (bin % 64)) & 1ull);
        same = same && got == (is_set ? 3u : 0u);
    }
    CHECK(same);
    for (uint32_t i = cnt + kWideSpareDwords; i < lds.size(); ++i) CHECK(lds[i] == 0);  // stages and partial maxima are not touched
}

static void rows()
{
    std::mt19937_64 rng(20261021);
    for (uint32_t lines : kWideLines) {
        const uint32_t cap = slot_entries(lines), big = cap * 70 / 128;
        for (uint32_t n_bins : kBins) {
            const uint32_t n_words = (n_bins + 63) / 64;
            for (uint32_t set : {0u, 1u, 2u, 63u, 64u, 65u, cap / 2 - 1, cap / 2, cap / 2 + 1, cap - 1, cap, cap + 1, cap + 70}) {
                one_row(row_with(rng, n_words, n_bins, set, ~0u), n_words, n_bins, lines, (uint32_t)(rng() % (1u << 20)));  // random
                one_row(row_with(rng, n_words, n_bins, set, set), n_words, n_bins, lines, (uint32_t)rng());                // all even
                one_row(row_with(rng, n_words, n_bins, set, 0), n_words, n_bins, lines, 3);                               // all odd
            }
            one_row(row_with(rng, n_words, n_bins, cap, big), n_words, n_bins, lines, 0);        // exactly cap, tilted both ways
            one_row(row_with(rng, n_words, n_bins, cap, cap - big), n_words, n_bins, lines, 0);
            one_row(row_with(rng, n_words, n_bins, cap - 5, big), n_words, n_bins, lines, 0);
            one_row(std::vector<uint64_t>(n_words, 0), n_words, n_bins, lines, 0);               // the empty row
            std::vector<uint64_t> last(n_words, 0);                                              // the last bin alone, and the first
            last[(n_bins - 1) / 64] |= 1ull << ((n_bins - 1) % 64);
            last[0] |= 1ull;
            one_row(last, n_words, n_bins, lines, 0);
            std::vector<uint64_t> pad(n_words, 0);                                               // pad bits list nothing
            if (n_bins % 64) pad[n_words - 1] = ~0ull << (n_bins % 64);
            one_row(pad, n_words, n_bins, lines, 0);
        }
    }
}

// no two lanes of one add instruction share a spare: an instruction is dword `which` of every lane's share and one half of it
static void spares()
{
    for (uint32_t lines : kWideLines)
        for (uint32_t n_bins : kBins) {
            const uint32_t per_lane = lane_dwords(lines);
            for (uint32_t which = 0; which < per_lane; ++which) {
                std::set<uint32_t> seen;
                for (uint32_t lane = 0; lane < 64; ++lane) {
                    const uint32_t s = resident_spare_dword(n_bins, lines, lane * per_lane + which);
                    CHECK(s == cnt_dwords(n_bins) + lane);  // the lane's own: what wide_batch blanks a slot to
                    CHECK(s * 4 + 4 <= 65536);
                    seen.insert(s);
                }
                CHECK(seen.size() == 64);
            }
        }
}

// (the malformed slots of test_lists.cpp / test_lists_resident.cpp, at a wide size)
static void malformed()
{
    const uint32_t n_bins = 31000, lines = 6, cap = slot_entries(lines);
    std::vector<uint16_t> canon(cap, kSentinel), back(cap), bins(cap);
    std::vector<uint32_t> res(cap / 2);
    uint32_t side = 0;
    canon[0] = 4, canon[1] = 9, canon[2] = 30999;
    CHECK(decode_slot(canon.data(), lines, n_bins, bins.data(), &side) == 3);
    CHECK(encode_resident(canon.data(), lines, n_bins, res.data()) && decode_resident(res.data(), lines, n_bins, back.data()) == 3);
    std::vector<uint16_t> c2 = canon;
    c2[1] = 4;  // not ascending
    CHECK(decode_slot(c2.data(), lines, n_bins, bins.data(), &side) == -2);
    c2 = canon, c2[5] = 100;  // a bin behind a sentinel
    CHECK(decode_slot(c2.data(), lines, n_bins, bins.data(), &side) == -2);
    c2 = canon, c2[2] = 31000;  // not a bin
    CHECK(decode_slot(c2.data(), lines, n_bins, bins.data(), &side) == -2);
    c2 = canon, c2[2] = kOverflowMark;  // a mark in the wrong place
    CHECK(decode_slot(c2.data(), lines, n_bins, bins.data(), &side) == -2);
    c2.assign(cap, kSentinel), c2[0] = kOverflowMark, c2[1] = 7, c2[2] = 1;
    CHECK(decode_slot(c2.data(), lines, n_bins, bins.data(), &side) == -1 && side == 65543);
    c2[3] = 5;  // an overflow slot holds nothing else
    CHECK(decode_slot(c2.data(), lines, n_bins, bins.data(), &side) == -2);
    std::vector<uint32_t> bad = res;
    bad[5] = (bad[5] & 0xFFFF0000u) | (resident_spare_dword(n_bins, lines, 9) * 4);  // another lane's spare
    CHECK(decode_resident(bad.data(), lines, n_bins, back.data()) == -2);
    bad = res, bad[7] = (bad[7] & 0xFFFF0000u) | 8u;  // bin 4 again
    CHECK(decode_resident(bad.data(), lines, n_bins, back.data()) == -2);
    bad = res, bad[7] = (bad[7] & 0x0000FFFFu) | ((30996u / 2 * 4) << 16);  // bin 30997, a fourth
    CHECK(decode_resident(bad.data(), lines, n_bins, back.data()) == 4);
    bad[8] = (bad[8] & 0x0000FFFFu) | ((31000u / 2 * 4) << 16);  // bin 31001 lies in the counters' pad: not a bin
    CHECK(decode_resident(bad.data(), lines, n_bins, back.data()) == -2);
    bad = res, bad[3] |= kResidentOverflow;  // the flag belongs to dword 0
    CHECK(decode_resident(bad.data(), lines, n_bins, back.data()) == -2);
    bad = res, bad[0] |= kResidentOverflow;  // an overflow slot lists nothing
    CHECK(decode_resident(bad.data(), lines, n_bins, back.data()) == -2);
    canon[0] = (uint16_t)n_bins;
    CHECK(!encode_resident(canon.data(), lines, n_bins, res.data()));
}

int main()
{
    arithmetic();
    rows();
    spares();
    malformed();
    std::printf("failures: %d\n", failures);
    return failures ? 1 : 0;
}

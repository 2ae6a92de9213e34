// test_lists_resident.cpp -- the RESIDENT form of a list-table slot (readbouncer_amd/csrc/rb_lists.h: each half of a dword a ready LDS
// byte offset, parity by position, spares for the halves that list nothing, two flag bits) on a CPU: canonical -> resident -> canonical
// for every population 0 .. cap + 1 at every slot size and several bin counts, with random, one-parity, unbalanced and empty rows; where
// every offset points; when a slot carries a flag; and a host emulation of what list_batch (rb_lists_device.h) does with a slot -- the
// two-instruction path for a slot without a flag, the careful path for the others -- whose counters must be the row's bits.
// Built plain and with -fsanitize=address,undefined by tests/test_list_addready_cpu.py.
#include <cstdint>
#include <cstdio>
#include <random>
#include <set>
#include <vector>

#include "../../readbouncer_amd/csrc/rb_lists.h"

static int failures = 0;
#define CHECK(c)                                                                 \
    do {                                                                         \
        if (!(c)) { ++failures; std::fprintf(stderr, "%s:%d CHECK(%s) failed\n", __FILE__, __LINE__, #c); } \
    } while (0)

using namespace rblist;

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

// the lane that holds dword `d` of a slot, and which of its dwords it is (list_batch: lane_dword)
static uint32_t lane_of(uint32_t lines, uint32_t d) { return lines == 4 ? d >> 1 : d; }

// What a wave does with one slot, on counters laid out as count_lds_bytes says.  The two-instruction path may only see a slot without
// a flag; the careful path blanks an overflow slot and counts its dense row, and adds swapped halves with the other constant.
static void emulate(const uint32_t *slot, uint32_t lines, uint32_t n_bins, const uint64_t *dense, std::vector<uint32_t> &lds)
{
    const uint32_t half = slot_entries(lines) / 2, cnt_dwords = count_cnt_dwords(n_bins);
    std::vector<uint32_t> v(slot, slot + half);
    uint32_t fold = 0;
    for (uint32_t d = 0; d < half; ++d) fold |= v[d];
    auto add = [&](uint32_t off, uint32_t what) {
        CHECK(off % 4 == 0 && off + 4 <= (cnt_dwords + kCountSpareDwords) * 4);
        if (off + 4 <= lds.size() * 4) lds[off / 4] += what;
    };
    if (fold & kResidentFlags) {  // the careful path
        if (v[0] & kResidentOverflow) {
            for (uint32_t d = 0; d < half; ++d) v[d] = ((cnt_dwords + lane_of(lines, d)) * 4u) * 0x10001u;
            for (uint32_t bin = 0; bin < n_bins; ++bin)
                if ((dense[bin / 64] >> (bin % 64)) & 1ull) lds[bin >> 1] += 1u << (16 * (bin & 1));
        } else {
            for (uint32_t d = 0; d < half; ++d) {
                const uint32_t spare_off = (cnt_dwords + lane_of(lines, d)) * 4u;
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
    const uint32_t cap = slot_entries(lines), half = cap / 2, cnt_dwords = count_cnt_dwords(n_bins);
    uint32_t n_par[2] = {0, 0};
    for (uint32_t bin = 0; bin < n_bins; ++bin)
        if ((row[bin / 64] >> (bin % 64)) & 1ull) ++n_par[bin & 1];
    const uint32_t set = n_par[0] + n_par[1];
    std::vector<uint16_t> canon(cap), back(cap, 7);
    std::vector<uint32_t> res(half, 0);
    const bool fits = encode_slot(row.data(), n_words, n_bins, lines, side, canon.data());
    CHECK(fits == (set <= cap));
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
            CHECK(off % 4 == 0 && off < count_lds_bytes(n_bins) && off + 4 <= (cnt_dwords + kCountSpareDwords) * 4);
            if (off / 4 >= cnt_dwords) CHECK(off / 4 == resident_spare_dword(n_bins, lines, d) && !(h & kResidentSwapped));
            else CHECK(fits && off / 4 * 2 + (pos ^ (h & kResidentSwapped)) < n_bins);
        }
    }
    if (!fits) CHECK(res[1] == side && (res[0] & kResidentFlags) == kResidentOverflow);
    CHECK(((fold & kResidentFlags) == 0) == (fits && n_par[0] <= half && n_par[1] <= half));  // zero exactly when balanced and fitting
    // ---- what the kernel's adds make of it, three times over: every listed bin counts 3, every other bin 0
    std::vector<uint32_t> lds(count_lds_bytes(n_bins) / 4, 0);
    for (int rep = 0; rep < 3; ++rep) emulate(res.data(), lines, n_bins, row.data(), lds);
    bool same = true;
    for (uint32_t bin = 0; bin < 2 * cnt_dwords; ++bin) {
        const uint32_t got = (lds[bin >> 1] >> (16 * (bin & 1))) & 0xFFFFu;
        const bool is_set = bin < n_bins && ((row[bin / 64] >> (bin % 64)) & 1ull);
        same = same && got == (is_set ? 3u : 0u);
    }
    CHECK(same);
    for (uint32_t i = (cnt_dwords + kCountSpareDwords); i < lds.size(); ++i) CHECK(lds[i] == 0);  // the staged bases are not touched
}

static void rows()
{
    std::mt19937_64 rng(20261020);
    for (uint32_t lines : {1u, 2u, 4u}) {
        const uint32_t cap = slot_entries(lines), big = cap * 70 / 128;  // 70 / 58 of a two-line slot, in proportion
        for (uint32_t n_bins : {8192u, 4096u, 4090u, 2112u}) {
            const uint32_t n_words = (n_bins + 63) / 64;
            for (uint32_t set = 0; set <= cap + 1; ++set) {
                one_row(row_with(rng, n_words, n_bins, set, ~0u), n_words, n_bins, lines, (uint32_t)(rng() % (1u << 20)));  // random
                one_row(row_with(rng, n_words, n_bins, set, set), n_words, n_bins, lines, (uint32_t)rng());                // all even
                one_row(row_with(rng, n_words, n_bins, set, 0), n_words, n_bins, lines, 3);                               // all odd
            }
            one_row(row_with(rng, n_words, n_bins, cap, big), n_words, n_bins, lines, 0);        // exactly cap, unbalanced both ways
            one_row(row_with(rng, n_words, n_bins, cap, cap - big), n_words, n_bins, lines, 0);
            one_row(std::vector<uint64_t>(n_words, 0), n_words, n_bins, lines, 0);               // the empty row
            std::vector<uint64_t> pad(n_words, 0);                                              // pad bits list nothing
            if (n_bins % 64) pad[n_words - 1] = ~0ull << (n_bins % 64);
            one_row(pad, n_words, n_bins, lines, 0);
        }
    }
}

// no two lanes of one add instruction share a spare: an instruction is one dword of every lane's (the first or the second of a four-line
// slot) and one half of it; lanes 32-63 of a one-line slot sit out
static void spares()
{
    for (uint32_t lines : {1u, 2u, 4u})
        for (uint32_t n_bins : {8192u, 4096u, 4090u, 2112u}) {
            const uint32_t half = slot_entries(lines) / 2, per_lane = lines == 4 ? 2 : 1, lanes = half / per_lane;
            CHECK(lanes == (lines == 1 ? 32u : 64u));
            for (uint32_t which = 0; which < per_lane; ++which) {
                std::set<uint32_t> seen;
                for (uint32_t lane = 0; lane < lanes; ++lane) {
                    const uint32_t s = resident_spare_dword(n_bins, lines, lane * per_lane + which);
                    CHECK(s == count_cnt_dwords(n_bins) + lane);  // the lane's own: what list_batch blanks a slot to
                    CHECK(s >= count_cnt_dwords(n_bins) && s < count_cnt_dwords(n_bins) + kCountSpareDwords);
                    seen.insert(s);
                }
                CHECK(seen.size() == lanes);
            }
        }
}

static void malformed()
{
    const uint32_t n_bins = 4090, lines = 2;
    std::vector<uint16_t> canon(128, kSentinel), back(128);
    std::vector<uint32_t> res(64);
    canon[0] = 4, canon[1] = 9;
    CHECK(encode_resident(canon.data(), lines, n_bins, res.data()) && decode_resident(res.data(), lines, n_bins, back.data()) == 2);
    std::vector<uint32_t> bad = res;
    bad[5] = (bad[5] & 0xFFFF0000u) | (resident_spare_dword(n_bins, lines, 6) * 4);  // another dword's spare
    CHECK(decode_resident(bad.data(), lines, n_bins, back.data()) == -2);
    bad = res, bad[7] = (bad[7] & 0xFFFF0000u) | 8u;  // bin 4 again
    CHECK(decode_resident(bad.data(), lines, n_bins, back.data()) == -2);
    bad = res, bad[7] = (bad[7] & 0x0000FFFFu) | ((4088u / 2 * 4) << 16);  // bin 4089 is the last; 4091 is not one
    CHECK(decode_resident(bad.data(), lines, n_bins, back.data()) == 3);
    bad[8] = (bad[8] & 0x0000FFFFu) | ((4090u / 2 * 4) << 16);
    CHECK(decode_resident(bad.data(), lines, n_bins, back.data()) == -2);
    bad = res, bad[3] |= kResidentOverflow;  // the flag belongs to dword 0
    CHECK(decode_resident(bad.data(), lines, n_bins, back.data()) == -2);
    canon[0] = (uint16_t)n_bins;
    CHECK(!encode_resident(canon.data(), lines, n_bins, res.data()));
}

int main()
{
    rows();
    spares();
    malformed();
    std::printf("failures: %d\n", failures);
    return failures ? 1 : 0;
}

// rb_wide_lists.h -- the slot layout of a filter's WIDE LIST TABLE (rb_dibf_wide_list_table_build; rb_wide_lists.hip,
// ibf_count_wide_lists_kernel), shared by the kernels, the engine and the tests.  No HIP in here: tests/cpp/test_wide_lists.cpp compiles
// it alone, plain and with sanitizers.
//
// The list table of rb_lists.h ends at 8192 bins and blocks of 128 words.  This is the same idea for filters of 8193 to kWideMaxBins bins
// (blocks of up to 504 words): one SLOT per N-free k-mer (the rank of the row table), a slot is `lines` lines of 128 bytes, lines in
// kWideLines = {4, 6, 8}, the same for every slot of a table, and holds up to 64 x lines entries of 16 bits.  The CANONICAL form is
// rb_lists.h's: the row's bin numbers ascending, then kSentinel; an overflow slot is kOverflowMark and the two halves of the index of
// its dense row (`stride` words) in the side table.  Bin numbers are below kWideMaxBins < kOverflowMark, so neither mark is a bin.
// The device keeps the RESIDENT ("add-ready") form, generalised from rb_lists.h: each 16-bit half of a dword is, in bits 15:2, the LDS
// byte offset of a counter dword (dword bin >> 1 from offset 0), its position is the bin's parity, bits 1:0 are the flags
// kResidentSwapped / kResidentOverflow with rb_lists.h's meaning, and a half that lists no bin names a spare dword behind the counters.
// Why 4, 6 and 8 lines: a filter sized for a false-positive rate of 1 % sets about 1 % of a row's bits, so a row of n bins lists
// n / 100 bins with a standard deviation of its root; mean + 4 sigma fits 4 lines (256 entries) up to about 20 000 bins, 6 lines (384)
// up to about 31 000 -- the GRCh38 filter at the default fragment size -- and 8 lines (512) to kWideMaxBins and for filters denser than
// their design.  Each is a whole number of dwords per lane of a wave (2, 3, 4), so a lane fetches its share of a slot with ONE load.
#pragma once
#include <cstdint>

#include "rb_lists.h"

namespace rbwide {

using rblist::kEntriesPerLine;
using rblist::kLineBytes;
using rblist::kOverflowMark;
using rblist::kSentinel;
using rblist::kResidentFlags;
using rblist::kResidentOffset;
using rblist::kResidentOverflow;
using rblist::kResidentSwapped;

constexpr uint32_t kWideSizes = 3;
constexpr uint32_t kWideLines[kWideSizes] = {4, 6, 8};
constexpr uint32_t kWideMaxLines = 8;
constexpr uint32_t kWideMinBins = rblist::kMaxBins + 1;  // what rb_lists.h serves stays there
constexpr uint32_t kWideMaxKmers = rblist::kMaxKmers;    // per strand: a bin's count fits its 16-bit counter
constexpr uint32_t kWideSpareDwords = 64;                // one per lane, shared by the waves of a workgroup
constexpr uint32_t kWideStageBytes = 128;                // per WAVE: the bases of the tile it has in hand (64 + k - 1 <= 76)
constexpr uint32_t kWideReduceBytes = 64;                // the waves' partial maxima
constexpr uint32_t kWideWaves = 4;                       // waves per workgroup the engine launches

constexpr uint32_t cnt_dwords(uint32_t n_bins) { return rblist::count_cnt_dwords(n_bins); }

// Offsets are 16 bits with two flag bits: counters and spares end within 64 KiB, the counters are whole multiples of 256 dwords.
constexpr uint32_t kWideMaxCntDwords = ((kResidentOffset + 4u) / 4u - kWideSpareDwords) & ~255u;  // 16 128
constexpr uint32_t kWideMaxBins = kWideMaxCntDwords * 2u;                                         // 32 256
static_assert(kWideMaxCntDwords == 16128 && kWideMaxBins == 32256, "64 KiB of offsets less 64 spares, in whole 1 KiB pieces");
static_assert(cnt_dwords(kWideMaxBins) == kWideMaxCntDwords && cnt_dwords(kWideMaxBins + 1) > kWideMaxCntDwords, "the last bin count that fits");
static_assert((cnt_dwords(kWideMaxBins) + kWideSpareDwords) * 4u <= kResidentOffset + 4u, "a spare's byte offset fits bits 15:2 of a half");
static_assert(kWideMaxBins < kOverflowMark, "no bin is a mark");
constexpr uint32_t kWideMaxWords = (kWideMaxBins + 63u) / 64u;  // 504

constexpr bool lines_valid(uint32_t lines) { return lines == 4 || lines == 6 || lines == 8; }
constexpr uint32_t slot_entries(uint32_t lines) { return lines * kEntriesPerLine; }
constexpr uint32_t slot_dwords(uint32_t lines) { return lines * (kLineBytes / 4u); }
constexpr uint64_t slot_bytes(uint32_t lines) { return (uint64_t)lines * kLineBytes; }
constexpr uint32_t lane_dwords(uint32_t lines) { return lines / 2u; }  // of a slot, per lane of the wave that gathers it
constexpr bool bins_served(uint64_t n_bins) { return n_bins >= kWideMinBins && n_bins <= kWideMaxBins; }

constexpr uint64_t side_capacity(uint64_t n_rows) { return rblist::side_capacity(n_rows); }

// What a workgroup of `waves` waves of ibf_count_wide_lists_kernel keeps in LDS: the counters, the spares, a stage per wave and the
// waves' partial maxima.  65 344 bytes at kWideMaxBins and four waves: below 64 KiB, two workgroups to a CU.
constexpr uint32_t count_lds_bytes(uint32_t n_bins, uint32_t waves = kWideWaves)
{
    return (cnt_dwords(n_bins) + kWideSpareDwords) * 4u + waves * kWideStageBytes + kWideReduceBytes;
}
constexpr uint32_t count_resident_workgroups(uint32_t n_bins, uint32_t waves = kWideWaves)
{
    return rblist::kLdsPerCuBytes / count_lds_bytes(n_bins, waves);
}
static_assert(count_lds_bytes(kWideMaxBins) <= 64u * 1024u, "no more than a workgroup may declare without asking");
// ... and a workgroup of the wide forms of locate and hits (rb_wide_pass_lists.hip): the same areas and nothing more -- their hit mask
// lives in registers, and what the waves exchange goes through the partial maxima's 64 bytes
constexpr uint32_t pass_lds_bytes(uint32_t n_bins, uint32_t waves = kWideWaves) { return count_lds_bytes(n_bins, waves); }
// How their scans share the counters: cnt_dwords / 256 rounds of 64 consecutive 16-byte pieces (512 bins), wave w at the rounds
// [w x per, (w + 1) x per) that exist.  A thread keeps one mask byte per round of its wave: per <= kWidePassMaskBytes.
constexpr uint32_t kWidePassMaskBytes = 16;
constexpr uint32_t pass_rounds(uint32_t n_bins) { return cnt_dwords(n_bins) / 256u; }
constexpr uint32_t pass_rounds_per_wave(uint32_t n_bins, uint32_t waves = kWideWaves) { return (pass_rounds(n_bins) + waves - 1u) / waves; }
constexpr uint32_t pass_wave_of_bin(uint32_t n_bins, uint32_t bin, uint32_t waves = kWideWaves) { return (bin / 512u) / pass_rounds_per_wave(n_bins, waves); }
static_assert(pass_rounds_per_wave(kWideMaxBins) <= kWidePassMaskBytes, "a thread's pieces fit its mask bytes");
static_assert(2u * kWideWaves * 4u <= kWideReduceBytes, "two dwords per wave of the pass kernels fit the partial maxima's area");

// The census's verdict, rblist::choose_lines's rule.  over[i] = sampled rows with more than 64 x kWideLines[i] set bits.
// -> lines of the smallest slot that at most sampled >> kOverflowShift rows overflow, or 0: too dense for every slot size
inline uint32_t choose_lines(const uint64_t over[kWideSizes], uint64_t sampled)
{
    const uint64_t allowed = sampled >> rblist::kOverflowShift;
    for (uint32_t i = 0; i < kWideSizes; ++i)
        if (over[i] <= allowed) return kWideLines[i];
    return 0;
}

// What one canonical slot says, as rblist::decode_slot: n >= 0 bins (ascending, written to bins[0..n)); -1: an overflow slot;
// -2: not a slot the builder writes.
inline int decode_slot(const uint16_t *slot, uint32_t lines, uint32_t n_bins, uint16_t *bins, uint32_t *side_index)
{
    const uint32_t cap = slot_entries(lines);
    if (slot[0] == kOverflowMark) {
        for (uint32_t i = 3; i < cap; ++i)
            if (slot[i] != kSentinel) return -2;
        *side_index = (uint32_t)slot[1] | ((uint32_t)slot[2] << 16);
        return -1;
    }
    uint32_t n = 0;
    while (n < cap && slot[n] != kSentinel) {
        if (slot[n] >= n_bins || (n && slot[n] <= slot[n - 1])) return -2;
        bins[n] = slot[n];
        ++n;
    }
    for (uint32_t i = n; i < cap; ++i)
        if (slot[i] != kSentinel) return -2;
    return (int)n;
}

// ... and the other way round: the set bits of a dense row of `n_words` words (bins below n_bins) into a canonical slot.
// -> false: the row overflows the slot, which then names side_index
inline bool encode_slot(const uint64_t *row, uint32_t n_words, uint32_t n_bins, uint32_t lines, uint32_t side_index, uint16_t *slot)
{
    const uint32_t cap = slot_entries(lines);
    uint32_t n = 0;
    bool fits = true;
    for (uint32_t i = 0; i < cap; ++i) slot[i] = kSentinel;
    for (uint32_t w = 0; w < n_words && fits; ++w)
        for (uint32_t b = 0; b < 64; ++b) {
            const uint32_t bin = w * 64 + b;
            if (bin >= n_bins || !((row[w] >> b) & 1ull)) continue;
            if (n == cap) {
                fits = false;
                break;
            }
            slot[n++] = (uint16_t)bin;
        }
    if (fits) return true;
    for (uint32_t i = 0; i < cap; ++i) slot[i] = kSentinel;
    slot[0] = kOverflowMark;
    slot[1] = (uint16_t)(side_index & 0xFFFFu);
    slot[2] = (uint16_t)(side_index >> 16);
    return false;
}

// ---- the resident form.  Lane l of the wave that gathers a slot reads its dwords lane_dwords x l ... in one load and adds each dword
// in an instruction of its own, so the spare of dword d is the one of the lane that reads it: no two lanes of one add share a spare.
constexpr uint32_t resident_spare_dword(uint32_t n_bins, uint32_t lines, uint32_t dword) { return cnt_dwords(n_bins) + dword / lane_dwords(lines); }
constexpr uint32_t resident_blank(uint32_t n_bins, uint32_t lines, uint32_t dword)
{
    return (resident_spare_dword(n_bins, lines, dword) * 4u) * 0x10001u;
}

// A canonical slot (what encode_slot writes, of a filter of n_bins bins) as lines x 32 resident dwords.  -> false: not such a slot
inline bool encode_resident(const uint16_t *slot, uint32_t lines, uint32_t n_bins, uint32_t *out)
{
    const uint32_t cap = slot_entries(lines), half = cap / 2;
    for (uint32_t d = 0; d < half; ++d) out[d] = resident_blank(n_bins, lines, d);
    if (slot[0] == kOverflowMark) {
        out[0] |= kResidentOverflow;
        out[1] = (uint32_t)slot[1] | ((uint32_t)slot[2] << 16);
        return true;
    }
    uint32_t n[2] = {0, 0}, total = 0;
    while (total < cap && slot[total] != kSentinel) {
        if (slot[total] >= n_bins) return false;
        ++n[slot[total++] & 1u];
    }
    uint32_t rank[2] = {0, 0};
    for (uint32_t i = 0; i < total; ++i) {
        const uint32_t par = slot[i] & 1u, off = (uint32_t)(slot[i] >> 1) * 4u, r = rank[par]++;
        // its own parity's halves first; what they cannot take goes behind the other parity's bins, flagged
        const uint32_t d = r < half ? r : n[par ^ 1u] + (r - half);
        const uint32_t in = r < half ? par : par ^ 1u;
        const uint32_t h = r < half ? off : off | kResidentSwapped;
        out[d] = in ? (out[d] & 0x0000FFFFu) | (h << 16) : (out[d] & 0xFFFF0000u) | h;
    }
    return true;
}

// ... and back: the canonical slot of lines x 32 resident dwords.  -> as decode_slot: the number of bins, -1 for an overflow slot, -2
// for what no builder writes (an offset that is neither a counter of a bin below n_bins nor the dword's spare, a bin twice, a flag
// out of place)
inline int decode_resident(const uint32_t *in, uint32_t lines, uint32_t n_bins, uint16_t *slot)
{
    const uint32_t cap = slot_entries(lines), half = cap / 2;
    for (uint32_t i = 0; i < cap; ++i) slot[i] = kSentinel;
    if (in[0] & kResidentOverflow) {
        for (uint32_t d = 0; d < half; ++d)
            if (d != 1 && (in[d] & ~kResidentOverflow) != resident_blank(n_bins, lines, d)) return -2;
        slot[0] = kOverflowMark;
        slot[1] = (uint16_t)(in[1] & 0xFFFFu);
        slot[2] = (uint16_t)(in[1] >> 16);
        return -1;
    }
    uint64_t seen[kWideMaxWords] = {};
    uint32_t n = 0;
    for (uint32_t d = 0; d < half; ++d)
        for (uint32_t pos = 0; pos < 2; ++pos) {
            const uint32_t h = (in[d] >> (16u * pos)) & 0xFFFFu, dw = (h & kResidentOffset) >> 2;
            if (h & kResidentOverflow) return -2;
            if (dw >= cnt_dwords(n_bins)) {
                if (h != resident_spare_dword(n_bins, lines, d) * 4u) return -2;
                continue;
            }
            const uint32_t bin = dw * 2u + (pos ^ (h & kResidentSwapped));
            if (bin >= n_bins || ((seen[bin / 64] >> (bin % 64)) & 1ull)) return -2;
            seen[bin / 64] |= 1ull << (bin % 64);
            ++n;
        }
    uint32_t at = 0;
    for (uint32_t w = 0; w < kWideMaxWords && at < n; ++w)
        for (uint32_t b = 0; b < 64; ++b)
            if ((seen[w] >> b) & 1ull) slot[at++] = (uint16_t)(w * 64 + b);
    return (int)n;
}

}  // namespace rbwide

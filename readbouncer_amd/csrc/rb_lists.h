// rb_lists.h -- the slot layout of a filter's LIST TABLE (rb_dibf_list_table_build; rb_lists.hip, ibf_count_lists_kernel), shared by the
// kernels, the engine and the tests.  No HIP in here: tests/cpp/test_lists.cpp compiles it alone, plain and with sanitizers.
//
// The row of an N-free k-mer -- the AND of its h blocks -- has d^h of its bits set (config 3 at design load: about 81 of 8192), so the bin
// numbers of the set bits take far fewer 128-byte lines than the bits.  The list table has one SLOT per such k-mer (the rank of the row
// table: base-4 digits, first base most significant).  A slot is `lines` lines of 128 bytes, lines in {1, 2, 4}, the same for every slot
// of a table, and holds up to 64 x lines entries of 16 bits: the row's bin numbers in ascending order, then kSentinel to the end.
// A row with more set bits than a slot holds is an OVERFLOW slot: entry 0 is kOverflowMark, entries 1 and 2 are the low and the high half
// of the index of its dense row (`stride` 64-bit words, as in the row table) in the table's side table, the rest is kSentinel.
// Bin numbers are below kMaxBins, so neither mark is a bin.
// That is the CANONICAL form: what rb_dibf_list_table_download returns and the tests read.  The device keeps the same slots in the
// RESIDENT form (below, encode_resident / decode_resident), whose entries are ready-made LDS addresses for the count kernels.
#pragma once
#include <cstdint>

namespace rblist {

constexpr uint32_t kLineBytes = 128;
constexpr uint32_t kEntriesPerLine = kLineBytes / 2;
constexpr uint32_t kMaxLines = 4;
constexpr uint16_t kSentinel = 0xFFFFu;
constexpr uint16_t kOverflowMark = 0xFFFEu;
constexpr uint32_t kMaxBins = 8192;      // one column slice of two words per lane: what the count kernel holds counters for
constexpr uint32_t kMaxKmers = 65535;    // per strand: a bin's count fits its 16-bit counter
// the census: a slot size serves a filter when at most one sampled row in 2^kOverflowShift overflows it
constexpr uint32_t kOverflowShift = 10;
constexpr uint64_t kCensusRows = 1ull << 16;

constexpr uint32_t slot_entries(uint32_t lines) { return lines * kEntriesPerLine; }
constexpr uint64_t slot_bytes(uint32_t lines) { return (uint64_t)lines * kLineBytes; }
constexpr bool lines_valid(uint32_t lines) { return lines == 1 || lines == 2 || lines == 4; }

// rows the side table holds for a table of n_rows slots: twice what the census allows to overflow, and never fewer than 64
constexpr uint64_t side_capacity(uint64_t n_rows) { return (n_rows >> (kOverflowShift - 1)) + 64; }

// What one wave of ibf_count_lists_kernel keeps in LDS, and what launch_lists_nt asks for: a 16-bit counter for every bin, two per dword,
// rounded up to 1 KiB (the kernel scans them in 16-byte pieces per lane: whole pieces, and the pad counts nothing); one spare dword per
// lane behind them, where the entries that are no bin are added -- junk that is never read or cleared; the bases of one 64-k-mer tile
// as Dna5 ordinals (64 + k - 1 <= 76 at k <= 13).
constexpr uint32_t kCountSpareDwords = 64;
constexpr uint32_t kCountStageBytes = 128;
constexpr uint32_t kLdsPerCuBytes = 160 * 1024;
constexpr uint32_t count_cnt_dwords(uint32_t n_bins) { return ((n_bins + 1u) / 2u + 255u) & ~255u; }
constexpr uint32_t count_lds_bytes(uint32_t n_bins) { return (count_cnt_dwords(n_bins) + kCountSpareDwords) * 4u + kCountStageBytes; }
// one wave per workgroup: the workgroups of a CU that the LDS leaves room for
constexpr uint32_t count_resident_workgroups(uint32_t n_bins) { return kLdsPerCuBytes / count_lds_bytes(n_bins); }

// What one wave of ibf_locate_lists_kernel and ibf_hits_lists_kernel keeps in LDS: the count kernel's counters, spares and stage, and
// behind them the HIT MASK -- one bit per counter half, so one byte per 16-byte piece of the counters (eight bins), written by the scan
// that ends the first strand and read by the scan that ends the second.  1 KiB at 8192 bins: nine workgroups per CU, as the count kernel.
constexpr uint32_t pass_mask_bytes(uint32_t n_bins) { return count_cnt_dwords(n_bins) / 4u; }
constexpr uint32_t pass_lds_bytes(uint32_t n_bins) { return count_lds_bytes(n_bins) + pass_mask_bytes(n_bins); }
constexpr uint32_t pass_resident_workgroups(uint32_t n_bins) { return kLdsPerCuBytes / pass_lds_bytes(n_bins); }

// The census's verdict. over[i] = sampled rows with more than 64 << i set bits (i = 0, 1, 2), of `sampled` rows.
// -> lines of the smallest slot that at most sampled >> kOverflowShift rows overflow, or 0: no slot size serves (the filter is too dense)
inline uint32_t choose_lines(const uint64_t over[3], uint64_t sampled)
{
    const uint64_t allowed = sampled >> kOverflowShift;
    for (uint32_t i = 0; i < 3; ++i)
        if (over[i] <= allowed) return 1u << i;
    return 0;
}

// What one slot says.  n >= 0: a list of n bins (ascending, written to bins[0..n)); -1: an overflow slot, *side_index names its dense
// row; -2: not a slot the builder writes (an entry out of order, a bin behind a sentinel, a mark in the wrong place).
inline int decode_slot(const uint16_t *slot, uint32_t lines, uint16_t *bins, uint32_t *side_index)
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
        if (slot[n] >= kMaxBins || (n && slot[n] <= slot[n - 1])) return -2;
        bins[n] = slot[n];
        ++n;
    }
    for (uint32_t i = n; i < cap; ++i)
        if (slot[i] != kSentinel) return -2;
    return (int)n;
}

// ... and the other way round, as the builder does it: the set bits of a dense row of `n_words` words (bins below n_bins) into a slot.
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

// ---- THE RESIDENT ("add-ready") FORM: what ibf_list_table_kernel writes and list_batch (rb_lists_device.h) reads; private to the
// device.  Slot size, slot count, side table and census are the canonical form's; only the 32 bits of a slot's dwords mean something else.
// Everything a count kernel would compute from a bin number depends on the filter alone, so the table holds it computed: each 16-bit
// HALF of a dword is, in bits 15:2, the LDS byte offset of a counter dword -- counters as count_lds_bytes lays them out: dword bin >> 1,
// half bin & 1, from offset 0 -- and the half's POSITION is the bin's parity: even bins in low halves, odd bins in high halves.  The
// kernel adds the constant 1 at `v & 0xFFFF` and the constant 1 << 16 at `v >> 16`.  A half that lists no bin holds the offset of a
// SPARE dword behind the counters, the one of the lane that reads the dword (resident_spare_dword: no two lanes of one add share one).
// Bits 1:0 of a half are flags, zero in nearly every slot; a group of slots whose dwords OR to no flag takes the two-instruction path.
//   kResidentSwapped  : the half lists a bin of the OTHER parity (a row that fits the slot, but whose even or odd bins alone exceed half
//                       of it, puts the excess there)
//   kResidentOverflow : in the low half of dword 0 alone: an overflow slot.  Dword 1 is the whole index of its dense row in the side
//                       table, every other half a spare.
// Order within a slot is free (adds commute); the builders here and on the device fill each parity's halves from dword 0 up.
constexpr uint32_t kResidentSwapped = 1u;
constexpr uint32_t kResidentOverflow = 2u;
constexpr uint32_t kResidentFlags = 0x00030003u;  // of a dword
constexpr uint32_t kResidentOffset = 0xFFFCu;     // of a half

// the spare that the non-bin halves of dword `dword` of a slot name: lane l reads dword l of a one- or two-line slot (l < 32 of one
// line), dwords 2 l and 2 l + 1 of a four-line slot, each dword in an add instruction of its own
constexpr uint32_t resident_spare_dword(uint32_t n_bins, uint32_t lines, uint32_t dword)
{
    return count_cnt_dwords(n_bins) + (lines == 4 ? dword >> 1 : dword);
}
constexpr uint32_t resident_blank(uint32_t n_bins, uint32_t lines, uint32_t dword)
{
    return (resident_spare_dword(n_bins, lines, dword) * 4u) * 0x10001u;
}
static_assert((count_cnt_dwords(kMaxBins) + kCountSpareDwords) * 4u <= kResidentOffset + 4u, "a counter's byte offset fits bits 15:2 of a half");

// A canonical slot (what encode_slot writes, of a filter of n_bins bins) as lines * 32 resident dwords.  -> false: not such a slot
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

// ... and back: the canonical slot (ascending bins, sentinels, or mark and index) of lines * 32 resident dwords.  -> as decode_slot:
// the number of bins, -1 for an overflow slot, -2 for what no builder writes (an offset that is neither a counter of a bin below
// n_bins nor the dword's spare, a bin twice, a flag out of place)
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
    uint64_t seen[kMaxBins / 64] = {};
    uint32_t n = 0;
    for (uint32_t d = 0; d < half; ++d)
        for (uint32_t pos = 0; pos < 2; ++pos) {
            const uint32_t h = (in[d] >> (16u * pos)) & 0xFFFFu, dw = (h & kResidentOffset) >> 2;
            if (h & kResidentOverflow) return -2;
            if (dw >= count_cnt_dwords(n_bins)) {
                if (h != resident_spare_dword(n_bins, lines, d) * 4u) return -2;
                continue;
            }
            const uint32_t bin = dw * 2u + (pos ^ (h & kResidentSwapped));
            if (bin >= n_bins || ((seen[bin / 64] >> (bin % 64)) & 1ull)) return -2;
            seen[bin / 64] |= 1ull << (bin % 64);
            ++n;
        }
    uint32_t at = 0;
    for (uint32_t w = 0; w < kMaxBins / 64 && at < n; ++w)
        for (uint32_t b = 0; b < 64; ++b)
            if ((seen[w] >> b) & 1ull) slot[at++] = (uint16_t)(w * 64 + b);
    return (int)n;
}

}  // namespace rblist

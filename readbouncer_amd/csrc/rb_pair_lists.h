// rb_pair_lists.h -- the slot layout of a filter's PAIR TABLE (rb_dibf_pair_table_build; rb_pair_lists.hip, ibf_count_pair_lists_kernel),
// shared by the kernels, the engine and the tests.  No HIP in here: tests/cpp/test_pair_lists.cpp compiles it alone, plain and with
// sanitizers.
//
// The list table of rb_lists.h spends two lines on a row of 81 +- 9 bins (config 3 at design load) and a read fetches the slots of a k-mer
// and of its reverse complement: four lines for 162 entries.  The pair table has one SLOT of THREE lines per N-free k-mer x, indexed by the
// row table's rank of x itself, that holds both lists:
//   list A = the bins of row(x), which the read's forward strand counts,
//   list B = the bins of row(rc(x)), which its reverse strand counts (rc: the reverse complement; a palindromic x has A = B, and both are
//            counted, as the oracle counts both strands).
// Every pair is therefore stored twice, under x and under rc(x): 4^k x 384 bytes.  The kernel needs the forward rank only.
//
// The counters are one LDS DWORD per bin: the low half is the forward strand's 16-bit count, the high half the reverse strand's.  A
// 16-bit HALF of a slot's dword is, as in rb_lists.h's resident form, the byte offset of a counter dword in bits 15:2, or a spare's.
//   lines 0-1 (dwords 0..63) are POSITIONAL: the low half of dword d is A[d], the high half B[d] (ascending bins; past a list's end the
//             spare of dword d).  The kernel adds 1 at `v & 0xFFFC` and 1 << 16 at `v >> 16`: bits 1:0 of these halves are zero.
//   line 2    (dwords 64..95) holds what is left of both lists, A[64..) then B[64..), half after half; bit 0 of a half (kPairListB)
//             says that it belongs to list B, and is evaluated for every half.  A half that lists nothing names spare q of its position
//             q in the line (a wave reads line 2 of two slots with one load, lanes 0-31 and 32-63).
// A slot whose lists leave more than 64 entries for line 2 keeps 62 of them there and its last dword (kPairIndexDword) is no pair of
// entries but an INDEX, marked by bit 1 of its low half (kPairIndex), which no other half of a slot ever carries:
//   a TAIL slot names one tail line of 128 bytes in the table's tail array: 64 more halves in line 2's format;
//   a DENSE slot (more than slot + tail hold: in practice a k-mer two of whose blocks coincide) names a pair of dense rows, row(x) and
//   row(rc(x)), `stride` words each, in the side table, and lists nothing itself (bit 0 of the index's low half: kPairDense).
// So a slot with max(nA - 64, 0) + max(nB - 64, 0) <= 64 -- every slot with nA + nB <= 192 and both lists <= 128 -- is counted with no
// test but the one on its line-2 dwords, slot + tail hold nA + nB <= 254 (at 64 or more in each list), and the census below refuses a
// filter that would send more than 1 pair in kPairTailShare to a tail or more than 1 in kPairDenseShare to dense rows.
// That is the RESIDENT form, the only one the device holds.  The CANONICAL form is what rb_dibf_pair_table_download returns and the tests
// read: kPairCanonEntries entries of 16 bits per slot: the slot's bins of A ascending, kSentinel, its bins of B ascending, kSentinel to
// entry 252; entries 253 and 254 are the halves of the index and entry 255 is kPairTailMark or kOverflowMark (dense) where the slot
// has one, kSentinel otherwise.  (A tail slot's canonical form lists what the SLOT holds: the tail line decodes on its own.)
#pragma once
#include <cstdint>

#include "rb_lists.h"

namespace rbpair {

using rblist::kLineBytes;
using rblist::kOverflowMark;
using rblist::kSentinel;

constexpr uint32_t kPairLines = 3;
constexpr uint32_t kPairDwords = kPairLines * kLineBytes / 4;  // 96
constexpr uint32_t kPairPositional = 64;                       // entries of either list in lines 0-1
constexpr uint32_t kPairRest = 64;                             // halves of line 2
constexpr uint32_t kPairRestIndexed = kPairRest - 2;           // ... of a slot whose last dword is an index
constexpr uint32_t kPairTailHalves = 64;                       // a tail line
constexpr uint32_t kPairTailDwords = kPairTailHalves / 2;
constexpr uint32_t kPairIndexDword = kPairDwords - 1;
constexpr uint32_t kPairCapacity = 2 * kPairPositional + kPairRest;                              // 192
constexpr uint32_t kPairTailCapacity = 2 * kPairPositional + kPairRestIndexed + kPairTailHalves;  // 254
constexpr uint32_t kPairListB = 1u;   // bit 0 of a line-2 or tail half: the half counts for the reverse strand
constexpr uint32_t kPairIndex = 2u;   // bit 1 of the low half of kPairIndexDword: the dword is an index
constexpr uint32_t kPairDense = 1u;   // bit 0 of that half: ... of a pair of dense rows (else of a tail line)
constexpr uint32_t kPairOffset = 0xFFFCu;
constexpr uint32_t kPairMaxBins = rblist::kMaxBins;
constexpr uint32_t kPairMaxKmers = rblist::kMaxKmers;
constexpr uint32_t kPairSpareDwords = 64;
constexpr uint32_t kPairStageBytes = 128;   // per wave: the bases of the tile it has in hand
constexpr uint32_t kPairReduceBytes = 64;   // the waves' partial maxima
constexpr uint32_t kPairWaves = 4;          // waves per workgroup (profiles/pair_lists/probe.txt)
constexpr uint16_t kPairTailMark = 0xFFFDu;
constexpr uint32_t kPairCanonEntries = 256;
// the census's caps: at most one sampled pair in 32 with a tail, one in 1024 with dense rows
constexpr uint32_t kPairTailShare = 5;    // log2
constexpr uint32_t kPairDenseShare = 10;  // log2

constexpr uint32_t cnt_dwords(uint32_t n_bins) { return (n_bins + 255u) & ~255u; }  // one dword per bin, whole 1 KiB pieces
constexpr uint32_t count_lds_bytes(uint32_t n_bins, uint32_t waves = kPairWaves)
{
    return (cnt_dwords(n_bins) + kPairSpareDwords) * 4u + waves * kPairStageBytes + kPairReduceBytes;
}
constexpr uint32_t count_resident_workgroups(uint32_t n_bins, uint32_t waves = kPairWaves)
{
    return rblist::kLdsPerCuBytes / count_lds_bytes(n_bins, waves);
}
static_assert((cnt_dwords(kPairMaxBins) + kPairSpareDwords) * 4u <= kPairOffset + 4u, "a spare's byte offset fits bits 15:2 of a half");
static_assert(count_resident_workgroups(kPairMaxBins) == 4, "four workgroups of four waves per CU at 8192 bins");
constexpr uint64_t slot_bytes() { return (uint64_t)kPairLines * kLineBytes; }

// the side arrays of a table of n_rows slots: twice what the census allows, and never fewer than 64; dense rows come in pairs
constexpr uint64_t tail_capacity(uint64_t n_rows) { return (n_rows >> (kPairTailShare - 1)) + 64; }
constexpr uint64_t side_capacity(uint64_t n_rows) { return 2 * ((n_rows >> (kPairDenseShare - 1)) + 64); }

// what is left of a pair for line 2 and beyond, and what becomes of it
constexpr uint32_t rest_of(uint32_t nA, uint32_t nB)
{
    return (nA > kPairPositional ? nA - kPairPositional : 0u) + (nB > kPairPositional ? nB - kPairPositional : 0u);
}
enum PairKind : int { kPlain = 0, kTail = 1, kDenseRows = 2 };
constexpr PairKind kind_of(uint32_t nA, uint32_t nB)
{
    return rest_of(nA, nB) <= kPairRest ? kPlain : rest_of(nA, nB) <= kPairRestIndexed + kPairTailHalves ? kTail : kDenseRows;
}

// The census's verdict.  over[0] = sampled slots that need a tail or more, over[1] = that need dense rows, of `sampled` slots.
// One pair is dense in EVERY filter and is not held against it: the k-mer of value 0, A^k, hashes to block 0 under every hash function,
// so its row is a whole block, and it has two slots, its own and T^k's (kPairAlwaysDense; at k = 5 they are two slots of 1024).
// -> kPairLines, or 0: the pair table does not serve this filter (no error: the list table may)
constexpr uint64_t kPairAlwaysDense = 2;
inline uint32_t choose_lines(const uint64_t over[3], uint64_t sampled)
{
    return over[0] <= (sampled >> kPairTailShare) + kPairAlwaysDense && over[1] <= (sampled >> kPairDenseShare) + kPairAlwaysDense ? kPairLines : 0u;
}

constexpr uint32_t spare_of_dword(uint32_t n_bins, uint32_t d) { return (cnt_dwords(n_bins) + d) * 4u; }   // lines 0-1: d < 64
constexpr uint32_t spare_of_half(uint32_t n_bins, uint32_t q) { return (cnt_dwords(n_bins) + q) * 4u; }    // line 2 and tail: q < 64
constexpr uint32_t index_dword(uint32_t index, bool dense)
{
    return ((index & 0x3FFFu) << 2) | kPairIndex | (dense ? kPairDense : 0u) | ((index >> 14) << 16);
}
constexpr uint32_t index_of(uint32_t dword) { return ((dword & 0xFFFFu) >> 2) | ((dword >> 16) << 14); }
constexpr uint32_t kPairMaxIndex = (1u << 30) - 1;

inline void put_half(uint32_t *dwords, uint32_t half, uint32_t value)
{
    uint32_t &d = dwords[half >> 1];
    d = (half & 1u) ? (d & 0x0000FFFFu) | (value << 16) : (d & 0xFFFF0000u) | value;
}
inline uint32_t get_half(const uint32_t *dwords, uint32_t half) { return (dwords[half >> 1] >> (16u * (half & 1u))) & 0xFFFFu; }

// The resident slot of a pair, as the builder writes it: A[0..nA) and B[0..nB) are ascending bins below n_bins.  `index` is what a tail
// or dense slot names (the tail line, or the first of its two dense rows).  slot: kPairDwords dwords; tail: kPairTailDwords dwords,
// written for a tail slot only.  -> the slot's kind
inline PairKind encode_pair(const uint16_t *A, uint32_t nA, const uint16_t *B, uint32_t nB, uint32_t n_bins, uint32_t index, uint32_t *slot,
                            uint32_t *tail)
{
    for (uint32_t d = 0; d < kPairPositional; ++d) slot[d] = spare_of_dword(n_bins, d) * 0x10001u;
    for (uint32_t q = 0; q < kPairRest; ++q) put_half(slot + kPairPositional, q, spare_of_half(n_bins, q));
    const PairKind kind = kind_of(nA, nB);
    if (kind == kDenseRows) {
        slot[kPairIndexDword] = index_dword(index, true);
        return kind;
    }
    if (kind == kTail) {
        for (uint32_t q = 0; q < kPairTailHalves; ++q) put_half(tail, q, spare_of_half(n_bins, q));
        slot[kPairIndexDword] = index_dword(index, false);
    }
    const uint32_t in_slot = kind == kTail ? kPairRestIndexed : kPairRest;
    uint32_t q = 0;
    for (uint32_t i = 0; i < nA; ++i) {
        if (i < kPairPositional) put_half(slot, 2 * i, (uint32_t)A[i] * 4u);
        else if (q < in_slot) put_half(slot + kPairPositional, q++, (uint32_t)A[i] * 4u);
        else put_half(tail, q++ - in_slot, (uint32_t)A[i] * 4u);
    }
    for (uint32_t i = 0; i < nB; ++i) {
        if (i < kPairPositional) put_half(slot, 2 * i + 1, (uint32_t)B[i] * 4u);
        else if (q < in_slot) put_half(slot + kPairPositional, q++, (uint32_t)B[i] * 4u | kPairListB);
        else put_half(tail, q++ - in_slot, (uint32_t)B[i] * 4u | kPairListB);
    }
    return kind;
}

// the bins two dense rows of n_words words list, ascending (at most kPairMaxBins each)
inline uint32_t bins_of_row(const uint64_t *row, uint32_t n_words, uint32_t n_bins, uint16_t *bins)
{
    uint32_t n = 0;
    for (uint32_t w = 0; w < n_words; ++w)
        for (uint32_t b = 0; b < 64; ++b)
            if (w * 64 + b < n_bins && ((row[w] >> b) & 1ull)) bins[n++] = (uint16_t)(w * 64 + b);
    return n;
}

// One half of line 2 or of a tail line at position q.  -> 0: a spare, 1: *bin of list A, 2: *bin of list B, -2: what no builder writes
inline int decode_rest_half(uint32_t h, uint32_t q, uint32_t n_bins, uint32_t *bin)
{
    if (h & kPairIndex) return -2;
    const uint32_t dw = (h & kPairOffset) >> 2;
    if (dw >= cnt_dwords(n_bins)) return h == spare_of_half(n_bins, q) ? 0 : -2;
    if (dw >= n_bins) return -2;
    *bin = dw;
    return (h & kPairListB) ? 2 : 1;
}

// `n_halves` halves of line 2 or of a tail line appended to the lists: A's entries first, then B's, then spares, each list ascending
// and above what it holds already.  -> false: what no builder writes
inline bool decode_rest(const uint32_t *dwords, uint32_t n_halves, uint32_t n_bins, uint16_t *A, uint32_t *nA, uint16_t *B, uint32_t *nB)
{
    int stage = 1;  // 1: A's entries, 2: B's, 0: spares
    for (uint32_t q = 0; q < n_halves; ++q) {
        uint32_t bin = 0;
        const int what = decode_rest_half(get_half(dwords, q), q, n_bins, &bin);
        if (what == -2) return false;
        if (what == 0) {
            stage = 0;
            continue;
        }
        if (stage == 0 || (stage == 2 && what == 1)) return false;
        stage = what;
        uint16_t *list = what == 1 ? A : B;
        uint32_t *n = what == 1 ? nA : nB;
        if (*n < kPairPositional || *n >= kPairMaxBins || bin <= list[*n - 1]) return false;  // line 2 begins where lines 0-1 are full
        list[(*n)++] = (uint16_t)bin;
    }
    return true;
}

// A resident slot back into its lists (what the slot itself holds).  -> the slot's kind and, for a tail or dense slot, *index;
// -2: what no builder writes (an offset that is neither a counter of a bin below n_bins nor the half's spare, a list out of order or
// with a gap, a flag out of place, a dense slot that lists something).  A, B: room for kPairMaxBins entries each.
inline int decode_pair(const uint32_t *slot, uint32_t n_bins, uint16_t *A, uint32_t *nA, uint16_t *B, uint32_t *nB, uint32_t *index)
{
    *nA = *nB = 0;
    for (uint32_t d = 0; d < kPairPositional; ++d)
        for (uint32_t pos = 0; pos < 2; ++pos) {
            const uint32_t h = get_half(slot, 2 * d + pos), dw = h >> 2;
            uint16_t *list = pos ? B : A;
            uint32_t *n = pos ? nB : nA;
            if (h & 3u) return -2;
            if (dw >= cnt_dwords(n_bins)) {
                if (h != spare_of_dword(n_bins, d)) return -2;
                continue;
            }
            if (dw >= n_bins || *n != d || (d && dw <= list[d - 1])) return -2;  // no gap, ascending
            list[(*n)++] = (uint16_t)dw;
        }
    const uint32_t last = slot[kPairIndexDword];
    const bool indexed = (last & kPairIndex) != 0;
    if (!decode_rest(slot + kPairPositional, indexed ? kPairRestIndexed : kPairRest, n_bins, A, nA, B, nB)) return -2;
    if (!indexed) return kPlain;
    *index = index_of(last);
    if (last & kPairDense) return *nA == 0 && *nB == 0 ? (int)kDenseRows : -2;
    return rest_of(*nA, *nB) == kPairRestIndexed ? (int)kTail : -2;  // a tail slot's line 2 is full
}

// The canonical slot (kPairCanonEntries entries) of a resident slot.  -> as decode_pair
inline int decode_resident(const uint32_t *slot, uint32_t n_bins, uint16_t *canon)
{
    uint16_t A[kPairMaxBins], B[kPairMaxBins];
    uint32_t nA = 0, nB = 0, index = 0;
    for (uint32_t i = 0; i < kPairCanonEntries; ++i) canon[i] = kSentinel;
    const int kind = decode_pair(slot, n_bins, A, &nA, B, &nB, &index);
    if (kind == -2 || nA + nB + 1 > kPairCanonEntries - 3) return -2;
    for (uint32_t i = 0; i < nA; ++i) canon[i] = A[i];
    for (uint32_t i = 0; i < nB; ++i) canon[nA + 1 + i] = B[i];
    if (kind != kPlain) {
        canon[253] = (uint16_t)(index & 0xFFFFu);
        canon[254] = (uint16_t)(index >> 16);
        canon[255] = kind == kTail ? kPairTailMark : kOverflowMark;
    }
    return kind;
}

// ... and the lists of a canonical slot.  -> its kind, or -2
inline int decode_canonical(const uint16_t *canon, uint32_t n_bins, uint16_t *A, uint32_t *nA, uint16_t *B, uint32_t *nB, uint32_t *index)
{
    uint32_t i = 0;
    *nA = *nB = 0;
    for (; i < 253 && canon[i] != kSentinel; ++i) {
        if (canon[i] >= n_bins || (*nA && canon[i] <= A[*nA - 1])) return -2;
        A[(*nA)++] = canon[i];
    }
    for (++i; i < 253 && canon[i] != kSentinel; ++i) {
        if (canon[i] >= n_bins || (*nB && canon[i] <= B[*nB - 1])) return -2;
        B[(*nB)++] = canon[i];
    }
    for (; i < 253; ++i)
        if (canon[i] != kSentinel) return -2;
    if (canon[255] == kSentinel) return canon[253] == kSentinel && canon[254] == kSentinel ? (int)kPlain : -2;
    *index = (uint32_t)canon[253] | ((uint32_t)canon[254] << 16);
    return canon[255] == kPairTailMark ? (int)kTail : canon[255] == kOverflowMark ? (int)kDenseRows : -2;
}

}  // namespace rbpair

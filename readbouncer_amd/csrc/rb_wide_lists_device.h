// rb_wide_lists_device.h -- the device code the wide list kernels share beyond rb_lists_device.h: a lane's share of a slot, the set bits
// of a dense row, one batch of slot gathers, one strand of an item counted in full by a workgroup, a range of it, and a wave's share of a
// scan.  Included by rb_wide_lists.hip (the count kernel and the table), rb_wide_pass_lists.hip (the wide forms of locate and hits) and
// rb_wide_prefix_lists.hip (the wide form of the prefix pass); HIP translation units only.
#pragma once
#include <hip/hip_runtime.h>

#include "rb_device.h"
#include "rb_lists.h"
#include "rb_lists_device.h"
#include "rb_wide_lists.h"

namespace rb {

template <int DW>
struct WideVec;
template <>
struct WideVec<2> {
    typedef unsigned int type __attribute__((ext_vector_type(2)));
};
template <>
struct WideVec<3> {
    typedef unsigned int type __attribute__((ext_vector_type(3), aligned(4)));  // lane l of a six-line slot begins at byte 12 l
};
template <>
struct WideVec<4> {
    typedef unsigned int type __attribute__((ext_vector_type(4)));
};

// the set bits of a dense row (an overflow slot's, or the AND of the blocks of a k-mer that has no slot), word `lane`, `lane + 64`, ...
// of it per lane, counted one by one
__device__ __forceinline__ void wide_count_word(uint32_t *cnt, uint64_t word, uint32_t w, uint32_t n_bins)
{
    while (word) {
        const uint32_t bit = (uint32_t)__builtin_ctzll(word);
        word &= word - 1;
        count_bin(cnt, w * 64u + bit, n_bins);
    }
}

// One batch of 16 slots of a wave's tile, slots first .. first + 15: `listed` says which of the tile's k-mers have a slot to count (in
// the strand, no base outside ACGT).  FULL: all 16 have, and nothing is guarded.  Lane l takes dwords DW l .. DW l + DW - 1 of every
// slot in ONE load (8, 12 or 16 bytes: an eight-line slot is a dwordx4 per lane), the loads are issued back to back, and a group of
// eight slots is added as soon as its loads have landed (list_batch's order, so the waits are counted).  Flags as in list_batch: the
// group's dwords ORed, one wave-wide test, and only a flagged group looks at its slots one by one.
template <int LINES, bool NT, bool FULL>
__device__ __forceinline__ void wide_batch(const IbfDev &f, uint32_t *cnt, const uint32_t *__restrict__ slots, const uint64_t *__restrict__ side,
                                           uint32_t side_rows, uint32_t rank, uint64_t listed, uint32_t first, uint32_t lane, uint32_t spare)
{
    constexpr int DW = LINES / 2;
    constexpr int R = 16;
    constexpr int G = 8;
    constexpr uint32_t SLOT_DWORDS = LINES * 32;
    typedef typename WideVec<DW>::type vec_t;
    const uint32_t spare_off = spare * 4u, blank = spare_off * 0x10001u;
    uint32_t v[R][DW];
#pragma unroll
    for (int u = 0; u < R; ++u) {
#pragma unroll
        for (int d = 0; d < DW; ++d) v[u][d] = blank;
        if (FULL || ((listed >> (first + (uint32_t)u)) & 1ull)) {  // wave-uniform
            const uint32_t slot = (uint32_t)__builtin_amdgcn_readlane((int)rank, (int)(first + (uint32_t)u));
            const uint32_t *base = slots + (uint64_t)slot * SLOT_DWORDS;  // slot < 4^k: masked digits; 64-bit: 4^13 slots of 1 KiB are 64 GiB
            const vec_t *p = reinterpret_cast<const vec_t *>(base + lane * (uint32_t)DW);
            const vec_t q = NT ? __builtin_nontemporal_load(p) : *p;
#pragma unroll
            for (int d = 0; d < DW; ++d) v[u][d] = q[d];
        }
    }
    __builtin_amdgcn_sched_barrier(0);
    uint32_t overflow = 0;  // the batch's overflow slots
#pragma unroll
    for (int g = 0; g < R / G; ++g) {
        if (FULL || ((listed >> (first + (uint32_t)(g * G))) & 0xFFull)) {  // wave-uniform
            uint32_t fold = 0;
#pragma unroll
            for (int u = 0; u < G; ++u)
#pragma unroll
                for (int d = 0; d < DW; ++d) fold |= v[g * G + u][d];
            if (__builtin_expect(__ballot((fold & rblist::kResidentFlags) != 0u) != 0ULL, 0)) {  // wave-uniform, rare
#pragma unroll
                for (int u = 0; u < G; ++u) {
                    const int s = g * G + u;
                    const uint32_t d0 = (uint32_t)__builtin_amdgcn_readlane((int)v[s][0], 0);  // dword 0 of the slot
                    if (d0 & rblist::kResidentOverflow) {  // wave-uniform: set aside, and blanked (its index is no address)
                        overflow |= 1u << s;
#pragma unroll
                        for (int d = 0; d < DW; ++d) v[s][d] = blank;
                    } else {
#pragma unroll
                        for (int d = 0; d < DW; ++d)
                            if (v[s][d] & rblist::kResidentFlags) v[s][d] = list_add_swapped(cnt, v[s][d], spare_off, true);
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < G; ++u)
#pragma unroll
                for (int d = 0; d < DW; ++d) list_add2(cnt, v[g * G + u][d]);
        }
    }
    while (overflow) {  // wave-uniform, rare: the slot's index dword once more, then the dense row's set bits one by one
        const int u = __builtin_ctz(overflow);
        overflow &= overflow - 1;
        const uint32_t slot = (uint32_t)__builtin_amdgcn_readlane((int)rank, (int)first + u);
        const uint32_t idx = slots[(uint64_t)slot * SLOT_DWORDS + 1];
        if (idx >= side_rows) continue;  // (the builder never names a row it did not write)
        const uint64_t *row = side + (uint64_t)idx * f.stride;
        for (uint32_t w = lane; w < f.bin_width; w += 64) wide_count_word(cnt, row[w], w, f.n_bins);
    }
}

// One strand of an item, counted in full by a workgroup of NW waves into the shared counters: the tile loop of
// ibf_count_wide_lists_kernel -- tile t of the strand to wave t mod NW, each wave staging its own tile's bases in `stage` (its own area),
// a k-mer with a base outside ACGT counted from the filter's own table -- without the bound and the strand skip, which stand around the
// loop there.  The caller puts the workgroup's barrier behind it.  `nh`: min(f.n_hash, rbspec::kMaxHash).
// (wide_count_range below is this loop over a range: keep the two in step.)
template <int LINES, bool NT, int NW>
__device__ __forceinline__ void wide_count_strand(const IbfDev &f, uint32_t *cnt, uint8_t *stage, const uint32_t *__restrict__ slots,
                                                  const uint64_t *__restrict__ side, uint32_t side_rows, const ListBaseSrc &seq, uint32_t len,
                                                  uint32_t n, int strand, uint32_t wave, uint32_t lane, uint32_t spare, uint32_t nh)
{
    const uint32_t k = f.k;
#pragma unroll 1
    for (uint32_t mt = wave * 64u; mt < n; mt += 64u * NW) {  // wave-uniform
        // ---- the tile's bases as Dna5 ordinals, and one rank per lane
        const uint32_t wlen = min(64u + k - 1u, len - mt);
        __builtin_amdgcn_wave_barrier();
        if (lane < wlen) stage[lane] = (uint8_t)seq.ord(mt + lane);
        if (lane + 64u < wlen) stage[lane + 64u] = (uint8_t)seq.ord(mt + 64u + lane);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
        __builtin_amdgcn_wave_barrier();
        const uint32_t p = mt + lane;
        uint32_t rank = 0;
        bool outside = false;
        if (p < n) {
            const uint8_t *b = stage + lane;
            if (strand == 0) {
                for (uint32_t i = 0; i < k; ++i) {
                    outside |= b[i] > 3u;
                    rank = (rank << 2) | (b[i] & 3u);
                }
            } else {
                for (uint32_t i = 0; i < k; ++i) {
                    outside |= b[k - 1 - i] > 3u;
                    rank = (rank << 2) | ((3u - b[k - 1 - i]) & 3u);
                }
            }
        }
        const uint64_t listed = __ballot(p < n && !outside);
        uint64_t unlisted = __ballot(p < n && outside);
        const uint32_t in_tile = min(64u, n - mt);
#pragma unroll 1
        for (uint32_t first = 0; first < in_tile; first += 16) {
            const uint32_t sub = (uint32_t)(listed >> first) & 0xFFFFu;
            if (sub == 0xFFFFu)  // wave-uniform
                wide_batch<LINES, NT, true>(f, cnt, slots, side, side_rows, rank, listed, first, lane, spare);
            else if (sub)
                wide_batch<LINES, NT, false>(f, cnt, slots, side, side_rows, rank, listed, first, lane, spare);
        }
        while (__builtin_expect(unlisted != 0ULL, 0)) {  // wave-uniform, rare: a k-mer with a base outside ACGT, from the filter's own table
            const uint32_t u = (uint32_t)__builtin_ctzll(unlisted);
            unlisted &= unlisted - 1;
            const uint8_t *b = stage + u;
            uint64_t value = 0;
            if (strand == 0) {
                for (uint32_t i = 0; i < k; ++i) value = value * 5u + b[i];
            } else {
                for (uint32_t i = 0; i < k; ++i) value = value * 5u + rbspec::dna5_comp(b[k - 1 - i], f.comp_n);
            }
            uint32_t blk[rbspec::kMaxHash];
#pragma unroll
            for (uint32_t h = 0; h < rbspec::kMaxHash; ++h)
                blk[h] = h < nh ? rbspec::block_index(value, f.precalc[h], f.n_blocks, f.magic, f.pow2_mask) : 0u;
            for (uint32_t w = lane; w < f.bin_width; w += 64) {
                uint64_t acc = ~0ULL;
#pragma unroll
                for (uint32_t h = 0; h < rbspec::kMaxHash; ++h)
                    if (h < nh) acc &= f.words[(uint64_t)blk[h] * f.stride + w];
                wide_count_word(cnt, acc, w, f.n_bins);
            }
        }
    }
}

// A wave's share of a scan of the counters (the wide forms of locate, hits and prefixes; the scheme is set out in rb_wide_pass_lists.hip
// and restated for the host in rb_wide_lists.h): cnt_dwords / 256 rounds of 64 consecutive 16-byte pieces, wave w at the rounds
// [w x per, (w + 1) x per) that exist, per = ceil(rounds / NW).
template <int NW>
struct WideShare {
    uint32_t r0, r1;  // the wave's rounds [r0, r1)
    __device__ __forceinline__ WideShare(uint32_t cnt_dwords, uint32_t wave)
    {
        const uint32_t rounds = cnt_dwords / 256u, per = (rounds + NW - 1) / NW;
        r0 = min(wave * per, rounds);
        r1 = min(r0 + per, rounds);
    }
};

// The RANGED count (the wide list form of the prefix pass): the k-mers [n_from, n_to) of one strand of the item's first `len` bases, n_to
// == len - k + 1 -- wide_count_strand's tile loop over the RANGE: tile t of the range to wave t mod NW, so wave w starts at k-mer n_from +
// 64 w, at a multiple of 64 or not (ListBaseSrc::ord addresses single bases at any offset), and a range shorter than a tile is wave 0's
// alone.  The counters are added to, not cleared; the caller puts the workgroup's barrier behind it.  Kept beside wide_count_strand and
// not under it, so that the count, locate and hits kernels compile as they did: the two loops must be kept in step.
template <int LINES, bool NT, int NW>
__device__ __forceinline__ void wide_count_range(const IbfDev &f, uint32_t *cnt, uint8_t *stage, const uint32_t *__restrict__ slots,
                                                 const uint64_t *__restrict__ side, uint32_t side_rows, const ListBaseSrc &seq, uint32_t len,
                                                 uint32_t n_from, uint32_t n_to, int strand, uint32_t wave, uint32_t lane, uint32_t spare,
                                                 uint32_t nh)
{
    const uint32_t k = f.k;
#pragma unroll 1
    for (uint32_t mt = n_from + wave * 64u; mt < n_to; mt += 64u * NW) {  // wave-uniform; n_to <= kWideMaxKmers: no wrap
        // ---- the tile's bases as Dna5 ordinals, and one rank per lane
        const uint32_t wlen = min(64u + k - 1u, len - mt);
        __builtin_amdgcn_wave_barrier();
        if (lane < wlen) stage[lane] = (uint8_t)seq.ord(mt + lane);
        if (lane + 64u < wlen) stage[lane + 64u] = (uint8_t)seq.ord(mt + 64u + lane);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
        __builtin_amdgcn_wave_barrier();
        const uint32_t p = mt + lane;
        uint32_t rank = 0;
        bool outside = false;
        if (p < n_to) {
            const uint8_t *b = stage + lane;
            if (strand == 0) {
                for (uint32_t i = 0; i < k; ++i) {
                    outside |= b[i] > 3u;
                    rank = (rank << 2) | (b[i] & 3u);
                }
            } else {
                for (uint32_t i = 0; i < k; ++i) {
                    outside |= b[k - 1 - i] > 3u;
                    rank = (rank << 2) | ((3u - b[k - 1 - i]) & 3u);
                }
            }
        }
        const uint64_t listed = __ballot(p < n_to && !outside);
        uint64_t unlisted = __ballot(p < n_to && outside);
        const uint32_t in_tile = min(64u, n_to - mt);
#pragma unroll 1
        for (uint32_t first = 0; first < in_tile; first += 16) {
            const uint32_t sub = (uint32_t)(listed >> first) & 0xFFFFu;
            if (sub == 0xFFFFu)  // wave-uniform
                wide_batch<LINES, NT, true>(f, cnt, slots, side, side_rows, rank, listed, first, lane, spare);
            else if (sub)
                wide_batch<LINES, NT, false>(f, cnt, slots, side, side_rows, rank, listed, first, lane, spare);
        }
        while (__builtin_expect(unlisted != 0ULL, 0)) {  // wave-uniform, rare: a k-mer with a base outside ACGT, from the filter's own table
            const uint32_t u = (uint32_t)__builtin_ctzll(unlisted);
            unlisted &= unlisted - 1;
            const uint8_t *b = stage + u;
            uint64_t value = 0;
            if (strand == 0) {
                for (uint32_t i = 0; i < k; ++i) value = value * 5u + b[i];
            } else {
                for (uint32_t i = 0; i < k; ++i) value = value * 5u + rbspec::dna5_comp(b[k - 1 - i], f.comp_n);
            }
            uint32_t blk[rbspec::kMaxHash];
#pragma unroll
            for (uint32_t h = 0; h < rbspec::kMaxHash; ++h)
                blk[h] = h < nh ? rbspec::block_index(value, f.precalc[h], f.n_blocks, f.magic, f.pow2_mask) : 0u;
            for (uint32_t w = lane; w < f.bin_width; w += 64) {
                uint64_t acc = ~0ULL;
#pragma unroll
                for (uint32_t h = 0; h < rbspec::kMaxHash; ++h)
                    if (h < nh) acc &= f.words[(uint64_t)blk[h] * f.stride + w];
                wide_count_word(cnt, acc, w, f.n_bins);
            }
        }
    }
}

}  // namespace rb

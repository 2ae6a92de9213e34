// rb_pass_lists_device.h -- the device code the list forms of the query passes share beyond rb_lists_device.h: which work items a list
// kernel takes, what a scan reads off a 16-byte piece of the counters, and one strand of an item counted in full.  Included by
// rb_pass_lists.hip (locate and hits), rb_wide_pass_lists.hip (their wide forms, for the pieces) and rb_resume_lists.hip (resume);
// rb_prefix_lists.hip (prefixes) adds the ranged count below.  HIP translation units only.
#pragma once
#include <hip/hip_runtime.h>

#include "rb_device.h"
#include "rb_lists.h"
#include "rb_lists_device.h"

namespace rb {

// Which work items the list kernels take: the item is RB_OK (item_status's rules: chunk_prep's verdict, the declared bound, the engine's
// largest k) and its chunk window holds no base outside ACGT, which is what the list table has slots for.  Called by a whole wave for
// one item; the answer is wave-uniform.
__device__ __forceinline__ bool pass_lists_takes(const ReadSrc &r, uint32_t item, const uint8_t *pre_status, uint32_t min_len, uint32_t lane)
{
    const uint32_t len = r.lens[item];
    if ((pre_status && pre_status[item] != RB_OK) || len > r.max_len || len < min_len) return false;
    const uint32_t rid = r.ids ? r.ids[item] : item;
    bool outside = false;
    if (r.nmask) {  // packed input: a base is outside exactly when its bit of the N bitmap is set
        const uint8_t *nm = r.nmask + r.nmask_offsets[rid];
        for (uint32_t i = lane; i < len; i += 64) outside |= ((nm[(r.base_off + i) >> 3] >> ((r.base_off + i) & 7u)) & 1u) != 0;
    } else {
        const uint8_t *s = r.seqs + r.offsets[rid] + r.base_off;
        for (uint32_t i = lane; i < len; i += 64) outside |= rbspec::dna5_ord(s[i]) > 3u;
    }
    return __ballot(outside) == 0ULL;
}

// A 16-byte piece of the counters, eight bins: counter j (a compile-time place), the largest of the eight, and the bits of those at or
// above t among the bins that exist.  A pad counter -- behind n_bins -- is never added to, and `valid` keeps it out even at t == 0.
__device__ __forceinline__ uint32_t piece_counter(const uint4 &q, int j)
{
    const uint32_t d = j < 2 ? q.x : j < 4 ? q.y : j < 6 ? q.z : q.w;
    return (j & 1) ? d >> 16 : d & 0xFFFFu;
}
__device__ __forceinline__ uint32_t piece_max(const uint4 &q)
{
    const list_u16x2 a = __builtin_elementwise_max(list_max2(__builtin_bit_cast(list_u16x2, q.x), q.y), list_max2(__builtin_bit_cast(list_u16x2, q.z), q.w));
    return max((uint32_t)a.x, (uint32_t)a.y);
}
__device__ __forceinline__ uint32_t piece_hits(const uint4 &q, uint32_t piece, uint32_t t, uint32_t n_bins)
{
    const uint32_t first = piece * 8u;
    const uint32_t valid = first >= n_bins ? 0u : (n_bins - first >= 8u ? 0xFFu : (1u << (n_bins - first)) - 1u);
    uint32_t bits = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) bits |= (piece_counter(q, j) >= t ? 1u : 0u) << j;
    return bits & valid;
}

__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += (uint32_t)__shfl_xor((int)v, d, 64);
    return v;
}

// One strand of an item, counted in full: the tile loop of ibf_count_lists_kernel without the bound, the strand skip and the stop.
template <int LINES, bool NT>
__device__ __forceinline__ void list_count_strand(const IbfDev &f, uint32_t *cnt, uint8_t *stage, const uint32_t *__restrict__ slots,
                                                  const uint64_t *__restrict__ side, uint32_t side_rows, const ListBaseSrc &seq, uint32_t len,
                                                  uint32_t n, int strand, uint32_t lane, uint32_t spare)
{
    constexpr uint32_t R = LINES == 4 ? 32 : 64;  // slots per batch (list_batch)
    const uint32_t k = f.k;
    uint32_t ahead0 = 0, ahead1 = 0;  // a tile's bases, loaded one tile ahead
    bool ahead = false;
#pragma unroll 1
    for (uint32_t mt = 0; mt < n; mt += 64) {
        const uint32_t wlen = min(64u + k - 1u, len - mt);
        if (!ahead) {  // wave-uniform
            ahead0 = lane < wlen ? seq.raw(mt + lane) : 0u;
            ahead1 = lane + 64u < wlen ? seq.raw(mt + 64u + lane) : 0u;
        }
        __builtin_amdgcn_wave_barrier();
        if (lane < wlen) stage[lane] = (uint8_t)seq.ord_of(ahead0, mt + lane);
        if (lane + 64u < wlen) stage[lane + 64u] = (uint8_t)seq.ord_of(ahead1, mt + 64u + lane);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
        __builtin_amdgcn_wave_barrier();
        const uint32_t p = mt + lane;
        uint32_t rank = 0;
        if (p < n) {
            const uint8_t *b = stage + lane;
            if (strand == 0) {
                for (uint32_t i = 0; i < k; ++i) rank = (rank << 2) | (b[i] & 3u);
            } else {
                for (uint32_t i = 0; i < k; ++i) rank = (rank << 2) | (rbspec::dna5_comp(b[k - 1 - i], f.comp_n) & 3u);
            }
        }
        const uint32_t in_tile = __builtin_amdgcn_readfirstlane(min(64u, n - mt));
        ahead = mt + 64u < n;
        if (ahead) {
            const uint32_t next = min(64u + k - 1u, len - (mt + 64u));
            ahead0 = lane < next ? seq.raw(mt + 64u + lane) : 0u;
            ahead1 = lane + 64u < next ? seq.raw(mt + 128u + lane) : 0u;
            __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll 1
        for (uint32_t first = 0; first < in_tile; first += R) {
            if (first + R <= in_tile)  // wave-uniform
                list_batch<LINES, NT, true>(f, cnt, slots, side, side_rows, rank, first, in_tile, lane, spare);
            else
                list_batch<LINES, NT, false>(f, cnt, slots, side, side_rows, rank, first, in_tile, lane, spare);
        }
    }
}

// The RANGED count (the list form of the prefix pass): the k-mers [n_from, n_to) of one strand of the item's first `len` bases, n_to ==
// len - k + 1 -- list_count_strand's tile loop begun at k-mer n_from instead of 0, so a tile starts wherever the last checkpoint ended,
// at a multiple of 64 or not: ListBaseSrc::raw / ord_of address single bases at any offset.  The counters are added to, not cleared.
// Kept beside list_count_strand and not under it, so that the kernels of locate, hits and resume compile as they did.
template <int LINES, bool NT>
__device__ __forceinline__ void list_count_range(const IbfDev &f, uint32_t *cnt, uint8_t *stage, const uint32_t *__restrict__ slots,
                                                 const uint64_t *__restrict__ side, uint32_t side_rows, const ListBaseSrc &seq, uint32_t len,
                                                 uint32_t n_from, uint32_t n_to, int strand, uint32_t lane, uint32_t spare)
{
    constexpr uint32_t R = LINES == 4 ? 32 : 64;  // slots per batch (list_batch)
    const uint32_t k = f.k;
    uint32_t ahead0 = 0, ahead1 = 0;  // a tile's bases, loaded one tile ahead
    bool ahead = false;
#pragma unroll 1
    for (uint32_t mt = n_from; mt < n_to; mt += 64) {
        const uint32_t wlen = min(64u + k - 1u, len - mt);
        if (!ahead) {  // wave-uniform
            ahead0 = lane < wlen ? seq.raw(mt + lane) : 0u;
            ahead1 = lane + 64u < wlen ? seq.raw(mt + 64u + lane) : 0u;
        }
        __builtin_amdgcn_wave_barrier();
        if (lane < wlen) stage[lane] = (uint8_t)seq.ord_of(ahead0, mt + lane);
        if (lane + 64u < wlen) stage[lane + 64u] = (uint8_t)seq.ord_of(ahead1, mt + 64u + lane);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
        __builtin_amdgcn_wave_barrier();
        const uint32_t p = mt + lane;
        uint32_t rank = 0;
        if (p < n_to) {
            const uint8_t *b = stage + lane;
            if (strand == 0) {
                for (uint32_t i = 0; i < k; ++i) rank = (rank << 2) | (b[i] & 3u);
            } else {
                for (uint32_t i = 0; i < k; ++i) rank = (rank << 2) | (rbspec::dna5_comp(b[k - 1 - i], f.comp_n) & 3u);
            }
        }
        const uint32_t in_tile = __builtin_amdgcn_readfirstlane(min(64u, n_to - mt));
        ahead = mt + 64u < n_to;
        if (ahead) {
            const uint32_t next = min(64u + k - 1u, len - (mt + 64u));
            ahead0 = lane < next ? seq.raw(mt + 64u + lane) : 0u;
            ahead1 = lane + 64u < next ? seq.raw(mt + 128u + lane) : 0u;
            __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll 1
        for (uint32_t first = 0; first < in_tile; first += R) {
            if (first + R <= in_tile)  // wave-uniform
                list_batch<LINES, NT, true>(f, cnt, slots, side, side_rows, rank, first, in_tile, lane, spare);
            else
                list_batch<LINES, NT, false>(f, cnt, slots, side, side_rows, rank, first, in_tile, lane, spare);
        }
    }
}

}  // namespace rb

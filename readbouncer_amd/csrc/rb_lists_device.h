// rb_lists_device.h -- the device code the list kernels share: how a read's bases are found (what rb_lists.hip needs of rb_kernels.hip,
// written again), the adds into the per-bin LDS counters, the scan for their maximum and one batch of slot gathers.  Included by
// rb_lists.hip (the count kernel and the table) and rb_pass_lists.hip (the list forms of locate and hits); HIP translation units only.
#pragma once
#include <hip/hip_runtime.h>

#include "rb_device.h"
#include "rb_lists.h"

namespace rb {

// (BaseSrc and make_base_src of rb_kernels.hip)
struct ListBaseSrc {
    const uint8_t *bytes;
    const uint8_t *nm;
    uint32_t first;
    // base i in two halves, so that the load can be issued well before the ordinal is needed: what is loaded, and the ordinal from it
    __device__ __forceinline__ uint32_t raw(uint32_t i) const
    {
        if (nm == nullptr) return bytes[i];
        const uint32_t b = first + i;
        return (uint32_t)bytes[b >> 2] | ((uint32_t)nm[b >> 3] << 8);
    }
    __device__ __forceinline__ uint32_t ord_of(uint32_t loaded, uint32_t i) const
    {
        if (nm == nullptr) return rbspec::dna5_ord(loaded);
        const uint32_t b = first + i;
        const uint32_t code = ((loaded & 0xFFu) >> ((b & 3u) << 1)) & 3u;
        return ((loaded >> (8u + (b & 7u))) & 1u) ? 4u : code;
    }
    __device__ __forceinline__ uint32_t ord(uint32_t i) const { return ord_of(raw(i), i); }
};

__device__ __forceinline__ ListBaseSrc make_list_base_src(const ReadSrc &r, uint32_t item, uint32_t *len_out)
{
    const uint32_t rid = r.ids ? r.ids[item] : item;
    const uint32_t len = r.lens[item];
    *len_out = (r.max_len && len > r.max_len) ? r.max_len : len;  // never beyond the declared bound
    ListBaseSrc b;
    if (r.nmask) {
        b.bytes = r.seqs + r.offsets[rid];
        b.nm = r.nmask + r.nmask_offsets[rid];
        b.first = r.base_off;
    } else {
        b.bytes = r.seqs + r.offsets[rid] + r.base_off;
        b.nm = nullptr;
        b.first = 0;
    }
    return b;
}

__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, d, 64));
    return v;
}

// one bin of a dense row: an add into its half of the counter dword; nothing comes back (the maximum is found by list_scan)
__device__ __forceinline__ void count_bin(uint32_t *cnt, uint32_t bin, uint32_t n_bins)
{
    if (bin < n_bins) __hip_atomic_fetch_add(&cnt[bin >> 1], 1u << ((bin & 1u) << 4), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// The two halves of a slot's dword in the resident form (rb_lists.h), from a group of slots that carries no flag: each half IS the byte
// offset of a counter dword -- a bin's, or the spare of the lane that holds the dword, where junk collects that nothing reads -- and its
// place is the parity, so the low half adds 1 and the high half 1 << 16.  No control flow and no value back: a group of slots issues
// its adds back to back and waits for none of them.  One vector instruction per add forms the address (the counters' base plus a
// 16-bit half).  (No two lanes share a spare: adds to one address serialise.)
__device__ __forceinline__ void list_add2(uint32_t *cnt, uint32_t v)
{
    char *base = reinterpret_cast<char *>(cnt);
    __hip_atomic_fetch_add(reinterpret_cast<uint32_t *>(base + (v & 0xFFFFu)), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    __hip_atomic_fetch_add(reinterpret_cast<uint32_t *>(base + (v >> 16)), 0x10000u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// A dword with a swapped half (kResidentSwapped: a bin of the other parity): that half is added here with the other constant and
// replaced by the lane's spare, so that list_add2 finds no flag.  `counts`: the lane takes part in the adds.
__device__ __forceinline__ uint32_t list_add_swapped(uint32_t *cnt, uint32_t v, uint32_t spare_off, bool counts)
{
    char *base = reinterpret_cast<char *>(cnt);
    if (v & rblist::kResidentSwapped) {
        if (counts)
            __hip_atomic_fetch_add(reinterpret_cast<uint32_t *>(base + (v & rblist::kResidentOffset)), 0x10000u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        v = (v & 0xFFFF0000u) | spare_off;
    }
    if (v & (rblist::kResidentSwapped << 16)) {
        if (counts)
            __hip_atomic_fetch_add(reinterpret_cast<uint32_t *>(base + ((v >> 16) & rblist::kResidentOffset)), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        v = (v & 0x0000FFFFu) | (spare_off << 16);
    }
    return v;
}

typedef unsigned int list_u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned short list_u16x2 __attribute__((ext_vector_type(2)));
constexpr uint32_t kListSpareDwords = rblist::kCountSpareDwords;  // one per lane, behind the counters

__device__ __forceinline__ list_u16x2 list_max2(list_u16x2 a, uint32_t dword)
{
    return __builtin_elementwise_max(a, __builtin_bit_cast(list_u16x2, dword));
}

// The largest counter: every lane reads 16-byte pieces of the cnt_dwords counter dwords (a multiple of 256: whole pieces, the same
// number for every lane) and keeps the packed maximum of their halves; one wave reduction at the end.  The spares are not looked at.
// CLEAR: the pieces are zeroed behind the read, for the next strand.
template <bool CLEAR>
__device__ __forceinline__ uint32_t list_scan(uint32_t *cnt, uint32_t cnt_dwords, uint32_t lane)
{
    uint4 *c4 = reinterpret_cast<uint4 *>(cnt);
    list_u16x2 a = {0, 0};
    for (uint32_t i = lane; i < cnt_dwords / 4; i += 64) {
        const uint4 q = c4[i];
        a = __builtin_elementwise_max(list_max2(list_max2(a, q.x), q.y), list_max2(__builtin_bit_cast(list_u16x2, q.z), q.w));
        if (CLEAR) c4[i] = make_uint4(0, 0, 0, 0);
    }
    return (uint32_t)__builtin_amdgcn_readfirstlane(wave_max_u32(max((uint32_t)a.x, (uint32_t)a.y)));
}

// One batch of R slots, `first` the tile's k-mer the batch begins at.  FULL: all R slots lie within the strand, and nothing is guarded;
// otherwise a slot past the end stays blank (the lane's spare in both halves) and a group of eight that begins past the end is skipped.
// `spare` is the lane's spare dword, cnt_dwords + lane: what the table's non-bin halves name in the dwords this lane reads
// (rblist::resident_spare_dword), so a blanked slot adds where an empty one would.
template <int LINES, bool NT, bool FULL>
__device__ __forceinline__ void list_batch(const IbfDev &f, uint32_t *cnt, const uint32_t *__restrict__ slots, const uint64_t *__restrict__ side,
                                           uint32_t side_rows, uint32_t rank, uint32_t first, uint32_t in_tile, uint32_t lane, uint32_t spare)
{
    constexpr int DW = LINES == 4 ? 2 : 1;  // dwords per lane and slot
    constexpr int R = 64 / DW;              // slots gathered back to back: 64 registers of a lane either way
    constexpr int G = 8;
    constexpr uint32_t SLOT_DWORDS = LINES * 32;
    const uint32_t lane_dword = LINES == 1 ? (lane & 31u) : lane * DW;
    const uint32_t spare_off = spare * 4u, blank = spare_off * 0x10001u;
    // ---- the gathers, back to back
    uint32_t v[R][DW];
#pragma unroll
    for (int u = 0; u < R; ++u) {
#pragma unroll
        for (int d = 0; d < DW; ++d) v[u][d] = blank;
        if (FULL || first + (uint32_t)u < in_tile) {  // wave-uniform
            const uint32_t slot = (uint32_t)__builtin_amdgcn_readlane((int)rank, (int)((R == 64 ? 0 : first) + u));
            const uint32_t *base = slots + (size_t)slot * SLOT_DWORDS;  // slot < 4^k: masked digits; wave-uniform
            if constexpr (DW == 2) {
                const list_u32x2 *p2 = reinterpret_cast<const list_u32x2 *>(base + lane_dword);
                const list_u32x2 q = NT ? __builtin_nontemporal_load(p2) : *p2;
                v[u][0] = q.x;
                v[u][1] = q.y;
            } else {
                v[u][0] = NT ? __builtin_nontemporal_load(base + lane_dword) : base[lane_dword];
            }
        }
    }
    __builtin_amdgcn_sched_barrier(0);
    uint64_t overflow = 0;  // the batch's overflow slots
#pragma unroll
    for (int g = 0; g < R / G; ++g) {
        if (FULL || first + (uint32_t)(g * G) < in_tile) {  // wave-uniform
            // the group's dwords ORed: a flag in any lane (rb_lists.h: an overflow slot, a swapped half) sends the group down the
            // careful path, which leaves its slots without one
            uint32_t fold = 0;
#pragma unroll
            for (int u = 0; u < G; ++u)
#pragma unroll
                for (int d = 0; d < DW; ++d) fold |= v[g * G + u][d];
            if (__builtin_expect(__ballot((fold & rblist::kResidentFlags) != 0u) != 0ULL, 0)) {  // wave-uniform, rare
                const bool counts = LINES != 1 || lane < 32;
#pragma unroll
                for (int u = 0; u < G; ++u) {
                    const int s = g * G + u;
                    const uint32_t d0 = (uint32_t)__builtin_amdgcn_readlane((int)v[s][0], 0);  // dword 0 of the slot
                    if (d0 & rblist::kResidentOverflow) {  // wave-uniform: set aside, and blanked (its index is no address)
                        overflow |= 1ull << s;
#pragma unroll
                        for (int d = 0; d < DW; ++d) v[s][d] = blank;
                    } else {
#pragma unroll
                        for (int d = 0; d < DW; ++d)
                            if (v[s][d] & rblist::kResidentFlags) v[s][d] = list_add_swapped(cnt, v[s][d], spare_off, counts);
                    }
                }
            }
            if (LINES != 1 || lane < 32) {  // a one-line slot is 32 dwords: the upper half of the wave sits the adds out
#pragma unroll
                for (int u = 0; u < G; ++u)
#pragma unroll
                    for (int d = 0; d < DW; ++d) list_add2(cnt, v[g * G + u][d]);
            }
        }
    }
    while (overflow) {  // wave-uniform, rare: the slot's index dword once more, then the dense row's set bits one by one
        const int u = __builtin_ctzll(overflow);
        overflow &= overflow - 1;
        const uint32_t slot = (uint32_t)__builtin_amdgcn_readlane((int)rank, (int)(R == 64 ? 0 : first) + u);
        const uint32_t idx = slots[(size_t)slot * SLOT_DWORDS + 1];
        if (idx >= side_rows) continue;  // (the builder never names a row it did not write)
        const uint64_t *row = side + (size_t)idx * f.stride;
        for (uint32_t w = lane; w < f.bin_width; w += 64) {
            uint64_t word = row[w];
            while (word) {
                const uint32_t bit = (uint32_t)__builtin_ctzll(word);
                word &= word - 1;
                count_bin(cnt, w * 64u + bit, f.n_bins);
            }
        }
    }
}

}  // namespace rb

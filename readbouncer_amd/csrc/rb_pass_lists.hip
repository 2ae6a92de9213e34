// rb_pass_lists.hip -- the LIST FORMS of the locate and hits passes (rb_engine_set_pass_lists): the kernels that serve them from a filter's
// list table (rb_lists.h) with the wave of ibf_count_lists_kernel, and the small kernel that says which work items they take.  A translation
// unit of its own beside rb_lists.hip, whose device code it shares through rb_lists_device.h; what it shares in turn with the list form of
// the resume pass (rb_resume_lists.hip) -- pass_lists_takes and list_count_strand -- is in rb_pass_lists_device.h.
#include <hip/hip_runtime.h>

#include "rb_device.h"
#include "rb_lists.h"
#include "rb_lists_device.h"
#include "rb_pass_lists_device.h"

namespace rb {

// ... decided once per call, one wave per item: the ONE predicate of both sides.  The list kernels read taken[]; the plain kernels are
// launched as they are, with plain_lens[] for the items' lengths -- 0 for a taken item, so they count nothing of it.
__global__ __launch_bounds__(256) void pass_lists_prep_kernel(ReadSrc src, uint32_t n_items, const uint8_t *__restrict__ pre_status, uint32_t min_len,
                                                              uint8_t *__restrict__ taken, uint32_t *__restrict__ plain_lens)
{
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t item = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (item >= n_items) return;  // wave-uniform
    const bool takes = pass_lists_takes(src, item, pre_status, min_len, lane);
    if (lane == 0) {
        taken[item] = takes ? 1 : 0;
        plain_lens[item] = takes ? 0u : src.lens[item];
    }
}

hipError_t launch_pass_lists_prep(const PassListsPrep &a, hipStream_t st)
{
    if (a.n_items == 0) return hipSuccess;
    if (!a.taken || !a.plain_lens || !a.src.lens) return hipErrorInvalidValue;
    hipLaunchKernelGGL(pass_lists_prep_kernel, dim3((a.n_items + 3) / 4), dim3(256), 0, st, a.src, a.n_items, a.pre_status, a.min_len, a.taken,
                       a.plain_lens);
    return hipGetLastError();
}

// ---- THE LIST FORMS OF LOCATE AND HITS: ibf_count_lists_kernel's wave -- one workgroup, one work item, the same slot gathers through
// list_batch, the same tile loop and ranks -- counted in full on both strands, with a richer scan at each strand's end.  They take the
// items the prep kernel marked in taken[]; the plain kernels take the others.  LDS: the count kernel's counters, spares and stage, then
// the hit mask (rblist::pass_lds_bytes), one byte per 16-byte piece of the counters: bit j of byte i is bin 8 i + j.  The lane that scans
// piece i on the first strand scans it on the second.

// LOCATE's scan of a strand's counters, lane l at the pieces l, l + 64, ... as list_scan.  -> wave-uniform (maximum << 16) | (0xFFFF - the
// lowest bin at it), 0 when nothing counted: a lane's pieces rise, so only a LARGER counter moves its first bin, and the wave's largest key
// is the largest maximum at its lowest bin.  FIRST (the forward strand): the bits of the bins at or above t go to the mask and the piece is
// cleared for the next strand; otherwise they are ORed with the mask's, and *hit_bins is the wave's count of set bits.
template <bool FIRST>
__device__ __forceinline__ uint32_t locate_scan(uint32_t *cnt, uint8_t *mask, uint32_t cnt_dwords, uint32_t n_bins, uint32_t t, uint32_t lane,
                                                uint32_t *hit_bins)
{
    uint4 *c4 = reinterpret_cast<uint4 *>(cnt);
    uint32_t m = 0, bin = 0, hits = 0;
    for (uint32_t i = lane; i < cnt_dwords / 4; i += 64) {
        const uint4 q = c4[i];
        const uint32_t mx = piece_max(q);
        if (mx > m) {
            m = mx;
            uint32_t j = 7;
#pragma unroll
            for (int u = 6; u >= 0; --u) j = piece_counter(q, u) == mx ? (uint32_t)u : j;
            bin = i * 8u + j;
        }
        const uint32_t bits = mx >= t ? piece_hits(q, i, t, n_bins) : 0u;  // (t == 0: every piece)
        if (FIRST) {
            mask[i] = (uint8_t)bits;
            c4[i] = make_uint4(0, 0, 0, 0);
        } else {
            hits += (uint32_t)__builtin_popcount(bits | mask[i]);
        }
    }
    if (!FIRST) *hit_bins = (uint32_t)__builtin_amdgcn_readfirstlane(wave_sum_u32(hits));
    const uint32_t key = m ? (m << 16) | (0xFFFFu - bin) : 0u;  // bin < kMaxBins, m <= kMaxKmers
    return (uint32_t)__builtin_amdgcn_readfirstlane(wave_max_u32(key));
}

template <int LINES, bool NT>
__global__ __launch_bounds__(64) void ibf_locate_lists_kernel(IbfDev f, const uint32_t *__restrict__ slots, const uint64_t *__restrict__ side,
                                                              uint32_t side_rows, ReadSrc src, uint32_t n_items, const uint16_t *__restrict__ thr,
                                                              uint32_t thr_len, uint32_t nf, uint32_t fi, const uint8_t *__restrict__ taken,
                                                              LocatePart *__restrict__ part, uint32_t cnt_dwords)
{
    static_assert(LINES == 1 || LINES == 2 || LINES == 4, "slot sizes of rb_lists.h");
    extern __shared__ uint32_t s_lds[];
    uint32_t *cnt = s_lds;                                                                 // as ibf_count_lists_kernel: counters, spares,
    uint8_t *stage = reinterpret_cast<uint8_t *>(s_lds + cnt_dwords + kListSpareDwords);  // stage,
    uint8_t *mask = stage + rblist::kCountStageBytes;                                      // and cnt_dwords / 4 bytes of hit mask
    const uint32_t lane = threadIdx.x;
    const uint32_t item = blockIdx.x;
    if (item >= n_items) return;
    if (!taken[item]) return;  // wave-uniform: the plain kernel's item

    uint32_t len;
    const ListBaseSrc seq = make_list_base_src(src, item, &len);
    const uint32_t n = len >= f.k ? len - f.k + 1 : 0;
    // t: the threshold the decision kernel reads for this length and filter (make_pass_wave's)
    const uint32_t tl = len < thr_len ? len : thr_len - 1;
    const uint32_t t = __builtin_amdgcn_readfirstlane((uint32_t)thr[((size_t)tl * nf + fi) * 2]);
    const uint32_t spare = cnt_dwords + lane;
    {  // the first strand's counters; the second strand's are cleared by the scan that ends the first
        __builtin_amdgcn_wave_barrier();
        uint4 *c4 = reinterpret_cast<uint4 *>(cnt);
        for (uint32_t i = lane; i < cnt_dwords / 4; i += 64) c4[i] = make_uint4(0, 0, 0, 0);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
        __builtin_amdgcn_wave_barrier();
    }
    uint32_t best = 0, best_bin = 0, best_strand = 0, hit_bins = 0;
#pragma unroll 1
    for (int strand = 0; strand < 2; ++strand) {
        list_count_strand<LINES, NT>(f, cnt, stage, slots, side, side_rows, seq, len, n, strand, lane, spare);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
        const uint32_t key = strand == 0 ? locate_scan<true>(cnt, mask, cnt_dwords, f.n_bins, t, lane, &hit_bins)
                                         : locate_scan<false>(cnt, mask, cnt_dwords, f.n_bins, t, lane, &hit_bins);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
        // rb_locate_out's rule, as ibf_locate_kernel combines its strands: the larger maximum; on equal maxima the lower first bin, and
        // strand 0 keeps an equal bin
        const uint32_t m = key >> 16, first = 0xFFFFu - (key & 0xFFFFu);
        if (m > 0 && (m > best || (m == best && first < best_bin))) {
            best_bin = first;
            best_strand = (uint32_t)strand;
        }
        best = max(best, m);
    }
    if (lane == 0) {
        LocatePart rec;
        rec.max_count = best;
        rec.first_bin = best_bin;
        rec.strand = best_strand;
        rec.hit_bins = hit_bins;
        part[item] = rec;  // slice 0 of one
    }
}

// HITS' scan of a strand's counters, in bin order: a round of the wave is 64 consecutive pieces, 512 bins, lane l at the round's piece l.
// Where a round holds a hit (one ballot; the common round holds none) a prefix sum over the lanes' hit counts places every lane's
// records behind those of the lower bins, and the lane stores its (bin, count | strand << 16) while their number is below max_hits.
// -> the strand's hits, whatever max_hits is.  FIRST: the piece's bits go to the mask and the piece is cleared; otherwise bin_reads
// (optional) takes one add per bit of mask | own -- the distinct hit bins of the item.
template <bool FIRST>
__device__ __forceinline__ uint32_t hits_scan(uint32_t *cnt, uint8_t *mask, uint32_t cnt_dwords, uint32_t n_bins, uint32_t t, uint32_t lane,
                                              uint32_t strand, rb_u32x2 *__restrict__ out, uint32_t max_hits,
                                              unsigned long long *__restrict__ bin_reads)
{
    uint4 *c4 = reinterpret_cast<uint4 *>(cnt);
    uint32_t total = 0;  // wave-uniform
    for (uint32_t round = 0; round < cnt_dwords / 4; round += 64) {  // (cnt_dwords / 4 is a multiple of 64: every lane has a piece)
        const uint32_t i = round + lane;
        const uint4 q = c4[i];
        const uint32_t bits = piece_max(q) >= t ? piece_hits(q, i, t, n_bins) : 0u;
        if (FIRST) {
            mask[i] = (uint8_t)bits;
            c4[i] = make_uint4(0, 0, 0, 0);
        } else if (bin_reads) {  // uniform
            uint32_t seen = bits | mask[i];
            while (seen) {
                const uint32_t j = (uint32_t)__builtin_ctz(seen);
                seen &= seen - 1;
                atomicAdd(bin_reads + (i * 8u + j), 1ULL);  // a set bit is a bin below n_bins
            }
        }
        if (__ballot(bits != 0u) == 0ULL) continue;  // wave-uniform
        const uint32_t mine = (uint32_t)__builtin_popcount(bits);
        uint32_t incl = mine;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t o = (uint32_t)__shfl_up((int)incl, d, 64);
            if (lane >= (uint32_t)d) incl += o;
        }
        uint32_t pos = total + incl - mine;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            if ((bits >> j) & 1u) {
                if (pos < max_hits) {  // inside the segment
                    rb_u32x2 rec;
                    rec.x = i * 8u + (uint32_t)j;
                    rec.y = piece_counter(q, j) | (strand << 16);
                    out[pos] = rec;
                }
                ++pos;
            }
        }
        total += (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
    }
    return total;
}

// The record and segment formats are ibf_hits_kernel's, byte for byte: seg[item][slice 0 of one][strand][0 .. max_hits) and
// seg_count[slice 0][strand][item]; launch_finish_hits merges the two strands' runs as it does behind that kernel.
template <int LINES, bool NT>
__global__ __launch_bounds__(64) void ibf_hits_lists_kernel(IbfDev f, const uint32_t *__restrict__ slots, const uint64_t *__restrict__ side,
                                                            uint32_t side_rows, ReadSrc src, uint32_t n_items, const uint16_t *__restrict__ thr,
                                                            uint32_t thr_len, uint32_t nf, uint32_t fi, uint32_t min_count, uint32_t max_hits,
                                                            const uint8_t *__restrict__ taken, rb_u32x2 *__restrict__ seg,
                                                            uint32_t *__restrict__ seg_count, unsigned long long *__restrict__ bin_reads,
                                                            uint32_t cnt_dwords)
{
    static_assert(LINES == 1 || LINES == 2 || LINES == 4, "slot sizes of rb_lists.h");
    extern __shared__ uint32_t s_lds[];
    uint32_t *cnt = s_lds;
    uint8_t *stage = reinterpret_cast<uint8_t *>(s_lds + cnt_dwords + kListSpareDwords);
    uint8_t *mask = stage + rblist::kCountStageBytes;
    const uint32_t lane = threadIdx.x;
    const uint32_t item = blockIdx.x;
    if (item >= n_items) return;
    if (!taken[item]) return;  // wave-uniform: the plain kernel's item, or none's (not RB_OK)

    uint32_t len;
    const ListBaseSrc seq = make_list_base_src(src, item, &len);
    const uint32_t n = len >= f.k ? len - f.k + 1 : 0;
    // t: the caller's threshold, or the one the decision kernel reads for this length and filter (make_pass_wave's)
    const uint32_t tl = len < thr_len ? len : thr_len - 1;
    const uint32_t t = min_count ? min_count : __builtin_amdgcn_readfirstlane((uint32_t)thr[((size_t)tl * nf + fi) * 2]);
    const uint32_t spare = cnt_dwords + lane;
    {
        __builtin_amdgcn_wave_barrier();
        uint4 *c4 = reinterpret_cast<uint4 *>(cnt);
        for (uint32_t i = lane; i < cnt_dwords / 4; i += 64) c4[i] = make_uint4(0, 0, 0, 0);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
        __builtin_amdgcn_wave_barrier();
    }
#pragma unroll 1
    for (uint32_t strand = 0; strand < 2; ++strand) {
        list_count_strand<LINES, NT>(f, cnt, stage, slots, side, side_rows, seq, len, n, (int)strand, lane, spare);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
        rb_u32x2 *out = seg + ((size_t)item * 2 + strand) * max_hits;
        const uint32_t total = strand == 0 ? hits_scan<true>(cnt, mask, cnt_dwords, f.n_bins, t, lane, strand, out, max_hits, bin_reads)
                                           : hits_scan<false>(cnt, mask, cnt_dwords, f.n_bins, t, lane, strand, out, max_hits, bin_reads);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
        if (lane == 0) seg_count[(size_t)strand * n_items + item] = total;
    }
}

// ---- locate and hits from the list table
bool pass_list_form_serves(const PlainPassLaunch &a)
{
    CountLaunch c{};
    c.f = a.f;
    c.src = a.src;
    c.lg = a.lg;
    c.wpl = a.wpl;
    c.planes = a.planes;
    c.n_slices = a.n_slices;
    return list_form_serves(c) && a.col_begin == 0 && a.col_end == a.f.bin_width;
}

static bool pass_lists_launch_ok(const PlainPassLaunch &a)
{
    return a.thr && a.thr_len && a.list_table && a.list_side && a.list_taken && a.list_plain_lens && rblist::lines_valid(a.list_lines) && pass_list_form_serves(a);
}

template <int LINES>
static hipError_t launch_locate_lists_nt(const LocateLaunch &a, hipStream_t st)
{
    const uint32_t cnt_dwords = rblist::count_cnt_dwords(a.f.n_bins);
    const size_t lds = rblist::pass_lds_bytes(a.f.n_bins);
    const uint32_t *slots = reinterpret_cast<const uint32_t *>(a.list_table);
    auto kern = a.list_nt ? &ibf_locate_lists_kernel<LINES, true> : &ibf_locate_lists_kernel<LINES, false>;
    hipLaunchKernelGGL(kern, dim3(a.n_items), dim3(64), lds, st, a.f, slots, a.list_side, a.list_side_rows, a.src, a.n_items, a.thr, a.thr_len, a.nf,
                       a.fi, a.list_taken, a.part, cnt_dwords);
    return hipGetLastError();
}

// The items the list kernel leaves from the filter's own table -- the plain launch as it is, over the lengths of launch_pass_lists_prep:
// a taken item has no k-mer there, so it costs a wave that counts nothing and leaves an empty record -- then the taken items from the list
// table, whose records stand.
hipError_t launch_ibf_locate_lists(const LocateLaunch &a, hipStream_t st)
{
    if (a.n_items == 0) return hipSuccess;
    if (!a.part || !pass_lists_launch_ok(a)) return hipErrorInvalidValue;
    LocateLaunch plain = a;
    plain.src.lens = a.list_plain_lens;
    hipError_t e = launch_ibf_locate(plain, st);
    if (e != hipSuccess) return e;
    return a.list_lines == 1 ? launch_locate_lists_nt<1>(a, st) : a.list_lines == 2 ? launch_locate_lists_nt<2>(a, st) : launch_locate_lists_nt<4>(a, st);
}

template <int LINES>
static hipError_t launch_hits_lists_nt(const HitsLaunch &a, hipStream_t st)
{
    const uint32_t cnt_dwords = rblist::count_cnt_dwords(a.f.n_bins);
    const size_t lds = rblist::pass_lds_bytes(a.f.n_bins);
    const uint32_t *slots = reinterpret_cast<const uint32_t *>(a.list_table);
    auto kern = a.list_nt ? &ibf_hits_lists_kernel<LINES, true> : &ibf_hits_lists_kernel<LINES, false>;
    hipLaunchKernelGGL(kern, dim3(a.n_items), dim3(64), lds, st, a.f, slots, a.list_side, a.list_side_rows, a.src, a.n_items, a.thr, a.thr_len, a.nf,
                       a.fi, a.min_count, a.max_hits, a.list_taken, (rb_u32x2 *)a.seg, a.seg_count, (unsigned long long *)a.bin_reads,
                       cnt_dwords);
    return hipGetLastError();
}

// As locate's.  The plain kernel leaves an item whose length is below min_len before it writes anything, and a taken item's is 0 there:
// every segment, counter and profile entry is written once.
hipError_t launch_ibf_hits_lists(const HitsLaunch &a, hipStream_t st)
{
    if (a.n_items == 0) return hipSuccess;
    if (!a.seg_count || (a.max_hits && !a.seg) || a.min_len == 0 || !pass_lists_launch_ok(a)) return hipErrorInvalidValue;
    HitsLaunch plain = a;
    plain.src.lens = a.list_plain_lens;
    hipError_t e = launch_ibf_hits(plain, st);
    if (e != hipSuccess) return e;
    return a.list_lines == 1 ? launch_hits_lists_nt<1>(a, st) : a.list_lines == 2 ? launch_hits_lists_nt<2>(a, st) : launch_hits_lists_nt<4>(a, st);
}

}  // namespace rb

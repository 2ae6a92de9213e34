// rb_wide_pass_lists.hip -- the WIDE LIST FORMS of the locate and hits passes (rb_engine_set_wide_pass_lists): the kernels that serve
// them from a filter's wide list table (rb_wide_lists.h, 8193 to 32 256 bins) with the workgroup of ibf_count_wide_lists_kernel, and the
// small kernel that says which work items they take.  A translation unit of its own beside rb_wide_lists.hip, whose device code it shares
// through rb_wide_lists_device.h; the reading of a 16-byte piece of the counters is rb_pass_lists_device.h's, as the one-wave forms'.
#include <hip/hip_runtime.h>

#include "rb_device.h"
#include "rb_lists.h"
#include "rb_lists_device.h"
#include "rb_pass_lists_device.h"
#include "rb_wide_lists.h"
#include "rb_wide_lists_device.h"

namespace rb {

// Which work items the wide kernels take, decided once per call, one thread per item: the item is RB_OK by item_status's rules -- chunk_prep's
// verdict, the declared bound, the engine's largest k.  No look at the bases: the wide kernels count a k-mer with a base outside ACGT
// themselves.  taken[] and plain_lens[] as pass_lists_prep_kernel writes them: the plain kernels run over plain_lens[], 0 for a taken item.
__global__ __launch_bounds__(256) void wide_pass_lists_prep_kernel(ReadSrc src, uint32_t n_items, const uint8_t *__restrict__ pre_status,
                                                                   uint32_t min_len, uint8_t *__restrict__ taken, uint32_t *__restrict__ plain_lens)
{
    const uint32_t item = blockIdx.x * 256u + threadIdx.x;
    if (item >= n_items) return;
    const uint32_t len = src.lens[item];
    const bool takes = !(pre_status && pre_status[item] != RB_OK) && len <= src.max_len && len >= min_len;
    taken[item] = takes ? 1 : 0;
    plain_lens[item] = takes ? 0u : len;
}

hipError_t launch_wide_pass_lists_prep(const PassListsPrep &a, hipStream_t st)
{
    if (a.n_items == 0) return hipSuccess;
    if (!a.taken || !a.plain_lens || !a.src.lens) return hipErrorInvalidValue;
    hipLaunchKernelGGL(wide_pass_lists_prep_kernel, dim3((a.n_items + 255) / 256), dim3(256), 0, st, a.src, a.n_items, a.pre_status, a.min_len,
                       a.taken, a.plain_lens);
    return hipGetLastError();
}

// ---- THE WIDE FORMS OF LOCATE AND HITS: ibf_count_wide_lists_kernel's workgroup -- NW waves, one work item, one shared array of 16-bit
// counters, the tiles dealt round-robin (wide_count_strand) -- counted in full on both strands, with the richer scan of rb_pass_lists.hip
// at each strand's end, spread across the waves.
// THE SCAN'S SHARES.  The counters are cnt_dwords / 4 pieces of 16 bytes, a multiple of 64: `rounds` rounds of 64 consecutive pieces, lane
// l at piece l of a round.  Wave w takes the rounds [w x per, (w + 1) x per) that exist, per = ceil(rounds / NW) <= 16: every wave's share
// is one stretch of rising bins, and the waves' stretches rise with the wave.
// THE HIT MASK lives in registers.  LDS is the count kernel's to the byte (rbwide::pass_lds_bytes: 65 344 of 65 536 bytes at 32 256
// bins, where the one-wave forms' mask of a byte per piece would add 4032), and the thread that scans a piece on the first strand scans
// it on the second: its at most 16 pieces are 16 bytes, two 64-bit registers, byte j the piece of its wave's round j.
// Exchanges across the waves go through red[] (kWideReduceBytes behind the stage areas): two dwords per wave.
// (WideShare<NW> itself is in rb_wide_lists_device.h, shared with the wide form of the prefix pass.)
static_assert(rbwide::pass_rounds_per_wave(rbwide::kWideMaxBins) <= rbwide::kWidePassMaskBytes && rbwide::kWidePassMaskBytes == 16,
              "a thread's pieces fit the two 64-bit registers of its mask (rb_wide_lists.h restates the shares for the host)");

// byte j (wave-uniform) of a thread's 16 mask bytes
__device__ __forceinline__ uint32_t wide_mask_get(uint64_t lo, uint64_t hi, uint32_t j)
{
    return (uint32_t)((j < 8u ? lo : hi) >> ((j & 7u) * 8u)) & 0xFFu;
}
__device__ __forceinline__ void wide_mask_or(uint64_t &lo, uint64_t &hi, uint32_t j, uint32_t bits)
{
    const uint64_t v = (uint64_t)bits << ((j & 7u) * 8u);
    if (j < 8u) lo |= v;
    else hi |= v;
}

// LOCATE.  Each wave reduces its share to locate_scan's key, (maximum << 16) | (0xFFFF - the lowest bin at it): a thread's pieces rise, so
// only a LARGER counter moves its first bin; a bin number is below 32 256 and fits the 16 bits.  The NW keys meet in red[], and the
// largest wins: the largest maximum at its lowest bin, whichever wave scanned it.  hit_bins is the sum over the waves of popcount(bits |
// mask).  The first strand's scan clears the counters.  The record is ibf_locate_kernel's; the filter is several column slices to the
// plain kernel and to the merge (reduce_locate_slices_kernel reads every slice's record), so the item's real record goes to slice 0 and
// an empty one to every other slice -- over what the plain launch, which ran before over a length of 0, left there.
template <int LINES, bool NT, int NW = 4>
__global__ __launch_bounds__(64 * NW) void ibf_locate_wide_lists_kernel(IbfDev f, const uint32_t *__restrict__ slots, const uint64_t *__restrict__ side,
                                                                        uint32_t side_rows, ReadSrc src, uint32_t n_items,
                                                                        const uint16_t *__restrict__ thr, uint32_t thr_len, uint32_t nf, uint32_t fi,
                                                                        const uint8_t *__restrict__ taken, LocatePart *__restrict__ part,
                                                                        uint32_t n_slices, uint32_t cnt_dwords)
{
    static_assert(LINES == 4 || LINES == 6 || LINES == 8, "slot sizes of rb_wide_lists.h");
    extern __shared__ uint32_t s_lds[];
    uint32_t *cnt = s_lds;  // cnt_dwords counters (a multiple of 256), kWideSpareDwords spares: ibf_count_wide_lists_kernel's areas
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    uint8_t *stage = reinterpret_cast<uint8_t *>(s_lds + cnt_dwords + rbwide::kWideSpareDwords) + wave * rbwide::kWideStageBytes;
    uint32_t *red = reinterpret_cast<uint32_t *>(reinterpret_cast<uint8_t *>(s_lds + cnt_dwords + rbwide::kWideSpareDwords) + NW * rbwide::kWideStageBytes);
    const uint32_t item = blockIdx.x;
    if (item >= n_items) return;
    if (!taken[item]) return;  // the whole workgroup, before any barrier: the plain kernel's item, or none's (not RB_OK)

    uint32_t len;
    const ListBaseSrc seq = make_list_base_src(src, item, &len);
    const uint32_t n = len >= f.k ? len - f.k + 1 : 0;
    const uint32_t tl = len < thr_len ? len : thr_len - 1;
    const uint32_t spare = cnt_dwords + lane;
    const uint32_t nh = f.n_hash < rbspec::kMaxHash ? f.n_hash : rbspec::kMaxHash;
    uint4 *c4 = reinterpret_cast<uint4 *>(cnt);
    for (uint32_t i = threadIdx.x; i < cnt_dwords / 4; i += 64 * NW) c4[i] = make_uint4(0, 0, 0, 0);
    __syncthreads();
    const WideShare<NW> share(cnt_dwords, wave);
    // t: the threshold the decision kernel reads for this length and filter (make_pass_wave's)
    const uint32_t t = __builtin_amdgcn_readfirstlane((uint32_t)thr[((size_t)tl * nf + fi) * 2]);
    uint64_t mask_lo = 0, mask_hi = 0;
    uint32_t best = 0, best_bin = 0, best_strand = 0, hit_bins = 0;
#pragma unroll 1
    for (int strand = 0; strand < 2; ++strand) {
        wide_count_strand<LINES, NT, NW>(f, cnt, stage, slots, side, side_rows, seq, len, n, strand, wave, lane, spare, nh);
        __syncthreads();
        uint32_t m = 0, bin = 0, hits = 0;
#pragma unroll 1
        for (uint32_t r = share.r0; r < share.r1; ++r) {  // wave-uniform
            const uint32_t i = r * 64u + lane, j = r - share.r0;
            const uint4 q = c4[i];
            const uint32_t mx = piece_max(q);
            if (mx > m) {
                m = mx;
                uint32_t at = 7;
#pragma unroll
                for (int u = 6; u >= 0; --u) at = piece_counter(q, u) == mx ? (uint32_t)u : at;
                bin = i * 8u + at;
            }
            const uint32_t bits = mx >= t ? piece_hits(q, i, t, f.n_bins) : 0u;  // (t == 0: every piece)
            if (strand == 0) {
                wide_mask_or(mask_lo, mask_hi, j, bits);
                c4[i] = make_uint4(0, 0, 0, 0);
            } else {
                hits += (uint32_t)__builtin_popcount(bits | wide_mask_get(mask_lo, mask_hi, j));
            }
        }
        const uint32_t wkey = wave_max_u32(m ? (m << 16) | (0xFFFFu - bin) : 0u);  // bin < kWideMaxBins, m <= kWideMaxKmers
        const uint32_t whits = wave_sum_u32(hits);
        if (lane == 0) {
            red[wave] = wkey;
            red[NW + wave] = whits;
        }
        __syncthreads();
        uint32_t key = 0, sum = 0;
#pragma unroll
        for (int w = 0; w < NW; ++w) {
            key = max(key, red[w]);
            sum += red[NW + w];
        }
        key = (uint32_t)__builtin_amdgcn_readfirstlane((int)key);
        hit_bins = (uint32_t)__builtin_amdgcn_readfirstlane((int)sum);  // (the second strand's stands)
        // rb_locate_out's rule, as ibf_locate_lists_kernel combines its strands: the larger maximum; on equal maxima the lower first bin,
        // and strand 0 keeps an equal bin
        const uint32_t sm = key >> 16, first = 0xFFFFu - (key & 0xFFFFu);
        if (sm > 0 && (sm > best || (sm == best && first < best_bin))) {
            best_bin = first;
            best_strand = (uint32_t)strand;
        }
        best = max(best, sm);
    }
    if (threadIdx.x < n_slices) {  // (the plain kernel cuts a block of at most 504 words into at most eight slices of a wave's columns)
        LocatePart rec;
        const bool real = threadIdx.x == 0;
        rec.max_count = real ? best : 0u;
        rec.first_bin = real ? best_bin : 0u;
        rec.strand = real ? best_strand : 0u;
        rec.hit_bins = real ? hit_bins : 0u;
        part[(size_t)threadIdx.x * n_items + item] = rec;
    }
}

// HITS.  Records leave in rising bin order, so a record's place is the number of hits in all lower bins, across the waves: ONE
// workgroup-wide exclusive prefix per strand.  Pass 1: every wave reads its share, keeps the pieces' hit bits (16 bytes per thread, as
// the mask) and sums its hits; the NW totals meet in red[]; a wave's records begin behind the totals of the waves below it.  Pass 2 is
// hits_scan's round over the kept bits: where a round holds a hit (one ballot) a prefix sum over the lanes places the lane's records, and
// they are stored while their place is below max_hits -- n_hits stays exact whatever the cap.  The first strand's pass 2 clears the
// pieces behind it, and a barrier closes it before the next strand's adds begin; bin_reads takes one add per bit of mask | own on the
// second strand.  No barrier stands inside a loop over a wave's rounds: every thread reaches the same three per strand.
// Segments and seg_count are ibf_hits_kernel's formats with the item's hits in slice 0; the plain kernel leaves a taken item (its length
// there is 0, below min_len) before it writes anything, so this kernel writes the zero seg_count of every other slice itself.
template <int LINES, bool NT, int NW = 4>
__global__ __launch_bounds__(64 * NW) void ibf_hits_wide_lists_kernel(IbfDev f, const uint32_t *__restrict__ slots, const uint64_t *__restrict__ side,
                                                                      uint32_t side_rows, ReadSrc src, uint32_t n_items,
                                                                      const uint16_t *__restrict__ thr, uint32_t thr_len, uint32_t nf, uint32_t fi,
                                                                      uint32_t min_count, uint32_t max_hits, const uint8_t *__restrict__ taken,
                                                                      rb_u32x2 *__restrict__ seg, uint32_t *__restrict__ seg_count,
                                                                      unsigned long long *__restrict__ bin_reads, uint32_t n_slices,
                                                                      uint32_t cnt_dwords)
{
    static_assert(LINES == 4 || LINES == 6 || LINES == 8, "slot sizes of rb_wide_lists.h");
    extern __shared__ uint32_t s_lds[];
    uint32_t *cnt = s_lds;  // cnt_dwords counters (a multiple of 256), kWideSpareDwords spares: ibf_count_wide_lists_kernel's areas
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    uint8_t *stage = reinterpret_cast<uint8_t *>(s_lds + cnt_dwords + rbwide::kWideSpareDwords) + wave * rbwide::kWideStageBytes;
    uint32_t *red = reinterpret_cast<uint32_t *>(reinterpret_cast<uint8_t *>(s_lds + cnt_dwords + rbwide::kWideSpareDwords) + NW * rbwide::kWideStageBytes);
    const uint32_t item = blockIdx.x;
    if (item >= n_items) return;
    if (!taken[item]) return;  // the whole workgroup, before any barrier: the plain kernel's item, or none's (not RB_OK)

    uint32_t len;
    const ListBaseSrc seq = make_list_base_src(src, item, &len);
    const uint32_t n = len >= f.k ? len - f.k + 1 : 0;
    const uint32_t tl = len < thr_len ? len : thr_len - 1;
    const uint32_t spare = cnt_dwords + lane;
    const uint32_t nh = f.n_hash < rbspec::kMaxHash ? f.n_hash : rbspec::kMaxHash;
    uint4 *c4 = reinterpret_cast<uint4 *>(cnt);
    for (uint32_t i = threadIdx.x; i < cnt_dwords / 4; i += 64 * NW) c4[i] = make_uint4(0, 0, 0, 0);
    __syncthreads();
    const WideShare<NW> share(cnt_dwords, wave);
    // t: the caller's threshold, or the one the decision kernel reads for this length and filter (make_pass_wave's)
    const uint32_t t = min_count ? min_count : __builtin_amdgcn_readfirstlane((uint32_t)thr[((size_t)tl * nf + fi) * 2]);
    uint64_t mask_lo = 0, mask_hi = 0;
#pragma unroll 1
    for (uint32_t strand = 0; strand < 2; ++strand) {
        wide_count_strand<LINES, NT, NW>(f, cnt, stage, slots, side, side_rows, seq, len, n, (int)strand, wave, lane, spare, nh);
        __syncthreads();
        // ---- pass 1: the share's hit bits, and the wave's total
        uint64_t own_lo = 0, own_hi = 0;
        uint32_t mine_all = 0;
#pragma unroll 1
        for (uint32_t r = share.r0; r < share.r1; ++r) {  // wave-uniform
            const uint32_t i = r * 64u + lane;
            const uint4 q = c4[i];
            const uint32_t bits = piece_max(q) >= t ? piece_hits(q, i, t, f.n_bins) : 0u;
            wide_mask_or(own_lo, own_hi, r - share.r0, bits);
            mine_all += (uint32_t)__builtin_popcount(bits);
        }
        const uint32_t wtotal = wave_sum_u32(mine_all);
        if (lane == 0) red[wave] = wtotal;
        __syncthreads();
        uint32_t total = 0, all = 0;  // wave-uniform: the hits of the waves below, of all waves
#pragma unroll
        for (int w = 0; w < NW; ++w) {
            const uint32_t v = red[w];
            total += (uint32_t)w < wave ? v : 0u;
            all += v;
        }
        total = (uint32_t)__builtin_amdgcn_readfirstlane((int)total);
        // ---- pass 2: the records, in bin order
        rb_u32x2 *out = seg + ((size_t)item * n_slices * 2 + strand) * max_hits;  // slice 0
#pragma unroll 1
        for (uint32_t r = share.r0; r < share.r1; ++r) {  // wave-uniform
            const uint32_t i = r * 64u + lane, j = r - share.r0;
            const uint32_t bits = wide_mask_get(own_lo, own_hi, j);
            if (strand == 1 && bin_reads) {  // uniform
                uint32_t seen = bits | wide_mask_get(mask_lo, mask_hi, j);
                while (seen) {
                    const uint32_t b = (uint32_t)__builtin_ctz(seen);
                    seen &= seen - 1;
                    atomicAdd(bin_reads + (i * 8u + b), 1ULL);  // a set bit is a bin below n_bins
                }
            }
            if (__ballot(bits != 0u) != 0ULL) {  // wave-uniform; the common round holds no hit
                const uint4 q = c4[i];
                const uint32_t mine = (uint32_t)__builtin_popcount(bits);
                uint32_t incl = mine;
#pragma unroll
                for (int d = 1; d < 64; d <<= 1) {
                    const uint32_t o = (uint32_t)__shfl_up((int)incl, d, 64);
                    if (lane >= (uint32_t)d) incl += o;
                }
                uint32_t pos = total + incl - mine;
#pragma unroll
                for (int b = 0; b < 8; ++b) {
                    if ((bits >> b) & 1u) {
                        if (pos < max_hits) {  // inside the segment
                            rb_u32x2 rec;
                            rec.x = i * 8u + (uint32_t)b;
                            rec.y = piece_counter(q, b) | (strand << 16);
                            out[pos] = rec;
                        }
                        ++pos;
                    }
                }
                total += (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
            }
            if (strand == 0) c4[i] = make_uint4(0, 0, 0, 0);
        }
        if (threadIdx.x < n_slices) seg_count[((size_t)threadIdx.x * 2 + strand) * n_items + item] = threadIdx.x == 0 ? all : 0u;
        mask_lo = own_lo;
        mask_hi = own_hi;
        __syncthreads();  // the pieces are read and cleared, and red[] is read, before another wave adds or writes there
    }
}

// ---- locate and hits from the wide list table
static bool wide_pass_launch_ok(const PlainPassLaunch &a)
{
    return a.thr && a.thr_len && a.wide_table && a.wide_side && a.list_taken && a.list_plain_lens && rbwide::lines_valid(a.wide_lines) &&
           wide_form_serves(a.f, a.src.max_len) && a.col_begin == 0 && a.col_end == a.f.bin_width && a.n_slices >= 1 &&
           a.n_slices <= 64 * rbwide::kWideWaves;
}

template <int LINES>
static hipError_t launch_locate_wide_nt(const LocateLaunch &a, hipStream_t st)
{
    constexpr int NW = (int)rbwide::kWideWaves;
    const uint32_t cnt_dwords = rbwide::cnt_dwords(a.f.n_bins);
    const size_t lds = rbwide::pass_lds_bytes(a.f.n_bins, NW);
    auto kern = a.wide_nt ? &ibf_locate_wide_lists_kernel<LINES, true, NW> : &ibf_locate_wide_lists_kernel<LINES, false, NW>;
    hipLaunchKernelGGL(kern, dim3(a.n_items), dim3(64 * NW), lds, st, a.f, a.wide_table, a.wide_side, a.wide_side_rows, a.src, a.n_items, a.thr,
                       a.thr_len, a.nf, a.fi, a.list_taken, a.part, a.n_slices, cnt_dwords);
    return hipGetLastError();
}

// The items the wide kernel leaves from the filter's own table -- the plain launch as it is, over the lengths of
// launch_wide_pass_lists_prep -- then the taken items from the wide list table, every slice's record of theirs written by the wide kernel.
hipError_t launch_ibf_locate_wide_lists(const LocateLaunch &a, hipStream_t st)
{
    if (a.n_items == 0) return hipSuccess;
    if (!a.part || !wide_pass_launch_ok(a)) return hipErrorInvalidValue;
    LocateLaunch plain = a;
    plain.src.lens = a.list_plain_lens;
    hipError_t e = launch_ibf_locate(plain, st);
    if (e != hipSuccess) return e;
    return a.wide_lines == 4 ? launch_locate_wide_nt<4>(a, st) : a.wide_lines == 6 ? launch_locate_wide_nt<6>(a, st) : launch_locate_wide_nt<8>(a, st);
}

template <int LINES>
static hipError_t launch_hits_wide_nt(const HitsLaunch &a, hipStream_t st)
{
    constexpr int NW = (int)rbwide::kWideWaves;
    const uint32_t cnt_dwords = rbwide::cnt_dwords(a.f.n_bins);
    const size_t lds = rbwide::pass_lds_bytes(a.f.n_bins, NW);
    auto kern = a.wide_nt ? &ibf_hits_wide_lists_kernel<LINES, true, NW> : &ibf_hits_wide_lists_kernel<LINES, false, NW>;
    hipLaunchKernelGGL(kern, dim3(a.n_items), dim3(64 * NW), lds, st, a.f, a.wide_table, a.wide_side, a.wide_side_rows, a.src, a.n_items, a.thr,
                       a.thr_len, a.nf, a.fi, a.min_count, a.max_hits, a.list_taken, (rb_u32x2 *)a.seg, a.seg_count,
                       (unsigned long long *)a.bin_reads, a.n_slices, cnt_dwords);
    return hipGetLastError();
}

// As locate's.  The plain kernel leaves an item whose length is below min_len before it writes anything, and a taken item's is 0 there:
// every segment, counter and profile entry is written once -- a taken item's by the wide kernel, in every slice.
hipError_t launch_ibf_hits_wide_lists(const HitsLaunch &a, hipStream_t st)
{
    if (a.n_items == 0) return hipSuccess;
    if (!a.seg_count || (a.max_hits && !a.seg) || a.min_len == 0 || !wide_pass_launch_ok(a)) return hipErrorInvalidValue;
    HitsLaunch plain = a;
    plain.src.lens = a.list_plain_lens;
    hipError_t e = launch_ibf_hits(plain, st);
    if (e != hipSuccess) return e;
    return a.wide_lines == 4 ? launch_hits_wide_nt<4>(a, st) : a.wide_lines == 6 ? launch_hits_wide_nt<6>(a, st) : launch_hits_wide_nt<8>(a, st);
}

}  // namespace rb

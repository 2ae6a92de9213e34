// rb_wide_prefix_lists.hip -- the WIDE LIST FORM of the prefix pass (rb_engine_set_wide_prefix_lists): the kernel that gives a work item's
// maximum at every prefix checkpoint from a filter's wide list table (rb_wide_lists.h, 8193 to 32 256 bins) with the workgroup of
// ibf_count_wide_lists_kernel, and the small kernel that says which work items it takes.  A translation unit of its own beside
// rb_wide_pass_lists.hip, whose device code it shares through rb_wide_lists_device.h (the ranged count, wide_count_range, is there beside
// wide_count_strand); the reading of a 16-byte piece of the counters is rb_pass_lists_device.h's.
#include <hip/hip_runtime.h>

#include "rb_device.h"
#include "rb_lists.h"
#include "rb_lists_device.h"
#include "rb_pass_lists_device.h"
#include "rb_wide_lists.h"
#include "rb_wide_lists_device.h"

namespace rb {

// Which items the wide form takes, decided once per call, one thread per item: prefix_lists_takes without its look at the bases (the wide
// kernel counts a k-mer with a base outside ACGT itself).  With w = min(len, c_last), the window the pass looks at: the item is RB_OK so
// far (chunk_prep's verdict) and w is within the call's bound (src.max_len, already min(the descriptor's, c_last): an understated bound
// leaves the item to the plain form and its status rules).  Any length: an item shorter than k, or empty, is taken and counts nothing.
// taken[] and plain_lens[] as prefix_lists_prep_kernel writes them; a wave then adds what it took and what it left to the engine's two
// counters of this form (rb_engine_wide_prefix_lists_items): one add per wave and counter.
__global__ __launch_bounds__(256) void wide_prefix_lists_prep_kernel(ReadSrc src, uint32_t n_items, const uint8_t *__restrict__ pre_status,
                                                                     uint32_t c_last, uint8_t *__restrict__ taken,
                                                                     uint32_t *__restrict__ plain_lens, unsigned long long *__restrict__ counters)
{
    const uint32_t item = blockIdx.x * 256u + threadIdx.x;
    const bool exists = item < n_items;
    bool takes = false;
    if (exists) {
        const uint32_t len = src.lens[item];
        takes = !(pre_status && pre_status[item] != RB_OK) && min(len, c_last) <= src.max_len;
        taken[item] = takes ? 1 : 0;
        plain_lens[item] = takes ? 0u : len;
    }
    const uint32_t n_taken = (uint32_t)__builtin_popcountll(__ballot(exists && takes));
    const uint32_t n_left = (uint32_t)__builtin_popcountll(__ballot(exists && !takes));
    if ((threadIdx.x & 63u) == 0) {
        if (n_taken) atomicAdd(counters + 0, (unsigned long long)n_taken);
        if (n_left) atomicAdd(counters + 1, (unsigned long long)n_left);
    }
}

hipError_t launch_wide_prefix_lists_prep(const PrefixListsPrep &a, hipStream_t st)
{
    if (a.n_items == 0) return hipSuccess;
    if (!a.taken || !a.plain_lens || !a.src.lens || !a.counters || a.c_last == 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(wide_prefix_lists_prep_kernel, dim3((a.n_items + 255) / 256), dim3(256), 0, st, a.src, a.n_items, a.pre_status, a.c_last,
                       a.taken, a.plain_lens, (unsigned long long *)a.counters);
    return hipGetLastError();
}

// ---- THE WIDE LIST FORM OF THE PREFIX PASS: ibf_locate_wide_lists_kernel's workgroup -- NW waves, one work item, one shared array of
// 16-bit counters, LDS the count kernel's to the byte (rbwide::count_lds_bytes) -- with the checkpoint loop of ibf_prefix_lists_kernel.
// ibf_prefix_kernel's argument holds here as there: the counters after the k-mers of a prefix ARE the counts of that prefix, on both
// strands.  Per strand the counters are cleared once; checkpoint p adds the k-mers [n_{p-1}, n_p) of the prefix of L_p = min(c_p, len)
// bases (wide_count_range: the range's tiles dealt round-robin to the waves), then every wave scans its WideShare of the counters for the
// maximum -- nothing is cleared, the next checkpoint adds on top -- and the NW maxima meet in red[].  A checkpoint that adds no k-mer
// repeats the maximum.  Lane p of EVERY wave keeps checkpoint p's maximum over the two strands (each wave reads all of red[]), so any wave
// can write it.  A strand's counters stay below 65 536: wide_form_serves admits calls of at most 65 535 k-mers at the last checkpoint.
// THE BARRIERS.  len and the checkpoint list are the workgroup's, so `n > n_prev` is uniform over the 256 threads and every barrier
// below is reached by all of them the same number of times; a checkpoint that adds nothing runs none.  One per strand, behind the clear:
// no wave adds into counters another wave has yet to zero (and the scans of the strand before lie behind that strand's last barrier).
// Two per checkpoint that adds:
//   (1) behind the adds, before the scan: a wave's share of the scan holds bins every wave has added to;
//   (2) behind the exchange -- the scans and the writes to red[] -- before red[] is read.  It also stands between every wave's scan and
//       the next range's adds (a wave still scanning would read counts of a later prefix), and, with the next checkpoint's (1), between
//       these reads of red[] and the next write to it.
// The filter is several column slices to the plain kernel and to finish_prefix_kernel, which takes the maximum over every slice's
// partials: the item's P maxima go to slice 0 and zeros to every other slice -- over what the plain launch, which ran before over a
// length of 0, left there.
template <int LINES, bool NT, int NW = 4>
__global__ __launch_bounds__(64 * NW) void ibf_prefix_wide_lists_kernel(IbfDev f, const uint32_t *__restrict__ slots, const uint64_t *__restrict__ side,
                                                                        uint32_t side_rows, ReadSrc src, uint32_t n_items, PrefixList cps,
                                                                        const uint8_t *__restrict__ taken, uint16_t *__restrict__ part,
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
    if (!taken[item]) return;  // the whole workgroup, before any barrier: the plain kernel's item

    uint32_t len_v;
    const ListBaseSrc seq = make_list_base_src(src, item, &len_v);
    const uint32_t len = __builtin_amdgcn_readfirstlane(len_v);  // the checkpoint loop below is scalar, and the same in every wave
    const uint32_t k = f.k;
    const uint32_t spare = cnt_dwords + lane;
    const uint32_t nh = f.n_hash < rbspec::kMaxHash ? f.n_hash : rbspec::kMaxHash;
    uint4 *c4 = reinterpret_cast<uint4 *>(cnt);
    const WideShare<NW> share(cnt_dwords, wave);
    uint32_t mine = 0;  // lane p: checkpoint p's maximum over the strands so far
#pragma unroll 1
    for (int strand = 0; strand < 2; ++strand) {
        for (uint32_t i = threadIdx.x; i < cnt_dwords / 4; i += 64 * NW) c4[i] = make_uint4(0, 0, 0, 0);
        __syncthreads();
        uint32_t n_prev = 0, m = 0;
#pragma unroll 1
        for (uint32_t p = 0; p < cps.n; ++p) {
            const uint32_t L = min(cps.c[p], len);
            const uint32_t n = L >= k ? L - k + 1 : 0;
            if (n > n_prev) {  // uniform over the workgroup
                wide_count_range<LINES, NT, NW>(f, cnt, stage, slots, side, side_rows, seq, L, n_prev, n, strand, wave, lane, spare, nh);
                __syncthreads();  // (1)
                uint32_t sm = 0;
#pragma unroll 1
                for (uint32_t r = share.r0; r < share.r1; ++r) sm = max(sm, piece_max(c4[r * 64u + lane]));  // wave-uniform trip count
                const uint32_t wm = wave_max_u32(sm);
                if (lane == 0) red[wave] = wm;
                __syncthreads();  // (2)
                uint32_t all = 0;
#pragma unroll
                for (int w = 0; w < NW; ++w) all = max(all, red[w]);
                m = (uint32_t)__builtin_amdgcn_readfirstlane((int)all);
                n_prev = n;
            }
            if (lane == p) mine = max(mine, m);
        }
    }
    // (the plain kernel cuts a block of at most 504 words into at most eight slices of a wave's columns)
    for (uint32_t s = wave; s < n_slices; s += NW)
        if (lane < cps.n) part[((size_t)s * n_items + item) * cps.n + lane] = s == 0 ? (uint16_t)mine : (uint16_t)0;
}

template <int LINES>
static hipError_t launch_prefix_wide_nt(const PrefixLaunch &a, hipStream_t st)
{
    constexpr int NW = (int)rbwide::kWideWaves;
    const uint32_t cnt_dwords = rbwide::cnt_dwords(a.f.n_bins);
    const size_t lds = rbwide::count_lds_bytes(a.f.n_bins, NW);
    auto kern = a.wide_nt ? &ibf_prefix_wide_lists_kernel<LINES, true, NW> : &ibf_prefix_wide_lists_kernel<LINES, false, NW>;
    hipLaunchKernelGGL(kern, dim3(a.n_items), dim3(64 * NW), lds, st, a.f, a.wide_table, a.wide_side, a.wide_side_rows, a.src, a.n_items, a.cps,
                       a.list_taken, a.part, a.n_slices, cnt_dwords);
    return hipGetLastError();
}

// Locate's arrangement: the plain launch as it is, over the lengths of launch_wide_prefix_lists_prep -- a taken item has no k-mer there
// -- then the taken items from the wide list table, every slice's partials of theirs written by the wide kernel.
hipError_t launch_ibf_prefix_wide_lists(const PrefixLaunch &a, hipStream_t st)
{
    if (a.n_items == 0) return hipSuccess;
    if (!a.part || a.cps.n == 0 || a.cps.n > kMaxPrefixes || !a.wide_table || !a.wide_side || !a.list_taken || !a.list_plain_lens ||
        !rbwide::lines_valid(a.wide_lines) || !wide_form_serves(a.f, a.src.max_len) || a.col_begin != 0 || a.col_end != a.f.bin_width ||
        a.n_slices < 1)
        return hipErrorInvalidValue;
    PrefixLaunch plain = a;
    plain.src.lens = a.list_plain_lens;
    hipError_t e = launch_ibf_prefix(plain, st);
    if (e != hipSuccess) return e;
    return a.wide_lines == 4 ? launch_prefix_wide_nt<4>(a, st) : a.wide_lines == 6 ? launch_prefix_wide_nt<6>(a, st) : launch_prefix_wide_nt<8>(a, st);
}

}  // namespace rb

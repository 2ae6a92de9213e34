// rb_prefix_lists.hip -- the LIST FORM of the prefix pass (rb_engine_set_prefix_lists): the kernel that gives a work item's maximum at
// every prefix checkpoint from a filter's list table (rb_lists.h) with the wave of ibf_count_lists_kernel, and the small kernel that says
// which work items it takes.  A translation unit of its own beside rb_pass_lists.hip, whose device code it shares through
// rb_pass_lists_device.h (the ranged count, list_count_range, is there beside list_count_strand).
#include <hip/hip_runtime.h>

#include "rb_device.h"
#include "rb_lists.h"
#include "rb_lists_device.h"
#include "rb_pass_lists_device.h"

namespace rb {

// Which items the list form takes.  The pass looks at w = min(len, c_last) bases of an item and no further, so that is the window the
// rule looks at: the item is RB_OK so far (chunk_prep's verdict), w is within the call's bound (src.max_len, already min(the
// descriptor's, c_last): an understated bound leaves the item to the plain form and its status rules), and the first w bases hold
// nothing outside ACGT -- an N behind the last checkpoint does not send a long read to the plain form.  Any length: an item shorter
// than k, or empty, is taken and counts nothing.  Called by a whole wave for one item; the answer is wave-uniform.
__device__ __forceinline__ bool prefix_lists_takes(const ReadSrc &r, uint32_t item, const uint8_t *pre_status, uint32_t c_last, uint32_t lane)
{
    const uint32_t w = min(r.lens[item], c_last);
    if ((pre_status && pre_status[item] != RB_OK) || w > r.max_len) return false;
    const uint32_t rid = r.ids ? r.ids[item] : item;
    bool outside = false;
    if (r.nmask) {  // packed input: a base is outside exactly when its bit of the N bitmap is set
        const uint8_t *nm = r.nmask + r.nmask_offsets[rid];
        for (uint32_t i = lane; i < w; i += 64) outside |= ((nm[(r.base_off + i) >> 3] >> ((r.base_off + i) & 7u)) & 1u) != 0;
    } else {
        const uint8_t *s = r.seqs + r.offsets[rid] + r.base_off;
        for (uint32_t i = lane; i < w; i += 64) outside |= rbspec::dna5_ord(s[i]) > 3u;
    }
    return __ballot(outside) == 0ULL;
}

// ... decided once per call, as launch_pass_lists_prep does for locate and hits: taken[] for the list kernel, plain_lens[] -- 0 for a
// taken item -- for the plain kernel.  A wave walks kPrepItemsPerWave items and then adds what it took and what it left to the engine's two
// counters (rb_engine_prefix_lists_items): one add per wave and counter.
constexpr uint32_t kPrepItemsPerWave = 8;
__global__ __launch_bounds__(256) void prefix_lists_prep_kernel(ReadSrc src, uint32_t n_items, const uint8_t *__restrict__ pre_status, uint32_t c_last,
                                                                uint8_t *__restrict__ taken, uint32_t *__restrict__ plain_lens,
                                                                unsigned long long *__restrict__ counters)
{
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t first = (blockIdx.x * 4u + (threadIdx.x >> 6)) * kPrepItemsPerWave;
    uint32_t n_taken = 0, n_left = 0;  // wave-uniform
    for (uint32_t item = first; item < first + kPrepItemsPerWave && item < n_items; ++item) {
        const bool takes = prefix_lists_takes(src, item, pre_status, c_last, lane);
        if (lane == 0) {
            taken[item] = takes ? 1 : 0;
            plain_lens[item] = takes ? 0u : src.lens[item];
        }
        n_taken += takes ? 1u : 0u;
        n_left += takes ? 0u : 1u;
    }
    if (lane == 0 && n_taken) atomicAdd(counters + 0, (unsigned long long)n_taken);
    if (lane == 0 && n_left) atomicAdd(counters + 1, (unsigned long long)n_left);
}

hipError_t launch_prefix_lists_prep(const PrefixListsPrep &a, hipStream_t st)
{
    if (a.n_items == 0) return hipSuccess;
    if (!a.taken || !a.plain_lens || !a.src.lens || !a.counters || a.c_last == 0) return hipErrorInvalidValue;
    const uint32_t per_block = 4u * kPrepItemsPerWave;
    hipLaunchKernelGGL(prefix_lists_prep_kernel, dim3((a.n_items + per_block - 1) / per_block), dim3(256), 0, st, a.src, a.n_items, a.pre_status,
                       a.c_last, a.taken, a.plain_lens, (unsigned long long *)a.counters);
    return hipGetLastError();
}

// ---- THE LIST FORM OF THE PREFIX PASS: ibf_locate_lists_kernel's wave -- one workgroup of 64 lanes, one work item, the slot gathers of
// list_batch -- with the count kernel's LDS (rblist::count_lds_bytes: counters, spares, stage; no hit mask).  ibf_prefix_kernel's
// argument holds here as there: the counters after the k-mers of a prefix ARE the counts of that prefix, on both strands.  Per strand the
// counters are cleared once; checkpoint p adds the k-mers [n_{p-1}, n_p) of the prefix of L_p = min(c_p, len) bases (list_count_range) and
// then scans the counters for their maximum (list_scan<false>: nothing is cleared, the next checkpoint adds on top).  A checkpoint that
// adds no k-mer repeats the maximum.  Lane p keeps checkpoint p's maximum over the two strands; lanes below P write part[item][0 .. P),
// slice 0 of one.  A strand's counters stay below 65 536: the list form serves calls of fewer than 65 536 k-mers at the last checkpoint.
template <int LINES, bool NT>
__global__ __launch_bounds__(64) void ibf_prefix_lists_kernel(IbfDev f, const uint32_t *__restrict__ slots, const uint64_t *__restrict__ side,
                                                              uint32_t side_rows, ReadSrc src, uint32_t n_items, PrefixList cps,
                                                              const uint8_t *__restrict__ taken, uint16_t *__restrict__ part, uint32_t cnt_dwords)
{
    static_assert(LINES == 1 || LINES == 2 || LINES == 4, "slot sizes of rb_lists.h");
    extern __shared__ uint32_t s_lds[];
    uint32_t *cnt = s_lds;
    uint8_t *stage = reinterpret_cast<uint8_t *>(s_lds + cnt_dwords + kListSpareDwords);
    const uint32_t lane = threadIdx.x;
    const uint32_t item = blockIdx.x;
    if (item >= n_items) return;
    if (!taken[item]) return;  // wave-uniform: the plain kernel's item

    uint32_t len_v;
    const ListBaseSrc seq = make_list_base_src(src, item, &len_v);
    const uint32_t len = __builtin_amdgcn_readfirstlane(len_v);  // the checkpoint loop below is scalar
    const uint32_t k = f.k;
    const uint32_t spare = cnt_dwords + lane;
    uint32_t mine = 0;  // lane p: checkpoint p's maximum over the strands so far
#pragma unroll 1
    for (int strand = 0; strand < 2; ++strand) {
        {
            __builtin_amdgcn_wave_barrier();
            uint4 *c4 = reinterpret_cast<uint4 *>(cnt);
            for (uint32_t i = lane; i < cnt_dwords / 4; i += 64) c4[i] = make_uint4(0, 0, 0, 0);
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
            __builtin_amdgcn_wave_barrier();
        }
        uint32_t n_prev = 0, m = 0;
#pragma unroll 1
        for (uint32_t p = 0; p < cps.n; ++p) {
            const uint32_t L = min(cps.c[p], len);
            const uint32_t n = L >= k ? L - k + 1 : 0;
            if (n > n_prev) {  // wave-uniform
                list_count_range<LINES, NT>(f, cnt, stage, slots, side, side_rows, seq, L, n_prev, n, strand, lane, spare);
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
                m = list_scan<false>(cnt, cnt_dwords, lane);
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
                n_prev = n;
            }
            if (lane == p) mine = max(mine, m);
        }
    }
    if (lane < cps.n) part[(size_t)item * cps.n + lane] = (uint16_t)mine;  // slice 0 of one
}

template <int LINES>
static hipError_t launch_prefix_lists_nt(const PrefixLaunch &a, hipStream_t st)
{
    const uint32_t cnt_dwords = rblist::count_cnt_dwords(a.f.n_bins);
    const size_t lds = rblist::count_lds_bytes(a.f.n_bins);
    const uint32_t *slots = reinterpret_cast<const uint32_t *>(a.list_table);
    auto kern = a.list_nt ? &ibf_prefix_lists_kernel<LINES, true> : &ibf_prefix_lists_kernel<LINES, false>;
    hipLaunchKernelGGL(kern, dim3(a.n_items), dim3(64), lds, st, a.f, slots, a.list_side, a.list_side_rows, a.src, a.n_items, a.cps, a.list_taken,
                       a.part, cnt_dwords);
    return hipGetLastError();
}

// Locate's arrangement: the plain launch as it is, over the lengths of launch_prefix_lists_prep -- a taken item has no k-mer there and
// gets P zero partials -- then the taken items from the list table, whose partials stand.
hipError_t launch_ibf_prefix_lists(const PrefixLaunch &a, hipStream_t st)
{
    if (a.n_items == 0) return hipSuccess;
    if (!a.part || a.cps.n == 0 || a.cps.n > kMaxPrefixes || !a.list_table || !a.list_side || !a.list_taken || !a.list_plain_lens ||
        !rblist::lines_valid(a.list_lines) || !pass_list_form_serves(a))
        return hipErrorInvalidValue;
    PrefixLaunch plain = a;
    plain.src.lens = a.list_plain_lens;
    hipError_t e = launch_ibf_prefix(plain, st);
    if (e != hipSuccess) return e;
    return a.list_lines == 1 ? launch_prefix_lists_nt<1>(a, st) : a.list_lines == 2 ? launch_prefix_lists_nt<2>(a, st) : launch_prefix_lists_nt<4>(a, st);
}

}  // namespace rb

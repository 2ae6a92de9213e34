// rb_resume_lists.hip -- the LIST FORM of the resume pass (rb_resume_set_lists): the kernel that counts a work item's new k-mers from a
// filter's list table (rb_lists.h) with the wave of ibf_count_lists_kernel and merges them into the slot's bit-sliced planes in HBM, and
// the small kernel that says which work items it takes.  A translation unit of its own beside rb_pass_lists.hip, whose device code it
// shares through rb_pass_lists_device.h; the merge's arithmetic is rb_resume_planes.h, which the CPU tests compile alone.
#include <hip/hip_runtime.h>

#include "rb_device.h"
#include "rb_lists.h"
#include "rb_lists_device.h"
#include "rb_pass_lists_device.h"
#include "rb_resume_planes.h"

namespace rb {

// ---- THE LIST FORM OF THE RESUME PASS (rb_resume_set_lists): the counting half is list_count_strand as it is, over the stitched item
// "tail + chunk", into LDS counters that start at zero and so hold THIS CALL'S DELTA only -- at most 65 535 per bin (the list form's
// bound on a call's k-mers), so the carry contract of the list kernels holds: a low half never carries into the odd bin above it.  The
// slot's totals never come to LDS (65 000 + 1 000 would carry into the neighbour).  The other half is the MERGE that ends a strand.

// Which items the list form takes, one wave per item after resume_prep_kernel: not refused (kResumeSkip) and no base outside ACGT in the
// stitched string -- pass_lists_takes on the stitched source, any length, zero and below k included; a tail that carries an N from an
// earlier chunk sends the item to the plain form.  plain_ctl is ctl with kResumeSkip ORed in for a taken item: ibf_resume_kernel,
// launched with it, writes a zero partial for the item and forms no address of its slot.
__global__ __launch_bounds__(256) void resume_lists_prep_kernel(ReadSrc src, uint32_t n_items, const uint8_t *__restrict__ pre_status,
                                                                const uint8_t *__restrict__ ctl, uint8_t *__restrict__ taken,
                                                                uint8_t *__restrict__ plain_ctl)
{
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t item = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (item >= n_items) return;  // wave-uniform
    const uint32_t c = ctl[item];
    const bool takes = !(c & kResumeSkip) && pass_lists_takes(src, item, pre_status, 0u, lane);
    if (lane == 0) {
        taken[item] = takes ? 1 : 0;
        plain_ctl[item] = (uint8_t)(takes ? c | kResumeSkip : c);
    }
}

hipError_t launch_resume_lists_prep(const ReadSrc &src, uint32_t n_items, const uint8_t *pre_status, const uint8_t *ctl, uint8_t *taken,
                                    uint8_t *plain_ctl, hipStream_t st)
{
    if (n_items == 0) return hipSuccess;
    if (!src.lens || !pre_status || !ctl || !taken || !plain_ctl) return hipErrorInvalidValue;
    hipLaunchKernelGGL(resume_lists_prep_kernel, dim3((n_items + 3) / 4), dim3(256), 0, st, src, n_items, pre_status, ctl, taken, plain_ctl);
    return hipGetLastError();
}

// THE MERGE of a strand: lane l takes the columns l, l + 64, ... below n_cols = ceil(n_bins / 64).  A column is 128 bytes of counters,
// eight 16-byte pieces, and the lanes stand 128 bytes apart: read in piece order, the sixteen lanes of a ds_read_b128 group would meet
// in two 16-byte places of the 256-byte bank row, eight deep.  So lane l reads (and clears) piece (q + r) & 7 in step q, r = (l >> 1) & 7:
// the eight even and the eight odd lanes of every group then stand on sixteen different places -- no conflict on the reads, two deep
// on the clearing stores' eight-lane groups.  The registers hold the column rotated by r pieces, which after the transpose is a rotation
// of every delta plane by 8 r bits (rbplanes::rotate_bins).  Columns at or beyond n_cols, and the bits behind n_bins, are neither read
// nor written: nothing adds to them.  -> the strand's maximum (wave-uniform)
template <bool LOADS, bool STORES>
__device__ __forceinline__ uint32_t resume_merge(uint32_t *cnt, uint64_t *__restrict__ planes, uint32_t pad_cols, uint32_t n_bins, uint32_t lane)
{
    uint4 *c4 = reinterpret_cast<uint4 *>(cnt);
    const uint32_t n_cols = (n_bins + 63u) >> 6;
    const uint32_t r = (lane >> 1) & 7u;
    uint32_t best = 0;
#pragma unroll 1
    for (uint32_t col = lane; col < n_cols; col += 64) {
        uint64_t st[rbplanes::kPlanes];
        if (LOADS) {
#pragma unroll
            for (int i = 0; i < rbplanes::kPlanes; ++i) st[i] = __builtin_nontemporal_load(planes + (size_t)i * pad_cols + col);
        }
        uint32_t c[rbplanes::kColumnDwords];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const uint32_t piece = col * 8u + (((uint32_t)q + r) & 7u);
            const uint4 v = c4[piece];
            c4[piece] = make_uint4(0, 0, 0, 0);
            c[q * 4 + 0] = v.x;
            c[q * 4 + 1] = v.y;
            c[q * 4 + 2] = v.z;
            c[q * 4 + 3] = v.w;
        }
        uint64_t delta[rbplanes::kPlanes];
        rbplanes::counters_to_planes(c, delta);
#pragma unroll
        for (int i = 0; i < rbplanes::kPlanes; ++i) delta[i] = rbplanes::rotate_bins(delta[i], r);
        if (LOADS) {
            rbplanes::ripple_add(st, delta);
        } else {
#pragma unroll
            for (int i = 0; i < rbplanes::kPlanes; ++i) st[i] = delta[i];
        }
        // (the plain form masks its maximum to the bins that exist, and so does this one: see DESIGN 4.11 on what may stand behind n_bins)
        const uint32_t left = n_bins - col * 64u;
        const uint64_t valid = left >= 64u ? ~0ULL : (1ULL << left) - 1ULL;
        best = max(best, rbplanes::planes_column_max(st, valid));
        if (STORES) {
#pragma unroll
            for (int i = 0; i < rbplanes::kPlanes; ++i) __builtin_nontemporal_store(st[i], planes + (size_t)i * pad_cols + col);
        }
    }
    return (uint32_t)__builtin_amdgcn_readfirstlane(wave_max_u32(best));
}

// One workgroup of 64 lanes per item, the count kernel's LDS (rblist::count_lds_bytes: counters, spares, stage; no hit mask).  It takes
// the items of taken[] and overwrites their partial maximum part[0 * n_items + item], which the plain launch before it left at zero.
// A FIRST item loads nothing and stores the delta itself -- also when it adds no k-mer: FIRST resets the slot.  A PEEK item stores
// nothing.  An item that adds no k-mer and is not FIRST loads (its row is the slot's maximum) and stores nothing.
template <int LINES, bool NT>
__global__ __launch_bounds__(64) void ibf_resume_lists_kernel(IbfDev f, const uint32_t *__restrict__ slots, const uint64_t *__restrict__ side,
                                                              uint32_t side_rows, ReadSrc src, uint32_t n_items, const uint8_t *__restrict__ taken,
                                                              ResumeSlots rs, uint16_t *__restrict__ part, uint32_t cnt_dwords)
{
    static_assert(LINES == 1 || LINES == 2 || LINES == 4, "slot sizes of rb_lists.h");
    extern __shared__ uint32_t s_lds[];
    uint32_t *cnt = s_lds;
    uint8_t *stage = reinterpret_cast<uint8_t *>(s_lds + cnt_dwords + kListSpareDwords);
    const uint32_t lane = threadIdx.x;
    const uint32_t item = blockIdx.x;
    if (item >= n_items) return;
    if (!taken[item]) return;  // wave-uniform: the plain kernel's item, or none's (refused)

    const uint32_t ctl = __builtin_amdgcn_readfirstlane((uint32_t)rs.ctl[item]);  // (no kResumeSkip: the item is taken, its slot vetted)
    const uint32_t slot = __builtin_amdgcn_readfirstlane(rs.slot[item]);
    uint32_t len;
    const ListBaseSrc seq = make_list_base_src(src, item, &len);
    const uint32_t n = len >= f.k ? len - f.k + 1 : 0;
    const uint32_t spare = cnt_dwords + lane;
    {  // the first strand's counters; the second strand's are cleared by the merge that ends the first
        __builtin_amdgcn_wave_barrier();
        uint4 *c4 = reinterpret_cast<uint4 *>(cnt);
        for (uint32_t i = lane; i < cnt_dwords / 4; i += 64) c4[i] = make_uint4(0, 0, 0, 0);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
        __builtin_amdgcn_wave_barrier();
    }
    const bool first = (ctl & kResumeFirst) != 0;
    const bool stores = !(ctl & kResumePeek) && (first || n != 0);
    uint32_t best = 0;
#pragma unroll 1
    for (uint32_t strand = 0; strand < 2; ++strand) {
        list_count_strand<LINES, NT>(f, cnt, stage, slots, side, side_rows, seq, len, n, (int)strand, lane, spare);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
        uint64_t *planes = rs.state + (uint64_t)slot * rs.slot_words + rs.filter_off + (uint64_t)(strand * kResumePlanes) * rs.pad_cols;
        uint32_t m;
        if (first)  // wave-uniform, as `stores`
            m = stores ? resume_merge<false, true>(cnt, planes, rs.pad_cols, f.n_bins, lane) : resume_merge<false, false>(cnt, planes, rs.pad_cols, f.n_bins, lane);
        else
            m = stores ? resume_merge<true, true>(cnt, planes, rs.pad_cols, f.n_bins, lane) : resume_merge<true, false>(cnt, planes, rs.pad_cols, f.n_bins, lane);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
        best = max(best, m);
    }
    if (lane == 0) part[item] = (uint16_t)best;  // slice 0 of one
}

template <int LINES>
static hipError_t launch_resume_lists_nt(const ResumeLaunch &a, hipStream_t st)
{
    const uint32_t cnt_dwords = rblist::count_cnt_dwords(a.f.n_bins);
    const size_t lds = rblist::count_lds_bytes(a.f.n_bins);
    const uint32_t *slots = reinterpret_cast<const uint32_t *>(a.list_table);
    auto kern = a.list_nt ? &ibf_resume_lists_kernel<LINES, true> : &ibf_resume_lists_kernel<LINES, false>;
    hipLaunchKernelGGL(kern, dim3(a.n_items), dim3(64), lds, st, a.f, slots, a.list_side, a.list_side_rows, a.src, a.n_items, a.list_taken, a.slots,
                       a.part, cnt_dwords);
    return hipGetLastError();
}

// The plain launch as it is, over plain_ctl -- the items the list kernel leaves, and a zero partial with no slot traffic for a taken one
// -- then the taken items from the list table on the same stream, whose partials stand.
hipError_t launch_ibf_resume_lists(const ResumeLaunch &a, hipStream_t st)
{
    if (a.n_items == 0) return hipSuccess;
    if (!a.part || !a.slots.state || !a.slots.slot || !a.slots.ctl || !a.list_plain_ctl || !a.list_taken || !a.list_table || !a.list_side ||
        !rblist::lines_valid(a.list_lines) || !pass_list_form_serves(a))
        return hipErrorInvalidValue;
    // one column slice: the slot's planes of this filter are pad_cols >= ceil(n_bins / 64) columns, inside the slot
    if (a.slots.pad_cols < (a.f.n_bins + 63u) / 64u || a.slots.filter_off + 2ull * kResumePlanes * a.slots.pad_cols > a.slots.slot_words)
        return hipErrorInvalidValue;
    ResumeLaunch plain = a;
    plain.slots.ctl = a.list_plain_ctl;
    hipError_t e = launch_ibf_resume(plain, st);
    if (e != hipSuccess) return e;
    return a.list_lines == 1 ? launch_resume_lists_nt<1>(a, st) : a.list_lines == 2 ? launch_resume_lists_nt<2>(a, st) : launch_resume_lists_nt<4>(a, st);
}

}  // namespace rb

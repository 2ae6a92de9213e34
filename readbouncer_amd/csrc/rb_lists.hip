// rb_lists.hip -- the LIST FORM of the plain count kernel: a filter's list table (rb_lists.h: per N-free k-mer the bin numbers of its
// row, the AND of its h blocks, in one slot of 1, 2 or 4 lines) and the kernel that counts from it.  A translation unit of its own: what
// it needs of rb_kernels.hip -- how a read's bases are found and turned into Dna5 ordinals -- is a few lines of rb_lists_device.h, written
// again there with the adds, the scan and the slot gathers that rb_pass_lists.hip shares.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "rb_device.h"
#include "rb_lists.h"
#include "rb_lists_device.h"

namespace rb {

// One wave, one workgroup, one read; N-free reads only (a wave whose read has a base outside ACGT leaves at once: the three-hash twin
// ibf_count_rows_kernel<.., false>, launched behind this kernel, writes those).  Per strand the wave keeps a 16-bit counter for every bin
// in LDS, two per dword, cleared first; per tile of 64 k-mers every lane ranks its own k-mer (base 4, first base most significant; the
// reverse strand: the rank of the reverse complement), the tile's slots are gathered back to back -- lane l takes dword l of a two-line
// slot, dwords 2l and 2l + 1 of a four-line slot (two halves of 32 slots then), dword l & 31 of a one-line slot, where lanes 32-63 count
// nothing -- and every half of a dword is one add to the LDS address it holds, with no value back (the table is in the RESIDENT form of
// rb_lists.h: the address arithmetic was done when the table was built): adds commute, so a group of eight slots is counted as soon as
// its loads have landed, and the strand's maximum is one scan of the counters at its end (list_scan).
// An overflow slot (rb_lists.h) names a dense row of the side table, and a row with too many bins of one parity has swapped halves; both
// carry a flag.  Every lane ORs the dwords it holds of a group's eight slots and one wave-wide test of the flag bits says whether any is
// set; only such a group looks at its slots one by one, sets the overflow slots aside and blanks them -- their index is no address --
// adds the swapped halves with the other constant, and the dense rows' set bits are counted one by one after the tile's lists.
// Pruning (flags & kPruneBound): the second strand is skipped when the first reached n, and it stops at the tile boundary where its
// maximum so far plus the k-mers still to come cannot pass the first strand's maximum, `best`.  That cannot happen while more than
// `best` k-mers are to come, so only the tile edges behind that point scan the counters.  Exact: the output is the maximum over both.

template <int LINES, bool NT>
__global__ __launch_bounds__(64) void ibf_count_lists_kernel(IbfDev f, const uint32_t *__restrict__ slots, const uint64_t *__restrict__ side,
                                                             uint32_t side_rows, ReadSrc src, uint32_t n_reads, uint16_t *__restrict__ out,
                                                             uint32_t out_read_stride, uint32_t flags, uint64_t *__restrict__ trace,
                                                             uint32_t cnt_dwords)
{
    static_assert(LINES == 1 || LINES == 2 || LINES == 4, "slot sizes of rb_lists.h");
    constexpr uint32_t R = LINES == 4 ? 32 : 64;  // slots per batch (list_batch)
    extern __shared__ uint32_t s_lds[];
    uint32_t *cnt = s_lds;                                                                   // cnt_dwords counters (a multiple of 256), kListSpareDwords spares
    uint8_t *stage = reinterpret_cast<uint8_t *>(s_lds + cnt_dwords + kListSpareDwords);    // rblist::kCountStageBytes
    const uint32_t lane = threadIdx.x;
    const uint32_t read = blockIdx.x;
    if (read >= n_reads) return;

    uint32_t len;
    const ListBaseSrc seq = make_list_base_src(src, read, &len);
    const uint32_t k = f.k;
    const uint32_t n = len >= k ? len - k + 1 : 0;
    bool outside = false;
    for (uint32_t i = lane; i < len; i += 64) outside |= seq.ord(i) > 3u;
    if (__ballot(outside) != 0ULL) return;  // wave-uniform: the twin's read

    const bool bound = (flags & kPruneBound) != 0;
    const uint32_t spare = cnt_dwords + lane;
    uint32_t best = 0, stops = 0;
    {  // the first strand's counters; the second strand's are cleared by the scan that ends the first
        __builtin_amdgcn_wave_barrier();
        uint4 *c4 = reinterpret_cast<uint4 *>(cnt);
        for (uint32_t i = lane; i < cnt_dwords / 4; i += 64) c4[i] = make_uint4(0, 0, 0, 0);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
        __builtin_amdgcn_wave_barrier();
    }
#pragma unroll 1
    for (int strand = 0; strand < 2; ++strand) {
        if (bound && strand == 1 && best >= n) break;  // wave-uniform
        uint32_t stopped = n, m = 0;
        // A tile's bases (64 + k - 1 <= 76 at k <= kRowTableMaxK: two per lane) are loaded one tile ahead, before the gathers of the tile
        // in hand are issued, so their way from memory is not on the way to the next tile's ranks.  Not across an edge where the
        // strand may stop: that tile loads its own.
        uint32_t ahead0 = 0, ahead1 = 0;
        bool ahead = false;
#pragma unroll 1
        for (uint32_t mt = 0; mt < n; mt += 64) {
            // a bin counts at most once per k-mer: nothing to come can pass `best` once so_far + (n - mt) <= best, and so_far >= 0
            if (bound && strand == 1 && n - mt <= best) {
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
                m = list_scan<false>(cnt, cnt_dwords, lane);
                if (m + (n - mt) <= best) {
                    stopped = mt;
                    break;
                }
            }
            // ---- the tile's bases as Dna5 ordinals, and one rank per lane
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
            ahead = mt + 64u < n && !(bound && strand == 1 && n - (mt + 64u) <= best);
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
        if (stopped == n) {  // (a strand that stopped has just scanned)
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
            m = strand == 0 ? list_scan<true>(cnt, cnt_dwords, lane) : list_scan<false>(cnt, cnt_dwords, lane);
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
        }
        best = max(best, m);
        stops = strand == 0 ? (stopped & 0xFFFFu) : (stops | (stopped << 16));
    }
    if (lane == 0) out[(size_t)read * out_read_stride] = (uint16_t)best;
    if (trace) {
        if (lane == 0) trace[read] = prune_trace_record(0u, false, 0u, stops & 0xFFFFu, stops >> 16, 0u);
    }
}

// The list table of a filter in the RESIDENT form (rb_lists.h), one wave per slot (the waves stride over the slots, as
// ibf_row_table_kernel's over its rows): the AND of the k-mer's h blocks, word `lane` and word `lane + 64` of it per lane (a block of at
// most 128 words); one wave prefix sum of the lanes' even and odd populations, packed into one word; and every lane writes the counter
// offsets of its set bits -- even bins into the low halves from dword 0 up, odd bins into the high halves, what one parity's halves
// cannot take into the other's free halves with the swapped flag -- into the slot's image in LDS, which starts as the dwords' spares and
// leaves as whole dwords.  Pad words and the bits behind n_bins list nothing.  A row with more set bits than the slot holds takes the next
// row of the side table (an atomic counter; the order may vary from build to build, the rows may not) and leaves an overflow slot; past
// `side_cap` it writes no row, and the host, which reads the counter, refuses the table.
// lines == 0 is the CENSUS: nothing is written but counters[1 + i] += 1 for a row with more than 64 << i set bits (i = 0, 1, 2); `step`
// is the distance between the rows it looks at.
__global__ __launch_bounds__(256) void ibf_list_table_kernel(IbfDev f, uint32_t *__restrict__ slots, uint64_t *__restrict__ side,
                                                             uint32_t *__restrict__ counters, uint64_t n_rows, uint64_t step, uint32_t lines,
                                                             uint32_t side_cap)
{
    __shared__ uint16_t s_slot[4][rblist::kMaxLines * rblist::kEntriesPerLine];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    const uint64_t S = f.stride;
    const uint32_t W = f.bin_width;
    const uint32_t nh = f.n_hash < rbspec::kMaxHash ? f.n_hash : rbspec::kMaxHash;
    const uint32_t rem = f.n_bins & 63u;
    const uint32_t cnt_dwords = rblist::count_cnt_dwords(f.n_bins);
    constexpr uint64_t kEven = 0x5555555555555555ULL;  // bin 64 w + b is even where b is
    uint16_t *img = s_slot[wave];
    for (uint64_t r = (((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6) * step; r < n_rows; r += waves * step) {  // wave-uniform
        uint64_t v = 0;
        for (uint32_t i = 0; i < f.k; ++i) v = v * 5u + ((r >> (2u * (f.k - 1u - i))) & 3u);
        uint64_t word[2];
        uint32_t mine = 0;  // the lane's even bins, and its odd bins << 16 (at most 64 each)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const uint32_t w = lane + 64u * j;
            uint64_t acc = 0;
            if (w < W) {
                acc = ~0ULL;
                for (uint32_t h = 0; h < nh; ++h) {
                    const uint32_t b = rbspec::block_index(v, f.precalc[h], f.n_blocks, f.magic, f.pow2_mask);
                    acc &= f.words[(uint64_t)b * S + w];
                }
                if (w == W - 1 && rem) acc &= (1ULL << rem) - 1;
            }
            word[j] = acc;
            mine += (uint32_t)__popcll(acc & kEven) + ((uint32_t)__popcll(acc & ~kEven) << 16);
        }
        uint32_t incl = mine;  // at most 4096 in either half
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t o = (uint32_t)__shfl_up((int)incl, d, 64);
            if (lane >= (uint32_t)d) incl += o;
        }
        const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
        const uint32_t n_par[2] = {total & 0xFFFFu, total >> 16};
        const uint32_t set = n_par[0] + n_par[1];
        if (lines == 0) {
            if (lane == 0)
                for (uint32_t i = 0; i < 3; ++i)
                    if (set > (64u << i)) atomicAdd(&counters[1 + i], 1u);
            continue;
        }
        const uint32_t cap = lines * rblist::kEntriesPerLine, half = cap / 2;
        __builtin_amdgcn_wave_barrier();
        {  // dwords 2 lane and 2 lane + 1 of the image, all kMaxLines lines: their spares in both halves
            const uint32_t d = 2u * lane;
            const uint32_t s0 = cnt_dwords + (lines == 4 ? d >> 1 : d), s1 = cnt_dwords + (lines == 4 ? d >> 1 : d + 1u);
            reinterpret_cast<uint2 *>(img)[lane] = make_uint2((s0 * 4u) * 0x10001u, (s1 * 4u) * 0x10001u);
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
        __builtin_amdgcn_wave_barrier();
        if (set <= cap) {
            uint32_t rank[2] = {(incl - mine) & 0xFFFFu, (incl - mine) >> 16};
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                uint64_t bits = word[j];
                while (bits) {
                    const uint32_t bit = (uint32_t)__builtin_ctzll(bits);
                    bits &= bits - 1;
                    const uint32_t par = bit & 1u;
                    const uint32_t off = ((lane + 64u * j) * 32u + (bit >> 1)) * 4u;  // counter dword bin >> 1
                    const uint32_t at = par ? rank[1]++ : rank[0]++;
                    // at < n_par[par]; past `half`, n_par[par ^ 1] + (at - half) < set - half <= half: every index below is < cap
                    if (at < half) img[2u * at + par] = (uint16_t)off;
                    else img[2u * (n_par[par ^ 1u] + (at - half)) + (par ^ 1u)] = (uint16_t)(off | rblist::kResidentSwapped);
                }
            }
        } else {
            uint32_t idx = 0;
            if (lane == 0) idx = atomicAdd(&counters[0], 1u);
            idx = (uint32_t)__builtin_amdgcn_readfirstlane((int)idx);
            if (lane == 0) {
                img[0] |= (uint16_t)rblist::kResidentOverflow;
                img[2] = (uint16_t)(idx & 0xFFFFu);
                img[3] = (uint16_t)(idx >> 16);
            }
            if (idx < side_cap) {
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const uint32_t w = lane + 64u * j;
                    if (w < S) side[(uint64_t)idx * S + w] = word[j];
                }
                for (uint32_t w = lane + 128u; w < S; w += 64) side[(uint64_t)idx * S + w] = 0;
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
        __builtin_amdgcn_wave_barrier();
        const uint32_t slot_dwords = lines * 32u;
        for (uint32_t d = lane; d < slot_dwords; d += 64) slots[r * slot_dwords + d] = reinterpret_cast<const uint32_t *>(img)[d];
    }
}

static hipError_t list_builder_args_ok(const IbfDev &f, uint64_t n_rows)
{
    if (n_rows == 0 || n_rows > (1ull << (2 * kRowTableMaxK)) || f.k == 0 || f.k > kRowTableMaxK) return hipErrorInvalidValue;
    if (f.bin_width == 0 || f.bin_width > 128 || f.n_bins > rblist::kMaxBins || f.stride < f.bin_width) return hipErrorInvalidValue;
    return hipSuccess;
}

hipError_t launch_list_census(const IbfDev &f, uint32_t *counters, uint64_t n_rows, uint64_t step, hipStream_t st)
{
    hipError_t e = list_builder_args_ok(f, n_rows);
    if (e != hipSuccess || step == 0) return hipErrorInvalidValue;
    const uint64_t looked_at = (n_rows + step - 1) / step;
    const uint64_t blocks = std::min<uint64_t>((looked_at + 3) / 4, 1ull << 20);
    hipLaunchKernelGGL(ibf_list_table_kernel, dim3((uint32_t)blocks), dim3(256), 0, st, f, (uint32_t *)nullptr, (uint64_t *)nullptr, counters, n_rows,
                       step, 0u, 0u);
    return hipGetLastError();
}

hipError_t launch_list_table(const IbfDev &f, uint16_t *slots, uint64_t *side, uint32_t *counters, uint64_t n_rows, uint32_t lines,
                             uint32_t side_cap, hipStream_t st)
{
    hipError_t e = list_builder_args_ok(f, n_rows);
    if (e != hipSuccess || !rblist::lines_valid(lines) || !slots || !side || !counters) return hipErrorInvalidValue;
    const uint64_t blocks = std::min<uint64_t>((n_rows + 3) / 4, 1ull << 20);
    hipLaunchKernelGGL(ibf_list_table_kernel, dim3((uint32_t)blocks), dim3(256), 0, st, f, reinterpret_cast<uint32_t *>(slots), side, counters, n_rows,
                       (uint64_t)1, lines, side_cap);
    return hipGetLastError();
}

// the list form serves what the row form serves, with one column slice of at most 128 words and strands of at most 65 535 k-mers (the
// engine checks the latter against the declared max_len: make_list_base_src never looks beyond it)
bool list_form_serves(const CountLaunch &a)
{
    return row_form_serves(a) && a.n_slices == 1 && a.f.n_bins <= rblist::kMaxBins && a.f.bin_width <= 128 && a.src.max_len != 0 &&
           a.src.max_len < a.f.k + rblist::kMaxKmers;
}

template <int LINES>
static hipError_t launch_lists_nt(const CountLaunch &a, hipStream_t st)
{
    const uint32_t cnt_dwords = rblist::count_cnt_dwords(a.f.n_bins);
    const size_t lds = rblist::count_lds_bytes(a.f.n_bins);
    const uint32_t flags = a.bound_prune ? kPruneBound : 0u;
    const uint32_t *slots = reinterpret_cast<const uint32_t *>(a.list_table);
    if (a.nt)
        hipLaunchKernelGGL((ibf_count_lists_kernel<LINES, true>), dim3(a.n_reads), dim3(64), lds, st, a.f, slots, a.list_side, a.list_side_rows, a.src,
                           a.n_reads, a.out, a.out_read_stride, flags, a.prune_trace, cnt_dwords);
    else
        hipLaunchKernelGGL((ibf_count_lists_kernel<LINES, false>), dim3(a.n_reads), dim3(64), lds, st, a.f, slots, a.list_side, a.list_side_rows, a.src,
                           a.n_reads, a.out, a.out_read_stride, flags, a.prune_trace, cnt_dwords);
    return hipGetLastError();
}

// the N-free reads from the list table, then the others from the filter's own table (launch_ibf_count_rows_twin, rb_kernels.hip)
hipError_t launch_ibf_count_lists(const CountLaunch &a, hipStream_t st)
{
    if (a.n_reads == 0) return hipSuccess;
    if (!a.list_table || !a.list_side || !list_form_serves(a)) return hipErrorInvalidValue;
    hipError_t e = a.list_lines == 1 ? launch_lists_nt<1>(a, st) : a.list_lines == 2 ? launch_lists_nt<2>(a, st) : a.list_lines == 4 ? launch_lists_nt<4>(a, st) : hipErrorInvalidValue;
    if (e != hipSuccess) return e;
    return launch_ibf_count_rows_twin(a, st);
}


}  // namespace rb

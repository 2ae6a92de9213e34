// rb_wide_lists.hip -- the WIDE LIST FORM of the plain count kernel, for filters of 8193 to 32 256 bins (rb_wide_lists.h): the filter's
// wide list table -- per N-free k-mer the bins of its row, the AND of its h blocks, in one slot of 4, 6 or 8 lines -- its builder and
// census, and the kernel that counts from it.  A translation unit of its own beside rb_lists.hip, whose device helpers
// (rb_lists_device.h: how a read's bases are found, the adds, the packed maximum) it shares; what it shares in turn with the wide forms
// of locate and hits (rb_wide_pass_lists.hip) -- a batch of slot gathers, a strand counted in full -- is in rb_wide_lists_device.h.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "rb_device.h"
#include "rb_lists.h"
#include "rb_lists_device.h"
#include "rb_wide_lists.h"
#include "rb_wide_lists_device.h"

namespace rb {

// One WORKGROUP of NW waves, one read.  At 31 000 bins the 16-bit counters of a strand take 62 KiB, so a CU holds two workgroups: with
// one wave each, as ibf_count_lists_kernel has, that would be two waves per CU.  So the NW waves of a workgroup share ONE counter array
// -- the LDS adds return nothing and commute across waves as they do across lanes -- and the strand's tiles of 64 k-mers are dealt to
// them round-robin (tile t to wave t mod NW); each wave stages its own tile's bases.  Clear and scan are split across the waves with a
// workgroup barrier around them, and the waves' partial maxima meet in LDS.
// A k-mer with a base outside ACGT has no slot but hashes to real blocks and counts (the forward strand hashes N as ordinal 4, the
// reverse strand f.comp_n): the wave that holds its tile fetches its h blocks from the filter's own table, ANDs them and counts the
// set bits one by one -- the dense-row path that overflow slots take.  No twin launch: a batch without an N pays one ballot per tile.
// Pruning (flags & kPruneBound): the second strand is not counted when the first reached n.  No stop within a strand (it would scan
// 62 KiB across waves at tile edges) and no trace: the engine gives a call that asks for one the plain kernel.
template <int LINES, bool NT, int NW>
__global__ __launch_bounds__(64 * NW) void ibf_count_wide_lists_kernel(IbfDev f, const uint32_t *__restrict__ slots, const uint64_t *__restrict__ side,
                                                                       uint32_t side_rows, ReadSrc src, uint32_t n_reads, uint16_t *__restrict__ out,
                                                                       uint32_t out_read_stride, uint32_t flags, uint32_t cnt_dwords)
{
    static_assert(LINES == 4 || LINES == 6 || LINES == 8, "slot sizes of rb_wide_lists.h");
    extern __shared__ uint32_t s_lds[];
    uint32_t *cnt = s_lds;  // cnt_dwords counters (a multiple of 256), kWideSpareDwords spares
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    uint8_t *stage = reinterpret_cast<uint8_t *>(s_lds + cnt_dwords + rbwide::kWideSpareDwords) + wave * rbwide::kWideStageBytes;
    uint32_t *red = reinterpret_cast<uint32_t *>(reinterpret_cast<uint8_t *>(s_lds + cnt_dwords + rbwide::kWideSpareDwords) + NW * rbwide::kWideStageBytes);
    const uint32_t read = blockIdx.x;
    if (read >= n_reads) return;  // the whole workgroup

    uint32_t len;
    const ListBaseSrc seq = make_list_base_src(src, read, &len);
    const uint32_t k = f.k;
    const uint32_t n = len >= k ? len - k + 1 : 0;
    const bool bound = (flags & kPruneBound) != 0;
    const uint32_t spare = cnt_dwords + lane;
    const uint32_t nh = f.n_hash < rbspec::kMaxHash ? f.n_hash : rbspec::kMaxHash;
    uint4 *c4 = reinterpret_cast<uint4 *>(cnt);
    for (uint32_t i = threadIdx.x; i < cnt_dwords / 4; i += 64 * NW) c4[i] = make_uint4(0, 0, 0, 0);
    __syncthreads();
    uint32_t best = 0;
#pragma unroll 1
    for (int strand = 0; strand < 2; ++strand) {
        if (bound && strand == 1 && best >= n) break;  // the same `best` in every wave
        // (the tile loop stands here and not as a call of wide_count_strand, which is this loop for the kernels that count a strand in
        // full: the call compiles to other instructions -- ten to fourteen more -- and this kernel keeps the measured ones)
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
        __syncthreads();
        // ---- the strand's maximum: every wave scans its share of the counters (and, behind the first strand, clears it)
        list_u16x2 a = {0, 0};
        for (uint32_t i = threadIdx.x; i < cnt_dwords / 4; i += 64 * NW) {
            const uint4 q = c4[i];
            a = __builtin_elementwise_max(list_max2(list_max2(a, q.x), q.y), list_max2(__builtin_bit_cast(list_u16x2, q.z), q.w));
            if (strand == 0) c4[i] = make_uint4(0, 0, 0, 0);
        }
        const uint32_t part = wave_max_u32(max((uint32_t)a.x, (uint32_t)a.y));
        if (lane == 0) red[wave] = part;
        __syncthreads();
        uint32_t m = 0;
#pragma unroll
        for (int w = 0; w < NW; ++w) m = max(m, red[w]);
        best = max(best, (uint32_t)__builtin_amdgcn_readfirstlane((int)m));
    }
    if (threadIdx.x == 0) out[(size_t)read * out_read_stride] = (uint16_t)best;
}

// The wide list table of a filter in the RESIDENT form (rb_wide_lists.h), one wave per slot, the waves striding over the slots: the AND
// of the k-mer's h blocks, words lane, lane + 64, ... lane + 448 of it per lane (a block of at most 504 words: up to 8 words per lane);
// one wave prefix sum of the lanes' even and odd populations, packed into one word (at most 16 128 either); and every lane writes the
// counter offsets of its set bits -- even bins into the low halves from dword 0 up, odd bins into the high halves, what one parity's
// halves cannot take into the other's free halves with the swapped flag -- into the slot's image in LDS, which starts as the dwords'
// spares and leaves as whole dwords.  A row with more set bits than the slot holds takes the next row of the side table (an atomic
// counter) and leaves an overflow slot; past `side_cap` it writes no row, and the host, which reads the counter, refuses the table.
// Slot addresses are 64-bit throughout: 4^13 slots of 8 lines are 64 GiB.
// lines == 0 is the CENSUS: nothing is written but counters[1 + i] += 1 for a row with more than 64 x kWideLines[i] set bits; `step`
// is the distance between the rows it looks at.
constexpr int kWideWordsPerLane = 8;
__global__ __launch_bounds__(256) void ibf_wide_list_table_kernel(IbfDev f, uint32_t *__restrict__ slots, uint64_t *__restrict__ side,
                                                                  uint32_t *__restrict__ counters, uint64_t n_rows, uint64_t step, uint32_t lines,
                                                                  uint32_t side_cap)
{
    __shared__ uint16_t s_slot[4][rbwide::kWideMaxLines * rblist::kEntriesPerLine];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    const uint64_t S = f.stride;
    const uint32_t W = f.bin_width;
    const uint32_t nh = f.n_hash < rbspec::kMaxHash ? f.n_hash : rbspec::kMaxHash;
    const uint32_t rem = f.n_bins & 63u;
    const uint32_t cnt_dwords = rbwide::cnt_dwords(f.n_bins);
    constexpr uint64_t kEven = 0x5555555555555555ULL;  // bin 64 w + b is even where b is
    uint16_t *img = s_slot[wave];
    for (uint64_t r = (((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6) * step; r < n_rows; r += waves * step) {  // wave-uniform
        uint64_t v = 0;
        for (uint32_t i = 0; i < f.k; ++i) v = v * 5u + ((r >> (2u * (f.k - 1u - i))) & 3u);
        uint32_t blk[rbspec::kMaxHash];
#pragma unroll
        for (uint32_t h = 0; h < rbspec::kMaxHash; ++h)
            blk[h] = h < nh ? rbspec::block_index(v, f.precalc[h], f.n_blocks, f.magic, f.pow2_mask) : 0u;
        uint64_t word[kWideWordsPerLane];
        uint32_t mine = 0;  // the lane's even bins, and its odd bins << 16 (at most 256 each)
#pragma unroll
        for (int j = 0; j < kWideWordsPerLane; ++j) {
            const uint32_t w = lane + 64u * j;
            uint64_t acc = 0;
            if (w < W) {
                acc = ~0ULL;
#pragma unroll
                for (uint32_t h = 0; h < rbspec::kMaxHash; ++h)
                    if (h < nh) acc &= f.words[(uint64_t)blk[h] * S + w];
                if (w == W - 1 && rem) acc &= (1ULL << rem) - 1;
            }
            word[j] = acc;
            mine += (uint32_t)__popcll(acc & kEven) + ((uint32_t)__popcll(acc & ~kEven) << 16);
        }
        uint32_t incl = mine;  // at most 16 128 in either half
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
                for (uint32_t i = 0; i < rbwide::kWideSizes; ++i)
                    if (set > rbwide::slot_entries(rbwide::kWideLines[i])) atomicAdd(&counters[1 + i], 1u);
            continue;
        }
        const uint32_t cap = lines * rblist::kEntriesPerLine, half = cap / 2, dw = lines / 2;
        __builtin_amdgcn_wave_barrier();
        for (uint32_t d = lane; d < half; d += 64)  // the image's dwords: their spares in both halves
            reinterpret_cast<uint32_t *>(img)[d] = ((cnt_dwords + d / dw) * 4u) * 0x10001u;
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
        __builtin_amdgcn_wave_barrier();
        if (set <= cap) {
            uint32_t rank[2] = {(incl - mine) & 0xFFFFu, (incl - mine) >> 16};
#pragma unroll 1
            for (int j = 0; j < kWideWordsPerLane; ++j) {
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
                for (int j = 0; j < kWideWordsPerLane; ++j) {
                    const uint32_t w = lane + 64u * j;
                    if (w < S) side[(uint64_t)idx * S + w] = word[j];
                }
                for (uint32_t w = lane + 64u * kWideWordsPerLane; w < S; w += 64) side[(uint64_t)idx * S + w] = 0;
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
        __builtin_amdgcn_wave_barrier();
        for (uint32_t d = lane; d < half; d += 64) slots[r * half + d] = reinterpret_cast<const uint32_t *>(img)[d];
    }
}

// what the wide table can be built for, whatever the bits
static hipError_t wide_builder_args_ok(const IbfDev &f, uint64_t n_rows)
{
    if (n_rows == 0 || n_rows > (1ull << (2 * kRowTableMaxK)) || f.k == 0 || f.k > kRowTableMaxK) return hipErrorInvalidValue;
    if (!rbwide::bins_served(f.n_bins) || f.bin_width != (f.n_bins + 63u) / 64u || f.stride < f.bin_width) return hipErrorInvalidValue;
    return hipSuccess;
}

hipError_t launch_wide_list_census(const IbfDev &f, uint32_t *counters, uint64_t n_rows, uint64_t step, hipStream_t st)
{
    hipError_t e = wide_builder_args_ok(f, n_rows);
    if (e != hipSuccess || step == 0 || !counters) return hipErrorInvalidValue;
    const uint64_t looked_at = (n_rows + step - 1) / step;
    const uint64_t blocks = std::min<uint64_t>((looked_at + 3) / 4, 1ull << 20);
    hipLaunchKernelGGL(ibf_wide_list_table_kernel, dim3((uint32_t)blocks), dim3(256), 0, st, f, (uint32_t *)nullptr, (uint64_t *)nullptr, counters,
                       n_rows, step, 0u, 0u);
    return hipGetLastError();
}

hipError_t launch_wide_list_table(const IbfDev &f, uint32_t *slots, uint64_t *side, uint32_t *counters, uint64_t n_rows, uint32_t lines,
                                  uint32_t side_cap, hipStream_t st)
{
    hipError_t e = wide_builder_args_ok(f, n_rows);
    if (e != hipSuccess || !rbwide::lines_valid(lines) || !slots || !side || !counters) return hipErrorInvalidValue;
    const uint64_t blocks = std::min<uint64_t>((n_rows + 3) / 4, 1ull << 20);
    hipLaunchKernelGGL(ibf_wide_list_table_kernel, dim3((uint32_t)blocks), dim3(256), 0, st, f, slots, side, counters, n_rows, (uint64_t)1, lines,
                       side_cap);
    return hipGetLastError();
}

// 8193 to 32 256 bins in blocks that carry just them, three hash functions, k <= 13, strands of at most 65 535 k-mers (the engine checks
// the latter against the declared max_len: make_list_base_src never looks beyond it)
bool wide_form_serves(const IbfDev &f, uint32_t max_len)
{
    return rbwide::bins_served(f.n_bins) && f.bin_width == (f.n_bins + 63u) / 64u && f.n_hash == 3 && f.k >= 1 && f.k <= kRowTableMaxK &&
           max_len != 0 && max_len < f.k + rbwide::kWideMaxKmers;
}

template <int LINES>
static hipError_t launch_wide_nt(const WideCountLaunch &a, hipStream_t st)
{
    constexpr int NW = (int)rbwide::kWideWaves;
    const uint32_t cnt_dwords = rbwide::cnt_dwords(a.f.n_bins);
    const size_t lds = rbwide::count_lds_bytes(a.f.n_bins, NW);
    const uint32_t flags = a.bound_prune ? kPruneBound : 0u;
    if (a.nt)
        hipLaunchKernelGGL((ibf_count_wide_lists_kernel<LINES, true, NW>), dim3(a.n_reads), dim3(64 * NW), lds, st, a.f, a.slots, a.side, a.side_rows,
                           a.src, a.n_reads, a.out, a.out_read_stride, flags, cnt_dwords);
    else
        hipLaunchKernelGGL((ibf_count_wide_lists_kernel<LINES, false, NW>), dim3(a.n_reads), dim3(64 * NW), lds, st, a.f, a.slots, a.side, a.side_rows,
                           a.src, a.n_reads, a.out, a.out_read_stride, flags, cnt_dwords);
    return hipGetLastError();
}

hipError_t launch_ibf_count_wide_lists(const WideCountLaunch &a, hipStream_t st)
{
    if (a.n_reads == 0) return hipSuccess;
    if (!a.slots || !a.side || !a.out || !wide_form_serves(a.f, a.src.max_len)) return hipErrorInvalidValue;
    return a.lines == 4 ? launch_wide_nt<4>(a, st) : a.lines == 6 ? launch_wide_nt<6>(a, st) : a.lines == 8 ? launch_wide_nt<8>(a, st) : hipErrorInvalidValue;
}

}  // namespace rb

// rb_pair_lists.hip -- the PAIR FORM of the plain count kernel: a filter's pair table (rb_pair_lists.h: per N-free k-mer x the bins of
// row(x) AND of row(rc(x)) in one slot of three lines), its builder and census, and the kernel that counts both strands from it.  A
// translation unit of its own beside rb_lists.hip, whose device helpers (rb_lists_device.h: how a read's bases are found, the adds, the
// packed maximum) it includes.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "rb_device.h"
#include "rb_lists.h"
#include "rb_lists_device.h"
#include "rb_pair_lists.h"
#include "rb_pair_lists_launch.h"

namespace rb {

typedef const uint32_t __attribute__((address_space(1))) *pair_gptr;  // global: the gathers are global_load and count on vmcnt alone

// slot `rank` of lane u, as a scalar pointer: the 64-bit product stays in scalar registers (4^13 slots of 384 bytes are 24 GiB), the
// lane's dword is the load's vector offset
__device__ __forceinline__ pair_gptr pair_slot_ptr(const uint32_t *__restrict__ slots, uint32_t rank, int u)
{
    const uint64_t a = reinterpret_cast<uint64_t>(slots) + (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)rank, u) * (rbpair::kPairDwords * 4u);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)a), hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(a >> 32));
    return reinterpret_cast<pair_gptr>(((uint64_t)hi << 32) | lo);
}

// a dword of line 2 or of a tail line: bit 0 of a half names the list, and is evaluated for every half
__device__ __forceinline__ void pair_add_rest(uint32_t *cnt, uint32_t v)
{
    char *base = reinterpret_cast<char *>(cnt);
    __hip_atomic_fetch_add(reinterpret_cast<uint32_t *>(base + (v & rbpair::kPairOffset)), (v & rbpair::kPairListB) * 0xFFFFu + 1u, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_WORKGROUP);
    __hip_atomic_fetch_add(reinterpret_cast<uint32_t *>(base + ((v >> 16) & rbpair::kPairOffset)), ((v >> 16) & rbpair::kPairListB) * 0xFFFFu + 1u,
                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// One tile of a wave: the slots of its k-mers 0 .. in_tile - 1 (FULL: all 64, and nothing is guarded).  Group by group of eight slots:
// eight loads of lines 0-1 (one dword per lane) and four of line 2 (two slots per load: lanes 0-31 the even slot, lanes 32-63 the odd
// one), all issued back to back; then, group by group as the loads land, the adds: lines 0-1 with list_add2 (low half forward strand,
// high half reverse strand), line 2 with the list bit.  No branch stands between the loads and the adds of a tile.  A line-2 dword that
// is an index (rb_pair_lists.h: the last dword of a tail or dense slot, lanes 31 and 63) is replaced by the lane's spares where it is
// found, by a select, and its slot is noted; the noted slots' tail lines and dense rows are counted behind the tile's adds.
template <bool NT, bool FULL>
__device__ __forceinline__ void pair_batch(const IbfDev &f, uint32_t *cnt, const uint32_t *__restrict__ slots, const uint32_t *__restrict__ tails,
                                           uint32_t tail_rows, const uint64_t *__restrict__ side, uint32_t side_rows, uint32_t rank, uint32_t in_tile,
                                           uint32_t lane, uint32_t cnt_dwords)
{
    constexpr int G = 8;
    const uint32_t blank_v = ((cnt_dwords + lane) * 4u) * 0x10001u;
    const uint32_t q0 = 2u * (lane & 31u);
    const uint32_t blank_w = ((cnt_dwords + q0) * 4u) | (((cnt_dwords + q0 + 1u) * 4u) << 16);
    uint32_t v[64], w[32];
#pragma unroll
    for (int g = 0; g < 64 / G; ++g) {
        if (FULL || (uint32_t)(g * G) < in_tile) {  // wave-uniform
#pragma unroll
            for (int u = 0; u < G; ++u) {
                const int s = g * G + u;
                v[s] = blank_v;
                if (FULL || (uint32_t)s < in_tile) {  // wave-uniform
                    const pair_gptr p = pair_slot_ptr(slots, rank, s) + lane;
                    v[s] = NT ? __builtin_nontemporal_load(p) : *p;
                }
            }
#pragma unroll
            for (int j = 0; j < G / 2; ++j) {
                const int s = g * G + 2 * j;
                w[s / 2] = blank_w;
                if (FULL || (uint32_t)s < in_tile) {  // wave-uniform
                    const bool odd = FULL || (uint32_t)(s + 1) < in_tile;
                    const pair_gptr r0 = pair_slot_ptr(slots, rank, s), r1 = odd ? pair_slot_ptr(slots, rank, s + 1) : r0;
                    const pair_gptr p = (lane < 32 ? r0 : r1) + rbpair::kPairPositional + (lane & 31u);
                    if (FULL || lane < 32 || odd) w[s / 2] = NT ? __builtin_nontemporal_load(p) : *p;
                }
            }
        }
        __builtin_amdgcn_sched_barrier(0);
    }
    uint64_t indexed = 0;  // bit 31 - j: slot 2 j is a tail or dense slot; bit 63 - j: slot 2 j + 1
#pragma unroll
    for (int g = 0; g < 64 / G; ++g) {
        if (FULL || (uint32_t)(g * G) < in_tile) {  // wave-uniform
#pragma unroll
            for (int u = 0; u < G; ++u) list_add2(cnt, v[g * G + u]);
#pragma unroll
            for (int j = 0; j < G / 2; ++j) {
                const int jj = g * (G / 2) + j;
                const bool is_index = (w[jj] & rbpair::kPairIndex) != 0u;
                indexed |= (__ballot(is_index) & 0x8000000080000000ull) >> jj;
                pair_add_rest(cnt, is_index ? blank_w : w[jj]);
            }
        }
        __builtin_amdgcn_sched_barrier(0);
    }
    while (__builtin_expect(indexed != 0ull, 0)) {  // wave-uniform, rare: the slot's index once more, then its tail line or its dense rows
        const uint32_t bit = (uint32_t)__builtin_ctzll(indexed);
        indexed &= indexed - 1;
        const uint32_t s = bit < 32u ? 2u * (31u - bit) : 2u * (63u - bit) + 1u;
        const uint32_t slot = (uint32_t)__builtin_amdgcn_readlane((int)rank, (int)s);
        const uint32_t last = slots[(uint64_t)slot * rbpair::kPairDwords + rbpair::kPairIndexDword];
        const uint32_t idx = rbpair::index_of(last);
        if (last & rbpair::kPairDense) {
            if (side_rows < 2u || idx > side_rows - 2u) continue;  // (the builder never names rows it did not write)
            const uint64_t *row = side + (uint64_t)idx * f.stride;
            for (uint32_t c = lane; c < f.bin_width; c += 64) {
                uint64_t fw = row[c], rv = row[f.stride + c];
                while (fw) {
                    const uint32_t bin = c * 64u + (uint32_t)__builtin_ctzll(fw);
                    fw &= fw - 1;
                    if (bin < f.n_bins) __hip_atomic_fetch_add(&cnt[bin], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                }
                while (rv) {
                    const uint32_t bin = c * 64u + (uint32_t)__builtin_ctzll(rv);
                    rv &= rv - 1;
                    if (bin < f.n_bins) __hip_atomic_fetch_add(&cnt[bin], 0x10000u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                }
            }
        } else {
            if (idx >= tail_rows) continue;
            if (lane < rbpair::kPairTailDwords) pair_add_rest(cnt, tails[(uint64_t)idx * rbpair::kPairTailDwords + lane]);
        }
    }
}

// One WORKGROUP of NW waves, one read, ONE counter array: a dword per bin, the low half the forward strand's count and the high half the
// reverse strand's.  N-free reads only (a workgroup whose read has a base outside ACGT leaves at once: the three-hash twin
// ibf_count_rows_kernel<.., false>, launched behind this kernel, writes those).  The read's tiles of 64 k-mers are dealt to the waves
// round-robin (tile t to wave t mod NW); each wave stages its own tile's bases and ranks its k-mers FORWARD only: the slot of x holds
// the list of rc(x) as well.  One clear at the start, one scan at the end: the packed 16-bit maximum over all halves is the maximum
// over both strands.  No strand skip and no stop within a strand -- both strands are fetched together -- so bound pruning changes nothing.
template <bool NT, int NW>
__global__ __launch_bounds__(64 * NW, NW) void ibf_count_pair_lists_kernel(IbfDev f, const uint32_t *__restrict__ slots,
                                                                           const uint32_t *__restrict__ tails, uint32_t tail_rows,
                                                                           const uint64_t *__restrict__ side, uint32_t side_rows, ReadSrc src,
                                                                           uint32_t n_reads, uint16_t *__restrict__ out, uint32_t out_read_stride,
                                                                           uint32_t cnt_dwords)
{
    extern __shared__ uint32_t s_lds[];
    uint32_t *cnt = s_lds;  // cnt_dwords counters (a multiple of 256), kPairSpareDwords spares
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    uint8_t *stage = reinterpret_cast<uint8_t *>(s_lds + cnt_dwords + rbpair::kPairSpareDwords) + wave * rbpair::kPairStageBytes;
    uint32_t *red = reinterpret_cast<uint32_t *>(reinterpret_cast<uint8_t *>(s_lds + cnt_dwords + rbpair::kPairSpareDwords) + NW * rbpair::kPairStageBytes);
    const uint32_t read = blockIdx.x;
    if (read >= n_reads) return;  // the whole workgroup

    uint32_t len;
    const ListBaseSrc seq = make_list_base_src(src, read, &len);
    const uint32_t k = f.k;
    const uint32_t n = len >= k ? len - k + 1 : 0;
    int outside = 0;
    for (uint32_t i = threadIdx.x; i < len; i += 64 * NW) outside |= seq.ord(i) > 3u;
    uint4 *c4 = reinterpret_cast<uint4 *>(cnt);
    for (uint32_t i = threadIdx.x; i < cnt_dwords / 4; i += 64 * NW) c4[i] = make_uint4(0, 0, 0, 0);
    if (__syncthreads_or(outside)) return;  // the whole workgroup: the twin's read
#pragma unroll 1
    for (uint32_t mt = wave * 64u; mt < n; mt += 64u * NW) {  // wave-uniform
        const uint32_t wlen = min(64u + k - 1u, len - mt);
        __builtin_amdgcn_wave_barrier();
        if (lane < wlen) stage[lane] = (uint8_t)seq.ord(mt + lane);
        if (lane + 64u < wlen) stage[lane + 64u] = (uint8_t)seq.ord(mt + 64u + lane);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
        __builtin_amdgcn_wave_barrier();
        uint32_t rank = 0;
        if (mt + lane < n) {
            const uint8_t *b = stage + lane;
            for (uint32_t i = 0; i < k; ++i) rank = (rank << 2) | (b[i] & 3u);
        }
        const uint32_t in_tile = (uint32_t)__builtin_amdgcn_readfirstlane((int)min(64u, n - mt));
        if (in_tile == 64u) pair_batch<NT, true>(f, cnt, slots, tails, tail_rows, side, side_rows, rank, in_tile, lane, cnt_dwords);
        else pair_batch<NT, false>(f, cnt, slots, tails, tail_rows, side, side_rows, rank, in_tile, lane, cnt_dwords);
    }
    __syncthreads();
    // ---- the read's maximum over both strands: every wave scans its share of the counters, the partial maxima meet in LDS
    list_u16x2 a = {0, 0};
    for (uint32_t i = threadIdx.x; i < cnt_dwords / 4; i += 64 * NW) {
        const uint4 q = c4[i];
        a = __builtin_elementwise_max(list_max2(list_max2(a, q.x), q.y), list_max2(__builtin_bit_cast(list_u16x2, q.z), q.w));
    }
    const uint32_t part = wave_max_u32(max((uint32_t)a.x, (uint32_t)a.y));
    if (lane == 0) red[wave] = part;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t m = 0;
#pragma unroll
        for (int w = 0; w < NW; ++w) m = max(m, red[w]);
        out[(size_t)read * out_read_stride] = (uint16_t)m;
    }
}

// The pair table of a filter, one wave per slot, the waves striding over the slots: the AND of the h blocks of x (list A) and of rc(x)
// (list B), words `lane` and `lane + 64` of each per lane (a block of at most 128 words); one wave prefix sum per list of the lanes'
// populations, the two words of a lane packed into one; and every lane writes the counter offsets of its set bits into the slot's image in LDS -- lines 0-1
// positional, line 2 and, for a tail slot, the tail line in list order -- which starts as the spares and leaves as whole dwords.  Tail
// lines and dense row pairs are allocated by atomic counters (the order may vary from build to build, the contents may not); past the
// capacities nothing is written, and the host, which reads the counters, refuses the table.
// build == 0 is the CENSUS: nothing is written but counters[1] += 1 for a pair that needs a tail or more and counters[2] += 1 for one
// that needs dense rows (and counters[0], counters[3] += 1 for a row(x) of more than 64, 128 bins: the list table's census on the same
// sample); `step` is the distance between the x it looks at.
__global__ __launch_bounds__(256) void ibf_pair_table_kernel(IbfDev f, uint32_t *__restrict__ slots, uint32_t *__restrict__ tails,
                                                             uint64_t *__restrict__ side, uint32_t *__restrict__ counters, uint64_t n_rows,
                                                             uint64_t step, uint32_t build, uint32_t tail_cap, uint32_t side_cap)
{
    constexpr uint32_t IMG = rbpair::kPairDwords + rbpair::kPairTailDwords;  // the slot, then the tail line
    __shared__ uint32_t s_img[4][IMG];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    const uint64_t S = f.stride;
    const uint32_t W = f.bin_width;
    const uint32_t nh = f.n_hash < rbspec::kMaxHash ? f.n_hash : rbspec::kMaxHash;
    const uint32_t rem = f.n_bins & 63u;
    const uint32_t cd = rbpair::cnt_dwords(f.n_bins);
    uint32_t *img = s_img[wave];
    uint16_t *img16 = reinterpret_cast<uint16_t *>(img);
    for (uint64_t r = (((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6) * step; r < n_rows; r += waves * step) {  // wave-uniform
        uint64_t val[2] = {0, 0};  // x and rc(x) as the filter hashes them: base 5, first base most significant
        for (uint32_t i = 0; i < f.k; ++i) {
            val[0] = val[0] * 5u + ((r >> (2u * (f.k - 1u - i))) & 3u);
            val[1] = val[1] * 5u + (3u - ((r >> (2u * i)) & 3u));
        }
        uint64_t word[2][2];
        uint32_t mine[2] = {0, 0};  // per list: the lane's bins in its word `lane`, and those in its word `lane + 64` << 16 (at most 64 each)
#pragma unroll
        for (int l = 0; l < 2; ++l)
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const uint32_t w = lane + 64u * j;
                uint64_t acc = 0;
                if (w < W) {
                    acc = ~0ULL;
                    for (uint32_t h = 0; h < nh; ++h) {
                        const uint32_t b = rbspec::block_index(val[l], f.precalc[h], f.n_blocks, f.magic, f.pow2_mask);
                        acc &= f.words[(uint64_t)b * S + w];
                    }
                    if (w == W - 1 && rem) acc &= (1ULL << rem) - 1;
                }
                word[l][j] = acc;
                mine[l] += (uint32_t)__popcll(acc) << (16 * j);
            }
        // the lists are ASCENDING: bins 64 w + b of the words w = 0 .. 63 come before those of the words 64 .. 127, so a lane's bins of
        // its first word rank behind the first words of the lanes below it, those of its second word behind all first words
        uint32_t incl[2] = {mine[0], mine[1]};  // at most 4096 in either half
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t o0 = (uint32_t)__shfl_up((int)incl[0], d, 64), o1 = (uint32_t)__shfl_up((int)incl[1], d, 64);
            if (lane >= (uint32_t)d) incl[0] += o0, incl[1] += o1;
        }
        const uint32_t total[2] = {(uint32_t)__builtin_amdgcn_readlane((int)incl[0], 63), (uint32_t)__builtin_amdgcn_readlane((int)incl[1], 63)};
        const uint32_t n_list[2] = {(total[0] & 0xFFFFu) + (total[0] >> 16), (total[1] & 0xFFFFu) + (total[1] >> 16)};
        const rbpair::PairKind kind = rbpair::kind_of(n_list[0], n_list[1]);
        if (!build) {
            if (lane == 0 && kind != rbpair::kPlain) atomicAdd(&counters[1], 1u);
            if (lane == 0 && kind == rbpair::kDenseRows) atomicAdd(&counters[2], 1u);
            // (what the list table's census would say of row(x): more than one line, more than two)
            if (lane == 0 && n_list[0] > rblist::kEntriesPerLine) atomicAdd(&counters[0], 1u);
            if (lane == 0 && n_list[0] > 2u * rblist::kEntriesPerLine) atomicAdd(&counters[3], 1u);
            continue;
        }
        __builtin_amdgcn_wave_barrier();
        img[lane] = rbpair::spare_of_dword(f.n_bins, lane) * 0x10001u;  // lines 0-1
        {  // line 2 (lanes 0-31) and the tail line (lanes 32-63): the spares of the halves' positions
            const uint32_t q = 2u * (lane & 31u);
            img[rbpair::kPairPositional + lane] = ((cd + q) * 4u) | (((cd + q + 1u) * 4u) << 16);
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
        __builtin_amdgcn_wave_barrier();
        uint32_t idx = 0;
        if (kind != rbpair::kDenseRows) {
            const uint32_t in_slot = kind == rbpair::kTail ? rbpair::kPairRestIndexed : rbpair::kPairRest;
            const uint32_t rest_a = n_list[0] > rbpair::kPairPositional ? n_list[0] - rbpair::kPairPositional : 0u;
#pragma unroll
            for (int l = 0; l < 2; ++l) {
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const uint32_t below = incl[l] - mine[l];
                    uint32_t at = j ? (total[l] & 0xFFFFu) + (below >> 16) : below & 0xFFFFu;
                    uint64_t bits = word[l][j];
                    while (bits) {
                        const uint32_t bit = (uint32_t)__builtin_ctzll(bits);
                        bits &= bits - 1;
                        const uint32_t off = ((lane + 64u * j) * 64u + bit) * 4u;  // the bin's counter dword
                        if (at < rbpair::kPairPositional) {
                            img16[2u * at + l] = (uint16_t)off;
                        } else {
                            // q < rest_of(nA, nB) <= 126: within line 2 (in_slot halves) and the tail line (64 halves)
                            const uint32_t q = (l ? rest_a : 0u) + (at - rbpair::kPairPositional);
                            const uint32_t h = off | (l ? rbpair::kPairListB : 0u);
                            if (q < in_slot) img16[2u * rbpair::kPairPositional + q] = (uint16_t)h;
                            else img16[2u * rbpair::kPairDwords + (q - in_slot)] = (uint16_t)h;
                        }
                        ++at;
                    }
                }
            }
            if (kind == rbpair::kTail) {
                if (lane == 0) idx = atomicAdd(&counters[1], 1u);
                idx = (uint32_t)__builtin_amdgcn_readfirstlane((int)idx);
                if (lane == 0) img[rbpair::kPairIndexDword] = rbpair::index_dword(idx, false);  // (its halves hold no entry: in_slot ends before them)
            }
        } else {
            if (lane == 0) idx = atomicAdd(&counters[0], 2u);
            idx = (uint32_t)__builtin_amdgcn_readfirstlane((int)idx);
            if (lane == 0) img[rbpair::kPairIndexDword] = rbpair::index_dword(idx, true);
            if (idx <= rbpair::kPairMaxIndex && (uint64_t)idx + 2u <= side_cap) {
#pragma unroll
                for (int l = 0; l < 2; ++l) {
#pragma unroll
                    for (int j = 0; j < 2; ++j) {
                        const uint32_t w = lane + 64u * j;
                        if (w < S) side[((uint64_t)idx + l) * S + w] = word[l][j];
                    }
                    for (uint32_t w = lane + 128u; w < S; w += 64) side[((uint64_t)idx + l) * S + w] = 0;
                }
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
        __builtin_amdgcn_wave_barrier();
        slots[r * rbpair::kPairDwords + lane] = img[lane];
        if (lane < 32) slots[r * rbpair::kPairDwords + 64u + lane] = img[64u + lane];
        if (kind == rbpair::kTail && idx < tail_cap && lane < rbpair::kPairTailDwords)
            tails[(uint64_t)idx * rbpair::kPairTailDwords + lane] = img[rbpair::kPairDwords + lane];
    }
}

// what the pair table can be built for, whatever the bits
static hipError_t pair_builder_args_ok(const IbfDev &f, uint64_t n_rows)
{
    if (n_rows == 0 || n_rows > (1ull << (2 * kRowTableMaxK)) || f.k == 0 || f.k > kRowTableMaxK || n_rows != (1ull << (2 * f.k))) return hipErrorInvalidValue;
    if (f.bin_width == 0 || f.bin_width > 128 || f.n_bins > rbpair::kPairMaxBins || f.stride < f.bin_width) return hipErrorInvalidValue;
    return hipSuccess;
}

hipError_t launch_pair_census(const IbfDev &f, uint32_t *counters, uint64_t n_rows, uint64_t step, hipStream_t st)
{
    hipError_t e = pair_builder_args_ok(f, n_rows);
    if (e != hipSuccess || step == 0 || !counters) return hipErrorInvalidValue;
    const uint64_t looked_at = (n_rows + step - 1) / step;
    const uint64_t blocks = std::min<uint64_t>((looked_at + 3) / 4, 1ull << 20);
    hipLaunchKernelGGL(ibf_pair_table_kernel, dim3((uint32_t)blocks), dim3(256), 0, st, f, (uint32_t *)nullptr, (uint32_t *)nullptr, (uint64_t *)nullptr,
                       counters, n_rows, step, 0u, 0u, 0u);
    return hipGetLastError();
}

hipError_t launch_pair_table(const IbfDev &f, uint32_t *slots, uint32_t *tails, uint64_t *side, uint32_t *counters, uint64_t n_rows,
                             uint32_t tail_cap, uint32_t side_cap, hipStream_t st)
{
    hipError_t e = pair_builder_args_ok(f, n_rows);
    if (e != hipSuccess || !slots || !tails || !side || !counters) return hipErrorInvalidValue;
    const uint64_t blocks = std::min<uint64_t>((n_rows + 3) / 4, 1ull << 20);
    hipLaunchKernelGGL(ibf_pair_table_kernel, dim3((uint32_t)blocks), dim3(256), 0, st, f, slots, tails, side, counters, n_rows, (uint64_t)1, 1u,
                       tail_cap, side_cap);
    return hipGetLastError();
}

// what the list form serves: the row form's launches with one column slice of at most 128 words, at most 8192 bins and strands of at
// most 65 535 k-mers (a count fits its half of a counter dword)
bool pair_form_serves(const CountLaunch &a) { return list_form_serves(a) && a.f.n_bins <= rbpair::kPairMaxBins; }

// the N-free reads from the pair table, then the others from the filter's own table (launch_ibf_count_rows_twin, rb_kernels.hip)
hipError_t launch_ibf_count_pair_lists(const PairCountLaunch &a, hipStream_t st)
{
    constexpr int NW = (int)rbpair::kPairWaves;
    const CountLaunch &c = a.count;
    if (c.n_reads == 0) return hipSuccess;
    if (!a.slots || !a.tails || !a.side || !c.out || c.prune_trace || !pair_form_serves(c)) return hipErrorInvalidValue;
    const uint32_t cnt_dwords = rbpair::cnt_dwords(c.f.n_bins);
    const size_t lds = rbpair::count_lds_bytes(c.f.n_bins, NW);
    if (c.nt)
        hipLaunchKernelGGL((ibf_count_pair_lists_kernel<true, NW>), dim3(c.n_reads), dim3(64 * NW), lds, st, c.f, a.slots, a.tails, a.tail_rows, a.side,
                           a.side_rows, c.src, c.n_reads, c.out, c.out_read_stride, cnt_dwords);
    else
        hipLaunchKernelGGL((ibf_count_pair_lists_kernel<false, NW>), dim3(c.n_reads), dim3(64 * NW), lds, st, c.f, a.slots, a.tails, a.tail_rows, a.side,
                           a.side_rows, c.src, c.n_reads, c.out, c.out_read_stride, cnt_dwords);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_ibf_count_rows_twin(c, st);
}

}  // namespace rb

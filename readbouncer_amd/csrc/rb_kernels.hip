// rb_kernels.hip -- hand-written CDNA4 (gfx950) kernels of the IBF classify path.
//
//   K1 ibf_count_max : seqan::count(filter, seq) + seqan::count(filter, TSeqRevComp(seq)) +
//                      the max over bins/strands of Read::max_matches
//                      (src/IBF/IBFClassify.cpp:149-150, 48-71); fuses the (Dna5String) conversion
//                      of src/main/classify.hpp:272.
//   K2 decide        : threshold + argmax + decision (IBFClassify.cpp:154-162, 262-273, 299-365;
//                      src/main/adaptive_sampling.hpp:35-113; src/main/classify.hpp:58-111,275-292)
//   K4 ibf_insert    : seqan::insertKmer (src/IBF/IBFBuild.cpp:190)
//   fill_synth       : benchmark filler
//
// Design (DESIGN.md has the long form).  The path is integer/bitwise and HBM-gather bound: per read
// and filter 2*(L-k+1)*h random blocks of 8*W bytes.  One 64-lane wave owns one (read, column slice):
//   * phase A: every lane hashes its own k-mer of a 64-k-mer tile (base-5 value, h multiplicative
//     hashes, Barrett reduction mod noOfBlocks) -- the block numbers stay in registers;
//   * phase B: the wave walks the tile; a group of LPB = 2^LG lanes covers one block with one
//     8-byte (or 16-byte) word column per lane, so every wave-level load instruction is 64/LPB
//     fully coalesced block gathers; block numbers travel by ds_bpermute / v_readlane;
//   * per-bin counters are BIT-SLICED: lane-private 64-bit planes, one bit per bin, fed by a
//     Harley-Seal carry-save tree (7 CSAs per 8 gathered words) -- no atomics, no LDS traffic,
//     10 or 16 planes (16 planes wrap at 65536 exactly like the reference's uint16_t counters);
//   * the max over bins is taken on the bit-sliced form with 64-wide ballots, MSB plane first.
// Forms that share that body (count_strand): the throughput form (one wave per read and column slice, both strands in
// sequence; slices of a read sit side by side in a workgroup), its MERGED variant (several narrow filters of one hash geometry
// in one table, one gather per lookup for all of them), the PHASED variant for narrow filters on their own (clock-phased
// slices of the table, bounds-checked buffer gathers, both strands in one round) and the latency form for micro-batches (one or several
// workgroups per read; their waves split strands and k-mer tiles, add their bit-sliced counters through LDS and -- across
// workgroups -- through a workspace and an arrival counter; one launch serves filters of different geometries).  Gathers are
// issued in batches of 12-24 per wave with no control flow around them and a schedule fence before the first use;
// filters beyond the Infinity Cache are read with non-temporal loads.  Inputs may be ASCII or 2-bit packed reads, whole
// or chunked on the device (BaseSrc / ReadSrc).
// No MFMA anywhere: there is no multiply-accumulate structure in this path.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <type_traits>

#include "rb_device.h"

namespace rb {

// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t shfl32(uint32_t v, int src_lane)
{
    return (uint32_t)__builtin_amdgcn_ds_bpermute(src_lane << 2, (int)v);
}
__device__ __forceinline__ uint64_t shfl64(uint64_t v, int src_lane)
{
    uint32_t lo = shfl32((uint32_t)v, src_lane), hi = shfl32((uint32_t)(v >> 32), src_lane);
    return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ uint32_t readlane32(uint32_t v, int uniform_lane)
{
    return (uint32_t)__builtin_amdgcn_readlane((int)v, uniform_lane);
}

// Table gathers.  NT = non-temporal: for a table far beyond the 256 MiB Infinity Cache every block is touched
// once and caching it only evicts something else (measured on config 3: +2.4 %); a table that fits the cache
// keeps the default policy (config 2 loses 1.9 % with NT).  The engine picks per filter by table size.
typedef unsigned long long rb_u64x2 __attribute__((ext_vector_type(2)));
template <bool NT>
__device__ __forceinline__ uint64_t load_word(const uint64_t *p)
{
    if constexpr (NT) return __builtin_nontemporal_load(p);
    else return *p;
}
template <bool NT>
__device__ __forceinline__ rb_u64x2 load_word2(const uint64_t *p)
{
    if constexpr (NT) return __builtin_nontemporal_load(reinterpret_cast<const rb_u64x2 *>(p));
    else return *reinterpret_cast<const rb_u64x2 *>(p);
}

// number of the XCD this wave runs on (0-7): a placement fact, used for speed only
__device__ __forceinline__ uint32_t xcc_id()
{
    uint32_t v;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(v));
    return v & 0xFu;
}

// carry-save adder on bit planes: (h, l) = a + b + c per bit position
#define RB_CSA(h, l, a, b, c)                \
    {                                        \
        const uint64_t u__ = (a) ^ (b);      \
        const uint64_t c__ = (c);            \
        (h) = ((a) & (b)) | (u__ & c__);     \
        (l) = u__ ^ c__;                     \
    }

template <int NP>
struct Planes {
    uint64_t p[NP];  // p[i] holds bit i of 64 per-bin counters
    __device__ __forceinline__ void clear()
    {
#pragma unroll
        for (int i = 0; i < NP; ++i) p[i] = 0;
    }
    // fold 8 one-bit-per-bin words into the counters (Harley-Seal)
    __device__ __forceinline__ void add8(const uint64_t x[8])
    {
        uint64_t twosA, twosB, foursA, foursB, eights;
        RB_CSA(twosA, p[0], p[0], x[0], x[1]);
        RB_CSA(twosB, p[0], p[0], x[2], x[3]);
        RB_CSA(foursA, p[1], p[1], twosA, twosB);
        RB_CSA(twosA, p[0], p[0], x[4], x[5]);
        RB_CSA(twosB, p[0], p[0], x[6], x[7]);
        RB_CSA(foursB, p[1], p[1], twosA, twosB);
        RB_CSA(eights, p[2], p[2], foursA, foursB);
        uint64_t carry = eights;
#pragma unroll
        for (int i = 3; i < NP; ++i) {
            const uint64_t t = p[i] & carry;
            p[i] ^= carry;
            carry = t;
        }
    }
    // counters += counters held by lane (lane ^ xor_mask)
    __device__ __forceinline__ void add_from_lane_xor(int lane, int xor_mask)
    {
        uint64_t carry = 0;
#pragma unroll
        for (int i = 0; i < NP; ++i) {
            const uint64_t o = shfl64(p[i], lane ^ xor_mask);
            uint64_t h, l;
            RB_CSA(h, l, p[i], o, carry);
            p[i] = l;
            carry = h;
        }
    }
};

// 64 x 64 bit-matrix transpose across the wave: bit j of lane i <-> bit i of lane j (six block swaps)
__device__ __forceinline__ uint64_t wave_transpose64(uint64_t x, int lane)
{
    constexpr uint64_t kMask[6] = {0x00000000FFFFFFFFULL, 0x0000FFFF0000FFFFULL, 0x00FF00FF00FF00FFULL,
                                   0x0F0F0F0F0F0F0F0FULL, 0x3333333333333333ULL, 0x5555555555555555ULL};
    // first swap (32 x 32 blocks): the high words of lanes 0-31 change places with the low words of lanes 32-63 -- one v_permlane32_swap
    // (gfx950) instead of two ds_bpermute and the selects around them
    {
        const auto r = __builtin_amdgcn_permlane32_swap((uint32_t)x, (uint32_t)(x >> 32), false, false);
        x = ((uint64_t)r[1] << 32) | r[0];
    }
#pragma unroll
    for (int t = 1; t < 6; ++t) {
        const int sft = 32 >> t;
        const uint64_t m = kMask[t];
        const uint64_t o = shfl64(x, lane ^ sft);
        x = (lane & sft) ? ((x & ~m) | ((o & ~m) >> sft)) : ((x & m) | ((o & m) << sft));
    }
    return x;
}

// per-bin counts of 4 one-bit-per-bin words per lane, summed over the 64 lanes: lane b returns the count of bin b.
// The lane-local sum (0..4 per bin) is three bit planes; each plane is transposed across the wave, so that lane b holds
// bit b of every lane's plane word, and a popcount finishes the sum -- 36 cross-lane moves instead of the 120 of a
// butterfly over ten counter planes.
__device__ __forceinline__ uint32_t wave_bin_counts4(uint64_t x0, uint64_t x1, uint64_t x2, uint64_t x3, int lane)
{
    uint64_t h, l;
    RB_CSA(h, l, x0, x1, x2);
    const uint64_t c = l & x3;
    const uint64_t p0 = l ^ x3, p1 = h ^ c, p2 = h & c;
    return (uint32_t)__popcll(wave_transpose64(p0, lane)) + 2u * (uint32_t)__popcll(wave_transpose64(p1, lane)) +
           4u * (uint32_t)__popcll(wave_transpose64(p2, lane));
}

// the same for 6 one-bit-per-bin words per lane (sums 0..6: still three planes, three transposes)
__device__ __forceinline__ uint32_t wave_bin_counts6(uint64_t x0, uint64_t x1, uint64_t x2, uint64_t x3, uint64_t x4,
                                                     uint64_t x5, int lane)
{
    uint64_t h1, l1, h2, l2, p2, p1;
    RB_CSA(h1, l1, x0, x1, x2);
    RB_CSA(h2, l2, x3, x4, x5);
    const uint64_t p0 = l1 ^ l2, c = l1 & l2;
    RB_CSA(p2, p1, h1, h2, c);
    return (uint32_t)__popcll(wave_transpose64(p0, lane)) + 2u * (uint32_t)__popcll(wave_transpose64(p1, lane)) +
           4u * (uint32_t)__popcll(wave_transpose64(p2, lane));
}

template <int T>
__device__ __forceinline__ uint32_t wave_bin_counts(const uint64_t *x, int lane)
{
    if constexpr (T == 6) return wave_bin_counts6(x[0], x[1], x[2], x[3], x[4], x[5], lane);
    else if constexpr (T == 2)  // sums 0..2: two planes, two transposes
        return (uint32_t)__popcll(wave_transpose64(x[0] ^ x[1], lane)) + 2u * (uint32_t)__popcll(wave_transpose64(x[0] & x[1], lane));
    else if constexpr (T == 3) {  // sums 0..3: one carry-save step, two planes
        uint64_t h, l;
        RB_CSA(h, l, x[0], x[1], x[2]);
        return (uint32_t)__popcll(wave_transpose64(l, lane)) + 2u * (uint32_t)__popcll(wave_transpose64(h, lane));
    }
    else return wave_bin_counts4(x[0], x[1], x[2], x[3], lane);
}

// max over all bins held by the wave (WPL plane sets per lane), MSB plane first
template <int NP, int WPL>
__device__ __forceinline__ uint32_t planes_max(const Planes<NP> (&pl)[WPL], const uint64_t (&valid)[WPL])
{
    uint64_t cand[WPL];
#pragma unroll
    for (int w = 0; w < WPL; ++w) cand[w] = valid[w];
    uint32_t res = 0;
#pragma unroll
    for (int i = NP - 1; i >= 0; --i) {
        uint64_t t[WPL];
        bool any = false;
#pragma unroll
        for (int w = 0; w < WPL; ++w) {
            t[w] = cand[w] & pl[w].p[i];
            any |= (t[w] != 0);
        }
        if (__ballot(any) != 0ULL) {  // wave-uniform
            res |= 1u << i;
#pragma unroll
            for (int w = 0; w < WPL; ++w) cand[w] = t[w];
        }
    }
    return res;
}

// steps of the plain kernels whose gathers go out together (8-byte lanes / 16-byte lanes).  The wide kernels are HBM bound
// and do not care: 4 waves per SIMD with half the loads in flight run at the same 0.864-0.866 of 8 TB/s on config 3
// (profiles/r03/window_sweep.txt, session 19)
#ifndef RB_HALF1
#define RB_HALF1 8
#endif
#ifndef RB_HALF2
#define RB_HALF2 4
#endif

// ---------------------------------------------------------------------------------------------
// K1.  LG: log2(lanes per block); WPL: 64-bit word columns per lane (1 or 2); NP: counter planes;
// H: compile-time number of hash functions, 0 = run-time (slow path, hashes in phase B).
constexpr int kWavesPerBlock = 4;
constexpr int kMaxTiles = 8;                                      // tiles per macro tile when LG < 3
constexpr int kStageBytes = 64 * kMaxTiles + rbspec::kMaxKmer;    // bases staged per macro tile

template <int LG>
struct TileShape {
    static constexpr int LPB = 1 << LG;                 // lanes that cover one block
    static constexpr int NG = 64 >> LG;                 // blocks gathered per wave instruction
    static constexpr int SPT = LPB;                     // phase-B steps per 64-k-mer tile
    static constexpr int J = SPT >= 8 ? 1 : 8 / SPT;    // tiles per macro tile (so that steps come in eights)
    static constexpr int STEPS = SPT * J;
    static constexpr int ITEMS = 64 * J;                // k-mers per macro tile
};

// per-lane view of the column slice a wave works on
template <int WPL>
struct LaneCols {
    uint64_t valid[WPL];        // bins of this lane's word(s) that exist (padding and foreign columns masked)
    const uint64_t *lane_base;  // f.words + first word column of this lane
    const uint64_t *safe_base;  // lane_base, or f.words for a lane that owns no (complete) column: always loadable
    bool colok;                 // lane owns at least one existing column
    bool col_full;              // WPL == 2: both words exist, a 16-byte load is allowed
};

template <int LG, int WPL>
__device__ __forceinline__ LaneCols<WPL> make_lane_cols(const IbfDev &f, int lane, uint32_t col_begin, uint32_t col_end,
                                                        uint32_t slice)
{
    constexpr int LPB = 1 << LG;
    const int c = lane & (LPB - 1);
    const uint32_t W = f.bin_width;
    const uint32_t col0 = col_begin + slice * (uint32_t)(LPB * WPL) + (uint32_t)(c * WPL);
    LaneCols<WPL> lc;
    lc.colok = false;
#pragma unroll
    for (int w = 0; w < WPL; ++w) {
        const uint32_t col = col0 + w;
        const bool ok = col < col_end;
        const uint32_t rem = f.n_bins & 63u;
        lc.valid[w] = !ok ? 0ULL : (col == W - 1 && rem) ? ((1ULL << rem) - 1) : ~0ULL;
        lc.colok |= ok;
    }
    lc.col_full = (col0 + WPL) <= col_end;
    lc.lane_base = f.words + col0;
    // WPL == 2 with an odd column count: the last lane owns one column; its 16-byte load also fetches the word
    // after it (next column of the block, or the first word past the block -- still inside the filter thanks to the
    // 256 metadata bits at the tail) and valid[1] == 0 masks it.  Blocks of an odd-width filter are only 8-byte
    // aligned: gfx950 executes 16-byte global loads at 8-byte alignment (checked on the device).
    lc.safe_base = lc.colok ? lc.lane_base : f.words;
    return lc;
}

// Bases of one read as the kernel sees them: ASCII bytes (nm == nullptr) or the packed form of SURVEY 8f.4 --
// 2 bits per base (A0 C1 G2 T3; base i in bits 2*(i&3) of byte i>>2) plus an N bitmap (bit i&7 of byte i>>3) that
// turns a base into Dna5 ordinal 4.  `first` = bases skipped at the start of the read (on-GPU chunking).
struct BaseSrc {
    const uint8_t *bytes;  // ASCII: already advanced to the first base; packed: start of the read's 2-bit payload
    const uint8_t *nm;     // packed: start of the read's N bitmap; ASCII: nullptr
    uint32_t first;        // packed: index of the first base of the chunk inside the read
    __device__ __forceinline__ uint32_t ord(uint32_t i) const
    {
        if (nm == nullptr) return rbspec::dna5_ord(bytes[i]);
        const uint32_t b = first + i;
        const uint32_t code = (bytes[b >> 2] >> ((b & 3u) << 1)) & 3u;
        return ((nm[b >> 3] >> (b & 7u)) & 1u) ? 4u : code;
    }
};

// Batch sizes of the phased window loop (phased_window_loop below): k-mers of a lane whose gathers go out together (B: one-word blocks, three 8-byte loads per k-mer; KB: two-word blocks,
// three 16-byte loads per k-mer).  Every load in flight holds its destination registers, so the batch size sets the
// occupancy: with ALL lookups of a window in flight (8 k-mers, 48 registers) the 250 bp one-word kernel has five waves per
// SIMD, with two k-mers per batch six (73 VGPRs) -- four waits per window instead of one, and 7 % less time per read; the
// six-tile kernel goes from four to five waves (93 VGPRs), the two-word 250 bp kernel from four to five (86).  Measured
// per shape in profiles/r03/window_sweep.txt; the window lengths of rb_engine.hip belong to these values.
#ifndef RB_GATHER_B1
#define RB_GATHER_B1 2
#endif
#ifndef RB_GATHER_KB1
#define RB_GATHER_KB1 1
#endif
#ifndef RB_GATHER_B3
#define RB_GATHER_B3 2
#endif
#ifndef RB_GATHER_KB3
#define RB_GATHER_KB3 2
#endif
#ifndef RB_WIDE_WAVES  // waves per SIMD the four-tile build for THREE-word blocks is compiled for (94 registers, no scratch; the
                       // four-word build would spill 104 bytes at five waves and stays at four: 116 registers)
#define RB_WIDE_WAVES 5
#endif
#ifndef RB_WIDE_TILES  // tiles per strand and round of the three- / four-word build for reads of 257-512 k-mers
#define RB_WIDE_TILES 3
#endif
#ifndef RB_GATHER_BG  // per-strand tiles of the general build (reads of more than 512 k-mers, blocks of 3-8 words)
#define RB_GATHER_BG 2
#endif
typedef unsigned int rb_u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int rb_u32x4 __attribute__((ext_vector_type(4)));
constexpr int kBufRsrcWord3 = 0x00020000;  // raw buffer, DATA_FORMAT = 32 bit (gfx9 family)

// Which slice a wave gathers next: the one the wall clock names NOW, if the wave has not served it yet; otherwise the wave
// sleeps until the clock has moved on.  A wave that is ahead of the clock therefore waits for its next window, and a wave
// that has fallen behind does NOT work through the windows it missed -- their slices have left the L2 -- but joins the chip on
// the current slice and picks the missed ones up when they come round again (round 2 walked the slices in a fixed order:
// a window that was too short for the waves then cost a factor of two, profiles/r03/window_sweep.txt).  Bounded: if the
// clock does not move for ~0.1 ms (its 32-bit wrap, a window length of 0) the lowest slice still open is taken.
__device__ __forceinline__ uint32_t phase_next_slice(uint32_t done, const PhaseCfg &ph)
{
    for (;;) {
        const uint32_t wn = (uint32_t)(((uint64_t)((uint32_t)wall_clock64() + ph.tskew) * ph.inv_ticks) >> 32);
        const uint32_t cur = (wn + ph.skew) % ph.n_slices;
        if (!((done >> cur) & 1u)) return cur;
        bool moved = false;
        for (uint32_t guard = 0; guard < 2048; ++guard) {
            __builtin_amdgcn_s_sleep(2);
            const uint32_t w2 = (uint32_t)(((uint64_t)((uint32_t)wall_clock64() + ph.tskew) * ph.inv_ticks) >> 32);
            if (w2 != wn) { moved = true; break; }
        }
        if (!moved) return (uint32_t)__builtin_ctz(~done);  // done has a zero bit below n_slices: the caller loops while it does
    }
}

// The window loop of the phased form -- ONE body for every block width a single lane holds (NW = 1 to 4 words; the three entry
// points below only name the load widths): x*[u] &= the words of the block at byte offset bn[u][*] of `words`, each gathered in the
// window of its slice.  0xFFFFFFFF = no lookup.  The predication is done by the BOUNDS CHECK of a raw buffer descriptor, not by
// exec masks: per window the wave points the descriptor at the slice of the moment (base = slice start, num_records = slice
// bytes) and issues every lookup as buffer_load with the offset (lookup - slice start): a lane whose lookup lies in another
// slice (or that has none) is out of range, makes no memory access and gets 0 back, which an OR with the lane's out-of-range
// mask turns into the neutral all-ones.  No saveexec, no branch around a load, no scalar work per lookup (the exec-masked loads
// of round 2: ~11 instructions per lookup and window, seven of them scalar or branches, every destination register kept
// initialised across the window loop).
// How a table is cut is carried by slice_shift (rb_engine.hip, plan_geometry): a plain value = slices of 2^slice_shift bytes
// (31: one slice that holds every offset -- with ph = {n_slices 1, inv_ticks 0} that is one batch of gathers with no waiting,
// for tables that need no phasing); bit 31 set + a non-zero length in the low bits = slices of that many BYTES, any multiple of
// the block size (equal-length slices, rb_phase_plan.h).  Blocks never straddle a slice.
// Loads per lookup: NW 1 = one 8-byte, 2 = one 16-byte, 3 = 16 + 8 bytes, 4 = two 16-byte (blocks of 3 and 4 words lie at a
// stride of 4 words, 32-byte aligned).  K k-mers of a lane go out together (KB): every load in flight holds its destination
// registers, so the batch size sets the occupancy (see RB_GATHER_* above).
template <int NW, int N, int H, int KB>
__device__ __forceinline__ void phased_window_loop(uint64_t (&x0)[N], uint64_t (&x1)[N], uint64_t (&x2)[N], uint64_t (&x3)[N],
                                                   const uint32_t (&bn)[N][H], const uint64_t *words, uint32_t slice_shift,
                                                   const PhaseCfg ph)
{
    static_assert(NW >= 1 && NW <= 4, "one lane holds blocks of one to four words");
    static_assert(N % KB == 0, "the k-mers of a lane are gathered in batches of KB");
    const uint32_t all = ph.n_slices >= 32 ? ~0u : (1u << ph.n_slices) - 1u;  // one bit per slice
    uint32_t done = 0;
#pragma unroll 1
    while (done != all) {
        const uint32_t cur = phase_next_slice(done, ph);
        done |= 1u << cur;
        const bool any_len = (slice_shift >> 31) != 0 && slice_shift != 0x80000000u;
        const uint32_t span = any_len ? (slice_shift & 0x7FFFFFFFu) : 1u << min(slice_shift, 31u);  // (slice_shift == 31: a single slice, cur == 0)
        const uint32_t start = any_len ? cur * span : cur << min(slice_shift, 31u);
        __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
            const_cast<char *>(reinterpret_cast<const char *>(words)) + start, 0, (int)span, kBufRsrcWord3);
#pragma unroll
        for (int part = 0; part < N / KB; ++part) {
            rb_u32x2 lo2[KB][H], hi2[KB][H];  // NW 1: the block; NW 3: its third word
            rb_u32x4 lo4[KB][H], hi4[KB][H];  // NW 2-4: words 0-1; NW 4: words 2-3
#pragma unroll
            for (int uu = 0; uu < KB; ++uu) {
#pragma unroll
                for (int h = 0; h < H; ++h) {
                    // (the offsets are made opaque at both uses: otherwise `offset - start` of all lookups is computed up front
                    // and kept for the masks below -- 24 registers, a wave per SIMD on the 250 bp one-word kernel)
                    uint32_t off = bn[part * KB + uu][h];
                    asm volatile("" : "+v"(off));
                    if constexpr (NW == 1) lo2[uu][h] = __builtin_amdgcn_raw_buffer_load_b64(rs, off - start, 0, 0);
                    else lo4[uu][h] = __builtin_amdgcn_raw_buffer_load_b128(rs, off - start, 0, 0);
                    // ("no lookup" stays out of range with bit 4 set)
                    if constexpr (NW == 3) hi2[uu][h] = __builtin_amdgcn_raw_buffer_load_b64(rs, (off - start) | 16u, 0, 0);
                    if constexpr (NW == 4) hi4[uu][h] = __builtin_amdgcn_raw_buffer_load_b128(rs, (off - start) | 16u, 0, 0);
                }
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int uu = 0; uu < KB; ++uu) {
#pragma unroll
                for (int h = 0; h < H; ++h) {
                    uint32_t off = bn[part * KB + uu][h];
                    asm volatile("" : "+v"(off));
                    const uint32_t out = (off - start) >= span ? 0xFFFFFFFFu : 0u;  // lanes that loaded nothing
                    const int u = part * KB + uu;
                    if constexpr (NW == 1) {
                        x0[u] &= (((uint64_t)(lo2[uu][h].y | out)) << 32) | (lo2[uu][h].x | out);
                    } else {
                        x0[u] &= (((uint64_t)(lo4[uu][h].y | out)) << 32) | (lo4[uu][h].x | out);
                        x1[u] &= (((uint64_t)(lo4[uu][h].w | out)) << 32) | (lo4[uu][h].z | out);
                    }
                    if constexpr (NW == 3) x2[u] &= (((uint64_t)(hi2[uu][h].y | out)) << 32) | (hi2[uu][h].x | out);
                    if constexpr (NW == 4) {
                        x2[u] &= (((uint64_t)(hi4[uu][h].y | out)) << 32) | (hi4[uu][h].x | out);
                        x3[u] &= (((uint64_t)(hi4[uu][h].w | out)) << 32) | (hi4[uu][h].z | out);
                    }
                }
            }
        }
    }
}

// one-word blocks (8-byte gathers): x = the word of each of the lane's N k-mers
template <int N, int H, bool NT, int B = N>
__device__ __forceinline__ void phased_gather(uint64_t (&x)[N], const uint32_t (&bn)[N][H], const uint64_t *words,
                                              uint32_t slice_shift, const PhaseCfg ph)
{
    phased_window_loop<1, N, H, B>(x, x, x, x, bn, words, slice_shift, ph);
}

// two-word blocks held by ONE lane (16-byte gathers): x0 / x1 = the two word columns of the lane's N k-mers
template <int N, int H, int KB>
__device__ __forceinline__ void phased_gather_x2(uint64_t (&x0)[N], uint64_t (&x1)[N], const uint32_t (&bn)[N][H],
                                                 const uint64_t *words, uint32_t slice_shift, const PhaseCfg ph)
{
    phased_window_loop<2, N, H, KB>(x0, x1, x1, x1, bn, words, slice_shift, ph);
}

// three- and four-word blocks (stride 4 words) held by ONE lane: two gathers per lookup
template <int N, int H, int KB, int NW = 4>
__device__ __forceinline__ void phased_gather_x4(uint64_t (&x0)[N], uint64_t (&x1)[N], uint64_t (&x2)[N], uint64_t (&x3)[N],
                                                 const uint32_t (&bn)[N][H], const uint64_t *words, uint32_t slice_shift,
                                                 const PhaseCfg ph)
{
    static_assert(NW == 3 || NW == 4, "narrower blocks have entry points of their own");
    phased_window_loop<NW, N, H, KB>(x0, x1, x2, x3, bn, words, slice_shift, ph);
}

// PH = clock-phased gathers (PhaseCfg): for a table of a few L2 sizes -- one- and two-word blocks, 10-20 MB -- every
// 8-byte gather that misses the XCD's 4 MiB L2 costs a full 128-byte fabric request, and the chip serves about 60 G of
// those per second whatever their useful size (profiles/r02/gather_probe.txt: 76 G gathers/s on 20 MiB against 269 G/s
// from an L2-resident slice).  So the chip is made to work on ONE slice of the table at a time: the block numbers of a
// macro tile stay in registers (they do anyway), the wall clock (s_memrealtime, the same on every CU) names the slice of
// the moment, and each wave gathers only its lookups that fall into that slice, ANDing them into the per-k-mer words it
// keeps in registers; after n_slices windows every lookup has been served once, in whatever window its slice came up.
// Nothing depends on the timing but the speed: a wave that is ahead of the clock sleeps until its next window opens, one
// that is behind never waits, and the result is the same AND of the same words.
// Counts one strand of one read into the wave's bit-sliced counters, visiting the macro tiles
// mt_first, mt_first + mt_step, ... (mt_step = ITEMS walks the whole read; the split kernel interleaves waves) and of
// each macro tile the eight-step blocks [blk_first, blk_end) (all STEPS / 8 of them, or a wave's share in the split kernel).
// EARLY (the opt-in early-decision mode of the throughput form, rb_engine_set_early_decision): after every macro tile the running
// maximum of this wave's counters is compared with `stop_at`; once it is reached the strand is left (the counters are a lower bound of
// the read's, which is all the decision needs: see ibf_count_max_kernel) and true is returned.
// BOUND PRUNING (`bound_best` != kNoBound; blocks of one wave's width, LG == 6, plain gathers): after every macro tile the wave takes
// M = max(bound_best, max of its counters) -- bound_best is the exact maximum of the strand(s) counted before -- and rem = k-mers of
// this strand still to come.  Every k-mer adds at most 1 to a bin, so a bin with c + rem <= M ends at or below M whatever it gathers
// later.  A lane whose valid bins are all in that state is DEAD: its `ok` predicate goes false, so from the next tile on it loads
// block 0 of its column (cache-resident, what past-the-end steps read anyway) and adds nothing; once the 8 lanes of a 128-byte line
// are dead the line is no longer fetched from HBM, and once the whole wave is dead the strand is left.  Why the maximum stays exact:
// every counter the wave keeps is at most the bin's true count (a dead bin's counter stops early), and every dead bin's true count is
// at most the M it died against, which is itself a counter the wave still holds (counters never shrink) or the earlier strands' exact
// maximum -- so max(counters, bound_best) is the true maximum.  M and rem are wave-uniform; the test "some valid bin has c > M - rem"
// is a bit-sliced compare of the planes against that constant, MSB first, with a scalar branch per plane.  The caller passes
// kNoBound where counters can wrap (n >= 2^NP: the 16-plane builds reproduce the reference's uint16_t wrap, and the bound is false
// there) and where the engine switched pruning off (rb_engine_set_bound_pruning).
//
// Four refinements of the bound (ibf_count_max_kernel's `prune` word, rb_engine_set_prune_parts), and why the maximum stays exact:
//   * SUB-TILE CHECKS (`sub_checks`): the same compare after every eight-step block of a tile, behind a scalar gate, with rem taken at that
//     point and M_stale = the M of the last tile boundary.  It is the argument above with a smaller rem and an M that is never above the
//     true one (counters never shrink): a smaller M only kills later.  For a negative read the gate opens in the last ~13 k-mers only.
//   * STRAND LEAD (the caller's doing: `mt_first` > 0, `mt_end`): both strands are counted for their first tile, the one with the larger
//     probe maximum is finished first and the other continues from k-mer 64 against the leader's maximum.  The output is the maximum
//     over the strands and the strands' counters are separate, so the order is free.  A strand that continues (mt_first > 0) is checked
//     on entry like at a tile boundary: its counters hold the first mt_first k-mers.
//   * CERTIFICATE (the caller again; H == 1, EARLY, stop_at = M + 1, bound_best = M): a k-mer counts for a bin only where ALL h blocks
//     have the bit, so the count of hash-0 bits alone is an upper bound of the count.  On top of the trailing strand's probe counters
//     the rest of the strand is gathered for hash 0 only -- a third of the lines; for every bin, probe count + hash-0 hits of the rest
//     >= true count, so if the maximum of that stays <= M (the leader's maximum) the strand's maximum is <= M and the read's result
//     is M.  The bound prunes this pass too (an upper bound that cannot pass M any more need not be followed); the pass is left as
//     failed the moment a counter exceeds M, and the strand is then counted in full from its probe counters.
//   * LEAD LINE (the caller once more; `lanes`): the leader strand's passes take a subset of the lanes each -- first the line of its best probe
//     bin, then the rest as a certificate or in full (ibf_count_max_kernel).  A lane outside `lanes` behaves as a dead one from the start.
//   * `stop_pos` reports the k-mer position at which this call's gathers ended (n, or where the whole wave was dead).
constexpr uint32_t kNoBound = 0xFFFFFFFFu;

// bit-sliced "some valid bin of this lane has c > t", MSB plane first (t wave-uniform: one scalar branch per plane): gt = bins already
// above t, eq = bins equal to t's leading bits so far.  (Locate and hits run the same loop for their hit masks.  It is written out in all
// three places: as a shared function the compiler holds every plane twice unless t is forced scalar inside it, and either form changes
// the registers of these kernels -- the count builds' code with them.)
template <int NP, int WPL>
__device__ __forceinline__ bool bound_alive(const Planes<NP> (&pl)[WPL], const uint64_t (&valid)[WPL], uint32_t t)
{
    bool alive = false;
    if (t < (1u << NP) - 1u) {
#pragma unroll
        for (int w = 0; w < WPL; ++w) {
            uint64_t gt = 0, eq = valid[w];
#pragma unroll
            for (int i = NP - 1; i >= 0; --i) {
                if ((t >> i) & 1u) {  // scalar branch
                    eq &= pl[w].p[i];
                } else {
                    gt |= eq & pl[w].p[i];
                    eq &= ~pl[w].p[i];
                }
            }
            alive |= gt != 0ULL;
        }
    }
    return alive;
}

// SITE: a caller that starts tiles anywhere (mt_first arbitrary: the prefix pass) names an instantiation of its own.  The body is the same; what
// the compiler learns from the other callers' arguments before it inlines (mt_first 0 or a tile multiple) then stays theirs, and their kernels
// compile to the code they had (profiles/isa_identity.py).
// ROWS (H == 1; ibf_count_rows_kernel): `f.words` is the filter's ROW TABLE -- one row per N-free k-mer, the AND of its h blocks -- and the
// block number of a k-mer is its base-4 rank (first base most significant).  The caller hands over N-free reads only; a digit is masked to
// two bits all the same, so no rank leaves the table.
template <int LG, int WPL, int NP, int H, bool NT, bool PH = false, bool EARLY = false, int SITE = 0, bool ROWS = false>
__device__ __forceinline__ bool count_strand(Planes<NP> (&pl)[WPL], const IbfDev &f, const LaneCols<WPL> &lc,
                                             const BaseSrc &seq, uint32_t len, uint32_t n, int strand,
                                             uint32_t mt_first, uint32_t mt_step, int blk_first, int blk_end,
                                             uint8_t *stage, int lane, const PhaseCfg ph = PhaseCfg{0, 0, 0, 0, 0}, uint32_t stop_at = 0xFFFFFFFFu,
                                             uint32_t bound_best = kNoBound, uint32_t mt_end = 0xFFFFFFFFu, bool sub_checks = false,
                                             uint32_t *stop_pos = nullptr, uint64_t lanes = ~0ULL)
{
    using T = TileShape<LG>;
    constexpr int NG = T::NG, SPT = T::SPT, J = T::J, ITEMS = T::ITEMS;
    constexpr int HR = H > 0 ? H : 1;
    // the bound needs every lane to hold whole counts of its bins (one lane group per block) and a whole strand per wave
    constexpr bool BOUND = (LG == 6) && !PH && (H > 0);
    const int g = lane >> LG;
    const uint32_t S = f.stride;  // words between consecutive blocks in HBM (>= bin_width, see rb_engine.hip)
    const uint32_t k = f.k;
    // lane gathers (BOUND: and is not dead yet).  `lanes` (wave-uniform; the lead line) names the lanes that take part at all: the others are
    // off from the start -- they read block 0 and add 0, as dead lanes do, and keep the counters they came with
    bool lane_on = lc.colok;
    if constexpr (BOUND) {
        if (lanes != ~0ULL) lane_on = lane_on && ((lanes >> lane) & 1ULL) != 0;  // (scalar branch; callers without the argument compile as they did)
    }
    const uint32_t n_end = min(n, mt_end);  // k-mers this call counts up to
    uint32_t m_stale = bound_best;          // BOUND: the M of the last boundary check (scalar)
    uint32_t stopped = n_end;               // where the gathers ended: n_end, or the check that found the whole wave dead
    if constexpr (BOUND) {
        // a strand that continues behind its probe tile: the check of the tile boundary it starts at
        if (bound_best != kNoBound && mt_first > 0 && mt_first < n_end) {
            const uint32_t M = __builtin_amdgcn_readfirstlane(max(planes_max<NP, WPL>(pl, lc.valid), bound_best));
            const uint32_t rem = __builtin_amdgcn_readfirstlane(n - mt_first);
            m_stale = M;
            if (M >= rem) {
                lane_on = lane_on && bound_alive<NP, WPL>(pl, lc.valid, M - rem);
                if (__ballot(lane_on) == 0ULL) {
                    if (stop_pos) *stop_pos = mt_first;
                    return false;  // wave-uniform (NG == 1: no butterfly below)
                }
            }
        }
    }

    for (uint32_t mt = mt_first; mt < n_end; mt += mt_step) {
        // ---- stage the bases of this macro tile as Dna5 ordinals ((Dna5String) conversion)
        const uint32_t wlen = min((uint32_t)(ITEMS + k - 1), len - mt);
        __builtin_amdgcn_wave_barrier();
        for (uint32_t i = lane; i < wlen; i += 64) stage[i] = (uint8_t)seq.ord(mt + i);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
        __builtin_amdgcn_wave_barrier();

        // ---- phase A: one k-mer per lane and tile
        uint32_t idx[J][HR];
        uint64_t kv[J];
#pragma unroll
        for (int j = 0; j < J; ++j) {
            const uint32_t p = mt + j * 64 + lane;
            uint64_t v = 0;
            if (p < n) {
                const uint8_t *b = stage + (p - mt);
                if (strand == 0) {
                    for (uint32_t i = 0; i < k; ++i) v = v * 5u + b[i];
                } else {  // k-mer of the reverse complement that covers the same window
                    for (uint32_t i = 0; i < k; ++i) v = v * 5u + rbspec::dna5_comp(b[k - 1 - i], f.comp_n);
                }
            }
            kv[j] = v;
            if constexpr (ROWS) {
                static_assert(H == 1 && !PH, "a row holds the AND of all hash functions");
                uint32_t r = 0;
                if (p < n) {
                    const uint8_t *b = stage + (p - mt);
                    if (strand == 0) {
                        for (uint32_t i = 0; i < k; ++i) r = (r << 2) | (b[i] & 3u);
                    } else {
                        for (uint32_t i = 0; i < k; ++i) r = (r << 2) | (rbspec::dna5_comp(b[k - 1 - i], f.comp_n) & 3u);
                    }
                }
                idx[j][0] = r;
            } else if constexpr (H > 0) {
#pragma unroll
                for (int h = 0; h < H; ++h)
                    idx[j][h] = rbspec::block_index(v, f.precalc[h], f.n_blocks, f.magic, f.pow2_mask);
            }
        }

        // ---- phase B: gather + count, eight steps at a time.
        // The loads of a batch of steps are issued back to back and consumed afterwards, so that a wave keeps
        // 8*H (WPL = 1) or 4*H (WPL = 2) gathers in flight.  There is no control flow around the loads: steps past
        // the end of the read and lanes without a column read block 0 of the filter (always a valid, cache-resident
        // address) and are masked out of the result -- a branch per step would make the compiler drain the
        // memory pipe after every step (3 loads in flight instead of 24).
#pragma unroll 1
        for (int blk = blk_first; blk < blk_end; ++blk) {
            {
                const int s0 = blk * 8;
                const uint32_t first = mt + (uint32_t)((s0 / SPT) * 64 + (s0 % SPT) * NG);
                if (first >= n) break;  // wave-uniform
            }
            uint64_t x[WPL][8];
            if constexpr (H > 0 && PH) {
                static_assert(WPL == 1, "the phased form serves blocks of at most 8 words");
                // what a lane keeps per lookup is the BYTE offset of its word in the table (32 bits: the engine plans this
                // form for tables far below 4 GiB), so that the gathers take the scalar-base + 32-bit-offset form -- block
                // numbers plus 64-bit addresses would not leave room for three waves per SIMD
                uint32_t bn[8][H];
                const uint32_t col_bytes = (uint32_t)((lc.lane_base - f.words) * 8);
                const uint32_t slice_shift = (ph.shift >> 31) ? (0x80000000u | ((ph.shift & 0x7FFFFFFFu) * (uint32_t)(S * 8)))
                                                              : min(31u, ph.shift + 3u + (31u - (uint32_t)__builtin_clz(S)));  // S (words per block) is a power of two here
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const int s = blk * 8 + u;
                    const int j = (SPT >= 8) ? 0 : (u / SPT);
                    const int it = (s % SPT) * NG + g;
                    const uint32_t p = mt + (uint32_t)(j * 64 + it);
                    const bool ok = (p < n) && lc.colok;
                    x[0][u] = ok ? lc.valid[0] : 0ULL;
#pragma unroll
                    for (int h = 0; h < H; ++h) {
                        uint32_t b;
                        if constexpr (LG == 0) b = idx[j][h];
                        else b = shfl32(idx[j][h], it);
                        // a lookup that is not to be made gets an offset no slice ever has
                        bn[u][h] = ok ? b * (S * 8u) + col_bytes : 0xFFFFFFFFu;
                    }
                }
                phased_gather<8, H, NT, RB_GATHER_BG>(x[0], bn, f.words, slice_shift, ph);
            } else if constexpr (H > 0) {
                // steps per load batch (the one-hash pass of the certificate, H == 1, has a third of the loads per step: eight steps at once)
                constexpr int HALF = (WPL == 1 || H == 1) ? RB_HALF1 : RB_HALF2;
#pragma unroll
                for (int half = 0; half < 8 / HALF; ++half) {
                    uint64_t ld[HALF][H][WPL];
                    bool okv[HALF];
#pragma unroll
                    for (int uu = 0; uu < HALF; ++uu) {
                        const int u = half * HALF + uu;
                        const int s = blk * 8 + u;
                        const int j = (SPT >= 8) ? 0 : (u / SPT);  // compile-time either way
                        const int it = (s % SPT) * NG + g;          // k-mer of this group within tile j
                        const uint32_t p = mt + (uint32_t)(j * 64 + it);
                        const bool ok = (p < n) && lane_on;
                        okv[uu] = ok;
#pragma unroll
                        for (int h = 0; h < H; ++h) {
                            uint32_t b;
                            if constexpr (LG == 0) b = idx[j][h];
                            else if constexpr (LG == 6) b = readlane32(idx[j][h], it);
                            else b = shfl32(idx[j][h], it);
                            const uint64_t *src = lc.safe_base + (uint64_t)(ok ? b : 0u) * S;
                            if constexpr (WPL == 1) {
                                ld[uu][h][0] = load_word<NT>(src);
                            } else {
                                const rb_u64x2 q = load_word2<NT>(src);
                                ld[uu][h][0] = q.x;
                                ld[uu][h][1] = q.y;
                            }
                        }
                    }
                    // every gather of the batch is issued before the first one is consumed: without this fence the
                    // scheduler sinks loads next to their uses to save registers (seen in the ISA: vmcnt(3) instead
                    // of vmcnt(11..23)) and the wave is back to a few gathers in flight
                    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                    for (int uu = 0; uu < HALF; ++uu) {
#pragma unroll
                        for (int w = 0; w < WPL; ++w) {
                            uint64_t acc = okv[uu] ? lc.valid[w] : 0ULL;
#pragma unroll
                            for (int h = 0; h < H; ++h) acc &= ld[uu][h][w];
                            x[w][half * HALF + uu] = acc;
                        }
                    }
                }
            } else {
#pragma unroll
                for (int u = 0; u < 8; ++u) {
                    const int s = blk * 8 + u;
                    const int j = (SPT >= 8) ? 0 : (u / SPT);
                    const int it = (s % SPT) * NG + g;
                    const uint32_t p = mt + (uint32_t)(j * 64 + it);
                    const bool ok = (p < n) && lc.colok;
                    uint64_t acc[WPL];
#pragma unroll
                    for (int w = 0; w < WPL; ++w) acc[w] = ok ? lc.valid[w] : 0ULL;
                    const uint64_t v = (LG == 0) ? kv[j] : shfl64(kv[j], it);
                    if (ok) {
                        for (uint32_t h = 0; h < f.n_hash; ++h) {
                            const uint32_t bi = rbspec::block_index(v, f.precalc[h], f.n_blocks, f.magic, f.pow2_mask);
                            const uint64_t *src = lc.lane_base + (uint64_t)bi * S;
#pragma unroll
                            for (int w = 0; w < WPL; ++w) acc[w] &= (lc.valid[w] ? load_word<NT>(src + w) : 0ULL);
                        }
                    }
#pragma unroll
                    for (int w = 0; w < WPL; ++w) x[w][u] = acc[w];
                }
            }
#pragma unroll
            for (int w = 0; w < WPL; ++w) pl[w].add8(x[w]);
            if constexpr (BOUND) {
                // sub-tile check (behind the batch's last use: no control flow between its loads); the tile's last block is the boundary's
                const uint32_t donek = mt + (uint32_t)(blk + 1) * 8u;
                if (sub_checks && bound_best != kNoBound && blk + 1 < T::STEPS / 8 && donek < n) {
                    const uint32_t rem = __builtin_amdgcn_readfirstlane(n - donek);
                    if (m_stale >= rem) {  // the scalar gate: below it every bin is still within reach
                        lane_on = lane_on && bound_alive<NP, WPL>(pl, lc.valid, m_stale - rem);
                        if (__ballot(lane_on) == 0ULL) {
                            stopped = donek;
                            break;  // wave-uniform
                        }
                    }
                }
            }
        }
        if constexpr (BOUND) {
            if (stopped != n_end) break;
        }
        if constexpr (EARLY && !BOUND) {
            // (with several lane groups per block every group holds the counts of ITS k-mers only: a lower bound of a lower bound, still
            // sufficient; the butterfly below is skipped when the wave leaves here)
            if (planes_max<NP, WPL>(pl, lc.valid) >= stop_at) return true;
        }
        if constexpr (BOUND) {
            uint32_t m = 0;
            if (EARLY || bound_best != kNoBound) m = planes_max<NP, WPL>(pl, lc.valid);  // wave-uniform
            if (EARLY && m >= stop_at) return true;
            const uint32_t done = mt + (uint32_t)ITEMS;
            if (bound_best != kNoBound && done < n) {  // (after the last tile there is nothing left to skip)
                const uint32_t M = __builtin_amdgcn_readfirstlane(max(m, bound_best));
                const uint32_t rem = __builtin_amdgcn_readfirstlane(n - done);
                m_stale = M;
                if (M >= rem) {
                    lane_on = lane_on && bound_alive<NP, WPL>(pl, lc.valid, M - rem);  // a bin stays alive while its count exceeds M - rem
                    if (__ballot(lane_on) == 0ULL) {  // wave-uniform: the rest of this strand cannot change the maximum
                        stopped = done;
                        break;
                    }
                }
            }
        }
    }

    // ---- sum the partial counters of the NG groups (butterfly): every group then holds the total
    if constexpr (NG > 1) {
#pragma unroll
        for (int m = T::LPB; m < 64; m <<= 1) {
#pragma unroll
            for (int w = 0; w < WPL; ++w) pl[w].add_from_lane_xor(lane, m);
        }
    }
    if (stop_pos) *stop_pos = stopped;
    return false;
}

__device__ __forceinline__ BaseSrc make_base_src(const ReadSrc &r, uint32_t item, uint32_t *len_out)
{
    const uint32_t rid = r.ids ? r.ids[item] : item;
    const uint32_t len = r.lens[item];  // effective length of this work item (chunked or whole read)
    // never beyond the declared bound: lengths above it are the caller's error (the decision kernel says so per read), and lengths
    // that are not lengths at all -- a buffer the caller has not finished writing -- must not send K1 reading gigabytes away
    *len_out = (r.max_len && len > r.max_len) ? r.max_len : len;
    BaseSrc b;
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

// throughput form: one wave per (read, column slice), both strands in sequence
#ifndef RB_WAVES_PLAIN  // waves per SIMD the plain throughput kernel is compiled for (one word per lane, ten planes)
#define RB_WAVES_PLAIN 3
#endif
// EARLY: the opt-in early-decision mode (rb_engine_set_early_decision; RB_MODE_CHECK_UNBLOCK calls that do not ask for the raw maxima).
// check_unblock (src/main/adaptive_sampling.hpp:35-113) looks at a filter's count only through "count >= threshold at r" and "count >=
// threshold at r - 0.02" (the rescan of :55-56); both are decided for good the moment some bin of the filter reaches the larger of the
// two thresholds on either strand -- the reference counts on (and counts again for the rescan).  A wave that gets there writes the
// maximum it has, a lower bound >= both thresholds, and stops: the decision kernel's predicates come out as with the full count.  Work is
// SKIPPED in this mode: its reads/s are a product figure, never a roofline figure (bench.py reports it as `c3_early`, apart).
struct EarlyCfg {
    const uint16_t *thr;  // [thr_len][nf][2] thresholds at r and r - 0.02 by read length (the decision kernel's table)
    uint32_t thr_len, nf;
    uint32_t fi[kMaxFused];  // blockIdx.y -> filter index in the table
};

// STRAND LEAD (prune.flags, kPruneLead; plain builds with the bound, reads of more than one tile): the forward strand always going first
// wastes the bound on reads given as reverse complements -- their forward strand is counted in full against nothing, and the strand
// that holds the maximum then has nobody left to prune.  So both strands are PROBED for their first tile (64 k-mers), the forward
// probe's counters wait in LDS meanwhile (after 64 k-mers only planes 0-6 can be set: kParkPlanes x WPL x 64 lanes x 8 bytes per
// wave), the strand with the larger probe maximum LEADS (a tie: forward, so a read always takes the same path), and the other one
// continues from k-mer 64 against the leader's maximum, its probe counters back from LDS -- after an attempt to CERTIFY it from hash 0
// alone (count_strand) where the leader's maximum makes that promising.  The passes of a lead build are one loop around one count_strand
// call per H, so the three-hash gather schedule exists once in it.
constexpr int kParkPlanes = 7;
constexpr bool plain_leads(int lg, int h, bool early) { return lg == 6 && h > 0 && !early; }

template <int LG, int WPL, int NP, int H, bool NT, bool EARLY = false>
__global__ __launch_bounds__(64 * kWavesPerBlock) __attribute__((amdgpu_waves_per_eu((WPL == 1 && NP == 10 && H == 3) ? RB_WAVES_PLAIN : 3, 8))) void ibf_count_max_kernel(
    FilterSet set, ReadSrc src, uint32_t n_reads, uint32_t n_slices, uint16_t *__restrict__ out_base,
    uint32_t out_read_stride, uint32_t out_slice_stride, EarlyCfg early, PruneCfg prune)
{
    constexpr bool LEADS = plain_leads(LG, H, EARLY);
    constexpr uint32_t TILE = (uint32_t)TileShape<LG>::ITEMS;
    __shared__ uint8_t s_stage[kWavesPerBlock][kStageBytes];
    __shared__ uint64_t s_park[LEADS ? kWavesPerBlock : 1][LEADS ? kParkPlanes * WPL : 1][64];
    const IbfDev &f = set.f[blockIdx.y];  // filters of equal kernel geometry may share a launch (micro-batches)
    const uint32_t col_begin = set.col_begin[blockIdx.y], col_end = set.col_end[blockIdx.y];
    uint16_t *__restrict__ out = out_base + set.out_offset[blockIdx.y];
    const int lane = threadIdx.x & 63;
    // (scalar in the builds that carry the strand lead's state: so are the item, its read and its slice, which leaves them the registers; the
    // other builds -- config 2's among them -- are compiled as they were)
    const int wave = LG == 6 ? __builtin_amdgcn_readfirstlane(threadIdx.x >> 6) : (int)(threadIdx.x >> 6);
    // work item = (read, column slice), slice fastest: the waves of a workgroup gather neighbouring parts of the same
    // blocks at about the same time (DRAM page locality for wide filters)
    const uint64_t item = (uint64_t)blockIdx.x * kWavesPerBlock + wave;
    const uint32_t read = (uint32_t)(item / n_slices);
    const uint32_t slice = (uint32_t)(item - (uint64_t)read * n_slices);
    if (read >= n_reads) return;  // wave-uniform; there are no block-level barriers below

    const LaneCols<WPL> lc = make_lane_cols<LG, WPL>(f, lane, col_begin, col_end, slice);
    uint32_t len;
    const BaseSrc seq = make_base_src(src, read, &len);
    const uint32_t n = len >= f.k ? len - f.k + 1 : 0;

    uint32_t stop_at = 0xFFFFFFFFu;
    if constexpr (EARLY) {
        // the larger of the read's two thresholds for this filter (a negative int16 threshold arrives as 65 5xx: never reached, as in K2),
        // and at least one hit (a threshold of 0 is met by every read, but "classified" also needs a count above 0)
        const uint32_t tl = len < early.thr_len ? len : early.thr_len - 1;
        const uint16_t *t = early.thr + ((size_t)tl * early.nf + early.fi[blockIdx.y]) * 2;
        stop_at = max(max((uint32_t)t[0], (uint32_t)t[1]), 1u);
    }
    // bound pruning (see count_strand): on when asked for and no counter can wrap
    const bool bound = (prune.flags & kPruneBound) && n < (1u << NP);
    const bool sub = LEADS && bound && (prune.flags & kPruneSubTile);
    const bool leads = LEADS && bound && (prune.flags & kPruneLead) && n > TILE;
    const bool cert = leads && (prune.flags & kPruneCert);
    // passes (all wave-uniform): without the lead 0 = forward, 1 = reverse, each whole; with it 0 / 1 = the probes, 2 = the leader
    // from k-mer 64, 3 = the other strand from k-mer 64
    const int n_pass = leads ? 4 : 2;
    uint32_t best = 0, probe0 = 0, lead = 0, cert_bits = 0;  // (probe0: the forward probe's maximum, then the trailing strand's)
    uint32_t stops = 0;  // per strand, 16 bits each: where its gathers ended (the trace)
    // A pass of a lead build is one to three calls (all wave-uniform), `stage` says which is next: 0 = the pass begins; 1 = the leader's
    // line is counted, the other lanes are due; 2 = a certificate has failed, the lanes it covered are counted in full
    const bool lead_line = cert && (prune.flags & kPruneLeadLine);
    uint32_t stage = 0, lead_probe = 0, line_bits = 0;
    uint64_t line = 0;  // the lanes of the leader's line
    Planes<NP> pl[WPL];
    if constexpr (!LEADS) {
        // (the builds without the lead keep the loop they had word for word -- `leads` is false in them -- and their code with it: any other
        // wording of these two passes, or one loop shared with the lead builds, changed their instructions; profiles/isa_identity.py)
#pragma unroll 1
        for (int pass = 0; pass < n_pass; ++pass) {
            const bool probe = leads && pass < 2;
            const int strand = (!leads || pass < 2) ? pass : (int)(lead ^ (uint32_t)(pass & 1));
            // a strand counts at most n per bin: once the first strand's maximum has reached n the second cannot exceed it
            if (bound && (pass & 1) && !probe && best >= n) break;  // wave-uniform
            if (!leads || pass < 2) {
#pragma unroll
                for (int w = 0; w < WPL; ++w) pl[w].clear();
            }
            uint32_t stopped = 0;
            const bool left = count_strand<LG, WPL, NP, H, NT, false, EARLY>(pl, f, lc, seq, len, n, strand, leads && pass >= 2 ? TILE : 0u, TILE, 0,
                                                                             TileShape<LG>::STEPS / 8, s_stage[wave], lane, PhaseCfg{0, 0, 0, 0, 0}, stop_at,
                                                                             !bound || probe ? kNoBound : best,
                                                                             probe ? TILE : 0xFFFFFFFFu, sub, &stopped);
            stops = strand == 0 ? (stops & 0xFFFF0000u) | (stopped & 0xFFFFu) : (stops & 0xFFFFu) | (stopped << 16);
            const uint32_t m = planes_max<NP, WPL>(pl, lc.valid);
            if (!probe) best = m > best ? m : best;
            if (EARLY && left) break;  // wave-uniform
        }
    } else {
#pragma unroll 1
        for (int pass = 0; pass < n_pass;) {
            const bool probe = leads && pass < 2;
            const int strand = (!leads || pass < 2) ? pass : (int)(lead ^ (uint32_t)(pass & 1));
            if (stage == 0) {
                // a strand counts at most n per bin: once the first strand's maximum has reached n the second cannot exceed it
                if (bound && (pass & 1) && !probe && best >= n) break;  // wave-uniform
                if constexpr (LEADS) {
                    if (leads && pass == 1) {  // the forward probe waits in LDS
#pragma unroll
                        for (int w = 0; w < WPL; ++w)
#pragma unroll
                            for (int i = 0; i < kParkPlanes; ++i) s_park[wave][w * kParkPlanes + i][lane] = pl[w].p[i];
                    }
                }
                if (!leads || pass < 2) {
#pragma unroll
                    for (int w = 0; w < WPL; ++w) pl[w].clear();
                }
            }
            uint64_t lanes = ~0ULL;                          // the lanes this call gathers for
            uint32_t from = leads && pass >= 2 ? TILE : 0u;  // ... from this k-mer
            bool one_hash = false;                           // ... as a certificate: hash 0 alone, left the moment a counter passes `best`
            bool more = false;                               // ... and the pass goes on behind it
            if constexpr (LEADS) {
                // the certificate's rule: worth a third of the lines when the maximum in hand clears the probe maximum of the bins in question plus
                // the hash-0 hits a bin of load d (the filter's fullest) is expected to add over the rest, z sigma up (cert_c = z sqrt(d (1 - d))).
                // The rule only picks the attempts; a failed one costs lines, never a result.
                const float rem = (float)(n - TILE);
                const float allowance = prune.cert_d * rem + prune.cert_c * __builtin_sqrtf(rem);
                if (leads && pass == 3) {  // the other strand's probe comes back (its planes above 6 are zero): at first, and after a failed certificate
#pragma unroll
                    for (int w = 0; w < WPL; ++w) {
                        pl[w].clear();
#pragma unroll
                        for (int i = 0; i < kParkPlanes; ++i) pl[w].p[i] = s_park[wave][w * kParkPlanes + i][lane];
                    }
                    if (stage == 0 && cert && (float)(best - min(best, probe0)) >= allowance) {
                        cert_bits = 1u;
                        one_hash = true;
                    }
                }
                // LEAD LINE (kPruneLeadLine): the leader is counted with all hashes on all lines until its own maximum has outgrown the k-mers left, and
                // nearly all of that goes to bins that only have to be shown to stay at or below that maximum.  The maximum is one bin's count, and
                // a bin lies in one 128-byte line of every block.  So the lanes of the line that holds the probe's best bin are counted first, alone:
                // H lines per k-mer, after which they hold exact totals and `best` is a count some bin truly reaches.  The other lanes kept their
                // probe counters and are then certified against it from hash 0 like a trailing strand (for every one of their bins, probe count +
                // hash-0 hits >= true count; if none passes `best` the strand's maximum is `best`), or, where the rule does not promise that, counted
                // in full from k-mer 64 against `best`.  After a failed certificate their counters are upper bounds: they are cleared and counted from
                // k-mer 0.  If the strand's best bin lies in another line, that is where it is found.  `lead_min` keeps reads without a match out of
                // the second walk over the read; like the rule it picks attempts and changes no result.
                if (leads && pass == 2 && lead_line) {
                    constexpr int LL = 16 / WPL;  // lanes whose columns share 128 bytes of a block
                    uint64_t others[WPL];
#pragma unroll
                    for (int w = 0; w < WPL; ++w) others[w] = ((line >> lane) & 1ULL) ? 0ULL : lc.valid[w];
                    if (stage == 0) {
                        if (lead_probe >= ((prune.flags >> kPruneLeadMinShift) & 0xFFu)) {
                            // lowest lane that holds the probe's maximum
                            const bool holds = lead_probe ? bound_alive<NP, WPL>(pl, lc.valid, lead_probe - 1u) : lc.colok;
                            const uint64_t b = __ballot(holds);
                            if (b != 0ULL) {
                                line = ((1ULL << LL) - 1ULL) << ((uint32_t)__builtin_ctzll(b) & ~(uint32_t)(LL - 1));
                                lanes = line;
                                more = true;
                                line_bits = 1u;
                            }
                        }
                    } else {
                        lanes = ~line;
                        if (stage == 1) {
                            const uint32_t theirs = planes_max<NP, WPL>(pl, others);
                            if ((float)(best - min(best, theirs)) >= allowance) {
                                line_bits |= 2u;
                                one_hash = true;
                            }
                        } else {  // what the failed certificate left in the other lanes is no count
                            from = 0u;
#pragma unroll
                            for (int w = 0; w < WPL; ++w)
#pragma unroll
                                for (int i = 0; i < NP; ++i) pl[w].p[i] = ((line >> lane) & 1ULL) ? pl[w].p[i] : 0ULL;
                        }
                    }
                }
                if (one_hash) {
                    const bool over = count_strand<LG, WPL, NP, 1, NT, false, true>(pl, f, lc, seq, len, n, strand, TILE, TILE, 0, TileShape<LG>::STEPS / 8,
                                                                                    s_stage[wave], lane, PhaseCfg{0, 0, 0, 0, 0}, best + 1u, best,
                                                                                    0xFFFFFFFFu, sub, nullptr, lanes);
                    if (!over && planes_max<NP, WPL>(pl, lc.valid) <= best) {  // wave-uniform: held
                        if (pass == 3) {
                            cert_bits = 3u;
                            break;
                        }
                        line_bits |= 4u;
                        pass = 3;
                        stage = 0;
                    } else {
                        stage = 2;
                    }
                    continue;
                }
            }
            uint32_t stopped = 0;
            const bool left = count_strand<LG, WPL, NP, H, NT, false, EARLY>(pl, f, lc, seq, len, n, strand, from, TILE, 0,
                                                                             TileShape<LG>::STEPS / 8, s_stage[wave], lane, PhaseCfg{0, 0, 0, 0, 0}, stop_at,
                                                                             !bound || probe ? kNoBound : best,
                                                                             probe ? TILE : 0xFFFFFFFFu, sub, &stopped, lanes);
            stops = strand == 0 ? (stops & 0xFFFF0000u) | (stopped & 0xFFFFu) : (stops & 0xFFFFu) | (stopped << 16);
            const uint32_t m = planes_max<NP, WPL>(pl, lc.valid);
            if (!probe) best = m > best ? m : best;
            if constexpr (LEADS) {
                if (leads && pass == 0) probe0 = m;
                if (leads && pass == 1) {
                    lead = m > probe0 ? 1u : 0u;  // a tie: forward
                    lead_probe = max(m, probe0);  // the leader's probe maximum
                    probe0 = min(m, probe0);      // the trailing strand's probe maximum
                    if (lead == 0) {  // the registers hold the reverse probe: change places with the forward one
#pragma unroll
                        for (int w = 0; w < WPL; ++w)
#pragma unroll
                            for (int i = 0; i < kParkPlanes; ++i) {
                                const uint64_t t = s_park[wave][w * kParkPlanes + i][lane];
                                s_park[wave][w * kParkPlanes + i][lane] = pl[w].p[i];
                                pl[w].p[i] = t;
                            }
                    }
                }
            }
            if (EARLY && left) break;  // wave-uniform
            stage = more ? 1u : 0u;
            if (!more) ++pass;
        }
    }
    if (lane == 0) out[(size_t)read * out_read_stride + (size_t)slice * out_slice_stride] = (uint16_t)best;
    if (prune.trace) {  // (one scalar branch when there is none)
        if (lane == 0)
            prune.trace[(size_t)blockIdx.y * n_reads * n_slices + item] =
                prune_trace_record(lead, leads, cert_bits, stops & 0xFFFFu, stops >> 16, line_bits);
    }
}

// ROW FORM of the kernel above (rb_dibf_row_table_build, rb_engine_set_row_table): for a resident filter the AND of a k-mer's h blocks is a
// function of the k-mer alone, and at k <= 13 there are at most 4^13 k-mers without an N.  `rows` holds that AND for each of them (row =
// base-4 rank), so a strand costs one gather per k-mer instead of h, and hash 0 alone being the whole count, nothing is left to certify:
// the bound, the sub-tile checks, the strand lead and the parked probe stay, the certificate and the lead line fall away.  A k-mer with an
// N hashes to real blocks and can count, but has no row: a read with any base outside ACGT takes the same passes with the three-hash
// gathers on the filter's own table.  The two kinds of read have a build each, ROWS and !ROWS, launched one behind the other over the
// whole batch: a wave looks over its read's bases first and leaves at once when the read is the other build's (wave-uniform), so every
// item is written by exactly one of them, no item list is made, and the row build carries neither the three-hash gather schedule nor its
// registers (one build with a branch between the two spilt at sixteen planes).  Every form of pruning is exact, so either way the result
// is the maximum the kernel above writes.  Blocks of a whole wave, three compile-time hash functions.
template <int WPL, int NP, bool NT, bool ROWS>
__global__ __launch_bounds__(64 * kWavesPerBlock) __attribute__((amdgpu_waves_per_eu(3, 8))) void ibf_count_rows_kernel(
    IbfDev f, const uint64_t *__restrict__ rows, uint32_t col_begin, uint32_t col_end, ReadSrc src, uint32_t n_reads, uint32_t n_slices,
    uint16_t *__restrict__ out, uint32_t out_read_stride, uint32_t out_slice_stride, PruneCfg prune)
{
    constexpr int LG = 6;
    constexpr uint32_t TILE = (uint32_t)TileShape<LG>::ITEMS;
    __shared__ uint8_t s_stage[kWavesPerBlock][kStageBytes];
    __shared__ uint64_t s_park[kWavesPerBlock][kParkPlanes * WPL][64];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint64_t item = (uint64_t)blockIdx.x * kWavesPerBlock + wave;
    const uint32_t read = (uint32_t)(item / n_slices);
    const uint32_t slice = (uint32_t)(item - (uint64_t)read * n_slices);
    if (read >= n_reads) return;  // wave-uniform; there are no block-level barriers below

    uint32_t len;
    const BaseSrc seq = make_base_src(src, read, &len);
    const uint32_t n = len >= f.k ? len - f.k + 1 : 0;
    bool outside = false;
    for (uint32_t i = lane; i < len; i += 64) outside |= seq.ord(i) > 3u;
    if ((__ballot(outside) != 0ULL) == ROWS) return;  // wave-uniform: the other build's read

    LaneCols<WPL> lc = make_lane_cols<LG, WPL>(f, lane, col_begin, col_end, slice);
    if constexpr (ROWS) {  // the same columns of the row table
        lc.lane_base = rows + (lc.lane_base - f.words);
        lc.safe_base = rows + (lc.safe_base - f.words);
    }

    const bool bound = (prune.flags & kPruneBound) && n < (1u << NP);
    const bool sub = bound && (prune.flags & kPruneSubTile);
    const bool leads = bound && (prune.flags & kPruneLead) && n > TILE;
    // passes (all wave-uniform), as in the kernel above: without the lead 0 = forward, 1 = reverse, each whole; with it 0 / 1 = the probes,
    // 2 = the leader from k-mer 64, 3 = the other strand from k-mer 64
    const int n_pass = leads ? 4 : 2;
    uint32_t best = 0, probe0 = 0, lead = 0, stops = 0;
    Planes<NP> pl[WPL];
#pragma unroll 1
    for (int pass = 0; pass < n_pass; ++pass) {
        const bool probe = leads && pass < 2;
        const int strand = (!leads || pass < 2) ? pass : (int)(lead ^ (uint32_t)(pass & 1));
        if (bound && (pass & 1) && !probe && best >= n) break;  // wave-uniform
        if (leads && pass == 1) {  // the forward probe waits in LDS
#pragma unroll
            for (int w = 0; w < WPL; ++w)
#pragma unroll
                for (int i = 0; i < kParkPlanes; ++i) s_park[wave][w * kParkPlanes + i][lane] = pl[w].p[i];
        }
        if (!leads || pass < 2 || pass == 3) {
#pragma unroll
            for (int w = 0; w < WPL; ++w) pl[w].clear();
        }
        if (leads && pass == 3) {  // the other strand's probe comes back (its planes above 6 are zero)
#pragma unroll
            for (int w = 0; w < WPL; ++w)
#pragma unroll
                for (int i = 0; i < kParkPlanes; ++i) pl[w].p[i] = s_park[wave][w * kParkPlanes + i][lane];
        }
        const uint32_t from = leads && pass >= 2 ? TILE : 0u;
        const uint32_t against = !bound || probe ? kNoBound : best;
        const uint32_t upto = probe ? TILE : 0xFFFFFFFFu;
        uint32_t stopped = 0;
        if constexpr (!ROWS)
            count_strand<LG, WPL, NP, 3, NT>(pl, f, lc, seq, len, n, strand, from, TILE, 0, TileShape<LG>::STEPS / 8, s_stage[wave], lane,
                                             PhaseCfg{0, 0, 0, 0, 0}, 0xFFFFFFFFu, against, upto, sub, &stopped);
        else
            count_strand<LG, WPL, NP, 1, NT, false, false, 0, true>(pl, f, lc, seq, len, n, strand, from, TILE, 0, TileShape<LG>::STEPS / 8,
                                                                    s_stage[wave], lane, PhaseCfg{0, 0, 0, 0, 0}, 0xFFFFFFFFu, against, upto, sub,
                                                                    &stopped);
        stops = strand == 0 ? (stops & 0xFFFF0000u) | (stopped & 0xFFFFu) : (stops & 0xFFFFu) | (stopped << 16);
        const uint32_t m = planes_max<NP, WPL>(pl, lc.valid);
        if (!probe) best = m > best ? m : best;
        if (leads && pass == 0) probe0 = m;
        if (leads && pass == 1) {
            lead = m > probe0 ? 1u : 0u;  // a tie: forward
            if (lead == 0) {  // the registers hold the reverse probe: change places with the forward one
#pragma unroll
                for (int w = 0; w < WPL; ++w)
#pragma unroll
                    for (int i = 0; i < kParkPlanes; ++i) {
                        const uint64_t t = s_park[wave][w * kParkPlanes + i][lane];
                        s_park[wave][w * kParkPlanes + i][lane] = pl[w].p[i];
                        pl[w].p[i] = t;
                    }
            }
        }
    }
    if (lane == 0) out[(size_t)read * out_read_stride + (size_t)slice * out_slice_stride] = (uint16_t)best;
    if (prune.trace) {  // (one scalar branch when there is none)
        if (lane == 0) prune.trace[item] = prune_trace_record(lead, leads, 0u, stops & 0xFFFFu, stops >> 16, 0u);
    }
}

// The row table of a filter: one wave per row.  Row r belongs to the k-mer whose base-4 digits are r (A, C, G, T as Dna5 ordinals 0-3,
// the first base most significant); its base-5 value is formed as count_strand's phase A forms it, its block numbers are the filter's own,
// and the row is the AND of those blocks over the padded stride (pad words are zero in every block, so they are zero in every row).
__global__ __launch_bounds__(256) void ibf_row_table_kernel(IbfDev f, uint64_t *__restrict__ rows, uint64_t n_rows)
{
    const int lane = threadIdx.x & 63;
    const uint64_t waves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    const uint64_t S = f.stride;
    const uint32_t nh = f.n_hash < rbspec::kMaxHash ? f.n_hash : rbspec::kMaxHash;
    // (a grid of one wave per row would pass 2^32 threads at k = 13: the waves stride over the rows)
    for (uint64_t r = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6; r < n_rows; r += waves) {  // wave-uniform
        uint64_t v = 0;
        for (uint32_t i = 0; i < f.k; ++i) v = v * 5u + ((r >> (2u * (f.k - 1u - i))) & 3u);
        for (uint64_t w = (uint64_t)lane; w < S; w += 64) {
            uint64_t acc = ~0ULL;
            for (uint32_t h = 0; h < nh; ++h) {
                const uint32_t b = rbspec::block_index(v, f.precalc[h], f.n_blocks, f.magic, f.pow2_mask);
                acc &= f.words[(uint64_t)b * S + w];
            }
            rows[r * S + w] = acc;
        }
    }
}

// What the opt-in query passes (locate, hits, spans) share.
// The status of a work item: chunk_prep's verdict first, then the declared bound, then "shorter than the k of some filter of the engine"
// (decide_one's rules are richer and its own).
__device__ __forceinline__ uint32_t item_status(const uint8_t *pre_status, uint32_t item, uint32_t raw_len, uint32_t max_len, uint32_t min_len)
{
    const uint32_t pre = pre_status ? (uint32_t)pre_status[item] : (uint32_t)RB_OK;
    if (pre != RB_OK) return pre;
    if (raw_len > max_len) return RB_ERR_INVALID_ARG;
    if (raw_len < min_len) return RB_ERR_SHORT_READ;
    return RB_OK;
}

// Locate and hits run one wave per (work item, column slice), as the plain count kernel.  SCALAR: the pair is made wave-uniform in
// scalar registers, so that addresses made from it are scalar arithmetic and cost no vector register across the gathers (hits, for its
// segment addresses; locate has none, and its whole-wave ten-plane build takes 23 registers more that way).
template <bool SCALAR>
__device__ __forceinline__ void wave_item_slice(uint32_t n_slices, int wave, uint32_t *item, uint32_t *slice)
{
    const uint64_t witem = (uint64_t)blockIdx.x * kWavesPerBlock + wave;
    const uint32_t it = (uint32_t)(witem / n_slices);
    const uint32_t sl = (uint32_t)(witem - (uint64_t)it * n_slices);
    *item = SCALAR ? __builtin_amdgcn_readfirstlane(it) : it;
    *slice = SCALAR ? __builtin_amdgcn_readfirstlane(sl) : sl;
}

// ... and what such a wave sets up before it counts
template <int WPL>
struct PassWave {
    LaneCols<WPL> lc;
    BaseSrc seq;
    uint32_t len, n;  // bases and k-mers of the item
    uint32_t t;       // wave-uniform: the caller's threshold, or the one the decision kernel reads for this length and filter
    uint32_t col0;    // first word column of the slice
    bool group0;      // the lane group whose columns are reported (every group holds the same totals)
    // word column of word w of lane `c` of group 0
    __device__ __forceinline__ uint32_t word_col(int c, int w) const { return col0 + (uint32_t)(c * WPL + w); }
};
template <int LG, int WPL>
__device__ __forceinline__ PassWave<WPL> make_pass_wave(const IbfDev &f, const ReadSrc &src, uint32_t col_begin, uint32_t col_end, uint32_t item,
                                                            uint32_t slice, int lane, const uint16_t *thr, uint32_t thr_len, uint32_t nf, uint32_t fi,
                                                            uint32_t min_count)
{
    PassWave<WPL> pw;
    pw.lc = make_lane_cols<LG, WPL>(f, lane, col_begin, col_end, slice);
    pw.seq = make_base_src(src, item, &pw.len);
    pw.n = pw.len >= f.k ? pw.len - f.k + 1 : 0;
    const uint32_t tl = pw.len < thr_len ? pw.len : thr_len - 1;
    pw.t = min_count ? min_count : __builtin_amdgcn_readfirstlane((uint32_t)thr[((size_t)tl * nf + fi) * 2]);
    pw.col0 = col_begin + slice * (uint32_t)((1 << LG) * WPL);
    pw.group0 = lane < (1 << LG);
    return pw;
}

// LOCATE: the opt-in second pass (rb_locate_batch_device) that says WHERE a read matched.  One wave per (work item, column slice) as
// in the plain kernel above and built from the same pieces -- make_lane_cols, make_base_src, count_strand with no bound, no early
// exit, no phasing -- so the gather schedule is the measured one; it always counts in full (bound pruning leaves stale counters in
// dead bins, and a dead bin may still TIE the maximum, so "the first bin at M" does not exist there).  What is new happens after a
// strand's counters are complete (lanes < 2^LG hold whole counts of their columns: count_strand's closing butterfly):
//   * M_s, MSB plane first as planes_max, but the candidate mask is kept: its lowest (word column, bit) over the wave is the lowest
//     bin at M_s (one ballot for the lowest lane that has a candidate, ffs there);
//   * a bit-sliced c >= t against the wave-uniform uint16_t threshold t of the decision kernel's table (the compare of the pruning
//     code, one scalar branch per plane); the hit mask is ORed over the two strands -- the only per-lane state that lives across them.
// The strands combine by the rule "lowest bin b with max(fwd[b], rev[b]) == M, forward wins a tie in that bin": M = max(M_0, M_1);
// the strand that reaches M alone gives bin and strand; when both do, the lower first bin wins and strand 0 takes an equal bin.
// A slice writes one partial record; reduce_locate_slices_kernel merges the slices of a filter and applies the per-item status.
template <int LG, int WPL, int NP, int H, bool NT>
__global__ __launch_bounds__(64 * kWavesPerBlock) __attribute__((amdgpu_waves_per_eu(3, 8))) void ibf_locate_kernel(
    IbfDev f, uint32_t col_begin, uint32_t col_end, ReadSrc src, uint32_t n_items, uint32_t n_slices, const uint16_t *__restrict__ thr,
    uint32_t thr_len, uint32_t nf, uint32_t fi, LocatePart *__restrict__ part)
{
    __shared__ uint8_t s_stage[kWavesPerBlock][kStageBytes];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    uint32_t item, slice;
    wave_item_slice<false>(n_slices, wave, &item, &slice);
    if (item >= n_items) return;  // wave-uniform; there are no block-level barriers below

    // t: the threshold the decision kernel reads for this length and filter, at the caller's error rate
    const PassWave<WPL> pw = make_pass_wave<LG, WPL>(f, src, col_begin, col_end, item, slice, lane, thr, thr_len, nf, fi, 0u);
    const LaneCols<WPL> &lc = pw.lc;
    const uint32_t t = pw.t;

    uint64_t hit[WPL];
#pragma unroll
    for (int w = 0; w < WPL; ++w) hit[w] = (t == 0) ? lc.valid[w] : 0ULL;
    uint32_t best = 0, best_bin = 0, best_strand = 0;
    for (int strand = 0; strand < 2; ++strand) {
        Planes<NP> pl[WPL];
#pragma unroll
        for (int w = 0; w < WPL; ++w) pl[w].clear();
        count_strand<LG, WPL, NP, H, NT>(pl, f, lc, pw.seq, pw.len, pw.n, strand, 0u, (uint32_t)TileShape<LG>::ITEMS, 0, TileShape<LG>::STEPS / 8,
                                         s_stage[wave], lane);
        // ---- the strand's maximum, and the bins that hold it
        uint64_t cand[WPL];
#pragma unroll
        for (int w = 0; w < WPL; ++w) cand[w] = lc.valid[w];
        uint32_t m = 0;
#pragma unroll
        for (int i = NP - 1; i >= 0; --i) {
            uint64_t c[WPL];
            bool any = false;
#pragma unroll
            for (int w = 0; w < WPL; ++w) {
                c[w] = cand[w] & pl[w].p[i];
                any |= (c[w] != 0);
            }
            if (__ballot(any) != 0ULL) {  // wave-uniform
                m |= 1u << i;
#pragma unroll
                for (int w = 0; w < WPL; ++w) cand[w] = c[w];
            }
        }
        if (m > 0) {  // wave-uniform
            bool has = false;
            uint32_t mine = 0;  // lowest candidate bin of this lane
#pragma unroll
            for (int w = WPL - 1; w >= 0; --w) {
                if (cand[w] != 0ULL) {
                    has = true;
                    mine = pw.word_col(lane & ((1 << LG) - 1), w) * 64u + (uint32_t)(__ffsll((unsigned long long)cand[w]) - 1);
                }
            }
            // columns rise with the lane number inside a group: the lowest lane of group 0 with a candidate holds the lowest bin
            const uint64_t who = __ballot(has && pw.group0);
            const uint32_t first = readlane32(mine, (int)__builtin_amdgcn_readfirstlane((uint32_t)(__ffsll((unsigned long long)who) - 1)));
            if (m > best || (m == best && first < best_bin)) {  // (strand 0 enters through m > 0 == best; an equal bin stays with strand 0)
                best_bin = first;
                best_strand = (uint32_t)strand;
            }
            best = m > best ? m : best;
        }
        // ---- bins with c >= t, i.e. c > t - 1 (t == 0: every bin, set above; t beyond what NP planes can hold: none)
        if (t > 0 && t <= (1u << NP) - 1u) {  // wave-uniform
            const uint32_t tt = t - 1u;
#pragma unroll
            for (int w = 0; w < WPL; ++w) {
                uint64_t gt = 0, eq = lc.valid[w];
#pragma unroll
                for (int i = NP - 1; i >= 0; --i) {
                    if ((tt >> i) & 1u) {  // scalar branch
                        eq &= pl[w].p[i];
                    } else {
                        gt |= eq & pl[w].p[i];
                        eq &= ~pl[w].p[i];
                    }
                }
                hit[w] |= gt;
            }
        }
    }
    uint32_t hits = 0;
#pragma unroll
    for (int w = 0; w < WPL; ++w) hits += (uint32_t)__popcll(hit[w]);
    if (!pw.group0) hits = 0;
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) hits += shfl32(hits, lane ^ s);
    if (lane == 0) {
        rb_u32x4 rec;
        rec.x = best;
        rec.y = best_bin;
        rec.z = best_strand;
        rec.w = hits;
        *reinterpret_cast<rb_u32x4 *>(part + ((size_t)slice * n_items + item)) = rec;
    }
}

// Merge the column slices of one filter (slices hold rising bins: on equal maxima the earlier slice has the lower bin) and write the
// outputs the caller asked for.  An item whose status is not RB_OK reports nothing: -1 / 0.  status[] itself is written by the call for
// filter 0.  One thread per work item.
__global__ void reduce_locate_slices_kernel(const LocatePart *__restrict__ part, uint32_t n_slices, uint32_t n_items,
                                            const uint32_t *__restrict__ lens, const uint8_t *__restrict__ pre_status, uint32_t max_len,
                                            uint32_t min_len, LocateOut out, uint32_t nf, uint32_t fidx)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_items) return;
    const uint8_t status = (uint8_t)item_status(pre_status, i, lens[i], max_len, min_len);
    uint32_t m = 0, bin = 0, strand = 0, hits = 0;
    if (status == RB_OK) {
        for (uint32_t s = 0; s < n_slices; ++s) {
            const LocatePart p = part[(size_t)s * n_items + i];
            if (p.max_count > m || (p.max_count == m && m > 0 && p.first_bin < bin)) {
                // (an equal bin cannot come from two slices: the second condition only guards the order of the slices)
                m = p.max_count;
                bin = p.first_bin;
                strand = p.strand;
            }
            hits += p.hit_bins;
        }
    }
    const size_t o = (size_t)i * nf + fidx;
    if (out.max_count) out.max_count[o] = (uint16_t)m;
    if (out.best_bin) out.best_bin[o] = m > 0 ? (int32_t)bin : -1;
    if (out.best_strand) out.best_strand[o] = m > 0 ? (uint8_t)strand : (uint8_t)0;
    if (out.hit_bins) out.hit_bins[o] = hits;
    if (out.status && fidx == 0) out.status[i] = status;
}

// PREFIXES: the opt-in pass (rb_prefix_batch_device) that gives a work item's maximum at every prefix checkpoint in ONE walk over its
// k-mers.  seqan::count adds one per k-mer, so the counters after the k-mers of a prefix ARE the counts of that prefix -- on both
// strands: the reverse complement of a prefix consists of the reverse complements of the prefix's own windows, and count_strand counts
// strand 1 window by window in the read's direction.  One wave per (work item, column slice) behind locate's prologue; per strand the
// planes are cleared once and checkpoint p is one count_strand call over the k-mers [n_{p-1}, n_p) of the prefix of L_p = min(c_p, len)
// bases, with no bound, no early exit and no phasing, followed by planes_max.  A checkpoint that adds no k-mer (below k, at or beyond
// the item's end, n_p == n_{p-1}) gathers nothing and repeats the maximum.
// THE BUTTERFLY RULE: count_strand ends by summing the partial counters of the NG lane groups (LG < 6), after which every group holds
// the totals.  A second call on those planes would add totals onto totals, so before every further call the planes of the lanes
// outside group 0 are cleared: the next butterfly then sums group 0's running totals with the other groups' new partials.
// Checkpoint p's running maximum over the two strands lives in lane p's one register -- the only state alive across strands; lanes
// below P of the wave write part[slice][item][0..P) coalesced.  finish_prefix_kernel merges the slices of a filter.
template <int LG, int WPL, int NP, int H, bool NT>
__global__ __launch_bounds__(64 * kWavesPerBlock) __attribute__((amdgpu_waves_per_eu(3, 8))) void ibf_prefix_kernel(
    IbfDev f, uint32_t col_begin, uint32_t col_end, ReadSrc src, uint32_t n_items, uint32_t n_slices, const uint16_t *__restrict__ thr,
    uint32_t thr_len, uint32_t nf, uint32_t fi, PrefixList cps, uint16_t *__restrict__ part)
{
    __shared__ uint8_t s_stage[kWavesPerBlock][kStageBytes];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    uint32_t item, slice;
    wave_item_slice<false>(n_slices, wave, &item, &slice);
    if (item >= n_items) return;  // wave-uniform; there are no block-level barriers below

    // (the threshold is the decision kernel's business here: a constant min_count keeps the prologue from reading the table)
    const PassWave<WPL> pw = make_pass_wave<LG, WPL>(f, src, col_begin, col_end, item, slice, lane, thr, thr_len, nf, fi, 1u);
    const LaneCols<WPL> &lc = pw.lc;
    const uint32_t len = __builtin_amdgcn_readfirstlane(pw.len);  // the checkpoint loop below is scalar
    const uint32_t k = f.k;

    uint32_t mine = 0;  // lane p: checkpoint p's maximum over the strands so far
    for (int strand = 0; strand < 2; ++strand) {
        Planes<NP> pl[WPL];
#pragma unroll
        for (int w = 0; w < WPL; ++w) pl[w].clear();
        uint32_t n_prev = 0, m = 0;
#pragma unroll 1
        for (uint32_t p = 0; p < cps.n; ++p) {
            const uint32_t L = min(cps.c[p], len);
            const uint32_t n = L >= k ? L - k + 1 : 0;
            if (n > n_prev) {  // wave-uniform
                if constexpr (LG < 6) {
                    if (!pw.group0) {  // the butterfly rule (nothing to clear before a strand's first call)
#pragma unroll
                        for (int w = 0; w < WPL; ++w) pl[w].clear();
                    }
                }
                count_strand<LG, WPL, NP, H, NT, false, false, 1>(pl, f, lc, pw.seq, L, n, strand, n_prev, (uint32_t)TileShape<LG>::ITEMS, 0,
                                                                  TileShape<LG>::STEPS / 8, s_stage[wave], lane);
                m = planes_max<NP, WPL>(pl, lc.valid);
                n_prev = n;
            }
            if ((uint32_t)lane == p) mine = max(mine, m);
        }
    }
    if ((uint32_t)lane < cps.n) part[((size_t)slice * n_items + item) * cps.n + (uint32_t)lane] = (uint16_t)mine;
}

// Merge the column slices of one filter into max_count[item][p][filter]; the call for filter 0 also writes the bases each row stands
// for and the row's pre-status (chunk_prep's verdict for the item, replicated), which is what the decision kernel then reads as `lens`
// and `pre_status` over the n_items x P rows.  One thread per (item, checkpoint).
__global__ void finish_prefix_kernel(const uint16_t *__restrict__ part, uint32_t n_slices, uint32_t n_items, PrefixList cps,
                                     const uint32_t *__restrict__ lens, const uint8_t *__restrict__ pre_status, uint16_t *__restrict__ max_count,
                                     uint32_t *__restrict__ prefix_len, uint8_t *__restrict__ row_pre, uint32_t nf, uint32_t fidx)
{
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_items * cps.n) return;
    const uint32_t i = r / cps.n, p = r - i * cps.n;
    uint16_t m = 0;
    for (uint32_t s = 0; s < n_slices; ++s) {
        const uint16_t v = part[((size_t)s * n_items + i) * cps.n + p];
        m = v > m ? v : m;
    }
    max_count[(size_t)r * nf + fidx] = m;
    if (fidx == 0) {
        prefix_len[r] = min(cps.c[p], lens[i]);
        row_pre[r] = pre_status ? pre_status[i] : (uint8_t)RB_OK;
    }
}

// first_decided[item] = the lowest checkpoint whose row is RB_OK with a decision other than 0; P when there is none.  One thread per item.
__global__ void first_decided_kernel(const uint8_t *__restrict__ decision, const uint8_t *__restrict__ status, uint32_t n_items, uint32_t n_prefixes,
                                     uint32_t *__restrict__ first_decided)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_items) return;
    uint32_t p = 0;
    while (p < n_prefixes && !(status[(size_t)i * n_prefixes + p] == RB_OK && decision[(size_t)i * n_prefixes + p] != 0)) ++p;
    first_decided[i] = p;
}

// RESUME: the opt-in pass (rb_resume_batch_device) that counts only the NEW k-mers of a read onto per-bin counters kept in HBM between
// calls.  seqan::count adds one per k-mer, on both strands window by window (the prefix pass's argument above), so the counters of a
// grown prefix are the counters of the shorter one plus one per new window, and the new windows are the k-mers of "the last k - 1 bases
// seen so far + the new chunk" -- the stitched item resume_prep_kernel wrote.  One wave per (work item, column slice) behind locate's
// prologue; per strand group 0's lanes load the slot's sixteen planes of their columns (a FIRST item: nothing), the other lane groups
// start from cleared planes -- THE BUTTERFLY RULE of the prefix pass: count_strand's closing butterfly sums the groups, and totals must
// never be added onto totals --, count_strand runs over the stitched item with no bound, no early exit and no phasing, planes_max gives
// the slice's maximum, and group 0 stores the planes back (a PEEK item: nothing).  Sixteen planes only: the counters wrap at 2^16 as the
// reference's do, whatever the read's length.  The state is streamed -- read once and written once per call, non-temporal both ways.
// A plane of a slice is one contiguous run of the state (ResumeSlots), every (item, slice) wave touches its own columns only: no
// atomics, no cross-wave order.  A refused item (kResumeSkip) touches no slot at all.
template <int LG, int WPL, int NP, int H, bool NT>
__global__ __launch_bounds__(64 * kWavesPerBlock) __attribute__((amdgpu_waves_per_eu(3, 8))) void ibf_resume_kernel(
    IbfDev f, uint32_t col_begin, uint32_t col_end, ReadSrc src, uint32_t n_items, uint32_t n_slices, const uint16_t *__restrict__ thr,
    uint32_t thr_len, uint32_t nf, uint32_t fi, ResumeSlots rs, uint16_t *__restrict__ part)
{
    static_assert(NP == (int)kResumePlanes, "the state holds sixteen planes");
    __shared__ uint8_t s_stage[kWavesPerBlock][kStageBytes];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    uint32_t item, slice;
    wave_item_slice<false>(n_slices, wave, &item, &slice);
    if (item >= n_items) return;  // wave-uniform; there are no block-level barriers below

    const uint32_t ctl = __builtin_amdgcn_readfirstlane((uint32_t)rs.ctl[item]);
    if (ctl & kResumeSkip) {  // wave-uniform: the slot number was never vetted, no address is formed from it
        if (lane == 0) part[(size_t)slice * n_items + item] = 0;
        return;
    }
    // (the threshold is the decision kernel's business: a constant min_count keeps the prologue from reading the table)
    const PassWave<WPL> pw = make_pass_wave<LG, WPL>(f, src, col_begin, col_end, item, slice, lane, thr, thr_len, nf, fi, 1u);
    const LaneCols<WPL> &lc = pw.lc;
    // This lane's columns of the slot and strand: group 0's lanes cover the slice's 2^LG * WPL padded columns side by side.  The address
    // is formed where it is used, from an opaque copy of the lane number: kept across count_strand it costs the two registers that
    // separate the h = 3 build for blocks of eight lanes from locate's four waves per SIMD.
    // (by value: `lane` captured by reference would reach the prologue through memory, and what the compiler knows about the lane
    // number in make_lane_cols is shared with every kernel that calls it -- profiles/isa_identity.py)
    const uint32_t slot = __builtin_amdgcn_readfirstlane(rs.slot[item]);
    auto strand_planes = [rs, slot, slice, lane](int strand) -> uint64_t * {
        uint32_t l = (uint32_t)lane;
        asm volatile("" : "+v"(l));
        return rs.state + (uint64_t)slot * rs.slot_words + rs.filter_off + (uint64_t)(strand * NP) * rs.pad_cols +
               (uint64_t)slice * (uint32_t)((1 << LG) * WPL) + (l & (uint32_t)((1 << LG) - 1)) * (uint32_t)WPL;
    };
    const bool loads = pw.group0 && !(ctl & kResumeFirst), stores = pw.group0 && !(ctl & kResumePeek);

    uint32_t best = 0;
    for (int strand = 0; strand < 2; ++strand) {
        Planes<NP> pl[WPL];
#pragma unroll
        for (int w = 0; w < WPL; ++w) pl[w].clear();
        if (loads) {
            const uint64_t *sp = strand_planes(strand);
#pragma unroll
            for (int i = 0; i < NP; ++i)
#pragma unroll
                for (int w = 0; w < WPL; ++w) pl[w].p[i] = __builtin_nontemporal_load(sp + (uint64_t)i * rs.pad_cols + w);
        }
        count_strand<LG, WPL, NP, H, NT, false, false, 2>(pl, f, lc, pw.seq, pw.len, pw.n, strand, 0u, (uint32_t)TileShape<LG>::ITEMS, 0,
                                                          TileShape<LG>::STEPS / 8, s_stage[wave], lane);
        const uint32_t m = planes_max<NP, WPL>(pl, lc.valid);
        best = m > best ? m : best;
        if (stores) {
            uint64_t *sp = strand_planes(strand);
#pragma unroll
            for (int i = 0; i < NP; ++i)
#pragma unroll
                for (int w = 0; w < WPL; ++w) __builtin_nontemporal_store(pl[w].p[i], sp + (uint64_t)i * rs.pad_cols + w);
        }
    }
    if (lane == 0) part[(size_t)slice * n_items + item] = (uint16_t)best;
}

// Before the pass: one wave per item.  Vets the item ON THE DEVICE -- no slot number forms an address before it is checked --, applies
// the descriptor's chunking as chunk_prep_kernel does, and writes the stitched string "tail + chunk" as ASCII where the pass reads it
// through the ordinary ReadSrc.  The chunk is read through BaseSrc::ord, so ASCII and packed input, chunk_start / chunk_length and
// d_read_ids work as in every descriptor call.  A refused item (slot >= n_slots, chunk longer than max_chunk_len, total beyond
// max_total_len: RB_ERR_INVALID_ARG; chunk_start beyond the read: RB_ERR_BAD_CHUNK) is an empty string with kResumeSkip.
// (a Dna5 ordinal as the ASCII letter dna5_ord reads back as that ordinal; arithmetic, not a string constant of the module)
__device__ __forceinline__ uint8_t dna5_ascii(uint32_t o)
{
    constexpr uint32_t kAcgt = (uint32_t)'A' | ((uint32_t)'C' << 8) | ((uint32_t)'G' << 16) | ((uint32_t)'T' << 24);
    return o < 4u ? (uint8_t)((kAcgt >> (8u * o)) & 0xFFu) : (uint8_t)'N';
}
__global__ __launch_bounds__(64 * kWavesPerBlock) void resume_prep_kernel(ResumePrep a)
{
    const int lane = threadIdx.x & 63;
    const uint32_t i = blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
    if (i >= a.n_items) return;
    const uint32_t rid = a.src.ids ? a.src.ids[i] : i;
    const uint32_t len = a.src.lens[rid];
    const bool bad_chunk = a.src.base_off > len;
    const uint32_t rest = bad_chunk ? 0u : len - a.src.base_off;
    const uint32_t chunk = (a.chunk_length && a.chunk_length < rest) ? a.chunk_length : rest;
    const uint32_t slot = a.slot[i];
    const uint32_t flags = a.flags ? (uint32_t)a.flags[i] : 0u;
    uint32_t status = bad_chunk ? (uint32_t)RB_ERR_BAD_CHUNK : (uint32_t)RB_OK;
    uint32_t old_total = 0, tail_len = 0;
    const bool slot_ok = slot < a.n_slots;
    if (status == RB_OK && (!slot_ok || chunk > a.max_chunk_len)) status = RB_ERR_INVALID_ARG;
    if (status == RB_OK && !(flags & kResumeFirst)) {
        old_total = a.meta[slot].total;
        tail_len = min(a.meta[slot].tail_len, min(a.k - 1u, kResumeMaxTail));
    }
    if (status == RB_OK && (uint64_t)old_total + chunk > (uint64_t)a.max_total_len) status = RB_ERR_INVALID_ARG;
    const bool ok = status == RB_OK;
    uint8_t *dst = a.stitched + (uint64_t)i * a.stitch_stride;
    if (ok) {
        if ((uint32_t)lane < tail_len) dst[lane] = dna5_ascii(a.meta[slot].tail[lane]);
        BaseSrc b;
        if (a.src.nmask) {
            b.bytes = a.src.seqs + a.src.offsets[rid];
            b.nm = a.src.nmask + a.src.nmask_offsets[rid];
            b.first = a.src.base_off;
        } else {
            b.bytes = a.src.seqs + a.src.offsets[rid] + a.src.base_off;
            b.nm = nullptr;
            b.first = 0;
        }
        for (uint32_t p = (uint32_t)lane; p < chunk; p += 64) dst[tail_len + p] = dna5_ascii(b.ord(p));
    }
    if (lane == 0) {
        a.st_offsets[i] = (uint64_t)i * a.stitch_stride;
        a.st_lens[i] = ok ? tail_len + chunk : 0u;
        a.total_lens[i] = ok ? old_total + chunk : 0u;
        a.pre_status[i] = (uint8_t)status;
        a.ctl[i] = ok ? (uint8_t)(flags & (kResumeFirst | kResumePeek)) : (uint8_t)kResumeSkip;
        if (a.out_total_len) a.out_total_len[i] = ok ? old_total + chunk : 0u;
    }
}

// After the last filter's pass: the slot's new total and tail -- the last min(total, k - 1) bases of the stitched string, which is
// "everything so far" while the total is below k.  Not for a PEEK or a refused item.  One thread per item.
__global__ void resume_commit_kernel(ResumeMeta *__restrict__ meta, const uint32_t *__restrict__ slot, const uint8_t *__restrict__ ctl,
                                     const uint8_t *__restrict__ stitched, uint32_t stitch_stride, const uint32_t *__restrict__ st_lens,
                                     const uint32_t *__restrict__ total_lens, uint32_t n_items, uint32_t k)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_items) return;
    if (ctl[i] & (kResumeSkip | kResumePeek)) return;
    const uint32_t sl = st_lens[i];
    const uint32_t tl = min(sl, min(k - 1u, kResumeMaxTail));
    const uint8_t *src = stitched + (uint64_t)i * stitch_stride + (sl - tl);
    ResumeMeta m;
    m.total = total_lens[i];
    m.tail_len = tl;
    for (uint32_t j = 0; j <= kResumeMaxTail; ++j) m.tail[j] = j < tl ? (uint8_t)rbspec::dna5_ord(src[j]) : (uint8_t)0;
    meta[slot[i]] = m;
}

// rb_resume_counts: the bit-sliced planes of one slot and filter as the two uint16_t count vectors of seqan::count.  One thread per
// (strand, bin).
__global__ void resume_counts_kernel(const uint64_t *__restrict__ planes, uint32_t pad_cols, uint32_t n_bins, uint16_t *__restrict__ counts)
{
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= 2u * n_bins) return;
    const uint32_t strand = t / n_bins, bin = t - strand * n_bins;
    const uint64_t *p = planes + (uint64_t)(strand * kResumePlanes) * pad_cols + (bin >> 6);
    uint32_t c = 0;
    for (uint32_t i = 0; i < kResumePlanes; ++i) c |= (uint32_t)((p[(uint64_t)i * pad_cols] >> (bin & 63u)) & 1ULL) << i;
    counts[t] = (uint16_t)c;
}

// HITS: the opt-in pass (rb_hits_batch_device) that lists EVERY (bin, strand) whose count reached the threshold, with the count --
// the sparse form of what seqan::count returns.  Up to the bit-sliced c > t-1 mask of a strand it runs what ibf_locate_kernel
// runs, behind the same wave prologue (make_pass_wave); then,
// while that strand's planes are still live (records are per strand so that only one strand's planes ever are):
//   * the wave walks the words that hold a hit in rising bin order (columns rise with the lane, words with w, bins with the bit): a
//     ballot finds the lanes, the lane's mask and planes travel as scalars (readlane), and lane j of the wave handles bin j of the word;
//   * a hit's number in the strand's run is the scalar count of the words before plus mbcnt within the word -- a prefix that needs no
//     scan; the count is rebuilt from the planes (bit i of the count is bit j of plane i) and the 8-byte record goes out with one vector
//     store into the (item, slice, strand) segment of the workspace while its number is below the cap.  The walk is wave-uniform, off
//     the gather path and bounded by 2^LG x WPL words; beyond the cap nothing is stored and the totals stay exact.
// No atomic decides a placement.  bin_reads (optional) takes one atomic add per distinct hit bin from the OR of the two masks.  An item
// whose status is not RB_OK is left alone: finish_hits_kernel does not look at its segments.  t == 0: every existing bin on both strands;
// t beyond what NP planes hold: none.
template <int LG, int WPL, int NP, int H, bool NT>
__global__ __launch_bounds__(64 * kWavesPerBlock) __attribute__((amdgpu_waves_per_eu(3, 8))) void ibf_hits_kernel(
    IbfDev f, uint32_t col_begin, uint32_t col_end, ReadSrc src, uint32_t n_items, uint32_t n_slices, const uint16_t *__restrict__ thr,
    uint32_t thr_len, uint32_t nf, uint32_t fi, uint32_t min_count, uint32_t max_hits, uint32_t min_len,
    const uint8_t *__restrict__ pre_status, rb_u32x2 *__restrict__ seg, uint32_t *__restrict__ seg_count,
    unsigned long long *__restrict__ bin_reads)
{
    __shared__ uint8_t s_stage[kWavesPerBlock][kStageBytes];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    uint32_t item, slice;
    wave_item_slice<true>(n_slices, wave, &item, &slice);
    if (item >= n_items) return;  // wave-uniform; there are no block-level barriers below
    // an item that is not RB_OK has no hits and feeds no profile
    if (item_status(pre_status, item, src.lens[item], src.max_len, min_len) != RB_OK) return;  // wave-uniform

    // t: the caller's threshold, or the one the decision kernel reads for this length and filter at the caller's error rate
    const PassWave<WPL> pw = make_pass_wave<LG, WPL>(f, src, col_begin, col_end, item, slice, lane, thr, thr_len, nf, fi, min_count);
    const LaneCols<WPL> &lc = pw.lc;
    const uint32_t t = pw.t;
    const bool group0 = pw.group0;

    uint64_t seen[WPL];  // hit on either strand: the only per-lane state that lives across the strands
#pragma unroll
    for (int w = 0; w < WPL; ++w) seen[w] = 0ULL;
    for (int strand = 0; strand < 2; ++strand) {
        Planes<NP> pl[WPL];
#pragma unroll
        for (int w = 0; w < WPL; ++w) pl[w].clear();
        count_strand<LG, WPL, NP, H, NT>(pl, f, lc, pw.seq, pw.len, pw.n, strand, 0u, (uint32_t)TileShape<LG>::ITEMS, 0, TileShape<LG>::STEPS / 8,
                                         s_stage[wave], lane);
        // ---- bins with c >= t, i.e. c > t - 1
        uint64_t hit[WPL];
#pragma unroll
        for (int w = 0; w < WPL; ++w) hit[w] = (t == 0 && group0) ? lc.valid[w] : 0ULL;
        if (t > 0 && t <= (1u << NP) - 1u) {  // wave-uniform
            const uint32_t tt = t - 1u;
#pragma unroll
            for (int w = 0; w < WPL; ++w) {
                uint64_t gt = 0, eq = lc.valid[w];
#pragma unroll
                for (int i = NP - 1; i >= 0; --i) {
                    if ((tt >> i) & 1u) {  // scalar branch
                        eq &= pl[w].p[i];
                    } else {
                        gt |= eq & pl[w].p[i];
                        eq &= ~pl[w].p[i];
                    }
                }
                hit[w] = group0 ? gt : 0ULL;
            }
        }
        bool mine = false;
#pragma unroll
        for (int w = 0; w < WPL; ++w) {
            mine |= hit[w] != 0ULL;
            seen[w] |= hit[w];
        }
        // ---- the records, one word of 64 bins at a time in rising bin order: the wave visits the lanes that hold a hit (lowest first;
        // a strand without one, the common case, ends at the ballot), takes such a lane's mask and planes as scalars, and lane j writes
        // bin j of the word.  The number of a hit is the scalar count of the words before plus mbcnt within the word.
        uint32_t total = 0;
        uint64_t who = __ballot(mine);
        rb_u32x2 *out = seg + (((size_t)item * n_slices + slice) * 2 + (size_t)strand) * max_hits;
        while (who != 0ULL) {  // wave-uniform, at most 2^LG rounds
            const int from = (int)__builtin_amdgcn_readfirstlane((uint32_t)(__ffsll((unsigned long long)who) - 1));
            who &= who - 1;
#pragma unroll
            for (int w = 0; w < WPL; ++w) {
                const uint32_t mlo = readlane32((uint32_t)hit[w], from), mhi = readlane32((uint32_t)(hit[w] >> 32), from);
                if ((mlo | mhi) == 0u) continue;  // scalar
                if (total < max_hits) {  // scalar: past the cap a word is counted, not stored
                    const uint32_t mhalf = lane < 32 ? mlo : mhi;
                    const bool set = (mhalf >> (lane & 31)) & 1u;
                    const uint32_t pos = total + __builtin_amdgcn_mbcnt_hi(mhi, __builtin_amdgcn_mbcnt_lo(mlo, 0u));
                    uint32_t c = 0;
#pragma unroll
                    for (int i = NP - 1; i >= 0; --i) {  // bit i of the count is bit j of plane i
                        const uint32_t half = lane < 32 ? readlane32((uint32_t)pl[w].p[i], from) : readlane32((uint32_t)(pl[w].p[i] >> 32), from);
                        c = (c << 1) | ((half >> (lane & 31)) & 1u);
                    }
                    if (set && pos < max_hits) {  // pos < max_hits: inside the segment
                        rb_u32x2 rec;
                        rec.x = pw.word_col(from, w) * 64u + (uint32_t)lane;
                        rec.y = c | ((uint32_t)strand << 16);
                        out[pos] = rec;
                    }
                }
                total += (uint32_t)__builtin_popcount(mlo) + (uint32_t)__builtin_popcount(mhi);
            }
        }
        if (lane == 0) seg_count[((size_t)slice * 2 + (size_t)strand) * n_items + item] = total;
    }
    if (bin_reads) {  // uniform: one add per distinct hit bin, word by word as above
        bool mine = false;
#pragma unroll
        for (int w = 0; w < WPL; ++w) mine |= seen[w] != 0ULL;
        uint64_t who = __ballot(mine);
        while (who != 0ULL) {
            const int from = (int)__builtin_amdgcn_readfirstlane((uint32_t)(__ffsll((unsigned long long)who) - 1));
            who &= who - 1;
#pragma unroll
            for (int w = 0; w < WPL; ++w) {
                const uint32_t mlo = readlane32((uint32_t)seen[w], from), mhi = readlane32((uint32_t)(seen[w] >> 32), from);
                if (((lane < 32 ? mlo : mhi) >> (lane & 31)) & 1u)
                    atomicAdd(bin_reads + ((size_t)pw.word_col(from, w) * 64u + (uint32_t)lane), 1ULL);
            }
        }
    }
}

// Finish one filter of a hits call: merge the column slices of an item (slices hold rising bins) and, inside a slice, the two strands'
// sorted runs into (bin, strand) order; apply the per-item status (item_status); write n_hits -- exact, whatever the cap --
// and the first min(n_hits, max_hits) records.  Slots beyond those are not written.  A run longer than the cap was cut at the cap by the
// kernel above: the first max_hits of the merge need no more than the first max_hits of either run.  One thread per work item.
__global__ void finish_hits_kernel(const rb_u32x2 *__restrict__ seg, const uint32_t *__restrict__ seg_count, uint32_t n_slices, uint32_t n_items,
                                   const uint32_t *__restrict__ lens, const uint8_t *__restrict__ pre_status, uint32_t max_len, uint32_t min_len,
                                   uint32_t max_hits, HitsOut out, uint32_t nf, uint32_t fidx)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_items) return;
    const uint8_t status = (uint8_t)item_status(pre_status, i, lens[i], max_len, min_len);
    const size_t o = (size_t)i * nf + fidx;
    uint32_t total = 0, written = 0;
    if (status == RB_OK) {
        rb_u32x2 *dst = out.hits ? out.hits + o * max_hits : nullptr;
        for (uint32_t s = 0; s < n_slices; ++s) {
            const uint32_t na = seg_count[((size_t)s * 2) * n_items + i], nb = seg_count[((size_t)s * 2 + 1) * n_items + i];
            total += na + nb;
            if (!dst || written >= max_hits || na + nb == 0) continue;
            const rb_u32x2 *a = seg + (((size_t)i * n_slices + s) * 2) * max_hits, *b = a + max_hits;
            const uint32_t ma = na < max_hits ? na : max_hits, mb = nb < max_hits ? nb : max_hits;
            uint32_t ia = 0, ib = 0;
            while (written < max_hits && (ia < ma || ib < mb)) {
                // forward first in an equal bin: (bin, strand) order
                const bool take_a = ib >= mb || (ia < ma && a[ia].x <= b[ib].x);
                dst[written++] = take_a ? a[ia++] : b[ib++];
            }
        }
    }
    if (out.n_hits) out.n_hits[o] = total;
    if (out.status && fidx == 0) out.status[i] = status;
}

// SPANS: the opt-in pass (rb_spans_batch_device) that says WHERE ALONG THE READ a bin matched.  A query is (work item, bin) against one
// filter; position p is the window of bases [p, p + k) of the item, in the read's own direction on both strands: strand 0 hits at p
// when all h words selected by that window's k-mer have the bin's bit -- the test by which seqan::count adds 1 to fwd[bin] -- and
// strand 1 when the same holds for the window's reverse complement (k-mer n - 1 - p of the reverse-complemented item), so the hit
// positions of the two strands number fwd[bin] and rev[bin].  One wave per query, built from the pieces of count_strand:
//   * make_base_src and a per-wave LDS area with the bases of kSpanTiles tiles as Dna5 ordinals; lane l of tile j owns position
//     64 j + l and evaluates both strands' base-5 values directly, reading every base once (the reverse complement's value is
//     the sum of comp(b[i]) 5^i: the same ring arithmetic modulo 2^64 as the oracle's Horner form);
//   * the bin is known, so a lookup is ONE 8-byte word, words[block * stride + (bin >> 6)]: 2 h kSpanTiles loads per lane go out
//     back to back with no control flow around them (positions past the end read block 0 and are masked out: the rule of
//     count_strand's phase B) and a schedule fence stands before the first use;
//   * a tile's result per strand is __ballot(hit) -- the mask word the caller gets, stored by one lane -- and count, first, last, the
//     longest run (the open run is carried from word to word) and the covered bases (the word smeared by k - 1 with doubling shifts
//     over previous word : this word) are wave-uniform integer arithmetic on those words.  No atomics, no LDS beyond the staging.
// Every output slot of a query is written, whatever its status: a query that is not RB_OK -- the item's status by item_status,
// or an item / bin that does not exist, which is tested here BEFORE anything is read through it -- gets n_kmers 0, a zero
// record with 0xFFFFFFFF positions and a zero mask.  Positions at or beyond 64 mask_words are left out of the mask only.
constexpr int kSpanTiles = 4;                                        // tiles of 64 positions per round: 2 h kSpanTiles loads in flight per lane
constexpr int kSpanStage = 64 * kSpanTiles + rbspec::kMaxKmer;       // bases staged per round
constexpr uint32_t kSpanNone = 0xFFFFFFFFu;

// what a (query, strand) knows so far; every member is wave-uniform
struct SpanAcc {
    uint32_t count, first, last, run_start, run_len, covered;
    uint32_t open_start, open_len;  // the run of hit positions that ends at the last position seen (open_len == 0: none)
    uint64_t prev;                  // the mask word before this one
};

__device__ __forceinline__ void span_clear(SpanAcc &a)
{
    a.count = 0; a.first = kSpanNone; a.last = kSpanNone; a.run_start = kSpanNone; a.run_len = 0; a.covered = 0;
    a.open_start = 0; a.open_len = 0; a.prev = 0ULL;
}

// bases of the word `cur` covers (64 bases from the word's first position on) that lie in [p, p + k) of a hit position p of prev : cur
__device__ __forceinline__ uint32_t span_covered(uint64_t prev, uint64_t cur, uint32_t k)
{
    uint64_t lo = prev, hi = cur;
    for (uint32_t c = 1; c < k;) {  // c: shifts 0 .. c - 1 are ORed in; k - 1 <= 31 never reaches beyond prev
        const uint32_t sh = min(c, k - c);
        hi |= (hi << sh) | (lo >> (64u - sh));
        lo |= lo << sh;
        c += sh;
    }
    return (uint32_t)__popcll(hi);
}

// the next mask word of a strand: positions base .. base + 63
__device__ __forceinline__ void span_add_word(SpanAcc &a, uint64_t w, uint32_t base, uint32_t k)
{
    a.covered += span_covered(a.prev, w, k);
    a.prev = w;
    const uint32_t carry_start = a.open_start, carry_len = (w & 1ULL) ? a.open_len : 0u;
    a.open_len = 0;
    if (w == 0ULL) return;
    if (a.count == 0) a.first = base + (uint32_t)(__ffsll((unsigned long long)w) - 1);
    a.last = base + 63u - (uint32_t)__clzll((long long)w);
    a.count += (uint32_t)__popcll(w);
    uint64_t x = w;
    uint32_t pos = 0;
    while (x != 0ULL) {  // one turn per run of the word, lowest first: the lowest of equally long runs stays
        const uint32_t tz = (uint32_t)(__ffsll((unsigned long long)x) - 1);
        x >>= tz;  // (tz <= 63)
        pos += tz;
        const uint32_t ones = (~x == 0ULL) ? 64u : (uint32_t)(__ffsll((unsigned long long)~x) - 1);
        const bool joins = pos == 0 && carry_len > 0;
        const uint32_t start = joins ? carry_start : base + pos;
        const uint32_t len = joins ? carry_len + ones : ones;
        if (len > a.run_len) {
            a.run_len = len;
            a.run_start = start;
        }
        if (pos + ones >= 64u) {  // the run reaches the end of the word: it stays open
            a.open_start = start;
            a.open_len = len;
            break;
        }
        x >>= ones;
        pos += ones;
    }
}

// One round's lookups: per (tile, strand, hash function) ONE word, the bin's column of the block the k-mer selects.  All loads of a batch
// -- 2 h kSpanTiles with a compile-time h, 2 kSpanTiles per hash function otherwise -- go out back to back and a schedule fence stands
// before the first use; a position that does not exist reads block 0 and is masked out.  POW2 names the modulus form of
// rbspec::block_index at compile time (the engine's pow2_mask is 0xFFFFFFFF for a block count that is no power of two), so that its
// test is not a branch between two loads.
template <int H, bool NT, bool POW2>
__device__ __forceinline__ void span_gather(bool (&hit)[kSpanTiles][2], const uint64_t (&kv)[kSpanTiles][2], const bool (&ok)[kSpanTiles],
                                            const IbfDev &f, const uint64_t *col, uint64_t S, uint64_t bit)
{
    constexpr int T = kSpanTiles;
    constexpr int HR = H > 0 ? H : 1;
    if constexpr (POW2) __builtin_assume(f.pow2_mask != 0xFFFFFFFFu);
    const uint32_t pm = POW2 ? f.pow2_mask : 0xFFFFFFFFu;
    if constexpr (H > 0) {
        uint64_t ld[T][2][HR];
#pragma unroll
        for (int j = 0; j < T; ++j)
#pragma unroll
            for (int s = 0; s < 2; ++s)
#pragma unroll
                for (int h = 0; h < H; ++h) {
                    const uint32_t b = rbspec::block_index(kv[j][s], f.precalc[h], f.n_blocks, f.magic, pm);
                    ld[j][s][h] = load_word<NT>(col + (uint64_t)(ok[j] ? b : 0u) * S);
                }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int j = 0; j < T; ++j)
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                uint64_t x = bit;
#pragma unroll
                for (int h = 0; h < H; ++h) x &= ld[j][s][h];
                hit[j][s] = ok[j] && x != 0ULL;
            }
    } else {
        uint64_t x[T][2];
#pragma unroll
        for (int j = 0; j < T; ++j) x[j][0] = x[j][1] = ok[j] ? bit : 0ULL;
        for (uint32_t h = 0; h < f.n_hash; ++h) {  // wave-uniform
            uint64_t ld[T][2];
#pragma unroll
            for (int j = 0; j < T; ++j)
#pragma unroll
                for (int s = 0; s < 2; ++s) {
                    const uint32_t b = rbspec::block_index(kv[j][s], f.precalc[h], f.n_blocks, f.magic, pm);
                    ld[j][s] = load_word<NT>(col + (uint64_t)(ok[j] ? b : 0u) * S);
                }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int j = 0; j < T; ++j) {
                x[j][0] &= ld[j][0];
                x[j][1] &= ld[j][1];
            }
        }
#pragma unroll
        for (int j = 0; j < T; ++j) {
            hit[j][0] = x[j][0] != 0ULL;
            hit[j][1] = x[j][1] != 0ULL;
        }
    }
}

template <int H, bool NT>
__global__ __launch_bounds__(64 * kWavesPerBlock) __attribute__((amdgpu_waves_per_eu(4, 8))) void ibf_spans_kernel(
    IbfDev f, ReadSrc src, uint32_t n_items, const rb_u32x2 *__restrict__ queries, uint32_t n_queries, uint32_t mask_words,
    const uint8_t *__restrict__ pre_status, uint32_t min_len, SpansOut out)
{
    __shared__ uint8_t s_stage[kWavesPerBlock][kSpanStage];
    constexpr int T = kSpanTiles;
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const uint32_t qi = __builtin_amdgcn_readfirstlane(blockIdx.x * (uint32_t)kWavesPerBlock + (uint32_t)wave);
    if (qi >= n_queries) return;  // wave-uniform; there are no block-level barriers below
    const rb_u32x2 q = queries[qi];
    const uint32_t item = __builtin_amdgcn_readfirstlane(q.x), bin = __builtin_amdgcn_readfirstlane(q.y);
    uint64_t *const mask0 = out.mask ? out.mask + (size_t)qi * 2 * mask_words : nullptr;  // strand 1 follows mask_words later

    // ---- the query's status: item and bin are tested before anything is read through them
    uint32_t status = RB_OK;
    if (item >= n_items || bin >= f.n_bins) {
        status = RB_ERR_INVALID_ARG;
    } else {
        status = item_status(pre_status, item, src.lens[item], src.max_len, min_len);
    }
    status = __builtin_amdgcn_readfirstlane(status);

    SpanAcc acc[2];
    span_clear(acc[0]);
    span_clear(acc[1]);
    uint32_t n = 0, words_done = 0;
    if (status == RB_OK) {  // wave-uniform
        uint32_t len;
        const BaseSrc seq = make_base_src(src, item, &len);
        const uint32_t k = f.k;
        n = len >= k ? len - k + 1 : 0;  // (min_len >= k: n >= 1)
        const uint64_t *const col = f.words + (bin >> 6);
        const uint64_t bit = 1ULL << (bin & 63u);
        const uint64_t S = f.stride;
        uint8_t *const stage = s_stage[wave];
        for (uint32_t mt = 0; mt < n; mt += 64u * T) {
            // ---- stage the bases of this round as Dna5 ordinals
            const uint32_t wlen = min((uint32_t)(64 * T) + k - 1u, len - mt);
            __builtin_amdgcn_wave_barrier();
            for (uint32_t i = lane; i < wlen; i += 64) stage[i] = (uint8_t)seq.ord(mt + i);
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
            __builtin_amdgcn_wave_barrier();

            // ---- both strands' k-mer value of this lane's position in every tile
            uint64_t kv[T][2];
            bool ok[T];
#pragma unroll
            for (int j = 0; j < T; ++j) {
                const uint32_t p = mt + (uint32_t)(j * 64 + lane);
                ok[j] = p < n;
                uint64_t vf = 0, vr = 0;
                if (ok[j]) {
                    const uint8_t *b = stage + (p - mt);
                    uint64_t pw = 1;
                    for (uint32_t i = 0; i < k; ++i) {
                        const uint32_t o = b[i];
                        vf = vf * 5u + o;
                        vr += pw * rbspec::dna5_comp(o, f.comp_n);
                        pw *= 5u;
                    }
                }
                kv[j][0] = vf;
                kv[j][1] = vr;
            }

            // ---- the gathers (span_gather): the modulus form is chosen here, outside the loads
            bool hit[T][2];
            if (f.pow2_mask != 0xFFFFFFFFu) span_gather<H, NT, true>(hit, kv, ok, f, col, S, bit);  // wave-uniform
            else span_gather<H, NT, false>(hit, kv, ok, f, col, S, bit);

            // ---- a tile's ballot is its mask word; the record follows from the words
#pragma unroll
            for (int j = 0; j < T; ++j) {
                const uint32_t base = mt + (uint32_t)(j * 64);
                if (base < n) {  // wave-uniform
                    const uint32_t wi = base >> 6;
#pragma unroll
                    for (int s = 0; s < 2; ++s) {
                        const uint64_t w = __ballot(hit[j][s]);
                        span_add_word(acc[s], w, base, k);
                        if (mask0 && wi < mask_words && lane == 0) mask0[(size_t)s * mask_words + wi] = w;
                    }
                    words_done = wi + 1;
                }
            }
        }
        // the bases beyond the last position word that its last k - 1 positions still cover
        acc[0].covered += span_covered(acc[0].prev, 0ULL, k);
        acc[1].covered += span_covered(acc[1].prev, 0ULL, k);
    }

    // ---- every slot of the query is written: the rest of the mask is zero ...
    if (mask0) {
#pragma unroll
        for (int s = 0; s < 2; ++s)
            for (uint32_t wi = words_done + (uint32_t)lane; wi < mask_words; wi += 64) mask0[(size_t)s * mask_words + wi] = 0ULL;
    }
    // ... and the two records are twelve consecutive 32-bit words, one per lane
    if (out.spans && lane < 12) {
        const bool rev = lane >= 6;
        const int m = rev ? lane - 6 : lane;
        const uint32_t v0 = m == 0 ? acc[0].count : m == 1 ? acc[0].first : m == 2 ? acc[0].last : m == 3 ? acc[0].run_start : m == 4 ? acc[0].run_len : acc[0].covered;
        const uint32_t v1 = m == 0 ? acc[1].count : m == 1 ? acc[1].first : m == 2 ? acc[1].last : m == 3 ? acc[1].run_start : m == 4 ? acc[1].run_len : acc[1].covered;
        out.spans[(size_t)qi * 12 + (uint32_t)lane] = rev ? v1 : v0;
    }
    if (lane == 0) {
        if (out.n_kmers) out.n_kmers[qi] = n;
        if (out.status) out.status[qi] = (uint8_t)status;
    }
}

// Throughput form over a MERGED table: several narrow filters of one hash geometry (same noOfBlocks, k and h -- every filter
// the reference builds with one fragment_size has them: noOfBits = BinSizeBits x 64 x binWidth, so noOfBlocks = BinSizeBits
// whatever the bin count, src/IBF/IBFBuild.cpp:404-413) hash a k-mer to the SAME block number, so their blocks can sit side
// by side in one table and ONE gather per (k-mer, hash function) serves all of them.  The path is bound by requests, not
// bytes: 1 deplete + 3 target filters of 2 + 1 + 1 + 1 words become one 64-byte gather instead of four lookups.  Counting is
// unchanged (one word column per lane, bit-sliced planes); the max over bins is taken per filter, over the lanes that hold
// that filter's columns, and lane g of the wave carries filter g's result across the strands.
template <int LG, int NP, bool NT>
__global__ __launch_bounds__(64 * kWavesPerBlock) void ibf_count_max_merged_kernel(IbfDev f, MergeMap map, ReadSrc src, uint32_t n_reads,
                                                                                   uint16_t *__restrict__ out, uint32_t out_read_stride)
{
    __shared__ uint8_t s_stage[kWavesPerBlock][kStageBytes];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const uint32_t read = blockIdx.x * kWavesPerBlock + wave;
    if (read >= n_reads) return;  // wave-uniform; no block-level barriers below
    LaneCols<1> lc = make_lane_cols<LG, 1>(f, lane, 0u, f.bin_width, 0u);
    // which bins of this lane's word column exist at all: the union of the members' bit ranges (word-aligned or packed)
    const uint32_t col = (uint32_t)lane & ((1u << LG) - 1u);
    uint64_t valid = 0;
    for (uint32_t g = 0; g < map.n; ++g) valid |= member_mask(map.bit_begin[g], map.bit_end[g], col);
    if (col >= map.width) valid = 0;
    lc.valid[0] = valid;
    lc.colok = valid != 0;
    lc.safe_base = lc.colok ? lc.lane_base : f.words;
    uint32_t len;
    const BaseSrc seq = make_base_src(src, read, &len);
    const uint32_t n = len >= f.k ? len - f.k + 1 : 0;
    uint32_t best = 0;  // lane g: filter g
    for (int strand = 0; strand < 2; ++strand) {
        Planes<NP> pl[1];
        pl[0].clear();
        count_strand<LG, 1, NP, 3, NT>(pl, f, lc, seq, len, n, strand, 0u, (uint32_t)TileShape<LG>::ITEMS, 0, TileShape<LG>::STEPS / 8,
                                       s_stage[wave], lane);
        for (uint32_t g = 0; g < map.n; ++g) {
            const uint64_t mine[1] = {col < map.width ? member_mask(map.bit_begin[g], map.bit_end[g], col) : 0ULL};
            const uint32_t m = planes_max<NP, 1>(pl, mine);
            if ((uint32_t)lane == g) best = m > best ? m : best;
        }
    }
    if ((uint32_t)lane < map.n) out[(size_t)read * out_read_stride + map.out_offset[lane]] = (uint16_t)best;
}

// merged table: block b of a filter (width words at stride s_src, n_bins bins) -> bits [dst_bit, dst_bit + n_bins) of block b of dst.
// One thread per (block, source word): the word is masked to the bins that exist and ORed into the one or two destination words it
// lands in (atomically: members that share a destination word are merged by separate launches on one stream, but two source words
// of ONE member can meet in a destination word when dst_bit is not a multiple of 64).
__global__ void merge_bits_kernel(const uint64_t *__restrict__ src, uint32_t s_src, uint32_t width, uint32_t n_bins, uint64_t *__restrict__ dst,
                                  uint32_t s_dst, uint32_t dst_bit, uint64_t n_blocks)
{
    const uint64_t total = n_blocks * width;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const uint64_t b = i / width;
        const uint32_t c = (uint32_t)(i - b * width);
        uint64_t v = src[b * s_src + c] & member_mask(0u, n_bins, c);
        if (v == 0) continue;
        const uint32_t at = dst_bit + c * 64u;
        const uint32_t w = at >> 6, sh = at & 63u;
        atomicOr(reinterpret_cast<unsigned long long *>(dst + b * s_dst + w), (unsigned long long)(v << sh));
        if (sh && (v >> (64u - sh))) atomicOr(reinterpret_cast<unsigned long long *>(dst + b * s_dst + w + 1), (unsigned long long)(v >> (64u - sh)));
    }
}

// throughput form with clock-phased gathers (see count_strand): narrow filters of a few L2 sizes, one column slice
// (three waves per SIMD: the lookups a CU holds in registers are what a window has to work with).  SHORT != 0: the engine
// knows that no read of the batch has more k-mers than one of the both-strands shapes below takes, and only that path is
// compiled in:
//   SHORT 1  <= 256 k-mers (the reference's default 250 bp chunk): ONE round of 4 tiles per strand -- 93 VGPRs, five waves
//            per SIMD for one-word blocks;
//   SHORT 3  <= 384 k-mers (360 bp reads, the length the reference recommends): ONE round of 6 tiles per strand.  Two rounds
//            of 4 tiles left the second one 36 % dense (92 of 256 k-mers per strand) while every round costs a full turn
//            of windows; 6 tiles are 91 % dense and the per-bin sums of six words still fit three bit planes;
//   SHORT 2  <= 512 k-mers: two rounds of 4 tiles (the general build, SHORT 0, takes this path too and falls back to
//            the per-strand tiles of count_strand for longer reads).
// bins of a word column as a mask (NarrowMerge::col_bits)
__device__ __forceinline__ uint64_t col_bits_mask(uint32_t bits) { return bits >= 64 ? ~0ULL : ((1ULL << bits) - 1); }

// The end of the one-lane-per-block rounds: lane b holds, per word column c, the larger of the two strands' counts of bin 64 c + b;
// every member of the (possibly merged) table gets the maximum over ITS bins -- the bit range [bit_begin, bit_end) of the block,
// word-aligned or packed -- and the wave.
template <int NC>
__device__ __forceinline__ void write_member_maxima(const uint32_t (&colmax)[NC], const NarrowMerge &nm, int lane, uint16_t *out)
{
    for (uint32_t g = 0; g < nm.n; ++g) {
        uint32_t m = 0;
        // bin 64 c + lane lies in [begin, end)  <=>  (lane - begin) + 64 c < end - begin in unsigned arithmetic: one subtraction per member
        // (the two-sided compare per column cost the two-word 250 bp build its 72nd register: 73 -> six instead of seven waves per SIMD,
        // 9.3 -> 10.8 ms per 1 M reads on a 20 MB table)
        const uint32_t rel = (uint32_t)lane - nm.bit_begin[g], span = nm.bit_end[g] - nm.bit_begin[g];
#pragma unroll
        for (int c = 0; c < NC; ++c) m = ((rel + (uint32_t)(c * 64)) < span && colmax[c] > m) ? colmax[c] : m;
#pragma unroll
        for (int sft = 1; sft < 64; sft <<= 1) {
            const uint32_t o = shfl32(m, lane ^ sft);
            m = o > m ? o : m;
        }
        if (lane == 0) out[nm.out_offset[g]] = (uint16_t)m;
    }
}

// k-mer values from staged TRIPLES of bases, for k <= 13 (the reference's default; 5^13 < 2^31, so a value fits 32 bits).  Beside the
// staged Dna5 ordinals ord[i] a read's staging area holds f3[i] = 25 ord[i] + 5 ord[i+1] + ord[i+2] and r3[i] = the same of the
// complemented bases in reverse order; the forward value of the window at p is then k/3 steps `v = 125 v + f3[..]` (v_mad_u32_u24: every
// step starts below 5^10 < 2^24, the 24-bit multiply is exact) plus k%3 single bases, the reverse-complement value the single bases from
// the right end first and then the triples from the right -- ~20 VALU instructions per window position and both strands where thirteen
// 64-bit multiply-adds per strand took ~180.  The narrow kernels are three quarters VALU-busy (profiles/r05/pmc_summary.csv, targets3:
// SQ_INSTS_VALU 4 207 per read x 4 cycles over 1 024 SIMDs = 7.3 of 9.5 ms), and the hashing was the largest part of it.
constexpr uint32_t kTripleMaxK = 13;
__device__ __forceinline__ void stage_triples(const uint8_t *ord, uint8_t *f3, uint8_t *r3, uint32_t len, uint32_t comp_n, int lane)
{
    for (uint32_t i = lane; i + 2 < len; i += 64) {
        const uint32_t a = ord[i], b = ord[i + 1], c = ord[i + 2];
        f3[i] = (uint8_t)(a * 25u + b * 5u + c);
        r3[i] = (uint8_t)(rbspec::dna5_comp(c, comp_n) * 25u + rbspec::dna5_comp(b, comp_n) * 5u + rbspec::dna5_comp(a, comp_n));
    }
}
// values of the k-mer at p and of its reverse complement; small_k: the triples are staged (k <= kTripleMaxK), q3 = k / 3, s1 = k % 3
__device__ __forceinline__ void kmer_values_both(const uint8_t *ord, const uint8_t *f3, const uint8_t *r3, uint32_t p, uint32_t k, uint32_t q3,
                                                 uint32_t s1, uint32_t comp_n, bool small_k, uint64_t &vf, uint64_t &vr)
{
    if (small_k) {
        uint32_t a = 0, b = 0;
        for (uint32_t t = 0; t < q3; ++t) a = __umul24(a, 125u) + f3[p + 3u * t];
        for (uint32_t t = 0; t < s1; ++t) a = a * 5u + ord[p + 3u * q3 + t];
        for (uint32_t t = 0; t < s1; ++t) b = b * 5u + rbspec::dna5_comp(ord[p + k - 1u - t], comp_n);
        for (uint32_t t = q3; t-- > 0;) b = __umul24(b, 125u) + r3[p + 3u * t];
        vf = a;
        vr = b;
    } else {
        const uint8_t *bs = ord + p;
        vf = 0;
        vr = 0;
        for (uint32_t i = 0; i < k; ++i) vf = vf * 5u + bs[i];
        for (uint32_t i = 0; i < k; ++i) vr = vr * 5u + rbspec::dna5_comp(bs[k - 1 - i], comp_n);
    }
}
// the same for ONE strand (rc: the reverse complement's k-mer over the window at p)
__device__ __forceinline__ uint64_t kmer_value_one(const uint8_t *ord, const uint8_t *f3, const uint8_t *r3, uint32_t p, uint32_t k, uint32_t q3,
                                                   uint32_t s1, uint32_t comp_n, bool small_k, bool rc)
{
    if (small_k) {
        uint32_t a = 0;
        if (!rc) {
            for (uint32_t t = 0; t < q3; ++t) a = __umul24(a, 125u) + f3[p + 3u * t];
            for (uint32_t t = 0; t < s1; ++t) a = a * 5u + ord[p + 3u * q3 + t];
        } else {
            for (uint32_t t = 0; t < s1; ++t) a = a * 5u + rbspec::dna5_comp(ord[p + k - 1u - t], comp_n);
            for (uint32_t t = q3; t-- > 0;) a = __umul24(a, 125u) + r3[p + 3u * t];
        }
        return a;
    }
    const uint8_t *bs = ord + p;
    uint64_t v = 0;
    if (!rc) {
        for (uint32_t i = 0; i < k; ++i) v = v * 5u + bs[i];
    } else {
        for (uint32_t i = 0; i < k; ++i) v = v * 5u + rbspec::dna5_comp(bs[k - 1 - i], comp_n);
    }
    return v;
}
// staging area of the one-lane-per-block register builds: the ordinals of a read of up to 512 + k - 1 bases, then the two triple arrays
constexpr int kTripleStride = 64 * kMaxTiles + rbspec::kMaxKmer;  // = kStageBytes: bytes per staged array
constexpr int kStageBytes3 = 3 * kTripleStride;

// Waves per SIMD each build of the phased kernel is compiled for (amdgpu_waves_per_eu minimum = the register budget the compiler
// works against).  Left to itself it stops at the first allocation that fits its default target; told to aim higher it finds
// 56 instead of 73 registers for the one-word 250 bp build (8 waves), 76 instead of 93 for the one-word 360 bp build (6 waves), 72
// instead of 86 for the two-word 250 bp build (7 waves) -- all without scratch (the two-word 360 bp build spills 96 bytes at five
// waves and stays at four).  More reads per cycle: 5-15 % less time per read at the (longer) windows that go with it
// (profiles/r03/slice_size.txt, session 54).
#ifndef RB_WAVES_0_1
#define RB_WAVES_0_1 7
#endif
#ifndef RB_WAVES_0_3
#define RB_WAVES_0_3 6
#endif
#ifndef RB_WAVES_1_1
#define RB_WAVES_1_1 6
#endif
#ifndef RB_WAVES_1_3
#define RB_WAVES_1_3 3
#endif
#ifndef RB_TILES_ROUNDS  // tiles per strand and round of the one-word build for reads of 385-512 k-mers: three (63 registers, eight waves per
                        // SIMD; two rounds of four tiles took 111 registers, four waves: session 61, 7-13 % slower); two-word blocks keep four
#define RB_TILES_ROUNDS 3
#endif
#ifndef RB_WIDE3_ROUNDS  // a three-word build for the rounds of three tiles as well (94 registers at five waves per SIMD; session 59: 3-10 % faster)
#define RB_WIDE3_ROUNDS 1
#endif
#ifndef RB_WAVES_0_2
#define RB_WAVES_0_2 7
#endif
#ifndef RB_WAVES_1_2
#define RB_WAVES_1_2 3
#endif
#ifndef RB_WAVES_2_2
#define RB_WAVES_2_2 3
#endif
#ifndef RB_WAVES_2_2_NW3
#define RB_WAVES_2_2_NW3 5
#endif
#ifndef RB_WAVES_GEN
#define RB_WAVES_GEN 3
#endif
constexpr int phased_min_waves(int lg, int shrt, int nw)
{
    if (lg == 0) return shrt == 1 ? RB_WAVES_0_1 : shrt == 3 ? RB_WAVES_0_3 : shrt ? RB_WAVES_0_2 : RB_WAVES_GEN;
    if (lg == 1) return shrt == 1 ? RB_WAVES_1_1 : shrt == 3 ? RB_WAVES_1_3 : shrt ? RB_WAVES_1_2 : RB_WAVES_GEN;
    if (lg == 2 && shrt == 1) return nw == 3 ? RB_WIDE_WAVES : 4;
    if (lg == 2) return nw == 3 ? RB_WAVES_2_2_NW3 : RB_WAVES_2_2;
    return 3;
}

template <int LG, int NP, int SHORT, int NW = 4>  // NW: words per block the one-lane build for stride-4 blocks holds (3: no fourth column)
__global__ __launch_bounds__(64 * kWavesPerBlock) __attribute__((amdgpu_waves_per_eu(phased_min_waves(LG, SHORT, NW), 8))) void ibf_count_max_phased_kernel(
    IbfDev f, uint32_t col_begin, uint32_t col_end, ReadSrc src, uint32_t n_reads, PhaseCfg ph, uint16_t *__restrict__ out,
    uint32_t out_read_stride, NarrowMerge nm)
{
    __shared__ uint8_t s_stage[kWavesPerBlock][kStageBytes3];  // (ordinals + the two triple arrays of stage_triples)
    if (ph.xcd_skew) ph.skew = xcc_id();
    if (ph.tskew) ph.tskew *= xcc_id();
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const uint32_t read = blockIdx.x * kWavesPerBlock + wave;
    if (read >= n_reads) return;  // wave-uniform; no block-level barriers below
    const LaneCols<1> lc = make_lane_cols<LG, 1>(f, lane, col_begin, col_end, 0);
    uint32_t len;
    const BaseSrc seq = make_base_src(src, read, &len);
    const uint32_t n = len >= f.k ? len - f.k + 1 : 0;
    uint32_t best = 0;
    constexpr int T = SHORT == 3 ? 6 : (SHORT == 2 && LG == 0) ? RB_TILES_ROUNDS : 4;  // 64-k-mer tiles per strand and round
    constexpr uint32_t kRound = 64u * T;                       // k-mers per strand and round
    constexpr bool kOneRound = SHORT == 1 || SHORT == 3;       // no loop state (registers)
    if constexpr (LG == 0) {
        // One-word blocks, reads of up to 512 k-mers: a 512-k-mer macro tile per strand would leave more than half of the 24
        // lookups a lane can keep in flight unused on the reference's default 250 bp chunk (238 k-mers) -- and the windows
        // of the phased form live on lookups held in registers.  So both strands share a macro tile: tiles 0..T-1 are
        // forward k-mers, tiles T..2T-1 the k-mers of the reverse complement over the same windows (separate counts, as in
        // the reference).
        constexpr uint32_t kBothMax = SHORT == 1 ? 256u : SHORT == 3 ? 384u : 512u;  // the general build takes two rounds as well
        if (n <= kBothMax) {  // len <= 512 + k - 1 <= kStageBytes: the whole read is staged once
            uint8_t *stage = s_stage[wave];
            for (uint32_t i = lane; i < len; i += 64) stage[i] = (uint8_t)seq.ord(i);
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
            __builtin_amdgcn_wave_barrier();
            const uint32_t k = f.k;
            // (the build with loop state, rounds of three tiles, keeps the 64-bit Horner: the triples' extra state costs it its eighth wave -- 72
            // registers and a spill)
            const bool small_k = !(SHORT == 2) && k <= kTripleMaxK;
            const uint32_t q3 = k / 3u, s1 = k - 3u * q3;
            if (small_k) {
                stage_triples(stage, stage + kTripleStride, stage + 2 * kTripleStride, len, f.comp_n, lane);
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
                __builtin_amdgcn_wave_barrier();
            }
            const uint32_t col_bytes = (uint32_t)((lc.lane_base - f.words) * 8);
            const uint32_t slice_shift = (ph.shift >> 31) ? (0x80000000u | ((ph.shift & 0x7FFFFFFFu) * (f.stride * 8u)))
                                                          : min(31u, ph.shift + 3u + (31u - (uint32_t)__builtin_clz(f.stride)));
            uint32_t cf = 0, cr = 0;  // lane b: count of bin b, forward / reverse complement
            // the counts of a round are summed across the wave at once, so no counter planes are carried
#pragma unroll 1
            for (uint32_t base = 0; base < (kOneRound ? 1u : n); base += kRound) {
            uint32_t bn[2 * T][3];
            uint64_t x[2 * T];
#pragma unroll
            for (int j = 0; j < 2 * T; ++j) {  // slots 0 .. T-1: forward k-mers; T .. 2T-1: those of the reverse complement over the same windows
                const uint32_t p = base + (uint32_t)((j % T) * 64 + lane);
                const bool ok = (p < n) && lc.colok;
                uint64_t v = 0;
                if (ok) v = kmer_value_one(stage, stage + kTripleStride, stage + 2 * kTripleStride, p, k, q3, s1, f.comp_n, small_k, j >= T);
#pragma unroll
                for (int h = 0; h < 3; ++h) {
                    const uint32_t blk = rbspec::block_index(v, f.precalc[h], f.n_blocks, f.magic, f.pow2_mask);
                    bn[j][h] = ok ? blk * (f.stride * 8u) + col_bytes : 0xFFFFFFFFu;
                }
                if constexpr (T == 6) __builtin_amdgcn_sched_barrier(0);  // one k-mer's hash chains at a time (registers)
            }
#pragma unroll
            for (int j = 0; j < 2 * T; ++j) x[j] = bn[j][0] != 0xFFFFFFFFu ? lc.valid[0] : 0ULL;  // after the hashing: 16 registers less there
            // (six tiles per strand: the 36 gathers of a window go out in two batches of 18)
            phased_gather<2 * T, 3, false, T == 6 ? RB_GATHER_B3 : (SHORT == 1 ? RB_GATHER_B1 : (T == 4 ? 8 : 2))>(x, bn, f.words, slice_shift, ph);
            cf += wave_bin_counts<T>(x, lane);
            cr += wave_bin_counts<T>(x + T, lane);
            }
            uint32_t m = cf > cr ? cf : cr;  // bins beyond noOfBins count 0: the gathered words were masked with lc.valid
#pragma unroll
            for (int sft = 1; sft < 64; sft <<= 1) {
                const uint32_t o = shfl32(m, lane ^ sft);
                m = o > m ? o : m;
            }
            if (lane == 0) out[(size_t)read * out_read_stride] = (uint16_t)m;
            return;
        }
    }
    if constexpr (LG == 1) {
        // Two-word blocks (65-128 bins), reads of up to 512 k-mers: the same both-strands tile with ONE lane per block and
        // 16-byte gathers -- twice the lookups a wave holds per round of windows compared with two lanes per block, and
        // a 20 MB table has to cross the fabric once per round whatever a wave asks of it.
        // (two rounds only in the build that has nothing else in it: next to the per-strand path the loop state spills)
        constexpr uint32_t kBothMax = SHORT == 2 ? 512u : SHORT == 3 ? 384u : 256u;
        if (n <= kBothMax && col_begin == 0 && col_end == 2 && f.stride == 2) {
            uint8_t *stage = s_stage[wave];
            for (uint32_t i = lane; i < len; i += 64) stage[i] = (uint8_t)seq.ord(i);
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
            __builtin_amdgcn_wave_barrier();
            const uint32_t k = f.k;
            const bool small_k = !(SHORT == 2) && k <= kTripleMaxK;  // (not in the builds with loop state: registers)
            const uint32_t q3 = k / 3u, s1 = k - 3u * q3;
            if (small_k) {
                stage_triples(stage, stage + kTripleStride, stage + 2 * kTripleStride, len, f.comp_n, lane);
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
                __builtin_amdgcn_wave_barrier();
            }
            const uint64_t valid0 = col_bits_mask(nm.col_bits[0]), valid1 = col_bits_mask(nm.col_bits[1]);
            const uint32_t slice_shift = (ph.shift >> 31) ? (0x80000000u | ((ph.shift & 0x7FFFFFFFu) * 16u)) : min(31u, ph.shift + 4u);
            uint32_t cf = 0, cr = 0;  // lane b: counts of bins b (low half) and 64 + b (high half), forward / reverse complement
#pragma unroll 1
            for (uint32_t base = 0; base < (SHORT == 2 ? n : 1u); base += kRound) {
            uint32_t bn[2 * T][3];
            uint64_t x0[2 * T], x1[2 * T];
#pragma unroll
            for (int j = 0; j < 2 * T; ++j) {
                const uint32_t p = base + (uint32_t)((j % T) * 64 + lane);
                const bool ok = p < n;
                uint64_t v = 0;
                if (ok) v = kmer_value_one(stage, stage + kTripleStride, stage + 2 * kTripleStride, p, k, q3, s1, f.comp_n, small_k, j >= T);
#pragma unroll
                for (int h = 0; h < 3; ++h) {
                    const uint32_t blk = rbspec::block_index(v, f.precalc[h], f.n_blocks, f.magic, f.pow2_mask);
                    bn[j][h] = ok ? blk * 16u : 0xFFFFFFFFu;
                }
                // six tiles: one k-mer's hash chains at a time (interleaved, the twelve of them spill 60 registers)
                if constexpr (T == 6) __builtin_amdgcn_sched_barrier(0);
            }
            // the AND accumulators start as "every existing bin" for the k-mers that exist (set up after the hashing: 32
            // registers less while the hash chains are in flight)
#pragma unroll
            for (int j = 0; j < 2 * T; ++j) {
                const bool ok = bn[j][0] != 0xFFFFFFFFu;
                x0[j] = ok ? valid0 : 0ULL;
                x1[j] = ok ? valid1 : 0ULL;
            }
            // (the builds with loop state or six tiles send two k-mers' gathers at a time: with four the state does not fit
            // three waves per SIMD)
            phased_gather_x2<2 * T, 3, SHORT == 1 ? RB_GATHER_KB1 : (SHORT == 3 ? RB_GATHER_KB3 : 2)>(x0, x1, bn, f.words, slice_shift, ph);
            cf += wave_bin_counts<T>(x0, lane) | (wave_bin_counts<T>(x1, lane) << 16);
            cr += wave_bin_counts<T>(x0 + T, lane) | (wave_bin_counts<T>(x1 + T, lane) << 16);
            }
            const uint32_t colmax[2] = {max(cf & 0xFFFFu, cr & 0xFFFFu), max(cf >> 16, cr >> 16)};  // at most 512 each: no carry between halves
            write_member_maxima<2>(colmax, nm, lane, out + (size_t)read * out_read_stride);
            return;
        }
    }
    if constexpr (LG == 2 && (SHORT == 2 || SHORT == 1)) {
        // Three- and four-word blocks (129-256 bins, stride 4 words), reads of up to 512 k-mers: ONE lane per block with two
        // 16-byte gathers, both strands in rounds of two 64-k-mer tiles each (a lane's AND accumulators are 4 words x 4 k-mers =
        // 32 registers; four tiles per strand would take 64 and leave three waves per SIMD)
        // SHORT 1: one round of four tiles per strand (<= 256 k-mers; 116 registers, four waves per SIMD); otherwise rounds of three
        // tiles (113 registers, four waves; 360 bp reads take two rounds, 91 % dense -- rounds of two tiles: three rounds, 11-17 %
        // instead of 30-50 % over the plain kernel; four tiles with the loop state: 163 registers, three waves, slower still)
        constexpr int T2 = SHORT == 1 ? 4 : RB_WIDE_TILES;
        if (n <= (SHORT == 1 ? 256u : 512u) && col_begin == 0 && (col_end == (uint32_t)NW || (NW == 4 && col_end == 3)) && f.stride == 4) {
            uint8_t *stage = s_stage[wave];
            for (uint32_t i = lane; i < len; i += 64) stage[i] = (uint8_t)seq.ord(i);
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
            __builtin_amdgcn_wave_barrier();
            const uint32_t k = f.k;
            const bool small_k = SHORT == 1 && k <= kTripleMaxK;  // (not in the builds with loop state: registers)
            const uint32_t q3 = k / 3u, s1 = k - 3u * q3;
            if (small_k) {
                stage_triples(stage, stage + kTripleStride, stage + 2 * kTripleStride, len, f.comp_n, lane);
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
                __builtin_amdgcn_wave_barrier();
            }
            const uint64_t valid0 = col_bits_mask(nm.col_bits[0]), valid1 = col_bits_mask(nm.col_bits[1]);
            const uint64_t valid2 = col_bits_mask(nm.col_bits[2]), valid3 = col_bits_mask(nm.col_bits[3]);
            const uint32_t slice_shift = (ph.shift >> 31) ? (0x80000000u | ((ph.shift & 0x7FFFFFFFu) * 32u)) : min(31u, ph.shift + 5u);
            uint32_t c01f = 0, c23f = 0, c01r = 0, c23r = 0;  // lane b: counts of bins b | 64 + b << 16, and 128 + b | 192 + b << 16
#pragma unroll 1
            for (uint32_t base = 0; base < (SHORT == 1 ? 1u : n); base += 64u * T2) {
                uint32_t bn[2 * T2][3];
                uint64_t x0[2 * T2], x1[2 * T2], x2[2 * T2], x3[2 * T2];
#pragma unroll
                for (int j = 0; j < 2 * T2; ++j) {
                    const uint32_t p = base + (uint32_t)((j % T2) * 64 + lane);
                    const bool ok = p < n;
                    uint64_t v = 0;
                    if (ok) v = kmer_value_one(stage, stage + kTripleStride, stage + 2 * kTripleStride, p, k, q3, s1, f.comp_n, small_k, j >= T2);
#pragma unroll
                    for (int h = 0; h < 3; ++h) {
                        const uint32_t blk = rbspec::block_index(v, f.precalc[h], f.n_blocks, f.magic, f.pow2_mask);
                        bn[j][h] = ok ? blk * 32u : 0xFFFFFFFFu;
                    }
                }
#pragma unroll
                for (int j = 0; j < 2 * T2; ++j) {
                    const bool ok = bn[j][0] != 0xFFFFFFFFu;
                    x0[j] = ok ? valid0 : 0ULL;
                    x1[j] = ok ? valid1 : 0ULL;
                    x2[j] = ok ? valid2 : 0ULL;
                    x3[j] = (ok && NW == 4) ? valid3 : 0ULL;
                }
                phased_gather_x4<2 * T2, 3, 1, NW>(x0, x1, x2, x3, bn, f.words, slice_shift, ph);
                c01f += wave_bin_counts<T2>(x0, lane) | (wave_bin_counts<T2>(x1, lane) << 16);
                c01r += wave_bin_counts<T2>(x0 + T2, lane) | (wave_bin_counts<T2>(x1 + T2, lane) << 16);
                if constexpr (NW == 4) {
                    c23f += wave_bin_counts<T2>(x2, lane) | (wave_bin_counts<T2>(x3, lane) << 16);
                    c23r += wave_bin_counts<T2>(x2 + T2, lane) | (wave_bin_counts<T2>(x3 + T2, lane) << 16);
                } else {
                    c23f += wave_bin_counts<T2>(x2, lane);
                    c23r += wave_bin_counts<T2>(x2 + T2, lane);
                }
            }
            const uint32_t colmax[4] = {max(c01f & 0xFFFFu, c01r & 0xFFFFu), max(c01f >> 16, c01r >> 16),
                                        max(c23f & 0xFFFFu, c23r & 0xFFFFu), max(c23f >> 16, c23r >> 16)};  // at most 512 each: no carry
            write_member_maxima<4>(colmax, nm, lane, out + (size_t)read * out_read_stride);
            return;
        }
    }
    if constexpr (!SHORT) {
        for (int strand = 0; strand < 2; ++strand) {
            Planes<NP> pl[1];
            pl[0].clear();
            count_strand<LG, 1, NP, 3, false, true>(pl, f, lc, seq, len, n, strand, 0u, (uint32_t)TileShape<LG>::ITEMS, 0,
                                                    TileShape<LG>::STEPS / 8, s_stage[wave], lane, ph);
            const uint32_t m = planes_max<NP, 1>(pl, lc.valid);
            best = m > best ? m : best;
        }
    }
    // SHORT: a read with more k-mers than promised (256 / 384 / 512) writes 0 here; the decision kernel turns a length above the
    // declared max_len into RB_ERR_INVALID_ARG, so the value is never used
    if (lane == 0) {
        out[(size_t)read * out_read_stride + nm.out_offset[0]] = (uint16_t)best;
        for (uint32_t g = 1; g < nm.n; ++g) out[(size_t)read * out_read_stride + nm.out_offset[g]] = 0;  // (merged tables: SHORT builds only)
    }
}

// ---------------------------------------------------------------------------------------------
// SEVERAL READS PER WAVE through one pass of the clock-phased windows (round 6; two-word blocks, reads of up to 256 k-mers: the
// build ibf_count_max_phased_kernel<1,10,1,4> serves with one read per wave).  Why: a pass of the chip over all slices reloads the
// table once per XCD, whatever the number of reads that ride along, so the fabric's share of a read's time falls with the reads a CU
// holds per pass -- and those are bounded by on-chip state: per read 8 slots x 64 lanes x (16 bytes of AND accumulator + three
// offsets).  The shipped build keeps both in registers (72 VGPRs, seven waves per SIMD: 28 reads per CU).  Here the accumulators of R
// reads stay in registers and the offsets live in LDS, three block numbers of 21 bits packed into one 64-bit word per (read, slot,
// lane) -- 4 KiB per read, read back once per window (ds_read_b64, lane-consecutive: conflict-free) and unpacked with four VALU
// operations; recomputing them per window from the staged bases instead (3 x 64-bit multiply + xor-shift + Barrett per k-mer) would
// cost more VALU time than a window has.  R = 2 at five waves per SIMD: 40 reads per CU, 160 KiB of LDS -- all of it, which is why
// a read's bases are staged inside its own last slot's region (the slot is hashed into registers before it is overwritten) and a
// workgroup is ONE wave (LDS is granted per workgroup: 8 KiB units pack where 32 KiB units would not).
// Packed block numbers (kPackBits, rb_device.h): tables of at most kPackMaxBlocks = 2^21 - 2 blocks (32 MiB of two-word blocks);
// 0x1FFFFF = no lookup, out of range of every slice because a slice's descriptor ends with the table.  Same windows, same slices, same
// counting as the one-read build; results are identical by construction (the same AND of the same words).
// One-word blocks (8 bytes each: a table of 2^21 of them is only 16 MiB) pack 22-bit block numbers (kPackBits1): the first two whole, the
// low 20 bits of the third, and its top two bits in a per-lane SPILL word held in a register (two bits per slot, at most twelve slots) --
// tables of up to kPackMaxBlocks1 = 2^22 - 2 blocks (32 MiB), which takes in the 64-bin filter of the reference's own test data (2.47 M
// blocks).  Two VALU operations more per slot and window; 0x3FFFFF = no lookup.
#ifndef RB_MULTI_WAVES
#define RB_MULTI_WAVES 5
#endif
#ifndef RB_MULTI_WAVES_W4  // the four-word build of four tiles (64 accumulator registers)
#define RB_MULTI_WAVES_W4 5
#endif

// three packed block numbers of one k-mer (PB = kPackBits each, or kPackBits1 with the third one's top two bits returned in hi2)
template <int PB>
__device__ __forceinline__ uint64_t pack_lookups(uint64_t v, const IbfDev &f, uint32_t &hi2)
{
    const uint64_t b0 = rbspec::block_index(v, f.precalc[0], f.n_blocks, f.magic, f.pow2_mask);
    const uint64_t b1 = rbspec::block_index(v, f.precalc[1], f.n_blocks, f.magic, f.pow2_mask);
    const uint64_t b2 = rbspec::block_index(v, f.precalc[2], f.n_blocks, f.magic, f.pow2_mask);
    hi2 = PB == (int)kPackBits ? 0u : (uint32_t)(b2 >> 20);
    return b0 | (b1 << PB) | (b2 << (2 * PB));  // (22 bits: the shift drops the third number's top two bits)
}

// Phase A of the multi-read build for ONE read: its k-mers' packed block numbers go to slots[j * 64 + lane], j = 0..3 the forward
// k-mers at p = 64 j + lane, j = 4..7 the k-mers of the reverse complement over the same windows (~0: no such k-mer).  Returns the
// number of k-mers (0: no such read, a read shorter than k, or one longer than the build was promised -- it counts 0 like the
// one-read build).  The read's bases are staged INSIDE the regions of its own slots 6 and 7 (1 KiB; the wave has no other LDS), so
// those two slots are hashed into registers and stored after every lane is through with the staged bases.
// k <= 13 (the reference's default; 5^13 < 2^31): the k-mer values are 32-bit and come from staged TRIPLES of bases -- f3[i] =
// 25 b[i] + 5 b[i+1] + b[i+2], r3[i] the same of the complemented bases in reverse order -- so a value is four v_mad_u32_u24 by 125
// and one step by 5 instead of thirteen 64-bit multiply-adds per strand (~20 instead of ~180 VALU instructions per window position
// and both strands).  The count kernels of the narrow filters are three quarters VALU-busy (profiles/r05/pmc_summary.csv, targets3:
// SQ_INSTS_VALU 4 207 per read, x 4 cycles over 1024 SIMDs = 7.3 of the kernel's 9.5 ms).  Longer k: 64-bit Horner over the bases.
// T: 64-k-mer tiles per strand (4: reads of up to 256 k-mers; 6: up to 384, the 360 bp prefixes the reference recommends); 2 T slots
// per lane.  The staging area is the region of the last NST slots (T 4: 1 KiB for up to 268 bases and their two triple arrays; T 6:
// 1.5 KiB for up to 396), which are reverse-strand slots of the last NST tiles.
template <int T>
struct MultiShape {
    static constexpr int S = 2 * T;                       // slots per lane
    static constexpr int NST = T == 4 ? 2 : 3;            // slot regions that hold the staged bases
    static constexpr uint32_t kMaxKmers = 64u * T;
    static constexpr uint32_t kArr = T == 4 ? 272u : 400u;  // bytes per staged array: ord, then f3, then r3
    static_assert(3 * kArr <= NST * 512u, "the staged arrays fit the slot regions they borrow");
};

template <int T, int PB>
__device__ __forceinline__ void multi_hash_staged(uint64_t *slots, const IbfDev &f, uint32_t len, uint32_t n, int lane, uint32_t &spill);
template <int T, int PB = (int)kPackBits>
__device__ __forceinline__ uint32_t multi_hash_read(uint64_t *slots, const IbfDev &f, const ReadSrc &src, uint32_t rid, uint32_t n_reads, int lane, uint32_t &spill)
{
    using M = MultiShape<T>;
    const uint32_t k = f.k;
    uint32_t len = 0, n = 0;
    uint8_t *ord = reinterpret_cast<uint8_t *>(slots + (M::S - M::NST) * 64);
    if (rid < n_reads) {
        const BaseSrc seq = make_base_src(src, rid, &len);
        n = len >= k ? len - k + 1 : 0;
        if (n > M::kMaxKmers) n = 0;
        if (n)
            for (uint32_t i = lane; i < len; i += 64) ord[i] = (uint8_t)seq.ord(i);
    }
    multi_hash_staged<T, PB>(slots, f, len, n, lane, spill);
    return n;
}

// the second half: the read's Dna5 ordinals are staged at the start of the staging area (by this wave; no fence taken yet)
// (spill: PB = 22 only -- bits 2 u, 2 u + 1 = the top two bits of slot u's third block number; all ones where a slot has no k-mer)
template <int T, int PB>
__device__ __forceinline__ void multi_hash_staged(uint64_t *slots, const IbfDev &f, uint32_t len, uint32_t n, int lane, uint32_t &spill)
{
    using M = MultiShape<T>;
    const uint32_t k = f.k;
    uint8_t *ord = reinterpret_cast<uint8_t *>(slots + (M::S - M::NST) * 64);
    uint8_t *f3 = ord + M::kArr, *r3 = ord + 2 * M::kArr;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
    const bool small_k = k <= kTripleMaxK;
    if (small_k && n) {
        stage_triples(ord, f3, r3, len, f.comp_n, lane);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
        __builtin_amdgcn_wave_barrier();
    }
    const uint32_t q3 = k / 3u, s1 = k - 3u * q3;  // k = 3 q3 + s1
    uint64_t held_r[M::NST];  // the last NST tiles: their reverse slots hold the staged bases
#pragma unroll
    for (int i = 0; i < M::NST; ++i) held_r[i] = ~0ULL;
#pragma unroll
    for (int j = 0; j < T; ++j) {
        const uint32_t p = (uint32_t)(j * 64 + lane);
        uint64_t pf = ~0ULL, pr = ~0ULL;
        if (p < n) {
            uint64_t vf, vr;
            uint32_t hf, hr;
            kmer_values_both(ord, f3, r3, p, k, q3, s1, f.comp_n, small_k, vf, vr);
            pf = pack_lookups<PB>(vf, f, hf);
            pr = pack_lookups<PB>(vr, f, hr);
            if constexpr (PB != (int)kPackBits)
                spill = (spill & ~((3u << (2 * j)) | (3u << (2 * (j + T))))) | (hf << (2 * j)) | (hr << (2 * (j + T)));
        }
        slots[j * 64 + lane] = pf;
        if (j < T - M::NST) slots[(j + T) * 64 + lane] = pr;
        else held_r[j - (T - M::NST)] = pr;
        __builtin_amdgcn_sched_barrier(0);  // one window position's hash chains at a time (registers)
    }
    // every lane has hashed its k-mers by now: the last slots take over the staging area
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int i = 0; i < M::NST; ++i) slots[(M::S - M::NST + i) * 64 + lane] = held_r[i];
}

// The accumulators of one read: x0 / x1 = the two word columns of every slot, combined over the three lookups.
// !INV: x = AND of the table words (a lane that loaded nothing got 0 from the bounds check and ORs in its all-ones mask first).
// INV: the table holds the COMPLEMENT of the filter's bits (the engine's merged copy has such a twin, rb_engine.hip), x = OR of
// the loaded words -- the bounds check's 0 is then neutral by itself: no compare, no mask, four ORs per lookup instead of a
// compare, a select, four ORs and four ANDs, and the relative offsets need not outlive the loads (six registers).  A bin is hit
// where x stays 0; slots without a k-mer start all-ones, bits beyond a column's bins as well.
template <bool INV, int T, int NW>
__device__ __forceinline__ void multi_init(uint64_t (&x)[NW][2 * T], uint32_t n_kmers, const NarrowMerge &nm, int lane)
{
#pragma unroll
    for (int c = 0; c < NW; ++c) {
        const uint64_t valid = col_bits_mask(nm.col_bits[c]);
#pragma unroll
        for (int j = 0; j < 2 * T; ++j) {
            const bool ok = (uint32_t)((j % T) * 64 + lane) < n_kmers;
            x[c][j] = INV ? (ok ? ~valid : ~0ULL) : (ok ? valid : 0ULL);
        }
    }
}

// One pass of the windows over the slices of the table for the R reads of a wave (their packed block numbers in s_off[r][slot][lane]).
// NW: words per block (2: 16-byte blocks, one 16-byte gather per lookup; 4: blocks of three or four words at a stride of four, two
// gathers).  (Measured and left out, profiles/r06/negative_results.md: cache-policy bits on the gathers -- sc0 / sc1 change nothing, nt
// keeps the lines out of the L2 and costs a factor of 2.4 --, two slots per batch of gathers.)
template <int R, bool INV, int T, int NW>
__device__ __forceinline__ void multi_windows(uint64_t (&x)[R][NW][2 * T], const uint64_t (*s_off)[2 * T][64], const IbfDev &f, const PhaseCfg &ph, int lane,
                                              const uint32_t (&spill)[R])
{
    static_assert(NW == 1 || NW == 2 || NW == 4, "one- and two-word blocks, or the stride-4 layout of three- and four-word blocks");
    constexpr int S = 2 * T;
    constexpr uint32_t kBlockShift = NW == 1 ? 3u : NW == 2 ? 4u : 5u;  // log2 bytes from one block to the next
    const uint32_t slice_shift = (ph.shift >> 31) ? (0x80000000u | ((ph.shift & 0x7FFFFFFFu) << kBlockShift)) : min(31u, ph.shift + kBlockShift);
    const uint32_t table_bytes = f.n_blocks << kBlockShift;  // (< 2^26: the launcher checked)
    const uint32_t all = ph.n_slices >= 32 ? ~0u : (1u << ph.n_slices) - 1u;
    uint32_t done = 0;
    // reads whose gathers of a slot go out together: all of them where the registers allow (OR form of the two-word build: no offsets
    // kept), else one by one
    constexpr int RB = (INV && NW == 2) ? R : 1;
    constexpr int G = NW == 1 ? 1 : NW / 2;  // gathers per lookup (8 bytes for one-word blocks, else 16)
#pragma unroll 1
    while (done != all) {
        const uint32_t cur = phase_next_slice(done, ph);
        done |= 1u << cur;
        asm volatile("" ::: "memory");  // the packed offsets are read again in every window, never carried in registers
        const bool any_len = (slice_shift >> 31) != 0 && slice_shift != 0x80000000u;
        const uint32_t span0 = any_len ? (slice_shift & 0x7FFFFFFFu) : 1u << min(slice_shift, 31u);
        const uint32_t start = any_len ? cur * span0 : cur << min(slice_shift, 31u);
        // a slice ends with the table: "no lookup" lies beyond it (made scalar by hand: left to itself the compiler takes the clamp to
        // the vector unit and then wraps every gather in a readfirstlane loop over a descriptor it no longer knows to be uniform)
        const uint32_t span = (uint32_t)__builtin_amdgcn_readfirstlane((int)min(span0, table_bytes - min(start, table_bytes)));
        __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
            const_cast<char *>(reinterpret_cast<const char *>(f.words)) + start, 0, (int)span, kBufRsrcWord3);
        const uint32_t nstart = 0u - start;
#pragma unroll
        for (int u = 0; u < S; ++u) {
#pragma unroll
            for (int r0 = 0; r0 < R; r0 += RB) {
                rb_u32x4 d[RB][3][G];
                uint32_t rel[RB][3];
#pragma unroll
                for (int rr = 0; rr < RB; ++rr) {
                    const uint64_t pk = s_off[r0 + rr][u][lane];
                    const uint32_t lo = (uint32_t)pk, hi = (uint32_t)(pk >> 32);
                    // (field extract + shift-and-add of the negated slice start: seven VALU operations per k-mer)
                    if constexpr (NW == 1) {  // 22-bit numbers, the third one's top two bits from the spill word
                        rel[rr][0] = ((lo & kPackMask1) << kBlockShift) + nstart;
                        rel[rr][1] = ((__builtin_amdgcn_alignbit(hi, lo, kPackBits1) & kPackMask1) << kBlockShift) + nstart;
                        rel[rr][2] = (((hi >> (2 * kPackBits1 - 32)) | (__builtin_amdgcn_ubfe(spill[r0 + rr], 2 * u, 2) << 20)) << kBlockShift) + nstart;
                    } else {
                        rel[rr][0] = ((lo & kPackMask) << kBlockShift) + nstart;
                        rel[rr][1] = ((__builtin_amdgcn_alignbit(hi, lo, kPackBits) & kPackMask) << kBlockShift) + nstart;
                        rel[rr][2] = (__builtin_amdgcn_ubfe(hi, 2 * kPackBits - 32, kPackBits) << kBlockShift) + nstart;
                    }
#pragma unroll
                    for (int h = 0; h < 3; ++h) {
#pragma unroll
                        for (int g = 0; g < G; ++g) {  // ("no lookup" stays out of range with bit 4 set: its offset ends in zeros)
                            if constexpr (NW == 1) {
                                const rb_u32x2 w = __builtin_amdgcn_raw_buffer_load_b64(rs, rel[rr][h], 0, 0);
                                d[rr][h][g] = rb_u32x4{w.x, w.y, 0u, 0u};
                            } else {
                                d[rr][h][g] = __builtin_amdgcn_raw_buffer_load_b128(rs, rel[rr][h] | (uint32_t)(16 * g), 0, 0);
                            }
                        }
                    }
                }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int rr = 0; rr < RB; ++rr) {
#pragma unroll
                    for (int h = 0; h < 3; ++h) {
                        const uint32_t o = (!INV && rel[rr][h] >= span) ? 0xFFFFFFFFu : 0u;  // AND form: lanes that loaded nothing
#pragma unroll
                        for (int g = 0; g < G; ++g) {
                            const uint64_t w0 = (((uint64_t)(d[rr][h][g].y | o)) << 32) | (d[rr][h][g].x | o);
                            if constexpr (INV) x[r0 + rr][NW == 1 ? 0 : 2 * g][u] |= w0;
                            else x[r0 + rr][NW == 1 ? 0 : 2 * g][u] &= w0;
                            if constexpr (NW > 1) {
                                const uint64_t w1 = (((uint64_t)(d[rr][h][g].w | o)) << 32) | (d[rr][h][g].z | o);
                                if constexpr (INV) x[r0 + rr][2 * g + 1][u] |= w1;
                                else x[r0 + rr][2 * g + 1][u] &= w1;
                            }
                        }
                    }
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    }
}

// per-bin sums of one read across the wave, maxima per member
template <bool INV, int T, int NW>
__device__ __forceinline__ void multi_finish(uint64_t (&x)[NW][2 * T], const NarrowMerge &nm, int lane, uint16_t *out_row)
{
    if constexpr (INV) {
#pragma unroll
        for (int c = 0; c < NW; ++c) {
#pragma unroll
            for (int j = 0; j < 2 * T; ++j) x[c][j] = ~x[c][j];
        }
    }
    uint32_t colmax[NW];  // lane b: the larger of the two strands' counts of bin 64 c + b (at most 384 each: two share a register)
    if constexpr (NW == 1) {
        const uint32_t cf = wave_bin_counts<T>(x[0], lane), cr = wave_bin_counts<T>(x[0] + T, lane);
        colmax[0] = max(cf, cr);
    }
#pragma unroll
    for (int c = 0; c + 1 < NW; c += 2) {
        const uint32_t cf = wave_bin_counts<T>(x[c], lane) | (wave_bin_counts<T>(x[c + 1], lane) << 16);
        const uint32_t cr = wave_bin_counts<T>(x[c] + T, lane) | (wave_bin_counts<T>(x[c + 1] + T, lane) << 16);
        colmax[c] = max(cf & 0xFFFFu, cr & 0xFFFFu);
        colmax[c + 1] = max(cf >> 16, cr >> 16);
    }
    write_member_maxima<NW>(colmax, nm, lane, out_row);
}

// waves per SIMD the builds are compiled for: two-word four tiles 8 (R = 1: 50 registers) / 5 (R = 2: 91), six tiles 6; four-word 4
constexpr int multi_min_waves(int r, int t, int nw) { return nw == 1 ? (t == 4 ? 8 : 7) : nw == 4 ? (t == 4 ? RB_MULTI_WAVES_W4 : 3) : t == 4 ? (r == 1 ? 8 : RB_MULTI_WAVES) : (r == 1 ? 6 : 3); }

template <int R, bool INV, int T = 4, int NW = 2>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(multi_min_waves(R, T, NW), 8))) void ibf_count_max_phased_multi_kernel(
    IbfDev f, ReadSrc src, uint32_t n_reads, PhaseCfg ph, uint16_t *__restrict__ out, uint32_t out_read_stride, NarrowMerge nm)
{
    constexpr int S = 2 * T;  // slots per lane: the 64-k-mer tiles of forward k-mers, then those of the reverse complement
    __shared__ uint64_t s_off[R][S][64];
    if (ph.xcd_skew) ph.skew = xcc_id();
    if (ph.tskew) ph.tskew *= xcc_id();
    const int lane = threadIdx.x;
    const uint32_t read0 = blockIdx.x * (uint32_t)R;
    uint32_t nk[R];  // k-mers of each read (0: no such read, or a read longer than promised -- it writes 0 like the one-read build)
    uint32_t spill[R];  // one-word blocks: the top two bits of every slot's third block number
    constexpr int PB = NW == 1 ? (int)kPackBits1 : (int)kPackBits;
    static_assert(NW != 1 || R == 1, "the 22-bit packing is built for one read per wave");

    // ---- phase A: hash every k-mer of every read once; the block numbers go to LDS
#pragma unroll
    for (int r = 0; r < R; ++r) nk[r] = 0, spill[r] = ~0u;
#pragma unroll 1
    for (int r = 0; r < R; ++r) {
        uint32_t sp = ~0u;
        const uint32_t n = multi_hash_read<T, PB>(&s_off[r][0][0], f, src, read0 + (uint32_t)r, n_reads, lane, sp);
#pragma unroll
        for (int q = 0; q < R; ++q)
            if (q == r) nk[q] = n, spill[q] = sp;
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();

    // ---- phase B: the windows
    uint64_t x[R][NW][S];
#pragma unroll
    for (int r = 0; r < R; ++r) multi_init<INV, T, NW>(x[r], nk[r], nm, lane);
    multi_windows<R, INV, T, NW>(x, s_off, f, ph, lane, spill);

    // ---- per-bin sums across the wave, maxima per member
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const uint32_t rid = read0 + (uint32_t)r;
        if (rid >= n_reads) break;  // wave-uniform
        multi_finish<INV, T, NW>(x[r], nm, lane, out + (size_t)rid * out_read_stride);
    }
}

// the inverted twin of a merged copy (ibf_count_max_phased_multi_kernel<R, true>): dst = ~src, word by word
__global__ void invert_words_kernel(const uint64_t *__restrict__ src, uint64_t *__restrict__ dst, uint64_t n_words)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_words; i += stride) dst[i] = ~src[i];
}

// ---------------------------------------------------------------------------------------------
// The decision for read i from the raw maxima of all filters: the body of K2, also run by the latency kernel for the reads of a
// micro-batch of a one-filter engine (FoldJob).  The maxima are read past this thread's caches.
__device__ __forceinline__ uint16_t load_count(const uint16_t *p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ void decide_one(const DecideParams &P, const uint16_t *maxcount, const uint32_t *lens,
                                           const uint8_t *pre_status, uint32_t i, int mode, int32_t *out_best_target,
                                           uint8_t *out_decision, uint8_t *out_status)
{
    const uint32_t nf = P.nd + P.nt;
    // raw maximum of (this read, filter fi): the max over the partial tables of the ranks (bin-sharded), or the one table
    auto raw_max = [&](uint32_t fi) -> uint32_t {
        uint16_t m = load_count(maxcount + (size_t)i * nf + fi);
        for (uint32_t q = 1; q < P.n_parts; ++q) {
            const uint16_t v = load_count(maxcount + (size_t)q * P.part_stride + (size_t)i * nf + fi);
            m = v > m ? v : m;
        }
        return m;
    };
    if (P.maxcount_copy) {
        for (uint32_t fi = 0; fi < nf; ++fi) P.maxcount_copy[(size_t)i * nf + fi] = (uint16_t)raw_max(fi);
    }
    if (pre_status && pre_status[i] != RB_OK) {  // e.g. a chunk beyond the end of the read: no decision
        if (out_best_target) out_best_target[i] = -1;
        if (out_decision) out_decision[i] = 0;
        if (out_status) out_status[i] = pre_status[i];
        return;
    }
    const uint32_t len = lens[i];
    if (len > P.max_len) {  // the caller understated max_len: counter width and threshold table were sized for less
        if (out_best_target) out_best_target[i] = -1;
        if (out_decision) out_decision[i] = 0;
        if (out_status) out_status[i] = RB_ERR_INVALID_ARG;
        return;
    }
    const uint32_t tl = len < P.thr_len ? len : P.thr_len - 1;  // len <= max_len < thr_len
    // group maxima at r (1) and at r - 0.02 (2), strictly-greater argmax at r (first wins ties)
    uint32_t D1 = 0, T1 = 0, D2 = 0, T2 = 0;
    int best_d = -1, best_t = -1;
    for (uint32_t fi = 0; fi < nf; ++fi) {
        const uint32_t M = raw_max(fi);
        uint32_t c1 = 0, c2 = 0;
        if (len >= P.k[fi]) {  // pair overload skips filters with k > len; others count 0 there anyway
            const uint16_t t1 = P.thr[((size_t)tl * nf + fi) * 2 + 0];
            const uint16_t t2 = P.thr[((size_t)tl * nf + fi) * 2 + 1];
            c1 = (M >= t1) ? M : 0;  // max_matches with the uint16_t threshold
            c2 = (M >= t2) ? M : 0;
        }
        if (fi < P.nd) {
            if (c1 > D1) { D1 = c1; best_d = (int)fi; }
            D2 = c2 > D2 ? c2 : D2;
        } else {
            if (c1 > T1) { T1 = c1; best_t = (int)(fi - P.nd); }
            T2 = c2 > T2 ? c2 : T2;
        }
    }
    uint8_t decision = 0, status = RB_OK;
    const bool short_d = P.nd && len < P.k[0];
    const bool short_t = P.nt && len < P.k[P.nd];
    if (mode == RB_MODE_CLASSIFY_ANY) {
        // Read::classify(std::vector<TIbf>&) -> find_matches -> select_matches (IBFClassify.cpp:181-226, 81-128, 16-38):
        // true iff some filter of the list (deplete entries first, then target) holds a bin with fwd >= t or rev >= t,
        // i.e. raw max >= t with the uint16_t threshold -- a threshold of 0 makes every read a hit, 0 matches included
        // (unlike max_matches, whose result is then 0 and reads as "no match").  No k > len skip here: find_matches
        // evaluates every filter; only filters[0].kmerSize is checked (ShortReadException).
        if (nf == 0) status = RB_ERR_NULL_FILTER;
        else if (len < P.k[0]) status = RB_ERR_SHORT_READ;
        else {
            bool found = false;
            for (uint32_t fi = 0; fi < nf; ++fi) found |= raw_max(fi) >= P.thr[((size_t)tl * nf + fi) * 2 + 0];
            decision = found ? 1 : 0;
        }
    } else if (mode == RB_MODE_CHECK_UNBLOCK) {
        if (P.nd && P.nt) {
            if (D1 > 0) {
                if (T1 > 0) decision = (D2 > 0 && T2 == 0) ? 1 : 0;
                else decision = 1;
            } else {
                decision = (T1 > 0) ? 2 : 0;
            }
        } else if (P.nd) {
            if (short_d) status = RB_ERR_SHORT_READ;
            else decision = (best_d > -1) ? 1 : 0;
        } else if (P.nt) {
            if (short_t) status = RB_ERR_SHORT_READ;
            else decision = (best_t < 0) ? 1 : 2;
        } else {
            status = RB_ERR_NULL_FILTER;
        }
    } else {  // RB_MODE_CLASSIFY_CHUNK
        if (P.nd && P.nt) {
            if (T1 > 0) {
                bool want_target = false;
                if (D1 > 0) {
                    if (T2 > 0 && D2 > 0) want_target = false;
                    else if (T2 > 0) want_target = true;
                } else {
                    want_target = true;
                }
                if (want_target) {  // r.classify(TargetFilters, Conf) at the restored error rate
                    if (short_t) status = RB_ERR_SHORT_READ;
                    else decision = (best_t != -1) ? 1 : 0;
                }
            }
        } else if (P.nd) {
            if (short_d) status = RB_ERR_SHORT_READ;
            else decision = (best_d > -1) ? 1 : 0;
        } else if (P.nt) {
            if (short_t) status = RB_ERR_SHORT_READ;
            else decision = (best_t != -1) ? 1 : 0;
        } else {
            status = RB_ERR_NULL_FILTER;
        }
    }
    if (out_best_target) out_best_target[i] = (P.nt && !short_t) ? best_t : -1;
    if (out_decision) out_decision[i] = decision;
    if (out_status) out_status[i] = status;
}

// every result of the call is in place: tell the host (DecideParams::done_flag).  Called by all threads of the decision kernel after their
// reads.  The results go to page-locked HOST memory and the host stops waiting for the stream once it sees the word, so every wave
// makes its own result stores visible at system scope before the barrier (thread 0's release orders only its own wave's
// stores behind the flag; the barrier alone is a workgroup-scope matter) -- four fences per 256 reads.
__device__ __forceinline__ void announce_done(const DecideParams &P)
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
    __syncthreads();
    if (threadIdx.x != 0) return;
    if (gridDim.x > 1) {
        const uint32_t t = __hip_atomic_fetch_add(P.done_count, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
        if (t != gridDim.x - 1) return;
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        *P.done_count = 0;  // ready for the next call on this stream
    }
    __hip_atomic_store(P.done_flag, P.done_seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// latency kernel of a one-filter engine, after its body: `fin` = the read whose raw maximum this workgroup has just written, or ~0u
__device__ __forceinline__ void fold_decide(const FoldJob &job, uint32_t fin)
{
    if (!job.on || fin == ~0u || threadIdx.x != 0) return;  // thread 0 wrote the maximum
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");  // own store before own load of the same element
    decide_one(job.P, job.maxcount, job.lens, job.pre_status, fin, job.mode, job.best_target, job.decision, job.status);
    // a call of ONE read (the engine asks for the word in a folded launch only then): this thread holds the call's last result
    if (job.P.done_flag) __hip_atomic_store(job.P.done_flag, job.P.done_seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// latency form for micro-batches: `parts` workgroups per (read, column slice).  Wave w of part p takes strand w&1 and
// slot = p * (waves/2) + (w>>1) of the per-strand work: share slot % sub of the eight-step blocks of every
// (slots/sub)-th macro tile starting at slot / sub.  Partial counters meet in LDS (bit-sliced adds); with parts > 1 the
// workgroups leave their sums in a workspace and the last one to finish (ticket counter) adds them and takes the max.
// A wide filter is latency bound per read -- 2088 dependent-free gathers, but only 12-24 of them in flight per wave --
// so the way to a short kernel is more waves per read than one workgroup holds.
// blockIdx.y selects one filter of the set; all filters of a micro-batch share ONE launch whatever their geometry (a
// micro-batch against deplete + several targets would otherwise queue one short kernel per filter, 10-25 us each, and
// the short kernel of a narrow target would wait for the long one of the wide deplete filter instead of hiding in it).
// The launch has grid_parts workgroups per (read, slice); a filter that wants fewer leaves the others idle.
template <int LG, int WPL, int NP, int H, bool NT>
__device__ __forceinline__ uint32_t split_body(const IbfDev &f, uint32_t col_begin, uint32_t col_end, uint32_t parts,
                                           uint32_t sub, const ReadSrc &src, uint32_t n_reads, uint32_t n_slices,
                                           uint16_t *__restrict__ out, uint32_t out_read_stride,
                                           uint32_t out_slice_stride, uint32_t grid_parts, uint64_t *__restrict__ ws,
                                           uint32_t *__restrict__ tickets, uint8_t *s_dyn)
{
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int n_waves = blockDim.x >> 6;
    const int wps = n_waves >> 1;  // waves per strand in this workgroup
    const int strand = wave & 1, lslot = wave >> 1;
    const uint32_t item = blockIdx.x / grid_parts;
    const uint32_t part = blockIdx.x - item * grid_parts;
    if (part >= parts) return ~0u;  // workgroup-uniform: this filter uses fewer workgroups per read than the launch has
    const uint32_t read = item / n_slices;
    const uint32_t slice = item - read * n_slices;
    const uint32_t slots = (uint32_t)wps * parts;  // per strand, over all parts
    const uint32_t slot = part * (uint32_t)wps + (uint32_t)lslot;

    uint64_t *s_planes = reinterpret_cast<uint64_t *>(s_dyn);  // [wave][WPL][NP][64]
    uint32_t *s_max = reinterpret_cast<uint32_t *>(s_dyn + (size_t)n_waves * WPL * NP * 64 * 8);  // [0..1] maxima, [2] ticket
    uint8_t *stage = s_dyn + (size_t)n_waves * WPL * NP * 64 * 8 + 16 + (size_t)wave * kStageBytes;

    const LaneCols<WPL> lc = make_lane_cols<LG, WPL>(f, lane, col_begin, col_end, slice);
    uint32_t len;
    const BaseSrc seq = make_base_src(src, read, &len);
    const uint32_t n = len >= f.k ? len - f.k + 1 : 0;
    constexpr uint32_t ITEMS = TileShape<LG>::ITEMS;
    constexpr int BPT = TileShape<LG>::STEPS / 8;  // eight-step blocks per macro tile
    const int bps = BPT / (int)sub;                // ... per share (sub divides BPT and slots)
    const int sb = (int)(slot % sub);

    Planes<NP> pl[WPL];
#pragma unroll
    for (int w = 0; w < WPL; ++w) pl[w].clear();
    count_strand<LG, WPL, NP, H, NT>(pl, f, lc, seq, len, n, strand, (slot / sub) * ITEMS, (slots / sub) * ITEMS, sb * bps,
                                     (sb + 1) * bps, stage, lane);

    if (lslot != 0) {
#pragma unroll
        for (int w = 0; w < WPL; ++w)
#pragma unroll
            for (int i = 0; i < NP; ++i) s_planes[(((size_t)wave * WPL + w) * NP + i) * 64 + lane] = pl[w].p[i];
    }
    __syncthreads();
    const size_t gitem = (size_t)blockIdx.y * ((size_t)n_reads * n_slices) + item;
    if (lslot == 0) {
        for (int o = 1; o < wps; ++o) {
            const int ow = (o << 1) | strand;
#pragma unroll
            for (int w = 0; w < WPL; ++w) {
                uint64_t carry = 0;
#pragma unroll
                for (int i = 0; i < NP; ++i) {
                    const uint64_t other = s_planes[(((size_t)ow * WPL + w) * NP + i) * 64 + lane];
                    uint64_t h, l;
                    RB_CSA(h, l, pl[w].p[i], other, carry);
                    pl[w].p[i] = l;
                    carry = h;
                }
            }
        }
        if (parts == 1) {
            const uint32_t m = planes_max<NP, WPL>(pl, lc.valid);
            if (lane == 0) s_max[strand] = m;
        } else {
            uint64_t *dst = ws + ((gitem * grid_parts + part) * 2 + (size_t)strand) * (2 * NP * 64);
#pragma unroll
            for (int w = 0; w < WPL; ++w)
#pragma unroll
                for (int i = 0; i < NP; ++i) dst[(w * NP + i) * 64 + lane] = pl[w].p[i];
        }
    }
    __syncthreads();
    if (parts > 1) {
        // The last workgroup of this (read, slice, filter) to arrive owns the result.  One agent-scope release per
        // workgroup (the barrier above orders the other waves' stores before it) and one acquire in the last one (the
        // barrier below orders it before the other waves' loads): on gfx950 a release writes the XCD's L2 back, which
        // costs about a microsecond and serialises per XCD -- fences per wave made 64-read batches 2.4x slower.
        if (threadIdx.x == 0) {
            const uint32_t t = __hip_atomic_fetch_add(&tickets[gitem], 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
            if (t == parts - 1) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            s_max[2] = t;
        }
        __syncthreads();
        if (s_max[2] != parts - 1) return ~0u;  // workgroup-uniform
        if (lslot == 0) {
#pragma unroll
            for (int w = 0; w < WPL; ++w) pl[w].clear();
            for (uint32_t q = 0; q < parts; ++q) {
                const uint64_t *srcp = ws + ((gitem * grid_parts + q) * 2 + (size_t)strand) * (2 * NP * 64);
#pragma unroll
                for (int w = 0; w < WPL; ++w) {
                    uint64_t carry = 0;
#pragma unroll
                    for (int i = 0; i < NP; ++i) {
                        const uint64_t other = srcp[(w * NP + i) * 64 + lane];
                        uint64_t h, l;
                        RB_CSA(h, l, pl[w].p[i], other, carry);
                        pl[w].p[i] = l;
                        carry = h;
                    }
                }
            }
            const uint32_t m = planes_max<NP, WPL>(pl, lc.valid);
            if (lane == 0) s_max[strand] = m;
        }
        __syncthreads();
        if (threadIdx.x == 0) tickets[gitem] = 0;  // ready for the next launch on this stream
    }
    if (threadIdx.x == 0) {
        const uint32_t a = s_max[0], b = s_max[1];
        out[(size_t)read * out_read_stride + (size_t)slice * out_slice_stride] = (uint16_t)(a > b ? a : b);
    }
    return item;  // the (read, slice) this workgroup has written (a FoldJob implies one slice: item = read)
}


// filters of ONE kernel geometry (single-filter engines, several targets of equal width): the body alone, with the
// workgroup size its register budget allows
template <int LG, int WPL, int NP, int H, bool NT>
__global__ __launch_bounds__(WPL == 2 ? (NP > 10 ? 512 : 768) : (LG == 0 ? 512 : 1024)) void ibf_count_max_split_kernel(
    FilterSet set, ReadSrc src, uint32_t n_reads, uint32_t n_slices, uint16_t *__restrict__ out_base,
    uint32_t out_read_stride, uint32_t out_slice_stride, uint32_t grid_parts, uint64_t *__restrict__ ws,
    uint32_t *__restrict__ tickets, FoldJob job)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t s_dyn[];
    const uint32_t fin = split_body<LG, WPL, NP, H, NT>(set.f[blockIdx.y], set.col_begin[blockIdx.y], set.col_end[blockIdx.y],
                                                        set.parts[blockIdx.y], set.sub[blockIdx.y], src, n_reads, n_slices,
                                                        out_base + set.out_offset[blockIdx.y], out_read_stride, out_slice_stride,
                                                        grid_parts, ws, tickets, s_dyn);
    fold_decide(job, fin);
}

// filters of DIFFERENT geometries in one launch (deplete = human genome, targets = a few small genomes): the geometry
// of the filter picked by blockIdx.y selects the body (workgroup-uniform branch).  Built for 512 threads: with all
// bodies in one function the scalar state of sixteen specialisations spills into vector registers, and at 768+
// threads that pushes the widest bodies over the budget.
template <int NP, bool WIDE>
__global__ __launch_bounds__(512) void ibf_count_max_split_any_kernel(
    FilterSet set, ReadSrc src, uint32_t n_reads, uint32_t n_slices, uint16_t *__restrict__ out_base,
    uint32_t out_read_stride, uint32_t out_slice_stride, uint32_t grid_parts, uint64_t *__restrict__ ws,
    uint32_t *__restrict__ tickets, FoldJob job)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t s_dyn[];
    uint32_t fin = ~0u;
    const IbfDev &f = set.f[blockIdx.y];
    const uint32_t col_begin = set.col_begin[blockIdx.y], col_end = set.col_end[blockIdx.y];
    uint16_t *__restrict__ out = out_base + set.out_offset[blockIdx.y];
    const uint32_t parts = set.parts[blockIdx.y], sub = set.sub[blockIdx.y];
#define RB_SPLIT_CASE(LG_, WPL_)                                                                                          \
    case (LG_) | ((WPL_) == 2 ? 8 : 0):                                                                                    \
        fin = split_body<LG_, WPL_, NP, 3, false>(f, col_begin, col_end, parts, sub, src, n_reads, n_slices, out,          \
                                                  out_read_stride, out_slice_stride, grid_parts, ws, tickets, s_dyn);      \
        break;                                                                                                             \
    case (LG_) | ((WPL_) == 2 ? 8 : 0) | 16:                                                                               \
        fin = split_body<LG_, WPL_, NP, 3, true>(f, col_begin, col_end, parts, sub, src, n_reads, n_slices, out,           \
                                                 out_read_stride, out_slice_stride, grid_parts, ws, tickets, s_dyn);       \
        break;
    switch (set.geom[blockIdx.y]) {
        RB_SPLIT_CASE(0, 1)
        RB_SPLIT_CASE(1, 1)
        RB_SPLIT_CASE(2, 1)
        RB_SPLIT_CASE(3, 1)
        RB_SPLIT_CASE(4, 1)
        RB_SPLIT_CASE(5, 1)
        RB_SPLIT_CASE(6, 1)
    default:
        if constexpr (WIDE) {
            switch (set.geom[blockIdx.y]) {
                RB_SPLIT_CASE(6, 2)
            default: break;
            }
        }
        break;
    }
#undef RB_SPLIT_CASE
    fold_decide(job, fin);
}

// combine the per-slice partial maxima of one filter: part[slice][read] -> maxcount[read*nf + f]
__global__ void reduce_slices_kernel(const uint16_t *__restrict__ part, uint32_t n_slices, uint32_t n_reads,
                                     uint16_t *__restrict__ maxcount, uint32_t nf, uint32_t fidx)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_reads) return;
    uint16_t m = 0;
    for (uint32_t s = 0; s < n_slices; ++s) {
        const uint16_t v = part[(size_t)s * n_reads + i];
        m = v > m ? v : m;
    }
    maxcount[(size_t)i * nf + fidx] = m;
}

// ---------------------------------------------------------------------------------------------
// on-GPU chunking (classify.hpp:264-271): work item i looks at bases [chunk_start, min(chunk_start+chunk_len, len)) of
// its read; a chunk that starts beyond the read's end is the reference's undefined infix -> RB_ERR_BAD_CHUNK
__global__ void chunk_prep_kernel(const uint32_t *__restrict__ lens, const uint32_t *__restrict__ ids, uint32_t n_items,
                                  uint32_t chunk_start, uint32_t chunk_len, uint32_t *__restrict__ eff_lens,
                                  uint8_t *__restrict__ pre_status)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_items) return;
    const uint32_t len = lens[ids ? ids[i] : i];
    const bool bad = chunk_start > len;
    const uint32_t rest = bad ? 0u : len - chunk_start;
    eff_lens[i] = (chunk_len && chunk_len < rest) ? chunk_len : rest;
    pre_status[i] = bad ? (uint8_t)RB_ERR_BAD_CHUNK : (uint8_t)RB_OK;
}

// K2: one thread per read.
__global__ void decide_kernel(DecideParams P, const uint16_t *__restrict__ maxcount, const uint32_t *__restrict__ lens,
                              const uint8_t *__restrict__ pre_status, uint32_t n_reads, int mode,
                              int32_t *__restrict__ out_best_target, uint8_t *__restrict__ out_decision,
                              uint8_t *__restrict__ out_status)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_reads) decide_one(P, maxcount, lens, pre_status, i, mode, out_best_target, out_decision, out_status);
    if (P.done_flag) announce_done(P);  // (kernel argument: uniform)
}

// ---------------------------------------------------------------------------------------------
// K4: one thread per (fragment, k-mer position); h atomicOr per k-mer.
__global__ void ibf_insert_kernel(IbfDev f, uint64_t *__restrict__ words, const uint8_t *__restrict__ seq,
                                  const uint64_t *__restrict__ starts, const uint64_t *__restrict__ ends,
                                  const uint64_t *__restrict__ bins, const uint64_t *__restrict__ kmer_prefix,
                                  uint32_t n_fragments, uint64_t total_kmers)
{
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= total_kmers) return;
    // fragment lookup: kmer_prefix[i] = number of k-mers in fragments < i (binary search)
    uint32_t lo = 0, hi = n_fragments;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (kmer_prefix[mid] <= t) lo = mid; else hi = mid;
    }
    const uint64_t pos = starts[lo] + (t - kmer_prefix[lo]);
    if (pos + f.k > ends[lo]) return;
    uint64_t v = 0;
    for (uint32_t i = 0; i < f.k; ++i) v = v * 5u + rbspec::dna5_ord(seq[pos + i]);
    const uint64_t bin = bins[lo];
    for (uint32_t h = 0; h < f.n_hash; ++h) {
        const uint64_t blk = rbspec::block_index(v, f.precalc[h], f.n_blocks, f.magic, f.pow2_mask);
        const uint64_t bit = blk * ((uint64_t)f.stride * 64u) + bin;  // padded HBM layout
        atomicOr(reinterpret_cast<unsigned long long *>(words + (bit >> 6)), 1ULL << (bit & 63));
    }
}

// Re-stride a block matrix: block b = src[b*s_src .. +w_copy) -> dst[b*s_dst .. +w_copy), the rest of each destination
// block (s_dst - w_copy words) is zero.  Serves resizeBins (wider blocks, new bins empty), the padded HBM layout
// (file layout -> aligned blocks) and the way back (download).
__global__ void restride_blocks_kernel(const uint64_t *__restrict__ src, uint32_t s_src, uint64_t *__restrict__ dst,
                                       uint32_t s_dst, uint32_t w_copy, uint64_t n_blocks)
{
    const uint64_t total = n_blocks * s_dst;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const uint64_t b = i / s_dst;
        const uint32_t c = (uint32_t)(i - b * s_dst);
        dst[i] = c < w_copy ? src[b * s_src + c] : 0ULL;
    }
}

// first-contact check (rb_dibf_compare): bit statistics of two filters of one geometry -- out[0] = bits set in a,
// out[1] = bits set in b, out[2] = bits set in b but not in a.  One 64-bit atomic per wave.
__global__ void compare_bits_kernel(const uint64_t *__restrict__ a, const uint64_t *__restrict__ b, uint64_t n_words,
                                    unsigned long long *__restrict__ out)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    uint64_t sa = 0, sb = 0, snew = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_words; i += stride) {
        const uint64_t x = a[i], y = b[i];
        sa += (uint64_t)__popcll(x);
        sb += (uint64_t)__popcll(y);
        snew += (uint64_t)__popcll(y & ~x);
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        sa += shfl64(sa, (threadIdx.x & 63) ^ m);
        sb += shfl64(sb, (threadIdx.x & 63) ^ m);
        snew += shfl64(snew, (threadIdx.x & 63) ^ m);
    }
    if ((threadIdx.x & 63) == 0) {
        atomicAdd(out + 0, (unsigned long long)sa);
        atomicAdd(out + 1, (unsigned long long)sb);
        atomicAdd(out + 2, (unsigned long long)snew);
    }
}

// word w of the FILE layout (block w / bin_width, column w % bin_width) gets synth_word(seed, w); it is stored at the
// padded position of that block
__global__ void fill_synth_kernel(uint64_t *__restrict__ words, uint64_t used_words, uint32_t bin_width, uint32_t stride_words,
                                  uint64_t last_mask, uint64_t seed)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t w = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; w < used_words; w += stride) {
        const uint64_t b = w / bin_width;
        const uint32_t c = (uint32_t)(w - b * bin_width);
        uint64_t x = rbspec::synth_word(seed, w);
        if (c == bin_width - 1) x &= last_mask;
        words[b * stride_words + c] = x;
    }
}

// synthetic batch for rb_engine_calibrate: n_reads reads of read_len uniform ACGT bases, back to back
__global__ void fill_reads_kernel(uint8_t *__restrict__ seqs, uint64_t *__restrict__ offsets, uint32_t *__restrict__ lens, uint64_t n_reads,
                                  uint32_t read_len, uint64_t seed)
{
    const uint64_t total = n_reads * read_len;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        // 32 bases per 64-bit word of a UNIFORM mixer (not synth_word: its bits are set with the filters' design load, 0.215 -- reads
        // of 62 % A would repeat their k-mers, hit the caches and mislead the calibration: round 4 saw it pick windows that were 13 %
        // slower on real reads)
        const uint64_t w = rbspec::mix64(seed + ((i >> 5) + 1) * 0x9E3779B97F4A7C15ULL);
        seqs[i] = (uint8_t)"ACGT"[(w >> ((i & 31u) * 2u)) & 3u];
        if (i < n_reads) {
            offsets[i] = i * read_len;
            lens[i] = read_len;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Per-bin occupancy of a resident filter (rb_dibf_bin_occupancy): out[j] += number of blocks whose bit j is set -- the column
// sums of the block-major bit matrix, read once from the filter's own device image.  The vertical-counter problem of K1 without
// the gathers: a lane keeps WPL word columns and walks DOWN the blocks; eight rows at a time go through the Harley-Seal tree of
// Planes::add8 into lane-private planes (about one carry-save step per loaded word, no per-bit work, no LDS, no atomics in the loop).
//   * A workgroup owns a column slice of 64 * WPL words of every block (WPL 2: 16-byte lanes for strides that are multiples of
//     16 words; WPL 1: 8-byte lanes for the power-of-two strides below).  A slice narrower than a wave row -- strides of 1 to 8
//     words, the 16 ... 112 words a stride leaves behind its last full slice -- is covered by 2^lg lanes per block, and the wave
//     takes 64 >> lg blocks per load instruction: lane's column = (lane mod 2^lg) * WPL, fixed for the whole walk.
//   * Loads: 16 / WPL wave rows (8 KiB per wave) go out together, no control flow between them, a schedule fence before the first use.
//     Every 128-byte line of the table is requested once; a lane whose words are all padding loads nothing (its neighbours
//     fetch the line), pad words and the bits at or beyond n_bins are masked when the planes are flushed.
//   * Flush: a wave walks at most kOccMaxChunkRows < 2^kOccPlanes rows, then expands its planes (64 bins x kOccPlanes bits per lane
//     word) into the workgroup's u32 counters in LDS and clears them.  When the workgroup has walked all its chunks, one 64-bit
//     atomicAdd per non-empty bin carries the counters to `out` (integer sums: the order does not matter).  DESIGN 4.6 has the
//     instruction shares.
// The launcher sizes the grid to one workgroup of 16 waves per CU.
constexpr int kOccPlanes = 12;
constexpr int kOccWaves = 16;                  // waves per workgroup
constexpr uint32_t kOccMaxChunkRows = 4080;    // wave rows between two flushes: the largest multiple of 16 below 2^kOccPlanes
constexpr uint32_t kOccMinChunkRows = 256;     // ... and no grid so large that a wave walks fewer (the flush is a fixed cost per chunk)
static_assert(kOccMaxChunkRows < (1u << kOccPlanes) && kOccMaxChunkRows % 16 == 0, "a chunk must not wrap the planes");

// counters += one one-bit-per-bin word (ripple add; the rows behind the last full batch of a chunk)
template <int NP>
__device__ __forceinline__ void planes_add1(Planes<NP> &pl, uint64_t x)
{
    uint64_t carry = x;
#pragma unroll
    for (int i = 0; i < NP; ++i) {
        const uint64_t t = pl.p[i] & carry;
        pl.p[i] ^= carry;
        carry = t;
    }
}

template <int WPL, bool NT>
__global__ __launch_bounds__(64 * kOccWaves) void ibf_bin_occupancy_kernel(OccLaunch a, unsigned long long *__restrict__ out)
{
    constexpr int RW = 64 * WPL;  // word columns of a slice
    constexpr int B = 16 / WPL;   // wave rows per batch of loads
    __shared__ uint32_t cnt[RW * 64];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));  // (uniform: the walk below is scalar)
    for (uint32_t i = threadIdx.x; i < (uint32_t)RW * 64u; i += blockDim.x) cnt[i] = 0;
    __syncthreads();

    const uint32_t slice = blockIdx.x / a.wgs_per_slice, wg = blockIdx.x - slice * a.wgs_per_slice;
    const uint64_t col_begin = (uint64_t)slice * RW;
    const uint32_t width = (uint32_t)min((uint64_t)RW, a.stride - col_begin);  // words of this slice per block, padding included
    uint32_t lg = 0;
    while ((uint32_t)WPL << lg < width) ++lg;  // lanes per block: the next power of two that holds the slice
    const uint32_t ng = 64u >> lg;             // blocks per wave row
    const uint32_t c = lane & ((1u << lg) - 1u), g = lane >> lg;
    const uint64_t col0 = col_begin + (uint64_t)c * WPL;
    uint64_t valid[WPL];
    bool active = false;
#pragma unroll
    for (int w = 0; w < WPL; ++w) {
        const uint64_t col = col0 + w;
        const uint32_t rem = a.n_bins & 63u;
        valid[w] = col >= a.bin_width ? 0ULL : (col == a.bin_width - 1 && rem) ? ((1ULL << rem) - 1) : ~0ULL;
        active |= valid[w] != 0;
    }
    const uint64_t n_rows = (a.n_blocks + ng - 1) / ng;  // wave rows of this slice
    const uint64_t n_full = a.n_blocks / ng;             // ... of which these hold a block for every lane group
    const uint64_t step = (uint64_t)ng * a.stride;       // words from one wave row to the next
    // a lane's place inside a wave row, in words: below 2^32 (g > 0 only for strides of at most 64 words; a block has fewer than 2^25)
    const uint32_t lane_off = (uint32_t)(g * a.stride + col0);

    for (uint32_t it = 0; it < a.iters; ++it) {
        const uint64_t chunk = ((uint64_t)it * a.wgs_per_slice + wg) * kOccWaves + wave;
        const uint64_t i0 = chunk * a.chunk_rows;
        if (i0 >= n_rows) break;  // (wave-uniform)
        const uint64_t i1 = min(i0 + a.chunk_rows, n_rows), f1 = min(i1, n_full);
        if (!active) continue;
        Planes<kOccPlanes> pl[WPL];
#pragma unroll
        for (int w = 0; w < WPL; ++w) pl[w].clear();
        const uint64_t *p = a.words + i0 * step;  // (uniform) first word of wave row i
        uint64_t i = i0;
#pragma unroll 1
        for (; i + B <= f1; i += B, p += B * step) {
            if constexpr (WPL == 2) {
                rb_u64x2 v[B];
#pragma unroll
                for (int j = 0; j < B; ++j) v[j] = load_word2<NT>(p + j * step + lane_off);
                __builtin_amdgcn_sched_barrier(0);
                uint64_t x0[8], x1[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    x0[j] = v[j].x;
                    x1[j] = v[j].y;
                }
                pl[0].add8(x0);
                pl[1].add8(x1);
            } else {
                uint64_t x[B];
#pragma unroll
                for (int j = 0; j < B; ++j) x[j] = load_word<NT>(p + j * step + lane_off);
                __builtin_amdgcn_sched_barrier(0);
                pl[0].add8(x);
                pl[0].add8(x + 8);
            }
        }
        // the rows behind the last full batch, and the wave row that holds fewer than ng blocks
#pragma unroll 1
        for (; i < i1; ++i, p += step) {
            const bool ok = i * ng + g < a.n_blocks;
#pragma unroll
            for (int w = 0; w < WPL; ++w) planes_add1(pl[w], ok ? load_word<NT>(p + lane_off + w) : 0ULL);
        }
        // flush: planes -> the workgroup's counters.  Word column lc of the slice keeps its 64 bins at cnt[lc * 64 ...], rotated by
        // the lane's column number so that the 64 lanes of a full-width slice hit 64 different banks
#pragma unroll
        for (int w = 0; w < WPL; ++w) {
            uint32_t lo[kOccPlanes], hi[kOccPlanes];
#pragma unroll
            for (int q = 0; q < kOccPlanes; ++q) {
                const uint64_t m = pl[w].p[q] & valid[w];
                lo[q] = (uint32_t)m;
                hi[q] = (uint32_t)(m >> 32);
            }
            uint32_t *dst = cnt + (c * WPL + w) * 64u;
#pragma unroll 2
            for (uint32_t b = 0; b < 32; ++b) {
                uint32_t v0 = 0, v1 = 0;
#pragma unroll
                for (int q = 0; q < kOccPlanes; ++q) {
                    v0 |= ((lo[q] >> b) & 1u) << q;
                    v1 |= ((hi[q] >> b) & 1u) << q;
                }
                atomicAdd(dst + ((b + c) & 63u), v0);
                atomicAdd(dst + ((b + 32u + c) & 63u), v1);
            }
        }
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < (uint32_t)RW * 64u; i += blockDim.x) {
        const uint32_t v = cnt[i];
        const uint32_t lc = i >> 6;
        const uint64_t bin = (col_begin + lc) * 64u + (((i & 63u) - lc / WPL) & 63u);
        if (v != 0 && bin < a.n_bins) atomicAdd(out + bin, (unsigned long long)v);
    }
}

// ---------------------------------------------------------------------------------------------
// Assembling a filter from bins of others (rb_dibf_assemble): out bin j of every block = OR of the source bits its list names.
// The plan is the same for every block, so it is read ONCE per workgroup and held in registers while the workgroup walks blocks:
//   * A workgroup (kAsmWaves waves) owns a TILE of up to kAsmTileWords out words (4 096 out bins) of every block of its chunks.
//     A wave holds the lists of `ow` = ceil(tile words / kAsmWaves) consecutive out words: lane = out bin of the word, up to
//     kAsmHeld refs per bin, each already translated to (word of the staged image << 6 | bit) -- 0 names the image's zero word,
//     so an absent ref needs no test.  A tile narrower than kAsmWaves words leaves waves over: they take further blocks
//     (`gpw` block groups per workgroup), every wave takes `kb` consecutive blocks per round, and a step has as many
//     rounds as its LDS image (about 32 KiB) holds: the loads of a whole step are in flight together.
//   * Per step the workgroup stages, for each of its gpw * kb blocks, the WINDOW of every source block that the tile's lists name
//     (AsmWindow: words [lo, lo + n); the host derives it from the plan, so an identity, a merge or a reversal stage exactly the
//     words they use and a source block is fetched once) into LDS: one global load per word, 2^lg lanes per block like the
//     occupancy pass.  Then lane ORs its refs' bits out of LDS (the r loop runs to the wave's longest held list, uniform), one
//     __ballot per out word -- every lane of the wave is inside it: all control flow around it is wave-uniform -- is the out
//     word, which lane k * ow + j keeps; one store per wave and step writes ow * kb words.
//   * Lists longer than kAsmHeld walk refs[] in memory behind the held part, to the wave's longest list (a ballot is the loop
//     condition; the loads are predicated per lane).
//   * Out words at or beyond ceil(n_out_bins / 64) (the pad of the stride) and bins at or beyond n_out_bins have no list: their
//     ballots are zero, so the image comes out padded with zeros without a pass of its own.
// All table addresses are 64-bit word numbers.  DESIGN 4.9 has the resources.
struct AsmShape { uint32_t ow, wpb, gpw, kb, rounds; };
__host__ __device__ inline AsmShape asm_shape(uint32_t tile_words, uint32_t staged_words)
{
    AsmShape s;
    s.ow = (tile_words + kAsmWaves - 1) / kAsmWaves;
    s.wpb = (tile_words + s.ow - 1) / s.ow;
    s.gpw = kAsmWaves / s.wpb;
    const uint32_t room = kAsmMaxLdsWords / staged_words;  // (>= 1: the host refuses wider windows)
    if (s.gpw > room) s.gpw = room;
    uint32_t kb = kAsmStepLdsWords / (s.gpw * staged_words);
    if (kb < 1) kb = 1;
    if (kb > 64u / s.ow) kb = 64u / s.ow;
    s.kb = kb;
    // ... and as many rounds of gpw * kb blocks per step as the step's LDS holds: the loads of a step are what is in flight
    uint32_t rounds = kAsmStepLdsWords / (s.gpw * kb * staged_words);
    if (rounds < 1) rounds = 1;
    if (rounds > 16) rounds = 16;
    s.rounds = rounds;
    return s;
}

template <bool NT>
__device__ __forceinline__ void store_word(uint64_t *p, uint64_t v)
{
    if constexpr (NT) __builtin_nontemporal_store(v, p);
    else *p = v;
}

// the OR phase of a full-width wave (kAsmOutWords out words), lists of at most R held refs: all R * kAsmOutWords LDS reads of a block
// go out with no control flow between them, so the out words do not wait for one another's read.  An absent ref is 0 = the zero word.
template <int R>
__device__ __forceinline__ void asm_or_words(const uint64_t *blk, const uint32_t (&held)[kAsmOutWords][kAsmHeld], uint64_t (&acc)[kAsmOutWords])
{
#pragma unroll
    for (uint32_t j = 0; j < kAsmOutWords; ++j) acc[j] = 0;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        // ref r of all the out words: the refs are decoded here, every time (hoisted out of the block loop the word numbers and shifts
        // would triple the registers), behind empty asm statements that come BEFORE the batch's reads, not between them
        // (four reads at a time: eight more live words spill)
#pragma unroll
        for (uint32_t j0 = 0; j0 < kAsmOutWords; j0 += 4) {
            uint32_t e[4];
            uint64_t w[4];
#pragma unroll
            for (uint32_t j = 0; j < 4; ++j) {
                e[j] = held[j0 + j][r];
                asm volatile("" : "+v"(e[j]));
            }
#pragma unroll
            for (uint32_t j = 0; j < 4; ++j) w[j] = blk[e[j] >> 6];
#pragma unroll
            for (uint32_t j = 0; j < 4; ++j) acc[j0 + j] |= w[j] >> (e[j] & 63u);
        }
    }
}

template <bool NT>
__global__ __launch_bounds__(64 * kAsmWaves, 4) void ibf_assemble_kernel(AsmLaunch a)
{
    extern __shared__ uint64_t asm_img[];  // gpw * kb staged blocks of `sw` words: [zero word | window of source 0 | window of source 1 ...]
    __shared__ uint32_t s_base[kAsmMaxSources], s_lo[kAsmMaxSources], s_n[kAsmMaxSources], s_lg[kAsmMaxSources], s_sw;
    __shared__ const uint64_t *s_src[kAsmMaxSources];
    __shared__ uint64_t s_stride[kAsmMaxSources];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t tile = blockIdx.x % a.n_tiles, wg = blockIdx.x / a.n_tiles;
    const uint64_t t0 = (uint64_t)tile * kAsmTileWords;
    const uint32_t tw = (uint32_t)min((uint64_t)kAsmTileWords, a.out_stride - t0);
    if (threadIdx.x == 0) {
        uint32_t base = 1;
#pragma unroll
        for (uint32_t s = 0; s < kAsmMaxSources; ++s) {
            AsmWindow w{0, 0};
            if (s < a.n_srcs) w = a.windows[(uint64_t)tile * kAsmMaxSources + s];
            uint32_t lg = 0;
            while ((1u << lg) < w.n && lg < 6) ++lg;
            s_base[s] = base;
            s_lo[s] = w.lo;
            s_n[s] = w.n;
            s_lg[s] = lg;
            s_src[s] = a.src[s];
            s_stride[s] = a.src_stride[s];
            base += w.n;
        }
        s_sw = base;
    }
    __syncthreads();
    const uint32_t sw = (uint32_t)__builtin_amdgcn_readfirstlane((int)s_sw);
    const AsmShape sh = asm_shape(tw, sw);
    const uint32_t ow = sh.ow, kb = sh.kb, nb = sh.gpw * sh.kb * sh.rounds;
    for (uint32_t i = threadIdx.x; i < nb; i += blockDim.x) asm_img[(uint64_t)i * sw] = 0ULL;

    // the wave's lists, once for all blocks
    const uint32_t grp = wave / sh.wpb, wq_in = (wave - grp * sh.wpb) * ow;  // (uniform)
    const bool wave_on = grp < sh.gpw;
    uint32_t held[kAsmOutWords][kAsmHeld];
    uint32_t held_len = 0;    // 4 bits per out word: the wave's longest held list
    uint32_t spill_mask = 0;  // out words with a list beyond kAsmHeld somewhere in the wave
#pragma unroll
    for (uint32_t j = 0; j < kAsmOutWords; ++j) {
        const uint64_t bin = (t0 + wq_in + j) * 64u + lane;
        uint64_t o0 = 0;
        uint32_t n = 0;
        if (wave_on && j < ow && wq_in + j < tw && bin < a.n_out_bins) {
            o0 = a.offsets[bin];
            n = (uint32_t)(a.offsets[bin + 1] - o0);
        }
#pragma unroll
        for (uint32_t r = 0; r < kAsmHeld; ++r) {
            held[j][r] = 0;
            if (r < n) {
                const uint2 rf = a.refs[o0 + r];
                held[j][r] = ((s_base[rf.x] + (rf.y >> 6) - s_lo[rf.x]) << 6) | (rf.y & 63u);
            }
            if (__ballot(r < n) != 0ULL) held_len += 1u << (4u * j);
        }
        if (__ballot(n > kAsmHeld) != 0ULL) spill_mask |= 1u << j;
    }
    held_len = (uint32_t)__builtin_amdgcn_readfirstlane((int)held_len);
    spill_mask = (uint32_t)__builtin_amdgcn_readfirstlane((int)spill_mask);
    uint32_t max_len = 0;  // the longest held list of the wave's out words
#pragma unroll
    for (uint32_t j = 0; j < kAsmOutWords; ++j) max_len = max(max_len, (held_len >> (4u * j)) & 15u);
    const bool full_wave = ow == kAsmOutWords;
    const uint32_t lane_k = lane / ow, lane_j = lane - lane_k * ow;  // the (block, out word) whose result this lane stores

    for (uint32_t it = 0; it < a.iters; ++it) {
        const uint64_t chunk = (uint64_t)it * a.wgs_per_tile + wg;
        const uint64_t cb = chunk * a.blocks_per_chunk;
        if (cb >= a.n_blocks) break;
        const uint64_t ce = min(cb + a.blocks_per_chunk, a.n_blocks);
#pragma unroll 1
        for (uint64_t b0 = cb; b0 < ce; b0 += nb) {
            const uint32_t nbe = (uint32_t)min((uint64_t)nb, ce - b0);
            __syncthreads();  // the step before has been read
            for (uint32_t s = 0; s < a.n_srcs; ++s) {
                const uint32_t ns = s_n[s];
                if (ns == 0) continue;
                const uint32_t lg = s_lg[s], per_row = 64u >> lg;
                const uint32_t q = lane >> lg, c0 = lane & ((1u << lg) - 1u);
                const uint64_t stride = s_stride[s];
                const uint64_t *sp = s_src[s] + s_lo[s];
                uint64_t *dp = asm_img + s_base[s];
                // four loads per lane go out before the first of them is written to LDS
                for (uint32_t c = c0; c < ns; c += 1u << lg) {
                    for (uint32_t bb = wave * per_row + q; bb < nbe; bb += 4u * kAsmWaves * per_row) {
                        uint64_t v[4];
#pragma unroll
                        for (uint32_t u = 0; u < 4; ++u) {
                            const uint32_t b = bb + u * kAsmWaves * per_row;
                            v[u] = b < nbe ? load_word<NT>(sp + (b0 + b) * stride + c) : 0ULL;
                        }
#pragma unroll
                        for (uint32_t u = 0; u < 4; ++u) {
                            const uint32_t b = bb + u * kAsmWaves * per_row;
                            if (b < nbe) dp[(uint64_t)b * sw + c] = v[u];
                        }
                    }
                }
            }
            __syncthreads();
            if (!wave_on) continue;
#pragma unroll 1
            for (uint32_t round = 0; round < sh.rounds; ++round) {
            const uint32_t first = (round * sh.gpw + grp) * kb;  // the kb consecutive blocks of this wave in this round
            if (first >= nbe) break;  // (uniform)
            uint64_t keep = 0;
#pragma unroll 1
            for (uint32_t k = 0; k < kb; ++k) {
                const uint32_t bsub = first + k;
                if (bsub >= nbe) break;  // (uniform)
                const uint64_t *blk = asm_img + (uint64_t)bsub * sw;
                uint64_t accs[kAsmOutWords];
                if (full_wave) {  // (uniform) one branch per block, none between the reads
                    if (max_len <= 1) asm_or_words<1>(blk, held, accs);
                    else if (max_len <= 2) asm_or_words<2>(blk, held, accs);
                    else if (max_len <= 4) asm_or_words<4>(blk, held, accs);
                    else asm_or_words<8>(blk, held, accs);
                } else {
#pragma unroll
                    for (uint32_t j = 0; j < kAsmOutWords; ++j) {
                        accs[j] = 0;
                        if (j >= ow) continue;  // (uniform)
                        const uint32_t len = (held_len >> (4u * j)) & 15u;
#pragma unroll
                        for (uint32_t r = 0; r < kAsmHeld; ++r) {
                            if (r < len) {  // (uniform guard: the wave's longest list)
                                uint32_t e = held[j][r];
                                asm volatile("" : "+v"(e));
                                accs[j] |= blk[e >> 6] >> (e & 63u);
                            }
                        }
                    }
                }
#pragma unroll
                for (uint32_t j = 0; j < kAsmOutWords; ++j) {
                    if (j >= ow) continue;  // (uniform)
                    uint64_t acc = accs[j];
                    if ((spill_mask >> j) & 1u) {  // (uniform) the lists' tails, from the plan in memory
                        const uint64_t bin = (t0 + wq_in + j) * 64u + lane;
                        uint64_t o0 = 0;
                        uint32_t n = 0;
                        if (wq_in + j < tw && bin < a.n_out_bins) {
                            o0 = a.offsets[bin];
                            n = (uint32_t)(a.offsets[bin + 1] - o0);
                        }
                        for (uint32_t i = kAsmHeld; __ballot(i < n) != 0ULL; ++i) {
                            if (i < n) {
                                const uint2 rf = a.refs[o0 + i];
                                acc |= blk[s_base[rf.x] + (rf.y >> 6) - s_lo[rf.x]] >> (rf.y & 63u);
                            }
                        }
                    }
                    const uint64_t word = __ballot((acc & 1ULL) != 0ULL);
                    if (lane == k * ow + j) keep = word;
                }
            }
            const uint32_t bsub = first + lane_k;
            if (lane_k < kb && bsub < nbe && wq_in + lane_j < tw)
                store_word<NT>(a.out + (b0 + bsub) * a.out_stride + t0 + wq_in + lane_j, keep);
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// launchers
// Run-time geometry -> compile-time constants, once for every kernel family: fn(int_c<LG>, int_c<WPL>) over the blocks of 2^LG lanes with
// one word per lane and the whole-wave block with two ...
template <int V>
using int_c = std::integral_constant<int, V>;
template <typename F>
static hipError_t dispatch_lg_wpl(int lg, int wpl, F &&fn)
{
    if (wpl == 2) return fn(int_c<6>{}, int_c<2>{});
    switch (lg) {
    case 0: return fn(int_c<0>{}, int_c<1>{});
    case 1: return fn(int_c<1>{}, int_c<1>{});
    case 2: return fn(int_c<2>{}, int_c<1>{});
    case 3: return fn(int_c<3>{}, int_c<1>{});
    case 4: return fn(int_c<4>{}, int_c<1>{});
    case 5: return fn(int_c<5>{}, int_c<1>{});
    default: return fn(int_c<6>{}, int_c<1>{});
    }
}
// ... and on top of it the counter planes and hash count of the plain-form kernels (count, locate, hits): fn(LG, WPL, int_c<NP>, int_c<H>),
// ten planes only with the compile-time three hash functions; H = 0 is the run-time hash count
template <typename F>
static hipError_t dispatch_planes_hash(uint32_t n_hash, int planes, int lg, int wpl, F &&fn)
{
    auto with = [&](auto np, auto h) { return dispatch_lg_wpl(lg, wpl, [&](auto LG, auto WPL) { return fn(LG, WPL, np, h); }); };
    int np = 0, h = 0;
    plain_planes_hash(n_hash, planes, &np, &h);
    if (h == 3) return np == 10 ? with(int_c<10>{}, int_c<3>{}) : with(int_c<16>{}, int_c<3>{});
    return with(int_c<16>{}, int_c<0>{});
}

// The filters of a launch as the count kernels take them: the fused ones, or the launch's own as a set of one; for the latency form
// (split) with each filter's geometry code, parts and shares.
static FilterSet make_filter_set(const CountLaunch &a, bool split)
{
    FilterSet set;
    set.n = a.n_fused > 0 ? (uint32_t)a.n_fused : 1u;
    if (a.n_fused > 0) {
        for (uint32_t i = 0; i < set.n; ++i) {
            set.f[i] = a.fused_f[i];
            set.col_begin[i] = a.fused_col_begin[i];
            set.col_end[i] = a.fused_col_end[i];
            set.out_offset[i] = a.fused_out_offset[i];
            if (!split) continue;
            set.geom[i] = a.fused_geom[i];
            set.parts[i] = a.fused_parts[i];
            set.sub[i] = a.fused_sub[i];
        }
    } else {
        set.f[0] = a.f;
        set.col_begin[0] = a.col_begin;
        set.col_end[0] = a.col_end;
        set.out_offset[0] = 0;
        if (split) {
            set.geom[0] = geom_code(a.lg, a.wpl, a.nt);
            set.parts[0] = (uint32_t)(a.split_parts > 1 ? a.split_parts : 1);
            set.sub[0] = (uint32_t)(a.split_sub > 1 ? a.split_sub : 1);
        }
    }
    return set;
}

template <int LG, int WPL, int NP, int H, bool NT>
static hipError_t launch_count_nt(const CountLaunch &a, hipStream_t st)
{
    const FilterSet set = make_filter_set(a, false);
    const uint64_t items = (uint64_t)a.n_reads * a.n_slices;
    dim3 grid((uint32_t)((items + kWavesPerBlock - 1) / kWavesPerBlock), set.n);
    EarlyCfg early{};
    PruneCfg prune{};
    prune.flags = a.bound_prune ? (kPruneBound | ((uint32_t)a.prune_parts << 1)) : 0u;
    prune.trace = a.n_fused == 0 ? a.prune_trace : nullptr;
    prune.cert_d = a.cert_d;
    prune.cert_c = a.cert_c;
    prune.flags |= (a.lead_min < 255u ? a.lead_min : 255u) << kPruneLeadMinShift;
    if (a.n_fused > 0) prune.flags &= ~(kPruneCert | kPruneLeadLine);  // (the allowance is one filter's)
    if constexpr (H == 3 && NP == 10) {  // (the early-decision builds exist for three hash functions and ten counter planes: what config 3 / 4 take)
        if (a.early_thr && a.n_fused == 0) {
            early.thr = a.early_thr;
            early.thr_len = a.early_thr_len;
            early.nf = a.early_nf;
            early.fi[0] = a.early_fi;
            hipLaunchKernelGGL((ibf_count_max_kernel<LG, WPL, NP, H, NT, true>), grid, dim3(64 * kWavesPerBlock), 0, st, set, a.src,
                               a.n_reads, a.n_slices, a.out, a.out_read_stride, a.out_slice_stride, early, prune);
            return hipGetLastError();
        }
    }
    hipLaunchKernelGGL((ibf_count_max_kernel<LG, WPL, NP, H, NT>), grid, dim3(64 * kWavesPerBlock), 0, st, set, a.src,
                       a.n_reads, a.n_slices, a.out, a.out_read_stride, a.out_slice_stride, early, prune);
    return hipGetLastError();
}

// latency form.  Dynamic LDS = plane exchange + maxima + per-wave staging; the opt-in for > 64 KiB of it is per function
// AND per device, remembered per device id.
template <typename K>
static hipError_t launch_split_kernel(K kern, std::atomic<uint64_t> &done, const FilterSet &set, const CountLaunch &a, int max_wpl,
                                      int np, uint32_t grid_parts, hipStream_t st)
{
    const int nw = a.split_waves;
    const size_t lds = (size_t)nw * max_wpl * np * 64 * 8 + 16 + (size_t)nw * kStageBytes;
    int dev = 0;
    (void)hipGetDevice(&dev);
    const uint64_t bit = (dev >= 0 && dev < 64) ? (1ULL << dev) : 0;
    if (!bit || !(done.load(std::memory_order_acquire) & bit)) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                                           160 * 1024);
        if (e != hipSuccess) return e;
        done.fetch_or(bit, std::memory_order_release);
    }
    dim3 grid(a.n_reads * a.n_slices * grid_parts, set.n);
    FoldJob job{};
    if (a.fold) {
        if (a.n_slices != 1 || set.n != 1 || !a.fold->maxcount || !a.fold->lens) return hipErrorInvalidValue;
        job = *a.fold;
    }
    hipLaunchKernelGGL(kern, grid, dim3(64 * nw), lds, st, set, a.src, a.n_reads, a.n_slices, a.out, a.out_read_stride,
                       a.out_slice_stride, grid_parts, a.split_ws, a.split_tickets, job);
    return hipGetLastError();
}

template <int LG, int WPL, int NP, bool NT>
static hipError_t launch_split_one(const FilterSet &set, const CountLaunch &a, uint32_t grid_parts, hipStream_t st)
{
    static std::atomic<uint64_t> done{0};
    return launch_split_kernel(ibf_count_max_split_kernel<LG, WPL, NP, 3, NT>, done, set, a, WPL, NP, grid_parts, st);
}

template <int NP>
static hipError_t launch_split(const CountLaunch &a, hipStream_t st)
{
    const FilterSet set = make_filter_set(a, true);
    const uint32_t grid_parts = a.grid_parts > 1 ? (uint32_t)a.grid_parts : 1u;
    bool same = true, wide = false;
    for (uint32_t i = 0; i < set.n; ++i) {
        if (set.parts[i] < 1 || set.parts[i] > grid_parts || set.sub[i] < 1) return hipErrorInvalidValue;
        same &= set.geom[i] == set.geom[0];
        wide |= (set.geom[i] & 8) != 0;
    }
    if (grid_parts > 1 && (!a.split_ws || !a.split_tickets)) return hipErrorInvalidValue;
    const int nw = a.split_waves;
    const int lg = (int)(set.geom[0] & 7), wpl = (set.geom[0] & 8) ? 2 : 1;
    const int cap = same ? split_waves_cap(wpl, NP, lg) : kSplitAnyWaves;
    if (nw < 2 || (nw & 1) || nw > cap) return hipErrorInvalidValue;
    if (same)
        return dispatch_lg_wpl(lg, wpl, [&](auto LG, auto WPL) {
            constexpr int L = decltype(LG)::value, W = decltype(WPL)::value;
            return (set.geom[0] & 16) ? launch_split_one<L, W, NP, true>(set, a, grid_parts, st) : launch_split_one<L, W, NP, false>(set, a, grid_parts, st);
        });
    static std::atomic<uint64_t> done[2];
    if (wide) return launch_split_kernel(ibf_count_max_split_any_kernel<NP, true>, done[1], set, a, 2, NP, grid_parts, st);
    return launch_split_kernel(ibf_count_max_split_any_kernel<NP, false>, done[0], set, a, 1, NP, grid_parts, st);
}

template <int LG, int WPL, int NP, int H>
static hipError_t launch_count(const CountLaunch &a, hipStream_t st)
{
    return a.nt ? launch_count_nt<LG, WPL, NP, H, true>(a, st) : launch_count_nt<LG, WPL, NP, H, false>(a, st);
}

// most waves a workgroup of the one-geometry latency kernel may have: the 16-byte-lane instantiations are built for
// 768 (10 planes) / 512 (16 planes) threads, the one-lane-per-block ones for 512 (eight tiles of block numbers in
// registers: at 1024 threads they spilled 36-49 registers; a 512-k-mer macro tile needs two waves anyway), the others
// for 1024, and the plane exchange of every wave has to fit the 160 KiB of LDS.  The mixed-geometry kernel takes
// kSplitAnyWaves.
int split_waves_cap(int wpl, int planes, int lg)
{
    const int np = planes <= 10 ? 10 : 16;
    const size_t per_wave = (size_t)wpl * np * 64 * 8 + kStageBytes;
    int cap = (int)((160 * 1024 - 16) / per_wave);
    const int by_bounds = wpl == 2 ? (np > 10 ? 8 : 12) : (lg == 0 ? 8 : 16);
    if (cap > by_bounds) cap = by_bounds;
    return cap & ~1;
}

// number of waves the latency form wants per read for this geometry (0 = latency form not applicable)
int split_waves_limit(int wpl, int planes, uint32_t max_kmers, int lg)
{
    int items = 64 * (lg >= 3 ? 1 : (8 >> lg));
    int tiles = (int)((max_kmers + items - 1) / items);
    int nw = 2 * (tiles < 1 ? 1 : tiles);
    const int cap = split_waves_cap(wpl, planes, lg);
    if (nw > cap) nw = cap;
    nw &= ~1;
    return nw >= 2 ? nw : 0;  // two waves = one per strand (reads that fit one macro tile, e.g. one-word filters)
}

// Several workgroups per read for the latency form (see ibf_count_max_split_kernel): worth it when a wave would
// otherwise walk many eight-step blocks in sequence, i.e. for blocks of 32+ lanes (filters of 17+ word columns).
// Returns parts (1 = keep the one-workgroup form and *nw untouched); with parts > 1 sets the waves per workgroup and
// the shares per macro tile.  parts * (*nw / 2) is a multiple of *sub, and *sub divides the blocks per macro tile.
int split_parts_plan(int wpl, int planes, uint32_t max_kmers, int lg, uint32_t n_items, uint32_t max_parts, uint32_t max_sub,
                     int *nw, int *sub)
{
    *sub = 1;
    if (max_parts <= 1 || lg < 5 || *nw < 2) return 1;
    const int bpt = lg == 6 ? 8 : 4;           // TileShape<LG>::STEPS / 8
    const uint32_t tiles = (max_kmers + 63) / 64;  // J == 1 for these shapes
    if (tiles == 0) return 1;
    const int wps = kSplitAnyWaves / 2;        // waves per strand and workgroup: fits every kernel of the latency form
    uint32_t cap = max_parts;
    // measured on the 8 GiB filter: beyond ~200 workgroups per launch the extra parts only queue behind each other
    // (64 reads: 3 parts 66 us, 4 parts 72 us, 6 parts 87 us, 1 part 82 us; 256 reads: 1 part is best)
    const uint32_t by_grid = n_items ? 200u / n_items : 1u;
    if (cap > by_grid) cap = by_grid;
    if (cap <= 1) return 1;
    int s0 = 1;
    while (s0 * 2 <= bpt && (uint32_t)(s0 * 2) <= max_sub) s0 *= 2;
    for (int s = s0; s >= 1; s >>= 1) {
        uint32_t p = (tiles * (uint32_t)s + (uint32_t)wps - 1) / (uint32_t)wps;
        if (p > cap) p = cap;
        const uint32_t m = s > wps ? (uint32_t)(s / wps) : 1u;
        p = p / m * m;
        if (p >= 2) {
            *nw = 2 * wps;
            *sub = s;
            return (int)p;
        }
    }
    return 1;
}

template <int LG, int NP>
static hipError_t launch_phased(const CountLaunch &a, hipStream_t st)
{
    dim3 grid((a.n_reads + kWavesPerBlock - 1) / kWavesPerBlock);
    // two-word blocks, reads of up to 256 / 384 k-mers, tables whose block numbers fit 21 bits: offsets in LDS, one or two reads per wave
    if constexpr (LG == 1 && NP == 10) {
        if (a.multi_reads && a.multi_tiles && a.col_begin == 0 && a.col_end == 2 && a.f.stride == 2) {
            if (a.f.n_blocks > kPackMaxBlocks) return hipErrorInvalidValue;
            const uint32_t R = a.multi_tiles == 6 ? 1u : (uint32_t)a.multi_reads;  // (six tiles: one read per wave)
            dim3 g2((a.n_reads + R - 1) / R);
#define RB_LAUNCH_MULTI(RR, INV, TT)                                                                                                    \
    hipLaunchKernelGGL((ibf_count_max_phased_multi_kernel<RR, INV, TT, 2>), g2, dim3(64), 0, st, a.f, a.src, a.n_reads, a.phase, a.out, \
                       a.out_read_stride, a.narrow)
            if (a.multi_tiles == 6 && a.multi_inv) RB_LAUNCH_MULTI(1, true, 6);
            else if (a.multi_tiles == 6) RB_LAUNCH_MULTI(1, false, 6);
            else if (R == 1 && a.multi_inv) RB_LAUNCH_MULTI(1, true, 4);
            else if (R == 1) RB_LAUNCH_MULTI(1, false, 4);
            else if (R == 2 && a.multi_inv) RB_LAUNCH_MULTI(2, true, 4);
            else if (R == 2) RB_LAUNCH_MULTI(2, false, 4);
            else return hipErrorInvalidValue;
#undef RB_LAUNCH_MULTI
            return hipGetLastError();
        }
    }
    // one-word blocks the same way (a filter of up to 64 bins on its own: the AND form)
    if constexpr (LG == 0 && NP == 10) {
        if (a.multi_reads && a.multi_tiles && a.col_begin == 0 && a.col_end == 1 && a.f.stride == 1) {
            if (a.f.n_blocks > kPackMaxBlocks1) return hipErrorInvalidValue;
            dim3 g1(a.n_reads);
            if (a.multi_tiles == 6)
                hipLaunchKernelGGL((ibf_count_max_phased_multi_kernel<1, false, 6, 1>), g1, dim3(64), 0, st, a.f, a.src, a.n_reads, a.phase, a.out, a.out_read_stride, a.narrow);
            else
                hipLaunchKernelGGL((ibf_count_max_phased_multi_kernel<1, false, 4, 1>), g1, dim3(64), 0, st, a.f, a.src, a.n_reads, a.phase, a.out, a.out_read_stride, a.narrow);
            return hipGetLastError();
        }
    }
    // both-strands-only build when every read of the batch fits it (LG 0/1, whole blocks owned by this rank)
    if constexpr (LG <= 1 && NP == 10) {
        if (a.short_only == 1 && (LG == 0 || (a.col_begin == 0 && a.col_end == 2 && a.f.stride == 2))) {
            hipLaunchKernelGGL((ibf_count_max_phased_kernel<LG, NP, 1>), grid, dim3(64 * kWavesPerBlock), 0, st, a.f, a.col_begin,
                               a.col_end, a.src, a.n_reads, a.phase, a.out, a.out_read_stride, a.narrow);
            return hipGetLastError();
        }
    }
    if constexpr (LG <= 1 && NP == 10) {
        if (a.short_only == 2 && (LG == 0 || (a.col_begin == 0 && a.col_end == 2 && a.f.stride == 2))) {
            hipLaunchKernelGGL((ibf_count_max_phased_kernel<LG, NP, 2>), grid, dim3(64 * kWavesPerBlock), 0, st, a.f, a.col_begin,
                               a.col_end, a.src, a.n_reads, a.phase, a.out, a.out_read_stride, a.narrow);
            return hipGetLastError();
        }
    }
    if constexpr (LG <= 1 && NP == 10) {
        if (a.short_only == 3 && (LG == 0 || (a.col_begin == 0 && a.col_end == 2 && a.f.stride == 2))) {
            hipLaunchKernelGGL((ibf_count_max_phased_kernel<LG, NP, 3>), grid, dim3(64 * kWavesPerBlock), 0, st, a.f, a.col_begin,
                               a.col_end, a.src, a.n_reads, a.phase, a.out, a.out_read_stride, a.narrow);
            return hipGetLastError();
        }
    }
    hipLaunchKernelGGL((ibf_count_max_phased_kernel<LG, NP, 0>), grid, dim3(64 * kWavesPerBlock), 0, st, a.f, a.col_begin,
                       a.col_end, a.src, a.n_reads, a.phase, a.out, a.out_read_stride, a.narrow);
    return hipGetLastError();
}

template <int NP>
static hipError_t dispatch_phased(const CountLaunch &a, hipStream_t st)
{
    // blocks of one and two words; three- and four-word blocks (stride 4) only in the both-strands build for reads of up to
    // 512 k-mers (short_only 4); wider blocks gain nothing from phases (rb_engine.hip, phase_slice_log2)
    if (a.lg == 2) {
        if constexpr (NP == 10) {
            // blocks of three and four words (stride 4), reads of up to 256 / 384 k-mers, block numbers of 21 bits: the builds with the offsets in LDS
            if (a.multi_reads && a.multi_tiles && a.col_begin == 0 && (a.col_end == 3 || a.col_end == 4) && a.f.stride == 4) {
                if (a.f.n_blocks > kPackMaxBlocks) return hipErrorInvalidValue;
                dim3 g1(a.n_reads);
#define RB_LAUNCH_MULTI4(INV, TT)                                                                                                       \
    hipLaunchKernelGGL((ibf_count_max_phased_multi_kernel<1, INV, TT, 4>), g1, dim3(64), 0, st, a.f, a.src, a.n_reads, a.phase, a.out, \
                       a.out_read_stride, a.narrow)
                if (a.multi_tiles == 6 && a.multi_inv) RB_LAUNCH_MULTI4(true, 6);
                else if (a.multi_tiles == 6) RB_LAUNCH_MULTI4(false, 6);
                else if (a.multi_inv) RB_LAUNCH_MULTI4(true, 4);
                else RB_LAUNCH_MULTI4(false, 4);
#undef RB_LAUNCH_MULTI4
                return hipGetLastError();
            }
            if ((a.short_only == 4 || a.short_only == 5) && a.col_begin == 0 && (a.col_end == 3 || a.col_end == 4) && a.f.stride == 4) {
                dim3 grid((a.n_reads + kWavesPerBlock - 1) / kWavesPerBlock);
                // short_only 5: every read of the batch has at most 256 k-mers: one round of four tiles per strand; three-word blocks
                // have a build without the fourth column (one 8-byte gather instead of the second 16-byte one, 16 registers less)
                if (a.short_only == 5 && a.col_end == 4)
                    hipLaunchKernelGGL((ibf_count_max_phased_kernel<2, 10, 1, 4>), grid, dim3(64 * kWavesPerBlock), 0, st, a.f, a.col_begin,
                                       a.col_end, a.src, a.n_reads, a.phase, a.out, a.out_read_stride, a.narrow);
                else if (a.short_only == 5)
                    hipLaunchKernelGGL((ibf_count_max_phased_kernel<2, 10, 1, 3>), grid, dim3(64 * kWavesPerBlock), 0, st, a.f, a.col_begin,
                                       a.col_end, a.src, a.n_reads, a.phase, a.out, a.out_read_stride, a.narrow);
#if RB_WIDE3_ROUNDS
                else if (a.col_end == 3)
                    hipLaunchKernelGGL((ibf_count_max_phased_kernel<2, 10, 2, 3>), grid, dim3(64 * kWavesPerBlock), 0, st, a.f, a.col_begin,
                                       a.col_end, a.src, a.n_reads, a.phase, a.out, a.out_read_stride, a.narrow);
#endif
                else  // (four-word blocks; at four waves per SIMD a three-word build had measured 7 % slower, at five it wins)
                    hipLaunchKernelGGL((ibf_count_max_phased_kernel<2, 10, 2, 4>), grid, dim3(64 * kWavesPerBlock), 0, st, a.f, a.col_begin,
                                       a.col_end, a.src, a.n_reads, a.phase, a.out, a.out_read_stride, a.narrow);
                return hipGetLastError();
            }
        }
        return hipErrorInvalidValue;
    }
    return a.lg == 0 ? launch_phased<0, NP>(a, st) : launch_phased<1, NP>(a, st);
}

hipError_t launch_ibf_count_max(const CountLaunch &a, hipStream_t st)
{
    if (a.n_reads == 0) return hipSuccess;
    if (a.phase.n_slices && a.split_waves < 2) {  // planned by the engine for: 3 hash functions, one slice, lg <= 1, wpl 1, n_fused 0
        if (a.f.n_hash != 3 || a.wpl != 1 || a.lg > 2 || a.n_slices != 1 || a.n_fused > 0 || a.phase.n_slices > 32) return hipErrorInvalidValue;
        // slice of a lookup = byte offset >> (shift + 3 + log2 stride): more than one slice needs a power-of-two block stride
        if (a.phase.n_slices > 1 && (a.f.stride & (a.f.stride - 1)) != 0) return hipErrorInvalidValue;
        return a.planes <= 10 ? dispatch_phased<10>(a, st) : dispatch_phased<16>(a, st);
    }
    if (a.split_waves >= 2) {  // latency form (three hash functions only; the engine plans it for those)
        if (a.f.n_hash != 3) return hipErrorInvalidValue;
        return a.planes <= 10 ? launch_split<10>(a, st) : launch_split<16>(a, st);
    }
    return dispatch_planes_hash(a.f.n_hash, a.planes, a.lg, a.wpl, [&](auto LG, auto WPL, auto NP, auto H) {
        return launch_count<decltype(LG)::value, decltype(WPL)::value, decltype(NP)::value, decltype(H)::value>(a, st);
    });
}

// the row form (ibf_count_rows_kernel): the engine plans it for the plain whole-wave builds with three compile-time hash functions only
template <int WPL, int NP, bool NT>
static hipError_t launch_rows_nt(const CountLaunch &a, hipStream_t st, bool twin_only = false)
{
    const uint64_t items = (uint64_t)a.n_reads * a.n_slices;
    dim3 grid((uint32_t)((items + kWavesPerBlock - 1) / kWavesPerBlock));
    PruneCfg prune{};
    prune.flags = a.bound_prune ? (kPruneBound | (((uint32_t)a.prune_parts & 3u) << 1)) : 0u;  // (no certificate, no lead line: nothing to certify)
    prune.trace = a.prune_trace;
    // the N-free reads from the row table, then the others from the filter's own: every item is one build's (twin_only: the list form's
    // kernel has written the N-free reads)
    if (!twin_only) {
        hipLaunchKernelGGL((ibf_count_rows_kernel<WPL, NP, NT, true>), grid, dim3(64 * kWavesPerBlock), 0, st, a.f, a.row_table, a.col_begin, a.col_end,
                           a.src, a.n_reads, a.n_slices, a.out, a.out_read_stride, a.out_slice_stride, prune);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL((ibf_count_rows_kernel<WPL, NP, NT, false>), grid, dim3(64 * kWavesPerBlock), 0, st, a.f, a.row_table, a.col_begin, a.col_end,
                       a.src, a.n_reads, a.n_slices, a.out, a.out_read_stride, a.out_slice_stride, prune);
    return hipGetLastError();
}

bool row_form_serves(const CountLaunch &a)
{
    int np = 0, h = 0;
    plain_planes_hash(a.f.n_hash, a.planes, &np, &h);
    return a.lg == 6 && h == 3 && a.split_waves < 2 && a.phase.n_slices == 0 && a.n_fused == 0 && !a.early_thr && a.f.k <= kRowTableMaxK;
}

static hipError_t launch_rows_builds(const CountLaunch &a, hipStream_t st, bool twin_only)
{
    const bool p10 = a.planes <= 10, nt = a.nt != 0;
    if (a.wpl == 2) {
        if (p10) return nt ? launch_rows_nt<2, 10, true>(a, st, twin_only) : launch_rows_nt<2, 10, false>(a, st, twin_only);
        return nt ? launch_rows_nt<2, 16, true>(a, st, twin_only) : launch_rows_nt<2, 16, false>(a, st, twin_only);
    }
    if (p10) return nt ? launch_rows_nt<1, 10, true>(a, st, twin_only) : launch_rows_nt<1, 10, false>(a, st, twin_only);
    return nt ? launch_rows_nt<1, 16, true>(a, st, twin_only) : launch_rows_nt<1, 16, false>(a, st, twin_only);
}

hipError_t launch_ibf_count_rows(const CountLaunch &a, hipStream_t st)
{
    if (a.n_reads == 0) return hipSuccess;
    if (!a.row_table || !row_form_serves(a)) return hipErrorInvalidValue;
    return launch_rows_builds(a, st, false);
}

hipError_t launch_ibf_count_rows_twin(const CountLaunch &a, hipStream_t st)
{
    if (a.n_reads == 0) return hipSuccess;
    if (!row_form_serves(a)) return hipErrorInvalidValue;
    return launch_rows_builds(a, st, true);
}

hipError_t launch_row_table(const IbfDev &f, uint64_t *rows, uint64_t n_rows, hipStream_t st)
{
    if (n_rows == 0 || n_rows > (1ull << (2 * kRowTableMaxK)) || f.k == 0 || f.k > kRowTableMaxK) return hipErrorInvalidValue;
    const uint64_t blocks = std::min<uint64_t>((n_rows + 3) / 4, 1ull << 20);  // four waves each; beyond 2^22 waves they stride
    hipLaunchKernelGGL(ibf_row_table_kernel, dim3((uint32_t)blocks), dim3(256), 0, st, f, rows, n_rows);
    return hipGetLastError();
}

template <int LG, int NP>
static hipError_t launch_merged_nt(const CountLaunch &a, const MergeMap &map, hipStream_t st)
{
    dim3 grid((a.n_reads + kWavesPerBlock - 1) / kWavesPerBlock);
    if (a.nt)
        hipLaunchKernelGGL((ibf_count_max_merged_kernel<LG, NP, true>), grid, dim3(64 * kWavesPerBlock), 0, st, a.f, map, a.src, a.n_reads,
                           a.out, a.out_read_stride);
    else
        hipLaunchKernelGGL((ibf_count_max_merged_kernel<LG, NP, false>), grid, dim3(64 * kWavesPerBlock), 0, st, a.f, map, a.src, a.n_reads,
                           a.out, a.out_read_stride);
    return hipGetLastError();
}

template <int NP>
static hipError_t launch_merged_lg(const CountLaunch &a, const MergeMap &map, hipStream_t st)
{
    switch (a.lg) {
    case 1: return launch_merged_nt<1, NP>(a, map, st);
    case 2: return launch_merged_nt<2, NP>(a, map, st);
    case 3: return launch_merged_nt<3, NP>(a, map, st);
    case 4: return launch_merged_nt<4, NP>(a, map, st);
    default: return hipErrorInvalidValue;
    }
}

hipError_t launch_ibf_count_max_merged(const CountLaunch &a, const MergeMap &map, hipStream_t st)
{
    if (a.n_reads == 0) return hipSuccess;
    if (a.f.n_hash != 3 || a.wpl != 1 || map.n == 0 || map.n > kMaxMerged || map.width == 0 || map.width > (1u << a.lg)) return hipErrorInvalidValue;
    return a.planes <= 10 ? launch_merged_lg<10>(a, map, st) : launch_merged_lg<16>(a, map, st);
}

hipError_t launch_merge_bits(const uint64_t *src, uint32_t s_src, uint32_t width, uint32_t n_bins, uint64_t *dst, uint32_t s_dst, uint32_t dst_bit,
                             uint64_t n_blocks, hipStream_t st)
{
    if (n_blocks == 0 || width == 0) return hipSuccess;
    uint64_t blocks = (n_blocks * width + 255) / 256;
    if (blocks > 256 * 32) blocks = 256 * 32;
    hipLaunchKernelGGL(merge_bits_kernel, dim3((uint32_t)blocks), dim3(256), 0, st, src, s_src, width, n_bins, dst, s_dst, dst_bit, n_blocks);
    return hipGetLastError();
}

hipError_t launch_invert_words(const uint64_t *src, uint64_t *dst, uint64_t n_words, hipStream_t st)
{
    if (n_words == 0) return hipSuccess;
    uint64_t blocks = (n_words + 255) / 256;
    if (blocks > 256 * 32) blocks = 256 * 32;
    hipLaunchKernelGGL(invert_words_kernel, dim3((uint32_t)blocks), dim3(256), 0, st, src, dst, n_words);
    return hipGetLastError();
}

// locate, hits and prefixes: one launch of a plain query pass.  A wave per (item, slice), the build picked as the count kernel's is; non-temporal
// builds for blocks of a whole wave only (the tables beyond the Infinity Cache are the wide ones; a narrow table of that size keeps the
// default cache policy, which costs speed, not results).  Pass::kernel<LG, WPL, NP, H, NT>() names the pass's kernel, `more` are its own
// arguments behind the shared ones.
struct LocatePass {
    template <int LG, int WPL, int NP, int H, bool NT>
    static constexpr auto kernel() { return &ibf_locate_kernel<LG, WPL, NP, H, NT>; }
};
struct HitsPass {
    template <int LG, int WPL, int NP, int H, bool NT>
    static constexpr auto kernel() { return &ibf_hits_kernel<LG, WPL, NP, H, NT>; }
};
template <typename Pass, typename... More>
static hipError_t launch_plain_pass(const PlainPassLaunch &a, hipStream_t st, More... more)
{
    if (!a.thr || a.thr_len == 0 || a.n_slices == 0 || (a.wpl != 1 && a.wpl != 2) || a.lg < 0 || a.lg > 6) return hipErrorInvalidValue;
    // every column the grid reaches lies inside the filter, every slice has its record / its segments
    if (a.col_end > a.f.bin_width || a.col_begin > a.col_end ||
        (uint64_t)a.n_slices * (uint64_t)((1u << a.lg) * (uint32_t)a.wpl) < (uint64_t)(a.col_end - a.col_begin))
        return hipErrorInvalidValue;
    const uint64_t items = (uint64_t)a.n_items * a.n_slices;
    const dim3 grid((uint32_t)((items + kWavesPerBlock - 1) / kWavesPerBlock));
    return dispatch_planes_hash(a.f.n_hash, a.planes, a.lg, a.wpl, [&](auto LG, auto WPL, auto NP, auto H) {
        constexpr int L = decltype(LG)::value, W = decltype(WPL)::value, P = decltype(NP)::value, HH = decltype(H)::value;
        auto kern = Pass::template kernel<L, W, P, HH, false>();
        if constexpr (L == 6) {
            if (plain_pass_nt(L, a.nt)) kern = Pass::template kernel<L, W, P, HH, true>();
        }
        hipLaunchKernelGGL(kern, grid, dim3(64 * kWavesPerBlock), 0, st, a.f, a.col_begin, a.col_end, a.src, a.n_items, a.n_slices, a.thr,
                           a.thr_len, a.nf, a.fi, more...);
        return hipGetLastError();
    });
}

hipError_t launch_ibf_locate(const LocateLaunch &a, hipStream_t st)
{
    if (a.n_items == 0) return hipSuccess;
    if (!a.part) return hipErrorInvalidValue;
    return launch_plain_pass<LocatePass>(a, st, a.part);
}

hipError_t launch_reduce_locate_slices(const LocatePart *part, uint32_t n_slices, uint32_t n_items, const uint32_t *lens,
                                       const uint8_t *pre_status, uint32_t max_len, uint32_t min_len, const LocateOut &out, uint32_t nf,
                                       uint32_t fidx, hipStream_t st)
{
    if (n_items == 0) return hipSuccess;
    hipLaunchKernelGGL(reduce_locate_slices_kernel, dim3((n_items + 255) / 256), dim3(256), 0, st, part, n_slices, n_items, lens, pre_status,
                       max_len, min_len, out, nf, fidx);
    return hipGetLastError();
}

struct PrefixPass {
    template <int LG, int WPL, int NP, int H, bool NT>
    static constexpr auto kernel() { return &ibf_prefix_kernel<LG, WPL, NP, H, NT>; }
};
hipError_t launch_ibf_prefix(const PrefixLaunch &a, hipStream_t st)
{
    if (a.n_items == 0) return hipSuccess;
    if (!a.part || a.cps.n == 0 || a.cps.n > kMaxPrefixes) return hipErrorInvalidValue;
    return launch_plain_pass<PrefixPass>(a, st, a.cps, a.part);
}

hipError_t launch_finish_prefix(const PrefixLaunch &a, const uint32_t *lens, const uint8_t *pre_status, uint16_t *max_count, uint32_t *prefix_len,
                                uint8_t *row_pre, hipStream_t st)
{
    const uint64_t rows = (uint64_t)a.n_items * a.cps.n;
    if (rows == 0) return hipSuccess;
    if (rows > 0x7FFFFFFFull || !max_count || !prefix_len || !row_pre) return hipErrorInvalidValue;
    hipLaunchKernelGGL(finish_prefix_kernel, dim3((uint32_t)((rows + 255) / 256)), dim3(256), 0, st, a.part, a.n_slices, a.n_items, a.cps, lens,
                       pre_status, max_count, prefix_len, row_pre, a.nf, a.fi);
    return hipGetLastError();
}

hipError_t launch_first_decided(const uint8_t *decision, const uint8_t *status, uint32_t n_items, uint32_t n_prefixes, uint32_t *first_decided,
                                hipStream_t st)
{
    if (n_items == 0) return hipSuccess;
    hipLaunchKernelGGL(first_decided_kernel, dim3((n_items + 255) / 256), dim3(256), 0, st, decision, status, n_items, n_prefixes, first_decided);
    return hipGetLastError();
}

// (sixteen planes whatever the launch says: the state holds no other kind, and no ten-plane build of this kernel exists)
struct ResumePass {
    template <int LG, int WPL, int NP, int H, bool NT>
    static constexpr auto kernel() { return &ibf_resume_kernel<LG, WPL, (int)kResumePlanes, H, NT>; }
};
hipError_t launch_ibf_resume(const ResumeLaunch &a, hipStream_t st)
{
    if (a.n_items == 0) return hipSuccess;
    if (!a.part || !a.slots.state || !a.slots.slot || !a.slots.ctl || a.planes != (int)kResumePlanes) return hipErrorInvalidValue;
    // every column a wave of the grid loads or stores lies inside the filter's share of a slot
    if ((uint64_t)a.n_slices * (uint64_t)((1u << a.lg) * (uint32_t)a.wpl) != (uint64_t)a.slots.pad_cols || a.col_begin != 0 ||
        a.slots.filter_off + 2ull * kResumePlanes * a.slots.pad_cols > a.slots.slot_words)
        return hipErrorInvalidValue;
    return launch_plain_pass<ResumePass>(a, st, a.slots, a.part);
}

hipError_t launch_resume_prep(const ResumePrep &a, hipStream_t st)
{
    if (a.n_items == 0) return hipSuccess;
    if (!a.slot || !a.meta || !a.stitched || !a.st_offsets || !a.st_lens || !a.total_lens || !a.pre_status || !a.ctl || a.k == 0 ||
        a.k > rbspec::kMaxKmer || (uint64_t)a.stitch_stride < (uint64_t)a.max_chunk_len + kResumeMaxTail)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(resume_prep_kernel, dim3((a.n_items + kWavesPerBlock - 1) / kWavesPerBlock), dim3(64 * kWavesPerBlock), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_resume_commit(ResumeMeta *meta, const uint32_t *slot, const uint8_t *ctl, const uint8_t *stitched, uint32_t stitch_stride,
                                const uint32_t *st_lens, const uint32_t *total_lens, uint32_t n_items, uint32_t k, hipStream_t st)
{
    if (n_items == 0) return hipSuccess;
    hipLaunchKernelGGL(resume_commit_kernel, dim3((n_items + 255) / 256), dim3(256), 0, st, meta, slot, ctl, stitched, stitch_stride, st_lens,
                       total_lens, n_items, k);
    return hipGetLastError();
}

hipError_t launch_resume_counts(const uint64_t *planes, uint32_t pad_cols, uint32_t n_bins, uint16_t *counts, hipStream_t st)
{
    if (n_bins == 0) return hipSuccess;
    if ((uint64_t)pad_cols * 64u < n_bins || n_bins >= (1u << 31)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(resume_counts_kernel, dim3((2u * n_bins + 255) / 256), dim3(256), 0, st, planes, pad_cols, n_bins, counts);
    return hipGetLastError();
}

hipError_t launch_ibf_hits(const HitsLaunch &a, hipStream_t st)
{
    if (a.n_items == 0) return hipSuccess;
    if (!a.seg_count || (a.max_hits && !a.seg)) return hipErrorInvalidValue;
    return launch_plain_pass<HitsPass>(a, st, a.min_count, a.max_hits, a.min_len, a.pre_status, (rb_u32x2 *)a.seg, a.seg_count,
                                       (unsigned long long *)a.bin_reads);
}

hipError_t launch_finish_hits(const HitsLaunch &a, const uint32_t *lens, const HitsOut &out, hipStream_t st)
{
    if (a.n_items == 0) return hipSuccess;
    hipLaunchKernelGGL(finish_hits_kernel, dim3((a.n_items + 255) / 256), dim3(256), 0, st, (const rb_u32x2 *)a.seg, a.seg_count, a.n_slices,
                       a.n_items, lens, a.pre_status, a.src.max_len, a.min_len, a.max_hits, out, a.nf, a.fi);
    return hipGetLastError();
}

// spans: the compile-time h = 3 build and the run-time-h build, each with its non-temporal twin
template <int H>
static hipError_t launch_spans_nt(const SpansLaunch &a, hipStream_t st)
{
    dim3 grid((a.n_queries + kWavesPerBlock - 1) / kWavesPerBlock);
    if (a.nt)
        hipLaunchKernelGGL((ibf_spans_kernel<H, true>), grid, dim3(64 * kWavesPerBlock), 0, st, a.f, a.src, a.n_items, a.queries, a.n_queries,
                           a.mask_words, a.pre_status, a.min_len, a.out);
    else
        hipLaunchKernelGGL((ibf_spans_kernel<H, false>), grid, dim3(64 * kWavesPerBlock), 0, st, a.f, a.src, a.n_items, a.queries, a.n_queries,
                           a.mask_words, a.pre_status, a.min_len, a.out);
    return hipGetLastError();
}

hipError_t launch_ibf_spans(const SpansLaunch &a, hipStream_t st)
{
    if (a.n_queries == 0) return hipSuccess;
    if (!a.queries || (!a.out.spans && !a.out.mask && !a.out.n_kmers && !a.out.status) || !a.f.words ||
        (a.n_items && (!a.src.lens || !a.src.offsets || !a.src.seqs)))
        return hipErrorInvalidValue;
    // what the kernel's addressing relies on: the bin's word column lies inside a block, a round's bases fit the staging area
    if (a.f.n_bins > (uint64_t)a.f.bin_width * 64u || a.f.bin_width > a.f.stride || a.f.k == 0 || a.f.k > rbspec::kMaxKmer || a.f.n_blocks == 0 ||
        a.f.n_hash == 0 || a.f.n_hash > rbspec::kMaxHash || a.min_len < a.f.k)
        return hipErrorInvalidValue;
    int np = 0, h = 0;  // (the hash form of the plain passes; spans has no counter planes)
    plain_planes_hash(a.f.n_hash, 16, &np, &h);
    return h == 3 ? launch_spans_nt<3>(a, st) : launch_spans_nt<0>(a, st);
}

hipError_t launch_reduce_slices(const uint16_t *part, uint32_t n_slices, uint32_t n_reads, uint16_t *maxcount,
                                uint32_t nf, uint32_t fidx, hipStream_t st)
{
    if (n_reads == 0) return hipSuccess;
    hipLaunchKernelGGL(reduce_slices_kernel, dim3((n_reads + 255) / 256), dim3(256), 0, st, part, n_slices, n_reads,
                       maxcount, nf, fidx);
    return hipGetLastError();
}

hipError_t launch_decide(const DecideParams &P, const uint16_t *maxcount, const uint32_t *lens, const uint8_t *pre_status,
                         uint32_t n_reads, int mode, int32_t *best_target, uint8_t *decision, uint8_t *status,
                         hipStream_t st)
{
    if (n_reads == 0) return hipSuccess;
    if (P.done_flag && n_reads > 256 && !P.done_count) return hipErrorInvalidValue;
    hipLaunchKernelGGL(decide_kernel, dim3((n_reads + 255) / 256), dim3(256), 0, st, P, maxcount, lens, pre_status, n_reads,
                       mode, best_target, decision, status);
    return hipGetLastError();
}

// A micro-batch's way into HBM: the runtime's copy of a few KB is a blit kernel of its own that takes 11 us per call (the driver's
// command under rocprofv3, profiles/r05/default_kernel_stats.csv: __amd_rocclr_copyBuffer, 75 k calls) -- a quarter of a micro-batch's
// service time.  This one reads the pinned (coherent) host block with 16 bytes per lane -- a GPU read of host memory crosses PCIe one
// request per lane -- and is queued like any other kernel of the call.  `units` 16-byte units.
__global__ __launch_bounds__(256) void copy_from_host_kernel(const rb_u32x4 *__restrict__ src, rb_u32x4 *__restrict__ dst, uint32_t units)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < units) dst[i] = __builtin_nontemporal_load(src + i);
}

hipError_t launch_copy_from_host(const void *h_src, void *d_dst, size_t bytes, hipStream_t st)
{
    const uint32_t units = (uint32_t)((bytes + 15) >> 4);
    if (units == 0) return hipSuccess;
    hipLaunchKernelGGL(copy_from_host_kernel, dim3((units + 255) / 256), dim3(256), 0, st, (const rb_u32x4 *)h_src, (rb_u32x4 *)d_dst, units);
    return hipGetLastError();
}

hipError_t launch_chunk_prep(const uint32_t *lens, const uint32_t *ids, uint32_t n_items, uint32_t chunk_start,
                             uint32_t chunk_len, uint32_t *eff_lens, uint8_t *pre_status, hipStream_t st)
{
    if (n_items == 0) return hipSuccess;
    hipLaunchKernelGGL(chunk_prep_kernel, dim3((n_items + 255) / 256), dim3(256), 0, st, lens, ids, n_items, chunk_start,
                       chunk_len, eff_lens, pre_status);
    return hipGetLastError();
}

hipError_t launch_insert(const IbfDev &f, uint64_t *words, const uint8_t *seq, const uint64_t *starts,
                         const uint64_t *ends, const uint64_t *bins, const uint64_t *kmer_prefix,
                         uint32_t n_fragments, uint64_t total_kmers, hipStream_t st)
{
    if (total_kmers == 0) return hipSuccess;
    const uint64_t blocks = (total_kmers + 255) / 256;
    hipLaunchKernelGGL(ibf_insert_kernel, dim3((uint32_t)blocks), dim3(256), 0, st, f, words, seq, starts, ends, bins,
                       kmer_prefix, n_fragments, total_kmers);
    return hipGetLastError();
}

hipError_t launch_restride_blocks(const uint64_t *src, uint32_t s_src, uint64_t *dst, uint32_t s_dst, uint32_t w_copy,
                                  uint64_t n_blocks, hipStream_t st)
{
    if (n_blocks == 0) return hipSuccess;
    uint64_t blocks = (n_blocks * s_dst + 255) / 256;
    if (blocks > 256 * 32) blocks = 256 * 32;
    hipLaunchKernelGGL(restride_blocks_kernel, dim3((uint32_t)blocks), dim3(256), 0, st, src, s_src, dst, s_dst, w_copy,
                       n_blocks);
    return hipGetLastError();
}

hipError_t launch_compare_bits(const uint64_t *a, const uint64_t *b, uint64_t n_words, uint64_t *out3, hipStream_t st)
{
    if (n_words == 0) return hipSuccess;
    uint64_t blocks = (n_words + 255) / 256;
    if (blocks > 256 * 32) blocks = 256 * 32;
    hipLaunchKernelGGL(compare_bits_kernel, dim3((uint32_t)blocks), dim3(256), 0, st, a, b, n_words,
                       reinterpret_cast<unsigned long long *>(out3));
    return hipGetLastError();
}

hipError_t launch_fill_reads(uint8_t *seqs, uint64_t *offsets, uint32_t *lens, size_t n_reads, uint32_t read_len, uint64_t seed, hipStream_t st)
{
    if (n_reads == 0 || read_len == 0) return hipSuccess;
    uint64_t blocks = ((uint64_t)n_reads * read_len + 255) / 256;
    if (blocks > 256 * 32) blocks = 256 * 32;
    hipLaunchKernelGGL(fill_reads_kernel, dim3((uint32_t)blocks), dim3(256), 0, st, seqs, offsets, lens, (uint64_t)n_reads, read_len, seed);
    return hipGetLastError();
}

hipError_t launch_fill_synth(uint64_t *words, uint64_t used_words, uint32_t bin_width, uint32_t stride_words,
                             uint64_t last_mask, uint64_t seed, hipStream_t st)
{
    if (used_words == 0) return hipSuccess;
    uint64_t blocks = (used_words + 255) / 256;
    if (blocks > 256 * 32) blocks = 256 * 32;
    hipLaunchKernelGGL(fill_synth_kernel, dim3((uint32_t)blocks), dim3(256), 0, st, words, used_words, bin_width,
                       stride_words, last_mask, seed);
    return hipGetLastError();
}

// rb_set_bin_occupancy_grid: workgroups per column slice at most, and the fewest rows of a chunk, for every later pass of this process
// (0 = the rule below).  Counts never depend on it; a small table then walks chunks of the full length and several of them per wave.
static std::atomic<uint32_t> g_occ_max_wgs{0}, g_occ_min_chunk_rows{0};
void set_bin_occupancy_grid(uint32_t max_wgs_per_slice, uint32_t min_chunk_rows)
{
    g_occ_max_wgs.store(max_wgs_per_slice);
    g_occ_min_chunk_rows.store(min_chunk_rows);
}

// One workgroup of kOccWaves waves per CU, shared out over the column slices; every wave walks `iters` chunks of `chunk_rows`
// wave rows (a multiple of 16, at most kOccMaxChunkRows).  `out` (u64 [n_bins]) is zeroed on the stream first.
hipError_t launch_bin_occupancy(const uint64_t *words, uint64_t n_blocks, uint64_t stride, uint32_t bin_width, uint32_t n_bins, int nt,
                                uint64_t *out, hipStream_t st)
{
    if (n_bins == 0) return hipSuccess;
    hipError_t e = hipMemsetAsync(out, 0, (size_t)n_bins * 8, st);
    if (e != hipSuccess || n_blocks == 0) return e;
    if (stride < bin_width || (stride >= 16 && stride % 16 != 0) || (stride < 16 && (stride & (stride - 1)) != 0)) return hipErrorInvalidValue;
    const int wpl = stride >= 16 ? 2 : 1;
    const uint64_t rw = 64u * (uint64_t)wpl;
    const uint64_t n_slices = (stride + rw - 1) / rw;
    uint32_t lg = 0;
    while (((uint64_t)wpl << lg) < std::min<uint64_t>(rw, stride)) ++lg;
    const uint64_t ng = 64u >> lg;
    const uint64_t n_rows = (n_blocks + ng - 1) / ng;  // wave rows of a full slice (a narrower last slice has fewer)
    int dev = 0, cus = 0;
    if ((e = hipGetDevice(&dev)) != hipSuccess) return e;
    if ((e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev)) != hipSuccess) return e;
    uint64_t want = std::max<uint64_t>(1, ((uint64_t)std::max(cus, 1) + n_slices - 1) / n_slices);
    if (const uint32_t cap = g_occ_max_wgs.load()) want = std::min<uint64_t>(want, cap);
    const uint64_t min_rows = g_occ_min_chunk_rows.load() ? g_occ_min_chunk_rows.load() : kOccMinChunkRows;
    const uint64_t useful = (n_rows + min_rows * kOccWaves - 1) / (min_rows * kOccWaves);
    OccLaunch a;
    a.words = words;
    a.n_blocks = n_blocks;
    a.stride = stride;
    a.bin_width = bin_width;
    a.n_bins = n_bins;
    a.wgs_per_slice = (uint32_t)std::min(want, useful);
    const uint64_t slots = (uint64_t)a.wgs_per_slice * kOccWaves;
    const uint64_t per_slot = (n_rows + slots - 1) / slots;
    a.iters = (uint32_t)((per_slot + kOccMaxChunkRows - 1) / kOccMaxChunkRows);
    a.chunk_rows = (uint32_t)(((per_slot + a.iters - 1) / a.iters + 15) / 16 * 16);
    if (a.chunk_rows > kOccMaxChunkRows || n_slices * a.wgs_per_slice > 0x7FFFFFFFull) return hipErrorInvalidValue;
    const dim3 grid((uint32_t)(n_slices * a.wgs_per_slice)), block(64 * kOccWaves);
    unsigned long long *o = reinterpret_cast<unsigned long long *>(out);
    if (wpl == 2) {
        if (nt) hipLaunchKernelGGL((ibf_bin_occupancy_kernel<2, true>), grid, block, 0, st, a, o);
        else hipLaunchKernelGGL((ibf_bin_occupancy_kernel<2, false>), grid, block, 0, st, a, o);
    } else {
        if (nt) hipLaunchKernelGGL((ibf_bin_occupancy_kernel<1, true>), grid, block, 0, st, a, o);
        else hipLaunchKernelGGL((ibf_bin_occupancy_kernel<1, false>), grid, block, 0, st, a, o);
    }
    return hipGetLastError();
}

// rb_set_assemble_grid: workgroups per launch at most, and the blocks of a chunk, for every later assemble of this process (0 = the
// rule below).  The bits never depend on it; a small table then walks several chunks per workgroup, short last chunks included.
static std::atomic<uint32_t> g_asm_max_wgs{0}, g_asm_blocks_per_chunk{0};
void set_assemble_grid(uint32_t max_workgroups, uint32_t blocks_per_chunk)
{
    g_asm_max_wgs.store(max_workgroups);
    g_asm_blocks_per_chunk.store(blocks_per_chunk);
}

// Four workgroups of kAsmWaves waves per CU, shared out over the tiles (workgroup = tile + n_tiles * slot, so the tiles of one chunk
// are dispatched side by side and meet each other's source lines in cache); a slot walks `iters` chunks of `blocks_per_chunk` blocks.
hipError_t launch_assemble(AsmLaunch a, const AsmWindow *windows_host, int nt, hipStream_t st)
{
    if (a.n_blocks == 0 || a.out_stride == 0) return hipSuccess;
    if (a.n_srcs == 0 || a.n_srcs > kAsmMaxSources) return hipErrorInvalidValue;
    const uint64_t n_tiles = (a.out_stride + kAsmTileWords - 1) / kAsmTileWords;
    if (n_tiles > 0x00FFFFFFull) return hipErrorInvalidValue;
    a.n_tiles = (uint32_t)n_tiles;
    uint64_t lds_words = 0;
    for (uint64_t t = 0; t < n_tiles; ++t) {
        uint64_t sw = 1;
        for (uint32_t s = 0; s < a.n_srcs; ++s) sw += windows_host[t * kAsmMaxSources + s].n;
        if (sw > kAsmMaxLdsWords) return hipErrorInvalidValue;
        const uint32_t tw = (uint32_t)std::min<uint64_t>(kAsmTileWords, a.out_stride - t * kAsmTileWords);
        const AsmShape sh = asm_shape(tw, (uint32_t)sw);
        lds_words = std::max<uint64_t>(lds_words, (uint64_t)sh.gpw * sh.kb * sh.rounds * sw);
    }
    int dev = 0, cus = 0;
    hipError_t e;
    if ((e = hipGetDevice(&dev)) != hipSuccess) return e;
    if ((e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev)) != hipSuccess) return e;
    const uint32_t bpc = g_asm_blocks_per_chunk.load() ? g_asm_blocks_per_chunk.load() : 1024u;
    const uint64_t n_chunks = (a.n_blocks + bpc - 1) / bpc;
    uint64_t wgs = std::max<uint64_t>(1, 4ull * (uint64_t)std::max(cus, 1));
    if (const uint32_t cap = g_asm_max_wgs.load()) wgs = std::min<uint64_t>(wgs, cap);
    uint64_t per_tile = std::max<uint64_t>(1, wgs / n_tiles);
    per_tile = std::min(per_tile, n_chunks);
    if (per_tile * n_tiles > 0x7FFFFFFFull) return hipErrorInvalidValue;
    a.wgs_per_tile = (uint32_t)per_tile;
    a.blocks_per_chunk = bpc;
    const uint64_t iters = (n_chunks + per_tile - 1) / per_tile;
    if (iters > 0xFFFFFFFFull) return hipErrorInvalidValue;
    a.iters = (uint32_t)iters;
    const dim3 grid((uint32_t)(per_tile * n_tiles)), block(64 * kAsmWaves);
    const size_t lds_bytes = (size_t)lds_words * 8;
    if (nt) hipLaunchKernelGGL((ibf_assemble_kernel<true>), grid, block, lds_bytes, st, a);
    else hipLaunchKernelGGL((ibf_assemble_kernel<false>), grid, block, lds_bytes, st, a);
    return hipGetLastError();
}

}  // namespace rb

// row_list_probe.hip -- step 0 of the sparse bin lists: before any kernel work, what would a count kernel
// deliver that gathers one 256-byte LIST of bin numbers per k-mer (two 128-byte lines) instead of the 1 KiB bit row (eight), and
// counts each listed bin with one returning LDS add?  No hashing, no reads, no pruning: the gather and the adds alone.
//   table  : 4^13 = 2^26 rows of 256 bytes = 16 GiB.  A row is a sorted list of distinct bin numbers < 8192 as uint16_t, 72-91 of
//            its 128 entries used (mean 81.5 = 63.7 %, the d^3 = (55/256)^3 of config 3 at design load), the rest 0xFFFF
//   wave   : one wave per "read", one 64-thread workgroup each, 16 KiB of LDS (8192 uint16_t counters, two per dword): ten waves
//            per CU is what the LDS allows.  A read is 704 rows (config 3 has 696 k-mers on two strands); the counters are
//            cleared once per read
//   tile   : R rows in flight per wave (32 or 64; a row costs ONE VGPR: one dword per lane).  Lane u of the tile draws the row
//            number of row u, as a lane of the count kernel ranks its own k-mer; the numbers travel by v_readlane; the R gathers
//            are issued back to back (sched_barrier), non-temporal or temporal
//   count  : per row and lane two returning adds (ds_add_rtn_u32 of 1 << 16·(bin & 1) at dword bin >> 1) for the entries below
//            8192, and a running maximum of "old half + 1", as the kernel would keep it
//   nolds  : the same loop with the LDS part replaced by an XOR
//   scan   : the count code ibf_count_lists_kernel has since taken: two adds per row and lane that return nothing (an entry that is no
//            bin is clamped to the lane's own spare dword behind the counters), no running maximum, and per read one scan of the
//            counters (ds_read_b128, packed 16-bit maximum, one wave reduction) fused with the clear.  Nine waves per CU then
//   rolling: the scan mode with a rolling refill: when group g (eight rows) of tile t has been counted, the loads of group g of tile
//            t + 1 are issued into the same registers, so a wave always has R - 8 to R rows in flight, across tile and read edges
//   ready  : the scan mode over a table in the RESIDENT ("add-ready") form of rb_lists.h: each 16-bit half of a dword holds the LDS byte
//            offset of a counter dword (even bins in low halves, odd bins in high halves, a half that lists no bin names the lane's
//            own spare), so the count is `add 1 at v & 0xFFFF` and `add 0x10000 at v >> 16`: two vector instructions per dword around
//            the two adds.  Third argument `addready`: only `no lds`, then `scan` and `ready` in turn, three times each (two tables)
//   pair   : step 0 of the pair table: one slot of 384 bytes (three lines) per k-mer holds the lists of the k-mer AND of its reverse
//            complement, 2^26 slots = 24 GiB.  One counter dword per bin (low half forward strand, high half reverse strand: 32 KiB, four
//            workgroups per CU), a read is 352 k-mers.  Lines 0-1 are positional (dword l: A[l] in the low half, B[l] in the high half:
//            `ready`'s two instructions per dword), line 2 holds what is left of both lists, bit 0 of a half naming list B, and is loaded
//            for two slots per instruction (lanes 0-31 and 32-63).  One workgroup of NW waves per read on one counter array, tile t of
//            the read to wave t mod NW; NW = 1 with the next tile's gathers issued before the current tile's adds ("two-tile"), and 1, 2,
//            4 with one tile in flight.  Third argument `pair`: `ready` and the pair settings in turn, three rounds, and the gate: a
//            k-mer's slot in at most 0.90 of the time `ready` takes for its two rows, in every round (the lines predict 0.75)
// Prints rows/s and lines/s (2 per row) per setting, best of 3 runs after one warm-up, and the gate of the issue: today's row
// kernel completes 6.16 G rows/s at 0.946 of its own probe, so the list form can only win above 6.5 G rows/s.
// build+run on the GPU box:  hipcc -O3 --offload-arch=gfx950 profiles/row_list_probe.hip -o /tmp/row_list_probe && /tmp/row_list_probe
//   optional arguments: [log2 rows, default 26] [reads per wave, default 48]
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#define CHECK(x)                                                                                        \
    do {                                                                                                \
        hipError_t e_ = (x);                                                                            \
        if (e_ != hipSuccess) {                                                                         \
            printf("%s failed: %s (line %d)\n", #x, hipGetErrorString(e_), __LINE__);                   \
            return 1;                                                                                   \
        }                                                                                               \
    } while (0)

constexpr uint32_t kBins = 8192;
constexpr uint32_t kRowDwords = 64;     // 256 bytes
constexpr uint32_t kRowsPerRead = 704;  // 11 tiles of 64, 22 of 32

__host__ __device__ __forceinline__ uint64_t mix(uint64_t z)
{
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}

// entry j of row r: the j-th of n_r sorted distinct bins, one in every stride of 8192 / n_r; 0xFFFF from n_r on
__device__ __forceinline__ uint32_t entry(uint64_t r, uint32_t j, uint32_t n_r, uint32_t stride)
{
    if (j >= n_r) return 0xFFFFu;
    return j * stride + (uint32_t)(mix(r * 128 + j) % stride);  // <= n_r * stride - 1 <= 8191
}

__global__ __launch_bounds__(256) void fill_rows(uint32_t *__restrict__ table, uint64_t n_rows)
{
    const uint64_t n = n_rows * kRowDwords;
    const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += step) {
        const uint64_t r = i / kRowDwords;
        const uint32_t l = (uint32_t)(i % kRowDwords);
        const uint32_t n_r = 72 + (uint32_t)(mix(~r) % 20);
        const uint32_t stride = kBins / n_r;
        table[i] = entry(r, 2 * l, n_r, stride) | (entry(r, 2 * l + 1, n_r, stride) << 16);
    }
}

constexpr uint32_t kSpareDwords = 64;

// the same rows in the resident form, one wave per row: lane l holds entries 2l and 2l + 1 of the sorted list; the even bins go to the low
// halves and the odd bins to the high halves in list order (72-91 entries: neither parity passes 64), the other halves name the spare of
// the lane that reads the dword
__global__ __launch_bounds__(64) void fill_rows_ready(uint32_t *__restrict__ table, uint64_t n_rows)
{
    __shared__ uint16_t img[2 * kRowDwords];
    const uint32_t lane = threadIdx.x;
    for (uint64_t r = blockIdx.x; r < n_rows; r += gridDim.x) {
        const uint32_t n_r = 72 + (uint32_t)(mix(~r) % 20);
        const uint32_t stride = kBins / n_r;
        const uint32_t e[2] = {entry(r, 2 * lane, n_r, stride), entry(r, 2 * lane + 1, n_r, stride)};
        __builtin_amdgcn_wave_barrier();
        img[2 * lane] = img[2 * lane + 1] = (uint16_t)((kBins / 2 + lane) * 4);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
        __builtin_amdgcn_wave_barrier();
        const uint64_t below = (1ull << lane) - 1;
        uint32_t at[2] = {0, 0};  // even and odd bins in the lanes below
        for (int j = 0; j < 2; ++j) {
            at[0] += (uint32_t)__popcll(__ballot(e[j] < kBins && !(e[j] & 1u)) & below);
            at[1] += (uint32_t)__popcll(__ballot(e[j] < kBins && (e[j] & 1u)) & below);
        }
        for (int j = 0; j < 2; ++j)
            if (e[j] < kBins) {
                const uint32_t par = e[j] & 1u;
                const uint32_t pos = at[par]++;
                if (pos < kRowDwords) img[2 * pos + par] = (uint16_t)((e[j] >> 1) * 4);
            }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
        __builtin_amdgcn_wave_barrier();
        table[r * kRowDwords + lane] = reinterpret_cast<const uint32_t *>(img)[lane];
    }
}

typedef unsigned short probe_u16x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ void add2(uint32_t *cnt, uint32_t v, uint32_t spare)
{
    __hip_atomic_fetch_add(&cnt[min((v & 0xFFFFu) >> 1, spare)], 1u << ((v << 4) & 16u), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    __hip_atomic_fetch_add(&cnt[min(v >> 17, spare)], 1u << ((v >> 12) & 16u), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

__device__ __forceinline__ void add2_ready(uint32_t *cnt, uint32_t v)
{
    char *base = reinterpret_cast<char *>(cnt);
    __hip_atomic_fetch_add(reinterpret_cast<uint32_t *>(base + (v & 0xFFFFu)), 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    __hip_atomic_fetch_add(reinterpret_cast<uint32_t *>(base + (v >> 16)), 0x10000u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

__device__ __forceinline__ uint32_t scan_and_clear(uint32_t *cnt, uint32_t lane)
{
    uint4 *c4 = reinterpret_cast<uint4 *>(cnt);
    probe_u16x2 a = {0, 0};
#pragma unroll
    for (uint32_t i = 0; i < kBins / 2 / 4 / 64; ++i) {
        const uint4 q = c4[i * 64 + lane];
        a = __builtin_elementwise_max(a, __builtin_elementwise_max(__builtin_elementwise_max(__builtin_bit_cast(probe_u16x2, q.x), __builtin_bit_cast(probe_u16x2, q.y)),
                                                                   __builtin_elementwise_max(__builtin_bit_cast(probe_u16x2, q.z), __builtin_bit_cast(probe_u16x2, q.w))));
        c4[i * 64 + lane] = make_uint4(0, 0, 0, 0);
    }
    uint32_t m = max((uint32_t)a.x, (uint32_t)a.y);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, d, 64));
    return m;
}

// the scan and rolling modes: kBins / 2 + kSpareDwords dwords of LDS
template <int R, bool NT, bool ROLLING, bool READY = false>
__global__ __launch_bounds__(64) void list_probe_scan(const uint32_t *__restrict__ table, uint32_t lg_rows, uint32_t reads, uint32_t *out)
{
    extern __shared__ uint32_t cnt[];
    constexpr int G = 8;
    constexpr uint32_t T = kRowsPerRead / R;
    const uint32_t lane = threadIdx.x;
    const uint32_t spare = kBins / 2 + lane;
    uint32_t best = 0;
    uint64_t s = mix((uint64_t)blockIdx.x + 1);
    scan_and_clear(cnt, lane);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    uint32_t v[R];
    s += 0x9E3779B97F4A7C15ULL;
    uint32_t mine = (uint32_t)(mix(s + lane) >> (64 - lg_rows));
    if constexpr (ROLLING) {
#pragma unroll
        for (int u = 0; u < R; ++u) {
            const uint32_t *p = table + (size_t)(uint32_t)__builtin_amdgcn_readlane((int)mine, u) * kRowDwords + lane;
            v[u] = NT ? __builtin_nontemporal_load(p) : *p;
        }
    }
#pragma unroll 1
    for (uint32_t t = 0; t < reads * T; ++t) {
        if constexpr (!ROLLING) {
#pragma unroll
            for (int u = 0; u < R; ++u) {
                const uint32_t *p = table + (size_t)(uint32_t)__builtin_amdgcn_readlane((int)mine, u) * kRowDwords + lane;
                v[u] = NT ? __builtin_nontemporal_load(p) : *p;
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        s += 0x9E3779B97F4A7C15ULL;
        mine = (uint32_t)(mix(s + lane) >> (64 - lg_rows));  // the next tile's rows
#pragma unroll
        for (int g = 0; g < R / G; ++g) {
#pragma unroll
            for (int u = 0; u < G; ++u) {
                if constexpr (READY) add2_ready(cnt, v[g * G + u]);
                else add2(cnt, v[g * G + u], spare);
            }
            if constexpr (ROLLING) {
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int u = 0; u < G; ++u) {
                    const uint32_t *p = table + (size_t)(uint32_t)__builtin_amdgcn_readlane((int)mine, g * G + u) * kRowDwords + lane;
                    v[g * G + u] = NT ? __builtin_nontemporal_load(p) : *p;
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        if (t % T == T - 1) {  // a read ends
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
            best = max(best, scan_and_clear(cnt, lane));
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
        }
    }
    uint32_t acc = 0;
    if constexpr (ROLLING) {
#pragma unroll
        for (int u = 0; u < R; ++u) acc ^= v[u];  // the last refill is waited for and used
    }
    if ((best ^ acc) == 0x12345678u) out[0] = best;
}

template <int R, bool NT, bool LDS>
__global__ __launch_bounds__(64) void list_probe(const uint32_t *__restrict__ table, uint32_t lg_rows, uint32_t reads, uint32_t *out)
{
    extern __shared__ uint32_t cnt[];  // kBins / 2 dwords, given at the launch so that the build without the adds keeps the occupancy
    const uint32_t lane = threadIdx.x;
    uint32_t best = 0, acc = 0;
    uint64_t s = mix((uint64_t)blockIdx.x + 1);
    for (uint32_t rd = 0; rd < reads; ++rd) {
        if constexpr (LDS) {
            uint4 *c4 = reinterpret_cast<uint4 *>(cnt);
#pragma unroll
            for (uint32_t i = 0; i < kBins / 2 / 4 / 64; ++i) c4[i * 64 + lane] = make_uint4(0, 0, 0, 0);
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
            __builtin_amdgcn_wave_barrier();
        }
        uint32_t m = 0;
#pragma unroll 1
        for (uint32_t t = 0; t < kRowsPerRead / R; ++t) {
            s += 0x9E3779B97F4A7C15ULL;
            const uint32_t mine = (uint32_t)(mix(s + lane) >> (64 - lg_rows));  // this lane's row number, < 2^lg_rows
            uint32_t v[R];
#pragma unroll
            for (int u = 0; u < R; ++u) {
                const uint32_t row = (uint32_t)__builtin_amdgcn_readlane((int)mine, u % 64);
                const uint32_t *p = table + (size_t)row * kRowDwords + lane;
                if constexpr (NT) v[u] = __builtin_nontemporal_load(p);
                else v[u] = *p;
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int u = 0; u < R; ++u) {
                if constexpr (LDS) {
                    const uint32_t b0 = v[u] & 0xFFFFu, b1 = v[u] >> 16;
                    if (b0 < kBins) {  // also the bound of the LDS index: bin >> 1 < 4096
                        const uint32_t sh = (b0 & 1u) * 16u;
                        const uint32_t old = __hip_atomic_fetch_add(&cnt[b0 >> 1], 1u << sh, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                        m = max(m, ((old >> sh) & 0xFFFFu) + 1u);
                    }
                    if (b1 < kBins) {
                        const uint32_t sh = (b1 & 1u) * 16u;
                        const uint32_t old = __hip_atomic_fetch_add(&cnt[b1 >> 1], 1u << sh, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                        m = max(m, ((old >> sh) & 0xFFFFu) + 1u);
                    }
                } else {
                    acc ^= v[u];
                }
            }
        }
        best = max(best, m);
    }
    if ((best ^ acc) == 0x12345678u) out[0] = best;
}

// ---- the pair mode: one 384-byte slot per k-mer for BOTH strands (the pair table's step 0)
constexpr uint32_t kPairDwords = 96;                  // three lines
constexpr uint32_t kPairKmers = kRowsPerRead / 2;     // 352 k-mers per read: five tiles of 64 and one of 32
constexpr uint32_t kPairTiles = (kPairKmers + 63) / 64;
constexpr uint32_t kPairLds = (kBins + kSpareDwords) * 4;  // one counter dword per bin (low half forward, high half reverse) and the spares

// half q of a pair slot: lines 0-1 are positional (dword l: A[l] low, B[l] high; both lists have 72-91 entries, so none is blank), line 2
// holds A[64..nA) then B[64..nB) with bit 0 naming list B, then spares (16-54 of its 64 halves are used)
__device__ __forceinline__ uint32_t pair_half(uint64_t r, uint64_t n_rows, uint32_t q)
{
    const uint32_t nA = 72 + (uint32_t)(mix(~r) % 20), nB = 72 + (uint32_t)(mix(~(r + n_rows)) % 20);
    const uint32_t sA = kBins / nA, sB = kBins / nB;
    if (q < 128) return (q & 1u) ? entry(r + n_rows, q >> 1, nB, sB) * 4u : entry(r, q >> 1, nA, sA) * 4u;
    const uint32_t i = q - 128, restA = nA - 64, restB = nB - 64;
    if (i < restA) return entry(r, 64 + i, nA, sA) * 4u;
    if (i < restA + restB) return entry(r + n_rows, 64 + i - restA, nB, sB) * 4u | 1u;
    return (kBins + i) * 4u;
}

__global__ __launch_bounds__(256) void fill_rows_pair(uint32_t *__restrict__ table, uint64_t n_rows)
{
    const uint64_t n = n_rows * kPairDwords;
    const uint64_t step = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += step) {
        const uint64_t r = i / kPairDwords;
        const uint32_t l = (uint32_t)(i % kPairDwords);
        table[i] = pair_half(r, n_rows, 2 * l) | (pair_half(r, n_rows, 2 * l + 1) << 16);
    }
}

// a line-2 dword: bits 15:2 of a half are the counter's byte offset, bit 0 says list B (add 1 << 16), evaluated for every half
__device__ __forceinline__ void add2_pair_rest(uint32_t *cnt, uint32_t v)
{
    char *base = reinterpret_cast<char *>(cnt);
    __hip_atomic_fetch_add(reinterpret_cast<uint32_t *>(base + (v & 0xFFFCu)), (v & 1u) * 0xFFFFu + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    __hip_atomic_fetch_add(reinterpret_cast<uint32_t *>(base + ((v >> 16) & 0xFFFCu)), ((v >> 16) & 1u) * 0xFFFFu + 1u, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_WORKGROUP);
}

struct PairTile {
    uint32_t v[64];  // dword `lane` of lines 0-1 of slot u
    uint32_t w[32];  // line 2 of slots 2j (lanes 0-31) and 2j + 1 (lanes 32-63)
};

// slot `mine` of lane u, as a scalar pointer (readfirstlane: the 64-bit product stays in scalar registers, the lane's dword is the
// load's vector offset)
typedef const uint32_t __attribute__((address_space(1))) *pair_gptr;  // global, so that the loads are global_load and count on vmcnt alone
__device__ __forceinline__ pair_gptr pair_slot(const uint32_t *__restrict__ table, uint32_t mine, int u)
{
    const uint64_t a = reinterpret_cast<uint64_t>(table) + (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)mine, u) * (kPairDwords * 4);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)a), hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(a >> 32));
    return reinterpret_cast<pair_gptr>(((uint64_t)hi << 32) | lo);
}

// COUNT slots (64, or 32 for a read's last tile), group by group: eight loads of lines 0-1 and four of line 2, in this order
template <bool NT, int COUNT>
__device__ __forceinline__ void pair_load_n(PairTile &t, const uint32_t *__restrict__ table, uint32_t mine, uint32_t lane)
{
#pragma unroll
    for (int g = 0; g < COUNT / 8; ++g) {
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const pair_gptr p = pair_slot(table, mine, g * 8 + u) + lane;
            t.v[g * 8 + u] = NT ? __builtin_nontemporal_load(p) : *p;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const pair_gptr r0 = pair_slot(table, mine, g * 8 + 2 * j), r1 = pair_slot(table, mine, g * 8 + 2 * j + 1);
            const pair_gptr p = (lane < 32 ? r0 : r1) + 64 + (lane & 31u);
            t.w[g * 4 + j] = NT ? __builtin_nontemporal_load(p) : *p;
        }
        __builtin_amdgcn_sched_barrier(0);
    }
}

template <int COUNT>
__device__ __forceinline__ void pair_add_n(const PairTile &t, uint32_t *cnt, uint32_t *flagged)
{
#pragma unroll
    for (int g = 0; g < COUNT / 8; ++g) {
        uint32_t fold = 0;  // the overflow test of the kernel: one per group, on lines 0-1 (no slot of this table is flagged)
#pragma unroll
        for (int u = 0; u < 8; ++u) fold |= t.v[g * 8 + u];
        *flagged += (uint32_t)(__ballot((fold & 0x00020002u) != 0u) != 0ULL);  // no branch: the compiler sinks the later groups' loads behind one
#pragma unroll
        for (int u = 0; u < 8; ++u) add2_ready(cnt, t.v[g * 8 + u]);
#pragma unroll
        for (int j = 0; j < 4; ++j) add2_pair_rest(cnt, t.w[g * 4 + j]);
        __builtin_amdgcn_sched_barrier(0);
    }
}

template <int NW>
__device__ __forceinline__ uint32_t pair_scan_and_clear(uint32_t *cnt, uint32_t wave, uint32_t lane)
{
    uint4 *c4 = reinterpret_cast<uint4 *>(cnt);
    probe_u16x2 a = {0, 0};
#pragma unroll
    for (uint32_t i = 0; i < kBins / 4 / 64 / NW; ++i) {
        const uint32_t at = (i * NW + wave) * 64 + lane;  // < kBins / 4
        const uint4 q = c4[at];
        a = __builtin_elementwise_max(a, __builtin_elementwise_max(__builtin_elementwise_max(__builtin_bit_cast(probe_u16x2, q.x), __builtin_bit_cast(probe_u16x2, q.y)),
                                                                   __builtin_elementwise_max(__builtin_bit_cast(probe_u16x2, q.z), __builtin_bit_cast(probe_u16x2, q.w))));
        c4[at] = make_uint4(0, 0, 0, 0);
    }
    uint32_t m = max((uint32_t)a.x, (uint32_t)a.y);  // the maximum over both strands
    m = max(m, (uint32_t)__builtin_amdgcn_ds_swizzle((int)m, 0x401F));  // lane ^ 16, ^ 8, ... ^ 1: no index registers kept over the tile loop
    m = max(m, (uint32_t)__builtin_amdgcn_ds_swizzle((int)m, 0x201F));
    m = max(m, (uint32_t)__builtin_amdgcn_ds_swizzle((int)m, 0x101F));
    m = max(m, (uint32_t)__builtin_amdgcn_ds_swizzle((int)m, 0x081F));
    m = max(m, (uint32_t)__builtin_amdgcn_ds_swizzle((int)m, 0x041F));
    return max((uint32_t)__builtin_amdgcn_readlane((int)m, 0), (uint32_t)__builtin_amdgcn_readlane((int)m, 32));
}

// One workgroup of NW waves per read on one counter array, tile t of a read to wave t mod NW.  DB: a wave issues its next tile's gathers
// before its current tile's adds (two tiles of registers).
template <int NW, bool DB, bool NT>
__global__ __launch_bounds__(64 * NW, NW) void pair_probe(  // four workgroups per CU: NW waves per SIMD
const uint32_t *__restrict__ table, uint32_t lg_rows, uint32_t reads, uint32_t *out)
{
    extern __shared__ uint32_t cnt[];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    uint32_t best = 0, flagged = 0;
    uint64_t s = mix((uint64_t)blockIdx.x * NW + wave + 1);
    pair_scan_and_clear<NW>(cnt, wave, lane);
    if (wave == 0) cnt[kBins + lane] = 0;
    __syncthreads();
#pragma unroll 1
    for (uint32_t rd = 0; rd < reads; ++rd) {
#define PAIR_DRAW() (s += 0x9E3779B97F4A7C15ULL, (uint32_t)(mix(s + lane) >> (64 - lg_rows)))
        if constexpr (DB) {  // NW == 1: the read's tiles in a fixed order, 64 64 64 64 64 32
            static_assert(NW == 1 && kPairTiles == 6 && kPairKmers % 64 == 32, "the two-tile order is written out for one wave");
            PairTile a, b;
            pair_load_n<NT, 64>(a, table, PAIR_DRAW(), lane);
#pragma unroll 1
            for (int i = 0; i < 2; ++i) {
                pair_load_n<NT, 64>(b, table, PAIR_DRAW(), lane);
                pair_add_n<64>(a, cnt, &flagged);
                pair_load_n<NT, 64>(a, table, PAIR_DRAW(), lane);
                pair_add_n<64>(b, cnt, &flagged);
            }
            pair_load_n<NT, 32>(b, table, PAIR_DRAW(), lane);
            pair_add_n<64>(a, cnt, &flagged);
            pair_add_n<32>(b, cnt, &flagged);
        } else {
#pragma unroll 1
            for (uint32_t t = wave; t < kPairTiles; t += NW) {  // wave-uniform
                PairTile a;
                const uint32_t mine = PAIR_DRAW();
                if (t * 64u + 64u <= kPairKmers) {
                    pair_load_n<NT, 64>(a, table, mine, lane);
                    pair_add_n<64>(a, cnt, &flagged);
                } else {
                    pair_load_n<NT, kPairKmers % 64>(a, table, mine, lane);
                    pair_add_n<kPairKmers % 64>(a, cnt, &flagged);
                }
            }
        }
#undef PAIR_DRAW
        __syncthreads();  // a read ends
        best = max(best, pair_scan_and_clear<NW>(cnt, wave, lane));
        __syncthreads();
    }
    if ((best ^ flagged) == 0x12345678u) out[0] = best;
}

template <int NW, bool DB, bool NT>
static int run_pair(const uint32_t *table, uint32_t lg_rows, uint32_t reads, uint32_t *out, double *kmers_per_s)
{
    const int blocks = 256 * 4 * 8;  // four workgroups per CU is what 32 KiB of counters allow, eight rounds
    hipEvent_t a, b;
    CHECK(hipEventCreate(&a));
    CHECK(hipEventCreate(&b));
    float best = 1e30f;
    for (int rep = 0; rep < 4; ++rep) {
        CHECK(hipEventRecord(a));
        hipLaunchKernelGGL((pair_probe<NW, DB, NT>), dim3(blocks), dim3(64 * NW), kPairLds, 0, table, lg_rows, reads, out);
        CHECK(hipGetLastError());
        CHECK(hipEventRecord(b));
        CHECK(hipEventSynchronize(b));
        float ms = 0;
        CHECK(hipEventElapsedTime(&ms, a, b));
        if (rep && ms < best) best = ms;
    }
    const double kmers = (double)blocks * reads * kPairKmers;
    *kmers_per_s = kmers / best / 1e6;  // G k-mers/s
    printf("pair   %d wave%s %-8s  %-8s : %7.2f G k-mers/s  %7.2f G lines/s  (%.1f ms)\n", NW, NW > 1 ? "s" : " ", DB ? "two-tile" : "one-tile",
           NT ? "nt" : "temporal", *kmers_per_s, 3.0 * *kmers_per_s, best);
    fflush(stdout);
    CHECK(hipEventDestroy(a));
    CHECK(hipEventDestroy(b));
    return 0;
}

template <int R, bool NT, bool LDS, int MODE = 0>
static int run(const uint32_t *table, uint32_t lg_rows, uint32_t reads, uint32_t *out, double *rows_per_s)
{
    const int blocks = 256 * 10 * 8;  // ten waves per CU, eight rounds
    hipEvent_t a, b;
    CHECK(hipEventCreate(&a));
    CHECK(hipEventCreate(&b));
    float best = 1e30f;
    for (int rep = 0; rep < 4; ++rep) {
        CHECK(hipEventRecord(a));
        if constexpr (MODE == 0)
            hipLaunchKernelGGL((list_probe<R, NT, LDS>), dim3(blocks), dim3(64), kBins * 2, 0, table, lg_rows, reads, out);
        else if constexpr (MODE == 3)
            hipLaunchKernelGGL((list_probe_scan<R, NT, false, true>), dim3(blocks), dim3(64), kBins * 2 + kSpareDwords * 4, 0, table, lg_rows, reads, out);
        else
            hipLaunchKernelGGL((list_probe_scan<R, NT, MODE == 2>), dim3(blocks), dim3(64), kBins * 2 + kSpareDwords * 4, 0, table, lg_rows, reads, out);
        CHECK(hipGetLastError());
        CHECK(hipEventRecord(b));
        CHECK(hipEventSynchronize(b));
        float ms = 0;
        CHECK(hipEventElapsedTime(&ms, a, b));
        if (rep && ms < best) best = ms;
    }
    const double rows = (double)blocks * reads * kRowsPerRead;
    *rows_per_s = rows / best / 1e6;  // G rows/s
    printf("rows in flight %2d  %-8s  %-8s : %7.2f G rows/s  %7.2f G lines/s  (%.1f ms)\n", R, NT ? "nt" : "temporal",
           MODE == 3 ? "ready" : MODE == 2 ? "rolling" : MODE == 1 ? "scan" : LDS ? "lds adds" : "no lds", *rows_per_s, 2.0 * *rows_per_s, best);
    fflush(stdout);
    CHECK(hipEventDestroy(a));
    CHECK(hipEventDestroy(b));
    return 0;
}

int main(int argc, char **argv)
{
    const uint32_t lg_rows = argc > 1 ? (uint32_t)atoi(argv[1]) : 26;
    const uint32_t reads = argc > 2 ? (uint32_t)atoi(argv[2]) : 48;
    const bool addready = argc > 3 && !strcmp(argv[3], "addready");
    const bool pair = argc > 3 && !strcmp(argv[3], "pair");
    if (lg_rows < 10 || lg_rows > 26 || reads < 1 || reads > 4096 || (argc > 3 && !addready && !pair)) {
        printf("usage: row_list_probe [log2 rows 10..26] [reads per wave 1..4096] [addready | pair]\n");
        return 2;
    }
    const uint64_t n_rows = 1ULL << lg_rows;
    const size_t bytes = (size_t)n_rows * kRowDwords * 4;
    uint32_t *table = nullptr, *out = nullptr;
    if (pair) {  // the pair table's gate: a k-mer's pair slot in at most 0.90 of the time `ready` takes for its two rows, in every round
        const size_t pair_bytes = (size_t)n_rows * kPairDwords * 4;
        uint32_t *slots = nullptr;
        CHECK(hipMalloc(&table, bytes));
        CHECK(hipMalloc(&slots, pair_bytes));
        CHECK(hipMalloc(&out, 4));
        hipLaunchKernelGGL(fill_rows_ready, dim3(256 * 64), dim3(64), 0, 0, table, n_rows);
        CHECK(hipGetLastError());
        hipLaunchKernelGGL(fill_rows_pair, dim3(256 * 32), dim3(256), 0, 0, slots, n_rows);
        CHECK(hipGetLastError());
        CHECK(hipDeviceSynchronize());
        const uint32_t pair_reads = reads * 5 / 2;  // 4 workgroups per CU against 10: the same k-mers per launch
        printf("ready table: 2^%u rows of 256 bytes = %.2f GiB, %u reads of %u rows per wave, 10 waves per CU\n", lg_rows, bytes / 1073741824.0, reads,
               kRowsPerRead);
        printf("pair table : 2^%u slots of 384 bytes = %.2f GiB, 2 x 72-91 of 192 entries per slot; %u reads of %u k-mers per workgroup, 4 per CU\n",
               lg_rows, pair_bytes / 1073741824.0, pair_reads, kPairKmers);
        const char *name[5] = {"1 wave two-tile", "2 waves one-tile", "4 waves one-tile temporal", "4 waves one-tile", "1 wave one-tile"};
        double worst[5] = {0, 0, 0, 0, 0};
        for (int rep = 0; rep < 3; ++rep) {
            double rdy, p[5];
            if (run<64, true, true, 3>(table, lg_rows, reads, out, &rdy)) return 1;
            if (run_pair<1, true, true>(slots, lg_rows, pair_reads, out, &p[0])) return 1;
            if (run_pair<2, false, true>(slots, lg_rows, pair_reads, out, &p[1])) return 1;
            if (run_pair<4, false, false>(slots, lg_rows, pair_reads, out, &p[2])) return 1;
            if (run_pair<4, false, true>(slots, lg_rows, pair_reads, out, &p[3])) return 1;
            if (run_pair<1, false, true>(slots, lg_rows, pair_reads, out, &p[4])) return 1;
            printf("round %d, time per k-mer over ready's time for two rows:", rep + 1);
            for (int i = 0; i < 5; ++i) {
                const double ratio = (rdy / 2.0) / p[i];  // (1 / p) / (2 / rdy)
                worst[i] = ratio > worst[i] ? ratio : worst[i];
                printf("  %s x%.4f", name[i], ratio);
            }
            printf("\n");
        }
        int pick = 0;
        for (int i = 1; i < 5; ++i) pick = worst[i] < worst[pick] ? i : pick;
        printf("best: %s, x%.4f in its slowest round; gate x0.90: %s\n", name[pick], worst[pick], worst[pick] <= 0.90 ? "go on" : "stop");
        CHECK(hipFree(slots));
        CHECK(hipFree(table));
        CHECK(hipFree(out));
        return 0;
    }
    CHECK(hipMalloc(&table, bytes));
    CHECK(hipMalloc(&out, 4));
    hipLaunchKernelGGL(fill_rows, dim3(256 * 32), dim3(256), 0, 0, table, n_rows);
    CHECK(hipGetLastError());
    CHECK(hipDeviceSynchronize());
    printf("table: 2^%u rows of 256 bytes = %.2f GiB, 72-91 of 128 entries per row; %u reads of %u rows per wave, 10 waves per CU\n", lg_rows,
           bytes / 1073741824.0, reads, kRowsPerRead);
    double g[16];
    int i = 0;
    if (addready) {  // the resident form beside the canonical one: is the two-instruction add worth a kernel change?
        uint32_t *ready = nullptr;
        CHECK(hipMalloc(&ready, bytes));
        hipLaunchKernelGGL(fill_rows_ready, dim3(256 * 64), dim3(64), 0, 0, ready, n_rows);
        CHECK(hipGetLastError());
        CHECK(hipDeviceSynchronize());
        double nolds, scan[3], rdy[3];
        if (run<64, true, false>(table, lg_rows, reads, out, &nolds)) return 1;
        for (int rep = 0; rep < 3; ++rep) {
            if (run<64, true, true, 1>(table, lg_rows, reads, out, &scan[rep])) return 1;
            if (run<64, true, true, 3>(ready, lg_rows, reads, out, &rdy[rep])) return 1;
        }
        double lo[2] = {scan[0], rdy[0]}, hi[2] = {scan[0], rdy[0]};
        for (int rep = 1; rep < 3; ++rep) {
            lo[0] = scan[rep] < lo[0] ? scan[rep] : lo[0], hi[0] = scan[rep] > hi[0] ? scan[rep] : hi[0];
            lo[1] = rdy[rep] < lo[1] ? rdy[rep] : lo[1], hi[1] = rdy[rep] > hi[1] ? rdy[rep] : hi[1];
        }
        printf("scan  %.2f .. %.2f G rows/s (spread %.2f %%), ready %.2f .. %.2f G rows/s (spread %.2f %%), no lds %.2f\n", lo[0], hi[0],
               100.0 * (hi[0] - lo[0]) / lo[0], lo[1], hi[1], 100.0 * (hi[1] - lo[1]) / lo[1], nolds);
        printf("ready over scan: x%.4f (slowest ready over fastest scan: x%.4f): %s\n", (rdy[0] + rdy[1] + rdy[2]) / (scan[0] + scan[1] + scan[2]),
               lo[1] / hi[0], lo[1] / hi[0] > 1.0 + (hi[0] - lo[0]) / lo[0] ? "go on" : "stop");
        CHECK(hipFree(ready));
        CHECK(hipFree(table));
        CHECK(hipFree(out));
        return 0;
    }
    if (run<32, true, true>(table, lg_rows, reads, out, &g[i++])) return 1;
    if (run<64, true, true>(table, lg_rows, reads, out, &g[i++])) return 1;
    if (run<32, false, true>(table, lg_rows, reads, out, &g[i++])) return 1;
    if (run<64, false, true>(table, lg_rows, reads, out, &g[i++])) return 1;
    if (run<32, true, false>(table, lg_rows, reads, out, &g[i++])) return 1;
    if (run<64, true, false>(table, lg_rows, reads, out, &g[i++])) return 1;
    if (run<32, false, false>(table, lg_rows, reads, out, &g[i++])) return 1;
    if (run<64, false, false>(table, lg_rows, reads, out, &g[i++])) return 1;
    // the count code the kernel has since taken, and the rolling refill on top of it (issue: build it if it gains more than 5 %)
    if (run<64, true, true, 1>(table, lg_rows, reads, out, &g[i++])) return 1;
    if (run<64, true, true, 2>(table, lg_rows, reads, out, &g[i++])) return 1;
    if (run<64, false, true, 1>(table, lg_rows, reads, out, &g[i++])) return 1;
    if (run<64, false, true, 2>(table, lg_rows, reads, out, &g[i++])) return 1;
    if (run<32, true, true, 1>(table, lg_rows, reads, out, &g[i++])) return 1;
    if (run<32, true, true, 2>(table, lg_rows, reads, out, &g[i++])) return 1;
    printf("rolling over scan, 64 rows in flight, nt: x%.4f\n", g[9] / g[8]);
    double best = 0;
    for (int k = 0; k < 4; ++k) best = g[k] > best ? g[k] : best;
    printf("best with the LDS adds: %.2f G rows/s; gate 6.50 G rows/s (6.16 / 0.946): %s\n", best, best > 6.5 ? "go on" : "stop");
    CHECK(hipFree(table));
    CHECK(hipFree(out));
    return 0;
}

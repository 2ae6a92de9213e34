// rb_resume_planes.h -- the arithmetic of the MERGE that ends a strand in ibf_resume_lists_kernel (rb_resume_lists.hip): one column of the
// list kernels' LDS counters -- 64 bins as 32 dwords, bin b in half b & 1 of dword b >> 1 -- becomes sixteen bit-sliced 64-bit DELTA
// planes (bit b of plane i = bit i of bin b's counter), which a ripple carry adds onto the slot's sixteen planes of that column.
// Host and device: tests/cpp/test_resume_lists.cpp compiles it alone, plain and with sanitizers, against plain uint16_t arithmetic.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define RB_PLANES_HD __host__ __device__ __forceinline__
#define RB_PLANES_UNROLL _Pragma("unroll")
#else
#define RB_PLANES_HD inline
#define RB_PLANES_UNROLL
#endif

namespace rbplanes {

constexpr int kPlanes = 16;        // == kResumePlanes: the counters wrap at 2^16
constexpr int kColumnDwords = 32;  // 64 bins of 16 bits

// One log step of the bit-matrix transpose.  The 1024 bits of a column have a 10-bit index: five bits name the dword, five the place
// in it.  A step exchanges dword-index bit RBIT with place bit PBIT: for every pair of dwords (u, v) that differ in RBIT alone, the
// bits of u at places with PBIT set change places with the bits of v at places with PBIT clear.  Two vector instructions per result
// (a shift and a bit-field insert), four per pair, 64 per step.  A step is its own inverse.
template <int RBIT, int PBIT>
RB_PLANES_HD void exchange_step(uint32_t x[kColumnDwords])
{
    constexpr uint32_t s = 1u << PBIT;
    constexpr uint32_t m = PBIT == 0 ? 0x55555555u : PBIT == 1 ? 0x33333333u : PBIT == 2 ? 0x0F0F0F0Fu : PBIT == 3 ? 0x00FF00FFu : 0x0000FFFFu;
    RB_PLANES_UNROLL
    for (int d = 0; d < kColumnDwords; ++d) {
        if (d & (1 << RBIT)) continue;
        const uint32_t u = x[d], v = x[d | (1 << RBIT)];
        x[d] = (u & m) | ((v << s) & ~m);
        x[d | (1 << RBIT)] = ((u >> s) & m) | (v & ~m);
    }
}

// Where the index bits stand.  Counters as loaded: dword index (b5 b4 b3 b2 b1), place (b0 i3 i2 i1 i0) -- b the bin of the column, i the
// bit of its counter.  Planes want the place to be (b4 b3 b2 b1 b0).  Five steps: b4 takes b0's place at the top (b0 waits in the dword
// index), b0 then takes i0's place, and b1, b2, b3 those of i1, i2, i3.  Afterwards the dword index reads (b5 i0 i3 i2 i1).
RB_PLANES_HD void exchange_forward(uint32_t x[kColumnDwords])
{
    exchange_step<3, 4>(x);
    exchange_step<3, 0>(x);
    exchange_step<0, 1>(x);
    exchange_step<1, 2>(x);
    exchange_step<2, 3>(x);
}
RB_PLANES_HD void exchange_backward(uint32_t x[kColumnDwords])
{
    exchange_step<2, 3>(x);
    exchange_step<1, 2>(x);
    exchange_step<0, 1>(x);
    exchange_step<3, 0>(x);
    exchange_step<3, 4>(x);
}
// the dword that holds bins 32 * half .. 32 * half + 31 of plane i after exchange_forward
constexpr int plane_dword(int i, int half) { return (half << 4) | ((i & 1) << 3) | (((i >> 3) & 1) << 2) | (((i >> 2) & 1) << 1) | ((i >> 1) & 1); }

// 16 x 64 -> 64 x 16: the column's counters (destroyed) to its sixteen planes ...
RB_PLANES_HD void counters_to_planes(uint32_t c[kColumnDwords], uint64_t plane[kPlanes])
{
    exchange_forward(c);
    RB_PLANES_UNROLL
    for (int i = 0; i < kPlanes; ++i) plane[i] = (uint64_t)c[plane_dword(i, 0)] | ((uint64_t)c[plane_dword(i, 1)] << 32);
}
// ... and back
RB_PLANES_HD void planes_to_counters(const uint64_t plane[kPlanes], uint32_t c[kColumnDwords])
{
    RB_PLANES_UNROLL
    for (int i = 0; i < kPlanes; ++i) {
        c[plane_dword(i, 0)] = (uint32_t)plane[i];
        c[plane_dword(i, 1)] = (uint32_t)(plane[i] >> 32);
    }
    exchange_backward(c);
}

// A plane whose bins were read 8 * pieces places low (the kernel reads the column's eight 16-byte pieces in a rotated order, to keep the
// LDS banks apart): every bin moves up by 8 * pieces, around the column's 64.
RB_PLANES_HD uint64_t rotate_bins(uint64_t plane, uint32_t pieces)
{
    const uint32_t s = (pieces & 7u) * 8u;
    return (plane << s) | (plane >> ((64u - s) & 63u));
}

// state += delta, per bin, modulo 2^16: a ripple carry up the sixteen planes.  The carry out of plane 15 is dropped -- the uint16_t wrap
// of the reference's counts -- and a carry moves between planes at its own bit only, never from one bin to another.
RB_PLANES_HD void ripple_add(uint64_t state[kPlanes], const uint64_t delta[kPlanes])
{
    uint64_t carry = 0;
    RB_PLANES_UNROLL
    for (int i = 0; i < kPlanes; ++i) {
        const uint64_t s = state[i], d = delta[i], t = s ^ d;
        state[i] = t ^ carry;
        carry = (s & d) | (t & carry);
    }
}

// the largest counter among the bins of `valid`, from the planes, most significant plane first: the candidates are narrowed to those
// with the plane's bit set wherever one of them has it
RB_PLANES_HD uint32_t planes_column_max(const uint64_t plane[kPlanes], uint64_t valid)
{
    uint64_t cand = valid;
    uint32_t m = 0;
    RB_PLANES_UNROLL
    for (int i = kPlanes - 1; i >= 0; --i) {
        const uint64_t t = cand & plane[i];
        if (t) {
            cand = t;
            m |= 1u << i;
        }
    }
    return m;
}

}  // namespace rbplanes

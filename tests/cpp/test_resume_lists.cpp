// The merge arithmetic of the resume pass's list form (readbouncer_amd/csrc/rb_resume_planes.h) against plain uint16_t arithmetic: the
// transpose of a column's 64 counters into sixteen planes, the rotation that undoes the kernel's rotated piece order, the ripple add
// with its wrap at 2^16, and the column maximum; and the LDS bytes of a workgroup (rb_lists.h).  Stand-alone: compiled plain and under the address and undefined-behaviour sanitizers
// by tests/test_resume_lists_cpu.py.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>

#include "../../readbouncer_amd/csrc/rb_lists.h"
#include "../../readbouncer_amd/csrc/rb_resume_planes.h"

using namespace rbplanes;

static int failures = 0;
#define CHECK(cond, ...)                       \
    do {                                       \
        if (!(cond)) {                         \
            ++failures;                        \
            if (failures <= 20) {              \
                std::printf("FAIL %s: ", #cond); \
                std::printf(__VA_ARGS__);      \
                std::printf("\n");             \
            }                                  \
        }                                      \
    } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd()
{
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}

// the LDS layout: bin b in half b & 1 of dword b >> 1
static void pack(const uint16_t bins[64], uint32_t c[kColumnDwords])
{
    for (int d = 0; d < kColumnDwords; ++d) c[d] = (uint32_t)bins[2 * d] | ((uint32_t)bins[2 * d + 1] << 16);
}
// the definition of the planes, one bit at a time
static void slow_planes(const uint16_t bins[64], uint64_t plane[kPlanes])
{
    for (int i = 0; i < kPlanes; ++i) {
        plane[i] = 0;
        for (int b = 0; b < 64; ++b) plane[i] |= (uint64_t)((bins[b] >> i) & 1u) << b;
    }
}
static void slow_bins(const uint64_t plane[kPlanes], uint16_t bins[64])
{
    for (int b = 0; b < 64; ++b) {
        bins[b] = 0;
        for (int i = 0; i < kPlanes; ++i) bins[b] |= (uint16_t)(((plane[i] >> b) & 1ull) << i);
    }
}

static void check_transpose(const uint16_t bins[64], const char *what)
{
    uint32_t c[kColumnDwords], back[kColumnDwords], orig[kColumnDwords];
    uint64_t got[kPlanes], want[kPlanes];
    pack(bins, c);
    std::memcpy(orig, c, sizeof c);
    counters_to_planes(c, got);
    slow_planes(bins, want);
    for (int i = 0; i < kPlanes; ++i) CHECK(got[i] == want[i], "%s plane %d got %016llx want %016llx", what, i, (unsigned long long)got[i], (unsigned long long)want[i]);
    planes_to_counters(got, back);
    CHECK(std::memcmp(back, orig, sizeof orig) == 0, "%s: there and back is not the identity", what);
}

// state + delta per bin in uint16_t against the ripple add over the planes; the maximum over `n_valid` bins
static void check_add(const uint16_t state[64], const uint16_t delta[64], int n_valid, const char *what)
{
    uint64_t sp[kPlanes], dp[kPlanes];
    slow_planes(state, sp);
    uint32_t c[kColumnDwords];
    pack(delta, c);
    counters_to_planes(c, dp);
    ripple_add(sp, dp);
    uint16_t got[64];
    slow_bins(sp, got);
    uint32_t want_max = 0;
    for (int b = 0; b < 64; ++b) {
        const uint16_t want = (uint16_t)(state[b] + delta[b]);
        CHECK(got[b] == want, "%s bin %d: %u + %u gave %u, want %u", what, b, state[b], delta[b], got[b], want);
        if (b < n_valid && want > want_max) want_max = want;
    }
    const uint64_t valid = n_valid >= 64 ? ~0ull : (1ull << n_valid) - 1ull;
    const uint32_t m = planes_column_max(sp, valid);
    CHECK(m == want_max, "%s maximum over %d bins: got %u want %u", what, n_valid, m, want_max);
}

int main(int argc, char **argv)
{
    // the LDS of a workgroup of ibf_resume_lists_kernel is the count kernel's, for the bin counts named on the command line; its columns
    // of 64 bins lie within the counters
    for (int a = 1; a < argc; ++a) {
        const uint32_t n_bins = (uint32_t)std::strtoul(argv[a], nullptr, 10);
        std::printf("resume_lds n_bins %u bytes %u resident %u\n", n_bins, rblist::count_lds_bytes(n_bins), rblist::count_resident_workgroups(n_bins));
        CHECK(((n_bins + 63u) / 64u) * (uint32_t)kColumnDwords <= rblist::count_cnt_dwords(n_bins), "columns of %u bins beyond the counters", n_bins);
    }
    // every single-bin pattern: one bin, one bit
    for (int b = 0; b < 64; ++b)
        for (int i = 0; i < kPlanes; ++i) {
            uint16_t bins[64] = {};
            bins[b] = (uint16_t)(1u << i);
            check_transpose(bins, "single bit");
        }
    // ... one bin, every value of a few kinds
    for (int b = 0; b < 64; ++b)
        for (uint32_t v : {1u, 0x7FFFu, 0x8000u, 0xFFFEu, 0xFFFFu, 0xA5C3u}) {
            uint16_t bins[64] = {};
            bins[b] = (uint16_t)v;
            check_transpose(bins, "single bin");
            uint16_t zero[64] = {};
            check_add(zero, bins, 64, "0 + single bin");
            check_add(bins, zero, 64, "single bin + 0");
        }
    // neighbours at the wrap: no carry crosses from a bin to the next, in a dword or across dwords and the column's halves
    for (int b = 0; b + 1 < 64; ++b) {
        uint16_t st[64] = {}, de[64] = {};
        st[b] = 0xFFFFu;
        de[b] = 1;  // 0xFFFF + 1 -> 0, the neighbour stays 0
        check_add(st, de, 64, "0xFFFF + 1");
        st[b + 1] = 5;
        de[b + 1] = 7;
        check_add(st, de, 64, "0xFFFF + 1 beside 5 + 7");
        de[b] = 0xFFFFu;  // 0xFFFF + 0xFFFF -> 0xFFFE
        check_add(st, de, 64, "0xFFFF + 0xFFFF");
        st[b + 1] = 0xFFFFu;
        de[b + 1] = 0xFFFFu;
        check_add(st, de, 64, "0xFFFF + 0xFFFF twice");
    }
    {
        uint16_t zero[64] = {};
        check_add(zero, zero, 64, "0 + 0");
        uint16_t full[64];
        for (int b = 0; b < 64; ++b) full[b] = 0xFFFFu;
        check_add(full, full, 64, "all 0xFFFF + all 0xFFFF");
        check_add(full, zero, 1, "one valid bin");
    }
    // seeded columns: the transpose, the add, and the maximum over the first n_valid bins
    for (int round = 0; round < 4000; ++round) {
        uint16_t st[64], de[64];
        const int kind = round & 3;
        for (int b = 0; b < 64; ++b) {
            const uint64_t r = rnd();
            st[b] = (uint16_t)r;
            de[b] = (uint16_t)(r >> 16);
            if (kind == 1) de[b] &= 0x3FFu;               // a feed's delta is small
            if (kind == 2 && (r >> 40) & 3u) st[b] = de[b] = 0;  // a sparse column
            if (kind == 3 && ((r >> 40) & 7u) == 0) st[b] = (uint16_t)(0xFFFFu - (de[b] & 3u));  // at the wrap
        }
        check_transpose(de, "seeded");
        check_add(st, de, 1 + (int)(rnd() % 64), "seeded");
    }
    // the rotated piece order: the kernel's lane reads piece (q + r) & 7 into place q; rotate_bins puts every plane right
    for (uint32_t r = 0; r < 8; ++r) {
        uint16_t bins[64], moved[64];
        for (int b = 0; b < 64; ++b) bins[b] = (uint16_t)rnd();
        for (int q = 0; q < 8; ++q)
            for (int j = 0; j < 8; ++j) moved[q * 8 + j] = bins[((q + (int)r) & 7) * 8 + j];
        uint32_t c[kColumnDwords];
        uint64_t got[kPlanes], want[kPlanes];
        pack(moved, c);
        counters_to_planes(c, got);
        slow_planes(bins, want);
        for (int i = 0; i < kPlanes; ++i) {
            const uint64_t g = rotate_bins(got[i], r);
            CHECK(g == want[i], "rotation %u plane %d got %016llx want %016llx", r, i, (unsigned long long)g, (unsigned long long)want[i]);
        }
    }
    std::printf("failures: %d\n", failures);
    return failures ? 1 : 0;
}

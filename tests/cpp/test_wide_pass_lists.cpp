// test_wide_pass_lists.cpp -- the host arithmetic of the wide forms of locate and hits (readbouncer_amd/csrc/rb_wide_lists.h:
// pass_lds_bytes, pass_rounds, pass_rounds_per_wave, pass_wave_of_bin) on a CPU, for every bin count the wide table serves: the pass
// kernels declare the count kernel's LDS and nothing more, two workgroups fit a CU at the largest bin counts, every round of the scan
// belongs to exactly one wave, the waves' shares are stretches of rising bins, and a thread never has more pieces than mask bytes.
// Built plain and with -fsanitize=address,undefined by tests/test_wide_pass_lists_cpu.py.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../readbouncer_amd/csrc/rb_wide_lists.h"

static int failures = 0;
#define CHECK(c)                                                                 \
    do {                                                                         \
        if (!(c)) { ++failures; std::fprintf(stderr, "%s:%d CHECK(%s) failed\n", __FILE__, __LINE__, #c); } \
    } while (0)

using namespace rbwide;

int main()
{
    CHECK(pass_lds_bytes(32256) == 65344 && pass_lds_bytes(31000) == 63296 && pass_lds_bytes(8193) == 18240);
    CHECK(pass_rounds(32256) == 63 && pass_rounds_per_wave(32256) == 16 && pass_rounds(31000) == 61 && pass_rounds(8193) == 17 &&
          pass_rounds_per_wave(8193) == 5);
    CHECK(pass_wave_of_bin(32256, 0) == 0 && pass_wave_of_bin(32256, 8191) == 0 && pass_wave_of_bin(32256, 8192) == 1 &&
          pass_wave_of_bin(32256, 32255) == 3 && pass_wave_of_bin(8193, 8192) == 3 && pass_wave_of_bin(8193, 5) == 0);
    for (uint32_t n_bins = kWideMinBins; n_bins <= kWideMaxBins; ++n_bins) {
        const uint32_t b = pass_lds_bytes(n_bins), rounds = pass_rounds(n_bins), per = pass_rounds_per_wave(n_bins);
        CHECK(b == count_lds_bytes(n_bins) && b <= 64u * 1024u);        // no attribute for the dynamic LDS
        CHECK(2u * b <= rblist::kLdsPerCuBytes);                          // two workgroups per CU at every bin count
        CHECK(rounds * 256u == cnt_dwords(n_bins) && rounds * 512u >= n_bins && (rounds - 1u) * 512u < n_bins + 512u);
        CHECK(per >= 1 && per <= kWidePassMaskBytes);
        // the kernels' walk: wave w at the rounds [min(w per, rounds), min(w per + per, rounds))
        std::vector<uint32_t> owner(rounds, 0xFFFFFFFFu);
        for (uint32_t w = 0; w < kWideWaves; ++w) {
            const uint32_t r0 = w * per < rounds ? w * per : rounds, r1 = r0 + per < rounds ? r0 + per : rounds;
            CHECK(r1 - r0 <= kWidePassMaskBytes);
            for (uint32_t r = r0; r < r1; ++r) {
                CHECK(owner[r] == 0xFFFFFFFFu);
                owner[r] = w;
            }
        }
        for (uint32_t r = 0; r < rounds; ++r) {
            CHECK(owner[r] != 0xFFFFFFFFu && owner[r] == pass_wave_of_bin(n_bins, r * 512u) && owner[r] == pass_wave_of_bin(n_bins, r * 512u + 511u));
            CHECK(r == 0 || owner[r] >= owner[r - 1]);
        }
        CHECK(pass_wave_of_bin(n_bins, 0) == 0 && pass_wave_of_bin(n_bins, n_bins - 1) > 0 && pass_wave_of_bin(n_bins, n_bins - 1) < kWideWaves);
    }
    std::printf("failures: %d\n", failures);
    return failures ? 1 : 0;
}

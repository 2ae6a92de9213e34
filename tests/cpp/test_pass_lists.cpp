// test_pass_lists.cpp -- what a wave of the list forms of locate and hits keeps in LDS (readbouncer_amd/csrc/rb_lists.h, pass_lds_bytes):
// the count kernel's counters, spares and stage, and one mask bit per counter half behind them.  At 8192 bins the mask must not cost a
// resident workgroup: the count kernel has nine per CU, and so have these.  Built plain by tests/test_pass_lists_cpu.py and with
// -fsanitize=address,undefined as well; the lines it prints are what that test reads.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../readbouncer_amd/csrc/rb_lists.h"

static int failures = 0;
#define CHECK(c)                                                                 \
    do {                                                                         \
        if (!(c)) { ++failures; std::fprintf(stderr, "%s:%d CHECK(%s) failed\n", __FILE__, __LINE__, #c); } \
    } while (0)

using namespace rblist;

int main(int argc, char **argv)
{
    std::vector<uint32_t> bins = {2049u, 2112u, 4090u, 4091u, 4096u, 8191u, 8192u};
    for (int i = 1; i < argc; ++i) bins.push_back((uint32_t)std::strtoul(argv[i], nullptr, 10));
    for (uint32_t n_bins : bins) {
        const uint32_t dwords = count_cnt_dwords(n_bins), mask = pass_mask_bytes(n_bins), bytes = pass_lds_bytes(n_bins);
        CHECK(mask * 8 == dwords * 2 && mask * 8 >= n_bins);  // a bit for every counter half, so for every bin
        CHECK(mask == dwords / 4 && mask % 64 == 0);          // a byte for every 16-byte piece; every lane of a round has one
        CHECK(bytes == count_lds_bytes(n_bins) + mask);       // behind the count kernel's layout
        CHECK(bytes <= 64 * 1024);                            // what one workgroup may ask for
        CHECK(pass_resident_workgroups(n_bins) * bytes <= kLdsPerCuBytes);
        // the mask as the kernels index it: piece i of the counters, bit j -> bin 8 i + j, and no piece lies outside it
        std::vector<uint8_t> m(mask, 0);
        for (uint32_t b = 0; b < n_bins; ++b) m[b / 8] |= (uint8_t)(1u << (b % 8));
        uint32_t set = 0;
        for (uint32_t i = 0; i < dwords / 4; ++i) set += (uint32_t)__builtin_popcount(m[i]);
        CHECK(set == n_bins);
        std::printf("pass_lds n_bins %u bytes %u resident %u count_resident %u\n", n_bins, bytes, pass_resident_workgroups(n_bins),
                    count_resident_workgroups(n_bins));
    }
    CHECK(pass_lds_bytes(8192) == 16768 + 1024 && pass_resident_workgroups(8192) == 9 && count_resident_workgroups(8192) == 9);
    CHECK(pass_lds_bytes(kMaxBins) <= 64 * 1024);
    std::printf("failures: %d\n", failures);
    return failures ? 1 : 0;
}

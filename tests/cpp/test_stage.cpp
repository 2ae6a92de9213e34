// test_stage.cpp -- the staging layout of the query passes (readbouncer_amd/csrc/rb_stage.h) on a CPU: seeded sequences of regions in
// any order never misalign or overlap and waste at most 15 bytes each; the table of staged outputs hands out null for an output the
// caller left out, never copies it, and lands a sub-batch's units at the right host address.  The "device" is a block of host memory.
// Built plain by tests/test_stage_cpu.py; the same program is meant to be built with -fsanitize=address,undefined as well.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "../../readbouncer_amd/csrc/rb_stage.h"

static int failures = 0;
#define CHECK(c)                                                                 \
    do {                                                                         \
        if (!(c)) { ++failures; std::fprintf(stderr, "%s:%d CHECK(%s) failed\n", __FILE__, __LINE__, #c); } \
    } while (0)

static void layouts()
{
    std::mt19937_64 rng(20260119);
    const size_t aligns[5] = {1, 2, 4, 8, 16};
    for (int seq = 0; seq < 4000; ++seq) {
        rb::StageLayout lay;
        struct Region { size_t off, bytes; };
        std::vector<Region> got;
        size_t sum = 0;
        const int n = 1 + (int)(rng() % 12);
        for (int i = 0; i < n; ++i) {
            const size_t align = aligns[rng() % 5];
            const size_t bytes = rng() % 4 == 0 ? 0 : (rng() % 3 == 0 ? 1 + rng() % 7 : 1 + rng() % 100000);
            const size_t off = i % 5 == 4 && align == 16 ? lay.take(bytes) : lay.take(bytes, align);  // (the default is 16)
            CHECK(off % align == 0);
            CHECK(off + bytes <= lay.bytes());  // the total covers every region, the last one too
            got.push_back({off, bytes});
            sum += bytes;
        }
        CHECK(lay.bytes() <= sum + 15 * (size_t)n);
        for (size_t a = 0; a < got.size(); ++a)
            for (size_t b = a + 1; b < got.size(); ++b)
                if (got[a].bytes && got[b].bytes) CHECK(got[a].off + got[a].bytes <= got[b].off || got[b].off + got[b].bytes <= got[a].off);
    }
    rb::StageLayout empty;
    CHECK(empty.bytes() == 0 && empty.take(0) == 0 && empty.bytes() == 0);
}

// A host form with three outputs of 6, 1 and 4 bytes per unit, the middle one left out or not, n units in sub-batches of sub_max
static void staged_outputs(bool with_middle, size_t n, size_t sub_max)
{
    std::vector<unsigned char> h_a(n * 6, 0xEE), h_b(n, 0xEE), h_c(n * 4, 0xEE);
    struct DevOut { void *a, *b, *c; } d_out{&h_a, &h_a, &h_a};
    rb::StageLayout lay;
    rb::StagedOuts outs;
    const size_t o_in = lay.take(3 * sub_max, 1);  // something else in the block, first: the outputs start behind it
    const size_t i_a = outs.add(lay, h_a.data(), &d_out.a, 6, sub_max, 2);
    const size_t i_b = outs.add(lay, with_middle ? h_b.data() : nullptr, &d_out.b, 1, sub_max, 1);
    const size_t i_c = outs.add(lay, h_c.data(), &d_out.c, 4, sub_max, 4);
    CHECK(outs.n == 3 && i_a == 0 && i_b == 1 && i_c == 2 && o_in == 0);
    std::vector<unsigned char> dev(lay.bytes() + 16, 0x11);  // exactly what the layout asks for (+ room to align the block itself)
    unsigned char *base = dev.data() + (16 - (uintptr_t)dev.data() % 16) % 16;
    outs.bind(base);
    CHECK(d_out.a == outs.dev(i_a, base) && d_out.b == outs.dev(i_b, base) && d_out.c == outs.dev(i_c, base));
    CHECK(d_out.a && d_out.c && (d_out.b != nullptr) == with_middle);
    CHECK((uintptr_t)d_out.a % 2 == 0 && (uintptr_t)d_out.c % 4 == 0);
    CHECK((unsigned char *)d_out.a >= base + 3 * sub_max);
    size_t copies = 0;
    for (size_t b0 = 0; b0 < n; b0 += sub_max) {
        const size_t sub = n - b0 < sub_max ? n - b0 : sub_max;
        // the "device form": unit u of the sub-batch is global unit b0 + u
        for (size_t u = 0; u < sub; ++u) {
            std::memset((unsigned char *)d_out.a + 6 * u, (int)((b0 + u) % 251), 6);
            if (d_out.b) ((unsigned char *)d_out.b)[u] = (unsigned char)((b0 + u) % 241);
            const uint32_t v = (uint32_t)(b0 + u) * 2654435761u;
            std::memcpy((unsigned char *)d_out.c + 4 * u, &v, 4);
        }
        const int rc = outs.copy_back(base, b0, sub, [&](void *dst, const void *src, size_t bytes) {
            CHECK(dst != nullptr && (const unsigned char *)src >= base && (const unsigned char *)src + bytes <= base + lay.bytes());
            std::memcpy(dst, src, bytes);
            ++copies;
            return 0;
        });
        CHECK(rc == 0);
    }
    CHECK(copies == ((n + sub_max - 1) / sub_max) * (with_middle ? 3 : 2));
    for (size_t u = 0; u < n; ++u) {
        for (int j = 0; j < 6; ++j) CHECK(h_a[6 * u + j] == u % 251);
        CHECK(h_b[u] == (with_middle ? u % 241 : 0xEE));  // a left-out output is never written
        uint32_t v;
        std::memcpy(&v, &h_c[4 * u], 4);
        CHECK(v == (uint32_t)u * 2654435761u);
    }
    // a copy that fails ends the copy-back with its status, at once
    int calls = 0;
    CHECK(outs.copy_back(base, 0, 1, [&](void *, const void *, size_t) { ++calls; return 7; }) == 7 && calls == 1);
}

int main()
{
    layouts();
    staged_outputs(true, 1000, 1000);  // one piece
    staged_outputs(true, 1000, 333);   // four, the last one short
    staged_outputs(false, 1000, 333);
    staged_outputs(false, 7, 1);
    std::printf("stage checks done, failures: %d\n", failures);
    return failures ? 1 : 0;
}

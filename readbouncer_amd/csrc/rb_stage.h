// rb_stage.h -- how the query passes (rb_engine.hip) cut one block of device memory into arrays: a layout that cannot misalign or
// overlap whatever the order of its regions, and on top of it the table of outputs a host form stages in such a block and copies back.
// Plain C++17, no HIP and no allocation: tests/cpp/test_stage.cpp checks it on a CPU.
#pragma once
#include <cassert>
#include <cstddef>

namespace rb {

struct StageLayout {
    size_t total = 0;
    // a region of `bytes` bytes (0: none, at most padding) at a multiple of `align`, a power of two; the block itself is aligned to 16 or more
    size_t take(size_t bytes, size_t align = 16)
    {
        assert(align && !(align & (align - 1)));
        const size_t off = (total + align - 1) & ~(align - 1);
        total = off + bytes;
        return off;
    }
    size_t bytes() const { return total; }  // what to `ensure`
};

// One output of a host form: the caller's array (nullptr: left out), its bytes per unit -- an item, a row or a query -- and where the
// device form writes it in the staging block.  `slot` is the member of the device-side output struct that bind() fills.
struct StagedOut {
    void *host;
    void **slot;
    size_t unit_bytes, off;
};

struct StagedOuts {
    static constexpr size_t kMax = 8;
    StagedOut o[kMax];
    size_t n = 0;
    // room for `units` units of the output in `lay` (none where the caller left it out); -> its index
    size_t add(StageLayout &lay, void *host, void **slot, size_t unit_bytes, size_t units, size_t align = 16)
    {
        assert(n < kMax);
        o[n] = StagedOut{host, slot, unit_bytes, lay.take(host ? unit_bytes * units : 0, align)};
        return n++;
    }
    void *dev(size_t i, void *base) const { return o[i].host ? (char *)base + o[i].off : nullptr; }
    void bind(void *base) const
    {
        for (size_t i = 0; i < n; ++i) *o[i].slot = dev(i, base);
    }
    // queues the copy of units [b0, b0 + sub) of every requested output, staged from unit 0 of `base`, to host + b0 * unit_bytes;
    // copy(dst, src, bytes) -> 0 or the status this returns at once
    template <class Copy>
    int copy_back(const void *base, size_t b0, size_t sub, Copy &&copy) const
    {
        for (size_t i = 0; i < n; ++i) {
            if (!o[i].host || !o[i].unit_bytes) continue;
            const int rc = copy((char *)o[i].host + b0 * o[i].unit_bytes, (const char *)base + o[i].off, sub * o[i].unit_bytes);
            if (rc) return rc;
        }
        return 0;
    }
};

}  // namespace rb

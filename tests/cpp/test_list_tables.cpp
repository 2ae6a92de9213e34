// test_list_tables.cpp -- the host side of a filter's list tables (readbouncer_amd/csrc/rb_list_tables.h) on a CPU: the whole decision of
// what a call does with a table -- current x capturing x may_build x every refusal x refused version x max_bytes, the branch for a
// capturing stream among it, which no test on a GPU takes --, the repay inequality against the two formulas the engine had written out
// (list_policy and wide_table_admitted_locked) at and around equality and at the largest operands, and what a fresh and a dropped state
// hold.  Built plain and with -fsanitize=address,undefined by tests/test_list_tables_cpu.py.
#include <cstdint>
#include <cstdio>
#include <initializer_list>

#include "../../readbouncer_amd/csrc/rb_list_tables.h"

static int failures = 0;
#define CHECK(c)                                                                 \
    do {                                                                         \
        if (!(c)) { ++failures; std::fprintf(stderr, "%s:%d CHECK(%s) failed\n", __FILE__, __LINE__, #c); } \
    } while (0)

using namespace rbtables;

static const uint32_t kRefusals[] = {RB_LIST_REFUSED_NONE,  RB_LIST_REFUSED_K,       RB_LIST_REFUSED_GEOMETRY, RB_LIST_REFUSED_MAX_BYTES, RB_LIST_REFUSED_FREE,
                                     RB_LIST_REFUSED_ALLOC, RB_LIST_REFUSED_CAPTURE, RB_LIST_REFUSED_DENSITY,  RB_LIST_REFUSED_SIDE_FULL};

static void decision_table()
{
    static_assert(sizeof kRefusals / sizeof kRefusals[0] == 9 && RB_LIST_REFUSED_SIDE_FULL == 8, "every RB_LIST_REFUSED_* value");
    const uint64_t version = 7, max_bytes = 1ull << 30;
    uint32_t slots[1] = {0};  // (never read: a table that exists)
    unsigned walked = 0, captures = 0, builds = 0, takes = 0;
    for (int is_current = 0; is_current < 2; ++is_current)
        for (int capturing = 0; capturing < 2; ++capturing)
            for (int may_build = 0; may_build < 2; ++may_build)
                for (uint32_t refused : kRefusals)
                    for (int same_version = 0; same_version < 2; ++same_version)
                        for (int same_max = 0; same_max < 2; ++same_max) {
                            ListTableState s;
                            s.table = slots;  // a table of these bits, or one the bits have moved away from
                            s.version = is_current ? version : version - 1;
                            s.refused = refused;
                            s.refused_version = same_version ? version : version - 1;
                            s.refused_max_bytes = same_max ? max_bytes : max_bytes / 2;
                            CHECK(current(s, version) == (is_current != 0));
                            // the rule of the remembered refusal, written out
                            bool stands = false;
                            switch (refused) {
                            case RB_LIST_REFUSED_NONE:
                            case RB_LIST_REFUSED_CAPTURE: stands = false; break;
                            case RB_LIST_REFUSED_MAX_BYTES: stands = same_version && same_max; break;
                            default: stands = same_version != 0; break;  // K, GEOMETRY, FREE, ALLOC, DENSITY, SIDE_FULL: until the version moves
                            }
                            CHECK(refusal_stands(s, version, max_bytes) == stands);
                            const TableCall c = table_call(current(s, version), capturing != 0, may_build != 0, refusal_stands(s, version, max_bytes));
                            ++walked;
                            captures += c.record_capture;
                            builds += c.build;
                            takes += c.take;
                            if (capturing) {
                                // nothing is taken, dropped or built, even from a current table; CAPTURE is noted where there is no current one
                                CHECK(!c.take && !c.drop_stale && !c.build);
                                CHECK(c.record_capture == !is_current);
                            } else if (is_current) {
                                CHECK(c.take && !c.drop_stale && !c.build && !c.record_capture);
                            } else {
                                // the stale table goes; a build where building is allowed and no refusal stands
                                CHECK(c.drop_stale && !c.take && !c.record_capture);
                                CHECK(c.build == (may_build && !stands));
                            }
                            // CAPTURE is recorded only where the call would otherwise have built, or where no current table exists
                            if (c.record_capture) CHECK(capturing && !is_current);
                            if (c.build) CHECK(!capturing && !is_current && may_build);
                        }
    CHECK(walked == 2 * 2 * 2 * 9 * 2 * 2);
    CHECK(captures == 2 * 9 * 4 && takes == 2 * 9 * 4);
    // not capturing, not current, may build: 9 x 4 states, of which 6 refusals stand in 2 and MAX_BYTES in 1
    CHECK(builds == 9 * 4 - 6 * 2 - 1);

    // no table at all is no current table, whatever the versions say; and a table of other bits is none
    ListTableState none;
    CHECK(!current(none, 0) && !current(none, version));
    none.version = version;
    CHECK(!current(none, version));
    // a CAPTURE refusal never stands; MAX_BYTES is lifted by another max_bytes and by a new version; the others by a new version alone
    ListTableState r;
    r.refused_version = version;
    r.refused_max_bytes = max_bytes;
    r.refused = RB_LIST_REFUSED_CAPTURE;
    CHECK(!refusal_stands(r, version, max_bytes));
    r.refused = RB_LIST_REFUSED_MAX_BYTES;
    CHECK(refusal_stands(r, version, max_bytes) && !refusal_stands(r, version, max_bytes * 2) && !refusal_stands(r, version, 0) && !refusal_stands(r, version + 1, max_bytes));
    for (uint32_t refused : {RB_LIST_REFUSED_FREE, RB_LIST_REFUSED_ALLOC, RB_LIST_REFUSED_DENSITY, RB_LIST_REFUSED_SIDE_FULL}) {
        r.refused = refused;
        CHECK(refusal_stands(r, version, max_bytes) && refusal_stands(r, version, max_bytes * 2) && refusal_stands(r, version, 0));
        CHECK(!refusal_stands(r, version + 1, max_bytes));
    }
}

// list_policy's inequality as rb_engine.hip had it: per_kmer is L where a dense row table stands, else L x h; a slot costs at most 4 lines
static bool list_formula(uint64_t n_reads, uint64_t kmers, uint64_t per_kmer, uint64_t L_h, uint64_t n_rows)
{
    const uint64_t kMaxLines = 4;
    if (per_kmer <= kMaxLines) return false;
    if ((uint64_t)n_reads * 2 * kmers * (per_kmer - kMaxLines) < n_rows * (L_h + kMaxLines)) return false;
    return true;
}

// wide_table_admitted_locked's, as rb_engine.hip had it: a k-mer costs L x h lines, a slot at most 8
static bool wide_formula(uint64_t n_items, uint64_t kmers, uint64_t L_h, uint64_t n_rows)
{
    const uint64_t kWideMaxLines = 8;
    if (L_h <= kWideMaxLines) return false;
    return (uint64_t)n_items * 2 * kmers * (L_h - kWideMaxLines) >= n_rows * (L_h + kWideMaxLines);
}

static void repay_rule()
{
    const uint64_t n_rows = 1ull << (2 * 5);  // k = 5
    const uint64_t kmers_of[] = {0, 1, 7, 64, 296, 65535};
    // the wide kind: L x h = 9 and 93 (a filter of 8 193 bins at h = 3 and the GRCh38 filter), and what never repays
    for (uint64_t L_h : {1ull, 8ull, 9ull, 93ull, 96ull})
        for (uint64_t kmers : kmers_of) {
            // the first item count that repays, if any does, and one either side of it
            const uint64_t gain = L_h > 8 ? 2 * kmers * (L_h - 8) : 0, cost = n_rows * (L_h + 8);
            const uint64_t first = gain ? (cost + gain - 1) / gain : 1;
            for (uint64_t n : {(uint64_t)0, first - 1, first, first + 1, first * 3}) {
                CHECK(repays(n, kmers, L_h, 8, n_rows, L_h) == wide_formula(n, kmers, L_h, n_rows));
                if (!gain) CHECK(!repays(n, kmers, L_h, 8, n_rows, L_h));  // max_len < k, or a slot may cost what the k-mer costs now
            }
            if (gain) CHECK(repays(first, kmers, L_h, 8, n_rows, L_h) && !repays(first - 1, kmers, L_h, 8, n_rows, L_h));
        }
    // equality itself: 136 items x 2 x 64 k-mers x (9 - 8) == 1024 x (9 + 8)
    CHECK(136ull * 2 * 64 * 1 == n_rows * 17);
    CHECK(!repays(135, 64, 9, 8, n_rows, 9) && repays(136, 64, 9, 8, n_rows, 9) && repays(137, 64, 9, 8, n_rows, 9));
    // the list kind: L x h <= 4 never repays (the early exit), = 5 does; per_kmer = L where the dense row table stands, the build reads L x h
    for (uint64_t L : {1ull, 2ull})
        for (uint64_t h : {1ull, 2ull, 3ull, 4ull, 5ull})
            for (uint64_t per_kmer : {L, L * h})
                for (uint64_t kmers : kmers_of) {
                    const uint64_t gain = per_kmer > 4 ? 2 * kmers * (per_kmer - 4) : 0, cost = n_rows * (L * h + 4);
                    const uint64_t first = gain ? (cost + gain - 1) / gain : 1;
                    for (uint64_t n : {(uint64_t)0, first - 1, first, first + 1, first * 3}) {
                        CHECK(repays(n, kmers, per_kmer, 4, n_rows, L * h) == list_formula(n, kmers, per_kmer, L * h, n_rows));
                        if (per_kmer <= 4 || kmers == 0) CHECK(!repays(n, kmers, per_kmer, 4, n_rows, L * h));
                    }
                    if (gain) CHECK(repays(first, kmers, per_kmer, 4, n_rows, L * h) && !repays(first - 1, kmers, per_kmer, 4, n_rows, L * h));
                }
    // equality itself: 72 items x 2 x 64 k-mers x (5 - 4) == 1024 x (5 + 4)
    CHECK(72ull * 2 * 64 * 1 == n_rows * 9);
    CHECK(!repays(71, 64, 5, 4, n_rows, 5) && repays(72, 64, 5, 4, n_rows, 5) && repays(73, 64, 5, 4, n_rows, 5));
    CHECK(!repays(1ull << 32, 65535, 4, 4, n_rows, 4) && !repays(1ull << 32, 65535, 8, 8, n_rows, 8));  // the early exit, whatever the batch
    // the largest operands an engine passes: 2^32 - 1 items, 65 535 k-mers, L x h = 3 x 32, 4^13 rows -- against 128-bit arithmetic
    const uint64_t n_max = (1ull << 32) - 1, kmers_max = 65535, lh_max = 3 * 32, rows_max = 1ull << (2 * 13);
    for (uint64_t slot : {4ull, 8ull})
        for (uint64_t n : {(uint64_t)1, (uint64_t)65536, n_max})
            for (uint64_t rows : {n_rows, rows_max}) {
                const unsigned __int128 lhs = (unsigned __int128)n * 2 * kmers_max * (lh_max - slot), rhs = (unsigned __int128)rows * (lh_max + slot);
                CHECK(lhs >> 64 == 0 && rhs >> 64 == 0);  // the 64-bit products do not wrap
                CHECK(repays(n, kmers_max, lh_max, slot, rows, lh_max) == (lhs >= rhs));
            }
    CHECK(repays(n_max, kmers_max, lh_max, 8, rows_max, lh_max) && !repays(1, 1, lh_max, 8, rows_max, lh_max));
}

static void fresh_and_dropped()
{
    const ListTableState fresh;  // no table, no refusal, zero builds
    CHECK(!fresh.table && !fresh.side && fresh.version == 0 && fresh.rows == 0 && fresh.bytes == 0 && fresh.side_bytes == 0);
    CHECK(fresh.lines == 0 && fresh.side_rows == 0 && fresh.side_cap == 0 && fresh.census_rows == 0);
    CHECK(fresh.census_over[0] == 0 && fresh.census_over[1] == 0 && fresh.census_over[2] == 0 && fresh.build_ms == 0.0 && fresh.alloc_s == 0.0);
    CHECK(fresh.refused == RB_LIST_REFUSED_NONE && fresh.refused_version == 0 && fresh.refused_max_bytes == 0 && fresh.builds == 0);
    CHECK(!current(fresh, 0) && !refusal_stands(fresh, 0, 0));
    const TableCall c = table_call(current(fresh, 0), false, true, refusal_stands(fresh, 0, 0));
    CHECK(c.build && c.drop_stale && !c.take && !c.record_capture);  // the first call under BUILD builds

    uint32_t slots[1] = {0};
    uint64_t side[1] = {0};
    ListTableState s;
    s.table = slots;
    s.side = side;
    s.version = 3;
    s.rows = 1024;
    s.bytes = 1024 * 256;
    s.side_bytes = 66 * 1024;
    s.lines = 2;
    s.side_rows = 5;
    s.side_cap = 66;
    s.census_rows = 1024;
    s.census_over[0] = 9;
    s.census_over[1] = 1;
    s.census_over[2] = 0;
    s.build_ms = 1.5;
    s.alloc_s = 0.25;
    s.refused = RB_LIST_REFUSED_SIDE_FULL;
    s.refused_version = 2;
    s.refused_max_bytes = 77;
    s.builds = 4;
    CHECK(current(s, 3));
    clear_dropped(s);
    CHECK(!s.table && !s.side && s.rows == 0 && s.bytes == 0 && s.side_bytes == 0 && s.lines == 0 && s.side_rows == 0 && s.side_cap == 0);
    CHECK(!current(s, 3));
    // what outlives a drop
    CHECK(s.refused == RB_LIST_REFUSED_SIDE_FULL && s.refused_version == 2 && s.refused_max_bytes == 77 && s.builds == 4);
    CHECK(s.census_rows == 1024 && s.census_over[0] == 9 && s.census_over[1] == 1 && s.census_over[2] == 0 && s.build_ms == 1.5 && s.alloc_s == 0.25);
}

int main()
{
    decision_table();
    repay_rule();
    fresh_and_dropped();
    std::printf("failures: %d\n", failures);
    return failures ? 1 : 0;
}

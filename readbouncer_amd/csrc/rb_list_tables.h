// rb_list_tables.h -- the HOST side of a filter's list tables, once for all kinds: the LIST TABLE (rb_lists.h: up to 8192 bins, slots of
// 1, 2 or 4 lines), the WIDE LIST TABLE (rb_wide_lists.h: 8193 to 32 256 bins, slots of 4, 6 or 8 lines) and the PAIR TABLE
// (rb_pair_lists.h: up to 8192 bins, one three-line slot for a k-mer and its reverse complement, and tail lines).  They differ in their slot
// sizes, their geometry rule and the kernels that build and read them (ListTableKind, rb_engine.hip); what a filter remembers of a table,
// when a table or a refusal still holds, what a call does with the table and when a batch repays a build are the same for all, and are
// here.  No HIP in here and nothing that touches the device: tests/cpp/test_list_tables.cpp compiles it alone, plain and with sanitizers,
// and walks the whole decision -- the branch for a capturing stream among it, which no test on a GPU takes.
#pragma once
#include <cstdint>

#include "../../include/readbouncer_amd_tuning.h"

namespace rbtables {

// What a filter keeps of one list table (rb_dibf holds one per kind, both under row_mu).  `table` and `side` are device memory: the slots
// in the resident form and the dense rows of the slots that overflow.  They hold for the bits of `version` only.
struct ListTableState {
    uint32_t *table = nullptr;  // (dwords of the resident form; the list table's kernels take them as 16-bit halves)
    uint64_t *side = nullptr;
    uint32_t *tails = nullptr;  // (the pair table alone: its tail lines)
    uint64_t version = 0, rows = 0, bytes = 0, side_bytes = 0, tail_bytes = 0;
    uint32_t lines = 0, side_rows = 0, side_cap = 0, tail_rows = 0, tail_cap = 0;
    // what outlives a drop: the last census, the last build's times, the tables built so far and why the last build did not happen
    uint64_t census_rows = 0, census_over[3] = {0, 0, 0};
    uint64_t census_extra = 0, census_version = 0;  // (the pair table's census: sampled rows of more than 64 bins, and the bits it looked at)
    double build_ms = 0.0, alloc_s = 0.0;
    uint32_t refused = RB_LIST_REFUSED_NONE;  // RB_LIST_REFUSED_*
    uint64_t refused_version = 0;             // ... the bits it was refused for: an engine does not ask again until they change
    uint64_t refused_max_bytes = 0;           // ... and the max_bytes of that build (refusal_stands)
    uint32_t builds = 0;
};

// the fields of a table that is gone, after its memory was freed: the refusal, the census, the times and `builds` stay
inline void clear_dropped(ListTableState &s)
{
    s.table = nullptr;
    s.side = nullptr;
    s.tails = nullptr;
    s.rows = s.bytes = s.side_bytes = s.tail_bytes = 0;
    s.lines = s.side_rows = s.side_cap = s.tail_rows = s.tail_cap = 0;
}

// a table of the bits as they are (`version`: the filter's)
inline bool current(const ListTableState &s, uint64_t version) { return s.table && s.version == version; }

// Does the last refusal still stand for a call that allows the table `max_bytes`?  Every refusal but the one of a capturing stream is
// remembered for the version of the bits it was given for, so that neither a call nor rb_engine_plan takes the census again only to be
// refused again: density and a full side table are properties of the bits; a table beyond max_bytes stays beyond it until the caller
// allows more; want of memory stands until the bits change or the table's _build / _drop is called (what the row table does).
inline bool refusal_stands(const ListTableState &s, uint64_t version, uint64_t max_bytes)
{
    if (s.refused == RB_LIST_REFUSED_NONE || s.refused == RB_LIST_REFUSED_CAPTURE) return false;
    if (s.refused_version != version) return false;
    return s.refused != RB_LIST_REFUSED_MAX_BYTES || max_bytes == s.refused_max_bytes;
}

// What a call does with a filter's table, in this order: note the refusal of a capturing stream, free a stale table, take the current one,
// or build one and take it if the build produced a table.
struct TableCall {
    bool record_capture, drop_stale, take, build;
};

// The one rule, for both kinds and for every path that reads a table (classify, locate, hits, prefix, resume).  A call whose stream is
// being captured takes nothing, table or no table, and changes nothing but the refusal: the graph would keep the table's address, and the
// next change of the bits frees it.  Any other call takes the current table; without one it frees what the bits have moved away from
// (whether or not it may build: dibf_changed drops both tables with every change of the bits, so a stale table is never seen to stay)
// and builds where the caller's setting allows it and this version of the bits was not refused a table already.
inline TableCall table_call(bool current, bool capturing, bool may_build, bool refusal_stands)
{
    TableCall c{};
    if (capturing) {
        c.record_capture = !current;
        return c;
    }
    c.take = current;
    c.drop_stale = !current;
    c.build = !current && may_build && !refusal_stands;
    return c;
}

// Does a batch alone repay the build of a table, in 128-byte lines?  A k-mer costs lines_per_kmer_now lines today and at most
// max_slot_lines from a slot, on both strands of n_items items of kmers_per_strand k-mers; the build reads build_read_lines lines per row
// and writes at most max_slot_lines.  Never where a slot may cost as much as the k-mer does now.  (The largest operands an engine passes,
// 2^32 items x 2 x 65 535 k-mers x 96 lines and 4^13 rows x 104 lines, stay below 2^57.)
inline bool repays(uint64_t n_items, uint64_t kmers_per_strand, uint64_t lines_per_kmer_now, uint64_t max_slot_lines, uint64_t n_rows,
                   uint64_t build_read_lines)
{
    if (lines_per_kmer_now <= max_slot_lines) return false;
    return n_items * 2 * kmers_per_strand * (lines_per_kmer_now - max_slot_lines) >= n_rows * (build_read_lines + max_slot_lines);
}

}  // namespace rbtables

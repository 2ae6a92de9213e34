// rb_device.h -- kernel argument structs and launcher declarations (HIP translation units only)
#pragma once
#include <hip/hip_runtime.h>

#include "rb_internal.h"

namespace rb {

constexpr unsigned kMaxFilters = 16;
// Tables beyond this size are read with non-temporal loads: 2x the 256 MiB Infinity Cache, beyond which caching cannot help.  The
// default of an engine's nt_threshold_bytes (rb_engine_set_nt_threshold) and the rule of the passes that have no engine.
constexpr uint64_t kNtThresholdBytes = 512ull << 20;

// by-value kernel argument describing one HBM-resident IBF
struct IbfDev {
    const uint64_t *words;  // block-major bit matrix, reference layout
    uint64_t magic;         // floor(2^64 / n_blocks) for the Barrett reduction
    uint64_t precalc[rbspec::kMaxHash];
    uint32_t n_blocks;
    uint32_t pow2_mask;  // n_blocks - 1 when n_blocks is a power of two, else 0xFFFFFFFF
    uint32_t n_bins;
    uint32_t bin_width;
    uint32_t stride;  // words from one block to the next in HBM (>= bin_width; padded layout)
    uint32_t k;
    uint32_t n_hash;
    uint32_t comp_n;  // ordinal the reverse strand holds for an N of the read (rbspec::kRevCompOfN unless the engine was told otherwise)
};

// where the bases of a batch live (by-value kernel argument)
struct ReadSrc {
    const uint8_t *seqs;            // ASCII bytes, or the 2-bit payload when nmask != nullptr
    const uint64_t *offsets;        // per READ: byte offset of its bases / of its packed payload
    const uint32_t *lens;           // per ITEM: effective length (whole read, or the chunk after chunk_prep)
    const uint8_t *nmask;           // packed input only: N bitmap payload
    const uint64_t *nmask_offsets;  // per READ: byte offset of its N bitmap
    const uint32_t *ids;            // optional item -> read indirection (nullptr = identity)
    uint32_t base_off;              // bases skipped at the start of every read (chunk start)
    uint32_t max_len;               // declared upper bound of the item lengths: K1 never looks at more bases of an item than this (a longer
                                    // item is answered with RB_ERR_INVALID_ARG by the decision kernel; 0 = no bound given)
};

// Clock-phased gathers for tables of a few L2 sizes (narrow filters; rb_kernels.hip, "phased form"): the table is cut into
// n_slices runs of 2^shift blocks, and window number (wall clock * inv_ticks) >> 32 tells the whole chip which slice to
// gather from.  n_slices == 0: off.
struct PhaseCfg {
    uint32_t shift;      // log2 blocks per slice; with bit 31 set the low bits are blocks per slice, any number (stride-4 one-lane builds)
    uint32_t n_slices;   // ceil(n_blocks / 2^shift), <= 32 (the engine plans <= 8)
    uint32_t inv_ticks;  // floor(2^32 / window length in 10 ns ticks)
    uint32_t skew;       // added to the window number: 0, or this wave's XCD number when xcd_skew is set (experiment)
    uint32_t xcd_skew;   // 1: every XCD works on a different slice at any time (slice = (window + XCD) mod n_slices)
    uint32_t tskew;      // wall-clock ticks by which each XCD's windows start later than the previous XCD's (the kernel multiplies by its XCD
                         // number): the XCDs then refill their L2s one after the other, not all in the same instant.  0: one clock for the chip
};

constexpr unsigned kMaxFused = 8;
constexpr int kSplitAnyWaves = 8;  // waves per workgroup of the mixed-geometry latency kernel (built for 512 threads)

// by-value kernel argument: up to 8 filters served by one launch (blockIdx.y picks one).  The throughput kernel takes
// filters of one kernel geometry; the latency kernel takes any mix and reads the geometry per filter.
struct FilterSet {
    uint32_t n;
    uint32_t col_begin[kMaxFused], col_end[kMaxFused];
    uint32_t out_offset[kMaxFused];  // element offset of the filter's column in the output
    uint32_t geom[kMaxFused];        // latency kernel: lg | (wpl == 2 ? 8 : 0) | (nt ? 16 : 0)
    uint32_t parts[kMaxFused];       // latency kernel: workgroups per (read, slice) that work for this filter (<= grid parts)
    uint32_t sub[kMaxFused];         // latency kernel: shares per macro tile
    IbfDev f[kMaxFused];
};

// Filters of one hash geometry merged into ONE table (rb_engine.hip, MergedGroup): which BITS of a merged block belong to which
// filter.  Member g owns the bins [bit_begin[g], bit_end[g]) of every block -- word-aligned when every member keeps whole word
// columns, packed bit to bit when that saves a word column (README shape: 122 + 43 + 29 + 49 bins = 243 bits = four words instead
// of five, which takes the table to the one-lane-per-block builds of the phased kernel).  By-value kernel argument of
// ibf_count_max_merged_kernel.
constexpr unsigned kMaxMerged = 16;
struct MergeMap {
    uint32_t n;                       // filters in the merged table
    uint32_t bit_begin[kMaxMerged];   // first bin of filter g in a merged block
    uint32_t bit_end[kMaxMerged];     // one past its last bin
    uint32_t out_offset[kMaxMerged];  // element offset of filter g's column in a row of the output
    uint32_t width;                   // word columns of a merged block
};

// bins of member [begin, end) that lie in word column c of a merged block, as a mask of that word
__host__ __device__ inline uint64_t member_mask(uint32_t begin, uint32_t end, uint32_t c)
{
    const uint32_t lo = c * 64u, hi = lo + 64u;
    const uint32_t b = begin > lo ? begin : lo, e = end < hi ? end : hi;
    if (b >= e) return 0ULL;
    const uint64_t upto_e = (e - lo) >= 64u ? ~0ULL : ((1ULL << (e - lo)) - 1);
    const uint64_t upto_b = (1ULL << (b - lo)) - 1;  // b - lo < 64
    return upto_e & ~upto_b;
}

// Merged tables of at most four word columns (two to eight narrow filters of one hash geometry, rb_engine.hip) are served by the
// both-strands builds of the phased kernel, which hold a whole block in one lane: which bins belong to which member (bit ranges as
// in MergeMap), how many of a column's 64 bits are bins at all (0: the column does not exist), and where each member's maximum
// goes in a row of the output.  A filter on its own is the case n = 1.
constexpr unsigned kMaxNarrow = 8;
struct NarrowMerge {
    uint32_t n;                       // members (1..8)
    uint32_t bit_begin[kMaxNarrow];   // member -> first bin in a block
    uint32_t bit_end[kMaxNarrow];     // member -> one past its last bin
    uint32_t col_bits[4];             // word column -> bins in it (64: all; 0: no such column)
    uint32_t out_offset[kMaxNarrow];  // member -> element offset in a row of the output
};

// Packed block numbers of the LDS-offset builds (ibf_count_max_phased_multi_kernel, rb_kernels.hip): three per k-mer in one 64-bit
// word, kPackBits each for blocks of two to four words, kPackBits1 for one-word blocks (the third number's top two bits in a spill
// register).  The all-ones number means "no lookup", so a table may hold at most 2^PB - 2 blocks: the ONE limit the planner, the
// launchers and the merged copy's complemented twin (rb_engine.hip) all test against.
constexpr uint32_t kPackBits = 21;
constexpr uint32_t kPackMask = (1u << kPackBits) - 1u;
constexpr uint32_t kPackBits1 = 22;
constexpr uint32_t kPackMask1 = (1u << kPackBits1) - 1u;
constexpr uint64_t pack_max_blocks(uint32_t pack_bits) { return (1ull << pack_bits) - 2u; }
constexpr uint64_t kPackMaxBlocks = pack_max_blocks(kPackBits);    // 2 097 150: 32 MiB of two-word blocks
constexpr uint64_t kPackMaxBlocks1 = pack_max_blocks(kPackBits1);  // 4 194 302: 32 MiB of one-word blocks

struct CountLaunch {
    IbfDev f;
    ReadSrc src;
    uint32_t n_reads;               // number of work items
    uint32_t col_begin, col_end;  // word columns of every block this launch covers
    uint32_t n_slices;            // column slices of 2^lg * wpl words
    int lg, wpl, planes;
    int nt;                       // non-temporal table gathers (tables beyond the Infinity Cache)
    PhaseCfg phase;               // throughput form on narrow filters: clock-phased gathers (n_slices == 0: off)
    NarrowMerge narrow;           // phased form on two- to four-word blocks: columns -> members (the engine fills it; n = 1: one filter)
    int phase_shape;              // engine bookkeeping (rbplan::PhaseShape of the planner's row for this launch; the kernels do not read it)
    uint32_t phase_slice_log2, phase_ticks;  // ... the slice size and window length in effect (10 ns ticks), for rb_engine_plan
    uint32_t phase_rule_ticks;               // ... and what the planner's table alone would give (rb_engine_calibrate may have replaced it)
    uint64_t phase_slice_bytes;              // ... and the slice length in effect (2^phase_slice_log2, or the equal-length slices of the four-word builds)
    int short_only;               // 1 / 3 / 2: the declared max_len gives at most 256 / 384 / 512 k-mers per read; 0: more
    int multi_reads;              // phased form, two-word blocks, short_only 1: reads per wave of ibf_count_max_phased_multi_kernel (0: the one-read build)
    int multi_tiles;              // ... tiles per strand of that build: 4 (reads of up to 256 k-mers) or 6 (up to 384)
    int multi_inv;                // ... and f.words is the COMPLEMENTED twin of a merged copy (the build that ORs instead of masking and ANDing)
    int split_waves;              // >= 2: latency form, workgroups of split_waves waves
    int split_parts, split_sub;   // latency form: workgroups per (read, slice) and shares per macro tile (0/1 = one workgroup)
    int grid_parts;               // latency form: workgroups launched per (read, slice) = max parts of the fused filters
    uint64_t *split_ws;           // parts > 1: partial counters [filter][item][grid part][strand][2][planes][64]
    uint32_t *split_tickets;      // parts > 1: arrival counters [filter][item], zero between launches
    uint16_t *out;
    uint32_t out_read_stride, out_slice_stride;
    // latency form only: n_fused > 0 = several filters in one launch (then f/col_begin/col_end above describe the first)
    int n_fused;
    IbfDev fused_f[kMaxFused];
    uint32_t fused_col_begin[kMaxFused], fused_col_end[kMaxFused], fused_out_offset[kMaxFused];
    uint8_t fused_geom[kMaxFused], fused_parts[kMaxFused], fused_sub[kMaxFused];  // latency form, see FilterSet
    const struct FoldJob *fold;   // latency form: the launch also makes the decisions (nullptr: it only counts)
    // opt-in early decision (plain throughput form, RB_MODE_CHECK_UNBLOCK without raw maxima): the decision kernel's threshold table, so that
    // a wave can stop counting once a bin has reached the larger of the read's two thresholds for this filter (nullptr: count everything)
    const uint16_t *early_thr;
    uint32_t early_thr_len, early_nf, early_fi;
    // plain throughput form: skip the gathers of bins that can no longer reach the read's maximum (rb_kernels.hip, count_strand; 0: off)
    int bound_prune;
    int prune_parts;          // ... and its refinements, bits as in rb_engine_set_prune_parts (ignored while bound_prune is 0)
    uint64_t *prune_trace;    // ... one record per (read, slice) of this launch (prune_trace_record), or nullptr
    float cert_d, cert_c;     // ... the certificate's allowance over rem k-mers: cert_d * rem + cert_c * sqrt(rem) (see PruneCfg)
    uint32_t lead_min;        // ... the probe maximum from which the leader's line is counted first (kPruneLeadMinShift)
    // row form (launch_ibf_count_rows): the filter's row table -- one row of `f.stride` words per N-free k-mer -- or nullptr
    const uint64_t *row_table;
    // list form (launch_ibf_count_lists, rb_lists.hip): the filter's list table -- one slot of list_lines lines per N-free k-mer (rb_lists.h) --
    // and its side table of list_side_rows dense rows for the slots that overflowed, or nullptr
    const uint16_t *list_table;
    const uint64_t *list_side;
    uint32_t list_side_rows, list_lines;
};

// By-value argument of ibf_count_max_kernel: how it prunes.
constexpr uint32_t kPruneBound = 1u;    // bound pruning on
constexpr uint32_t kPruneSubTile = 2u;  // ... checked after every eight k-mers, not only at tile boundaries
constexpr uint32_t kPruneLead = 4u;     // ... both strands probed, the stronger finished first
constexpr uint32_t kPruneCert = 8u;     // ... the trailing strand certified from hash 0 alone where that is promising
constexpr uint32_t kPruneLeadLine = 16u;  // ... the 128-byte line of the leader's best probe bin counted first, its other lanes certified likewise
constexpr uint32_t kPruneLeadMinShift = 8;  // bits 8-15 of the flags: the lead line is attempted when the leader's probe maximum is at least this
                                            // (reads without a match stay below it; a probe counts at most 64, so 65 and more mean never)
struct PruneCfg {
    uint32_t flags;
    float cert_d, cert_c;  // the load d of the filter's fullest bin and z * sqrt(d (1 - d)): a certificate is attempted when the leader's maximum is at
                           // least the trailing probe's maximum + cert_d * rem + cert_c * sqrt(rem), rem = k-mers behind the probe
    uint64_t *trace;
};
// The 8-byte record a wave leaves per (read, slice) when a trace is asked for (rb_engine_set_prune_trace): bit 0 = the strand that was
// finished first (0 forward, 1 reverse), bit 1 = the strands were probed (the lead was chosen, not given), bit 2 = a certificate was
// attempted for the trailing strand, bit 3 = it held, bit 4 = the leader's line was counted first, bit 5 = a certificate was attempted for
// the leader's other lanes, bit 6 = it held, bit 15 = record written,
// bits 16-31 / 32-47 = the k-mer position at which the gathers of the forward / reverse strand ended (n: counted to the end; less:
// the whole wave was dead there, or the strand was not continued behind its probe, or -- 0 -- not counted at all; a leader whose line
// was counted first reports its last all-hash call: the line's where the other lanes' certificate held, the other lanes' otherwise).
__host__ __device__ inline uint64_t prune_trace_record(uint32_t lead, bool probed, uint32_t cert_bits, uint32_t stop_fwd, uint32_t stop_rev,
                                                         uint32_t line_bits = 0)
{
    return (uint64_t)(lead & 1u) | (probed ? 2ull : 0ull) | ((uint64_t)(cert_bits & 3u) << 2) | ((uint64_t)(line_bits & 7u) << 4) | (1ull << 15) | ((uint64_t)(stop_fwd & 0xFFFFu) << 16) | ((uint64_t)(stop_rev & 0xFFFFu) << 32);
}

inline uint8_t geom_code(int lg, int wpl, int nt) { return (uint8_t)(lg | (wpl == 2 ? 8 : 0) | (nt ? 16 : 0)); }

struct DecideParams {
    uint32_t nd, nt;
    uint32_t k[kMaxFilters];
    const uint16_t *thr;  // [thr_len][nf][2]: thresholds at r and at r-0.02 by read length
    uint32_t thr_len;
    uint32_t max_len;  // declared upper bound of the read lengths of this batch
    uint16_t *maxcount_copy;  // optional second destination of the maxcount rows (pinned host memory of the micro-batch path)
    // bin-sharded operation: maxcount holds n_parts partial tables (one per rank, all-gathered), part_stride elements apart;
    // the raw maximum of a (read, filter) is the max over them.  1 = a plain table.
    uint32_t n_parts;
    uint64_t part_stride;
    // Completion word of the host micro-batch path (nullptr: none): when every result of the call is written, done_seq is stored -- behind a
    // system-scope release -- into this word of page-locked host memory, and the host, which spins on it, does not wait for the stream
    // (hipStreamSynchronize returns 4 us later than the word arrives: profiles/r05/graph_launch_probe.txt).  Decision kernels of more than one
    // workgroup count their arrivals in done_count (zero between calls).
    uint32_t *done_flag;
    uint32_t done_seq;
    uint32_t *done_count;
};

// The decision of a micro-batch made by the latency kernel itself, for engines with ONE filter: the workgroup that writes a read's raw
// maximum runs the decision for that read, and the dependent launch of the decision kernel goes away (1.1-1.8 us of a 40-120 us call
// up to 256 reads; with several filters the reads would need arrival counters of their own, and one more agent-scope release per
// (read, filter) costs more than the launch did: profiles/r05/negative_results.md, entry 10).  By-value kernel argument.
struct FoldJob {
    uint32_t on;  // 0: the kernel only counts
    int mode;
    const uint16_t *maxcount;  // the table [n_reads][1] the launch writes into
    const uint32_t *lens;
    const uint8_t *pre_status;
    int32_t *best_target;
    uint8_t *decision;
    uint8_t *status;
    DecideParams P;
};

// locate pass (rb_locate_batch_device; rb_kernels.hip, ibf_locate_kernel): what one column slice of a filter knows about a work item ...
struct LocatePart {
    uint32_t max_count;
    uint32_t first_bin;  // lowest bin at max_count in this slice (undefined when max_count == 0)
    uint32_t strand;
    uint32_t hit_bins;   // bins of this slice with fwd >= t or rev >= t
};
// ... the caller's output arrays (any may be nullptr) ...
struct LocateOut {
    uint16_t *max_count;
    int32_t *best_bin;
    uint8_t *best_strand;
    uint32_t *hit_bins;
    uint8_t *status;
};
// ... and one filter's launch.  What locate and hits share: the plain form over the filter's own table, counted in full -- and, where the
// engine chose it (rb_engine_set_pass_lists), the list form in front of it
struct PlainPassLaunch {
    IbfDev f;
    ReadSrc src;
    uint32_t n_items;
    uint32_t col_begin, col_end;
    uint32_t n_slices;
    int lg, wpl, planes, nt;
    const uint16_t *thr;  // the decision kernel's table [thr_len][nf][2]
    uint32_t thr_len, nf, fi;
    // list form of locate and hits (rb_pass_lists.hip): the filter's list table and its side table as in CountLaunch, or nullptr: the
    // plain form alone.  list_nt: non-temporal slot gathers (the list table's bytes against the engine's threshold, as the count path).
    // list_taken / list_plain_lens: what launch_pass_lists_prep made of the call's items
    const uint16_t *list_table;
    const uint64_t *list_side;
    uint32_t list_side_rows, list_lines;
    int list_nt;
    const uint8_t *list_taken;
    const uint32_t *list_plain_lens;
    // wide list form of locate and hits (rb_wide_pass_lists.hip): the filter's wide list table and its side table as in WideCountLaunch,
    // or nullptr.  A filter has one table or the other (their bin counts do not meet); list_taken / list_plain_lens are then what
    // launch_wide_pass_lists_prep made of the call's items
    const uint32_t *wide_table;
    const uint64_t *wide_side;
    uint32_t wide_side_rows, wide_lines;
    int wide_nt;
};
struct LocateLaunch : PlainPassLaunch {
    LocatePart *part;     // [n_slices][n_items]
};
// Which work items the list kernels of locate and hits take (rb_pass_lists.hip, pass_lists_takes: the item is RB_OK and its chunk window
// holds no base outside ACGT), decided ONCE per call for both sides: taken[item] = 1 for the list kernels' items, and plain_lens[item] is
// the item's length, or 0 for a taken item -- the lengths the plain kernels are launched with, unchanged themselves, so that they count
// nothing of what the list kernels count.
struct PassListsPrep {
    ReadSrc src;
    uint32_t n_items;
    const uint8_t *pre_status;  // chunk_prep's per-item status, or nullptr
    uint32_t min_len;           // item_status's: the largest k of the engine
    uint8_t *taken;
    uint32_t *plain_lens;
};
hipError_t launch_pass_lists_prep(const PassListsPrep &a, hipStream_t st);
// Which build a plain-form launch takes, as host arithmetic: the launchers of rb_kernels.hip instantiate by these two, and
// rb_engine_plan_pass reports them.  Ten counter planes only with the compile-time three hash functions (*h = 3); *h = 0 is the
// run-time hash count, always on sixteen planes.  The query passes have a non-temporal twin for blocks of a whole wave only.
inline void plain_planes_hash(uint32_t n_hash, int planes, int *np, int *h)
{
    *h = n_hash == 3 ? 3 : 0;
    *np = (*h == 3 && planes <= 10) ? 10 : 16;
}
inline bool plain_pass_nt(int lg, int nt) { return lg == 6 && nt != 0; }
hipError_t launch_ibf_locate(const LocateLaunch &a, hipStream_t st);
// ... the list form (rb_pass_lists.hip): launch_ibf_locate over a.list_plain_lens -- the items the list kernel leaves, from the filter's
// own table; a taken item has no k-mer there and gets an empty record -- and then ibf_locate_lists_kernel, whose records of the taken
// items stand
bool pass_list_form_serves(const PlainPassLaunch &a);  // list_form_serves for a launch of locate or hits
hipError_t launch_ibf_locate_lists(const LocateLaunch &a, hipStream_t st);
// ... the wide list form (rb_wide_pass_lists.hip).  Which items it takes, once per call: taken[item] = 1 when the item is RB_OK (the
// status rules alone: the wide kernels count a k-mer with a base outside ACGT themselves), plain_lens[] as launch_pass_lists_prep's.
// launch_ibf_locate_wide_lists is launch_ibf_locate over a.list_plain_lens and then ibf_locate_wide_lists_kernel, which writes a taken
// item's record into slice 0 and an empty record into every other slice of the a.n_slices the merge reads
hipError_t launch_wide_pass_lists_prep(const PassListsPrep &a, hipStream_t st);
hipError_t launch_ibf_locate_wide_lists(const LocateLaunch &a, hipStream_t st);
hipError_t launch_reduce_locate_slices(const LocatePart *part, uint32_t n_slices, uint32_t n_items, const uint32_t *lens,
                                       const uint8_t *pre_status, uint32_t max_len, uint32_t min_len, const LocateOut &out, uint32_t nf,
                                       uint32_t fidx, hipStream_t st);

// prefix pass (rb_prefix_batch_device; rb_kernels.hip, ibf_prefix_kernel): the checkpoints, strictly rising and none 0, as a by-value
// kernel argument ...
constexpr uint32_t kMaxPrefixes = 64;  // == RB_PREFIX_MAX: checkpoint p's maximum lives in lane p
struct PrefixList {
    uint32_t n;
    uint32_t c[kMaxPrefixes];
};
// ... and one filter's launch
struct PrefixLaunch : PlainPassLaunch {
    PrefixList cps;
    uint16_t *part;  // [n_slices][n_items][cps.n]
};
hipError_t launch_ibf_prefix(const PrefixLaunch &a, hipStream_t st);
// ... the list form (rb_prefix_lists.hip; rb_engine_set_prefix_lists).  Which items it takes, once per call: with w = min(lens[item], c_last),
// taken[item] = 1 when the item's pre-status is RB_OK, w <= src.max_len and the first w bases of its chunk window are all ACGT -- any
// length, below k and empty included; plain_lens[item] is the item's length, or 0 for a taken item.  counters[0] += the items taken,
// counters[1] += the items left.  launch_ibf_prefix_lists is launch_ibf_prefix over a.list_plain_lens and then
// ibf_prefix_lists_kernel<LINES, NT>, which overwrites the taken items' partials of slice 0 (of one).
struct PrefixListsPrep {
    ReadSrc src;
    uint32_t n_items;
    const uint8_t *pre_status;  // chunk_prep's per-item status, or nullptr
    uint32_t c_last;            // the last checkpoint
    uint8_t *taken;
    uint32_t *plain_lens;
    uint64_t *counters;         // two, the engine's
};
hipError_t launch_prefix_lists_prep(const PrefixListsPrep &a, hipStream_t st);
hipError_t launch_ibf_prefix_lists(const PrefixLaunch &a, hipStream_t st);
// ... the wide list form (rb_wide_prefix_lists.hip; rb_engine_set_wide_prefix_lists).  Which items it takes: the list form's rule without the
// look at the bases -- the pre-status is RB_OK and w <= src.max_len -- with taken[], plain_lens[] and counters[] (two of this form's own)
// as above.  launch_ibf_prefix_wide_lists is launch_ibf_prefix over a.list_plain_lens and then ibf_prefix_wide_lists_kernel<LINES, NT>,
// which writes a taken item's partials into slice 0 and zeros into every other slice of the a.n_slices the merge reads.
hipError_t launch_wide_prefix_lists_prep(const PrefixListsPrep &a, hipStream_t st);
hipError_t launch_ibf_prefix_wide_lists(const PrefixLaunch &a, hipStream_t st);
// max_count [n_items][cps.n][nf] <- the maximum over the slices; for fidx == 0 also prefix_len / row_pre [n_items][cps.n]
hipError_t launch_finish_prefix(const PrefixLaunch &a, const uint32_t *lens, const uint8_t *pre_status, uint16_t *max_count, uint32_t *prefix_len,
                                uint8_t *row_pre, hipStream_t st);
hipError_t launch_first_decided(const uint8_t *decision, const uint8_t *status, uint32_t n_items, uint32_t n_prefixes, uint32_t *first_decided,
                                hipStream_t st);

// resume pass (rb_resume_batch_device; rb_kernels.hip, ibf_resume_kernel): a slot's bookkeeping beside its counter planes ...
constexpr uint32_t kResumePlanes = 16;   // counters wrap at 2^16 as the reference's uint16_t counts do
constexpr uint32_t kResumeMaxTail = 31;  // k - 1 at the largest k
struct ResumeMeta {
    uint32_t total;                // bases committed to the slot since its last FIRST
    uint32_t tail_len;             // min(total, k - 1)
    uint8_t tail[kResumeMaxTail + 1];  // the last tail_len bases as Dna5 ordinals
};
// ... what the prep kernel makes of an item for the pass (bits 0 and 1 are the caller's RB_RESUME_FIRST / RB_RESUME_PEEK) ...
constexpr uint32_t kResumeFirst = 1u;  // start from zero, load nothing
constexpr uint32_t kResumePeek = 2u;   // store nothing
constexpr uint32_t kResumeSkip = 4u;   // refused: the slot is neither read nor written (its number may not even exist)
// ... the slots as the pass kernel sees them (by-value kernel argument; the planes of slot s and this filter are
// state[s * slot_words + filter_off + (strand * 16 + plane) * pad_cols + column]) ...
struct ResumeSlots {
    uint64_t *state;
    const uint32_t *slot;  // per item; vetted by the prep kernel wherever ctl has no kResumeSkip
    const uint8_t *ctl;    // per item: kResume* bits
    uint64_t slot_words;   // words of one slot, all filters
    uint64_t filter_off;   // words before this filter's planes inside a slot
    uint32_t pad_cols;     // n_slices * 2^lg * wpl >= bin_width
};
// ... one filter's launch (src: the stitched items "tail + chunk" in the workspace) ...
struct ResumeLaunch : PlainPassLaunch {
    ResumeSlots slots;
    uint16_t *part;  // [n_slices][n_items]
    const uint8_t *list_plain_ctl;  // list form: slots.ctl with kResumeSkip set for the items of list_taken (launch_resume_lists_prep)
};
hipError_t launch_ibf_resume(const ResumeLaunch &a, hipStream_t st);
// ... the list form (rb_resume_lists.hip; rb_resume_set_lists).  Which items it takes, once per call after the prep kernel below: taken[item]
// = 1 when the item is not refused and its stitched string holds no base outside ACGT (any length), and plain_ctl[item] = ctl[item], with
// kResumeSkip for a taken item.  launch_ibf_resume_lists is launch_ibf_resume over list_plain_ctl -- a taken item gets a zero partial there
// and no address of its slot is formed -- and then ibf_resume_lists_kernel<LINES, NT>, which counts a taken item's new k-mers from the
// list table into LDS and merges them into the slot's planes (rb_resume_planes.h), overwriting the item's partial of slice 0.
hipError_t launch_resume_lists_prep(const ReadSrc &src, uint32_t n_items, const uint8_t *pre_status, const uint8_t *ctl, uint8_t *taken,
                                    uint8_t *plain_ctl, hipStream_t st);
hipError_t launch_ibf_resume_lists(const ResumeLaunch &a, hipStream_t st);
// ... and the small kernels around the pass.  Prep: vets item i (slot number, chunk length, total), writes its stitched string as ASCII at
// stitched + i * stitch_stride, its length, the bytes offset, the total the row stands for, its pre-status and its ctl bits.
struct ResumePrep {
    ReadSrc src;               // the caller's reads (src.lens: FULL read lengths; src.base_off: chunk_start)
    uint32_t chunk_length;     // rb_batch_desc's (0: to the end of the read)
    const uint32_t *slot;
    const uint8_t *flags;      // or nullptr
    const ResumeMeta *meta;
    uint32_t n_items, n_slots, max_chunk_len, max_total_len, k;
    uint8_t *stitched;
    uint32_t stitch_stride;
    uint64_t *st_offsets;
    uint32_t *st_lens, *total_lens;
    uint8_t *pre_status, *ctl;
    uint32_t *out_total_len;   // the caller's, or nullptr
};
hipError_t launch_resume_prep(const ResumePrep &a, hipStream_t st);
hipError_t launch_resume_commit(ResumeMeta *meta, const uint32_t *slot, const uint8_t *ctl, const uint8_t *stitched, uint32_t stitch_stride,
                                const uint32_t *st_lens, const uint32_t *total_lens, uint32_t n_items, uint32_t k, hipStream_t st);
// counts [2][n_bins] u16 <- the planes of one slot and filter (planes: state + slot * slot_words + filter_off)
hipError_t launch_resume_counts(const uint64_t *planes, uint32_t pad_cols, uint32_t n_bins, uint16_t *counts, hipStream_t st);

// hits pass (rb_hits_batch_device; rb_kernels.hip, ibf_hits_kernel): a record as the kernels move it -- x = bin, y = count | strand << 16,
// the eight bytes of rb_hit ...
typedef unsigned int rb_u32x2 __attribute__((ext_vector_type(2)));
// ... the caller's output arrays (any may be nullptr) ...
struct HitsOut {
    rb_u32x2 *hits;    // [n_items][nf][max_hits]
    uint32_t *n_hits;  // [n_items][nf]
    uint8_t *status;   // [n_items]
};
// ... and one filter's launch
struct HitsLaunch : PlainPassLaunch {
    uint32_t min_count;   // 0: the table's entry; else the threshold itself
    uint32_t max_hits;    // records kept per (item, slice, strand) segment and per (item, filter) list
    uint32_t min_len;     // an item shorter than this is RB_ERR_SHORT_READ
    const uint8_t *pre_status;  // chunk_prep's per-item status, or nullptr
    void *seg;            // rb_u32x2 [n_items][n_slices][2][max_hits]
    uint32_t *seg_count;  // [n_slices][2][n_items]: hits of the (slice, strand) run, whatever the cap
    uint64_t *bin_reads;  // this filter's n_bins counters, or nullptr
};
hipError_t launch_ibf_hits(const HitsLaunch &a, hipStream_t st);
// ... the list form (rb_pass_lists.hip): launch_ibf_hits over a.list_plain_lens, where a taken item is too short to be looked at, and
// ibf_hits_lists_kernel for the taken items: every segment is written once
hipError_t launch_ibf_hits_lists(const HitsLaunch &a, hipStream_t st);
// ... the wide list form (rb_wide_pass_lists.hip): as above, and ibf_hits_wide_lists_kernel writes a taken item's segments and counters of
// slice 0 and a zero counter for every other slice -- the plain kernel writes nothing for an item it leaves
hipError_t launch_ibf_hits_wide_lists(const HitsLaunch &a, hipStream_t st);
hipError_t launch_finish_hits(const HitsLaunch &a, const uint32_t *lens, const HitsOut &out, hipStream_t st);

// spans pass (rb_spans_batch_device; rb_kernels.hip, ibf_spans_kernel): the caller's output arrays (any may be nullptr) ...
struct SpansOut {
    uint32_t *spans;    // rb_span [n_queries][2] as 32-bit words: count, first, last, run_start, run_len, covered
    uint64_t *mask;     // [n_queries][2][mask_words]
    uint32_t *n_kmers;  // [n_queries]
    uint8_t *status;    // [n_queries]
};
// ... and the launch: one wave per query (x = work item, y = bin) against ONE filter's own table
struct SpansLaunch {
    IbfDev f;
    ReadSrc src;
    uint32_t n_items;
    const rb_u32x2 *queries;
    uint32_t n_queries;
    uint32_t mask_words;
    uint32_t min_len;           // an item shorter than this is RB_ERR_SHORT_READ (item_status: the largest k of the engine)
    const uint8_t *pre_status;  // chunk_prep's per-item status, or nullptr
    int nt;
    SpansOut out;
};
hipError_t launch_ibf_spans(const SpansLaunch &a, hipStream_t st);

hipError_t launch_ibf_count_max(const CountLaunch &a, hipStream_t st);
// Row form of the plain whole-wave builds (rb_kernels.hip, ibf_count_rows_kernel): one gather per k-mer from a.row_table.  A filter has
// a row table only for k <= kRowTableMaxK (4^13 rows: the block number of a row is a 32-bit rank and 4^k * stride must fit the device).
constexpr uint32_t kRowTableMaxK = 13;
bool row_form_serves(const CountLaunch &a);  // the launch is one the row form has a build for (geometry, form, hash count, k)
hipError_t launch_ibf_count_rows(const CountLaunch &a, hipStream_t st);
// rows[r * f.stride + w] <- the AND of the h blocks of the k-mer whose base-4 rank is r, for r < n_rows = 4^k
hipError_t launch_row_table(const IbfDev &f, uint64_t *rows, uint64_t n_rows, hipStream_t st);
// ... the three-hash build of the row form alone (the reads with a base outside ACGT): what the list form launches behind its own kernel
hipError_t launch_ibf_count_rows_twin(const CountLaunch &a, hipStream_t st);
// List form (rb_lists.hip, ibf_count_lists_kernel): one gather of a.list_lines lines per k-mer from a.list_table, a returning LDS add per listed bin.
bool list_form_serves(const CountLaunch &a);  // the row form's launches with one column slice, at most 8192 bins and strands below 65 536 k-mers
hipError_t launch_ibf_count_lists(const CountLaunch &a, hipStream_t st);
// counters[1 + i] += rows among 0, step, 2 step, ... < n_rows with more than 64 << i set bits (i = 0, 1, 2); counters start zeroed
hipError_t launch_list_census(const IbfDev &f, uint32_t *counters, uint64_t n_rows, uint64_t step, hipStream_t st);
// slots <- the list table at `lines` lines per slot, side <- the dense rows of the slots that overflow (at most side_cap are written),
// counters[0] += such slots; counters start zeroed
hipError_t launch_list_table(const IbfDev &f, uint16_t *slots, uint64_t *side, uint32_t *counters, uint64_t n_rows, uint32_t lines, uint32_t side_cap,
                             hipStream_t st);
// Wide list form (rb_wide_lists.hip, ibf_count_wide_lists_kernel; rb_wide_lists.h): filters of 8193 to 32 256 bins from a table of their
// own, one workgroup of several waves per read, every item written once (k-mers with a base outside ACGT are counted in the kernel).
struct WideCountLaunch {
    IbfDev f;
    ReadSrc src;
    uint32_t n_reads;
    uint16_t *out;
    uint32_t out_read_stride;
    int nt;           // non-temporal slot gathers
    int bound_prune;  // the second strand is skipped when the first reached n
    const uint32_t *slots;  // the filter's wide list table, `lines` lines per slot (resident form)
    const uint64_t *side;   // ... and its side table of side_rows dense rows
    uint32_t side_rows, lines;
};
bool wide_form_serves(const IbfDev &f, uint32_t max_len);
hipError_t launch_ibf_count_wide_lists(const WideCountLaunch &a, hipStream_t st);
// counters[1 + i] += rows among 0, step, 2 step, ... < n_rows with more than 64 x rbwide::kWideLines[i] set bits; counters start zeroed
hipError_t launch_wide_list_census(const IbfDev &f, uint32_t *counters, uint64_t n_rows, uint64_t step, hipStream_t st);
// slots <- the wide list table at `lines` lines per slot, side <- the dense rows of the slots that overflow (at most side_cap are
// written), counters[0] += such slots; counters start zeroed
hipError_t launch_wide_list_table(const IbfDev &f, uint32_t *slots, uint64_t *side, uint32_t *counters, uint64_t n_rows, uint32_t lines,
                                  uint32_t side_cap, hipStream_t st);
hipError_t launch_ibf_count_max_merged(const CountLaunch &a, const MergeMap &map, hipStream_t st);
// block b of a filter (width words at stride s_src, n_bins bins) -> bits [dst_bit, dst_bit + n_bins) of block b of dst (ORed in: dst starts zeroed)
hipError_t launch_invert_words(const uint64_t *src, uint64_t *dst, uint64_t n_words, hipStream_t st);
hipError_t launch_merge_bits(const uint64_t *src, uint32_t s_src, uint32_t width, uint32_t n_bins, uint64_t *dst, uint32_t s_dst, uint32_t dst_bit,
                             uint64_t n_blocks, hipStream_t st);
int split_waves_limit(int wpl, int planes, uint32_t max_kmers, int lg);
int split_waves_cap(int wpl, int planes, int lg);
int split_parts_plan(int wpl, int planes, uint32_t max_kmers, int lg, uint32_t n_items, uint32_t max_parts, uint32_t max_sub,
                     int *nw, int *sub);
hipError_t launch_reduce_slices(const uint16_t *part, uint32_t n_slices, uint32_t n_reads, uint16_t *maxcount,
                                uint32_t nf, uint32_t fidx, hipStream_t st);
hipError_t launch_decide(const DecideParams &P, const uint16_t *maxcount, const uint32_t *lens, const uint8_t *pre_status,
                         uint32_t n_reads, int mode, int32_t *best_target, uint8_t *decision, uint8_t *status,
                         hipStream_t st);
// micro-batches: pinned host block -> device staging by a kernel of the call's own stream (16-byte units; both blocks hold whole units)
hipError_t launch_copy_from_host(const void *h_src, void *d_dst, size_t bytes, hipStream_t st);
hipError_t launch_chunk_prep(const uint32_t *lens, const uint32_t *ids, uint32_t n_items, uint32_t chunk_start,
                             uint32_t chunk_len, uint32_t *eff_lens, uint8_t *pre_status, hipStream_t st);
hipError_t launch_insert(const IbfDev &f, uint64_t *words, const uint8_t *seq, const uint64_t *starts,
                         const uint64_t *ends, const uint64_t *bins, const uint64_t *kmer_prefix,
                         uint32_t n_fragments, uint64_t total_kmers, hipStream_t st);
hipError_t launch_restride_blocks(const uint64_t *src, uint32_t s_src, uint64_t *dst, uint32_t s_dst, uint32_t w_copy,
                                  uint64_t n_blocks, hipStream_t st);
hipError_t launch_compare_bits(const uint64_t *a, const uint64_t *b, uint64_t n_words, uint64_t *out3, hipStream_t st);
// per-bin occupancy (rb_dibf_bin_occupancy; rb_kernels.hip, ibf_bin_occupancy_kernel): by-value kernel argument ...
struct OccLaunch {
    const uint64_t *words;
    uint64_t n_blocks;
    uint64_t stride;         // words from one block to the next
    uint32_t bin_width, n_bins;
    uint32_t chunk_rows;     // wave rows a wave walks between two flushes of its planes
    uint32_t iters;          // chunks per wave
    uint32_t wgs_per_slice;  // workgroups that share one column slice
};
// ... and the launch: out (u64 [n_bins]) is zeroed on `st`, then out[j] = blocks whose bit j is set.  nt: non-temporal loads
void set_bin_occupancy_grid(uint32_t max_wgs_per_slice, uint32_t min_chunk_rows);
hipError_t launch_bin_occupancy(const uint64_t *words, uint64_t n_blocks, uint64_t stride, uint32_t bin_width, uint32_t n_bins, int nt,
                                uint64_t *out, hipStream_t st);
// assembling a filter from bins of others (rb_dibf_assemble; rb_kernels.hip, ibf_assemble_kernel): the source tables by value, the
// plan (CSR: offsets u64 [n_out_bins + 1], refs {u32 filter, u32 bin}) and the per-tile staging windows in device memory
constexpr uint32_t kAsmMaxSources = 8;     // == RB_ASSEMBLE_MAX_SOURCES
constexpr uint32_t kAsmWaves = 8;          // waves per workgroup
constexpr uint32_t kAsmOutWords = 8;       // out words a wave holds the lists of
constexpr uint32_t kAsmHeld = 8;           // refs per out bin held in registers; longer lists walk the plan in memory
constexpr uint32_t kAsmTileWords = kAsmWaves * kAsmOutWords;  // out words of a tile: 64 (4 096 bins)
constexpr uint32_t kAsmMaxLdsWords = 7680; // 60 KiB: the staged source windows of one step (the kernel's small tables fit beside them below 64 KiB)
constexpr uint32_t kAsmStepLdsWords = 4096; // ... and what a step is sized to when a block's windows leave the choice
struct AsmWindow { uint32_t lo, n; };      // words [lo, lo + n) of a source's block are what a tile's lists name
struct AsmLaunch {
    const uint64_t *src[kAsmMaxSources];
    uint64_t src_stride[kAsmMaxSources];
    uint64_t *out;
    uint64_t out_stride;         // words; the tiles cover all of it, so pad words are written (zero: no list names them)
    uint64_t n_blocks;
    uint64_t n_out_bins;
    const uint64_t *offsets;
    const uint2 *refs;           // .x = filter, .y = bin
    const AsmWindow *windows;    // [n_tiles][kAsmMaxSources]
    uint32_t n_srcs;
    uint32_t n_tiles;
    uint32_t wgs_per_tile;
    uint32_t blocks_per_chunk;   // a workgroup walks chunks of that many blocks, chunk = iteration * wgs_per_tile + workgroup
    uint32_t iters;
};
void set_assemble_grid(uint32_t max_workgroups, uint32_t blocks_per_chunk);
// windows_host: the same table the launch reads on the device (the launcher sizes every tile's step from it)
hipError_t launch_assemble(AsmLaunch a, const AsmWindow *windows_host, int nt, hipStream_t st);
hipError_t launch_fill_reads(uint8_t *seqs, uint64_t *offsets, uint32_t *lens, size_t n_reads, uint32_t read_len, uint64_t seed, hipStream_t st);
hipError_t launch_fill_synth(uint64_t *words, uint64_t used_words, uint32_t bin_width, uint32_t stride_words,
                             uint64_t last_mask, uint64_t seed, hipStream_t st);

}  // namespace rb

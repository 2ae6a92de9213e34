/*
 * readbouncer_amd_tuning.h -- measurement aids and scheduling knobs of libreadbouncer_amd.so.
 *
 * Nothing in this header has a counterpart in the reference and nothing in it changes a result: these calls pick kernel
 * forms, window lengths and batch cuts for A/B measurements, report what the engine planned, time its kernels, probe what the
 * device delivers, fill filters with synthetic bits and replay arrival processes.  bench.py, profiles/ and the tests use them;
 * a ReadBouncer integration needs only include/readbouncer_amd.h (the reference-mapped calls of INTEGRATION.md section 1).
 * Same shared library, same symbols.
 */
#ifndef READBOUNCER_AMD_TUNING_H_
#define READBOUNCER_AMD_TUNING_H_

#include "readbouncer_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- synthetic data ------------------------------------------------------------------------ */
/* synthetic filler for benchmarks: every bin bit ~ Bernoulli(55/256), padding bits clear */
RB_API int rb_dibf_fill_synth(rb_dibf *f, uint64_t seed);

/* ---- pool: statistics and scheduling ---------------------------------------------------------- */
/* Per worker, since creation or the last reset: the device it drives, seconds spent inside its engine's rb_classify_batch, reads
 * and parts of calls served.  busy / wall time = the share of the time that device's engine had work (bench.py --pool). */
RB_API int rb_pool_get_stats(rb_pool *p, size_t n, int *devices, double *busy_seconds, uint64_t *reads, uint64_t *calls, int reset);
RB_API int rb_pool_set_min_split(rb_pool *p, size_t reads_per_device);
/* Calls from several host threads run concurrently: each worker (engine + host thread per device) has a FIFO of its own,
 * an unsplit micro-batch goes to the least loaded worker, and callers only meet while a call's parts are queued -- K calling
 * threads keep K engines busy, like the reference's N classification threads behind one queue
 * (src/main/adaptive_sampling.hpp:745-751).  Per calling thread the calls stay ordered (each returns before the next starts).
 * rb_pool_set_serialize(p, 1) is a diagnostic: one call at a time, whoever makes it. */
RB_API int rb_pool_set_serialize(rb_pool *p, int enabled);
/* Kernel timing of every engine of the pool (rb_engine_set_timing / rb_engine_kernel_time per worker): total_ms[i] = summed K1 time
 * of worker i since the last collection, n_launches[i] = bracketed launches (a host batch crosses PCIe in slices, one launch
 * each).  For bench.py's pool legs: a roofline figure per device from kernel time, beside the PCIe-inclusive rate. */
RB_API int rb_pool_set_timing(rb_pool *p, int enabled);
RB_API int rb_pool_kernel_time(rb_pool *p, size_t n, double *total_ms, uint64_t *n_launches);

/* ---- arrival replay (config 5) ------------------------------------------------------------------ */
/* Replay of an arrival process through the engine (measurement aid for the live scenario; rb_live.cpp): chunk i = read_len
 * bytes at seqs + i*read_len, available arrival_s[i] seconds after the start (ascending); a work-conserving dispatcher
 * takes everything that has arrived (<= max_batch chunks, 0 = 16384) per rb_classify_batch call (check_unblock).
 * out_latency_s[i] = decision - arrival; the first call_cap calls report their size and service time; out_calls = number of
 * calls made.  The reference's counterpart is its classification thread popping one read at a time
 * (src/main/adaptive_sampling.hpp:214-356). */
RB_API int rb_replay_arrivals(rb_engine *e, const char *seqs, uint32_t read_len, size_t n, const double *arrival_s,
                              size_t max_batch, double error_rate, double significance, uint8_t *out_decision,
                              double *out_latency_s, uint32_t *out_call_reads, double *out_call_service_s, size_t call_cap,
                              size_t *out_calls, double *out_elapsed_s);
/* (max_batch is clamped to min(max_batch, n, 2^20); arrival_s that is not ascending is RB_ERR_INVALID_ARG; the dispatcher
 * spins on the steady clock between arrivals -- it owns a core for the length of the replay, like the reference's
 * classification thread polling its queue, adaptive_sampling.hpp:226-228.)
 * The same dispatcher in front of the live step: chunk i belongs to read read_ids[i] and goes through rb_live_process, so
 * an undecided read's next chunk is classified as the concatenation with what once_seen holds (up to the cut-off, i.e.
 * reads of up to ~1.9 kbp) -- adaptive_sampling.hpp:276-338.  out_action as rb_live_process. */
RB_API int rb_live_replay_arrivals(rb_live *lv, const uint32_t *read_ids, const char *seqs, uint32_t read_len, size_t n,
                                   const double *arrival_s, size_t max_batch, uint8_t *out_action, double *out_latency_s,
                                   uint32_t *out_classified_len, uint32_t *out_call_reads, double *out_call_service_s,
                                   size_t call_cap, size_t *out_calls, double *out_elapsed_s);

/* ---- where a large table lies in HBM ---------------------------------------------------------------
 * Filters of 1 GiB and more are placed by trial: the same table gathers 1.7-2.9 % slower or faster from one allocation of a process to
 * the next (where the driver finds the pages -- an 8 GiB power-of-two table always gets the fast kind, a reference-sized 4.7 GB one does
 * or does not), so rb_dibf_create / _upload / _open / _clone_to / _resize_bins allocate up to `tries` candidates (default 5), probe each
 * with random whole-block gathers (~0.1 s), stop early only when one is 3 % faster than the slowest seen, keep the best and free the others.
 * Transient cost: up to (tries - 1) x the table of HBM at load time (never more than half of what is free) and 1-2 s.  tries = 0 or 1: off.
 * Never done on a device where an engine of this process is alive (see rb_dibf_placement_cost).  Process-wide; results never depend on it.  rb_dibf_placement: how many allocations were probed for this filter (0: not placed by
 * trial), what the kept one and the slowest one delivered in GB/s. */
RB_API int rb_set_placement_tries(int tries);
/* How rb_dibf_bin_occupancy[_device] cuts a table, for every later pass of this process: at most max_workgroups_per_slice workgroups
 * (16 waves each) per column slice and no chunk shorter than min_chunk_rows wave rows; 0 = the built-in rule (one workgroup per CU,
 * chunks of at least 256 rows).  A wave flushes its counter planes after every chunk and a chunk never exceeds 4 080 rows, so with few
 * workgroups a table of a hundred MiB walks full-length chunks, several per wave -- what a table of 16 GiB does by itself.  Counts
 * never depend on it; tests and experiments. */
RB_API void rb_set_bin_occupancy_grid(uint32_t max_workgroups_per_slice, uint32_t min_chunk_rows);
/* How rb_dibf_assemble / rb_dibf_select_bins cut a table, for every later call of this process: at most max_workgroups workgroups
 * (8 waves each) in all, and chunks of blocks_per_chunk blocks; 0 = the built-in rule (four workgroups per CU, chunks of 1 024 blocks).
 * A workgroup reads its part of the plan once and then walks chunk after chunk, so with one workgroup and chunks of 1 or 5 blocks a
 * table of a few thousand blocks goes through many chunks, short last ones and short steps included.  The bits never depend on it;
 * tests and experiments.  The counterpart of rb_set_bin_occupancy_grid. */
RB_API void rb_set_assemble_grid(uint32_t max_workgroups, uint32_t blocks_per_chunk);
/* seconds the kernel of the last successful rb_dibf_assemble / rb_dibf_select_bins of the calling thread ran (a hipEvent pair around
 * the launch; 0.0 before the first) -- what `--edit-ibf` prints and profiles/assemble_cost.py measures */
RB_API double rb_assemble_last_seconds(void);
/* table size beyond which the library reads with non-temporal loads: the default of rb_engine_set_nt_threshold and the rule of the
 * passes that have no engine (rb_dibf_bin_occupancy) */
RB_API uint64_t rb_nt_threshold_default(void);
RB_API int rb_dibf_placement(const rb_dibf *f, uint32_t *tries, double *kept_gbps, double *worst_gbps);
/* What the trial cost for this filter: seconds spent allocating and probing the candidates, seconds waited afterwards until the kept
 * table probed as in the trial (bounded by 3 s; the driver clears the freed candidates in the background), the most HBM the candidates
 * held at once, and -- for a table of 1 GiB or more that was NOT placed by trial -- why: 1 = an engine was alive on the device (a
 * process that is already classifying there is not stalled by probe launches and transient copies: the table takes the first
 * allocation), 2 = less than twice the table was free.  bench.py keeps these per filter in bench_detail.json.  Any pointer may be NULL. */
RB_API int rb_dibf_placement_cost(const rb_dibf *f, double *trial_seconds, double *settle_seconds, uint64_t *peak_bytes, uint32_t *skipped);

/* ---- engine: kernel forms, planner, timing, probe ------------------------------------------------ */
/* Filters of one hash geometry in one table.  Every filter the reference builds with one fragment_size has noOfBits =
 * BinSizeBits x 64 x binWidth (src/IBF/IBFBuild.cpp:404-413), i.e. the same noOfBlocks whatever its bin count; with equal k and
 * three hash functions a k-mer then hashes to the same block number in all of them.  For such filters (blocks of at most 8
 * words, at most 16 words together) the engine keeps a merged copy in which their blocks sit side by side, and one gather per
 * (k-mer, hash function) serves all of them -- the narrow filters are bound by requests, not bytes.  mode 1 (default): when it
 * pays -- the members one after the other are estimated to take longer than one pass over the merged table (a merged table of
 * two to four words is served by the clock-phased kernel like a filter of that width, wider ones by plain gathers): the
 * reference's README shape (a two-word deplete filter and three one-word targets), any two filters too large for the
 * clock-phased kernels, small ones whose merged copy still fits an L2, two or three one-word filters of up to 30 MiB --;
 * 2: whenever two or more filters qualify; 0: never.  Large batches only (micro-batches keep the latency kernels); the copy
 * follows changes of its members (rb_dibf_insert ...).  Results are identical. */
RB_API int rb_engine_set_merge(rb_engine *e, int mode);
/* What the engine has merged (or will, at its next large batch): the number of merged tables, the filters they serve and the HBM
 * bytes of the copies, which live beside the members and are SHARED by every engine of the process that merges the same filters in
 * the same order on the same device (N threads with an engine each -- adaptive_sampling.hpp:745-751 -- gather from one copy; it
 * is freed with its last engine).  A copy larger than 16 GiB (RB_MERGE_MAX_BYTES) is not made,
 * and a group whose copy the device has no room for dissolves at its first call: its members are then served one by one.
 * Any out pointer may be NULL. */
RB_API int rb_engine_merge_info(rb_engine *e, uint32_t *n_tables, uint32_t *n_filters, uint64_t *copy_bytes);

/* Micro-batch latency: batches of at most max_reads reads (x column slices) run the latency form of the
 * count kernel (one workgroup per read, its waves share the read's k-mers and strands); larger batches
 * run the throughput form (one wave per read).  Results are identical.  0 disables; default 2048. */
RB_API int rb_engine_set_split_threshold(rb_engine *e, uint32_t max_reads);

/* The count kernels of different filters run concurrently (filter 0 on the call's stream, the others on the engine's
 * auxiliary streams, joined by events before the decision kernel) -- the reference starts one std::async per filter
 * (src/IBF/IBFClassify.cpp:256-260).  0 serialises them on one stream.  Default on. */
RB_API int rb_engine_set_overlap(rb_engine *e, int enabled);

/* Latency kernel on wide filters (blocks of 17+ word columns): up to max_parts workgroups share one read, each wave
 * walking 1/max_shares of a 64-k-mer tile (default 8 and 4); 0 or 1 parts = one workgroup per read.  The partial
 * counters are added by the last workgroup to finish.  Results are identical. */
RB_API int rb_engine_set_split_parts(rb_engine *e, uint32_t max_parts, uint32_t max_shares);

/* Engines with one filter, micro-batches of up to 512 reads in the latency form: the count kernel makes the decisions too -- the
 * workgroup that writes a read's raw maximum runs check_unblock's decision for it (src/main/adaptive_sampling.hpp:35-113) -- instead
 * of a decision kernel launched behind it: one dependent launch less per call (1-2 us).  0 keeps the two launches.  Default on.
 * Results are identical. */
RB_API int rb_engine_set_fold_decide(rb_engine *e, int enabled);

/* Opt-in.  rb_classify_batch with up to 2 048 reads: the kernel that writes the call's last result also stores a sequence number into a
 * word of page-locked host memory (behind a system-scope release), and the calling thread spins on that word instead of waiting for the
 * stream -- the stream's own wait returns about 4 us later than the results are there (median of a call: one read 40.6 -> 36.1 us).  The
 * price is the tail: the runtime retires its commands in the stream's wait, without it in bulk every few hundred calls (p99 of config 5's
 * replay + 0-20 us from box to box), which is why this is off by default.  A word that has not arrived after 20 ms falls back to the
 * stream, which also reports a failed kernel, and every 256th call waits for the stream as well.  0 = off (default), 1 = on, a value
 * above 1 = on with that period instead of 256 (measurements).  Results are identical. */
RB_API int rb_engine_set_completion_word(rb_engine *e, int enabled);

/* Filters larger than table_bytes are gathered with non-temporal loads (default 512 MiB = 2x the Infinity
 * Cache; measured +2.4 % on the 8 GiB filter, -1.9 % on a 0.41 GB one).  Results are identical. */
RB_API int rb_engine_set_nt_threshold(rb_engine *e, uint64_t table_bytes);

/* Narrow filters -- blocks of one to eight words, tables of a few L2 sizes (10-20 MB: a bacterial genome at the reference's
 * default fragment_size) -- are bound by cache and fabric REQUESTS, not bytes: each 8-byte gather that misses the XCD's 4 MiB
 * L2 costs a 128-byte request.  Two measures, both leave the results untouched:
 *  - filters of at most `table_bytes` (default 128 MiB) never run beside another filter of the same call, so each has the
 *    L2 to itself (rb_engine_set_serial_table_bytes; 0 = overlap everything as rb_engine_set_overlap says);
 *  - for tables of one- to four-word blocks of [min_table_bytes, max_table_bytes] (default 1.25-128 MiB; three and four words:
 *    4.5-48 MiB) and batches of at least min_reads (2049: everything above the latency kernel's micro-batches; more for tables
 *    beyond 32 MiB) the throughput kernel gathers in clock-phased slices: the
 *    table is cut into slices of 0.5 to 4 MiB (at most 32) and the 100 MHz wall clock tells every wave which slice to gather
 *    from, in windows of base_ticks + ticks_per_mib * table MiB ticks of 10 ns -- both 0 = the built-in rule, a whole cycle
 *    over the table of 33-60 us by kernel shape -- so an XCD's L2 holds one slice at a time
 *    (rb_engine_set_phased; max_table_bytes = 0 switches it off; all five arguments 0 also takes one-word filters back to
 *    the plain kernel, whose 512-k-mer tiles are half empty on 250 bp reads).  Blocks of five and more words gain nothing
 *    from phases and keep the plain kernel. */
RB_API int rb_engine_set_serial_table_bytes(rb_engine *e, uint64_t table_bytes);
RB_API int rb_engine_set_phased(rb_engine *e, uint64_t min_table_bytes, uint64_t max_table_bytes, uint32_t base_ticks,
                                uint32_t ticks_per_mib, uint32_t min_reads);
/* What the engine would launch for filter `filter_index` (deplete filters first) on a batch of n_reads reads of at most max_len
 * bases, with its current settings: kernel form, geometry, and -- for the phased form -- the row of the planner's table
 * (readbouncer_amd/csrc/rb_phase_plan.h) with the slice size and window length it gives.  For bench.py's roofline line (which
 * kernel was timed), profiles/phase_rule_check.py (rule against measured best) and the tests; no reference counterpart. */
typedef struct rb_plan_info {
    char kernel[48];             /* ibf_count_max_kernel | _phased_kernel | _merged_kernel | _split_kernel */
    uint64_t table_bytes;        /* of the table the lookups go to (the merged copy when merged_members > 0) */
    uint32_t block_words, stride_words;
    uint32_t merged_members;     /* > 0: the filter is served from a merged table of that many filters */
    uint32_t lanes_per_block_log2, words_per_lane, column_slices, counter_planes, nontemporal;
    uint32_t split_waves;        /* latency form: waves per workgroup (0: throughput form) */
    uint32_t phased;             /* 1: clock-phased gathers */
    uint32_t phase_shape;        /* rbplan::PhaseShape */
    char phase_shape_name[64];
    uint32_t phase_slice_log2, phase_slices, phase_window_ticks;  /* window length in effect, in 10 ns ticks */
    uint32_t phase_rule_ticks;   /* what the planner's table alone gives (differs after rb_engine_calibrate) */
    uint32_t reserved0;
    uint64_t phase_slice_bytes;  /* slice length in effect: 2^phase_slice_log2, or -- four-word one-lane builds -- the equal-length slices
                                  * the table is cut into instead (fewer and up to 1.19 x longer; rb_phase_plan.h, phase_equal_slices) */
    uint64_t row_table_bytes;    /* > 0: kernel is ibf_count_rows_kernel, the row form of the plain kernel (rb_engine_set_row_table), gathering
                                  * from the filter's row table of that size -- the one it has, or the one the call would build */
} rb_plan_info;
RB_API int rb_engine_plan(rb_engine *e, size_t filter_index, size_t n_reads, uint32_t max_len, rb_plan_info *out);
/* The same question for the query passes of readbouncer_amd.h (locate, hits, prefixes and spans, host and device forms),
 * which none of the settings above but rb_engine_set_nt_threshold reaches (the list settings below are their own: rb_engine_set_pass_lists
 * for locate and hits, rb_engine_set_prefix_lists for prefixes): the build a call on items of at most max_len bases takes
 * for filter `filter_index` (prefixes: no item is longer than the last checkpoint), filled by the functions the launches themselves go
 * through.  Host arithmetic only; for the tests, which pin every build of a pass to the oracle and need to know which one a launch
 * took. */
typedef struct rb_pass_plan {
    uint32_t lanes_per_block_log2, words_per_lane, column_slices;
    uint32_t counter_planes;     /* 10 while the k-mers of max_len bases fit them and the filter has three hash functions, else 16 */
    uint32_t nontemporal;        /* locate, hits, prefixes: 1 = the non-temporal twin (blocks of a whole wave beyond the threshold) */
    uint32_t hash_functions;     /* 3: the build with three compile-time hash functions; 0: the run-time hash count */
    uint32_t spans_nontemporal;  /* spans (one wave per query, no geometry, no planes): 1 = its non-temporal twin, at any block width */
    uint32_t list_lines;         /* locate and hits only (spans are not affected; prefixes answer in rb_engine_plan_prefix): 0 = the plain build the fields above describe;
                                    1, 2 or 4 = the list form (rb_engine_set_pass_lists) at that slot size, for this filter, this max_len and
                                    the engine's setting as it stands -- items the list form does not take still run the plain build */
} rb_pass_plan;
RB_API int rb_engine_plan_pass(rb_engine *e, size_t filter_index, uint32_t max_len, rb_pass_plan *out);
/* The locate and hits passes of readbouncer_amd.h (host and device forms) from a filter's LIST TABLE (below: rb_dibf_list_table_build), opt-in.  The list
 * form counts an item in full on both strands from the slots the count kernel gathers -- 2 x lines of 128 bytes per k-mer, not h whole
 * blocks per strand -- and scans its per-bin counters for the maximum, its lowest bin, the bins at the threshold and the records;
 * results are those of the plain form, bit for bit.  Decided per filter and per call, so an engine may mix the forms: a filter takes it
 * when the mode allows, the list form serves its geometry and the call's max_len (what RB_ROW_TABLE_LISTS serves: whole-wave blocks in
 * one column slice of at most 8192 bins, three hash functions, k <= 13, fewer than 65 536 k-mers), the engine is no column shard, the
 * call's stream is not being captured, and the filter has a list table of the present version of its bits.  Work items with a base
 * outside ACGT, and items that are not RB_OK, are served from the filter's own table in the same call.
 *   RB_PASS_LISTS_OFF (default): the passes read each filter's own table, always.
 *   RB_PASS_LISTS_CURRENT: a filter's list table is used when it has a current one; none is ever built.
 *   RB_PASS_LISTS_BUILD: a filter without a current table gets one built by the call, under the rules of the count path's list form
 *     (rb_engine_set_row_table's max_bytes, free memory, density); a refusal means the plain form, not an error.
 * rb_engine_plan_pass reports the choice in list_lines.  Spans, prefixes and resume are not affected (resume has a setting of its
 * own, per slot set: rb_resume_set_lists below; so have prefixes, per engine: rb_engine_set_prefix_lists below). */
#define RB_PASS_LISTS_OFF 0
#define RB_PASS_LISTS_CURRENT 1
#define RB_PASS_LISTS_BUILD 2
RB_API int rb_engine_set_pass_lists(rb_engine *e, int mode);
/* The resume pass of readbouncer_amd.h (host and device forms) from a filter's list table, opt-in PER SLOT SET -- the
 * engine's setting above does not reach it.  mode is RB_PASS_LISTS_OFF (the default) / _CURRENT / _BUILD with the meaning above; any other
 * value is RB_ERR_INVALID_ARG.  Decided per filter and per call by the rules of locate and hits, with max_chunk_len + 31 bases (the
 * stitched "tail + chunk") as the call's bound: whole-wave blocks in one column slice of at most 8192 bins, three hash functions,
 * k <= 13, fewer than 65 536 k-mers, no column shard, no stream capture, a list table of the present version of the filter's bits.  An
 * engine may mix list-served and plain-served filters in one call.  For a served filter, an item that is not refused and whose stitched
 * string holds no base outside ACGT -- any length; a tail that carries an N from an earlier chunk counts -- has its new k-mers counted
 * from the list table (2 x lines of 128 bytes per k-mer) into 16-bit counters on chip, which are then added onto the slot's sixteen
 * bit-sliced planes, exactly at the uint16_t wrap; every other item runs the plain form in the same call.  The slot format is the plain
 * form's: results, the count vectors read back and the slots' bytes are identical whichever form served which feed, so the setting may change
 * between calls on live slots.  FIRST, PEEK, refusals, the duplicate-slot check and the staleness check are as without it. */
RB_API int rb_resume_set_lists(rb_resume *r, int mode);
/* What a resume call takes for filter `filter_index` of the set's engine, as things stand now: the plain build (ibf_resume_kernel always
 * has sixteen planes) and list_lines -- 0 = the plain form alone; 1, 2 or 4 = the list form at that slot size for the items it takes.
 * Host arithmetic only: nothing is built or dropped (RB_PASS_LISTS_BUILD reports the table once a call has built it). */
typedef struct rb_resume_plan_info {
    uint32_t lanes_per_block_log2, words_per_lane, column_slices;
    uint32_t nontemporal;   /* 1 = the plain build's non-temporal twin (blocks of a whole wave beyond the threshold) */
    uint32_t list_lines;
} rb_resume_plan_info;
RB_API int rb_resume_plan(rb_resume *r, size_t filter_index, rb_resume_plan_info *out);
/* The prefix pass of readbouncer_amd.h (host and device forms) from a filter's list table, opt-in with a setting of ITS
 * OWN: rb_engine_set_pass_lists does not reach the prefix pass, and this setting does not reach locate or hits.  mode is
 * RB_PASS_LISTS_OFF (the default) / _CURRENT / _BUILD with the meaning above; any other value is RB_ERR_INVALID_ARG.  Decided per filter
 * and per call by the rules of locate and hits, with min(the call's max_len, the last checkpoint) as the call's bound -- so "fewer than
 * 65 536 k-mers" is asked of the last checkpoint, not of the reads -- whole-wave blocks in one column slice of at most 8192 bins, three
 * hash functions, k <= 13, no column shard, no stream capture, a list table of the present version of the filter's bits.  For a served
 * filter, an item whose status so far is RB_OK, whose w = min(length, last checkpoint) bases lie within the call's bound and are all
 * ACGT -- any length; a base outside ACGT BEHIND the last checkpoint does not matter -- has the k-mers between two checkpoints counted from
 * the list table (2 x lines of 128 bytes per k-mer) into 16-bit counters on chip, which are scanned for their maximum at every checkpoint
 * that adds a k-mer; every other item runs the plain form in the same call.  Results are the plain form's, bit for bit. */
RB_API int rb_engine_set_prefix_lists(rb_engine *e, int mode);
/* What a prefix call takes for filter `filter_index` on items of at most max_len bases with `last_checkpoint` as its last checkpoint, as
 * things stand now: the plain build (the fields of rb_pass_plan for min(max_len, last_checkpoint) bases) and list_lines -- 0 = the plain
 * form alone; 1, 2 or 4 = the list form at that slot size for the items it takes.  Host arithmetic only: nothing is built or dropped
 * (RB_PASS_LISTS_BUILD reports the table once a call has built it). */
typedef struct rb_prefix_plan_info {
    uint32_t lanes_per_block_log2, words_per_lane, column_slices;
    uint32_t counter_planes, nontemporal, hash_functions;   /* as rb_pass_plan's */
    uint32_t list_lines;
} rb_prefix_plan_info;
RB_API int rb_engine_plan_prefix(rb_engine *e, size_t filter_index, uint32_t max_len, uint32_t last_checkpoint, rb_prefix_plan_info *out);
/* The work items the list form of the prefix pass took (*listed) and left to the plain form (*plain) since the last reset, summed over
 * the calls in which at least one filter was list-served (counted on the device by the kernel that decides it; a call with no list-served
 * filter counts nothing).  Either pointer may be NULL.  reset != 0 zeroes both afterwards.  Waits for the engine's own stream. */
RB_API int rb_engine_prefix_lists_items(rb_engine *e, uint64_t *listed, uint64_t *plain, int reset);
/* Fits the window lengths of the clock-phased gathers to THIS device: the planner's table was measured on one box, and clocks,
 * firmware and compilers move the optima.  For every table the engine would serve with the phased form on batches of n_reads reads
 * of read_len bases, K1 is timed on synthetic reads with the table's window and with 0.7 / 0.85 / 1.2 / 1.45 x that (same slice
 * size); the best point of the curve smoothed along the window length replaces the rule for that table and kernel shape when it
 * wins by 4 % and a second measurement confirms it, until the engine goes away or rb_engine_set_phased /
 * rb_engine_set_phase_slices is called.  Calibrate at the batch size the engine will be given: where the dips and cliffs of the
 * two-word and wide shapes lie moves with it.  Stops trying new windows after max_ms (0 = no limit); a few
 * launches per table, tens of milliseconds in all.  Results never depend on it; call it on an idle engine.  n_tables: phased
 * tables found; n_changed: how many got a new window.  No reference counterpart (profiles/phase_rule_check.py is the
 * offline form of the same sweep, with an exit code). */
RB_API int rb_engine_calibrate(rb_engine *e, size_t n_reads, uint32_t read_len, double max_ms, uint32_t *n_tables, uint32_t *n_changed);

/* How the phased form cuts a table, for tests and experiments: slices of 2^slice_log2 bytes (0 = the built-in rule, 0.5 to 4 MiB
 * by table size and block width; 1-5 = as small as max_slices allows, which puts test-sized tables through many slices), and
 * never more than max_slices (1-32, default 32; a table that would need more gets larger slices).  Results are identical. */
RB_API int rb_engine_set_phase_slices(rb_engine *e, uint32_t slice_log2, uint32_t max_slices);
/* ... or into n_slices slices of EQUAL length, any number of blocks each (1-32; 0 = back to the built-in rule, which itself cuts the
 * four-word tables, the two-word tables of the LDS-offset builds and one-word tables from 50 MiB on this way: slices shorter than an
 * L2 leave the lines of the window before in place while the next slice arrives).  Ignored while rb_engine_set_phase_slices names a
 * slice size.  Results are identical. */
RB_API int rb_engine_set_phase_equal_slices(rb_engine *e, uint32_t n_slices);

/* Two-word tables (65-128 bins, or two to three small targets merged) of up to 2^21 - 2 blocks (32 MiB), reads of up to 256 k-mers, phased
 * form: `reads` = 2 or 3 takes the build that carries that many reads per wave through one pass of the windows -- AND accumulators in
 * registers, block numbers packed into LDS -- so that a pass, which reloads the table once per XCD whatever rides along, serves more
 * reads (40 instead of 28 per CU at two reads per wave); 1 = one read per wave with the offsets in LDS (eight waves per SIMD);
 * 0 = the one-read build that keeps the offsets in registers.  On a merged table these builds gather from a complemented twin of the
 * copy (the bounds check's zero is then neutral and the masking goes away); + 16 keeps the AND form there too (measurements).
 * Results are identical. */
RB_API int rb_engine_set_reads_per_wave(rb_engine *e, uint32_t reads);

/* OPT-IN, off by default; never part of a roofline figure (work is skipped).  check_unblock (src/main/adaptive_sampling.hpp:35-113) looks at a
 * filter's count only through "count >= threshold(r)" and "count >= threshold(r - 0.02)" (the rescan of :55-56); both are settled the moment
 * some bin of the filter reaches the larger of the two thresholds on either strand -- the reference counts on, and counts again for the
 * rescan.  With this mode on, RB_MODE_CHECK_UNBLOCK calls of the throughput form (batches above the micro-batch limit) that do NOT ask for
 * the raw maxima (out_maxcount / d_maxcount NULL) let a wave of the plain count kernel (filters of five and more word columns: the
 * depletion filter) stop there; target filters do so only when best_target is not asked for either (their counts pick it).  Every
 * output the call returns is identical to the mode being off.  In host depletion most reads are positive and stop after a fraction of
 * one strand. */
RB_API int rb_engine_set_early_decision(rb_engine *e, int enabled);

/* On by default.  The plain count kernel (wide filters, throughput form) stops gathering a lane's 16-byte column of the blocks once
 * none of its bins can reach the read's maximum any more: every k-mer adds at most 1, so a bin whose count plus the k-mers still to
 * come is at most the best count seen on either strand cannot change the maximum.  The maxima stay exact; 0 gathers everything (A/B
 * runs, tests).  Results are identical. */
RB_API int rb_engine_set_bound_pruning(rb_engine *e, int enabled);

/* Refinements of bound pruning, all on by default; they change which gathers are skipped, never a result.  Bit 0 of `mask`: the
 * bound is checked after every eight k-mers instead of after every 64 (behind a scalar gate that opens once the best count so far
 * reaches the k-mers still to come).  Bit 1: both strands are counted for their first 64 k-mers, the one with the larger maximum so
 * far is finished first (a tie: forward) and the other continues against that maximum -- a read given as its reverse complement no
 * longer counts its forward strand in full against nothing.  Bit 2 (needs bit 1): before the second strand is continued, its remaining
 * k-mers are gathered for the FIRST hash only, on top of its 64-k-mer counts -- a k-mer counts for a bin only where all hashes have
 * the bit, so this is an upper bound at a third of the lines; if its maximum does not pass the first strand's maximum the strand is
 * done, otherwise it is counted in full.  Attempted where the first strand's maximum makes it promising (rb_engine_set_cert_load);
 * never in a launch that several filters share (fused micro-batches).  Bit 3 (needs bits 1 and 2): the first strand is itself finished in
 * two steps.  Its best bin after 64 k-mers lies in one 128-byte line of every block; the bins of that line are counted to the end first,
 * alone, which gives a count that some bin truly reaches at an eighth of the lines, and all other bins of the strand are then shown not
 * to pass it from the FIRST hash only, as for the second strand (where that is not promising, or fails, they are counted in full against
 * it).  Attempted where the first strand's 64-k-mer maximum is large enough (rb_engine_set_lead_min).
 * 0 = the bound as rb_engine_set_bound_pruning alone gives it; ignored while bound pruning is off.  Applies to the plain count kernel's builds that take the bound (wide filters, throughput form, no early
 * decision). */
RB_API int rb_engine_set_prune_parts(rb_engine *e, uint32_t mask);

/* When the certificate of rb_engine_set_prune_parts (bit 2) is attempted for filter `filter_index` (deplete filters first, as in
 * rb_engine_plan): when the first strand's maximum is at least the other strand's 64-k-mer maximum + ceil(d rem + 4.5 sqrt(d (1 - d) rem)),
 * rem = the k-mers behind the first 64 and d = `load`, a bit load (set bits / blocks of a bin).  load < 0 (the default): d is the
 * load of the filter's FULLEST bin -- an attempt fails on the one bin that passes the allowance, so it has to cover every bin --
 * measured with the occupancy pass (rb_dibf_bin_occupancy_device, into memory the engine owns) by the first call that can attempt
 * a certificate on the filter, and again after its bits have changed; a call whose stream is being captured does not measure and
 * goes without the certificate.  0: always attempt; >= 1: never.  The rule only picks the attempts: results never depend on it. */
RB_API int rb_engine_set_cert_load(rb_engine *e, size_t filter_index, double load);

/* When bit 3 of rb_engine_set_prune_parts is attempted for filter `filter_index`: when the first strand's maximum after 64 k-mers is at
 * least `min_count`.  min_count < 0 (the default): the smallest count that a read without a match is not expected to reach there -- with
 * d the load rb_engine_set_cert_load describes and h hash functions a bin counts a foreign k-mer with probability d^h, and the value is
 * the smallest t with 2 n_bins P(Binomial(64, d^h) >= t) <= 0.01 (8 for d = 0.21, h = 3 and 8192 bins) -- so that such reads, which gain
 * nothing, do not walk the read twice.  0: always attempt.  The value only picks the attempts: results never depend on it. */
RB_API int rb_engine_set_lead_min(rb_engine *e, size_t filter_index, int min_count);

/* Measurement and test aid, NULL by default: device memory into which every wave of the plain count kernel (throughput form) writes one
 * 8-byte record when it has finished its (read, column slice) -- bit 0: the strand finished first (0 forward, 1 reverse); bit 1: both
 * strands were probed and the lead chosen; bit 2: a certificate was attempted for the other strand; bit 3: it held; bit 4: the line of the first strand's best bin was counted first;
 * bit 5: a certificate was attempted for that strand's other bins; bit 6: it held; bit 15: always set; bits 16-31 and 32-47: the k-mer position at which the gathers of the
 * forward and of the reverse strand ended (the number of k-mers: counted to the end; less: no lane could reach the maximum any more,
 * or the strand was not continued behind its 64-k-mer probe; 0: not counted).  Records lie filter after filter in engine order,
 * within a filter [read][column slice] (rb_engine_plan names the slices); a filter that the call does not launch on its own takes NO
 * room in that order -- one served by a merged table of several narrow filters, and, on a column-sharded engine, one of which this
 * rank holds no column; the caller sizes and zeroes the memory and keeps it alive
 * while set.  Calls of other kernel forms write nothing, and neither do micro-batches in which several filters of one kernel geometry
 * share a launch (batches up to rb_engine_set_split_threshold on an engine with several filters): a fused launch writes no record and
 * never attempts the certificate of rb_engine_set_prune_parts. */
RB_API int rb_engine_set_prune_trace(rb_engine *e, void *d_trace);

/* ROW TABLE of a resident filter (k <= 13, blocks of a whole wave: more than 32 words).  A k-mer counts in a bin where all h of its
 * blocks have the bit, and for a resident filter that AND depends on the k-mer alone; there are only 4^k k-mers without an N.  The table
 * holds that AND for each of them -- row r for the k-mer whose base-4 digits are r (A C G T = 0 1 2 3, first base most significant), 4^k
 * rows of the filter's block stride -- so that the count kernel gathers ONE block per k-mer instead of h (ibf_count_rows_kernel).  Results
 * are identical: reads with a base outside ACGT have k-mers without a row and are counted from the filter's own table by a second
 * launch over the same batch, the three-hash twin of the row build (a wave of either launch leaves at once when its read is the other's).  The FILTER owns the table: engines on one filter share it, rb_dibf_free frees it, and every call that changes the filter's
 * bits (insert, add_sequence, fill_synth, rb_dibf_touch) drops it; filters made from others (resize, assemble, select, clone, open,
 * upload) start without one.
 *   rb_dibf_row_table_build: build it now unless a current one exists.  max_bytes = 0: no limit of the caller's; the rule that a table
 *     takes at most half of the device memory free at that moment holds whatever max_bytes says.  A refusal is not an
 *     error: the call returns RB_OK and rb_dibf_row_table_info says why (refused != 0) -- k above 13, narrow blocks, 4^k x stride above
 *     max_bytes or above half of the free device memory, or the allocation failed.
 *   rb_dibf_row_table_drop: free it.
 *   rb_dibf_row_table_info: bytes and rows of the current table (0: none), what building it cost, why the last build was refused.
 *   rb_dibf_row_table_download: the table's words into host memory (tests).
 *   rb_engine_set_row_table(mode, max_bytes): RB_ROW_TABLE_OFF never uses a table; RB_ROW_TABLE_AUTO (default, max_bytes 96 GiB) uses
 *     it -- building it inside the classify call when there is none -- for launches of the plain count kernel on whole-wave blocks with
 *     three hash functions (no latency form, no fused micro-batch, no early-decision mode, no column shard, no trace asked for, k <= 13)
 *     whose batch alone repays the build: items x 2 x k-mers x (h - 1) >= 4^k x (h + 1) block transfers (config 3: 193 000 reads of
 *     360 bp); RB_ROW_TABLE_FORCE drops the batch-size rule and the trace rule.  A call whose stream is being captured neither builds
 *     nor uses a table (a graph would keep the address of memory that the next change of the filter frees).  The row launches are
 *     non-temporal when the ROW TABLE is beyond rb_engine_set_nt_threshold, whatever the filter's own size.
 *     Wherever a condition fails or the build is refused the call runs the three-hash kernel as before.  max_bytes = 0 keeps the value. */
#define RB_ROW_TABLE_OFF 0
#define RB_ROW_TABLE_AUTO 1
#define RB_ROW_TABLE_FORCE 2
#define RB_ROW_REFUSED_NONE 0
#define RB_ROW_REFUSED_K 1         /* k above 13 */
#define RB_ROW_REFUSED_NARROW 2    /* blocks of 32 words or fewer */
#define RB_ROW_REFUSED_MAX_BYTES 3 /* 4^k x stride above max_bytes */
#define RB_ROW_REFUSED_FREE 4      /* ... above half of the free device memory */
#define RB_ROW_REFUSED_ALLOC 5     /* the allocation failed */
#define RB_ROW_REFUSED_CAPTURE 6   /* the call's stream was being captured (engine builds only) */
typedef struct rb_row_table_info {
    uint64_t bytes, rows;   /* of the current table; 0: none */
    uint64_t want_bytes;    /* 4^k x stride x 8 (0: k above 13) */
    double build_ms;        /* kernel time of the last build */
    double alloc_s;         /* seconds its allocation took */
    uint32_t refused;       /* RB_ROW_REFUSED_*: why the last build did not happen */
    uint32_t builds;        /* tables built for this filter so far */
} rb_row_table_info;
RB_API int rb_dibf_row_table_build(rb_dibf *f, uint64_t max_bytes);
RB_API int rb_dibf_row_table_drop(rb_dibf *f);
RB_API int rb_dibf_row_table_info(rb_dibf *f, rb_row_table_info *out);
RB_API int rb_dibf_row_table_download(rb_dibf *f, uint64_t *words, uint64_t n_words);
RB_API int rb_engine_set_row_table(rb_engine *e, int mode, uint64_t max_bytes);

/* LIST TABLE of a resident filter: the row table's content as sparse lists.  A row has d^h of its bits set (a filter sized for a
 * false-positive rate of 0.01: about 1 %), so per N-free k-mer the table holds the BIN NUMBERS of its row, ascending, as 16-bit entries in
 * one slot of 1, 2 or 4 lines of 128 bytes, the rest of the slot 0xFFFF; the count kernel (ibf_count_lists_kernel) gathers that slot
 * instead of the row's 8 lines and counts each listed bin with one LDS add into per-read 16-bit counters.  The slot size is the smallest
 * that at most one in 1024 of up to 65 536 sampled rows overflows; a row that does overflow keeps its dense row in a side table that its
 * slot names (first entry 0xFFFE, then the row's index in two entries).  Serves what the row table serves with, in addition, one column
 * slice of at most 128 words (8192 bins) and reads of fewer than 65 536 k-mers; results are identical.  Owned, dropped and freed like
 * the row table; reads with a base outside ACGT go to the three-hash twin as there.
 *   rb_dibf_list_table_build: build it now unless a current one exists; max_bytes as for the row table.  A refusal is not an error
 *     (RB_LIST_REFUSED_*): besides the row table's reasons, a filter of more than 8192 bins or 128 words, a filter too dense for
 *     every slot size (DENSITY), or more overflowing rows than the side table holds (SIDE_FULL: 4^k / 512 + 64 rows, or what
 *     rb_set_list_side_capacity says).
 *   rb_dibf_list_table_info / _drop / _download (entries: rows x lines x 64 of uint16_t; side: side_rows x stride words; either may be
 *     null with a count of 0).
 *   rb_engine_set_row_table(RB_ROW_TABLE_LISTS): the list form wherever the geometry serves, else as RB_ROW_TABLE_FORCE.
 *   RB_ROW_TABLE_AUTO prefers the list form when (a) the DENSE row table would lie beyond rb_engine_set_list_min_dense_bytes (default
 *     512 MiB, 2 x the Infinity Cache: below it the dense table is cache-served and lines do not limit it), (b) the launch is one
 *     the row table's rule (a) admits, (c) the batch alone repays the build in 128-byte lines -- items x 2 x k-mers x (L x h - 4) >=
 *     4^k x (L x h + 4), L = lines per block (config 3: 135 000 reads of 360 bp) -- (d) the table fits max_bytes and half of the free
 *     device memory, (e) the stream is not being captured.  Where the list build is refused, AUTO goes on to the row table's rule, and an
 *     engine does not ask again (nor does rb_engine_plan report the list form) for the same bits and max_bytes until
 *     rb_dibf_list_table_build or _drop is called. */
#define RB_ROW_TABLE_LISTS 3
#define RB_LIST_REFUSED_NONE 0
#define RB_LIST_REFUSED_K 1          /* k above 13 */
#define RB_LIST_REFUSED_GEOMETRY 2   /* blocks of 32 words or fewer, of more than 128 words, or more than 8192 bins */
#define RB_LIST_REFUSED_MAX_BYTES 3  /* the table and its side table above max_bytes */
#define RB_LIST_REFUSED_FREE 4       /* the table above half of the free device memory */
#define RB_LIST_REFUSED_ALLOC 5      /* the allocation failed */
#define RB_LIST_REFUSED_CAPTURE 6    /* the call's stream was being captured (engine builds only) */
#define RB_LIST_REFUSED_DENSITY 7    /* more than one sampled row in 1024 overflows even a four-line slot */
#define RB_LIST_REFUSED_SIDE_FULL 8  /* more overflowing rows than the side table holds */
typedef struct rb_list_table_info {
    uint64_t bytes, rows;    /* of the current table's slots; 0: none */
    uint64_t side_bytes;     /* of its side table */
    uint32_t lines;          /* 128-byte lines per slot: 1, 2 or 4 */
    uint32_t side_rows;      /* overflow rows in use */
    uint32_t side_capacity;  /* ... and how many the side table holds */
    uint32_t refused;        /* RB_LIST_REFUSED_*: why the last build did not happen */
    uint32_t builds;         /* tables built for this filter so far */
    uint32_t stride_words;   /* words per row of the side table (the filter's block stride) */
    uint64_t census_rows, census_over[3]; /* rows the last census looked at, and how many of them had more than 64, 128, 256 bits set */
    double build_ms;         /* kernel time of the last build, census included */
    double alloc_s;          /* seconds its allocations took */
} rb_list_table_info;
RB_API int rb_dibf_list_table_build(rb_dibf *f, uint64_t max_bytes);
RB_API int rb_dibf_list_table_drop(rb_dibf *f);
RB_API int rb_dibf_list_table_info(rb_dibf *f, rb_list_table_info *out);
/* The first n_entries 16-bit entries of the table in its CANONICAL form -- per slot the row's bin numbers ascending, 0xFFFF to the end;
 * an overflow slot is 0xFFFE and the two halves of its side-table index -- and the first n_side_words words of the side table.  The
 * device itself keeps the slots in another, private form (ready LDS addresses for the count kernels: csrc/rb_lists.h) that no caller
 * sees: the whole slots that cover the prefix are copied and converted on the host, so a short prefix of a large table stays cheap. */
RB_API int rb_dibf_list_table_download(rb_dibf *f, uint16_t *entries, uint64_t n_entries, uint64_t *side_words, uint64_t n_side_words);
/* the dense-table size from which RB_ROW_TABLE_AUTO prefers the list form (0: always, where the other rules hold) */
RB_API int rb_engine_set_list_min_dense_bytes(rb_engine *e, uint64_t bytes);
/* rows of the side table of list tables built from now on (process-wide; 0: the default, 4^k / 512 + 64) */
RB_API void rb_set_list_side_capacity(uint32_t rows);

/* PAIR TABLE of a resident filter: the lists of a k-mer AND of its reverse complement in one slot of three lines (384 bytes), so that a
 * read's two strands cost three lines per k-mer where the list table's two-line slots cost four.  One slot per N-free k-mer x, indexed by
 * the rank of x itself (every pair is stored twice: 4^k x 384 bytes, 24 GiB at k = 13); ibf_count_pair_lists_kernel ranks the forward
 * strand only and counts into one LDS dword per bin, the low half the forward strand's count and the high half the reverse strand's, one
 * workgroup of four waves per read.  A pair that leaves more than 64 entries behind the first 64 of either list takes a TAIL line of 128
 * bytes in a side array (up to 254 entries in all), one beyond that a pair of dense rows in the side table; the census samples up to 65 536
 * pairs and refuses the table (RB_LIST_REFUSED_DENSITY) where more than one in 32 needs a tail or more than one in 1024 dense rows.
 * Serves what the list table serves, with three hash functions; results are identical.  No strand is skipped and none stops early -- both
 * are fetched together -- so bound pruning changes nothing, and a call with a prune trace keeps the list form.
 *   rb_dibf_pair_table_build / _drop / _info: as the list table's calls.  _download: the first n_entries entries of the CANONICAL form,
 *     256 per slot -- the slot's bins of row(x) ascending, 0xFFFF, its bins of row(rc(x)) ascending, 0xFFFF to entry 252; entries 253 and
 *     254 are the halves of an index and entry 255 is 0xFFFD (a tail slot: the index of its tail line) or 0xFFFE (a dense slot, which lists
 *     nothing: the index of the first of its two rows in the side table), 0xFFFF otherwise -- the first n_tail_dwords dwords of the tail
 *     lines as the device holds them (32 per line; a 16-bit half is 4 x bin, + 1 for a bin of row(rc(x)), or beyond 4 x the bin count:
 *     nothing; first what is left of row(x), then of row(rc(x))), and the first n_side_words words of the side table.
 *   rb_engine_set_row_table(RB_ROW_TABLE_PAIRS): the pair form wherever it serves, else as RB_ROW_TABLE_LISTS.
 *   RB_ROW_TABLE_AUTO takes the pair table instead of the list table when the list rules (a)-(e) hold with the pair table's lines and
 *     bytes, the list table's census on the same sample would choose two lines (a one-line list table already costs two lines per k-mer),
 *     the pair census serves, and the pair table is at least rb_engine_set_pair_min_bytes (default 1 GiB: k <= 10 keeps the list table)
 *     large.  The locate, hits, prefix and resume passes keep reading the list table under their own settings. */
#define RB_ROW_TABLE_PAIRS 4
typedef struct rb_pair_table_info {
    uint64_t bytes, rows;    /* of the current table's slots; 0: none */
    uint64_t side_bytes;     /* of its side table (dense rows) */
    uint64_t tail_bytes;     /* of its tail lines */
    uint32_t lines;          /* 128-byte lines per slot: 3 */
    uint32_t side_rows;      /* dense rows in use (two per dense slot) */
    uint32_t side_capacity;  /* ... and how many the side table holds */
    uint32_t tail_rows;      /* tail lines in use */
    uint32_t tail_capacity;  /* ... and how many the tail array holds */
    uint32_t refused;        /* RB_LIST_REFUSED_*: why the last build did not happen */
    uint32_t builds;         /* tables built for this filter so far */
    uint32_t stride_words;   /* words per row of the side table (the filter's block stride) */
    uint64_t census_rows, census_over[3]; /* pairs the last census looked at; how many need a tail or more, how many dense rows, and how
                                             many have more than 128 bins in row(x) */
    uint64_t census_one_line; /* ... and how many have more than 64 bins in row(x) */
    double build_ms;         /* kernel time of the last build, census included */
    double alloc_s;          /* seconds its allocations took */
} rb_pair_table_info;
RB_API int rb_dibf_pair_table_build(rb_dibf *f, uint64_t max_bytes);
RB_API int rb_dibf_pair_table_drop(rb_dibf *f);
RB_API int rb_dibf_pair_table_info(rb_dibf *f, rb_pair_table_info *out);
RB_API int rb_dibf_pair_table_download(rb_dibf *f, uint16_t *entries, uint64_t n_entries, uint32_t *tail_dwords, uint64_t n_tail_dwords,
                                       uint64_t *side_words, uint64_t n_side_words);
RB_API int rb_engine_set_pair_min_bytes(rb_engine *e, uint64_t bytes);
/* dense rows and tail lines of pair tables built from now on (process-wide; 0: the defaults, 2 x (4^k / 512 + 64) and 4^k / 16 + 64) */
RB_API void rb_set_pair_side_capacity(uint32_t rows, uint32_t tails);

/* WIDE LIST TABLE of a resident filter: the list table's idea for filters of 8193 to 32 256 bins (blocks of up to 504 words), which the
 * list table refuses (RB_LIST_REFUSED_GEOMETRY) -- GRCh38 at the default fragment size has about 31 000.  A second object beside the
 * list table with calls and a setting of its own, off by default.  Per N-free k-mer one slot of 4, 6 or 8 lines of 128 bytes with the
 * row's bin numbers as 16-bit entries, chosen by the list table's census rule (the smallest slot that at most one in 1024 of up to
 * 65 536 sampled rows overflows; census_over counts rows with more than 256, 384 and 512 set bits); overflowing rows keep a dense row in
 * a side table.  ibf_count_wide_lists_kernel gathers that slot instead of h blocks of up to 32 lines each, one workgroup of four waves
 * per read sharing one array of 16-bit counters in LDS; k-mers with a base outside ACGT are counted in the same kernel from the
 * filter's own table.  Serves h = 3, k <= 13, reads of fewer than 65 536 k-mers; results are identical to the plain kernel's.
 *   rb_dibf_wide_list_table_build / _drop / _info / _download: as the list table's calls; refusals are RB_LIST_REFUSED_* (GEOMETRY: not
 *     8193 to 32 256 bins, or h != 3; DENSITY: too dense even for eight lines).  _download returns the canonical form (rows x lines x 64
 *     entries of uint16_t: bins ascending, then 0xFFFF; an overflow slot is 0xFFFE and the two halves of its side-table index).
 *   rb_engine_set_wide_lists: RB_PASS_LISTS_OFF (default: nothing changes for any call) / _CURRENT (a filter's wide table is used where
 *     it has a current one; none is built) / _BUILD (a classify call builds it when the batch alone repays the build in 128-byte lines --
 *     items x 2 x k-mers x (L x h - 8) >= 4^k x (L x h + 8), L = lines per block -- the table fits the max_bytes of
 *     rb_engine_set_row_table and half of the free device memory, and the stream is not being captured; a refusal is remembered for the
 *     bits and max_bytes it was given for, and means the plain kernel).  Any other value is RB_ERR_INVALID_ARG.  Taken by classify calls
 *     alone, and only by launches that row_policy's rule (a) admits -- no latency form, fused micro-batch, early-decision mode, column
 *     shard -- with no prune trace asked for; locate and hits, and the prefix pass, read the wide table under settings of their own (below);
 *     spans and resume do not read it.  rb_engine_plan names ibf_count_wide_lists_kernel where a call would take it.
 *   rb_engine_set_wide_pass_lists: the same three values for the locate and hits calls of the boundary header, off by default and a
 *     setting of its OWN: rb_engine_set_wide_lists does not reach locate or hits, this setting does not reach classify, and
 *     rb_engine_set_pass_lists does not reach filters beyond 8192 bins.  Decided per filter and per call (an engine may mix wide-served,
 *     list-served and plain-served filters in one call): the mode allows it, the geometry serves the call's max_len (h = 3, k <= 13,
 *     fewer than 65 536 k-mers per strand), the engine is no column shard, the stream is not being captured, and the filter has a wide
 *     table of the present version of its bits -- under _BUILD built by the call under the rules a classify call has (the repay
 *     inequality with this call's items and max_len, max_bytes, half of the free memory, remembered refusals); a refusal means the plain
 *     form, never an error.  ibf_locate_wide_lists_kernel / ibf_hits_wide_lists_kernel then serve the items that are RB_OK -- whatever
 *     their bases: a k-mer with an N is counted in the kernel -- one workgroup of four waves per item, both strands counted in full, and
 *     the plain kernels the others; every output is the plain form's, byte for byte.  Any other value is RB_ERR_INVALID_ARG.
 *   rb_engine_wide_pass_lines: *lines_out = 4, 6 or 8 -- the slot size a locate or hits call on items of at most max_len bases would take
 *     for this filter as things stand -- or 0: the plain (or the list) form.  Host arithmetic only; nothing is built or dropped, so under
 *     _BUILD it reports the table once it stands.  rb_pass_plan is unchanged, and its list_lines stays 0 for these filters.
 *   rb_engine_set_wide_prefix_lists: the same three values for the prefix calls of the boundary header, off by
 *     default and a setting of its OWN: rb_engine_set_prefix_lists, rb_engine_set_wide_pass_lists and rb_engine_set_wide_lists do not
 *     reach it, and it reaches none of them.  Decided per filter and per call by rb_engine_set_wide_pass_lists's rules with this mode
 *     and the call's bound min(max_len, last checkpoint): at most 65 535 k-mers per strand at the last checkpoint.
 *     ibf_prefix_wide_lists_kernel then serves the items whose status so far is RB_OK and whose first min(len, last checkpoint) bases lie
 *     within the bound -- any length, and whatever their bases -- one workgroup of four waves per item, and the plain kernel the
 *     others; a filter served by neither list form runs the plain form in the same call.  Every output is the plain form's, byte for
 *     byte.  Any other value is RB_ERR_INVALID_ARG.
 *   rb_engine_wide_prefix_lines: *lines_out = 4, 6 or 8 -- the slot size a prefix call on items of at most max_len bases with that last
 *     checkpoint would take for this filter as things stand -- or 0.  Host arithmetic only; nothing is built or dropped.
 *     rb_prefix_plan_info is unchanged, and its list_lines stays 0 for these filters.
 *   rb_engine_wide_prefix_lists_items: rb_engine_prefix_lists_items for this form, counters of its own: the items the wide form took and
 *     left since the last reset, over the calls in which some filter was wide-served.  Waits for the engine's stream. */
typedef struct rb_wide_list_table_info {
    uint64_t bytes, rows;    /* of the current table's slots; 0: none */
    uint64_t side_bytes;     /* of its side table */
    uint32_t lines;          /* 128-byte lines per slot: 4, 6 or 8 */
    uint32_t side_rows;      /* overflow rows in use */
    uint32_t side_capacity;  /* ... and how many the side table holds */
    uint32_t refused;        /* RB_LIST_REFUSED_*: why the last build did not happen */
    uint32_t builds;         /* tables built for this filter so far */
    uint32_t stride_words;   /* words per row of the side table (the filter's block stride) */
    uint64_t census_rows, census_over[3]; /* rows the last census looked at, and how many of them had more than 256, 384, 512 bits set */
    double build_ms;         /* kernel time of the last build, census included */
    double alloc_s;          /* seconds its allocations took */
} rb_wide_list_table_info;
RB_API int rb_dibf_wide_list_table_build(rb_dibf *f, uint64_t max_bytes);
RB_API int rb_dibf_wide_list_table_drop(rb_dibf *f);
RB_API int rb_dibf_wide_list_table_info(rb_dibf *f, rb_wide_list_table_info *out);
RB_API int rb_dibf_wide_list_table_download(rb_dibf *f, uint16_t *entries, uint64_t n_entries, uint64_t *side_words, uint64_t n_side_words);
RB_API int rb_engine_set_wide_lists(rb_engine *e, int mode);
RB_API int rb_engine_set_wide_pass_lists(rb_engine *e, int mode);
RB_API int rb_engine_wide_pass_lines(rb_engine *e, size_t filter_index, uint32_t max_len, uint32_t *lines_out);
RB_API int rb_engine_set_wide_prefix_lists(rb_engine *e, int mode);
RB_API int rb_engine_wide_prefix_lines(rb_engine *e, size_t filter_index, uint32_t max_len, uint32_t last_checkpoint, uint32_t *lines_out);
RB_API int rb_engine_wide_prefix_lists_items(rb_engine *e, uint64_t *listed, uint64_t *plain, int reset);
/* rows of the side table of wide list tables built from now on (process-wide; 0: the default, 4^k / 512 + 64) */
RB_API void rb_set_wide_list_side_capacity(uint32_t rows);

/* How the eight XCDs walk the slices of a phased table (each has an L2 of its own, so each reloads every slice): bit 0 of `mode` -- at
 * any time every XCD works on a different slice (slice = (window + XCD number) mod slices); bit 1 -- the XCDs' windows start an eighth
 * of a window apart, so that they refill their L2s one after the other instead of all in the same instant.  0 (default): one clock, one
 * slice for the whole chip.  Results are identical. */
RB_API int rb_engine_set_phase_xcd_skew(rb_engine *e, uint32_t mode);

/* Host batches above 8 MB of read bytes cross PCIe in slices of about slice_bytes (default 32 MiB): slice i+1 is
 * copied on a copy stream while slice i is counted.  0 = one slice (no overlap).  Results are identical. */
RB_API int rb_engine_set_host_slice_bytes(rb_engine *e, uint64_t slice_bytes);

/* Kernel timing for the roofline figure: when enabled every rb_classify_batch* call brackets its
 * count kernels (K1, all filters) with a hipEvent pair recorded on the launch stream, without
 * synchronising.  rb_engine_kernel_time waits for the recorded pairs, returns their summed elapsed
 * time and the number of calls, and resets the accumulation. */
RB_API int rb_engine_set_timing(rb_engine *e, int enabled);
RB_API int rb_engine_kernel_time(rb_engine *e, double *total_ms, uint64_t *n_calls);

/* Measurement aid, NOT part of the classify path (no reference counterpart): what this device delivers for the access pattern
 * of the wide count kernels -- random gathers of whole rows of row_bytes (128, 1024 or 4096) from the first table_bytes (0 = all)
 * of the filter's own table in HBM, 16 bytes per lane, loads_in_flight (12 or 24) wave instructions issued back to back,
 * nontemporal as rb_engine_set_nt_threshold would choose, no compute attached; runs of about target_ms (0 = 200), best of three.
 * bench.py calls it on the filter it has just timed so that `roofline` carries a same-box, same-run reference point
 * (`read_peak_probe`) beside the 8 TB/s spec figure. */
RB_API int rb_dibf_probe_read_peak(rb_dibf *f, uint64_t table_bytes, uint32_t row_bytes, int nontemporal, uint32_t loads_in_flight,
                                   double target_ms, double *gbps_out, double *ms_out);

#ifdef __cplusplus
}
#endif
#endif /* READBOUNCER_AMD_TUNING_H_ */

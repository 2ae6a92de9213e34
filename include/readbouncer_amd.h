/*
 * readbouncer_amd.h -- C ABI of the MI355X-native IBF read-classification engine.
 *
 * This is the drop-in boundary for ONE path of ReadBouncer: src/IBF classify
 * (k-mer extraction -> h-fold hash -> IBF bulk-contains -> per-bin counting ->
 * error-model threshold -> unblock/keep decision).  The reference exposes that path as
 * a C++ static library whose types leak SeqAn templates (src/IBF/CMakeLists.txt:5,
 * src/IBF/IBF.hpp:92-94), so there is no binary FFI to bind; every entry point below
 * names the reference interface it replaces.  INTEGRATION.md shows the reference-side
 * shim.  include/readbouncer_amd.hpp is the C++ mirror (interleave::Read, IBF, IBFMeta,
 * ClassifyConfig, exceptions) over these calls.
 *
 * All compute entry points need a gfx950 device and fail with RB_ERR_NO_DEVICE /
 * RB_ERR_HIP otherwise -- there is no CPU fallback.  Plain pointers and sizes only.
 */
#ifndef READBOUNCER_AMD_H_
#define READBOUNCER_AMD_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RB_API __attribute__((visibility("default")))

/* ---- status codes (the reference throws; src/IBF/IBFExceptions.hpp) ------------------ */
enum rb_status {
    RB_OK = 0,
    RB_ERR_NULL_FILTER = 1,  /* NullFilterException      IBFExceptions.hpp:178 */
    RB_ERR_SHORT_READ = 2,   /* ShortReadException       IBFExceptions.hpp:96  */
    RB_ERR_COUNT_KMER = 3,   /* CountKmerException       IBFExceptions.hpp:123 */
    RB_ERR_MISSING_FILE = 4, /* MissingIBFFileException  IBFExceptions.hpp:317 */
    RB_ERR_PARSE_IBF = 5,    /* ParseIBFFileException    IBFExceptions.hpp:344 */
    RB_ERR_BAD_CHUNK = 6,    /* chunk start beyond read end (classify.hpp:264-273, undefined there) */
    RB_ERR_STORE = 7,        /* StoreFilterException */
    RB_ERR_INVALID_ARG = 8,
    RB_ERR_UNSUPPORTED = 9,  /* filter geometry outside what the kernels handle */
    RB_ERR_NO_DEVICE = 10,   /* no gfx950 GPU visible: the engine has no CPU fallback */
    RB_ERR_HIP = 11,         /* a HIP runtime call failed, see rb_last_error() */
    RB_ERR_NOMEM = 12
};

RB_API const char *rb_status_string(int status);
/* thread-local text of the last failure on the calling thread */
RB_API const char *rb_last_error(void);
RB_API const char *rb_version(void);
/* number of visible HIP devices, or a negative rb_status */
RB_API int rb_device_count(void);

/* ---- filter geometry ------------------------------------------------------------------
 * Mirrors the public members of interleave::TIbf =
 * seqan::BinningDirectory<InterleavedBloomFilter, BDConfig<Dna5,Normal,Uncompressed>>
 * that the reference reads (noOfBins: IBFClassify.cpp:27,58; kmerSize: :102,154,192,248;
 * getNumberOfBins/getKmerSize: IBFBuild.cpp:380-381). */
typedef struct rb_ibf_info {
    uint64_t n_bins;     /* noOfBins */
    uint64_t n_hash;     /* noOfHashFunc */
    uint64_t kmer_size;  /* kmerSize */
    uint64_t n_bits;     /* noOfBits, without the 256 metadata bits */
    uint64_t bin_width;  /* 64-bit words per block = ceil(n_bins/64) */
    uint64_t n_blocks;   /* n_bits / (64*bin_width) */
    uint64_t n_words;    /* payload words incl. metadata = (n_bits+256+63)/64 */
} rb_ibf_info;

/* ---- host-side filter image (.ibf file <-> memory) ------------------------------------ */
typedef struct rb_ibf rb_ibf;

/* IBF::load_filter -> seqan::retrieve (src/IBF/IBFBuild.cpp:329-396).
 * RB_ERR_MISSING_FILE if the file cannot be opened, RB_ERR_PARSE_IBF if it is not an IBF. */
RB_API int rb_ibf_open(const char *path, rb_ibf **out);
/* TIbf(bins, hash_functions, kmer_size, filter_size_bits) (src/IBF/IBFBuild.cpp:465): zeroed */
RB_API int rb_ibf_create(uint64_t n_bins, uint64_t n_hash, uint64_t kmer_size, uint64_t n_bits, rb_ibf **out);
/* seqan::store (src/IBF/IBFBuild.cpp:505,307) */
RB_API int rb_ibf_store(const rb_ibf *f, const char *path);
RB_API int rb_ibf_get_info(const rb_ibf *f, rb_ibf_info *info);
/* payload words (n_words of them), owned by the handle */
RB_API uint64_t *rb_ibf_words(rb_ibf *f);
RB_API void rb_ibf_close(rb_ibf *f);
/* ConfigReader::filterException (src/config/configReader.cpp:210-224): 1 = IBF file, 0 = not */
RB_API int rb_is_ibf_file(const char *path);

/* ---- error model (host, double) -------------------------------------------------------
 * calculateCI / NormalCDFInverse (src/IBF/IBF.hpp:320-338, 284-308) and the threshold
 * expression of count_matches (src/IBF/IBFClassify.cpp:154-162), returned as the
 * uint16_t that max_matches receives (negative int16 thresholds wrap). */
RB_API int rb_calculate_ci(double error_rate, uint8_t kmer_size, uint32_t readlen, double significance,
                           uint16_t *low, uint16_t *high);
RB_API uint16_t rb_threshold(uint64_t readlen, uint64_t kmer_size, double error_rate, double significance);

/* ---- build-side helpers (host) --------------------------------------------------------- */
/* IBF::calculate_filter_size_bits (src/IBF/IBFBuild.cpp:404-413) */
RB_API uint64_t rb_calculate_filter_size_bits(uint64_t fragment_length, uint64_t kmer_size,
                                              uint64_t hash_functions, double max_fp, uint64_t n_bins);
/* IBF::cutOutNNNs + concatenation (src/IBF/IBFBuild.cpp:81-88,112-132); out holds >= len bytes */
RB_API size_t rb_cut_out_nnns(const char *seq, size_t len, char *out);
/* fragment loop of add_sequences_to_filter (src/IBF/IBFBuild.cpp:165-204): fills
 * starts/ends (capacity cap) and returns the number of fragments of a sequence of length len */
RB_API size_t rb_fragment_bounds(uint64_t len, uint64_t fragment_length, uint64_t kmer_size,
                                 uint64_t overlap_length, uint64_t *starts, uint64_t *ends, size_t cap);

/* ---- device-resident filter (the IBF in HBM) -------------------------------------------
 * Layout in HBM: the reference's block-major bit matrix with every block starting on a boundary that suits the
 * memory system -- block b at word b*stride, stride >= bin_width (equal when bin_width is a multiple of 16 words, i.e.
 * the .ibf payload is then uploaded verbatim; otherwise blocks are padded to the next power of two / multiple of
 * 128 bytes).  Bin j of block b is bit b*64*stride + j.  Upload, download, build and resize convert; the .ibf file
 * format never changes. */
typedef struct rb_dibf rb_dibf;

RB_API int rb_dibf_create(int device, uint64_t n_bins, uint64_t n_hash, uint64_t kmer_size, uint64_t n_bits,
                          rb_dibf **out);
RB_API int rb_dibf_upload(int device, const rb_ibf *host, rb_dibf **out);
/* load_filter straight into HBM, streamed through pinned staging (no full host copy) */
RB_API int rb_dibf_open(int device, const char *path, rb_dibf **out);
RB_API int rb_dibf_download(const rb_dibf *f, rb_ibf **out);
/* replica of a resident filter on another GPU (or the same one), copied device to device -- over xGMI when the pair
 * has peer access -- in its HBM layout: no host image, no conversion */
RB_API int rb_dibf_clone_to(const rb_dibf *src, int device, rb_dibf **out);
/* the same, reporting how the copy travelled: *used_peer = 1 when the destination mapped the source (peer access, xGMI
 * between two GPUs of a node), 0 for the runtime's staged path or a same-device copy; *seconds = wall time of the copy */
RB_API int rb_dibf_clone_to_ex(const rb_dibf *src, int device, rb_dibf **out, int *used_peer, double *seconds);
RB_API int rb_dibf_get_info(const rb_dibf *f, rb_ibf_info *info);
/* The device image itself.  Engines that keep a merged copy of several filters (rb_engine_set_merge) notice changes made through
 * rb_dibf_insert / rb_dibf_add_sequence / rb_dibf_fill_synth by themselves; a caller that WRITES through this pointer calls
 * rb_dibf_touch afterwards (with its writes complete), or merged copies keep serving the old bits. */
RB_API void *rb_dibf_device_words(rb_dibf *f);
RB_API int rb_dibf_touch(rb_dibf *f);
/* words between consecutive blocks of the device image (see above) */
RB_API uint64_t rb_dibf_device_stride(const rb_dibf *f);
RB_API int rb_dibf_device(const rb_dibf *f);
RB_API void rb_dibf_free(rb_dibf *f);
/* resizeBins of IBF::update_filter (src/IBF/IBFBuild.cpp:274): same blocks and hash positions, every block widened
 * to ceil(new_bins/64) words, new bins empty, noOfBits = noOfBlocks * new block size.  Returns a new filter. */
RB_API int rb_dibf_resize_bins(const rb_dibf *f, uint64_t new_bins, rb_dibf **out);
/* ---- assemble: a new resident filter from bins of others (select, reorder, drop, merge, join) ---------
 * The reference only appends (IBF::update_filter, src/IBF/IBFBuild.cpp:223-321); everything else is a rebuild from the FASTA.
 * Every bin of the new filter is the OR of a list of (filter, bin) pairs of resident filters that share noOfBlocks, noOfHashFunc
 * and kmerSize -- a block number depends on the k-mer, the hash number and noOfBlocks only, so the result is bit for bit what
 * the builder writes when those fragments are inserted into those bins at that block count (the argument of resizeBins):
 *   out bin j = OR of srcs[refs[i].filter] bin refs[i].bin for i in [offsets[j], offsets[j+1]); an empty list = an empty bin
 * One ref per list selects, reorders or drops; several merge fragments into coarser bins; refs into several sources join
 * filters.  A ref may repeat.  The result is a fresh filter on the sources' device with noOfBins = n_out_bins and noOfBits =
 * noOfBlocks * ceil(n_out_bins / 64) * 64 (as rb_dibf_resize_bins makes it); the sources are not written and engines that
 * hold them see no change.  The plan is vetted on the host before anything is launched -- RB_ERR_INVALID_ARG, with
 * rb_last_error() naming the out bin or source at fault, for: a null argument, n_srcs of 0 or above
 * RB_ASSEMBLE_MAX_SOURCES, n_out_bins of 0, sources on different devices or of different noOfBlocks / noOfHashFunc / kmerSize,
 * offsets[0] != 0 or a descending offset, a ref whose filter >= n_srcs or whose bin is at or beyond that source's noOfBins.
 * RB_ERR_UNSUPPORTED: 2^32 refs or more, or 4 096 consecutive out bins whose lists together span more than 60 KiB of one
 * block of the sources (some 490 000 source bins). */
#define RB_ASSEMBLE_MAX_SOURCES 8
#define RB_BIN_NONE UINT64_MAX
typedef struct rb_bin_ref { uint32_t filter; uint32_t bin; } rb_bin_ref;   /* 8 bytes */
RB_API int rb_dibf_assemble(const rb_dibf *const *srcs, size_t n_srcs, const uint64_t *offsets, const rb_bin_ref *refs,
                            uint64_t n_out_bins, rb_dibf **out);
/* the one-source, one-ref-per-bin case: out bin j = src bin bins[j], RB_BIN_NONE = empty */
RB_API int rb_dibf_select_bins(const rb_dibf *src, const uint64_t *bins, uint64_t n_out_bins, rb_dibf **out);

/* seqan::insertKmer for a batch of fragments (src/IBF/IBFBuild.cpp:189-190) on the GPU:
 * fragment i = seq[starts[i], ends[i]) goes to bin bins[i]. seq is host ASCII. */
RB_API int rb_dibf_insert(rb_dibf *f, const char *seq, size_t len, const uint64_t *starts,
                          const uint64_t *ends, const uint64_t *bins, size_t n_fragments);
/* one reference sequence through the reference fragmenter; *next_bin = first_bin + #fragments */
RB_API int rb_dibf_add_sequence(rb_dibf *f, const char *seq, size_t len, uint64_t fragment_length,
                                uint64_t overlap_length, uint64_t first_bin, uint64_t *next_bin);

/* First-contact check for a filter that came from somewhere else (a .ibf written by the reference).  The hash constants
 * and the bit layout of the IBF live in a dependency that is not part of the reference tree (ibf_spec.h), so a filter
 * file is the first place where a wrong constant would show: re-insert the reference sequences the file was built from
 * (the reference fragmenter + insertKmer, src/IBF/IBFBuild.cpp:165-204,190) into an EMPTY filter of the same geometry
 * and compare.  With matching constants the rebuilt bits are a subset of the file's bits: new_bits == 0 (SURVEY 7:
 * "re-inserting a known reference must set no new bits") and rebuilt_bits / file_bits says how much of the file the
 * given sequences explain; under a different seed, shift, k-mer encoding or block order about (1 - load) of the
 * rebuilt bits land on clear positions. */
typedef struct rb_ibf_compare {
    uint64_t file_bits;     /* bits set in the block payload of the filter under test */
    uint64_t rebuilt_bits;  /* bits the re-insertion sets */
    uint64_t new_bits;      /* of those, bits that are clear in the filter under test -- must be 0 */
    uint64_t payload_bits;  /* noOfBlocks * noOfBins: the positions insertKmer can reach */
} rb_ibf_compare;
RB_API int rb_dibf_compare(const rb_dibf *file_filter, const rb_dibf *rebuilt, rb_ibf_compare *out);

/* ---- how full is each bin, and what false-positive rate does that mean -------------------------------
 * The reference sizes a filter for max_fp = 0.01 (src/IBF/IBFConfig.hpp:77; calculate_filter_size_bits,
 * src/IBF/IBFBuild.cpp:404-413) under the assumption that every bin holds fragment_size - k + 1 k-mers, and reports bins only
 * by number (print_build_stats / print_load_stats, src/IBF/IBF.hpp:340-341); nothing holds a filter that was updated
 * (update_filter, IBFBuild.cpp:223-321) or written elsewhere to that assumption.  One streaming pass over the resident table
 * counts, per bin, the blocks whose bit is set:
 *   out[j] = #{ b < noOfBlocks : bit (b, j) set },  j < noOfBins
 * -- the block payload only (the positions rb_ibf_compare::payload_bits names): padding words of the HBM layout and bits at or
 * beyond noOfBins are never counted.  It reads the filter's own table (never an engine's merged copy), needs no engine and
 * touches no engine's workspace.  Host form: out_bits is host memory, u64 [n_bins]. */
RB_API int rb_dibf_bin_occupancy(const rb_dibf *f, uint64_t *out_bits);
/* Device form of the same count (what max_fp, src/IBF/IBFConfig.hpp:77, is to be held against): d_out_bits is a device pointer (u64 [n_bins]) on the filter's device; it is zeroed and filled asynchronously on
 * `stream` (a hipStream_t).  stream == NULL: the pass runs on a stream of its own, which is synchronised before returning -- a non-blocking stream, NOT ordered
 * after work the caller has pending on the default stream or anywhere else: such work must have completed before the call.  The
 * filter's bits must be complete on `stream` (work that writes them on another stream -- rb_dibf_insert and the other builders
 * synchronise by themselves -- has to be ordered before this call by the caller); d_out_bits may be read once `stream` has passed. */
RB_API int rb_dibf_bin_occupancy_device(const rb_dibf *f, void *d_out_bits, void *stream);

typedef struct rb_bin_occupancy_summary {
    uint64_t n_bins, n_blocks, n_hash;
    uint64_t bits_total;          /* == rb_ibf_compare::file_bits of the same filter */
    uint64_t empty_bins;          /* bins with no bit set */
    uint64_t max_bits;  uint64_t max_bin;     /* the fullest bin, lowest index on a tie */
    uint64_t min_bits;  uint64_t min_bin;     /* the emptiest NON-empty bin, lowest index on a tie; 0 / 0 when all are empty */
    double   mean_load, max_load; /* bits / n_blocks; the mean over non-empty bins */
    double   mean_fpr,  max_fpr;  /* load ^ n_hash; the mean over non-empty bins */
    uint64_t bins_over_max_fp;    /* bins with fpr > max_fp */
} rb_bin_occupancy_summary;
/* pure host arithmetic on a count vector: works without a GPU.  max_fp: the reference's default is 0.01 (IBFConfig.hpp:77).
 * RB_ERR_INVALID_ARG when n_blocks or n_hash is 0. */
RB_API int rb_bin_occupancy_summarize(const uint64_t *bits, uint64_t n_bins, uint64_t n_blocks, uint64_t n_hash,
                                      double max_fp, rb_bin_occupancy_summary *out);
/* per bin, the three derived figures (any pointer may be NULL): load = bits/n_blocks, fpr = load^h,
 * est_kmers = -(n_blocks / h) * ln(1 - load)  (distinct k-mers the bin holds, the usual Bloom estimate -- the inverse of the
 * sizing formula of IBFBuild.cpp:404-413; +inf at load 1) */
RB_API int rb_bin_occupancy_derive(const uint64_t *bits, uint64_t n_bins, uint64_t n_blocks, uint64_t n_hash,
                                   double *load, double *fpr, double *est_kmers);
/* Text of what the last rb_ibf_open / rb_dibf_open / rb_is_ibf_file on this thread found odd about a file that still
 * parsed (non-zero spare metadata word, a hash-function count or k-mer size the reference never writes, tail bits set
 * beyond the last block); empty string when there was nothing. */
RB_API const char *rb_last_warning(void);

/* ---- classification engine --------------------------------------------------------------
 * One engine per GPU.  It borrows the filters (like the reference's
 * std::vector<IBFMeta>& DepletionFilters / TargetFilters, classify.hpp:142,
 * adaptive_sampling.hpp:214) and owns streams, threshold tables and workspaces. */
typedef struct rb_engine rb_engine;

RB_API int rb_engine_create(int device, rb_dibf *const *deplete, size_t n_deplete,
                            rb_dibf *const *target, size_t n_target, rb_engine **out);
RB_API void rb_engine_destroy(rb_engine *e);

enum rb_mode {
    /* check_unblock (src/main/adaptive_sampling.hpp:35-113): decision 0 wait / 1 unblock / 2 stop_receiving */
    RB_MODE_CHECK_UNBLOCK = 0,
    /* one chunk of classify_reads (src/main/classify.hpp:275-292, 58-111): decision 1 = classified */
    RB_MODE_CLASSIFY_CHUNK = 1,
    /* Read::classify(std::vector<TIbf>&) -> find_matches / select_matches (src/IBF/IBFClassify.cpp:181-226, 81-128,
     * 16-38): decision 1 = some filter of the list (deplete entries first, then target entries) holds a bin whose
     * forward or reverse count is >= the uint16_t threshold -- with a threshold of 0 that is every read, matches or
     * not; status RB_ERR_SHORT_READ when the read is shorter than the first filter's k */
    RB_MODE_CLASSIFY_ANY = 2
};

/* Batch form of Read::classify x3 + the decision, inputs and outputs in HOST memory.
 *   seqs/offsets/lens : read i is the ASCII bytes seqs[offsets[i] .. offsets[i]+lens[i])
 *                       ((seqan::Dna5String) conversion is done on the device)
 *   error_rate        : ClassifyConfig::error_rate, by value (the reference mutates a shared
 *                       config, adaptive_sampling.hpp:55-59); significance: 0.95 in the reference
 *   out_maxcount      : [n_reads x (n_deplete+n_target)] raw max k-mer count over bins and both
 *                       strands per filter, deplete filters first (before thresholding); may be NULL
 *   out_best_target   : [n_reads] Read::classify(TargetFilters) -> index or -1; may be NULL
 *   out_decision      : [n_reads] per rb_mode
 *   out_status        : [n_reads] RB_OK / RB_ERR_SHORT_READ / RB_ERR_NULL_FILTER per read --
 *                       one bad read never aborts the batch (classify.hpp:306-316)          */
RB_API int rb_classify_batch(rb_engine *e, const char *seqs, const uint64_t *offsets, const uint32_t *lens,
                             size_t n_reads, double error_rate, double significance, int mode,
                             uint16_t *out_maxcount, int32_t *out_best_target, uint8_t *out_decision,
                             uint8_t *out_status);

/* Pointer-array form of rb_classify_batch: read i = seq_ptrs[i][0 .. lens[i]) (one buffer per read, as a basecaller
 * hands them over; the reference's RTPair carries one std::string per read, src/interfaces/ont_read.hpp:24-61). */
RB_API int rb_classify_batch_ptrs(rb_engine *e, const char *const *seq_ptrs, const uint32_t *lens, size_t n_reads,
                                  double error_rate, double significance, int mode, uint16_t *out_maxcount,
                                  int32_t *out_best_target, uint8_t *out_decision, uint8_t *out_status);

/* Page-locked host memory for read buffers handed to rb_classify_batch: the copy to the GPU is then a plain DMA
 * (pageable buffers are pinned on the fly by the runtime, which costs more than the copy itself and serialises with
 * threads that page-fault on a memory-mapped read file).  Optional: any host pointer works. */
RB_API int rb_host_alloc(size_t bytes, void **out);
RB_API void rb_host_free(void *p);

/* Same with every buffer already resident in HBM (device pointers) and asynchronous on
 * `stream` (a hipStream_t, NULL = the engine's own stream, which is then synchronised
 * before returning).  max_len = an upper bound of lens[]: a longer read gets status RB_ERR_INVALID_ARG, and its row of
 * d_maxcount is then UNDEFINED (the narrow-filter kernels are built per max_len and write 0 for it) -- callers that consume raw
 * maxima without the decision stage (the bin-sharded layout) must not understate it.  The inputs must be complete on `stream`
 * (work that produces them on another stream has to be ordered before this call by the caller).  An engine's
 * workspaces (partial maxima, threshold tables, arrival counters) are per engine: calls on one engine may come from
 * several threads, but their GPU work must be ordered -- use one stream per engine, or order the streams with events;
 * for independent streams create one engine per stream (filters are shared, not copied). */
RB_API int rb_classify_batch_device(rb_engine *e, const void *d_seqs, const void *d_offsets, const void *d_lens,
                                    size_t n_reads, uint32_t max_len, double error_rate, double significance,
                                    int mode, void *d_maxcount, void *d_best_target, void *d_decision,
                                    void *d_status, void *stream);

/* Descriptor form of the device entry point: packed reads and on-GPU chunking.
 *   d_nmask != NULL : d_seqs holds 2 bits per base (A0 C1 G2 T3; base i of a read in bits 2*(i&3) of byte i>>2 of the
 *                     read's payload, d_offsets[] = byte offset of that payload) and d_nmask an N bitmap (bit i&7 of
 *                     byte i>>3, d_nmask_offsets[]); a flagged base is hashed as Dna5 ordinal 4 exactly like an
 *                     'N' in ASCII input.  rb_pack_reads builds both arrays on the host.
 *   chunk_start / chunk_length : classify bases [chunk_start, min(chunk_start+chunk_length, len)) of every read
 *                     (chunk_length 0 = to the end) -- chunk i of classify_reads is chunk_start = i*chunk_length
 *                     (src/main/classify.hpp:264-271); reads uploaded once serve every chunk iteration.  A chunk that
 *                     starts beyond the read's end gets status RB_ERR_BAD_CHUNK.
 *   d_read_ids      : optional u32[n_items]: work item j classifies read d_read_ids[j] (the reads still unclassified
 *                     after the previous chunk); outputs are indexed by work item.  d_lens/d_offsets stay per read. */
typedef struct rb_batch_desc {
    const void *d_seqs;
    const void *d_offsets;        /* u64 per read */
    const void *d_lens;           /* u32 per read: full read lengths */
    size_t n_items;               /* work items (= reads unless d_read_ids is given) */
    uint32_t max_len;             /* upper bound of the full read lengths */
    const void *d_nmask;          /* NULL = ASCII input */
    const void *d_nmask_offsets;  /* u64 per read */
    uint32_t chunk_start;
    uint32_t chunk_length;
    const void *d_read_ids;       /* NULL = identity */
} rb_batch_desc;
RB_API int rb_classify_batch_device_ex(rb_engine *e, const rb_batch_desc *desc, double error_rate, double significance,
                                       int mode, void *d_maxcount, void *d_best_target, void *d_decision,
                                       void *d_status, void *stream);
/* host helper for the packed form; call once with packed == NULL to obtain the sizes and offsets */
RB_API int rb_pack_reads(const char *seqs, const uint64_t *offsets, const uint32_t *lens, size_t n_reads, uint8_t *packed,
                         uint64_t *packed_offsets, uint8_t *nmask, uint64_t *nmask_offsets, uint64_t *packed_bytes,
                         uint64_t *nmask_bytes);

/* ---- locate: WHICH bin and strand a read matched, and how many bins hit ---------------------------
 * The reference has no such call.  It computes everything this reports and throws it away: count_matches counts both
 * strands per bin (src/IBF/IBFClassify.cpp:149-150), max_matches keeps only the maximum over bins (:48-71) and
 * select_matches leaves at the first bin with fwd >= t or rev >= t (:16-38).  A bin is a fragment_size stretch of a
 * reference record (src/IBF/IBFBuild.cpp:165-204), so the bin number is a locus.  An opt-in second pass over the work
 * items the caller selects; it always counts in full, whatever the engine's pruning / early-decision / merge / phased
 * settings are, and changes nothing rb_classify_batch* returns.  It reads each filter's own table unless the engine was told
 * to serve it from a filter's list table (rb_engine_set_pass_lists, readbouncer_amd_tuning.h; off by default): the results are
 * defined, and come out, the same either way.  Per (work item, filter), deplete filters first:
 *   max_count   u16  M = max over bins b of max(fwd[b], rev[b]) -- the out_maxcount of rb_classify_batch for the same read
 *                    (uint16_t counts: they wrap at 65 536 as seqan::count's vectors do)
 *   best_bin    i32  the LOWEST bin b with max(fwd[b], rev[b]) == M; -1 when M == 0 or the item's status is not RB_OK
 *   best_strand u8   0 when fwd[best_bin] == M, else 1 (forward wins a tie); 0 when best_bin == -1
 *   hit_bins    u32  bins with fwd[b] >= t or rev[b] >= t, t = rb_threshold(length, k, error_rate, significance) as the
 *                    decision stage reads it (t == 0 counts every bin, a wrapped t of 65 5xx none); 0 when status != RB_OK
 * and per work item
 *   status      u8   RB_OK, RB_ERR_BAD_CHUNK (chunk start beyond the read), RB_ERR_INVALID_ARG (longer than max_len),
 *                    RB_ERR_SHORT_READ (shorter than the k of some filter of the engine)
 * fwd / rev follow the engine's N rule (rb_engine_set_revcomp_of_n).  A column-sharded engine (rb_engine_set_column_shard,
 * world > 1) refuses with RB_ERR_INVALID_ARG: a shard sees only its own bins. */
typedef struct rb_locate_out { /* any member may be NULL, not all */
    void *max_count;   /* u16 [n_items x n_filters] */
    void *best_bin;    /* i32 [n_items x n_filters] */
    void *best_strand; /* u8  [n_items x n_filters] */
    void *hit_bins;    /* u32 [n_items x n_filters] */
    void *status;      /* u8  [n_items] */
} rb_locate_out;
/* Device pointers, asynchronous on `stream` (NULL = the engine's own stream, synchronised before returning); rb_batch_desc
 * in full: packed reads, chunk_start / chunk_length, d_read_ids = "only these reads".  Workspaces are the engine's: one
 * stream per engine, as for rb_classify_batch_device. */
RB_API int rb_locate_batch_device(rb_engine *e, const rb_batch_desc *desc, double error_rate, double significance,
                                  const rb_locate_out *d_out, void *stream);
/* Host buffers.  read_ids (may be NULL) selects the reads to locate: work item j is read read_ids[j], outputs are indexed
 * by work item; with read_ids == NULL the work items are the n_reads reads and n_items is not looked at. */
RB_API int rb_locate_batch(rb_engine *e, const char *seqs, const uint64_t *offsets, const uint32_t *lens, size_t n_reads,
                           const uint32_t *read_ids, size_t n_items, double error_rate, double significance,
                           const rb_locate_out *out);

/* ---- hits: EVERY bin a read hit, per strand, with its k-mer count ---------------------------------
 * The reference has no such call.  This is what seqan::count returns and select_matches walks (src/IBF/IBFClassify.cpp:16-38,
 * 97-98, 149-150): which bins reached the threshold, on which strand, with what count -- the list behind the hit_bins of the
 * locate pass.  An opt-in pass of its own, like locate: it always counts in full, whatever the engine's pruning /
 * early-decision / merge / phased settings are, and changes nothing any other call returns; from each filter's own table
 * unless rb_engine_set_pass_lists (readbouncer_amd_tuning.h; off by default) lets a filter's list table serve it, which
 * changes no result.
 * Per (work item, filter), deplete filters first: fwd[b], rev[b] = the two uint16_t count vectors of seqan::count under the
 * engine's N rule, t = the threshold; a HIT is a (bin b, strand s) with c_s[b] >= t.  Records are per (bin, strand): a bin that
 * reaches t on both strands yields two.
 *   min_count == 0 : t = rb_threshold(length, k, error_rate, significance) as the decision stage reads it -- the t of
 *                    rb_locate_out's hit_bins (t == 0 lists every existing bin on both strands, a wrapped t of 65 5xx nothing)
 *   min_count  > 0 : t = min_count for every filter; min_count = 1 with max_hits = 2 x n_bins is seqan::count in sparse form
 *   hits      rb_hit [n_items x n_filters x max_hits]  the first min(n_hits, max_hits) hits in rising (bin, strand) order;
 *                    slots beyond those are NOT written.  Order and truncation are deterministic
 *   n_hits    u32 [n_items x n_filters]  the exact number of hits, whatever max_hits is: n_hits > max_hits = truncated
 *   status    u8  [n_items]  the status rules of rb_locate_out; an item that is not RB_OK has n_hits == 0 and no record
 *   bin_reads u64, one entry per bin of every filter, concatenated in filter order: the call ADDS 1 per distinct hit bin
 *                    (either strand) of every RB_OK item, whatever max_hits is.  The caller zeroes it; it accumulates over calls
 * The distinct bins of an untruncated list number rb_locate_out's hit_bins, and its highest count is max_count whenever that
 * is >= t.  max_hits == 0 is legal (n_hits / bin_reads only).  A column-sharded engine refuses with RB_ERR_INVALID_ARG. */
typedef struct rb_hit {
    uint32_t bin;
    uint16_t count;
    uint8_t strand;   /* 0 forward, 1 reverse complement */
    uint8_t reserved; /* 0 */
} rb_hit;
typedef struct rb_hits_out { /* any member may be NULL, but not hits, n_hits and bin_reads all at once */
    void *hits;      /* rb_hit [n_items x n_filters x max_hits] */
    void *n_hits;    /* u32 [n_items x n_filters] */
    void *status;    /* u8  [n_items] */
    void *bin_reads; /* u64 [sum of the filters' bins] */
} rb_hits_out;
/* Device pointers, asynchronous on `stream` (NULL = the engine's own stream, synchronised before returning); rb_batch_desc in
 * full.  Allocates (and keeps, as the engine's) a workspace of n_items x S x 2 x max_hits records of 8 bytes plus
 * n_items x S x 2 counters, S = the most column slices of any filter (ceil(bin_width / 128) beyond 64 words, else 1): a caller
 * with a large max_hits bounds it by the size of its calls.  One stream per engine, as for rb_classify_batch_device. */
RB_API int rb_hits_batch_device(rb_engine *e, const rb_batch_desc *desc, double error_rate, double significance,
                                uint16_t min_count, uint32_t max_hits, const rb_hits_out *d_out, void *stream);
/* Host buffers; read_ids / n_items as in rb_locate_batch.  Large calls are processed in sub-batches so that the device
 * workspace and the staged outputs together stay at or below 256 MiB (one work item at a time where a single item needs more). */
RB_API int rb_hits_batch(rb_engine *e, const char *seqs, const uint64_t *offsets, const uint32_t *lens, size_t n_reads,
                         const uint32_t *read_ids, size_t n_items, double error_rate, double significance, uint16_t min_count,
                         uint32_t max_hits, const rb_hits_out *out);

/* ---- spans: WHERE ALONG THE READ a bin matched: mask, span and longest run ---------------------------
 * The reference has no such call.  seqan::count adds 1 per k-mer whose h words all hold the bin's bit (src/IBF/IBFClassify.cpp:97-98,
 * 149-150) and nothing keeps WHICH k-mers of the read those were: max_matches and select_matches see the sums only (:48-71, :16-38).
 * A bin is a fragment_size stretch of a reference record (src/IBF/IBFBuild.cpp:165-204); this is the other half of "the read matched
 * record R around position P": which part of the read did.  An opt-in pass of its own, like locate and hits: it always reads the
 * named filter's own table, whatever the engine's pruning / early-decision / merge / phased settings are, changes nothing any other
 * call returns, and has no threshold (so no error_rate / significance).
 * A QUERY is (work item, bin) against ONE filter of the engine (`filter`: deplete filters first).  With len = the bases rb_batch_desc
 * selects for the item, k the filter's k-mer size and n_kmers = len - k + 1, POSITION p in [0, n_kmers) is the window of bases
 * [p, p + k) of the chunk, in the read's own direction on both strands:
 *   strand 0: p is a hit when all h words selected by the k-mer of that window have the bin's bit set -- the test by which seqan::count
 *             adds 1 to fwd[bin]
 *   strand 1: the same for the reverse complement of that window under the engine's N rule (rb_engine_set_revcomp_of_n) -- k-mer
 *             n_kmers - 1 - p of the reverse-complemented chunk, so the hit positions of strand 1 number rev[bin]
 * Per (query, strand) one rb_span; every slot of every output is written for every query (all mask_words words per (query, strand):
 * zero beyond n_kmers, zero beyond what fits -- the caller clears nothing).  Positions at or beyond 64 x mask_words are left out of
 * the MASK only: the record is exact whatever mask_words is, and mask_words == 0 is legal.
 *   status   the item's status by the rules of rb_locate_out (RB_OK, RB_ERR_BAD_CHUNK, RB_ERR_INVALID_ARG for longer than max_len,
 *            RB_ERR_SHORT_READ), and RB_ERR_INVALID_ARG when item >= n_items or bin >= the filter's n_bins -- both tested on the device
 *            before anything is read through them: queries may come straight from another kernel's output
 *   a query that is not RB_OK has n_kmers = 0, zero counts, 0xFFFFFFFF positions and a zero mask
 * A column-sharded engine refuses with RB_ERR_INVALID_ARG, as locate does. */
typedef struct rb_span {
    uint32_t count;     /* hit positions, exact; its low 16 bits are seqan::count's uint16_t entry for this bin and strand */
    uint32_t first;     /* lowest hit position;  0xFFFFFFFF when count == 0 */
    uint32_t last;      /* highest hit position; 0xFFFFFFFF when count == 0 */
    uint32_t run_start; /* start of the longest run of consecutive hit positions, the lowest such run on a tie; 0xFFFFFFFF when none */
    uint32_t run_len;   /* its length; 0 when count == 0 */
    uint32_t covered;   /* bases b of the chunk with a hit position p, p <= b < p + k */
} rb_span;
typedef struct rb_span_query { uint32_t item; uint32_t bin; } rb_span_query;
typedef struct rb_spans_out {   /* any member may be NULL, not all */
    void *spans;    /* rb_span [n_queries x 2]: strand 0, then strand 1 */
    void *mask;     /* u64 [n_queries x 2 x mask_words]: bit p & 63 of word p >> 6 = position p is a hit */
    void *n_kmers;  /* u32 [n_queries] */
    void *status;   /* u8  [n_queries] */
} rb_spans_out;
/* Device pointers (d_queries: rb_span_query [n_queries]), asynchronous on `stream` (NULL = the engine's own stream, synchronised before
 * returning); rb_batch_desc in full.  filter >= the engine's filters, a null descriptor or an rb_spans_out with no output is
 * RB_ERR_INVALID_ARG.  No workspace beyond the chunk bookkeeping every descriptor call shares: one stream per engine, as for
 * rb_classify_batch_device. */
RB_API int rb_spans_batch_device(rb_engine *e, const rb_batch_desc *desc, size_t filter, const void *d_queries, size_t n_queries,
                                 uint32_t mask_words, const rb_spans_out *d_out, void *stream);
/* Host buffers; read_ids / n_items as in rb_locate_batch (queries name work items).  The reads are uploaded once; the queries are
 * processed in sub-batches so that what they stage on the device (masks, records, n_kmers, status and the queries themselves) stays at or
 * below 256 MiB (one query at a time where a single one needs more). */
RB_API int rb_spans_batch(rb_engine *e, const char *seqs, const uint64_t *offsets, const uint32_t *lens, size_t n_reads,
                          const uint32_t *read_ids, size_t n_items, size_t filter, const rb_span_query *queries, size_t n_queries,
                          uint32_t mask_words, const rb_spans_out *out);

/* ---- prefixes: the decision at EVERY prefix checkpoint of a read, from one pass over its k-mers -----
 * The reference's live loop concatenates a read's chunks and runs check_unblock again on the whole grown prefix
 * (src/main/adaptive_sampling.hpp:280-331; classify_reads does the same per chunk, src/main/classify.hpp:262-299): the decision
 * for a read is a function of the prefix length, and not a monotone one -- the threshold grows with the length.  seqan::count adds
 * one per k-mer, so the per-bin counters after the k-mers of a prefix are exactly the counts of that prefix, on both strands (the
 * reverse complement of a prefix consists of the reverse complements of the prefix's own windows); one pass over the longest
 * checkpoint, with the maximum over bins taken at each checkpoint, yields every row, where P calls of rb_classify_batch_device_ex
 * would gather the sum of the checkpoints' worth of filter lines.
 * prefix_lens: n_prefixes (1 to RB_PREFIX_MAX) checkpoints c_0 < c_1 < ... in bases, none 0, counted from chunk_start; a HOST array
 * in both forms.  ROW (work item i, checkpoint p) holds exactly what rb_classify_batch_device_ex writes for work item i with the same
 * descriptor, error rate, significance and mode, but chunk_length replaced by c_p (by min(c_p, desc->chunk_length) when the descriptor
 * has one): decision, best target and status -- RB_ERR_SHORT_READ for a prefix shorter than k, RB_ERR_BAD_CHUNK, RB_ERR_INVALID_ARG for a
 * row longer than max_len included -- and max_count wherever the row's status is RB_OK.  A checkpoint at or beyond the item's end
 * repeats the whole-item row; prefix_len says so.  All three modes.
 * Like locate an opt-in pass of its own: it always counts in full, whatever the engine's pruning / early-decision / merge / phased
 * settings are, and changes nothing any other call returns; from each filter's own table unless rb_engine_set_prefix_lists
 * (readbouncer_amd_tuning.h; off by default) lets a filter's list table serve it, which returns the same bytes.
 * RB_ERR_INVALID_ARG, with an rb_last_error() that names the fault: null arguments, n_prefixes of 0 or above RB_PREFIX_MAX, a
 * checkpoint of 0, a list that is not strictly rising, an rb_prefix_out with no output, an unknown mode, a column-sharded engine. */
#define RB_PREFIX_MAX 64
typedef struct rb_prefix_out {   /* any member may be NULL, not all */
    void *max_count;      /* u16 [n_items x n_prefixes x n_filters], deplete filters first */
    void *decision;       /* u8  [n_items x n_prefixes], per rb_mode */
    void *best_target;    /* i32 [n_items x n_prefixes] */
    void *status;         /* u8  [n_items x n_prefixes] */
    void *prefix_len;     /* u32 [n_items x n_prefixes]: bases the row stands for = min(c_p, bases the descriptor selects for the item) */
    void *first_decided;  /* u32 [n_items]: lowest p with status RB_OK and decision != 0; n_prefixes when there is none */
} rb_prefix_out;
/* Device pointers (prefix_lens: host), asynchronous on `stream` (NULL = the engine's own stream, synchronised before returning);
 * rb_batch_desc in full.  Workspaces are the engine's (S x n_items x n_prefixes partial maxima of 2 bytes, S = the most column
 * slices of any filter, plus the rows the caller left out): one stream per engine, as for rb_classify_batch_device. */
RB_API int rb_prefix_batch_device(rb_engine *e, const rb_batch_desc *desc, const uint32_t *prefix_lens, uint32_t n_prefixes,
                                  double error_rate, double significance, int mode, const rb_prefix_out *d_out, void *stream);
/* Host buffers; read_ids / n_items as in rb_locate_batch.  The reads are uploaded once; large calls are processed in sub-batches
 * so that the device workspace and the staged outputs together stay at or below 256 MiB (one work item at a time where a single
 * item needs more). */
RB_API int rb_prefix_batch(rb_engine *e, const char *seqs, const uint64_t *offsets, const uint32_t *lens, size_t n_reads,
                           const uint32_t *read_ids, size_t n_items, const uint32_t *prefix_lens, uint32_t n_prefixes,
                           double error_rate, double significance, int mode, const rb_prefix_out *out);

/* ---- resume: a read's counts stay in HBM between chunks, a call counts the NEW k-mers only ----------
 * Reads arrive from the sequencer a chunk at a time and every decision is taken on the prefix grown so far.  The reference
 * concatenates a read's undecided chunks and runs check_unblock on the whole prefix again (src/main/adaptive_sampling.hpp:280-331), so
 * a read that needs four chunks gathers 1 + 2 + 3 + 4 chunks' worth of filter lines.  The prefix pass above needs all bases at once.
 * This is the state between the calls: seqan::count adds one per k-mer, on both strands window by window, so the per-bin counters of a
 * prefix are the counters of the shorter prefix plus one per new window, and the new windows are exactly the k-mers of "the last k - 1
 * bases seen so far + the new chunk".  A set of SLOTS in HBM each holds one read's per-bin uint16_t counters (they wrap at 65 536 as
 * seqan::count's do), both strands, for every filter of the engine, plus the read's last k - 1 bases and its length so far; a call
 * takes new chunks only and counts only their k-mers onto the slots.
 * CONTRACT.  The row of item i is what rb_classify_batch_device_ex writes for ONE read that is the concatenation of every chunk
 * committed to slot d_slots[i] since its last RB_RESUME_FIRST, followed by this chunk, with max_len = max_total_len and the same error
 * rate, significance and mode -- all three modes; max_count is valid wherever the status is RB_OK, and total_len is that read's length.
 * A chunk of zero bases is allowed and repeats the slot's row; while the total is below k the status is RB_ERR_SHORT_READ and the bases
 * are kept.  Error rate and significance may differ from call to call: the state holds counts, not decisions.  The counts follow the
 * engine's N rule (rb_engine_set_revcomp_of_n) as it stood when each chunk was fed.
 * Like locate and prefixes an opt-in pass of its own: it always counts in full from each filter's own table, whatever the engine's
 * pruning / early-decision / merge / phased / row-table settings are, and changes nothing any other call returns -- unless the set's
 * own rb_resume_set_lists (readbouncer_amd_tuning.h; off by default) lets a filter's list table serve a call's N-free items, which
 * changes no result and no byte of a slot.
 * PER ITEM, vetted on the device before any address is formed from it, the slot left exactly as it was, status, decision 0,
 * best_target -1 and total_len 0 in the row, the other items of the batch unaffected:
 *   RB_ERR_INVALID_ARG  slot >= n_slots; a chunk longer than max_chunk_len; a total that would exceed max_total_len
 *   RB_ERR_BAD_CHUNK    chunk_start beyond the end of the read (as in every descriptor call)
 * REFUSED WHOLE with RB_ERR_INVALID_ARG and an rb_last_error() that names the fault: null arguments, an rb_resume_out with no member,
 * an unknown mode, a column-sharded engine, an engine whose filters do not all share one k, a filter of the engine whose bits changed
 * since rb_resume_create (the counters are stale: create a new set); rb_resume_create with 0 slots, or with max_chunk_len 0 or above
 * max_total_len.  HBM that cannot be had is RB_ERR_NOMEM.
 * A SLOT AT MOST ONCE PER CALL.  The host form finds a slot named twice and refuses the call; in the device form it is the caller's
 * precondition.  Breaking it leaves that slot's counts undefined until its next RB_RESUME_FIRST; it harms no other slot and reads or
 * writes nothing outside the slot.
 * The slots cost rb_resume_bytes(): per slot, for every filter 2 strands x 16 planes x 8 bytes x the filter's padded word columns
 * (bin_width rounded up to the next power of two up to 64; beyond 64 to a multiple of 128), plus 40 bytes.  A set belongs to its
 * engine and is destroyed before it. */
typedef struct rb_resume rb_resume;
#define RB_RESUME_FIRST 1u   /* this chunk starts a new read in the slot: what it held is dropped */
#define RB_RESUME_PEEK  2u   /* answer as if the chunk were appended; leave the slot exactly as it was */
typedef struct rb_resume_out {   /* any member may be NULL, not all */
    void *max_count;   /* u16 [n_items x n_filters], deplete filters first */
    void *decision;    /* u8  [n_items], per rb_mode */
    void *best_target; /* i32 [n_items] */
    void *status;      /* u8  [n_items] */
    void *total_len;   /* u32 [n_items]: bases the row stands for */
} rb_resume_out;
RB_API int rb_resume_create(rb_engine *e, uint32_t n_slots, uint32_t max_chunk_len, uint32_t max_total_len, rb_resume **out);
RB_API void rb_resume_destroy(rb_resume *r);
RB_API uint64_t rb_resume_bytes(const rb_resume *r);   /* HBM held by the slots */
/* Device pointers, asynchronous on `stream` (NULL = the engine's own stream, synchronised before returning).  rb_batch_desc selects
 * each item's CHUNK as in every descriptor call: packed reads, chunk_start / chunk_length, d_read_ids; desc->max_len is not looked at
 * (max_chunk_len bounds a chunk).  d_slots: u32 per item; d_flags: u8 per item of RB_RESUME_* bits, NULL = 0.  Workspaces are the
 * engine's (n_items x (max_chunk_len + 31) bytes of stitched bases and the partial maxima): one stream per engine, as for
 * rb_classify_batch_device. */
RB_API int rb_resume_batch_device(rb_resume *r, const rb_batch_desc *desc, const void *d_slots, const void *d_flags,
                                  double error_rate, double significance, int mode, const rb_resume_out *d_out, void *stream);
/* Host buffers: read i is the new chunk of slot slots[i] (flags may be NULL). */
RB_API int rb_resume_batch(rb_resume *r, const char *seqs, const uint64_t *offsets, const uint32_t *lens, size_t n_reads,
                           const uint32_t *slots, const uint8_t *flags, double error_rate, double significance, int mode,
                           const rb_resume_out *out);
/* One slot's counters of one filter as the two count vectors of seqan::count (forward, then reverse complement), and the slot's total
 * length; either output may be NULL, not both.  Synchronous, on the engine's own stream. */
RB_API int rb_resume_counts(rb_resume *r, uint32_t slot, size_t filter, uint16_t *out_counts /* [2][n_bins] */, uint32_t *out_total_len);

/* bin-sharded operation: restrict the engine to word columns
 * [rank*ceil(W/world) , ...) of every block; out_maxcount then holds PARTIAL maxima that the
 * caller combines with an all-reduce(max) before rb_decide_device. world=1 restores the default. */
RB_API int rb_engine_set_column_shard(rb_engine *e, int rank, int world);
/* decision stage alone (K2) on device-resident raw maxima */
RB_API int rb_decide_device(rb_engine *e, const void *d_maxcount, const void *d_lens, size_t n_reads,
                            uint32_t max_len, double error_rate, double significance, int mode,
                            void *d_best_target, void *d_decision, void *d_status, void *stream);

/* Same for a bin-sharded node: d_maxcount holds n_parts partial tables (the all-gathered outputs of the ranks, each
 * [n_reads x filters] u16, part_stride elements apart); the raw maximum of a (read, filter) is the max over them, taken
 * inside the decision kernel -- no separate reduction pass and no widening of the u16 values for a collective. */
RB_API int rb_decide_device_parts(rb_engine *e, const void *d_maxcount, uint32_t n_parts, uint64_t part_stride,
                                  const void *d_lens, size_t n_reads, uint32_t max_len, double error_rate,
                                  double significance, int mode, void *d_best_target, void *d_decision, void *d_status,
                                  void *stream);

/* ---- single-process multi-GPU pool -----------------------------------------------------------
 * One engine + one host thread per entry of devices[] (an entry may repeat), every filter replicated into each
 * device's HBM from its host image, batches cut into contiguous slices of ceil(n/parts) reads, no collective
 * (SURVEY 8e).  Batches with fewer than min_split reads per device are not split: they go to one device,
 * round-robin.  Outputs as rb_classify_batch. */
typedef struct rb_pool rb_pool;
RB_API int rb_pool_create(const int *devices, size_t n_devices, const rb_ibf *const *deplete, size_t n_deplete,
                          const rb_ibf *const *target, size_t n_target, rb_pool **out);
/* The same pool from .ibf FILES, without a host image of any filter (rb_pool_create needs rb_ibf images: 8 GiB on the host
 * and one PCIe upload per device for a GRCh38 filter): every file is streamed once into the HBM of devices[0]
 * (rb_dibf_open) and replicated from there to all other devices AT ONCE, device to device -- xGMI is point to point,
 * devices[0] has a link of its own to each peer, so the N-1 copies run side by side at link speed (no ring, no tree:
 * a tree would only add hops on a fully connected node).  A device that refuses peer access gets its copy by the
 * runtime's staged path; if that fails too it streams the file itself.  replication_seconds (may be NULL): wall time
 * of all device-to-device copies. */
RB_API int rb_pool_create_from_files(const int *devices, size_t n_devices, const char *const *deplete_paths, size_t n_deplete,
                                     const char *const *target_paths, size_t n_target, rb_pool **out,
                                     double *replication_seconds);
/* The same from filters that are already resident on some device (built there, or loaded once): every entry of `devices` gets
 * a replica of its own, copied device to device like above (the source's own device included -- the pool owns what it
 * classifies against; the caller keeps its filters). */
RB_API int rb_pool_create_from_device(const int *devices, size_t n_devices, rb_dibf *const *deplete, size_t n_deplete,
                                      rb_dibf *const *target, size_t n_target, rb_pool **out, double *replication_seconds);
RB_API void rb_pool_destroy(rb_pool *p);
RB_API size_t rb_pool_size(const rb_pool *p);
RB_API int rb_pool_classify_batch(rb_pool *p, const char *seqs, const uint64_t *offsets, const uint32_t *lens,
                                  size_t n_reads, double error_rate, double significance, int mode,
                                  uint16_t *out_maxcount, int32_t *out_best_target, uint8_t *out_decision,
                                  uint8_t *out_status);

/* ---- live micro-batch shim ----------------------------------------------------------------
 * Batch form of classify_live_reads (src/main/adaptive_sampling.hpp:214-356), the step between the reference's
 * classification_queue and action_queue: keeps the once_seen map, concatenates undecided chunks of a read,
 * applies the 1500 bp cut-off (:315) and maps decisions to actions like Data::sendActions
 * (src/minknow/Data.cpp:169-187).  Read ids are opaque byte strings. */
typedef struct rb_live rb_live;
RB_API int rb_live_create(rb_engine *e, double error_rate, double significance, uint32_t max_undecided_len,
                          rb_live **out);
RB_API void rb_live_destroy(rb_live *lv);
/* out_action[i]: 0 = none yet (read kept in once_seen), 1 = unblock_read, 2 = stop_receiving_data;
 * out_status[i] != RB_OK = the reference's caught-exception case (no action, state untouched);
 * out_classified_len[i] = length of the (possibly concatenated) sequence the decision was taken on. */
RB_API int rb_live_process(rb_live *lv, const char *ids, const uint64_t *id_offsets, const uint32_t *id_lens,
                           const char *seqs, const uint64_t *offsets, const uint32_t *lens, size_t n,
                           uint8_t *out_action, uint8_t *out_status, uint32_t *out_classified_len);
/* reads currently waiting for more data (size of once_seen) */
RB_API size_t rb_live_pending(rb_live *lv);
/* drop a read that ended on the sequencer before a decision was reached */
RB_API int rb_live_forget(rb_live *lv, const char *id, uint32_t id_len);

/* What the reverse strand holds where the read has an N.  The reference counts the second strand on
 * ModifiedString<ModifiedString<Dna5String, ModComplementDna>, ModReverse> (src/IBF/IBF.hpp:96-97, used at
 * src/IBF/IBFClassify.cpp:98,150): the four-letter complement functor over a Dna5 host, for which SeqAn converts N to A
 * (value & 3) before complementing -- the reverse strand sees T (ordinal 3), the forward strand hashes N as ordinal 4.
 * That is the default (rbspec::kRevCompOfN in readbouncer_amd/csrc/ibf_spec.h, a recalled SeqAn fact like the hash
 * constants).  ordinal = 4 gives the other candidate, "N stays N" (ModComplementDna5); anything else is refused.  Only
 * k-mers of the reverse strand that cover an N are affected. */
RB_API int rb_engine_set_revcomp_of_n(rb_engine *e, uint32_t ordinal);
/* The same for every engine this process creates FROM NOW ON (the C++ mirror and the CLI create their engines themselves:
 * interleave::set_revcomp_of_n, `readbouncer_amd_cli --revcomp-of-n 4`).  This is the only process-wide switch that changes a
 * result, and it is a call, not an environment variable. */
RB_API int rb_set_default_revcomp_of_n(uint32_t ordinal);

#ifdef __cplusplus
}
#endif
#endif /* READBOUNCER_AMD_H_ */

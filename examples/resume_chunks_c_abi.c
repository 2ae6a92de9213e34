/* Resumable counting from plain C99: a read's per-bin counters stay in HBM between the chunks a sequencer delivers, and every
 * call counts the k-mers of the NEW chunk only (include/readbouncer_amd.h, "resume").
 *
 * Builds one depletion filter in HBM, gives each of three reads a slot and feeds them in four chunks of 360 bases -- the live loop of
 * src/main/adaptive_sampling.hpp:280-331 without concatenating anything on the host.  After every feed the row of each read must be
 * exactly what rb_classify_batch returns for the concatenation of the chunks fed so far: raw maximum, decision, best target, status.
 *
 *   gcc -std=c99 -Iinclude examples/resume_chunks_c_abi.c -Lreadbouncer_amd -lreadbouncer_amd \
 *       -Wl,-rpath,$PWD/readbouncer_amd -o resume_chunks_c_abi
 *
 * Exit code 0: every row equal.  2: no GPU (the engine has no CPU path).  1: anything else. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "readbouncer_amd.h"

#define CHECK(call)                                                                                          \
    do {                                                                                                     \
        int st_ = (call);                                                                                    \
        if (st_ != RB_OK) {                                                                                  \
            fprintf(stderr, "%s -> %s (%s)\n", #call, rb_status_string(st_), rb_last_error());               \
            return st_ == RB_ERR_NO_DEVICE ? 2 : 1;                                                          \
        }                                                                                                    \
    } while (0)

static uint64_t lcg_state = 0x13198A2E03707344ull;
static uint32_t lcg(void)
{
    lcg_state = lcg_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(lcg_state >> 33);
}

static void random_dna(char *dst, size_t n)
{
    size_t i;
    for (i = 0; i < n; ++i) dst[i] = "ACGT"[lcg() & 3];
}

enum { REF_LEN = 200000, CHUNK = 360, N_CHUNKS = 4, N_READS = 3, READ_LEN = CHUNK * N_CHUNKS, FRAGMENT = 10000, KMER = 13 };

int main(void)
{
    char *ref, *reads, *chunks;
    uint64_t offsets[N_READS], next_bin = 0, n_bins, n_bits;
    uint32_t lens[N_READS], slots[N_READS], total_len[N_READS];
    uint8_t flags[N_READS], decision[N_READS], status[N_READS], want_decision[N_READS], want_status[N_READS];
    uint16_t maxcount[N_READS], want_maxcount[N_READS];
    int32_t best_target[N_READS], want_best[N_READS];
    rb_dibf *dep = NULL;
    rb_engine *eng = NULL;
    rb_resume *set = NULL;
    rb_resume_out out;
    int i, j, c, wrong = 0;

    printf("%s, %d device(s)\n", rb_version(), rb_device_count());
    if (rb_device_count() <= 0) {
        fprintf(stderr, "no gfx950 GPU visible: the engine has no CPU fallback\n");
        return 2;
    }

    ref = (char *)malloc(REF_LEN);
    reads = (char *)malloc((size_t)N_READS * READ_LEN);
    chunks = (char *)malloc((size_t)N_READS * CHUNK);
    if (!ref || !reads || !chunks) return 1;
    random_dna(ref, REF_LEN);
    n_bins = rb_fragment_bounds(REF_LEN, FRAGMENT, KMER, 500, NULL, NULL, 0);
    n_bits = rb_calculate_filter_size_bits(FRAGMENT, KMER, 3, 0.01, n_bins);
    CHECK(rb_dibf_create(0, n_bins, 3, KMER, n_bits, &dep));
    CHECK(rb_dibf_add_sequence(dep, ref, REF_LEN, FRAGMENT, 500, 0, &next_bin));

    /* read 0: from the reference with 4 % substitutions; read 1: random; read 2: random up to base 700, from the reference behind it */
    memcpy(reads, ref + 12345, READ_LEN);
    for (j = 0; j < READ_LEN; ++j)
        if (lcg() % 25 == 0) reads[j] = "ACGT"[lcg() & 3];
    random_dna(reads + READ_LEN, READ_LEN);
    random_dna(reads + 2 * READ_LEN, 700);
    memcpy(reads + 2 * READ_LEN + 700, ref + 99000, READ_LEN - 700);

    CHECK(rb_engine_create(0, &dep, 1, NULL, 0, &eng));
    CHECK(rb_resume_create(eng, N_READS, CHUNK, READ_LEN, &set));
    printf("%d slots hold %llu bytes of HBM\n", N_READS, (unsigned long long)rb_resume_bytes(set));
    out.max_count = maxcount;
    out.decision = decision;
    out.best_target = best_target;
    out.status = status;
    out.total_len = total_len;

    for (c = 0; c < N_CHUNKS; ++c) {
        /* what the sequencer delivered this round: chunk c of every read, for the slot of its channel */
        for (i = 0; i < N_READS; ++i) {
            memcpy(chunks + (size_t)i * CHUNK, reads + (size_t)i * READ_LEN + (size_t)c * CHUNK, CHUNK);
            offsets[i] = (uint64_t)i * CHUNK;
            lens[i] = CHUNK;
            slots[i] = (uint32_t)i;
            flags[i] = (uint8_t)(c == 0 ? RB_RESUME_FIRST : 0);
        }
        CHECK(rb_resume_batch(set, chunks, offsets, lens, N_READS, slots, flags, 0.1, 0.95, RB_MODE_CHECK_UNBLOCK, &out));
        /* the reference's way: the whole prefix again */
        for (i = 0; i < N_READS; ++i) {
            offsets[i] = (uint64_t)i * READ_LEN;
            lens[i] = (uint32_t)((c + 1) * CHUNK);
        }
        CHECK(rb_classify_batch(eng, reads, offsets, lens, N_READS, 0.1, 0.95, RB_MODE_CHECK_UNBLOCK, want_maxcount, want_best, want_decision,
                                want_status));
        for (i = 0; i < N_READS; ++i) {
            const int same = maxcount[i] == want_maxcount[i] && decision[i] == want_decision[i] && best_target[i] == want_best[i] &&
                             status[i] == want_status[i] && total_len[i] == lens[i];
            printf("chunk %d read %d: %u bases, max count %u, decision %u%s\n", c, i, total_len[i], maxcount[i], decision[i],
                   same ? "" : "  <- differs from rb_classify_batch on the concatenation");
            wrong += !same;
        }
    }
    printf("%d rows, %d differ\n", N_READS * N_CHUNKS, wrong);

    rb_resume_destroy(set);
    rb_engine_destroy(eng);
    rb_dibf_free(dep);
    free(ref);
    free(reads);
    free(chunks);
    return wrong ? 1 : 0;
}

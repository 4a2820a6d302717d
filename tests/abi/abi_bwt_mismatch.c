/* abi_bwt_mismatch.c -- the search with mismatches through the C ABI, without Python: two threads share one handle per
 * text ("banana" and (ACGT)^3) and each takes every pattern of length 1..4 over {A, C, G, T, N, $} plus patterns of length
 * n, n + 1 and 2n through polyhip_bwt_count_mismatch and polyhip_bwt_locate_mismatch for k = 0..4, against a brute-force
 * compare written here; then the capacity rule (first[] filled, pos / mm untouched, the size named) and the thread's own
 * polyhip_bwt_mismatch_last_info.  Prints "abi_bwt_mismatch ok" and exits 0, or says what differed and exits 1. */
#include <pthread.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "polyhip.h"

#define MAXPAT 1600
#define MAXLEN 32

static const char SYMBOLS[] = "ACGTN$";

typedef struct {
    const char *text;
    polyhip_bwt *h;
    int thread, failed;
    char why[256];
} job_t;

static int fail(job_t *j, const char *what, int k, uint64_t at)
{
    snprintf(j->why, sizeof j->why, "thread %d on \"%s\", k = %d: %s at %llu (%s)", j->thread, j->text, k, what,
             (unsigned long long)at, polyhip_last_error());
    j->failed = 1;
    return 1;
}

static uint64_t make_patterns(const char *text, uint8_t *buf, uint64_t *off)
{
    uint64_t np = 0, nb = 0;
    off[0] = 0;
    for (int m = 1; m <= 4; ++m) {
        int total = 1;
        for (int q = 0; q < m; ++q)
            total *= 6;
        for (int v = 0; v < total; ++v) {
            int w = v;
            for (int q = 0; q < m; ++q, w /= 6)
                buf[nb++] = (uint8_t)SYMBOLS[w % 6];
            off[++np] = nb;
        }
    }
    char lng[4][MAXLEN];
    snprintf(lng[0], MAXLEN, "%s", text);                 /* n */
    snprintf(lng[1], MAXLEN, "C%s", text + 1);            /* n, one symbol changed */
    snprintf(lng[2], MAXLEN, "%s%c", text, text[0]);      /* n + 1 */
    snprintf(lng[3], MAXLEN, "%s%s", text, text);         /* 2n */
    for (int q = 0; q < 4; ++q) {
        memcpy(buf + nb, lng[q], strlen(lng[q]));
        nb += strlen(lng[q]);
        off[++np] = nb;
    }
    return np;
}

static int run_text(job_t *j)
{
    static const uint32_t SENT = 0xDEADBEEFu;
    const uint8_t *S = (const uint8_t *)j->text;
    const uint64_t n = strlen(j->text);
    uint8_t *buf = malloc(MAXPAT * MAXLEN);
    uint64_t *off = malloc((MAXPAT + 1) * sizeof *off), *first = malloc((MAXPAT + 1) * sizeof *first);
    const uint64_t np = make_patterns(j->text, buf, off);
    const uint64_t cap = np * n + 1;
    uint32_t *counts = malloc(np * 5 * sizeof *counts), *err = malloc(np * sizeof *err), *pos = malloc(cap * sizeof *pos);
    uint8_t *mm = malloc(cap);
    for (int k = 0; k <= 4 && !j->failed; ++k) {
        if (polyhip_bwt_count_mismatch(j->h, buf, off, np, (uint32_t)k, counts, err) != POLYHIP_OK)
            return fail(j, "count_mismatch failed", k, 0);
        if (polyhip_bwt_locate_mismatch(j->h, buf, off, np, (uint32_t)k, first, pos, mm, cap, err) != POLYHIP_OK)
            return fail(j, "locate_mismatch failed", k, 0);
        uint64_t at = 0;
        for (uint64_t p = 0; p < np; ++p) {
            const uint8_t *P = buf + off[p];
            const uint64_t m = off[p + 1] - off[p];
            uint32_t want[5] = {0, 0, 0, 0, 0};
            if (first[p] != at)
                return fail(j, "first differs", k, p);
            if (err[p])
                return fail(j, "err set", k, p);
            for (uint64_t s = 0; m <= n && s + m <= n; ++s) {
                uint32_t d = 0;
                for (uint64_t q = 0; q < m; ++q)
                    d += S[s + q] != P[q];
                if (d > (uint32_t)k)
                    continue;
                ++want[d];
                if (pos[at] != s || mm[at] != d)
                    return fail(j, "hit differs", k, p);
                ++at;
            }
            for (int d = 0; d <= k; ++d)
                if (counts[p * (uint64_t)(k + 1) + d] != want[d])
                    return fail(j, "count differs", k, p);
        }
        if (first[np] != at)
            return fail(j, "total differs", k, np);
        polyhip_bwt_mismatch_info info;
        if (polyhip_bwt_mismatch_last_info(&info) != POLYHIP_OK || info.patterns != np || info.hits != at || info.leaves > info.nodes)
            return fail(j, "last_info differs", k, info.hits);
        /* capacity: one entry short fails, names the size, fills first[] and leaves pos / mm alone */
        if (at > 0) {
            for (uint64_t q = 0; q < at; ++q) {
                pos[q] = SENT;
                mm[q] = 0xEE;
            }
            first[np] = 0;
            char need[32];
            snprintf(need, sizeof need, "%llu", (unsigned long long)at);
            if (polyhip_bwt_locate_mismatch(j->h, buf, off, np, (uint32_t)k, first, pos, mm, at - 1, err) != POLYHIP_ERR_INVALID ||
                !strstr(polyhip_last_error(), need))
                return fail(j, "capacity - 1 was not refused with the size", k, at);
            if (first[np] != at)
                return fail(j, "first[] not filled on a short buffer", k, at);
            for (uint64_t q = 0; q < at; ++q)
                if (pos[q] != SENT || mm[q] != 0xEE)
                    return fail(j, "a short buffer was written", k, q);
            if (polyhip_bwt_locate_mismatch(j->h, buf, off, np, (uint32_t)k, first, pos, mm, at, err) != POLYHIP_OK || pos[at - 1] == SENT)
                return fail(j, "capacity == total failed", k, at);
        }
    }
    free(buf), free(off), free(first), free(counts), free(err), free(pos), free(mm);
    return j->failed;
}

static void *worker(void *arg)
{
    run_text((job_t *)arg);
    return NULL;
}

int main(void)
{
    static const char *TEXTS[2] = {"banana", "ACGTACGTACGT"};
    uint32_t e = 0;
    uint64_t f0 = 7;
    if (polyhip_bwt_count_mismatch(NULL, NULL, NULL, 0, 5, NULL, NULL) != POLYHIP_ERR_UNSUPPORTED ||
        polyhip_bwt_count_mismatch(NULL, NULL, NULL, 0, 4, NULL, NULL) != POLYHIP_ERR_INVALID) {
        printf("abi_bwt_mismatch: the argument errors come in another order\n");
        return 1;
    }
    for (int t = 0; t < 2; ++t) {
        polyhip_bwt *h = NULL;
        if (polyhip_bwt_create((const uint8_t *)TEXTS[t], strlen(TEXTS[t]), &h) != POLYHIP_OK) {
            printf("abi_bwt_mismatch: create failed: %s\n", polyhip_last_error());
            return 1;
        }
        if (polyhip_bwt_locate_mismatch(h, NULL, NULL, 0, 2, &f0, NULL, NULL, 0, &e) != POLYHIP_OK || f0 != 0) {
            printf("abi_bwt_mismatch: npat == 0 is not an empty successful call\n");
            return 1;
        }
        job_t jobs[2];
        pthread_t th[2];
        for (int i = 0; i < 2; ++i) {
            jobs[i] = (job_t){TEXTS[t], h, i, 0, ""};
            pthread_create(&th[i], NULL, worker, &jobs[i]);
        }
        for (int i = 0; i < 2; ++i)
            pthread_join(th[i], NULL);
        polyhip_bwt_destroy(h);
        for (int i = 0; i < 2; ++i)
            if (jobs[i].failed) {
                printf("abi_bwt_mismatch: %s\n", jobs[i].why);
                return 1;
            }
    }
    printf("abi_bwt_mismatch ok: 2 threads x 2 texts x k = 0..4\n");
    return 0;
}

/* quintet_host_check.c -- the host-only calls of DESIGN.md section 22 (tq_quintet_class_table and the jackknife on sums of
 * slots, tq_dstat_jackknife_masks) on designed block rows, driven from a plain C program.
 * Built and run under the host sanitizers by tools/host_checks.sh.
 *
 * No device is needed or touched: neither call takes a context.  Every buffer is allocated at its exact size, so a read
 * or write past a row, a block, a test or the table shows as a sanitizer report.  The values are checked against a
 * restatement of the rule in this file (long double sums, a tolerance), not bit for bit: that is the Python tests' part.
 * Prints "quintet_host_check: ok" and returns 0 when every check held. */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "tetrad_hip.h"

static uint64_t state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(uint32_t n)
{
    state = state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)((state >> 33) % n);
}

#define CHECK(cond)                                                                        \
    do {                                                                                   \
        if (!(cond)) {                                                                     \
            fprintf(stderr, "quintet_host_check: line %d: %s\n", __LINE__, #cond);         \
            exit(1);                                                                       \
        }                                                                                  \
    } while (0)

static int close_to(double got, long double want)
{
    if (isnan(want)) return isnan(got);
    return fabsl((long double)got - want) <= 1e-9L * (fabsl(want) > 1.0L ? fabsl(want) : 1.0L);
}

/* the class rule again: count the distinct bases, then the four comparisons with x0 */
static void check_table(void)
{
    uint8_t *table = (uint8_t *)malloc(1024);
    int per_class[16] = {0};
    CHECK(table);
    CHECK(tq_quintet_class_table(NULL) == TQ_ERR_INVALID_ARG);
    CHECK(tq_quintet_class_table(table) == TQ_OK);
    for (int p = 0; p < 1024; ++p) {
        const int x[5] = {p >> 8, (p >> 6) & 3, (p >> 4) & 3, (p >> 2) & 3, p & 3};
        int present = 0, k = 0;
        for (int i = 0; i < 5; ++i) present |= 1 << x[i];
        for (int i = 1; i < 5; ++i) k |= (x[i] != x[0]) << (i - 1);
        const int two = present == 3 || present == 5 || present == 9 || present == 6 || present == 10 || present == 12;
        CHECK(table[p] == (two ? k : 0));
        per_class[table[p]]++;
    }
    CHECK(per_class[0] == 1024 - 180);
    for (int k = 1; k < 16; ++k) CHECK(per_class[k] == 12);
    free(table);
}

static long double mask_sum(const uint32_t *row, unsigned mask)
{
    long double s = 0;
    for (int k = 0; k < 16; ++k)
        if ((mask >> k) & 1) s += row[k];
    return s;
}

/* the jackknife again, in long double */
static void restate(const uint32_t *rows, int64_t B, unsigned lm, unsigned rm, long double *out)
{
    long double A = 0, Bs = 0;
    int64_t g = 0;
    for (int64_t j = 0; j < B; ++j) {
        const long double a = mask_sum(rows + 16 * j, lm), b = mask_sum(rows + 16 * j, rm);
        A += a;
        Bs += b;
        g += (a + b) > 0;
    }
    const long double n = A + Bs;
    out[0] = (long double)g;
    out[1] = out[2] = out[3] = NAN;
    if (n == 0) return;
    const long double theta = (A - Bs) / n;
    out[1] = theta;
    if (g < 2) return;
    long double sJ = 0, sV = 0;
    for (int64_t j = 0; j < B; ++j) {
        const long double a = mask_sum(rows + 16 * j, lm), b = mask_sum(rows + 16 * j, rm), m = a + b;
        if (m == 0) continue;
        sJ += (n - m) / n * (((A - a) - (Bs - b)) / (n - m));
    }
    const long double tJ = g * theta - sJ;
    for (int64_t j = 0; j < B; ++j) {
        const long double a = mask_sum(rows + 16 * j, lm), b = mask_sum(rows + 16 * j, rm), m = a + b;
        if (m == 0) continue;
        const long double h = n / m, tj = ((A - a) - (Bs - b)) / (n - m);
        const long double e = h * theta - (h - 1) * tj - tJ;
        sV += e * e / (h - 1);
    }
    out[2] = tJ;
    out[3] = sV / g;
}

/* two valid masks: every slot 1..15 goes left, right or nowhere, each side at least one slot */
static void draw_masks(uint16_t *lm, uint16_t *rm)
{
    do {
        *lm = *rm = 0;
        for (int k = 1; k < 16; ++k) {
            const uint32_t side = rnd(3);
            if (side == 1) *lm |= (uint16_t)(1u << k);
            if (side == 2) *rm |= (uint16_t)(1u << k);
        }
    } while (*lm == 0 || *rm == 0);
}

/* kind 0: random with empty blocks; 1: 2^32 - 1 in every slot; 2: all empty; 3: one non-empty block; 4: two non-empty
 * blocks; 5: all fifteen slots in use, seven left and eight right */
static void run(int64_t M, int64_t B, int64_t N, int kind)
{
    uint32_t *rows = (uint32_t *)malloc(sizeof(uint32_t) * 16 * (size_t)(M * B));
    uint32_t *set_of = (uint32_t *)malloc(sizeof(uint32_t) * (size_t)N);
    uint16_t *lm = (uint16_t *)malloc(sizeof(uint16_t) * (size_t)N), *rm = (uint16_t *)malloc(sizeof(uint16_t) * (size_t)N);
    double *out = (double *)malloc(sizeof(double) * 4 * (size_t)N);
    CHECK(rows && set_of && lm && rm && out);
    for (int64_t i = 0; i < M * B; ++i) {
        const int64_t j = i % B;
        const int empty = kind == 2 || (kind == 0 && rnd(6) == 0) || (kind == 3 && j != B / 2) ||
                          (kind == 4 && j != 0 && j != B - 1);
        for (int k = 0; k < 16; ++k) rows[16 * i + k] = empty ? 0 : (kind == 1 ? 0xFFFFFFFFu : 1 + rnd(5000));
    }
    for (int64_t t = 0; t < N; ++t) {
        set_of[t] = t == 0 ? (uint32_t)(M - 1) : rnd((uint32_t)M);       /* the last set is read */
        draw_masks(lm + t, rm + t);
        if (kind == 5) { lm[t] = 0x00FE; rm[t] = 0xFF00; }
    }
    if (N > 1) { lm[1] = 0x8000; rm[1] = 0x0002; }                      /* the last and the first slot */
    for (int64_t i = 0; i < 4 * N; ++i) out[i] = -7.0;
    CHECK(tq_dstat_jackknife_masks(rows, M, B, set_of, lm, rm, N, out) == TQ_OK);
    for (int64_t t = 0; t < N; ++t) {
        long double want[4];
        restate(rows + 16 * B * (int64_t)set_of[t], B, lm[t], rm[t], want);
        for (int k = 0; k < 4; ++k) CHECK(close_to(out[4 * t + k], want[k]));
        if (kind == 2) CHECK(out[4 * t] == 0.0 && isnan(out[4 * t + 1]));
        if (kind == 3) CHECK(out[4 * t] == 1.0 && isnan(out[4 * t + 3]));
        if (kind == 1) CHECK(out[4 * t] == (double)B);
        if (!isnan(out[4 * t + 3])) CHECK(out[4 * t + 3] >= 0.0);
    }
    /* refusals write nothing */
    for (int64_t i = 0; i < 4 * N; ++i) out[i] = -7.0;
    const uint32_t keep = set_of[N - 1];
    const uint16_t keep_l = lm[N - 1], keep_r = rm[N - 1];
    set_of[N - 1] = (uint32_t)M;
    CHECK(tq_dstat_jackknife_masks(rows, M, B, set_of, lm, rm, N, out) == TQ_ERR_INVALID_ARG);
    CHECK(strstr(tq_last_error(NULL), "set_of"));
    set_of[N - 1] = keep;
    lm[N - 1] = (uint16_t)(keep_l | 1);                                 /* bit 0 */
    CHECK(tq_dstat_jackknife_masks(rows, M, B, set_of, lm, rm, N, out) == TQ_ERR_INVALID_ARG);
    CHECK(strstr(tq_last_error(NULL), "masks"));
    lm[N - 1] = 0;                                                      /* empty */
    CHECK(tq_dstat_jackknife_masks(rows, M, B, set_of, lm, rm, N, out) == TQ_ERR_INVALID_ARG);
    lm[N - 1] = keep_l;
    rm[N - 1] = (uint16_t)(keep_r | keep_l);                            /* overlapping */
    CHECK(tq_dstat_jackknife_masks(rows, M, B, set_of, lm, rm, N, out) == TQ_ERR_INVALID_ARG);
    rm[N - 1] = keep_r;
    CHECK(tq_dstat_jackknife_masks(rows, M, 0, set_of, lm, rm, N, out) == TQ_ERR_INVALID_ARG);
    CHECK(tq_dstat_jackknife_masks(rows, M, 4097, set_of, lm, rm, N, out) == TQ_ERR_INVALID_ARG);
    CHECK(strstr(tq_last_error(NULL), "4096"));
    CHECK(tq_dstat_jackknife_masks(rows, M, B, set_of, lm, rm, -1, out) == TQ_ERR_INVALID_ARG);
    CHECK(tq_dstat_jackknife_masks(NULL, M, B, set_of, lm, rm, N, out) == TQ_ERR_INVALID_ARG);
    CHECK(tq_dstat_jackknife_masks(rows, M, B, set_of, lm, rm, N, NULL) == TQ_ERR_INVALID_ARG);
    for (int64_t i = 0; i < 4 * N; ++i) CHECK(out[i] == -7.0);
    CHECK(tq_dstat_jackknife_masks(rows, M, B, set_of, lm, rm, N, out) == TQ_OK);      /* restored: valid again */
    CHECK(tq_dstat_jackknife_masks(NULL, 0, B, NULL, NULL, NULL, 0, NULL) == TQ_OK);
    free(out); free(rm); free(lm); free(set_of); free(rows);
}

int main(void)
{
    static const int64_t Bs[] = {1, 2, 3, 50, 4096};
    static const int64_t Ns[] = {1, 64, 65, 1000};
    check_table();
    for (int kind = 0; kind < 6; ++kind)
        for (size_t b = 0; b < sizeof Bs / sizeof Bs[0]; ++b)
            for (size_t n = 0; n < sizeof Ns / sizeof Ns[0]; ++n)
                run(Bs[b] == 4096 ? 9 : 40, Bs[b], Ns[n], kind);
    printf("quintet_host_check: ok\n");
    return 0;
}

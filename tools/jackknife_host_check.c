/* jackknife_host_check.c -- the host execution of the block jackknife (tq_dstat_jackknife) on
 * designed block rows, driven from a plain C program.
 * Built and run under the host sanitizers by tools/host_checks.sh.
 *
 * No device is needed or touched: the call takes no context.  Every buffer is allocated at its exact size, so a read or
 * write past a row, a block or a test shows as a sanitizer report.  The values are checked against a restatement of
 * the rule in this file (long double sums, a tolerance), not bit for bit: that is the Python tests' part.  Prints
 * "jackknife_host_check: ok" and returns 0 when every check held. */
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
            fprintf(stderr, "jackknife_host_check: line %d: %s\n", __LINE__, #cond);       \
            exit(1);                                                                       \
        }                                                                                  \
    } while (0)

static int close_to(double got, long double want)
{
    if (isnan(want)) return isnan(got);
    return fabsl((long double)got - want) <= 1e-9L * (fabsl(want) > 1.0L ? fabsl(want) : 1.0L);
}

/* the rule again, in long double */
static void restate(const uint32_t *rows, int64_t B, int ca, int cb, long double *out)
{
    long double A = 0, Bs = 0;
    int64_t g = 0;
    for (int64_t j = 0; j < B; ++j) {
        A += rows[16 * j + ca];
        Bs += rows[16 * j + cb];
        g += ((uint64_t)rows[16 * j + ca] + rows[16 * j + cb]) > 0;
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
        const long double a = rows[16 * j + ca], b = rows[16 * j + cb], m = a + b;
        if (m == 0) continue;
        sJ += (n - m) / n * (((A - a) - (Bs - b)) / (n - m));
    }
    const long double tJ = g * theta - sJ;
    for (int64_t j = 0; j < B; ++j) {
        const long double a = rows[16 * j + ca], b = rows[16 * j + cb], m = a + b;
        if (m == 0) continue;
        const long double h = n / m, tj = ((A - a) - (Bs - b)) / (n - m);
        const long double e = h * theta - (h - 1) * tj - tJ;
        sV += e * e / (h - 1);
    }
    out[2] = tJ;
    out[3] = sV / g;
}

/* kind 0: random with empty blocks; 1: counts of 2^32 - 1 everywhere; 2: all empty; 3: one non-empty block;
 * 4: two non-empty blocks; 5: a < b everywhere */
static void run(int64_t M, int64_t B, int64_t N, int kind)
{
    uint32_t *rows = (uint32_t *)malloc(sizeof(uint32_t) * 16 * (size_t)(M * B));
    uint32_t *set_of = (uint32_t *)malloc(sizeof(uint32_t) * (size_t)N);
    uint8_t *ia = (uint8_t *)malloc((size_t)N), *ib = (uint8_t *)malloc((size_t)N);
    double *out = (double *)malloc(sizeof(double) * 4 * (size_t)N);
    CHECK(rows && set_of && ia && ib && out);
    for (int64_t i = 0; i < M * B; ++i) {
        const int64_t j = i % B;
        const int empty = kind == 2 || (kind == 0 && rnd(6) == 0) || (kind == 3 && j != B / 2) ||
                          (kind == 4 && j != 0 && j != B - 1);
        for (int k = 0; k < 16; ++k) {
            uint32_t v = kind == 1 ? 0xFFFFFFFFu : rnd(5000);
            if (kind == 5) v = (k & 1) ? 0xFFFFFF00u - rnd(100) : rnd(50);
            rows[16 * i + k] = empty ? 0 : v;
        }
    }
    for (int64_t t = 0; t < N; ++t) {
        set_of[t] = t == 0 ? (uint32_t)(M - 1) : rnd((uint32_t)M);       /* the last set is read */
        ia[t] = (uint8_t)(kind == 5 ? 2 * rnd(7) : rnd(15));
        ib[t] = (uint8_t)(kind == 5 ? 2 * rnd(7) + 1 : (ia[t] + 1 + rnd(14)) % 15);
    }
    if (N > 1 && kind != 5) { ia[1] = 14; ib[1] = 0; }                   /* the last and the first class */
    for (int64_t i = 0; i < 4 * N; ++i) out[i] = -7.0;
    CHECK(tq_dstat_jackknife(rows, M, B, set_of, ia, ib, N, out) == TQ_OK);
    for (int64_t t = 0; t < N; ++t) {
        long double want[4];
        restate(rows + 16 * B * (int64_t)set_of[t], B, ia[t], ib[t], want);
        for (int k = 0; k < 4; ++k) CHECK(close_to(out[4 * t + k], want[k]));
        if (kind == 2) CHECK(out[4 * t] == 0.0 && isnan(out[4 * t + 1]));
        if (kind == 3) CHECK(out[4 * t] <= 1.0 && isnan(out[4 * t + 3]));
        if (kind == 5) CHECK(out[4 * t + 1] < 0.0);
        if (!isnan(out[4 * t + 3])) CHECK(out[4 * t + 3] >= 0.0);
    }
    /* refusals write nothing */
    for (int64_t i = 0; i < 4 * N; ++i) out[i] = -7.0;
    const uint32_t keep = set_of[N - 1];
    const uint8_t keep_a = ia[N - 1];
    set_of[N - 1] = (uint32_t)M;
    CHECK(tq_dstat_jackknife(rows, M, B, set_of, ia, ib, N, out) == TQ_ERR_INVALID_ARG);
    CHECK(strstr(tq_last_error(NULL), "set_of"));
    set_of[N - 1] = keep;
    ia[N - 1] = 15;
    CHECK(tq_dstat_jackknife(rows, M, B, set_of, ia, ib, N, out) == TQ_ERR_INVALID_ARG);
    CHECK(strstr(tq_last_error(NULL), "class index"));
    ia[N - 1] = keep_a;
    CHECK(tq_dstat_jackknife(rows, M, 0, set_of, ia, ib, N, out) == TQ_ERR_INVALID_ARG);
    CHECK(tq_dstat_jackknife(rows, M, 4097, set_of, ia, ib, N, out) == TQ_ERR_INVALID_ARG);
    CHECK(strstr(tq_last_error(NULL), "4096"));
    CHECK(tq_dstat_jackknife(rows, M, B, set_of, ia, ib, -1, out) == TQ_ERR_INVALID_ARG);
    CHECK(tq_dstat_jackknife(NULL, M, B, set_of, ia, ib, N, out) == TQ_ERR_INVALID_ARG);
    CHECK(tq_dstat_jackknife(rows, M, B, set_of, ia, ib, N, NULL) == TQ_ERR_INVALID_ARG);
    for (int64_t i = 0; i < 4 * N; ++i) CHECK(out[i] == -7.0);
    CHECK(tq_dstat_jackknife(NULL, 0, B, NULL, NULL, NULL, 0, NULL) == TQ_OK);
    free(out); free(ib); free(ia); free(set_of); free(rows);
}

int main(void)
{
    static const int64_t Bs[] = {1, 2, 3, 50, 4096};
    static const int64_t Ns[] = {1, 64, 65, 1000};
    for (int kind = 0; kind < 6; ++kind)
        for (size_t b = 0; b < sizeof Bs / sizeof Bs[0]; ++b)
            for (size_t n = 0; n < sizeof Ns / sizeof Ns[0]; ++n)
                run(Bs[b] == 4096 ? 9 : 40, Bs[b], Ns[n], kind);
    printf("jackknife_host_check: ok\n");
    return 0;
}

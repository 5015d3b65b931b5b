/* stability_host_check.c -- the host back end of the leaf stability accumulator (tq_ls_* without a context, DESIGN.md
 * section 28), driven from a plain C program.
 * Built and run under the host sanitizers by tools/host_checks.sh.
 *
 * No device is needed or touched.  The counts of five hard-coded trees of six taxa are known by hand; those of random
 * trees are recounted from taxon sets -- a tree displays a,b|c,d when some node has a and b below it and neither c nor
 * d, or c and d and neither a nor b -- with a loop over the trees per quartet, and the sums per taxon from those counts.
 * Prints "stability_host_check: ok" and returns 0 when every check held; a sanitizer report or a failed check ends it
 * with a non-zero status. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "tetrad_hip.h"

static uint64_t state = 0xD1B54A32D192ED03ull;
static uint32_t rnd(uint32_t n)
{
    state = state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)((state >> 33) % n);
}

#define CHECK(cond)                                                                   \
    do {                                                                              \
        if (!(cond)) {                                                                \
            fprintf(stderr, "stability_host_check: line %d: %s\n", __LINE__, #cond);  \
            exit(1);                                                                  \
        }                                                                             \
    } while (0)

/* six taxa.  ((0,1),(2,3),(4,5)); ((0,2),(1,3),(4,5)); the star; ((0,1),2,3,4,5) under a root of degree 2 with a unary
 * node; the first tree again, rooted on the edge above (4,5). */
enum { T6 = 6, N6 = 5, STRIDE6 = 12, Q6 = 15 };
static const int32_t trees6[N6][STRIDE6] = {
    {6, 6, 7, 7, 8, 8, 9, 9, 9, -1, -1, -1},
    {6, 7, 6, 7, 8, 8, 9, 9, 9, -1, -1, -1},
    {6, 6, 6, 6, 6, 6, -1, -1, -1, -1, -1, -1},
    {6, 6, 8, 8, 8, 8, 7, 9, 9, -1, -1, -1},
    {6, 6, 7, 7, 8, 8, 9, 9, 10, 10, -1, -1},
};
static const int64_t nodes6[N6] = {10, 10, 7, 10, 11};
/* by hand, per quartet in rank order: the trees that show ab|cd, ac|bd, ad|bc, none.  Trees 0 and 4 are one tree; tree 3
 * resolves only the quartets with 0 and 1, as 01|xy; the star none. */
static const uint16_t want6[Q6][4] = {
    {3, 1, 0, 1}, /* 0123: 01|23 in 0, 3, 4; 02|13 in 1 */
    {3, 1, 0, 1}, /* 0124: 01|24; 02|14 in 1 */
    {3, 1, 0, 1}, /* 0125 */
    {3, 0, 1, 1}, /* 0134: 01|34; 13|04 in 1 */
    {3, 0, 1, 1}, /* 0135 */
    {4, 0, 0, 1}, /* 0145: 01|45 in all but the star */
    {1, 0, 2, 2}, /* 0234: 23|04 in 0, 4; 02|34 in 1 */
    {1, 0, 2, 2}, /* 0235 */
    {3, 0, 0, 2}, /* 0245: 02|45 in 0, 1, 4 */
    {3, 0, 0, 2}, /* 0345 */
    {0, 1, 2, 2}, /* 1234: 23|14 in 0, 4; 13|24 in 1 */
    {0, 1, 2, 2}, /* 1235 */
    {3, 0, 0, 2}, /* 1245 */
    {3, 0, 0, 2}, /* 1345 */
    {3, 0, 0, 2}, /* 2345: 23|45 in 0, 1, 4 */
};

/* (quartets, res, top, dif) of every taxon from the counts rows, top and second by comparisons written out */
static void sums_of(int32_t T, const int32_t *quart, const uint16_t *counts, int64_t Q, uint64_t *acc)
{
    memset(acc, 0, sizeof(uint64_t) * 4 * (size_t)T);
    for (int64_t i = 0; i < Q; ++i) {
        uint32_t n[3] = {counts[4 * i], counts[4 * i + 1], counts[4 * i + 2]};
        for (int x = 0; x < 2; ++x)             /* descending */
            for (int y = 0; y < 2 - x; ++y)
                if (n[y] < n[y + 1]) { const uint32_t s = n[y]; n[y] = n[y + 1]; n[y + 1] = s; }
        for (int k = 0; k < 4; ++k) {
            uint64_t *a = acc + 4 * (size_t)quart[4 * i + k];
            a[0] += 1;
            a[1] += n[0] + n[1] + n[2];
            a[2] += n[0];
            a[3] += n[0] - n[1];
        }
    }
}

/* 1 when the tree displays a,b|c,d */
static int displays(int32_t T, const uint8_t *below, int64_t n, int a, int b, int c, int d)
{
    for (int64_t v = 0; v < n; ++v) {
        const uint8_t *s = below + (size_t)v * T;
        if ((s[a] && s[b] && !s[c] && !s[d]) || (s[c] && s[d] && !s[a] && !s[b])) return 1;
    }
    return 0;
}

static int code_of(int32_t T, const uint8_t *below, int64_t n, const int32_t *q)
{
    if (displays(T, below, n, q[0], q[1], q[2], q[3])) return 0;
    if (displays(T, below, n, q[0], q[2], q[1], q[3])) return 1;
    if (displays(T, below, n, q[0], q[3], q[1], q[2])) return 2;
    return 3;
}

/* random joins of two subtrees (three now and then), a unary node now and then; room for 3 T nodes */
static int64_t make_tree(int32_t T, int polytomies, int32_t *parent)
{
    int32_t n = T, nroots = T;
    int32_t *roots = (int32_t *)malloc(sizeof(int32_t) * (size_t)T);
    CHECK(roots);
    for (int32_t t = 0; t < T; ++t) { roots[t] = t; parent[t] = -1; }
    while (nroots > 1) {
        const int32_t k = (polytomies && nroots >= 3 && rnd(3) == 0) ? 3 : 2;
        int32_t v = n++;
        parent[v] = -1;
        for (int32_t j = 0; j < k; ++j) {
            const uint32_t p = rnd((uint32_t)nroots);
            parent[roots[p]] = v;
            roots[p] = roots[--nroots];
        }
        if (rnd(10) == 0) { parent[v] = n; v = n++; parent[v] = -1; }
        roots[nroots++] = v;
    }
    free(roots);
    return n;
}

static void run_random(int32_t T, int64_t Q)
{
    enum { R = 7 };
    const int64_t stride = 3 * (int64_t)T + 4;
    int32_t *reps = (int32_t *)malloc(sizeof(int32_t) * (size_t)(R * stride));
    uint8_t *below = (uint8_t *)calloc((size_t)R * (size_t)stride * (size_t)T, 1);
    int32_t *quart = (int32_t *)malloc(sizeof(int32_t) * 4 * (size_t)Q);
    uint16_t *want = (uint16_t *)calloc(4 * (size_t)Q, sizeof(uint16_t));
    uint16_t *got = (uint16_t *)malloc(sizeof(uint16_t) * 4 * (size_t)Q);
    uint64_t *acc_want = (uint64_t *)malloc(sizeof(uint64_t) * 4 * (size_t)T);
    uint64_t *acc_got = (uint64_t *)malloc(sizeof(uint64_t) * 4 * (size_t)T);
    int64_t n_nodes[R];
    CHECK(reps && below && quart && want && got && acc_want && acc_got);
    for (int r = 0; r < R; ++r) {
        int32_t *t = reps + r * stride;
        for (int64_t i = 0; i < stride; ++i) t[i] = -1;
        if (r == 5) { memcpy(t, reps + 3 * stride, sizeof(int32_t) * (size_t)stride); n_nodes[r] = n_nodes[3]; }
        else n_nodes[r] = make_tree(T, r & 1, t);
        CHECK(n_nodes[r] <= stride);
        uint8_t *bl = below + (size_t)r * stride * T;
        for (int32_t x = 0; x < T; ++x)
            for (int32_t v = x; v >= 0; v = t[v]) bl[(size_t)v * T + x] = 1;
    }
    for (int64_t i = 0; i < Q; ++i) {       /* four distinct taxa in any order; a row may come again */
        int32_t *q = quart + 4 * i;
        for (int k = 0; k < 4; ++k) {
            int again = 1;
            while (again) {
                q[k] = (int32_t)rnd((uint32_t)T);
                again = 0;
                for (int j = 0; j < k; ++j) again |= q[j] == q[k];
            }
        }
        for (int r = 0; r < R; ++r) want[4 * i + code_of(T, below + (size_t)r * stride * T, n_nodes[r], q)] += 1;
    }
    sums_of(T, quart, want, Q, acc_want);
    tq_ls *acc = NULL;
    int64_t gT = -1, nt = -1;
    uint64_t nq = 99;
    CHECK(tq_ls_create(&acc, T, R, NULL) == TQ_OK && acc);
    CHECK(tq_ls_shape(acc, &gT, &nt, &nq) == TQ_OK && gT == T && nt == 0 && nq == 0);
    /* nothing added: R = 0, and scores of no trees are no-ops that leave the array alone */
    CHECK(tq_ls_add(acc, NULL, NULL, 0, 0, NULL) == TQ_OK);
    got[0] = 777;
    CHECK(tq_ls_score(acc, quart, Q, got, NULL) == TQ_OK && tq_ls_score_ranks(acc, NULL, 0, 1, got, NULL) == TQ_OK);
    CHECK(got[0] == 777 && tq_ls_shape(acc, NULL, &nt, &nq) == TQ_OK && nt == 0 && nq == 0);
    CHECK(tq_ls_read(acc, acc_got) == TQ_OK);
    for (int i = 0; i < 4 * T; ++i) CHECK(acc_got[i] == 0);
    /* all at once, recounted */
    CHECK(tq_ls_add(acc, reps, n_nodes, R, stride, NULL) == TQ_OK);
    CHECK(tq_ls_score(acc, quart, 0, got, NULL) == TQ_OK && got[0] == 777);
    CHECK(tq_ls_score(acc, quart, Q, got, NULL) == TQ_OK);
    CHECK(tq_ls_shape(acc, NULL, &nt, &nq) == TQ_OK && nt == R && nq == (uint64_t)Q);
    CHECK(!memcmp(got, want, sizeof(uint16_t) * 4 * (size_t)Q));
    for (int64_t i = 0; i < Q; ++i) CHECK(got[4 * i] + got[4 * i + 1] + got[4 * i + 2] + got[4 * i + 3] == R);
    CHECK(tq_ls_read(acc, acc_got) == TQ_OK && !memcmp(acc_got, acc_want, sizeof(uint64_t) * 4 * (size_t)T));
    /* clear keeps the trees; three calls, two of them without an array, make the same sums */
    CHECK(tq_ls_clear(acc) == TQ_OK && tq_ls_shape(acc, NULL, &nt, &nq) == TQ_OK && nt == R && nq == 0);
    CHECK(tq_ls_read(acc, acc_got) == TQ_OK);
    for (int i = 0; i < 4 * T; ++i) CHECK(acc_got[i] == 0);
    memset(got, 0xEE, sizeof(uint16_t) * 4 * (size_t)Q);
    CHECK(tq_ls_score(acc, quart, Q / 3, NULL, NULL) == TQ_OK);
    CHECK(tq_ls_score(acc, quart + 4 * (Q / 3), 1, got + 4 * (Q / 3), NULL) == TQ_OK);
    CHECK(tq_ls_score(acc, quart + 4 * (Q / 3 + 1), Q - Q / 3 - 1, NULL, NULL) == TQ_OK);
    CHECK(!memcmp(got + 4 * (Q / 3), want + 4 * (Q / 3), sizeof(uint16_t) * 4) && got[4 * (Q / 3 + 1)] == 0xEEEE);
    CHECK(tq_ls_read(acc, acc_got) == TQ_OK && tq_ls_read(acc, acc_got) == TQ_OK);
    CHECK(!memcmp(acc_got, acc_want, sizeof(uint64_t) * 4 * (size_t)T));
    /* refusals: nothing of the call is added or scored */
    {
        int32_t *bad = (int32_t *)malloc(sizeof(int32_t) * 4 * 8);
        uint64_t rk[3] = {0, 0, 1};
        int64_t st[7] = {-1, -1, -1, -1, -1, -1, -1};
        CHECK(bad);
        memcpy(bad, quart, sizeof(int32_t) * 4 * 8);
        bad[4 * 5 + 2] = bad[4 * 5 + 1];
        CHECK(tq_ls_score(acc, bad, 8, got, NULL) == TQ_ERR_INVALID_ARG && strstr(tq_last_error(NULL), "tq_ls_score: quartet 5: repeated taxon"));
        bad[4 * 5 + 2] = T;
        CHECK(tq_ls_score(acc, bad, 8, NULL, NULL) == TQ_ERR_INVALID_ARG && strstr(tq_last_error(NULL), "quartet 5: taxon out of range"));
        bad[4 * 5 + 2] = -1;
        CHECK(tq_ls_score(acc, bad, 8, NULL, NULL) == TQ_ERR_INVALID_ARG);
        rk[1] = (uint64_t)T * (T - 1) / 2 * (T - 2) / 3 * (T - 3) / 4;
        CHECK(tq_ls_score_ranks(acc, rk, 0, 3, got, NULL) == TQ_ERR_INVALID_ARG && strstr(tq_last_error(NULL), "tq_ls_score_ranks: rank 1"));
        CHECK(tq_ls_score_ranks(acc, NULL, rk[1] - 1, 2, NULL, NULL) == TQ_ERR_INVALID_ARG && strstr(tq_last_error(NULL), "rank range"));
        CHECK(tq_ls_score_ranks(acc, NULL, rk[1] + 5, 1, NULL, NULL) == TQ_ERR_INVALID_ARG);
        CHECK(tq_ls_score_ranks(acc, NULL, 0, -1, NULL, NULL) == TQ_ERR_INVALID_ARG && tq_ls_score(acc, NULL, 3, NULL, NULL) == TQ_ERR_INVALID_ARG);
        CHECK(tq_ls_add(acc, reps, n_nodes, 1, stride, NULL) == TQ_ERR_INVALID_ARG && strstr(tq_last_error(NULL), "tq_ls_add: quartets have been scored"));
        CHECK(tq_ls_read(acc, NULL) == TQ_ERR_INVALID_ARG);
        CHECK(!memcmp(got + 4 * (Q / 3), want + 4 * (Q / 3), sizeof(uint16_t) * 4));
        CHECK(tq_ls_read(acc, acc_got) == TQ_OK && !memcmp(acc_got, acc_want, sizeof(uint64_t) * 4 * (size_t)T));
        CHECK(tq_ls_shape(acc, NULL, &nt, &nq) == TQ_OK && nt == R && nq == (uint64_t)Q);
        CHECK(tq_ls_stats(acc, st) == TQ_OK && st[0] == 64 * st[4] && st[1] >= 4 && st[2] == R && st[3] == 0 && st[5] == 0 && st[6] > 0);
        free(bad);
    }
    /* reset; bad trees; too many trees */
    CHECK(tq_ls_reset(acc) == TQ_OK && tq_ls_shape(acc, NULL, &nt, &nq) == TQ_OK && nt == 0 && nq == 0);
    CHECK(tq_ls_add(acc, reps, n_nodes, R - 3, stride, NULL) == TQ_OK);
    {
        int32_t *bad = (int32_t *)malloc(sizeof(int32_t) * (size_t)(3 * stride));
        int64_t nn[3] = {n_nodes[3], n_nodes[4] + 2, n_nodes[5]};
        CHECK(bad);
        memcpy(bad, reps + 3 * stride, sizeof(int32_t) * (size_t)(3 * stride));
        CHECK(n_nodes[4] + 2 <= stride);
        bad[stride + n_nodes[4]] = (int32_t)n_nodes[4] + 1;         /* a cycle of two nodes beside tree 1 */
        bad[stride + n_nodes[4] + 1] = (int32_t)n_nodes[4];
        CHECK(tq_ls_add(acc, bad, nn, 3, stride, NULL) == TQ_ERR_INVALID_ARG && strstr(tq_last_error(NULL), "tq_ls_add: tree 1"));
        nn[1] = stride + 1;
        CHECK(tq_ls_add(acc, bad, nn, 3, stride, NULL) == TQ_ERR_INVALID_ARG && strstr(tq_last_error(NULL), "stride"));
        CHECK(tq_ls_add(acc, reps, n_nodes, 4, stride, NULL) == TQ_ERR_INVALID_ARG && strstr(tq_last_error(NULL), "max_trees"));
        CHECK(tq_ls_add(acc, NULL, nn, 3, stride, NULL) == TQ_ERR_INVALID_ARG && tq_ls_add(acc, bad, NULL, 3, stride, NULL) == TQ_ERR_INVALID_ARG);
        CHECK(tq_ls_add(acc, bad, nn, -1, stride, NULL) == TQ_ERR_INVALID_ARG && tq_ls_add(NULL, bad, nn, 3, stride, NULL) == TQ_ERR_INVALID_ARG);
        CHECK(tq_ls_shape(acc, NULL, &nt, NULL) == TQ_OK && nt == R - 3);
        /* the first R - 3 trees alone: the recount again without the last three */
        memset(want, 0, sizeof(uint16_t) * 4 * (size_t)Q);
        for (int64_t i = 0; i < Q; ++i)
            for (int r = 0; r < R - 3; ++r) want[4 * i + code_of(T, below + (size_t)r * stride * T, n_nodes[r], quart + 4 * i)] += 1;
        sums_of(T, quart, want, Q, acc_want);
        CHECK(tq_ls_score(acc, quart, Q, got, NULL) == TQ_OK && tq_ls_read(acc, acc_got) == TQ_OK);
        CHECK(!memcmp(got, want, sizeof(uint16_t) * 4 * (size_t)Q) && !memcmp(acc_got, acc_want, sizeof(uint64_t) * 4 * (size_t)T));
        free(bad);
    }
    tq_ls_destroy(acc);
    free(acc_got); free(acc_want); free(got); free(want); free(quart); free(below); free(reps);
}

/* the six-taxon trees over all 15 quartets, against the table written by hand */
static void run_six(void)
{
    tq_ls *acc = NULL;
    uint16_t got[Q6 * 4], perm[Q6 * 4];
    uint64_t sums[T6 * 4], want[T6 * 4], sums2[T6 * 4];
    int32_t q[Q6 * 4], qp[Q6 * 4];
    uint64_t rk[Q6], nq = 0;
    int n = 0;
    for (int a = 0; a < 6; ++a)
        for (int b = a + 1; b < 6; ++b)
            for (int c = b + 1; c < 6; ++c)
                for (int d = c + 1; d < 6; ++d) {
                    q[4 * n] = a; q[4 * n + 1] = b; q[4 * n + 2] = c; q[4 * n + 3] = d;
                    qp[4 * n] = d; qp[4 * n + 1] = a; qp[4 * n + 2] = c; qp[4 * n + 3] = b;     /* (d, a, c, b) */
                    ++n;
                }
    CHECK(n == Q6);
    sums_of(T6, q, &want6[0][0], Q6, want);
    /* every taxon is in C(5,3) = 10 quartets; res by hand: the resolved entries of the rows that hold the taxon */
    for (int t = 0; t < T6; ++t) CHECK(want[4 * t] == 10);
    CHECK(want[4 * 0 + 1] == 6 * 4 + 4 * 3);        /* taxon 0: the six rows with 0 and 1 at 4, 02xy and 03xy at 3 */
    CHECK(want[4 * 5 + 1] == 3 * 4 + 7 * 3);        /* taxon 5: 0125, 0135, 0145 at 4, the other seven at 3 */
    CHECK(tq_ls_create(&acc, T6, N6, NULL) == TQ_OK);
    CHECK(tq_ls_add(acc, &trees6[0][0], nodes6, N6, STRIDE6, NULL) == TQ_OK);
    CHECK(tq_ls_score_ranks(acc, NULL, 0, Q6, got, NULL) == TQ_OK);
    CHECK(tq_ls_read(acc, sums) == TQ_OK && tq_ls_shape(acc, NULL, NULL, &nq) == TQ_OK && nq == Q6);
    CHECK(!memcmp(got, want6, sizeof got) && !memcmp(sums, want, sizeof sums));
    /* the same quartets as explicit ranks, backwards; as taxa in the order (d, a, c, b), which turns ab|cd into ad|bc of
     * the new row, ac|bd into ... written out: new (a', b', c', d') = (d, a, c, b); a'b'|c'd' = da|cb = old ad|bc (2),
     * a'c'|b'd' = dc|ab = old ab|cd (0), a'd'|b'c' = db|ac = old ac|bd (1) */
    for (int i = 0; i < Q6; ++i) rk[i] = (uint64_t)(Q6 - 1 - i);
    CHECK(tq_ls_clear(acc) == TQ_OK && tq_ls_score_ranks(acc, rk, 0, Q6, got, NULL) == TQ_OK);
    for (int i = 0; i < Q6; ++i) CHECK(!memcmp(got + 4 * i, want6[Q6 - 1 - i], 8));
    CHECK(tq_ls_read(acc, sums2) == TQ_OK && !memcmp(sums, sums2, sizeof sums));
    CHECK(tq_ls_clear(acc) == TQ_OK && tq_ls_score(acc, qp, Q6, perm, NULL) == TQ_OK);
    for (int i = 0; i < Q6; ++i)
        CHECK(perm[4 * i] == want6[i][2] && perm[4 * i + 1] == want6[i][0] && perm[4 * i + 2] == want6[i][1] && perm[4 * i + 3] == want6[i][3]);
    CHECK(tq_ls_read(acc, sums2) == TQ_OK && !memcmp(sums, sums2, sizeof sums));
    /* a range in two calls; then the first row once more: it counts twice */
    CHECK(tq_ls_clear(acc) == TQ_OK && tq_ls_score_ranks(acc, NULL, 0, 7, got, NULL) == TQ_OK);
    CHECK(tq_ls_score_ranks(acc, NULL, 7, 8, got + 4 * 7, NULL) == TQ_OK && !memcmp(got, want6, sizeof got));
    CHECK(tq_ls_read(acc, sums2) == TQ_OK && !memcmp(sums, sums2, sizeof sums));
    CHECK(tq_ls_score(acc, q, 1, NULL, NULL) == TQ_OK && tq_ls_read(acc, sums2) == TQ_OK);
    for (int t = 0; t < T6; ++t) {          /* row 0123 = (3, 1, 0, 1): res 4, top 3, dif 2 */
        const uint64_t in = t < 4;
        CHECK(sums2[4 * t] == sums[4 * t] + in && sums2[4 * t + 1] == sums[4 * t + 1] + 4 * in);
        CHECK(sums2[4 * t + 2] == sums[4 * t + 2] + 3 * in && sums2[4 * t + 3] == sums[4 * t + 3] + 2 * in);
    }
    tq_ls_destroy(acc);
}

int main(void)
{
    {   /* outside the limits */
        tq_ls *acc = (tq_ls *)&state;
        CHECK(tq_ls_create(&acc, 3, 4, NULL) == TQ_ERR_INVALID_ARG && acc == NULL);
        acc = (tq_ls *)&state;
        CHECK(tq_ls_create(&acc, 1025, 4, NULL) == TQ_ERR_INVALID_ARG && acc == NULL);
        CHECK(strstr(tq_last_error(NULL), "tq_ls_create: T must be 4..1024"));
        CHECK(tq_ls_create(&acc, 8, 0, NULL) == TQ_ERR_INVALID_ARG && tq_ls_create(&acc, 8, 8193, NULL) == TQ_ERR_INVALID_ARG);
        CHECK(strstr(tq_last_error(NULL), "max_trees"));
        CHECK(tq_ls_create(NULL, 8, 4, NULL) == TQ_ERR_INVALID_ARG);
        CHECK(tq_ls_reset(NULL) == TQ_ERR_INVALID_ARG && tq_ls_clear(NULL) == TQ_ERR_INVALID_ARG);
        CHECK(tq_ls_shape(NULL, NULL, NULL, NULL) == TQ_ERR_INVALID_ARG && tq_ls_read(NULL, NULL) == TQ_ERR_INVALID_ARG);
        CHECK(tq_ls_stats(NULL, NULL) == TQ_ERR_INVALID_ARG && tq_ls_score(NULL, NULL, 0, NULL, NULL) == TQ_ERR_INVALID_ARG);
        CHECK(tq_ls_score_ranks(NULL, NULL, 0, 0, NULL, NULL) == TQ_ERR_INVALID_ARG);
        tq_ls_destroy(NULL);
    }
    run_six();
    run_random(4, 40);
    run_random(12, 300);
    run_random(65, 700);
    run_random(129, 70000);             /* more than one host chunk of 65 536 quartets */
    printf("stability_host_check: ok\n");
    return 0;
}

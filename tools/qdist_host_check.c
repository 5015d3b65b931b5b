/* qdist_host_check.c -- the host back end of the quartet distance accumulator (tq_qd_* without a context, DESIGN.md
 * section 27), driven from a plain C program.
 * Built and run under the host sanitizers by tools/host_checks.sh.
 *
 * No device is needed or touched.  The word rule is recounted from a loop over the bits; the matrices of a few
 * hard-coded trees are known by hand, and those of random trees are recounted from taxon sets: a tree displays a,b|c,d
 * when some node has a and b below it and neither c nor d, or c and d and neither a nor b.
 * Prints "qdist_host_check: ok" and returns 0 when every check held; a sanitizer report or a failed check ends it with
 * a non-zero status. */
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

#define CHECK(cond)                                                               \
    do {                                                                          \
        if (!(cond)) {                                                            \
            fprintf(stderr, "qdist_host_check: line %d: %s\n", __LINE__, #cond);  \
            exit(1);                                                              \
        }                                                                         \
    } while (0)

/* six taxa.  ((0,1),(2,3),(4,5)); ((0,2),(1,3),(4,5)); the star; ((0,1),2,3,4,5) under a root of degree 2 with a unary
 * node; the first tree again, rooted on the edge above (4,5). */
enum { T6 = 6, N6 = 5, STRIDE6 = 12 };
static const int32_t trees6[N6][STRIDE6] = {
    {6, 6, 7, 7, 8, 8, 9, 9, 9, -1, -1, -1},
    {6, 7, 6, 7, 8, 8, 9, 9, 9, -1, -1, -1},
    {6, 6, 6, 6, 6, 6, -1, -1, -1, -1, -1, -1},
    {6, 6, 8, 8, 8, 8, 7, 9, 9, -1, -1, -1},
    {6, 6, 7, 7, 8, 8, 9, 9, 10, 10, -1, -1},
};
static const int64_t nodes6[N6] = {10, 10, 7, 10, 11};

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
    uint8_t *codes = (uint8_t *)malloc((size_t)R * (size_t)Q);
    int64_t n_nodes[R];
    uint64_t same[R * R], both[R * R], same2[R * R], both2[R * R];
    CHECK(reps && below && quart && codes);
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
    for (int64_t i = 0; i < Q; ++i) {       /* four distinct taxa in any order */
        int32_t *q = quart + 4 * i;
        for (int k = 0; k < 4; ++k) {
            int again = 1;
            while (again) {
                q[k] = (int32_t)rnd((uint32_t)T);
                again = 0;
                for (int j = 0; j < k; ++j) again |= q[j] == q[k];
            }
        }
        for (int r = 0; r < R; ++r) codes[(size_t)r * Q + i] = (uint8_t)code_of(T, below + (size_t)r * stride * T, n_nodes[r], q);
    }
    tq_qd *acc = NULL;
    int64_t gT = -1, nt = -1;
    uint64_t nq = 99;
    CHECK(tq_qd_create(&acc, T, R, NULL) == TQ_OK && acc);
    CHECK(tq_qd_shape(acc, &gT, &nt, &nq) == TQ_OK && gT == T && nt == 0 && nq == 0);
    /* nothing added: R = 0, scores and reads of no trees are no-ops */
    CHECK(tq_qd_add(acc, NULL, NULL, 0, 0, NULL) == TQ_OK);
    CHECK(tq_qd_score(acc, quart, Q, NULL) == TQ_OK && tq_qd_score_ranks(acc, NULL, 0, 1, NULL) == TQ_OK);
    same[0] = 77;
    CHECK(tq_qd_read(acc, same, NULL) == TQ_OK && same[0] == 77 && tq_qd_read(acc, NULL, NULL) == TQ_OK);
    CHECK(tq_qd_shape(acc, NULL, &nt, &nq) == TQ_OK && nt == 0 && nq == 0);
    /* all at once, recounted */
    CHECK(tq_qd_add(acc, reps, n_nodes, R, stride, NULL) == TQ_OK);
    CHECK(tq_qd_read(acc, same, both) == TQ_OK);
    for (int i = 0; i < R * R; ++i) CHECK(same[i] == 0 && both[i] == 0);
    CHECK(tq_qd_score(acc, quart, Q, NULL) == TQ_OK && tq_qd_score(acc, quart, 0, NULL) == TQ_OK);
    CHECK(tq_qd_read(acc, same, both) == TQ_OK);
    CHECK(tq_qd_shape(acc, NULL, &nt, &nq) == TQ_OK && nt == R && nq == (uint64_t)Q);
    for (int i = 0; i < R; ++i)
        for (int j = 0; j < R; ++j) {
            uint64_t s = 0, b = 0;
            for (int64_t k = 0; k < Q; ++k) {
                const int x = codes[(size_t)i * Q + k], y = codes[(size_t)j * Q + k];
                s += x < 3 && x == y;
                b += x < 3 && y < 3;
            }
            CHECK(same[i * R + j] == s && both[i * R + j] == b);
        }
    CHECK(same[3 * R + 5] == both[3 * R + 3] && both[0] == (uint64_t)Q);    /* a tree and its copy; a binary tree */
    /* clear keeps the trees; three calls make the same matrices; an add is possible again only after the clear */
    CHECK(tq_qd_add(acc, reps, n_nodes, 0, stride, NULL) == TQ_OK);
    CHECK(tq_qd_clear(acc) == TQ_OK && tq_qd_shape(acc, NULL, &nt, &nq) == TQ_OK && nt == R && nq == 0);
    CHECK(tq_qd_score(acc, quart, Q / 3, NULL) == TQ_OK);
    CHECK(tq_qd_read(acc, NULL, both2) == TQ_OK);
    CHECK(tq_qd_score(acc, quart + 4 * (Q / 3), 1, NULL) == TQ_OK);
    CHECK(tq_qd_score(acc, quart + 4 * (Q / 3 + 1), Q - Q / 3 - 1, NULL) == TQ_OK);
    CHECK(tq_qd_read(acc, same2, both2) == TQ_OK && tq_qd_read(acc, same2, both2) == TQ_OK);
    CHECK(!memcmp(same, same2, sizeof same) && !memcmp(both, both2, sizeof both));
    /* refusals: nothing of the call is added or scored */
    {
        int32_t *bad = (int32_t *)malloc(sizeof(int32_t) * 4 * 8);
        uint64_t rk[3] = {0, 0, 1};
        int64_t st[6] = {-1, -1, -1, -1, -1, -1};
        CHECK(bad);
        memcpy(bad, quart, sizeof(int32_t) * 4 * 8);
        bad[4 * 5 + 2] = bad[4 * 5 + 1];
        CHECK(tq_qd_score(acc, bad, 8, NULL) == TQ_ERR_INVALID_ARG && strstr(tq_last_error(NULL), "quartet 5: repeated taxon"));
        bad[4 * 5 + 2] = T;
        CHECK(tq_qd_score(acc, bad, 8, NULL) == TQ_ERR_INVALID_ARG && strstr(tq_last_error(NULL), "quartet 5: taxon out of range"));
        bad[4 * 5 + 2] = -1;
        CHECK(tq_qd_score(acc, bad, 8, NULL) == TQ_ERR_INVALID_ARG);
        rk[1] = (uint64_t)T * (T - 1) / 2 * (T - 2) / 3 * (T - 3) / 4;
        CHECK(tq_qd_score_ranks(acc, rk, 0, 3, NULL) == TQ_ERR_INVALID_ARG && strstr(tq_last_error(NULL), "rank 1"));
        CHECK(tq_qd_score_ranks(acc, NULL, rk[1] - 1, 2, NULL) == TQ_ERR_INVALID_ARG && strstr(tq_last_error(NULL), "rank range"));
        CHECK(tq_qd_score_ranks(acc, NULL, rk[1] + 5, 1, NULL) == TQ_ERR_INVALID_ARG);
        CHECK(tq_qd_score_ranks(acc, NULL, 0, -1, NULL) == TQ_ERR_INVALID_ARG && tq_qd_score(acc, NULL, 3, NULL) == TQ_ERR_INVALID_ARG);
        CHECK(tq_qd_add(acc, reps, n_nodes, 1, stride, NULL) == TQ_ERR_INVALID_ARG && strstr(tq_last_error(NULL), "scored"));
        CHECK(tq_qd_read(acc, same2, both2) == TQ_OK && !memcmp(same, same2, sizeof same) && !memcmp(both, both2, sizeof both));
        CHECK(tq_qd_shape(acc, NULL, &nt, &nq) == TQ_OK && nt == R && nq == (uint64_t)Q);
        CHECK(tq_qd_stats(acc, st) == TQ_OK && st[0] == 64 * st[5] && st[1] >= 4 && st[2] == 0 && st[3] == R && st[4] == 0);
        free(bad);
    }
    /* reset; bad trees; too many trees */
    CHECK(tq_qd_reset(acc) == TQ_OK && tq_qd_shape(acc, NULL, &nt, &nq) == TQ_OK && nt == 0 && nq == 0);
    CHECK(tq_qd_add(acc, reps, n_nodes, R - 3, stride, NULL) == TQ_OK);
    {
        int32_t *bad = (int32_t *)malloc(sizeof(int32_t) * (size_t)(3 * stride));
        int64_t nn[3] = {n_nodes[3], n_nodes[4] + 2, n_nodes[5]};
        CHECK(bad);
        memcpy(bad, reps + 3 * stride, sizeof(int32_t) * (size_t)(3 * stride));
        CHECK(n_nodes[4] + 2 <= stride);
        bad[stride + n_nodes[4]] = (int32_t)n_nodes[4] + 1;         /* a cycle of two nodes beside tree 1 */
        bad[stride + n_nodes[4] + 1] = (int32_t)n_nodes[4];
        CHECK(tq_qd_add(acc, bad, nn, 3, stride, NULL) == TQ_ERR_INVALID_ARG && strstr(tq_last_error(NULL), "tq_qd_add: tree 1"));
        nn[1] = stride + 1;
        CHECK(tq_qd_add(acc, bad, nn, 3, stride, NULL) == TQ_ERR_INVALID_ARG && strstr(tq_last_error(NULL), "stride"));
        CHECK(tq_qd_add(acc, reps, n_nodes, 4, stride, NULL) == TQ_ERR_INVALID_ARG && strstr(tq_last_error(NULL), "max_trees"));
        CHECK(tq_qd_add(acc, NULL, nn, 3, stride, NULL) == TQ_ERR_INVALID_ARG && tq_qd_add(acc, bad, NULL, 3, stride, NULL) == TQ_ERR_INVALID_ARG);
        CHECK(tq_qd_add(acc, bad, nn, -1, stride, NULL) == TQ_ERR_INVALID_ARG && tq_qd_add(NULL, bad, nn, 3, stride, NULL) == TQ_ERR_INVALID_ARG);
        CHECK(tq_qd_shape(acc, NULL, &nt, NULL) == TQ_OK && nt == R - 3);
        CHECK(tq_qd_score(acc, quart, Q, NULL) == TQ_OK && tq_qd_read(acc, same2, both2) == TQ_OK);
        for (int i = 0; i < R - 3; ++i)
            for (int j = 0; j < R - 3; ++j)
                CHECK(same2[i * (R - 3) + j] == same[i * R + j] && both2[i * (R - 3) + j] == both[i * R + j]);
        free(bad);
    }
    tq_qd_destroy(acc);
    free(codes); free(quart); free(below); free(reps);
}

/* the six-taxon trees over all 15 quartets, by ranks: by hand, tree 0 resolves the 12 quartets that take two taxa of
 * one cherry, tree 1 likewise; they agree on the 4 quartets with 4 and 5 and two of {0,1,2,3} that are no cherry of
 * either... counted below from the taxon sets instead. */
static void run_six(void)
{
    tq_qd *acc = NULL;
    uint64_t same[N6 * N6], both[N6 * N6], same2[N6 * N6], both2[N6 * N6];
    uint64_t nq = 0;
    CHECK(tq_qd_create(&acc, T6, N6, NULL) == TQ_OK);
    CHECK(tq_qd_add(acc, &trees6[0][0], nodes6, N6, STRIDE6, NULL) == TQ_OK);
    CHECK(tq_qd_score_ranks(acc, NULL, 0, 15, NULL) == TQ_OK);
    CHECK(tq_qd_read(acc, same, both) == TQ_OK && tq_qd_shape(acc, NULL, NULL, &nq) == TQ_OK && nq == 15);
    /* resolved: three cherries leave only (one of each cherry... ) none unresolved but the 8 quartets a,b,c,d with one
     * cherry whole: every quartet of 6 taxa in 3 cherries holds a whole cherry (pigeonhole), so 15; the star 0;
     * ((0,1),2,3,4,5): the C(4,2) = 6 quartets with 0 and 1 */
    CHECK(both[0 * N6 + 0] == 15 && both[1 * N6 + 1] == 15 && both[2 * N6 + 2] == 0 && both[3 * N6 + 3] == 6);
    CHECK(both[4 * N6 + 4] == 15 && same[0 * N6 + 4] == 15);       /* rerooting changes nothing */
    /* trees 0 and 1 agree on the quartets that hold 4 and 5: C(4,2) = 6, and on {0,1,2,3}?  01|23 against 02|13: no. */
    CHECK(same[0 * N6 + 1] == 6 && both[0 * N6 + 1] == 15);
    /* tree 3 displays 0,1|x,y; so does tree 0 for all 6; tree 1 for the one with 4,5 only (as 4,5|0,1) */
    CHECK(same[0 * N6 + 3] == 6 && both[0 * N6 + 3] == 6 && same[1 * N6 + 3] == 1 && both[1 * N6 + 3] == 6);
    for (int i = 0; i < N6; ++i) {
        CHECK(same[i * N6 + i] == both[i * N6 + i] && both[2 * N6 + i] == 0 && same[i * N6 + 2] == 0);
        for (int j = 0; j < N6; ++j) CHECK(same[i * N6 + j] == same[j * N6 + i] && both[i * N6 + j] == both[j * N6 + i]);
    }
    /* the same quartets as explicit ranks, backwards, and as taxa in another order */
    {
        uint64_t rk[15];
        int32_t q[15 * 4];
        int n = 0;
        for (int i = 0; i < 15; ++i) rk[i] = (uint64_t)(14 - i);
        for (int a = 0; a < 6; ++a)
            for (int b = a + 1; b < 6; ++b)
                for (int c = b + 1; c < 6; ++c)
                    for (int d = c + 1; d < 6; ++d) { q[4 * n] = d; q[4 * n + 1] = a; q[4 * n + 2] = c; q[4 * n + 3] = b; ++n; }
        CHECK(n == 15);
        CHECK(tq_qd_clear(acc) == TQ_OK && tq_qd_score_ranks(acc, rk, 0, 15, NULL) == TQ_OK);
        CHECK(tq_qd_read(acc, same2, both2) == TQ_OK && !memcmp(same, same2, sizeof same) && !memcmp(both, both2, sizeof both));
        CHECK(tq_qd_clear(acc) == TQ_OK && tq_qd_score(acc, q, 15, NULL) == TQ_OK);
        CHECK(tq_qd_read(acc, same2, both2) == TQ_OK && !memcmp(same, same2, sizeof same) && !memcmp(both, both2, sizeof both));
        CHECK(tq_qd_clear(acc) == TQ_OK && tq_qd_score_ranks(acc, NULL, 0, 7, NULL) == TQ_OK);
        CHECK(tq_qd_score_ranks(acc, NULL, 7, 8, NULL) == TQ_OK);
        CHECK(tq_qd_read(acc, same2, both2) == TQ_OK && !memcmp(same, same2, sizeof same) && !memcmp(both, both2, sizeof both));
    }
    tq_qd_destroy(acc);
}

int main(void)
{
    {   /* outside the limits */
        tq_qd *acc = (tq_qd *)&state;
        CHECK(tq_qd_create(&acc, 3, 4, NULL) == TQ_ERR_INVALID_ARG && acc == NULL);
        acc = (tq_qd *)&state;
        CHECK(tq_qd_create(&acc, 1025, 4, NULL) == TQ_ERR_INVALID_ARG && acc == NULL);
        CHECK(strstr(tq_last_error(NULL), "T must be 4..1024"));
        CHECK(tq_qd_create(&acc, 8, 0, NULL) == TQ_ERR_INVALID_ARG && tq_qd_create(&acc, 8, 8193, NULL) == TQ_ERR_INVALID_ARG);
        CHECK(strstr(tq_last_error(NULL), "max_trees"));
        CHECK(tq_qd_create(NULL, 8, 4, NULL) == TQ_ERR_INVALID_ARG);
        CHECK(tq_qd_reset(NULL) == TQ_ERR_INVALID_ARG && tq_qd_clear(NULL) == TQ_ERR_INVALID_ARG);
        CHECK(tq_qd_shape(NULL, NULL, NULL, NULL) == TQ_ERR_INVALID_ARG && tq_qd_read(NULL, NULL, NULL) == TQ_ERR_INVALID_ARG);
        CHECK(tq_qd_stats(NULL, NULL) == TQ_ERR_INVALID_ARG && tq_qd_score(NULL, NULL, 0, NULL) == TQ_ERR_INVALID_ARG);
        CHECK(tq_qd_score_ranks(NULL, NULL, 0, 0, NULL) == TQ_ERR_INVALID_ARG);
        tq_qd_destroy(NULL);
    }
    for (int i = 0; i < 1000; ++i) {    /* the word rule against a loop over the bits; codes 0..3 per bit */
        uint64_t x[3] = {0, 0, 0}, y[3] = {0, 0, 0};
        uint32_t want_same = 0, want_both = 0, same = 99, both = 99;
        for (int b = 0; b < 64; ++b) {
            const uint32_t cx = i % 5 == 0 ? 0 : rnd(4), cy = i % 7 == 0 ? cx : rnd(4);
            if (cx < 3) x[cx] |= (uint64_t)1 << b;
            if (cy < 3) y[cy] |= (uint64_t)1 << b;
            want_same += cx < 3 && cx == cy;
            want_both += cx < 3 && cy < 3;
        }
        tq_qd_word_counts(x[0], x[1], x[2], y[0], y[1], y[2], &same, &both);
        CHECK(same == want_same && both == want_both);
        tq_qd_word_counts(x[0], x[1], x[2], y[0], y[1], y[2], NULL, NULL);
    }
    {
        uint32_t same = 0, both = 0;
        tq_qd_word_counts(~(uint64_t)0, 0, 0, ~(uint64_t)0, 0, 0, &same, &both);
        CHECK(same == 64 && both == 64);
        tq_qd_word_counts(~(uint64_t)0, 0, 0, 0, ~(uint64_t)0, 0, &same, &both);
        CHECK(same == 0 && both == 64);
        tq_qd_word_counts(0, 0, 0, 0, 0, ~(uint64_t)0, &same, &both);
        CHECK(same == 0 && both == 0);
    }
    run_six();
    run_random(4, 40);
    run_random(12, 300);
    run_random(65, 700);
    run_random(129, 70000);             /* more than one host chunk of 65 536 quartets */
    printf("qdist_host_check: ok\n");
    return 0;
}

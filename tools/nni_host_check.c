/* nni_host_check.c -- the host paths of the NNI scan and the polish search (tq_stree_nni_scan / tq_stree_polish on an
 * accumulator without a context), driven from a plain C program.
 * Built and run under the host sanitizers by tools/host_checks.sh.
 *
 * No device is needed or touched.  Scans are recounted from the corner masks the library reports (a row counts on an edge
 * when its four taxa fall one into each mask); polishes are checked through tq_stree_fit of the tree before and after.
 * Prints "nni_host_check: ok" and returns 0 when every check held; a sanitizer report or a failed check ends it with a
 * non-zero status. */
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

#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) {                                                               \
            fprintf(stderr, "nni_host_check: line %d: %s\n", __LINE__, #cond);       \
            exit(1);                                                                 \
        }                                                                            \
    } while (0)

enum { RANDOM = 0, CATERPILLAR = 1, STAR = 2, POLYTOMIES = 3 };

/* parent array of T taxa (room for 3 T nodes); random joins of two subtrees (three now and then with POLYTOMIES), a unary
 * node now and then; the root of a RANDOM tree has two children.  Returns the node count. */
static int64_t make_tree(int32_t T, int shape, int32_t *parent)
{
    int32_t n = T;
    if (shape == STAR) {
        for (int32_t t = 0; t < T; ++t) parent[t] = T;
        parent[T] = -1;
        return T + 1;
    }
    if (shape == CATERPILLAR) {
        int32_t cur = 0;
        for (int32_t t = 1; t < T; ++t) {
            parent[cur] = n;
            parent[t] = n;
            cur = n++;
        }
        parent[cur] = -1;
        return n;
    }
    int32_t *roots = (int32_t *)malloc(sizeof(int32_t) * (size_t)T);
    int32_t nroots = T;
    CHECK(roots);
    for (int32_t t = 0; t < T; ++t) { roots[t] = t; parent[t] = -1; }
    while (nroots > 1) {
        const int32_t k = (shape == POLYTOMIES && nroots >= 3 && rnd(3) == 0) ? 3 : 2;
        int32_t v = n++;
        parent[v] = -1;
        for (int32_t j = 0; j < k; ++j) {
            const uint32_t p = rnd((uint32_t)nroots);
            parent[roots[p]] = v;
            roots[p] = roots[--nroots];
        }
        if (nroots > 0 && rnd(10) == 0) { parent[v] = n; v = n++; parent[v] = -1; }    /* never above the last join: */
        roots[nroots++] = v;                                                            /* reroot() would leave it a tip */
    }
    free(roots);
    return n;
}

/* the same unrooted tree hung from internal node `at` */
static void reroot(int32_t *parent, int32_t at)
{
    int32_t prev = -1, v = at;
    while (v >= 0) {
        const int32_t up = parent[v];
        parent[v] = prev;
        prev = v;
        v = up;
    }
}

/* newick with numeric tips -> parent array (tips = their numbers, internal nodes T, T + 1, ... in order of '(') */
static int64_t parse_newick(const char *s, int64_t len, int32_t T, int32_t *parent)
{
    int32_t *stack = (int32_t *)malloc(sizeof(int32_t) * (size_t)(2 * T + 2));
    int32_t depth = 0, n = T;
    CHECK(stack);
    for (int64_t i = 0; i < len; ++i) {
        const char c = s[i];
        if (c == '(') {
            parent[n] = depth ? stack[depth - 1] : -1;
            stack[depth++] = n++;
        } else if (c == ')') {
            --depth;
        } else if (c >= '0' && c <= '9') {
            int32_t t = 0;
            while (i < len && s[i] >= '0' && s[i] <= '9') t = 10 * t + (s[i++] - '0');
            --i;
            CHECK(t < T && depth > 0);
            parent[t] = stack[depth - 1];
        } else {
            CHECK(c == ',' || c == ';');
        }
    }
    CHECK(depth == 0);
    free(stack);
    return n;
}

static int in_mask(const uint64_t *m, uint32_t x) { return (int)((m[x >> 6] >> (x & 63)) & 1); }

/* `search`: 0 leaves out the search to convergence (a round on the host costs T^2 table entries) */
static void run(int32_t T, int shape, int64_t nrows, int search)
{
    const int64_t W = (T + 63) / 64, EC = T > 3 ? T - 3 : 1;
    int32_t *parent = (int32_t *)malloc(sizeof(int32_t) * (size_t)(3 * T + 4));
    int32_t *after = (int32_t *)malloc(sizeof(int32_t) * (size_t)(3 * T + 4));
    uint32_t *q = (uint32_t *)malloc(sizeof(uint32_t) * 4 * (size_t)nrows);
    uint32_t *st = (uint32_t *)malloc(sizeof(uint32_t) * 2 * (size_t)nrows);
    double *sc = (double *)malloc(sizeof(double) * 3 * (size_t)nrows);
    uint32_t *sp = (uint32_t *)malloc(sizeof(uint32_t) * 4 * (size_t)nrows);
    uint64_t *k = (uint64_t *)malloc(sizeof(uint64_t) * (size_t)nrows);
    uint8_t *elig = (uint8_t *)malloc((size_t)EC);
    uint64_t *corners = (uint64_t *)malloc(sizeof(uint64_t) * (size_t)(EC * 4 * W));
    uint64_t *w = (uint64_t *)malloc(sizeof(uint64_t) * 3 * (size_t)EC), *w2 = (uint64_t *)malloc(sizeof(uint64_t) * 3 * (size_t)EC);
    const int64_t cap = 16 * (int64_t)T + 64;
    char *nwk = (char *)malloc((size_t)cap), *nwk2 = (char *)malloc((size_t)cap);
    CHECK(parent && after && q && st && sc && sp && k && elig && corners && w && w2 && nwk && nwk2);
    const int64_t n_nodes = make_tree(T, shape, parent);
    for (int64_t i = 0; i < nrows; ++i) {
        uint32_t *r = q + 4 * i;
        for (int a = 0; a < 4;) {                                   /* four distinct taxa, half of the rows from a window */
            r[a] = (i & 1) && T > 8 ? (uint32_t)((i * 7) % (T - 7)) + rnd(8) : rnd((uint32_t)T);
            int dup = 0;
            for (int b = 0; b < a; ++b) dup |= r[b] == r[a];
            a += !dup;
        }
        st[2 * i] = rnd(3);
        st[2 * i + 1] = 1 + rnd(500);
        for (int j = 0; j < 3; ++j) sc[3 * i + j] = (double)(100 + rnd(40000));
        sc[3 * i + st[2 * i]] = (double)(1 + rnd(99));
    }
    tq_stree *acc = NULL;
    CHECK(tq_stree_create(&acc, T, nrows, 1, 0, 1.0, NULL) == TQ_OK && acc);
    /* no rows yet: all zeros, polish converges at once */
    int64_t E = -1, written = -1, rounds = -1, kept = -1;
    int conv = -1;
    uint64_t trace[2 * 8];
    CHECK(tq_stree_nni_scan(acc, parent, n_nodes, NULL, &E, elig, corners, w) == TQ_OK && E >= 0 && E <= T - 3);
    for (int64_t i = 0; i < 3 * E; ++i) CHECK(w[i] == 0);
    CHECK(tq_stree_polish(acc, parent, n_nodes, 8, NULL, nwk, cap, &written, trace, &rounds, &conv) == TQ_OK);
    CHECK(rounds == 0 && conv == 1 && written > 0 && nwk[written - 1] == ';');
    const int64_t half = nrows / 2;
    CHECK(tq_stree_add(acc, q, st, sc, NULL, half) == TQ_OK);
    CHECK(tq_stree_add(acc, q + 4 * half, st + 2 * half, sc + 3 * half, NULL, nrows - half) == TQ_OK);
    CHECK(tq_stree_rows(acc, sp, k, &kept) == TQ_OK && kept == nrows);

    /* scan, recounted from the masks */
    CHECK(tq_stree_nni_scan(acc, parent, n_nodes, NULL, &E, elig, corners, w) == TQ_OK);
    if (shape == STAR) CHECK(E == 0);
    if (shape == CATERPILLAR) CHECK(E == T - 3);
    int64_t n_elig = 0;
    uint64_t total = 0;
    memset(w2, 0, sizeof(uint64_t) * 3 * (size_t)EC);
    for (int64_t e = 0; e < E; ++e) {
        const uint64_t *m = corners + e * 4 * W;
        int64_t bits = 0;
        for (int64_t i = 0; i < 4 * W; ++i) bits += __builtin_popcountll(m[i]);
        if (!elig[e]) {
            CHECK(bits == 0 && !w[3 * e] && !w[3 * e + 1] && !w[3 * e + 2]);
            continue;
        }
        ++n_elig;
        CHECK(bits == T);
        for (int64_t i = 0; i < W; ++i) CHECK((m[i] & m[W + i]) == 0 && ((m[i] | m[W + i]) & (m[2 * W + i] | m[3 * W + i])) == 0 &&
                                              (m[2 * W + i] & m[3 * W + i]) == 0);
        total += w[3 * e] + w[3 * e + 1] + w[3 * e + 2];
    }
    if (shape == RANDOM || shape == CATERPILLAR) CHECK(n_elig == E);
    if (T <= 300)
        for (int64_t i = 0; i < kept; ++i)
            for (int64_t e = 0; e < E; ++e) {
                if (!elig[e]) continue;
                const uint64_t *m = corners + e * 4 * W;
                int c[4], seen = 0;
                for (int a = 0; a < 4; ++a) {
                    c[a] = -1;
                    for (int j = 0; j < 4; ++j)
                        if (in_mask(m + j * W, sp[4 * i + a])) c[a] = j;
                    if (c[a] >= 0) seen |= 1 << c[a];
                }
                if (seen != 15) continue;
                const int cls = (c[0] >> 1) == (c[1] >> 1) ? 0 : ((c[0] & 1) == (c[1] & 1) ? 1 : 2);
                w2[3 * e + cls] += k[i];
            }
    if (T <= 300)
        for (int64_t i = 0; i < 3 * E; ++i) CHECK(w[i] == w2[i]);
    if (E && nrows >= 1000) CHECK(total > 0);
    /* NULL outputs, each alone */
    CHECK(tq_stree_nni_scan(acc, parent, n_nodes, NULL, NULL, NULL, NULL, NULL) == TQ_OK);
    CHECK(tq_stree_nni_scan(acc, parent, n_nodes, NULL, NULL, NULL, NULL, w2) == TQ_OK);
    for (int64_t i = 0; i < 3 * E; ++i) CHECK(w[i] == w2[i]);
    CHECK(tq_stree_nni_scan(acc, parent, n_nodes, NULL, NULL, elig, NULL, NULL) == TQ_OK);
    CHECK(tq_stree_nni_scan(acc, parent, n_nodes, NULL, NULL, NULL, corners, NULL) == TQ_OK);

    /* the same tree hung from another internal node: the same edges, so the same total */
    if (shape != STAR) {
        memcpy(after, parent, sizeof(int32_t) * (size_t)n_nodes);
        reroot(after, T + (int32_t)rnd((uint32_t)(n_nodes - T)));
        int64_t E2 = -1;
        uint64_t total2 = 0;
        CHECK(tq_stree_nni_scan(acc, after, n_nodes, NULL, &E2, elig, NULL, w2) == TQ_OK && E2 == E);
        for (int64_t i = 0; i < 3 * E2; ++i) total2 += w2[i];
        CHECK(total2 == total);
    }

    /* polish: max_rounds 0 rewrites, 1 makes one round, the full search ends converged; the fit rises by the gains */
    uint64_t f0[6], f1[6];
    int64_t nn = n_nodes;
    CHECK(tq_stree_fit(acc, parent, &nn, 1, n_nodes, NULL, f0) == TQ_OK);
    CHECK(tq_stree_polish(acc, parent, n_nodes, 0, NULL, nwk, cap, &written, trace, &rounds, &conv) == TQ_OK);
    CHECK(rounds == 0 && conv == 0);
    int64_t n_after = parse_newick(nwk, written, T, after);
    CHECK(tq_stree_fit(acc, after, &n_after, 1, n_after, NULL, f1) == TQ_OK);
    for (int j = 0; j < 6; ++j) CHECK(f0[j] == f1[j]);
    CHECK(tq_stree_polish(acc, parent, n_nodes, 1, NULL, nwk, cap, &written, trace, &rounds, &conv) == TQ_OK);
    CHECK(rounds <= 1 && (rounds == 1 || conv == 1));
    n_after = parse_newick(nwk, written, T, after);
    CHECK(tq_stree_fit(acc, after, &n_after, 1, n_after, NULL, f1) == TQ_OK);
    CHECK(f1[0] - f0[0] == (rounds ? trace[1] : 0) && f1[2] == f0[2]);
    const int64_t max_rounds = 4096;
    uint64_t *tr = (uint64_t *)malloc(sizeof(uint64_t) * 2 * (size_t)max_rounds);
    CHECK(tr);
    CHECK(tq_stree_polish(acc, parent, n_nodes, search ? max_rounds : 2, NULL, nwk, cap, &written, tr, &rounds, &conv) == TQ_OK);
    CHECK(search ? conv == 1 && rounds < max_rounds : rounds <= 2);
    uint64_t gains = 0;
    for (int64_t r = 0; r < rounds; ++r) {
        CHECK(tr[2 * r] >= 1 && tr[2 * r + 1] >= tr[2 * r]);
        gains += tr[2 * r + 1];
    }
    n_after = parse_newick(nwk, written, T, after);
    CHECK(tq_stree_fit(acc, after, &n_after, 1, n_after, NULL, f1) == TQ_OK);
    CHECK(f1[0] - f0[0] == gains && f0[1] - f1[1] == gains && f1[2] == f0[2]);
    /* the result is a fixed point, written the same way again */
    int64_t written2 = -1;
    CHECK(tq_stree_polish(acc, after, n_after, 8, NULL, nwk2, cap, &written2, NULL, &rounds, &conv) == TQ_OK);
    CHECK(written2 == written);                                     /* the same taxa and as many internal nodes */
    if (search) CHECK(rounds == 0 && conv == 1 && !memcmp(nwk, nwk2, (size_t)written));
    /* cap too small: the needed size and nothing else; NULL trace, rounds, converged */
    memset(nwk2, 'x', (size_t)cap);
    written2 = -1;
    CHECK(tq_stree_polish(acc, after, n_after, 8, NULL, nwk2, written - 1, &written2, NULL, NULL, NULL) == TQ_ERR_OOM);
    CHECK(written2 == written && nwk2[0] == 'x');
    CHECK(tq_stree_polish(acc, after, n_after, 8, NULL, NULL, 0, &written2, NULL, NULL, NULL) == TQ_ERR_OOM && written2 == written);
    CHECK(tq_stree_polish(acc, after, n_after, 8, NULL, nwk2, written, &written2, NULL, NULL, NULL) == TQ_OK);

    /* bad trees and bad arguments: refused, nothing written */
    {
        int64_t E3 = -7, wr = -7, rd = -7;
        int cv = -7;
        memcpy(after, parent, sizeof(int32_t) * (size_t)n_nodes);
        after[n_nodes] = after[0];                                  /* a tip that is no taxon */
        CHECK(tq_stree_nni_scan(acc, after, n_nodes + 1, NULL, &E3, NULL, NULL, NULL) == TQ_ERR_INVALID_ARG && E3 == -7);
        CHECK(strstr(tq_last_error(NULL), "tq_stree_nni_scan: tree 0"));
        CHECK(tq_stree_polish(acc, after, n_nodes + 1, 8, NULL, nwk2, cap, &wr, NULL, &rd, &cv) == TQ_ERR_INVALID_ARG);
        CHECK(wr == -7 && rd == -7 && cv == -7 && strstr(tq_last_error(NULL), "tq_stree_polish: tree 0"));
        after[n_nodes] = (int32_t)n_nodes + 1;                      /* a cycle of two nodes beside the tree */
        after[n_nodes + 1] = (int32_t)n_nodes;
        CHECK(tq_stree_nni_scan(acc, after, n_nodes + 2, NULL, &E3, NULL, NULL, NULL) == TQ_ERR_INVALID_ARG && E3 == -7);
        CHECK(strstr(tq_last_error(NULL), "cycle"));
        CHECK(tq_stree_polish(acc, after, n_nodes + 2, 8, NULL, nwk2, cap, &wr, NULL, &rd, &cv) == TQ_ERR_INVALID_ARG && wr == -7);
        CHECK(tq_stree_nni_scan(acc, parent, 64 * 4096 + 1, NULL, &E3, NULL, NULL, NULL) == TQ_ERR_INVALID_ARG && E3 == -7);
        CHECK(tq_stree_nni_scan(acc, parent, T - 1, NULL, &E3, NULL, NULL, NULL) == TQ_ERR_INVALID_ARG && E3 == -7);
        CHECK(tq_stree_nni_scan(acc, NULL, n_nodes, NULL, &E3, NULL, NULL, NULL) == TQ_ERR_INVALID_ARG);
        CHECK(tq_stree_nni_scan(NULL, parent, n_nodes, NULL, &E3, NULL, NULL, NULL) == TQ_ERR_INVALID_ARG);
        CHECK(tq_stree_polish(acc, parent, n_nodes, -1, NULL, nwk2, cap, &wr, NULL, NULL, NULL) == TQ_ERR_INVALID_ARG && wr == -7);
        CHECK(tq_stree_polish(acc, parent, n_nodes, 65537, NULL, nwk2, cap, &wr, NULL, NULL, NULL) == TQ_ERR_INVALID_ARG);
        CHECK(strstr(tq_last_error(NULL), "max_rounds"));
        CHECK(tq_stree_polish(acc, parent, n_nodes, 8, NULL, nwk2, cap, NULL, NULL, NULL, NULL) == TQ_ERR_INVALID_ARG);
        CHECK(tq_stree_polish(acc, parent, n_nodes, 8, NULL, NULL, cap, &wr, NULL, NULL, NULL) == TQ_ERR_INVALID_ARG);
        CHECK(tq_stree_polish(NULL, parent, n_nodes, 8, NULL, nwk2, cap, &wr, NULL, NULL, NULL) == TQ_ERR_INVALID_ARG);
    }
    /* reset and reuse */
    CHECK(tq_stree_reset(acc) == TQ_OK);
    CHECK(tq_stree_nni_scan(acc, parent, n_nodes, NULL, &E, NULL, NULL, w) == TQ_OK);
    for (int64_t i = 0; i < 3 * E; ++i) CHECK(w[i] == 0);
    CHECK(tq_stree_add(acc, q, st, sc, NULL, half) == TQ_OK);
    CHECK(tq_stree_nni_scan(acc, parent, n_nodes, NULL, &E, NULL, NULL, w) == TQ_OK);
    tq_stree_destroy(acc);
    free(tr); free(nwk2); free(nwk); free(w2); free(w); free(corners); free(elig); free(k); free(sp); free(sc); free(st);
    free(q); free(after); free(parent);
}

int main(void)
{
    {   /* fewer than 4 taxa: no tree to scan */
        tq_stree *acc = NULL;
        int32_t three[4] = {3, 3, 3, -1};
        int64_t E = -7, wr = -7;
        char buf[32];
        CHECK(tq_stree_create(&acc, 3, 10, 0, 0, 1.0, NULL) == TQ_OK);
        CHECK(tq_stree_nni_scan(acc, three, 4, NULL, &E, NULL, NULL, NULL) == TQ_ERR_INVALID_ARG && E == -7);
        CHECK(tq_stree_polish(acc, three, 4, 0, NULL, buf, 32, &wr, NULL, NULL, NULL) == TQ_ERR_INVALID_ARG && wr == -7);
        tq_stree_destroy(acc);
    }
    run(4, RANDOM, 50, 1);
    run(4, STAR, 50, 1);
    run(5, CATERPILLAR, 200, 1);
    run(6, POLYTOMIES, 500, 1);
    run(9, RANDOM, 2000, 1);
    run(40, RANDOM, 20000, 1);
    run(40, POLYTOMIES, 20000, 1);
    run(65, CATERPILLAR, 20000, 1);
    run(257, RANDOM, 50000, 1);
    run(257, POLYTOMIES, 50000, 1);
    run(300, STAR, 1000, 1);
    run(1024, CATERPILLAR, 20000, 0);           /* the fit's host table walks every pair up: keep the deep tree small */
    run(4096, RANDOM, 20000, 0);
    printf("nni_host_check: ok\n");
    return 0;
}

/* scf_host_check.c -- the host paths of the two accumulators on a fixed tree, which share their host code: the site
 * concordance accumulator (tq_scf_create / tq_scf_add / tq_scf_read with a NULL context) and the
 * quartet concordance accumulator (tq_conc_create / tq_conc_add / tq_conc_read / tq_conc_reset, section 11, its counts
 * against a recount from the split masks in this file), driven from a plain C program.
 * Built and run under the host sanitizers by tools/host_checks.sh.
 *
 * No device is needed or touched: every accumulator is created without a context.  Prints "scf_host_check: ok" and
 * returns 0 when every check held; a sanitizer report or a failed check ends it with a non-zero status. */
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
            fprintf(stderr, "scf_host_check: line %d: %s\n", __LINE__, #cond);       \
            exit(1);                                                                 \
        }                                                                            \
    } while (0)

/* random joins of two or three subtrees, a unary node now and then; returns the node count */
static int64_t random_tree(int32_t T, int32_t *parent)
{
    int32_t *roots = (int32_t *)malloc(sizeof(int32_t) * (size_t)T);
    int32_t nroots = T, n = T;
    CHECK(roots);
    for (int32_t t = 0; t < T; ++t) { roots[t] = t; parent[t] = -1; }
    while (nroots > 1) {
        const int32_t k = (nroots >= 3 && rnd(5) == 0) ? 3 : 2;
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

/* The concordance accumulator on the same tree: `nrows` rows with whole-number scores (their 6-decimal rounding is the
 * identity, and sums made in row order are bit-equal to the library's) against a recount that knows only the split masks
 * the library reports: a row is induced on an edge iff that split alone separates its taxa two against two. */
static void run_conc(int32_t T, int caterpillar, const int32_t *parent, int64_t n_nodes, int64_t nrows)
{
    const int64_t min_snps = 3;
    const double min_ratio = 1.25;
    tq_conc *acc = NULL;
    CHECK(tq_conc_create(&acc, parent, n_nodes, T, min_snps, min_ratio, NULL) == TQ_OK && acc);
    int64_t t = 0, E = 0, W = 0;
    CHECK(tq_conc_shape(acc, &t, &E, &W) == TQ_OK && t == T && W == (T + 63) / 64);
    const size_t e1 = (size_t)(E ? E : 1);
    uint32_t *q = (uint32_t *)malloc(sizeof(uint32_t) * 4 * (size_t)nrows);
    uint32_t *st = (uint32_t *)malloc(sizeof(uint32_t) * 2 * (size_t)nrows);
    double *sc = (double *)malloc(sizeof(double) * 3 * (size_t)nrows);
    uint8_t *fl = (uint8_t *)malloc((size_t)nrows);
    int64_t *counts = (int64_t *)malloc(sizeof(int64_t) * 6 * e1), *want = (int64_t *)calloc(6 * e1, sizeof(int64_t));
    double *sums = (double *)malloc(sizeof(double) * 2 * e1), *wsum = (double *)calloc(2 * e1, sizeof(double));
    uint64_t *masks = (uint64_t *)malloc(sizeof(uint64_t) * e1 * (size_t)W);
    int64_t *tips = (int64_t *)malloc(sizeof(int64_t) * 2 * (size_t)T), *wtips = (int64_t *)calloc(2 * (size_t)T, sizeof(int64_t));
    CHECK(q && st && sc && fl && counts && want && sums && wsum && masks && tips && wtips);
    for (int64_t i = 0; i < nrows; ++i) {
        const int window = caterpillar && T > 8;
        const uint32_t base = window ? rnd((uint32_t)T - 7) : 0, span = window ? 8 : (uint32_t)T;
        for (int k = 0; k < 4; ++k) q[4 * i + k] = base + rnd(span);
        const uint32_t kind = rnd(40);
        if (kind == 0) q[4 * i + 1] = (uint32_t)T;
        if (kind == 1) q[4 * i + 2] = q[4 * i];
        st[2 * i] = kind == 2 ? 3 : rnd(3);
        st[2 * i + 1] = rnd(12);
        for (int k = 0; k < 3; ++k) sc[3 * i + k] = rnd(8) ? (double)rnd(400) : 0.0;
        fl[i] = kind == 3 ? (uint8_t)(1u << rnd(5)) : 0;
    }
    const int64_t half = nrows / 2;
    CHECK(tq_conc_add(acc, q, st, sc, fl, half) == TQ_OK);
    CHECK(tq_conc_add(acc, q + 4 * half, st + 2 * half, sc + 3 * half, fl + half, nrows - half) == TQ_OK);
    CHECK(tq_conc_add(acc, NULL, NULL, NULL, NULL, 0) == TQ_OK);
    CHECK(tq_conc_add(acc, q, NULL, sc, fl, 3) == TQ_ERR_INVALID_ARG);
    CHECK(tq_conc_add(acc, q, st, sc, fl, -1) == TQ_ERR_INVALID_ARG);
    CHECK(tq_conc_add_dev(acc, q, st, sc, fl, 1, NULL) == TQ_ERR_INVALID_ARG);
    CHECK(strstr(tq_last_error(NULL), "tq_conc_add_dev: the accumulator was created without a context"));
    int64_t skipped = -1, wskipped = 0;
    CHECK(tq_conc_read(acc, counts, sums, masks, tips, &skipped) == TQ_OK);
    CHECK(tq_conc_read(acc, NULL, NULL, NULL, NULL, NULL) == TQ_OK);
    for (int64_t i = 0; i < nrows; ++i) {
        const uint32_t *r = q + 4 * i;
        int bad = (fl[i] & (4 | 16)) || st[2 * i] > 2;
        for (int a = 0; a < 4; ++a) {
            if (r[a] >= (uint32_t)T) bad = 1;
            for (int b = a + 1; b < 4; ++b)
                if (r[a] == r[b]) bad = 1;
        }
        if (bad) { ++wskipped; continue; }
        int64_t edge = -1;
        int nsep = 0, res = 0;
        for (int64_t e = 0; e < E; ++e) {
            int in[4];
            for (int k = 0; k < 4; ++k) in[k] = (int)(masks[e * W + (r[k] >> 6)] >> (r[k] & 63)) & 1;
            if (in[0] + in[1] + in[2] + in[3] != 2) continue;
            ++nsep;
            edge = e;
            res = in[0] == in[1] ? 0 : in[0] == in[2] ? 1 : 2;
        }
        if (nsep != 1) continue;
        double y[3] = {sc[3 * i], sc[3 * i + 1], sc[3 * i + 2]}, tmp;
        if (y[0] > y[1]) { tmp = y[0]; y[0] = y[1]; y[1] = tmp; }
        if (y[1] > y[2]) { tmp = y[1]; y[1] = y[2]; y[2] = tmp; }
        if (y[0] > y[1]) { tmp = y[0]; y[0] = y[1]; y[1] = tmp; }
        const double weight = (y[1] + y[2]) / 2.0, score = y[0] == 0.0 ? 0.0 : weight / y[0];
        const int topo = (int)st[2 * i], lower = res == 0 ? 1 : 0;
        const int informative = !(score < min_ratio || (int64_t)st[2 * i + 1] < min_snps);
        const int cls = !informative ? 4 : topo == res ? 1 : topo == lower ? 2 : 3;    /* conc, disc1, disc2, nu */
        want[6 * edge + cls] += 1;
        want[6 * edge + 5] += st[2 * i + 1];
        wsum[2 * edge] += weight;
        wsum[2 * edge + 1] += score;
        if (informative)
            for (int k = 0; k < 4; ++k) wtips[2 * r[k] + (cls == 1 ? 0 : 1)] += 1;
    }
    CHECK(skipped == wskipped);
    int64_t induced = 0;
    for (int64_t e = 0; e < E; ++e) {
        CHECK(counts[6 * e] > 0);                                  /* nqrts: every edge induces some quartet */
        for (int k = 1; k < 6; ++k) CHECK(counts[6 * e + k] == want[6 * e + k]);
        CHECK(memcmp(&sums[2 * e], &wsum[2 * e], 2 * sizeof(double)) == 0);
        induced += counts[6 * e + 1] + counts[6 * e + 2] + counts[6 * e + 3] + counts[6 * e + 4];
    }
    for (int64_t i = 0; i < 2 * (int64_t)T; ++i) CHECK(tips[i] == wtips[i]);
    if (E) CHECK(induced > 0);
    CHECK(tq_conc_reset(acc) == TQ_OK);
    CHECK(tq_conc_read(acc, counts, sums, NULL, tips, &skipped) == TQ_OK && skipped == 0);
    for (int64_t e = 0; e < E; ++e) {
        for (int k = 1; k < 6; ++k) CHECK(counts[6 * e + k] == 0);
        CHECK(sums[2 * e] == 0.0 && sums[2 * e + 1] == 0.0);
    }
    for (int64_t i = 0; i < 2 * (int64_t)T; ++i) CHECK(tips[i] == 0);
    tq_conc_destroy(acc);
    free(wtips); free(tips); free(masks); free(wsum); free(sums); free(want); free(counts);
    free(fl); free(sc); free(st); free(q);
}

static void run(int32_t T, int caterpillar, int64_t nrows)
{
    int32_t *parent = (int32_t *)malloc(sizeof(int32_t) * 3 * (size_t)T);
    int64_t n_nodes;
    CHECK(parent);
    if (caterpillar) {
        int32_t prev = 0;
        n_nodes = T;
        for (int32_t t = 0; t < T; ++t) parent[t] = -1;
        for (int32_t t = 1; t < T; ++t) {
            const int32_t v = (int32_t)n_nodes++;
            parent[v] = -1;
            parent[prev] = v;
            parent[t] = v;
            prev = v;
        }
    } else {
        n_nodes = random_tree(T, parent);
    }
    tq_scf *acc = NULL;
    CHECK(tq_scf_create(&acc, parent, n_nodes, T, NULL) == TQ_OK && acc);
    int64_t t = 0, E = 0, W = 0;
    CHECK(tq_scf_shape(acc, &t, &E, &W) == TQ_OK && t == T && W == (T + 63) / 64);
    if (caterpillar) CHECK(E == T - 3);

    uint32_t *sets = (uint32_t *)malloc(sizeof(uint32_t) * 4 * (size_t)nrows);
    uint32_t *classes = (uint32_t *)malloc(sizeof(uint32_t) * 16 * (size_t)nrows);
    CHECK(sets && classes);
    int64_t bad = 0;
    for (int64_t i = 0; i < nrows; ++i) {
        uint32_t *q = sets + 4 * i, *c = classes + 16 * i;
        const int window = caterpillar && T > 8;          /* four taxa drawn from the whole caterpillar are hardly ever one edge apart */
        const uint32_t base = window ? rnd((uint32_t)T - 7) : 0, span = window ? 8 : (uint32_t)T;
        for (int k = 0; k < 4; ++k) q[k] = base + rnd(span);
        const uint32_t kind = rnd(40);
        if (kind == 0) q[1] = (uint32_t)T;
        if (kind == 1) q[3] = 0xFFFFFFFFu;
        if (kind == 2) q[2] = q[0];
        for (int k = 0; k < 16; ++k) c[k] = rnd(3000);
        const uint32_t v = rnd(8);
        if (v == 0) c[3] = c[6] = c[8] = 0xFFFFFFFFu;
        if (v == 1) c[3] = c[6] = c[8] = 0;
        if (v == 2) { c[3] = 0xFFFFFFFFu; c[6] = 0; c[8] = 1; }
        int rowbad = 0;
        for (int a = 0; a < 4; ++a) {
            if (q[a] >= (uint32_t)T) rowbad = 1;
            for (int b = a + 1; b < 4; ++b)
                if (q[a] == q[b]) rowbad = 1;
        }
        bad += rowbad;
    }
    const int64_t half = nrows / 2;
    CHECK(tq_scf_add(acc, sets, classes, half) == TQ_OK);
    CHECK(tq_scf_add(acc, sets + 4 * half, classes + 16 * half, nrows - half) == TQ_OK);
    CHECK(tq_scf_add(acc, NULL, NULL, 0) == TQ_OK);
    CHECK(tq_scf_add(acc, NULL, classes, 3) == TQ_ERR_INVALID_ARG);
    CHECK(tq_scf_add(acc, sets, classes, -1) == TQ_ERR_INVALID_ARG);
    CHECK(tq_scf_add_dev(acc, sets, classes, 1, NULL) == TQ_ERR_INVALID_ARG);
    CHECK(strstr(tq_last_error(NULL), "without a context"));

    int64_t *counts = (int64_t *)malloc(sizeof(int64_t) * 8 * (size_t)(E ? E : 1));
    uint64_t *masks = (uint64_t *)malloc(sizeof(uint64_t) * (size_t)((E ? E : 1) * W));
    int64_t skipped = -1, induced = 0;
    CHECK(counts && masks);
    CHECK(tq_scf_read(acc, counts, masks, &skipped) == TQ_OK);
    CHECK(tq_scf_read(acc, NULL, NULL, NULL) == TQ_OK);
    CHECK(skipped == bad);
    for (int64_t e = 0; e < E; ++e) {
        const uint64_t *w = (const uint64_t *)counts + 8 * e;
        induced += (int64_t)(w[0] + w[1]);
        /* the three shares of a row add up to 2^32 less at most two truncations */
        CHECK(w[5] + w[6] + w[7] <= (w[0] << 32) && w[5] + w[6] + w[7] + 2 * w[0] >= (w[0] << 32));
        if (!w[0]) CHECK(!w[2] && !w[3] && !w[4]);
        int64_t side = 0;
        for (int64_t k = 0; k < W; ++k) side += __builtin_popcountll(masks[e * W + k]);
        CHECK(side >= 2 && side <= T - 2);
    }
    CHECK(induced + skipped <= nrows);
    if (E) CHECK(induced > 0);
    CHECK(tq_scf_reset(acc) == TQ_OK);
    CHECK(tq_scf_read(acc, counts, NULL, &skipped) == TQ_OK && skipped == 0);
    for (int64_t i = 0; i < 8 * E; ++i) CHECK(counts[i] == 0);
    tq_scf_destroy(acc);
    run_conc(T, caterpillar, parent, n_nodes, nrows < 10000 ? nrows : 10000);
    free(masks); free(counts); free(classes); free(sets); free(parent);
}

int main(void)
{
    tq_scf *acc = (tq_scf *)1;
    int32_t three[5] = {3, 3, 3, -1, 0};
    CHECK(tq_scf_create(&acc, three, 4, 3, NULL) == TQ_ERR_INVALID_ARG && acc == NULL);
    CHECK(tq_scf_create(&acc, NULL, 4, 4, NULL) == TQ_ERR_INVALID_ARG);
    CHECK(tq_scf_create(NULL, three, 4, 3, NULL) == TQ_ERR_INVALID_ARG);
    {
        int32_t *big = (int32_t *)malloc(sizeof(int32_t) * 4098);
        CHECK(big);
        for (int i = 0; i < 4097; ++i) big[i] = 4097;
        big[4097] = -1;
        CHECK(tq_scf_create(&acc, big, 4098, 4097, NULL) == TQ_ERR_INVALID_ARG && acc == NULL);
        CHECK(strstr(tq_last_error(NULL), "4096"));
        /* a star of 4096 taxa: no edge, every row of distinct taxa is induced on none */
        for (int i = 0; i < 4096; ++i) big[i] = 4096;
        big[4096] = -1;
        int64_t E = -1;
        CHECK(tq_scf_create(&acc, big, 4097, 4096, NULL) == TQ_OK && tq_scf_shape(acc, NULL, &E, NULL) == TQ_OK && E == 0);
        uint32_t q[4] = {0, 4095, 7, 9}, c[16] = {0};
        int64_t skipped = -1;
        CHECK(tq_scf_add(acc, q, c, 1) == TQ_OK && tq_scf_read(acc, NULL, NULL, &skipped) == TQ_OK && skipped == 0);
        tq_scf_destroy(acc);
        free(big);
    }
    tq_scf_destroy(NULL);
    {
        tq_conc *c = (tq_conc *)1;
        CHECK(tq_conc_create(&c, three, 4, 3, 0, 1.0, NULL) == TQ_ERR_INVALID_ARG && c == NULL);
        CHECK(strstr(tq_last_error(NULL), "tq_conc_create: "));
        CHECK(tq_conc_create(&c, three, 4, 4, 0, 0.0 / 0.0, NULL) == TQ_ERR_INVALID_ARG && c == NULL);
        CHECK(tq_conc_reset(NULL) == TQ_ERR_INVALID_ARG && tq_conc_shape(NULL, NULL, NULL, NULL) == TQ_ERR_INVALID_ARG);
        tq_conc_destroy(NULL);
    }
    run(4, 1, 200);
    run(5, 0, 2000);
    run(40, 0, 200000);
    run(257, 0, 200000);
    run(4096, 0, 200000);
    run(4096, 1, 200000);
    printf("scf_host_check: ok\n");
    return 0;
}

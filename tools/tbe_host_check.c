/* tbe_host_check.c -- the host back end of the transfer bootstrap accumulator (tq_tbe_* without a context, DESIGN.md
 * section 25), driven from a plain C program.
 * Built and run under the host sanitizers by tools/host_checks.sh.
 *
 * No device is needed or touched.  Every phi is recounted here from taxon lists: the taxa below every node of the
 * replicate as bytes, the distance to a branch as a loop over the taxa, the minimum over every edge, tip edges included.
 * Prints "tbe_host_check: ok" and returns 0 when every check held; a sanitizer report or a failed check ends it with a
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
            fprintf(stderr, "tbe_host_check: line %d: %s\n", __LINE__, #cond);       \
            exit(1);                                                                 \
        }                                                                            \
    } while (0)

enum { RANDOM = 0, CATERPILLAR = 1, STAR = 2, POLYTOMIES = 3 };

/* parent array of T taxa (room for 3 T nodes); random joins of two subtrees (three now and then with POLYTOMIES), a unary
 * node now and then.  Returns the node count. */
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
        if (rnd(10) == 0) { parent[v] = n; v = n++; parent[v] = -1; }
        roots[nroots++] = v;
    }
    free(roots);
    return n;
}

/* phi of the branch `mask` in the tree: the minimum over every non-root node of min(d, T - d), d = the taxa on which
 * "below the node" and "in the mask" differ */
static uint32_t phi_of(const uint64_t *mask, int32_t T, const int32_t *parent, int64_t n, uint8_t *below)
{
    memset(below, 0, (size_t)n * (size_t)T);
    for (int32_t t = 0; t < T; ++t)
        for (int32_t v = t; v >= 0; v = parent[v]) below[(size_t)v * T + t] = 1;
    uint32_t best = (uint32_t)T;
    for (int64_t v = 0; v < n; ++v) {
        if (parent[v] < 0) continue;
        uint32_t d = 0;
        for (int32_t t = 0; t < T; ++t) d += below[(size_t)v * T + t] != ((mask[t >> 6] >> (t & 63)) & 1);
        if (T - d < d) d = (uint32_t)T - d;
        if (d < best) best = d;
    }
    return best;
}

static void run(int32_t T, int ref_shape)
{
    enum { R = 9 };
    const int64_t W = (T + 63) / 64, EC = T - 3, stride = 3 * (int64_t)T + 4;
    int32_t *ref = (int32_t *)malloc(sizeof(int32_t) * (size_t)stride);
    int32_t *reps = (int32_t *)malloc(sizeof(int32_t) * (size_t)(R * stride));
    int64_t n_nodes[R];
    uint64_t *masks = (uint64_t *)malloc(sizeof(uint64_t) * (size_t)(EC * W));
    int64_t *p = (int64_t *)malloc(sizeof(int64_t) * (size_t)EC);
    uint64_t *sum = (uint64_t *)malloc(sizeof(uint64_t) * (size_t)EC), *sum2 = (uint64_t *)malloc(sizeof(uint64_t) * (size_t)EC);
    uint16_t *phi = (uint16_t *)malloc(sizeof(uint16_t) * (size_t)(R * EC));
    uint8_t *below = (uint8_t *)malloc((size_t)stride * (size_t)T);
    CHECK(ref && reps && masks && p && sum && sum2 && phi && below);
    const int64_t n_ref = make_tree(T, ref_shape, ref);
    for (int r = 0; r < R; ++r) {
        int32_t *t = reps + r * stride;
        for (int64_t i = 0; i < stride; ++i) t[i] = -1;
        if (r == 0) { memcpy(t, ref, sizeof(int32_t) * (size_t)n_ref); n_nodes[r] = n_ref; }
        else n_nodes[r] = make_tree(T, r == 1 ? STAR : r == 2 ? CATERPILLAR : r & 1 ? RANDOM : POLYTOMIES, t);
        CHECK(n_nodes[r] <= stride);
    }
    tq_tbe *acc = NULL;
    int64_t gT = -1, gW = -1, E = -1, nt = -1;
    CHECK(tq_tbe_create(&acc, T, ref, n_ref, NULL) == TQ_OK && acc);
    CHECK(tq_tbe_shape(acc, &gT, &gW, &E, &nt) == TQ_OK && gT == T && gW == W && E >= 0 && E <= EC && nt == 0);
    if (ref_shape == STAR) CHECK(E == 0);
    if (ref_shape == CATERPILLAR) CHECK(E == EC);
    CHECK(tq_tbe_read(acc, masks, p, sum) == TQ_OK);
    for (int64_t e = 0; e < E; ++e) {
        int64_t pc = 0;
        for (int64_t w = 0; w < W; ++w) pc += __builtin_popcountll(masks[e * W + w]);
        CHECK(!(masks[e * W] & 1) && pc >= 2 && pc <= T - 2 && p[e] == (pc < T - pc ? pc : T - pc) && sum[e] == 0);
        if (e) {                                                    /* ascending as one integer */
            int64_t w = W - 1;
            while (w > 0 && masks[e * W + w] == masks[(e - 1) * W + w]) --w;
            CHECK(masks[e * W + w] > masks[(e - 1) * W + w]);
        }
    }
    /* R = 0 with and without phi_out; NULL outputs */
    CHECK(tq_tbe_add(acc, NULL, NULL, 0, 0, NULL, NULL) == TQ_OK);
    CHECK(tq_tbe_add(acc, reps, n_nodes, 0, stride, NULL, phi) == TQ_OK);
    CHECK(tq_tbe_shape(acc, NULL, NULL, NULL, &nt) == TQ_OK && nt == 0);
    CHECK(tq_tbe_read(acc, NULL, NULL, NULL) == TQ_OK);
    /* all at once with the matrix, recounted */
    memset(phi, 0xEE, sizeof(uint16_t) * (size_t)(R * EC));
    CHECK(tq_tbe_add(acc, reps, n_nodes, R, stride, NULL, phi) == TQ_OK);
    CHECK(tq_tbe_read(acc, NULL, NULL, sum) == TQ_OK);
    for (int64_t e = 0; e < E; ++e) {
        uint64_t s = 0;
        for (int r = 0; r < R; ++r) {
            const uint32_t want = phi_of(masks + e * W, T, reps + r * stride, n_nodes[r], below);
            CHECK(phi[r * E + e] == want && want <= (uint32_t)p[e] - 1);
            s += want;
        }
        CHECK(phi[e] == 0 && phi[E + e] == p[e] - 1 && s == sum[e]);     /* the reference itself, then a star */
    }
    /* reset keeps the branches; two adds without the matrix make the same sums */
    CHECK(tq_tbe_reset(acc) == TQ_OK);
    CHECK(tq_tbe_shape(acc, NULL, NULL, &gT, &nt) == TQ_OK && gT == E && nt == 0);
    CHECK(tq_tbe_add(acc, reps, n_nodes, 4, stride, NULL, NULL) == TQ_OK);
    CHECK(tq_tbe_add(acc, reps + 4 * stride, n_nodes + 4, R - 4, stride, NULL, NULL) == TQ_OK);
    CHECK(tq_tbe_read(acc, NULL, NULL, sum2) == TQ_OK && tq_tbe_shape(acc, NULL, NULL, NULL, &nt) == TQ_OK && nt == R);
    for (int64_t e = 0; e < E; ++e) CHECK(sum2[e] == sum[e]);
    /* refusals: nothing of the call is added */
    {
        int32_t *bad = (int32_t *)malloc(sizeof(int32_t) * (size_t)(3 * stride));
        int64_t nn[3] = {n_nodes[3], n_nodes[4] + 2, n_nodes[5]};
        CHECK(bad);
        memcpy(bad, reps + 3 * stride, sizeof(int32_t) * (size_t)(3 * stride));
        bad[stride + n_nodes[4]] = (int32_t)n_nodes[4] + 1;         /* a cycle of two nodes beside tree 1 */
        bad[stride + n_nodes[4] + 1] = (int32_t)n_nodes[4];
        CHECK(n_nodes[4] + 2 <= stride);
        CHECK(tq_tbe_add(acc, bad, nn, 3, stride, NULL, phi) == TQ_ERR_INVALID_ARG);
        CHECK(strstr(tq_last_error(NULL), "tq_tbe_add: tree 1"));
        nn[1] = stride + 1;
        CHECK(tq_tbe_add(acc, bad, nn, 3, stride, NULL, NULL) == TQ_ERR_INVALID_ARG);
        CHECK(strstr(tq_last_error(NULL), "stride"));
        CHECK(tq_tbe_add(acc, NULL, nn, 3, stride, NULL, NULL) == TQ_ERR_INVALID_ARG);
        CHECK(tq_tbe_add(acc, bad, NULL, 3, stride, NULL, NULL) == TQ_ERR_INVALID_ARG);
        CHECK(tq_tbe_add(acc, bad, nn, -1, stride, NULL, NULL) == TQ_ERR_INVALID_ARG);
        CHECK(tq_tbe_add(NULL, bad, nn, 3, stride, NULL, NULL) == TQ_ERR_INVALID_ARG);
        CHECK(tq_tbe_read(acc, NULL, NULL, sum2) == TQ_OK && tq_tbe_shape(acc, NULL, NULL, NULL, &nt) == TQ_OK && nt == R);
        for (int64_t e = 0; e < E; ++e) CHECK(sum2[e] == sum[e]);
        tq_tbe *none = (tq_tbe *)&state;
        bad[0] = -1;                                                /* a second root */
        CHECK(tq_tbe_create(&none, T, bad, n_nodes[3], NULL) == TQ_ERR_INVALID_ARG && none == NULL);
        CHECK(strstr(tq_last_error(NULL), "tq_tbe_create"));
        CHECK(tq_tbe_create(&none, T, NULL, n_ref, NULL) == TQ_ERR_INVALID_ARG && none == NULL);
        CHECK(tq_tbe_create(NULL, T, ref, n_ref, NULL) == TQ_ERR_INVALID_ARG);
        free(bad);
    }
    int64_t st[2] = {-1, -1};
    CHECK(tq_tbe_stats(acc, st) == TQ_OK && st[0] == 0 && st[1] == 0);
    tq_tbe_destroy(acc);
    free(below); free(phi); free(sum2); free(sum); free(p); free(masks); free(reps); free(ref);
}

int main(void)
{
    {   /* outside 4..4096 taxa */
        tq_tbe *acc = (tq_tbe *)&state;
        int32_t three[4] = {3, 3, 3, -1};
        CHECK(tq_tbe_create(&acc, 3, three, 4, NULL) == TQ_ERR_INVALID_ARG && acc == NULL);
        CHECK(tq_tbe_create(&acc, 4097, three, 4, NULL) == TQ_ERR_INVALID_ARG && acc == NULL);
        CHECK(strstr(tq_last_error(NULL), "T must be 4..4096"));
        CHECK(tq_tbe_reset(NULL) == TQ_ERR_INVALID_ARG && tq_tbe_shape(NULL, NULL, NULL, NULL, NULL) == TQ_ERR_INVALID_ARG);
        CHECK(tq_tbe_read(NULL, NULL, NULL, NULL) == TQ_ERR_INVALID_ARG);
        tq_tbe_destroy(NULL);
    }
    const int32_t sizes[3] = {4, 65, 129};
    for (int i = 0; i < 3; ++i)
        for (int shape = RANDOM; shape <= POLYTOMIES; ++shape) run(sizes[i], shape);
    printf("tbe_host_check: ok\n");
    return 0;
}

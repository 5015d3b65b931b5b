/* treedist_host_check.c -- the host back end of the tree distance accumulator (tq_rf_* without a context, DESIGN.md
 * section 26), driven from a plain C program.
 * Built and run under the host sanitizers by tools/host_checks.sh.
 *
 * No device is needed or touched.  Every count is recounted here from taxon lists: the taxa below every node as bytes,
 * named by the side without taxon 0; two trees share a split when some node of each has the same bytes.
 * Prints "treedist_host_check: ok" and returns 0 when every check held; a sanitizer report or a failed check ends it
 * with a non-zero status. */
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
            fprintf(stderr, "treedist_host_check: line %d: %s\n", __LINE__, #cond);  \
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

/* sides[k][T] bytes: the distinct splits of the tree, each the side without taxon 0.  Returns their number. */
static int64_t sides_of(int32_t T, const int32_t *parent, int64_t n, uint8_t *below, uint8_t *sides)
{
    int64_t k = 0;
    memset(below, 0, (size_t)n * (size_t)T);
    for (int32_t t = 0; t < T; ++t)
        for (int32_t v = t; v >= 0; v = parent[v]) below[(size_t)v * T + t] = 1;
    for (int64_t v = 0; v < n; ++v) {
        uint8_t *s = sides + (size_t)k * T;
        int32_t size = 0;
        for (int32_t t = 0; t < T; ++t) {
            s[t] = below[(size_t)v * T] ? !below[(size_t)v * T + t] : below[(size_t)v * T + t];
            size += s[t];
        }
        if (size < 2 || size > T - 2) continue;
        int dup = 0;
        for (int64_t j = 0; j < k && !dup; ++j) dup = !memcmp(sides + (size_t)j * T, s, (size_t)T);
        if (!dup) ++k;
    }
    return k;
}

static void run(int32_t T)
{
    enum { R = 9 };
    const int64_t stride = 3 * (int64_t)T + 4;
    int32_t *reps = (int32_t *)malloc(sizeof(int32_t) * (size_t)(R * stride));
    int64_t n_nodes[R], nside[R];
    uint8_t *below = (uint8_t *)malloc((size_t)stride * (size_t)T);
    uint8_t *sides = (uint8_t *)malloc((size_t)R * (size_t)stride * (size_t)T);
    int32_t nsplits[R], want_n[R];
    uint32_t shared[R * R], rf[R * R], want_s[R * R], shared2[R * R], rf2[R * R];
    CHECK(reps && below && sides);
    for (int r = 0; r < R; ++r) {
        int32_t *t = reps + r * stride;
        for (int64_t i = 0; i < stride; ++i) t[i] = -1;
        if (r == 5) { memcpy(t, reps + 3 * stride, sizeof(int32_t) * (size_t)stride); n_nodes[r] = n_nodes[3]; }
        else n_nodes[r] = make_tree(T, r == 1 ? STAR : r == 2 ? CATERPILLAR : r & 1 ? RANDOM : POLYTOMIES, t);
        CHECK(n_nodes[r] <= stride);
        nside[r] = sides_of(T, t, n_nodes[r], below, sides + (size_t)r * stride * T);
        want_n[r] = (int32_t)nside[r];
    }
    int64_t distinct = 0, columns = 0;
    for (int i = 0; i < R; ++i)
        for (int64_t a = 0; a < nside[i]; ++a) {            /* first seen in tree i?  held by how many trees? */
            const uint8_t *x = sides + ((size_t)i * stride + a) * T;
            int first = 1, holders = 0;
            for (int j = 0; j < R; ++j)
                for (int64_t b = 0; b < nside[j]; ++b)
                    if (!memcmp(x, sides + ((size_t)j * stride + b) * T, (size_t)T)) {
                        ++holders;
                        if (j < i) first = 0;
                    }
            distinct += first;
            columns += first && holders >= 2;
        }
    for (int i = 0; i < R; ++i)
        for (int j = 0; j < R; ++j) {
            uint32_t s = 0;
            for (int64_t a = 0; a < nside[i]; ++a)
                for (int64_t b = 0; b < nside[j]; ++b)
                    s += !memcmp(sides + ((size_t)i * stride + a) * T, sides + ((size_t)j * stride + b) * T, (size_t)T);
            want_s[i * R + j] = s;
        }
    tq_rf *acc = NULL;
    int64_t gT = -1, gW = -1, nt = -1, nd = -1, nc = -1;
    CHECK(tq_rf_create(&acc, T, R, R * (int64_t)T, NULL) == TQ_OK && acc);
    CHECK(tq_rf_shape(acc, &gT, &gW, &nt, &nd, &nc) == TQ_OK && gT == T && gW == (T + 63) / 64 && nt == 0 && nd == 0 && nc == 0);
    /* nothing added: R = 0, NULL outputs, a read of no trees writes nothing */
    CHECK(tq_rf_add(acc, NULL, NULL, 0, 0, NULL) == TQ_OK);
    CHECK(tq_rf_add(acc, reps, n_nodes, 0, stride, NULL) == TQ_OK);
    nsplits[0] = -7; shared[0] = 77; rf[0] = 77;
    CHECK(tq_rf_read(acc, nsplits, shared, rf) == TQ_OK && nsplits[0] == -7 && shared[0] == 77 && rf[0] == 77);
    CHECK(tq_rf_read(acc, NULL, NULL, NULL) == TQ_OK);
    /* all at once, recounted */
    CHECK(tq_rf_add(acc, reps, n_nodes, R, stride, NULL) == TQ_OK);
    CHECK(tq_rf_read(acc, nsplits, shared, rf) == TQ_OK);
    CHECK(tq_rf_shape(acc, NULL, NULL, &nt, &nd, &nc) == TQ_OK && nt == R && nd == distinct && nc == columns);
    for (int i = 0; i < R; ++i) {
        CHECK(nsplits[i] == want_n[i] && nsplits[i] <= T - 3);
        for (int j = 0; j < R; ++j) {
            CHECK(shared[i * R + j] == want_s[i * R + j] && shared[i * R + j] == shared[j * R + i]);
            CHECK(rf[i * R + j] == (uint32_t)(want_n[i] + want_n[j]) - 2 * want_s[i * R + j]);
        }
        CHECK(shared[i * R + i] == (uint32_t)nsplits[i] && rf[i * R + i] == 0);
    }
    CHECK(nsplits[1] == 0 && nsplits[2] == T - 3 && rf[3 * R + 5] == 0);   /* star, caterpillar, a tree and its copy */
    /* reset; three adds with a read in between make the same matrices */
    CHECK(tq_rf_reset(acc) == TQ_OK);
    CHECK(tq_rf_shape(acc, NULL, NULL, &nt, &nd, &nc) == TQ_OK && nt == 0 && nd == 0 && nc == 0);
    CHECK(tq_rf_add(acc, reps, n_nodes, 4, stride, NULL) == TQ_OK);
    CHECK(tq_rf_read(acc, NULL, shared2, NULL) == TQ_OK);
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) CHECK(shared2[i * 4 + j] == want_s[i * R + j]);
    CHECK(tq_rf_add(acc, reps + 4 * stride, n_nodes + 4, 1, stride, NULL) == TQ_OK);
    CHECK(tq_rf_add(acc, reps + 5 * stride, n_nodes + 5, R - 5, stride, NULL) == TQ_OK);
    CHECK(tq_rf_read(acc, NULL, shared2, rf2) == TQ_OK && tq_rf_read(acc, NULL, shared2, rf2) == TQ_OK);
    CHECK(!memcmp(shared, shared2, sizeof shared) && !memcmp(rf, rf2, sizeof rf));
    /* refusals: nothing of the call is added */
    {
        int32_t *bad = (int32_t *)malloc(sizeof(int32_t) * (size_t)(3 * stride));
        int64_t nn[3] = {n_nodes[3], n_nodes[4] + 2, n_nodes[5]};
        CHECK(bad);
        CHECK(tq_rf_add(acc, reps, n_nodes, 1, stride, NULL) == TQ_ERR_INVALID_ARG);       /* R trees are held: full */
        CHECK(strstr(tq_last_error(NULL), "max_trees"));
        CHECK(tq_rf_reset(acc) == TQ_OK && tq_rf_add(acc, reps, n_nodes, R - 3, stride, NULL) == TQ_OK);
        memcpy(bad, reps + 3 * stride, sizeof(int32_t) * (size_t)(3 * stride));
        bad[stride + n_nodes[4]] = (int32_t)n_nodes[4] + 1;         /* a cycle of two nodes beside tree 1 */
        bad[stride + n_nodes[4] + 1] = (int32_t)n_nodes[4];
        CHECK(n_nodes[4] + 2 <= stride);
        CHECK(tq_rf_add(acc, bad, nn, 3, stride, NULL) == TQ_ERR_INVALID_ARG);
        CHECK(strstr(tq_last_error(NULL), "tq_rf_add: tree 1"));
        nn[1] = stride + 1;
        CHECK(tq_rf_add(acc, bad, nn, 3, stride, NULL) == TQ_ERR_INVALID_ARG);
        CHECK(strstr(tq_last_error(NULL), "stride"));
        CHECK(tq_rf_add(acc, reps, n_nodes, 4, stride, NULL) == TQ_ERR_INVALID_ARG);       /* R - 3 + 4 > R */
        CHECK(tq_rf_add(acc, NULL, nn, 3, stride, NULL) == TQ_ERR_INVALID_ARG);
        CHECK(tq_rf_add(acc, bad, NULL, 3, stride, NULL) == TQ_ERR_INVALID_ARG);
        CHECK(tq_rf_add(acc, bad, nn, -1, stride, NULL) == TQ_ERR_INVALID_ARG);
        CHECK(tq_rf_add(NULL, bad, nn, 3, stride, NULL) == TQ_ERR_INVALID_ARG);
        CHECK(tq_rf_read(acc, NULL, shared2, NULL) == TQ_OK && tq_rf_shape(acc, NULL, NULL, &nt, NULL, NULL) == TQ_OK);
        CHECK(nt == R - 3);
        for (int i = 0; i < R - 3; ++i)
            for (int j = 0; j < R - 3; ++j) CHECK(shared2[i * (R - 3) + j] == want_s[i * R + j]);
        free(bad);
    }
    int64_t st[8] = {-1, -1, -1, -1, -1, -1, -1, -1};
    CHECK(tq_rf_stats(acc, st) == TQ_OK && st[0] == 0 && st[1] == 0 && st[2] >= 0 && st[3] == 0 && st[4] == 0 && st[5] == 0);
    tq_rf_destroy(acc);
    /* more distinct splits than max_splits: refused until a reset */
    if (want_n[2] > 1) {
        CHECK(tq_rf_create(&acc, T, R, want_n[2], NULL) == TQ_OK);
        CHECK(tq_rf_add(acc, reps + 2 * stride, n_nodes + 2, 1, stride, NULL) == TQ_OK);    /* the caterpillar fits */
        CHECK(tq_rf_add(acc, reps + 7 * stride, n_nodes + 7, 1, stride, NULL) == TQ_ERR_INVALID_ARG);
        CHECK(strstr(tq_last_error(NULL), "max_splits"));
        CHECK(tq_rf_read(acc, nsplits, NULL, NULL) == TQ_ERR_INVALID_ARG);
        CHECK(tq_rf_reset(acc) == TQ_OK && tq_rf_add(acc, reps + 2 * stride, n_nodes + 2, 1, stride, NULL) == TQ_OK);
        CHECK(tq_rf_read(acc, nsplits, NULL, NULL) == TQ_OK && nsplits[0] == T - 3);
        tq_rf_destroy(acc);
    }
    free(sides); free(below); free(reps);
}

int main(void)
{
    {   /* outside the limits */
        tq_rf *acc = (tq_rf *)&state;
        CHECK(tq_rf_create(&acc, 3, 4, 4, NULL) == TQ_ERR_INVALID_ARG && acc == NULL);
        acc = (tq_rf *)&state;
        CHECK(tq_rf_create(&acc, 4097, 4, 4, NULL) == TQ_ERR_INVALID_ARG && acc == NULL);
        CHECK(strstr(tq_last_error(NULL), "T must be 4..4096"));
        CHECK(tq_rf_create(&acc, 8, 0, 4, NULL) == TQ_ERR_INVALID_ARG && tq_rf_create(&acc, 8, 8193, 4, NULL) == TQ_ERR_INVALID_ARG);
        CHECK(strstr(tq_last_error(NULL), "max_trees"));
        CHECK(tq_rf_create(&acc, 8, 4, 0, NULL) == TQ_ERR_INVALID_ARG);
        CHECK(strstr(tq_last_error(NULL), "max_splits"));
        CHECK(tq_rf_create(NULL, 8, 4, 4, NULL) == TQ_ERR_INVALID_ARG);
        CHECK(tq_rf_reset(NULL) == TQ_ERR_INVALID_ARG && tq_rf_shape(NULL, NULL, NULL, NULL, NULL, NULL) == TQ_ERR_INVALID_ARG);
        CHECK(tq_rf_read(NULL, NULL, NULL, NULL) == TQ_ERR_INVALID_ARG && tq_rf_stats(NULL, NULL) == TQ_ERR_INVALID_ARG);
        tq_rf_destroy(NULL);
    }
    for (int i = 0; i < 1000; ++i) {    /* the word rule of the product against a loop over the bits */
        const uint64_t x = ((uint64_t)rnd(1u << 31) << 33) ^ ((uint64_t)rnd(1u << 31) << 11) ^ rnd(1u << 11);
        const uint64_t y = i % 7 == 0 ? ~(uint64_t)0 : ((uint64_t)rnd(1u << 31) << 33) ^ ((uint64_t)rnd(1u << 31) << 2) ^ rnd(4);
        uint32_t want = 0;
        for (int b = 0; b < 64; ++b) want += (uint32_t)((x >> b) & (y >> b) & 1);
        CHECK(tq_rf_word_shared(x, y) == want);
    }
    CHECK(tq_rf_word_shared(~(uint64_t)0, ~(uint64_t)0) == 64 && tq_rf_word_shared(~(uint64_t)0, 0) == 0);
    const int32_t sizes[4] = {4, 12, 65, 129};
    for (int i = 0; i < 4; ++i) run(sizes[i]);
    printf("treedist_host_check: ok\n");
    return 0;
}

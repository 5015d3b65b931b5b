/* taxdist_host_check.c -- the host execution of the taxon counts and neighbour joining (tq_taxon_counts_host, tq_nj_tree;
 * DESIGN.md section 29), driven from a plain C program.
 * Built and run under the host sanitizers by tools/host_checks.sh.
 *
 * No device is needed or touched.  The counts of a hand-written matrix of 4 taxa and 70 sites are known by hand, for two
 * blocks that cut inside a 64-site word; those of random matrices are recounted cell by cell, with random blocks; the
 * neighbour-joining tree of a hand-made additive matrix of five taxa is known by hand, ties included.
 * Prints "taxdist_host_check: ok" and returns 0 when every check held; a sanitizer report or a failed check ends it with a
 * non-zero status. */
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

#define CHECK(cond)                                                                 \
    do {                                                                            \
        if (!(cond)) {                                                              \
            fprintf(stderr, "taxdist_host_check: line %d: %s\n", __LINE__, #cond);  \
            exit(1);                                                                \
        }                                                                           \
    } while (0)

static int refused(int rc, const char *word)
{
    return rc == TQ_ERR_INVALID_ARG && strstr(tq_last_error(NULL), word) != NULL;
}

/* four taxa, 70 sites */
enum { T4 = 4, S4 = 70 };
static const char *rows4[T4] = {
    "AAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAA", /* A x 70 */
    "AAAAAAAAAAAAAAAAAAAAGGGGGGGGGGGGGGGGGGGGCCCCCCCCCCCCCCCCCCCCNNNNNNNNNN", /* A x 20, G x 20, C x 20, N x 10 */
    "NNNNNAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAA", /* N x 5, A x 65 */
    "TTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTTNNNNNNNNNNNNNNNNNNNNNNNNNNNNNNGGGGG", /* T x 35, N x 30, G x 5 */
};
/* by hand: (both, diff, ts, tv) of the pairs (0,0) (0,1) (0,2) (0,3) (1,1) (1,2) (1,3) (2,2) (2,3) (3,3), for the blocks
 * [0, 33) and [33, 70) */
static const uint32_t want4[2][10][4] = {
    {{33, 0, 0, 0}, {33, 13, 13, 0}, {28, 0, 0, 0}, {33, 33, 0, 33}, {33, 0, 0, 0},
     {28, 13, 13, 0}, {33, 33, 0, 33}, {28, 0, 0, 0}, {28, 28, 0, 28}, {33, 0, 0, 0}},
    {{37, 0, 0, 0}, {27, 27, 7, 20}, {37, 0, 0, 0}, {7, 7, 5, 2}, {27, 0, 0, 0},
     {27, 27, 7, 20}, {2, 2, 0, 2}, {37, 0, 0, 0}, {7, 7, 5, 2}, {7, 0, 0, 0}},
};

static void hand_matrix(void)
{
    uint8_t arr[T4 * S4];
    for (int t = 0; t < T4; ++t) {
        CHECK(strlen(rows4[t]) == S4);
        for (int s = 0; s < S4; ++s) {
            const char c = rows4[t][s];
            arr[t * S4 + s] = c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : c == 'T' ? 3 : 78;
        }
    }
    const int64_t starts[3] = {0, 33, 70}, whole[2] = {0, 70};
    uint32_t out[2][T4][T4][4], one[T4][T4][4];
    CHECK(tq_taxon_counts_host(arr, T4, S4, starts, 2, &out[0][0][0][0]) == TQ_OK);
    CHECK(tq_taxon_counts_host(arr, T4, S4, whole, 1, &one[0][0][0]) == TQ_OK);
    for (int b = 0; b < 2; ++b) {
        int pair = 0;
        for (int i = 0; i < T4; ++i)
            for (int j = i; j < T4; ++j, ++pair)
                for (int k = 0; k < 4; ++k) {
                    CHECK(out[b][i][j][k] == want4[b][pair][k]);
                    CHECK(out[b][j][i][k] == want4[b][pair][k]);
                }
    }
    for (int i = 0; i < T4; ++i)
        for (int j = 0; j < T4; ++j)
            for (int k = 0; k < 4; ++k) CHECK(one[i][j][k] == out[0][i][j][k] + out[1][i][j][k]);
    CHECK(one[0][1][0] == 60 && one[0][1][1] == 40 && one[0][1][2] == 20 && one[0][1][3] == 20);
}

static void random_matrices(void)
{
    static const uint8_t gone[3] = {4, 78, 255};
    for (int round = 0; round < 30; ++round) {
        const int64_t T = 2 + rnd(8), S = 1 + rnd(round < 10 ? 70 : 400);
        uint8_t *arr = malloc((size_t)(T * S));
        CHECK(arr);
        for (int64_t i = 0; i < T * S; ++i) arr[i] = rnd(4) == 0 ? gone[rnd(3)] : (uint8_t)rnd(4);
        /* blocks: random distinct cuts, so most fall inside a word; the first start and the last end are free */
        int64_t starts[12];
        int B = 0;
        starts[0] = rnd((uint32_t)S);
        while (B < 11 && starts[B] < S) {
            const int64_t next = starts[B] + 1 + rnd(90);
            starts[B + 1] = next > S ? S : next;
            ++B;
            if (rnd(4) == 0) break;
        }
        uint32_t *out = malloc((size_t)(B * T * T) * 4 * sizeof(uint32_t));
        CHECK(out);
        memset(out, 0xAB, (size_t)(B * T * T) * 4 * sizeof(uint32_t));
        CHECK(tq_taxon_counts_host(arr, T, S, starts, B, out) == TQ_OK);
        for (int b = 0; b < B; ++b)
            for (int64_t i = 0; i < T; ++i)
                for (int64_t j = 0; j < T; ++j) {
                    uint32_t both = 0, diff = 0, ts = 0;
                    for (int64_t s = starts[b]; s < starts[b + 1]; ++s) {
                        const uint8_t x = arr[i * S + s], y = arr[j * S + s];
                        if (x > 3 || y > 3) continue;
                        ++both;
                        if (x == y) continue;
                        ++diff;
                        if ((x == 0 && y == 2) || (x == 2 && y == 0) || (x == 1 && y == 3) || (x == 3 && y == 1)) ++ts;
                    }
                    const uint32_t *row = out + ((b * T + i) * T + j) * 4;
                    CHECK(row[0] == both && row[1] == diff && row[2] == ts && row[3] == diff - ts);
                }
        free(out);
        free(arr);
    }
}

static void neighbour_joining(void)
{
    /* ((0:2,1:3):1,(2:4,3:1):2,4:5); the second round ties (0,1) with (4,5): the lower pair is joined */
    static const double d[5][5] = {
        {0, 5, 9, 6, 8}, {5, 0, 10, 7, 9}, {9, 10, 0, 5, 11}, {6, 7, 5, 0, 8}, {8, 9, 11, 8, 0},
    };
    static const int32_t want_parent[8] = {6, 6, 5, 5, 7, 7, 7, -1};
    static const double want_length[8] = {2, 3, 4, 1, 5, 2, 1, 0};
    int32_t parent[8];
    double length[8];
    CHECK(tq_nj_tree(&d[0][0], 5, parent, length) == TQ_OK);
    for (int v = 0; v < 8; ++v) CHECK(parent[v] == want_parent[v] && length[v] == want_length[v]);
    /* three taxa: the end case alone */
    static const double d3[3][3] = {{7, 3, 4}, {3, 7, 5}, {4, 5, 7}};      /* the diagonal is ignored */
    CHECK(tq_nj_tree(&d3[0][0], 3, parent, length) == TQ_OK);
    CHECK(parent[0] == 3 && parent[1] == 3 && parent[2] == 3 && parent[3] == -1);
    CHECK(length[0] == 1 && length[1] == 2 && length[2] == 3 && length[3] == 0);
}

static void refusals(void)
{
    uint8_t arr[3 * 10] = {0};
    uint32_t out[3 * 3 * 3 * 4];
    const int64_t one[2] = {0, 10};
    CHECK(tq_taxon_counts_host(arr, 3, 10, one, 1, out) == TQ_OK);
    CHECK(refused(tq_taxon_counts_host(NULL, 3, 10, one, 1, out), "NULL"));
    CHECK(refused(tq_taxon_counts_host(arr, 3, 10, NULL, 1, out), "NULL"));
    CHECK(refused(tq_taxon_counts_host(arr, 3, 10, one, 1, NULL), "NULL"));
    CHECK(refused(tq_taxon_counts_host(arr, 1, 10, one, 1, out), "T >= 2"));
    CHECK(refused(tq_taxon_counts_host(arr, 3, 0, one, 1, out), "S >= 1"));
    CHECK(refused(tq_taxon_counts_host(arr, 3, 10, one, 0, out), "B=0"));
    CHECK(refused(tq_taxon_counts_host(arr, 3, 10, one, 4097, out), "B=4097"));
    const int64_t same[4] = {0, 5, 5, 10}, down[4] = {0, 7, 5, 10}, neg[2] = {-1, 10}, past[2] = {0, 11};
    CHECK(refused(tq_taxon_counts_host(arr, 3, 10, same, 3, out), "not above"));
    CHECK(refused(tq_taxon_counts_host(arr, 3, 10, down, 3, out), "not above"));
    CHECK(refused(tq_taxon_counts_host(arr, 3, 10, neg, 1, out), "negative"));
    CHECK(refused(tq_taxon_counts_host(arr, 3, 10, past, 1, out), "past"));

    double d[4][4] = {{0, 1, 2, 3}, {1, 0, 2, 3}, {2, 2, 0, 3}, {3, 3, 3, 0}};
    int32_t parent[6];
    double length[6];
    CHECK(tq_nj_tree(&d[0][0], 4, parent, length) == TQ_OK);
    CHECK(refused(tq_nj_tree(&d[0][0], 2, parent, length), "at least 3"));
    CHECK(refused(tq_nj_tree(NULL, 4, parent, length), "NULL"));
    d[1][2] = d[2][1] = NAN;
    CHECK(refused(tq_nj_tree(&d[0][0], 4, parent, length), "pair (1, 2) is not finite"));
    d[1][2] = d[2][1] = INFINITY;
    CHECK(refused(tq_nj_tree(&d[0][0], 4, parent, length), "pair (1, 2) is not finite"));
    d[1][2] = 2;
    d[2][1] = 2.5;
    CHECK(refused(tq_nj_tree(&d[0][0], 4, parent, length), "not symmetric at the pair (1, 2)"));
}

int main(void)
{
    hand_matrix();
    random_matrices();
    neighbour_joining();
    refusals();
    printf("taxdist_host_check: ok\n");
    return 0;
}

/* species_quintet_host_check.c -- the host-only call of DESIGN.md section 23 (tq_pooled_quintet_site_classes: the pooled
 * five-taxon rule for one site, through the functions the kernel runs), driven from a plain C program.
 * Built and run under the host sanitizers by tools/host_checks.sh.
 *
 * No device is needed or touched: the call takes no context.  The five packed words and the sixteen slots are allocated at
 * their exact sizes, so a read or write past either shows as a sanitizer report.  The values are checked against an
 * enumeration of the 1024 patterns in 64-bit integers, on inputs inside the range rule (every count below 2^32).  Prints
 * "species_quintet_host_check: ok" and returns 0 when every check held. */
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

#define CHECK(cond)                                                                                \
    do {                                                                                           \
        if (!(cond)) {                                                                             \
            fprintf(stderr, "species_quintet_host_check: line %d: %s\n", __LINE__, #cond);         \
            exit(1);                                                                               \
        }                                                                                          \
    } while (0)

/* the rule by enumeration: every pattern (x0..x4) weighs n0[x0] n1[x1] n2[x2] n3[x3] n4[x4]; two distinct bases: the class
 * is the "differs from x0" bits of positions 1..4 */
static void enumerate(const uint32_t n[5][4], uint64_t want[16])
{
    memset(want, 0, 16 * sizeof(uint64_t));
    for (int p = 0; p < 1024; ++p) {
        const int x[5] = {p >> 8, (p >> 6) & 3, (p >> 4) & 3, (p >> 2) & 3, p & 3};
        int present = 0, k = 0, bases = 0;
        uint64_t w = 1;
        for (int i = 0; i < 5; ++i) present |= 1 << x[i];
        for (int b = 0; b < 4; ++b) bases += (present >> b) & 1;
        if (bases != 2) continue;
        for (int i = 1; i < 5; ++i) k |= (x[i] != x[0]) << (i - 1);
        for (int i = 0; i < 5; ++i) w *= n[i][x[i]];
        want[k] += w;
        want[0] += w;
    }
}

static void check(const uint32_t n[5][4])
{
    uint32_t *packed = (uint32_t *)malloc(5 * sizeof(uint32_t)), *out = (uint32_t *)malloc(16 * sizeof(uint32_t));
    uint64_t want[16];
    CHECK(packed && out);
    for (int i = 0; i < 5; ++i) packed[i] = n[i][0] | (n[i][1] << 8) | (n[i][2] << 16) | (n[i][3] << 24);
    for (int k = 0; k < 16; ++k) out[k] = 0xABABABABu;
    CHECK(tq_pooled_quintet_site_classes(packed, out) == TQ_OK);
    enumerate(n, want);
    for (int k = 0; k < 16; ++k) CHECK(want[k] < (1ull << 32) && out[k] == (uint32_t)want[k]);
    free(out);
    free(packed);
}

/* a species of `size` lineages spread over the bases, a share of them missing */
static void spread(uint32_t n[4], uint32_t size)
{
    memset(n, 0, 4 * sizeof(uint32_t));
    const uint32_t present = rnd(4) == 0 ? rnd(size + 1) : size;
    const uint32_t bases = 1 + rnd(4);
    for (uint32_t l = 0; l < present; ++l) n[rnd(bases)]++;
}

int main(void)
{
    uint32_t n[5][4];
    uint32_t out[16];
    CHECK(tq_pooled_quintet_site_classes(NULL, out) == TQ_ERR_INVALID_ARG);
    CHECK(tq_pooled_quintet_site_classes(out, NULL) == TQ_ERR_INVALID_ARG);
    CHECK(strstr(tq_last_error(NULL), "tq_pooled_quintet_site_classes"));
    /* all 1024 unit patterns */
    for (int p = 0; p < 1024; ++p) {
        const int x[5] = {p >> 8, (p >> 6) & 3, (p >> 4) & 3, (p >> 2) & 3, p & 3};
        memset(n, 0, sizeof n);
        for (int i = 0; i < 5; ++i) n[i][x[i]] = 1;
        check(n);
    }
    /* four species of 255 on one base, the fifth of size 1 on another: 255^4 in one slot, for each position */
    for (int odd = 0; odd < 5; ++odd) {
        memset(n, 0, sizeof n);
        for (int i = 0; i < 5; ++i) n[i][1] = 255;
        n[odd][1] = 0;
        n[odd][3] = 1;
        check(n);
        for (int i = 0; i < 5; ++i) { n[i][0] = 128; n[i][1] = 0; n[i][2] = 127; n[i][3] = 0; }      /* quadruple dots > 2^24 */
        n[odd][0] = 1;
        n[odd][2] = 0;
        check(n);
    }
    /* random sizes whose product stays below 2^32 */
    for (int r = 0; r < 20000; ++r) {
        uint32_t size[5];
        uint64_t prod;
        do {
            prod = 1;
            for (int i = 0; i < 5; ++i) {
                size[i] = 1 + rnd(1u << (1 + rnd(8)));
                if (size[i] > 255) size[i] = 255;
                prod *= size[i];
            }
        } while (prod >= (1ull << 32));
        for (int i = 0; i < 5; ++i) spread(n[i], size[i]);
        check(n);
    }
    printf("species_quintet_host_check: ok\n");
    return 0;
}

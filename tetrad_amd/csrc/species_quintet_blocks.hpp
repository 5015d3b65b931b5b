// species_quintet_blocks.hpp -- pooled five-taxon site-pattern class counts of species sets per block of sites, from the
// species count table.  Part of the single translation unit tetrad_hip.hip (included inside its
// anonymous namespace, after species_blocks.hpp and quintet_blocks.hpp).
//
// Rule: a species set is five ids k0 < k1 < k2 < k3 < k4; n_i[x] (x = 0..3) is the byte of the species table (species.hpp)
// of species k_i for base x at a site.  The pooled count of class k (1..15, quintet_class of quintet_blocks.hpp) at the
// site is the number of lineage quintets, one lineage per species in position order, whose five bases take exactly two
// values and whose quintet_class is k.  Let M be the positions i >= 1 whose bit i - 1 is set in k, Mc = {0..4} minus M,
// and for a set T of positions d(T) = sum over x of the product over i in T of n_i[x] (a total, a pair dot, a triple
// dot, ...).  Then
//   count_k(site) = d(Mc) d(M) - d({0, 1, 2, 3, 4}):
// the product counts every (x, y) with Mc on base x and M on base y, the quintuple dot takes the x = y cases out.  Two
// values only, so there is no lattice to invert (species_blocks.hpp has one).  A lane sums F_k = d(Mc) d(M) for the 15
// classes and Qn = the quintuple dot over its sites; the subtraction is linear and is done once per (set, block):
// row[k] = F_k - Qn for k = 1..15, row[0] = their sum (pooled5_finish).  Invariant sites and sites with three or four
// bases count nowhere, option count_invariant is not read, a missing lineage is in no byte of the table.
//
// Arithmetic is u32.  Every F_k of a site is at most t_0 t_1 t_2 t_3 t_4 (a sum of products of non-negative terms is at
// most the product of the sums), Qn is at most every F_k, and the five-species range rule (species_quintet_ready: S x
// product of the five largest species sizes < 2^32) bounds the sum over the sites: no F_k, no Qn and no slot wraps.
// Multiplier widths: a species holds at most 255 lineages, so a total is <= 255, a pair dot <= 255^2 and a triple dot
// <= 255^3 < 2^24 (a dot is at most the product of the totals); with the bytes and the products of two or three bytes
// they fit the 24-bit multiplier (pooled_mul).  A quadruple dot reaches 255^4 > 2^24: the five products quadruple dot x
// total take the full multiply (pooled5_mul_full, v_mul_lo_u32), everything else -- the quadruple and quintuple byte
// products included, whose factors are a triple product and a byte or a pair product -- the 24-bit one.
//
// The rows are written by tq_block_rows_kernel<SpeciesQuintetRule> (block_rows.hpp has the kernel, the table walk and the
// rule): per site of the block one dword per species, the 16 sums; lane 0 finishes the summed f.  A species id >= K, or a
// row that repeats species so that it breaks the range rule of five, gives a row of zeros.
#pragma once

// x y modulo 2^32 for any operands (v_mul_lo_u32: quarter rate): where a factor can reach 2^24
constexpr __host__ __device__ uint32_t pooled5_mul_full(uint32_t x, uint32_t y) { return x * y; }

// f[0] += the quintuple dot, f[k] += d(Mc) d(M) of class k = 1..15, for one site, from the packed table entries of the
// five species in position order
constexpr __host__ __device__ void pooled5_site_f(uint32_t n0, uint32_t n1, uint32_t n2, uint32_t n3, uint32_t n4,
                                                  uint32_t (&f)[PAT_ROW])
{
    constexpr uint32_t ONES = 0x01010101u;
    // (the mask tells the compiler that a total is at most 4 x 255, as in pooled_site_f)
    const uint32_t t0 = pooled_dot4(n0, ONES) & 0x3FFu, t1 = pooled_dot4(n1, ONES) & 0x3FFu, t2 = pooled_dot4(n2, ONES) & 0x3FFu;
    const uint32_t t3 = pooled_dot4(n3, ONES) & 0x3FFu, t4 = pooled_dot4(n4, ONES) & 0x3FFu;
    const uint32_t p01 = pooled_dot4(n0, n1), p02 = pooled_dot4(n0, n2), p03 = pooled_dot4(n0, n3), p04 = pooled_dot4(n0, n4);
    const uint32_t p12 = pooled_dot4(n1, n2), p13 = pooled_dot4(n1, n3), p14 = pooled_dot4(n1, n4);
    const uint32_t p23 = pooled_dot4(n2, n3), p24 = pooled_dot4(n2, n4), p34 = pooled_dot4(n3, n4);
    uint32_t d012 = 0, d013 = 0, d014 = 0, d023 = 0, d024 = 0, d034 = 0, d123 = 0, d124 = 0, d134 = 0, d234 = 0;
    uint32_t d0123 = 0, d0124 = 0, d0134 = 0, d0234 = 0, d1234 = 0, q = 0;
    for (int x = 0; x < 4; ++x) {
        const uint32_t a = (n0 >> (8 * x)) & 0xFFu, b = (n1 >> (8 * x)) & 0xFFu, c = (n2 >> (8 * x)) & 0xFFu;
        const uint32_t d = (n3 >> (8 * x)) & 0xFFu, e = (n4 >> (8 * x)) & 0xFFu;
        const uint32_t ab = pooled_mul(a, b), ac = pooled_mul(a, c), bc = pooled_mul(b, c), de = pooled_mul(d, e);
        const uint32_t abc = pooled_mul(ab, c);
        d012 += abc;
        d013 += pooled_mul(ab, d);
        d014 += pooled_mul(ab, e);
        d023 += pooled_mul(ac, d);
        d024 += pooled_mul(ac, e);
        d034 += pooled_mul(de, a);
        d123 += pooled_mul(bc, d);
        d124 += pooled_mul(bc, e);
        d134 += pooled_mul(de, b);
        d234 += pooled_mul(de, c);
        d0123 += pooled_mul(abc, d);
        d0124 += pooled_mul(abc, e);
        d0134 += pooled_mul(ab, de);
        d0234 += pooled_mul(ac, de);
        d1234 += pooled_mul(bc, de);
        q += pooled_mul(abc, de);
    }
    f[0] += q;                                  //        {01234}
    f[1] += pooled5_mul_full(d0234, t1);        // 0001   {0234}{1}
    f[2] += pooled5_mul_full(d0134, t2);        // 0010   {0134}{2}
    f[3] += pooled_mul(d034, p12);              // 0011   {034}{12}
    f[4] += pooled5_mul_full(d0124, t3);        // 0100   {0124}{3}
    f[5] += pooled_mul(d024, p13);              // 0101   {024}{13}
    f[6] += pooled_mul(d014, p23);              // 0110   {014}{23}
    f[7] += pooled_mul(d123, p04);              // 0111   {04}{123}
    f[8] += pooled5_mul_full(d0123, t4);        // 1000   {0123}{4}
    f[9] += pooled_mul(d023, p14);              // 1001   {023}{14}
    f[10] += pooled_mul(d013, p24);             // 1010   {013}{24}
    f[11] += pooled_mul(d124, p03);             // 1011   {03}{124}
    f[12] += pooled_mul(d012, p34);             // 1100   {012}{34}
    f[13] += pooled_mul(d134, p02);             // 1101   {02}{134}
    f[14] += pooled_mul(d234, p01);             // 1110   {01}{234}
    f[15] += pooled5_mul_full(d1234, t0);       // 1111   {0}{1234}
}

// the class row of the sums: row[k] = F_k - Qn for k = 1..15 (never negative: Qn counts a subset of what F_k counts),
// row[0] = their sum
__host__ __device__ __forceinline__ constexpr void pooled5_finish(const uint32_t (&f)[PAT_ROW], uint32_t (&row)[PAT_ROW])
{
    row[0] = 0;
#pragma unroll
    for (int k = 1; k < PAT_ROW; ++k) {
        row[k] = f[k] - f[0];
        row[0] += row[k];
    }
}

// one site with unit count vectors is one pattern: it must land in exactly the slot quintet_class gives it (and in the
// total), or nowhere, for all 1024 patterns
constexpr bool pooled5_rule_ok()
{
    for (int p = 0; p < 1024; ++p) {
        const int x0 = p >> 8, x1 = (p >> 6) & 3, x2 = (p >> 4) & 3, x3 = (p >> 2) & 3, x4 = p & 3;
        uint32_t f[PAT_ROW] = {}, row[PAT_ROW] = {};
        pooled5_site_f(1u << (8 * x0), 1u << (8 * x1), 1u << (8 * x2), 1u << (8 * x3), 1u << (8 * x4), f);
        pooled5_finish(f, row);
        const int want = quintet_class(x0, x1, x2, x3, x4);
        for (int c = 1; c < PAT_ROW; ++c)
            if (row[c] != (c == want ? 1u : 0u)) return false;
        if (row[0] != (want > 0 ? 1u : 0u)) return false;
    }
    return true;
}
static_assert(pooled5_rule_ok(), "the pooled five-taxon counts must follow quintet_class");

// The row's own range rule, five ids: S x n_0 n_1 n_2 n_3 n_4 < 2^32 (species_row_in_range for four).  The lineage product
// can pass 2^32 by itself (255^5), so it is judged before it is multiplied by S.
__device__ __forceinline__ bool species_row5_in_range(const int32_t *__restrict__ offsets, uint32_t k0, uint32_t k1, uint32_t k2,
                                                      uint32_t k3, uint32_t k4, int64_t S)
{
    const uint64_t p = (uint64_t)(offsets[k0 + 1] - offsets[k0]) * (uint64_t)(offsets[k1 + 1] - offsets[k1]) *
                       (uint64_t)(offsets[k2 + 1] - offsets[k2]) * (uint64_t)(offsets[k3 + 1] - offsets[k3]) *
                       (uint64_t)(offsets[k4 + 1] - offsets[k4]);
    return (uint64_t)S < (1ull << 32) && p < (1ull << 32) && (uint64_t)S * p < (1ull << 32);
}

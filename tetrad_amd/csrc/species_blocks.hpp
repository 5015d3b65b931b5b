// species_blocks.hpp -- pooled site-pattern class counts of species sets per block of sites, from the species count table
// (DESIGN.md section 21).  Part of the single translation unit tetrad_hip.hip (included inside its anonymous namespace,
// after species.hpp and pattern_blocks.hpp).
//
// Rule: for a species set (A, B, C, D) and a site s let a[x], b[x], c[x], d[x] (x = 0..3) be the bytes of the species
// table (species.hpp: lineages of the species with base x at s).  The pooled count of class k at s is the sum of
// a[x0] b[x1] c[x2] d[x3] over the patterns with pattern_class(x0, x1, x2, x3) = k; a block row is u32[16] = these counts
// summed over the block's sites, class 0 (xxxx) always 0 as in the pooled matrix of section 12, slot 15 = the sum of
// slots 1..14.
//
// A class is a set partition of the four positions (its restricted-growth string).  For a partition sigma let
//   f(sigma) = product over the blocks of sigma of  sum_x  product over i in the block of n_i[x]:
// 4 totals, 6 pair dots, 4 triple dots and 1 quadruple dot give all 15 (pooled_site_f).  f(sigma) counts the patterns
// whose partition is sigma or coarser, so the exact counts follow by Moebius inversion on the partition lattice,
//   count(pi) = sum over sigma >= pi of mu(pi, sigma) f(sigma),
//   mu(pi, sigma) = product over the blocks of sigma of (-1)^(m - 1) (m - 1)!,  m = blocks of pi merged into that block.
// The inversion is linear with integer coefficients: it is applied once per (set, block) to the f sums over the block's
// sites (pooled_invert), not per site.
//
// Arithmetic is u32 modulo 2^32.  Every f(sigma) of a site is at most f(all singletons) = t_A t_B t_C t_D (a sum of
// products of non-negative terms is at most the product of the sums), and the range rule of section 12 (species_ready:
// S x product of the four largest species sizes < 2^32) bounds the sum of that over the sites.  So no f sum and no class
// count wraps; only the signed intermediate steps of the inversion rely on the wrap-around.
//
// The rows are written by tq_block_rows_kernel<SpeciesRule> (block_rows.hpp has the kernel, the table walk and the rule):
// per site of the block the four species' packed entries, the 15 products, 15 adds; lane 0 inverts the summed f.  A
// species id >= K, or a row that repeats species so that it breaks the range rule, gives a row of zeros.
#pragma once

// sum of the four byte products of two packed words: one v_dot4_u32_u8 on the device
constexpr __host__ __device__ uint32_t pooled_dot4(uint32_t a, uint32_t b)
{
#if defined(__HIP_DEVICE_COMPILE__)
    if (!__builtin_is_constant_evaluated()) return __builtin_amdgcn_udot4(a, b, 0u, false);
#endif
    return (a & 0xFFu) * (b & 0xFFu) + ((a >> 8) & 0xFFu) * ((b >> 8) & 0xFFu) + ((a >> 16) & 0xFFu) * ((b >> 16) & 0xFFu) +
           (a >> 24) * (b >> 24);
}

// x y for operands below 2^24 (every factor here is: a byte, a product of two bytes or two totals, a pair dot <= 255^2, a
// triple dot <= 255^3 < 2^24) and a product below 2^32: the 24-bit multiplier of the device (v_mul_u32_u24 /
// v_mad_u32_u24, full rate; v_mul_lo_u32 is not) gives the same 32 bits
constexpr __host__ __device__ uint32_t pooled_mul(uint32_t x, uint32_t y)
{
#if defined(__HIP_DEVICE_COMPILE__)
    if (!__builtin_is_constant_evaluated()) return __umul24(x, y);
#endif
    return x * y;
}

// f[class of sigma] += f(sigma) of one site, from the packed table entries of the four species
constexpr __host__ __device__ void pooled_site_f(uint32_t a, uint32_t b, uint32_t c, uint32_t d, uint32_t (&f)[PAT_CLASSES])
{
    constexpr uint32_t ONES = 0x01010101u;
    // (a total is at most 4 x 255: the mask changes nothing and tells the compiler so -- without it the products of two
    // totals below, of which only 24 bits are used further on, come out as full 32-bit multiplies)
    const uint32_t tA = pooled_dot4(a, ONES) & 0x3FFu, tB = pooled_dot4(b, ONES) & 0x3FFu;
    const uint32_t tC = pooled_dot4(c, ONES) & 0x3FFu, tD = pooled_dot4(d, ONES) & 0x3FFu;
    const uint32_t pAB = pooled_dot4(a, b), pAC = pooled_dot4(a, c), pAD = pooled_dot4(a, d);
    const uint32_t pBC = pooled_dot4(b, c), pBD = pooled_dot4(b, d), pCD = pooled_dot4(c, d);
    uint32_t tABC = 0, tABD = 0, tACD = 0, tBCD = 0, q = 0;
    for (int x = 0; x < 4; ++x) {
        const uint32_t ax = (a >> (8 * x)) & 0xFFu, bx = (b >> (8 * x)) & 0xFFu;
        const uint32_t cx = (c >> (8 * x)) & 0xFFu, dx = (d >> (8 * x)) & 0xFFu;
        const uint32_t ab = pooled_mul(ax, bx), cd = pooled_mul(cx, dx);
        tABC += pooled_mul(ab, cx);
        tABD += pooled_mul(ab, dx);
        tACD += pooled_mul(ax, cd);
        tBCD += pooled_mul(bx, cd);
        q += pooled_mul(ab, cd);
    }
    const uint32_t tAB = pooled_mul(tA, tB), tAC = pooled_mul(tA, tC), tAD = pooled_mul(tA, tD);
    const uint32_t tBC = pooled_mul(tB, tC), tBD = pooled_mul(tB, tD), tCD = pooled_mul(tC, tD);
    f[0] += q;                          // 0000  {ABCD}
    f[1] += pooled_mul(tABC, tD);       // 0001  {ABC}{D}
    f[2] += pooled_mul(tABD, tC);       // 0010  {ABD}{C}
    f[3] += pooled_mul(pAB, pCD);       // 0011  {AB}{CD}
    f[4] += pooled_mul(pAB, tCD);       // 0012  {AB}{C}{D}
    f[5] += pooled_mul(tACD, tB);       // 0100  {ACD}{B}
    f[6] += pooled_mul(pAC, pBD);       // 0101  {AC}{BD}
    f[7] += pooled_mul(pAC, tBD);       // 0102  {AC}{B}{D}
    f[8] += pooled_mul(pAD, pBC);       // 0110  {AD}{BC}
    f[9] += pooled_mul(tBCD, tA);       // 0111  {A}{BCD}
    f[10] += pooled_mul(pBC, tAD);      // 0112  {A}{BC}{D}
    f[11] += pooled_mul(pAD, tBC);      // 0120  {AD}{B}{C}
    f[12] += pooled_mul(pBD, tAC);      // 0121  {A}{BD}{C}
    f[13] += pooled_mul(pCD, tAB);      // 0122  {A}{B}{CD}
    f[14] += pooled_mul(tAB, tCD);      // 0123  {A}{B}{C}{D}
}

// label of position i (0..3) in the restricted-growth string of class k
constexpr __host__ __device__ int pooled_label(int k, int i)
{
    int rank = 0, s = 0;
    for (; s < 64; ++s)
        if (pattern_rgs_valid(s) && rank++ == k) break;
    return i == 0 ? 0 : (s >> (2 * (3 - i))) & 3;
}

// mu(pi, sigma) of the partition lattice for the classes pi and sigma; 0 unless sigma is pi or coarser
constexpr __host__ __device__ int pooled_mobius(int pi, int sigma)
{
    const int lp[4] = {0, pooled_label(pi, 1), pooled_label(pi, 2), pooled_label(pi, 3)};
    const int ls[4] = {0, pooled_label(sigma, 1), pooled_label(sigma, 2), pooled_label(sigma, 3)};
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < i; ++j)
            if (lp[i] == lp[j] && ls[i] != ls[j]) return 0;
    int mu = 1;
    for (int blk = 0; blk < 4; ++blk) {         // the blocks of sigma by label
        int m = 0;                              // blocks of pi inside it: positions that open a pi label
        for (int i = 0; i < 4; ++i) {
            if (ls[i] != blk) continue;
            bool opens = true;
            for (int j = 0; j < i; ++j) opens = opens && lp[j] != lp[i];
            m += opens ? 1 : 0;
        }
        for (int t = 1; t < m; ++t) mu *= -t;   // (-1)^(m - 1) (m - 1)!
    }
    return mu;
}

// (a static member is evaluated once; a constexpr local would be evaluated again in every step of the check below)
template <int PI, int SIGMA>
struct PooledMu {
    static constexpr int value = pooled_mobius(PI, SIGMA);
};

template <int PI, int SIGMA>
__host__ __device__ __forceinline__ constexpr uint32_t pooled_invert_from(const uint32_t (&f)[PAT_CLASSES])
{
    constexpr int mu = PooledMu<PI, SIGMA>::value;
    uint32_t v = 0;
    if constexpr (mu != 0) v = (uint32_t)mu * f[SIGMA];
    if constexpr (SIGMA > 0) v += pooled_invert_from<PI, SIGMA - 1>(f);     // a coarser partition has a smaller string
    return v;
}

template <int PI>
__host__ __device__ __forceinline__ constexpr void pooled_invert_class(const uint32_t (&f)[PAT_CLASSES], uint32_t (&row)[PAT_ROW])
{
    row[PI] = pooled_invert_from<PI, PI>(f);
    row[PAT_CLASSES] += row[PI];
    if constexpr (PI + 1 < PAT_CLASSES) pooled_invert_class<PI + 1>(f, row);
}

// the class row of f sums: row[0] = 0 (the invariant bins of the pooled matrix are zeroed, whatever count_invariant says),
// row[k] = count(class k) for k = 1..14, row[15] = their sum.  Signed coefficients as u32: exact modulo 2^32, and the
// counts themselves are below 2^32 (see the head of this file).
__host__ __device__ __forceinline__ constexpr void pooled_invert(const uint32_t (&f)[PAT_CLASSES], uint32_t (&row)[PAT_ROW])
{
    row[0] = 0;
    row[PAT_CLASSES] = 0;
    pooled_invert_class<1>(f, row);
}

// one site with unit count vectors is one pattern: it must land in exactly the class pattern_class gives it (class 0
// nowhere), for all 256 patterns
constexpr bool pooled_rule_ok()
{
    for (int p = 0; p < 256; ++p) {
        const int x0 = p >> 6, x1 = (p >> 4) & 3, x2 = (p >> 2) & 3, x3 = p & 3;
        uint32_t f[PAT_CLASSES] = {}, row[PAT_ROW] = {};
        pooled_site_f(1u << (8 * x0), 1u << (8 * x1), 1u << (8 * x2), 1u << (8 * x3), f);
        pooled_invert(f, row);
        const int want = pattern_class(x0, x1, x2, x3);
        for (int c = 0; c < PAT_CLASSES; ++c)
            if (row[c] != (c == want && c != 0 ? 1u : 0u)) return false;
        if (row[PAT_CLASSES] != (want != 0 ? 1u : 0u)) return false;
    }
    return true;
}
static_assert(pooled_rule_ok(), "the inverted partition sums must follow pattern_class");

// pattern_blocks.hpp -- site-pattern class counts per (set, block of sites) from the bit planes, and the delete-one-block
// jackknife of D on top of them.  Part of the single translation unit tetrad_hip.hip (included
// inside its anonymous namespace, after patterns.hpp).
//
// Rule (full mode only): a site is counted for a set (a, b, c, d) when none of the four bases is missing and -- unless
// option count_invariant is set -- the four are not all equal.  Its class is the restricted-growth string of
// patterns.hpp.  Block j of `starts` i64[B + 1] is sites [starts[j], starts[j + 1]) of the resident replicate; a block
// row is u32[16] = the 15 class counts of the block's sites and their sum.
//
// The rows are written by tq_block_rows_kernel<QuartetRule> (block_rows.hpp has the kernel, the plane walk and the rule):
// per word of the block four plane records, six equality words, the 15 class masks as products of the equality words and
// their complements (pattern_masks), 15 popcount-adds.  A taxon >= T gives a row of zeros.
//
// dstat_jackknife_row: Busing, Meijer & van der Leeden 1999, block weight m_j = a_j + b_j, every floating operation
// rounded once and in one fixed order (see the function), so device, host and Python floats agree bit for bit.
#pragma once

constexpr int PBLK_THREADS = 256;           // 4 wavefronts = 16 items per workgroup
constexpr int PBLK_ITEMS = PBLK_THREADS / 16;
constexpr int JK_THREADS = 128;
constexpr int64_t PBLK_MAX_BLOCKS = 4096;

// The 15 class masks of 32 sites from the six equality words (e_xy: position x and y hold the same base).  `on` is
// AND-ed into every mask.  One definition for the kernel and for the compile-time check below.
struct PatternMasks {
    uint32_t m[PAT_CLASSES];
};

constexpr __host__ __device__ PatternMasks pattern_masks(uint32_t e01, uint32_t e02, uint32_t e03, uint32_t e12, uint32_t e13,
                                                         uint32_t e23, uint32_t on)
{
    PatternMasks r{};
    const uint32_t s = on & e01, d = on & ~e01;        // x1 = x0 / x1 new
    const uint32_t s2 = s & e02, n2 = s & ~e02;        // 000. / 001.
    r.m[0] = s2 & e03;                                 // 0000
    r.m[1] = s2 & ~e03;                                // 0001
    r.m[2] = n2 & e03;                                 // 0010
    const uint32_t n23 = n2 & ~e03;
    r.m[3] = n23 & e23;                                // 0011
    r.m[4] = n23 & ~e23;                               // 0012
    const uint32_t d0 = d & e02;                       // 010.
    r.m[5] = d0 & e03;                                 // 0100
    const uint32_t d0n = d0 & ~e03;
    r.m[6] = d0n & e13;                                // 0101
    r.m[7] = d0n & ~e13;                               // 0102
    const uint32_t dn = d & ~e02;
    const uint32_t d1 = dn & e12;                      // 011.
    r.m[8] = d1 & e03;                                 // 0110
    const uint32_t d1n = d1 & ~e03;
    r.m[9] = d1n & e13;                                // 0111
    r.m[10] = d1n & ~e13;                              // 0112
    const uint32_t d2 = dn & ~e12;                     // 012.
    r.m[11] = d2 & e03;                                // 0120
    const uint32_t d2n = d2 & ~e03;
    r.m[12] = d2n & e13;                               // 0121
    const uint32_t d2nn = d2n & ~e13;
    r.m[13] = d2nn & e23;                              // 0122
    r.m[14] = d2nn & ~e23;                             // 0123
    return r;
}

// every one of the 256 patterns sets exactly the mask of its class (pattern_class, patterns.hpp)
constexpr bool pattern_masks_ok()
{
    for (int p = 0; p < 256; ++p) {
        const int x0 = p >> 6, x1 = (p >> 4) & 3, x2 = (p >> 2) & 3, x3 = p & 3;
        const PatternMasks r = pattern_masks(x0 == x1, x0 == x2, x0 == x3, x1 == x2, x1 == x3, x2 == x3, 1u);
        const int want = pattern_class(x0, x1, x2, x3);
        for (int c = 0; c < PAT_CLASSES; ++c)
            if (r.m[c] != (c == want ? 1u : 0u)) return false;
    }
    return true;
}
static_assert(pattern_masks_ok(), "the class masks must follow pattern_class");

struct PlaneRec {
    uint32_t miss, b0, b1;
};

__device__ __forceinline__ PlaneRec pblk_load(const uint32_t *row, int64_t w)
{
    typedef uint32_t v3 __attribute__((ext_vector_type(3)));
    const v3 v = *reinterpret_cast<const v3 *>(row + w * 3);
    return PlaneRec{v.x, v.y, v.z};
}

__device__ __forceinline__ uint32_t pblk_eq(const PlaneRec &x, const PlaneRec &y)
{
    return ~((x.b0 ^ y.b0) | (x.b1 ^ y.b1));
}

// The delete-one-block jackknife of one test.  rows = the B block rows u32[B][16] of the test's set, fetch = how a row
// gives (a_j, b_j): the classes that play ABBA and BABA (JackknifeClassPair) or two sums of slots (quintet_blocks.hpp).  Returns {g, theta, theta_J, var}: g = blocks with a_j + b_j > 0, theta = (A - Bs) / n over all
// blocks, theta_J the jackknife estimate and var the jackknife variance with block weight m_j = a_j + b_j (Busing et
// al. 1999).  n = 0: {0, NaN, NaN, NaN}; g < 2: {g, theta, NaN, NaN}.  The integers are exact (B <= 4096 blocks
// of at most 15 slots below 2^32 a side: n < 2^48).  Every floating operation is one correctly rounded f64 operation in the order written: contraction
// is off for this function (see dstat_add, patterns.hpp), so the products and sums stay apart on the device as well.
struct JackknifeRow {
    double g, theta, theta_j, var;
};

// How a block's (a_j, b_j) is fetched from its row: the class-index form of the four-taxon D test.  The mask form of
// quintet_blocks.hpp (sums of slots) is the other instantiation; the rule below is stated once for both.
struct JackknifeClassPair {
    uint32_t ca, cb;
    __host__ __device__ __forceinline__ void operator()(const uint32_t *row, uint64_t &a, uint64_t &b) const
    {
        a = row[ca];
        b = row[cb];
    }
};

template <class Fetch>
__host__ __device__ __forceinline__ JackknifeRow dstat_jackknife_row(const uint32_t *rows, int64_t B, const Fetch fetch)
{
#pragma clang fp contract(off)
    const double qnan = __builtin_bit_cast(double, (uint64_t)0x7FF8000000000000ull);
    uint64_t A = 0, Bs = 0, g = 0;
    for (int64_t j = 0; j < B; ++j) {
        uint64_t a, b;
        fetch(rows + j * PAT_ROW, a, b);
        A += a;
        Bs += b;
        g += (a + b) > 0 ? 1u : 0u;
    }
    const uint64_t n = A + Bs;
    if (n == 0) return JackknifeRow{0.0, qnan, qnan, qnan};
    const double nf = (double)n, gf = (double)g;
    const double theta = (double)((int64_t)A - (int64_t)Bs) / nf;
    if (g < 2) return JackknifeRow{gf, theta, qnan, qnan};
    double sJ = 0.0;
    for (int64_t j = 0; j < B; ++j) {
        uint64_t a, b;
        fetch(rows + j * PAT_ROW, a, b);
        const uint64_t m = a + b;
        if (m == 0) continue;
        const double r = (double)(n - m);
        const double tj = (double)((int64_t)(A - a) - (int64_t)(Bs - b)) / r;
        const double wgt = r / nf;
        const double p = wgt * tj;
        sJ = sJ + p;
    }
    const double gt = gf * theta;
    const double thetaJ = gt - sJ;
    double sV = 0.0;
    for (int64_t j = 0; j < B; ++j) {
        uint64_t a, b;
        fetch(rows + j * PAT_ROW, a, b);
        const uint64_t m = a + b;
        if (m == 0) continue;
        const double r = (double)(n - m);
        const double tj = (double)((int64_t)(A - a) - (int64_t)(Bs - b)) / r;
        const double h = nf / (double)m;
        const double h1 = h - 1.0;
        const double ht = h * theta;
        const double hj = h1 * tj;
        const double tau = ht - hj;
        const double e = tau - thetaJ;
        const double ee = e * e;
        const double q = ee / h1;
        sV = sV + q;
    }
    return JackknifeRow{gf, theta, thetaJ, sV / gf};
}

// The test forms of the jackknife: how test t names its (a_j, b_j).  A form holds the two per-test arrays a and b and
// gives the Fetch of test t, whether that Fetch is a valid test, and the text of the host forms' refusal (arguments: who,
// t, a[t], b[t]).  ClassPairTests: two u8 class indices below 15, the classes that play ABBA and BABA.
// MaskPairTests is in quintet_blocks.hpp.
struct ClassPairTests {
    const uint8_t *a, *b;
    static constexpr const char *refusal = "%s: test %lld has a class index above 14 (%u, %u)";
    __host__ __device__ __forceinline__ JackknifeClassPair operator[](int64_t t) const { return JackknifeClassPair{a[t], b[t]}; }
    static __host__ __device__ __forceinline__ bool valid(const JackknifeClassPair &p)
    {
        return p.ca < (uint32_t)PAT_CLASSES && p.cb < (uint32_t)PAT_CLASSES;
    }
};

__host__ __device__ __forceinline__ void jackknife_store(double *out, int64_t t, const JackknifeRow &r)
{
    out[4 * t + 0] = r.g;
    out[4 * t + 1] = r.theta;
    out[4 * t + 2] = r.theta_j;
    out[4 * t + 3] = r.var;
}

// test t reads the block rows of set set_of[t]; one thread per test.  An invalid test (set_of out of range, or not valid
// by its form): the thread returns without touching memory.  The output row is overwritten.
template <class Tests>
__global__ __launch_bounds__(JK_THREADS) void tq_jackknife_kernel(const uint32_t *__restrict__ bclasses, int64_t n_sets, int64_t B,
                                                                  const uint32_t *__restrict__ set_of, const Tests tests,
                                                                  int64_t N, double *__restrict__ out)
{
    const int64_t t = (int64_t)blockIdx.x * JK_THREADS + threadIdx.x;
    if (t >= N) return;
    const uint32_t s = set_of[t];
    const auto fetch = tests[t];
    const bool valid = Tests::valid(fetch);     // judged before the branch: the three loads go out together
    if ((int64_t)s >= n_sets || !valid) return;
    jackknife_store(out, t, dstat_jackknife_row(bclasses + (int64_t)s * B * PAT_ROW, B, fetch));
}

// the host execution; the caller has checked set_of and the tests
template <class Tests>
inline void jackknife_host(const uint32_t *bclasses, int64_t B, const uint32_t *set_of, const Tests tests, int64_t N, double *out)
{
    for (int64_t t = 0; t < N; ++t)
        jackknife_store(out, t, dstat_jackknife_row(bclasses + (int64_t)set_of[t] * B * PAT_ROW, B, tests[t]));
}

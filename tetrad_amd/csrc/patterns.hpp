// patterns.hpp -- the 15 site-pattern classes of a quartet and the ABBA-BABA D statistic with bootstrap moments
// (DESIGN.md section 18).  Part of the single translation unit tetrad_hip.hip (included inside its anonymous namespace).
//
// Rule (one constexpr function, `pattern_class`, for the host table, the kernel and the tests): a pattern is four
// bases (x0, x1, x2, x3) in the order of the quartet's taxa, slab index 64 x0 + 16 x1 + 4 x2 + x3.  Its class is its
// restricted-growth string -- position 0 gets label 0, every base not seen before the next label -- and the 15
// strings in lexicographic order number the classes: 0000 0001 0010 0011 0012 0100 0101 0102 0110 0111 0112 0120
// 0121 0122 0123.  A class row is u32[16]: the 15 class counts and their sum.
//
// tq_pattern_class_kernel: 16 lanes per quartet, four quartets per wavefront; lane l of a group owns matrix row
// (x0, x1) = (l / 4, l % 4), 16 counts = 64 contiguous bytes, read as four 16-byte loads (a wavefront reads 4 KiB
// contiguous).  The class of a pattern does not change when the four bases are renamed, so a lane renames them by the
// permutation that sends x0 to 0 (and x1 to 1 when it differs; the others keep their order): the row permutation is
// folded into the addresses of the four loads, the column permutation is three selects per count, and after that
// every count sits at a compile-time position (0, 0 or 1, y2, y3) whose class is a constant.  The 16 lanes are summed
// with four DPP butterfly steps inside their row and one lane stores the 64-byte class row.  No LDS, no scratch,
// u32 end to end (33 VGPRs, 24 SGPRs, group segment 0 on gfx950).
//
// tq_dstat_kernel: one thread per test adds the replicate's D = (a - b) / (a + b) to {n, sum, sum of squares, last}
// with `dstat_add`, the function the host execution runs: every operation rounded once, product and sum kept apart.
#pragma once

constexpr int PAT_CLASSES = 15;
constexpr int PAT_ROW = 16;                 // u32 per class row: 15 classes + their sum
constexpr int PAT_THREADS = 256;            // 4 wavefronts = 16 quartets per workgroup
constexpr int DSTAT_THREADS = 256;

// restricted-growth labels of a pattern as l1 * 16 + l2 * 4 + l3 (l0 = 0)
constexpr __host__ __device__ int pattern_rgs(int x0, int x1, int x2, int x3)
{
    int next = 1;
    const int l1 = x1 == x0 ? 0 : next++;
    const int l2 = x2 == x0 ? 0 : (x2 == x1 ? l1 : next++);
    const int l3 = x3 == x0 ? 0 : (x3 == x1 ? l1 : (x3 == x2 ? l2 : next++));
    return l1 * 16 + l2 * 4 + l3;
}

// a restricted-growth string: every label is at most one above the largest label before it
constexpr __host__ __device__ bool pattern_rgs_valid(int s)
{
    const int l1 = s >> 4, l2 = (s >> 2) & 3, l3 = s & 3;
    const int m2 = l2 > l1 ? l2 : l1;
    return l1 <= 1 && l2 <= l1 + 1 && l3 <= m2 + 1;
}

// class = the rank of the pattern's string among the restricted-growth strings (lexicographic = numeric in base 4)
constexpr __host__ __device__ int pattern_class(int x0, int x1, int x2, int x3)
{
    const int mine = pattern_rgs(x0, x1, x2, x3);
    int rank = 0;
    for (int s = 0; s < mine; ++s) rank += pattern_rgs_valid(s) ? 1 : 0;
    return rank;
}

// the lane's renaming of the bases: inv[y] = the base that is called y.  x0 -> 0, x1 -> 1 when it differs, the rest
// in ascending order.
constexpr __host__ __device__ int pattern_inv(int x0, int x1, int y)
{
    if (y == 0) return x0;
    if (x1 != x0 && y == 1) return x1;
    int left = y - (x1 != x0 ? 2 : 1);
    for (int b = 0; b < 4; ++b)
        if (b != x0 && b != x1 && left-- == 0) return b;
    return -1;
}

// what the kernel relies on: the rule has 15 classes, and the class of (x0, x1, inv[y2], inv[y3]) is the class of
// (0, x0 != x1, y2, y3) for every lane
constexpr bool pattern_rule_ok()
{
    int top = 0;
    for (int p = 0; p < 256; ++p) {
        const int c = pattern_class(p >> 6, (p >> 4) & 3, (p >> 2) & 3, p & 3);
        top = c > top ? c : top;
    }
    if (top != PAT_CLASSES - 1) return false;
    for (int r = 0; r < 16; ++r)
        for (int y = 0; y < 16; ++y) {
            const int x0 = r >> 2, x1 = r & 3;
            const int x2 = pattern_inv(x0, x1, y >> 2), x3 = pattern_inv(x0, x1, y & 3);
            if (x2 < 0 || x3 < 0) return false;
            if (pattern_class(x0, x1, x2, x3) != pattern_class(0, x0 != x1 ? 1 : 0, y >> 2, y & 3)) return false;
        }
    return true;
}
static_assert(pattern_rule_ok(), "the class rule must be invariant under renaming the bases");

// c[class of (0, 0, y2, y3)] and c[class of (0, 1, y2, y3)] += w[4 y2 + y3], all indices compile-time
template <int E>
__device__ __forceinline__ void pattern_add_renamed(uint32_t (&c)[PAT_CLASSES], const uint32_t (&w)[16])
{
    constexpr int same = pattern_class(0, 0, E >> 2, E & 3), diff = pattern_class(0, 1, E >> 2, E & 3);
    c[same] += w[E];
    c[diff] += w[E];
    if constexpr (E < 15) pattern_add_renamed<E + 1>(c, w);
}

__device__ __forceinline__ uint32_t pattern_row_sum(uint32_t v)
{
    v += (uint32_t)dpp_xor16<1>((int)v);
    v += (uint32_t)dpp_xor16<2>((int)v);
    v += (uint32_t)dpp_xor16<7>((int)v);
    v += (uint32_t)dpp_xor16<15>((int)v);
    return v;
}

// the renamings of the 16 lanes, one byte per lane: bits 2y, 2y + 1 = inv[y]; lanes 0..7 and 8..15
constexpr uint64_t pattern_inv_pack(int first_lane)
{
    uint64_t v = 0;
    for (int l = 0; l < 8; ++l)
        for (int y = 0; y < 4; ++y)
            v |= (uint64_t)pattern_inv((first_lane + l) >> 2, (first_lane + l) & 3, y) << (8 * l + 2 * y);
    return v;
}

// cm u32[n][256] (rows of the count slab) -> classes u32[n][16]
__global__ __launch_bounds__(PAT_THREADS) void tq_pattern_class_kernel(const uint32_t *__restrict__ cm, int64_t n,
                                                                       uint32_t *__restrict__ classes)
{
    const int l = threadIdx.x & 15;
    const int64_t q = (int64_t)blockIdx.x * (PAT_THREADS / 16) + (threadIdx.x >> 4);
    const bool live = q < n;                    // the same for the 16 lanes of a DPP row
    const bool same = (l >> 2) == (l & 3);      // x0 == x1
    constexpr uint64_t INV_LO = pattern_inv_pack(0), INV_HI = pattern_inv_pack(8);
    const uint32_t inv = (uint32_t)((l < 8 ? INV_LO : INV_HI) >> (8 * (l & 7))) & 0xFFu;
    // a group past the end reads row 0 (n >= 1) and stores nothing: no lane of another group sees its values
    const uint4 *row = reinterpret_cast<const uint4 *>(cm + (size_t)(live ? q : 0) * 256 + l * 16);
    // the four column selectors of the lane, once; every loaded count is then chosen by two of them.  The loaded row
    // stays one value per iteration (no array of rows): an indexed private array would be promoted to LDS
    bool odd[4], high[4];
#pragma unroll
    for (int y3 = 0; y3 < 4; ++y3) {
        odd[y3] = ((inv >> (2 * y3)) & 1u) != 0;
        high[y3] = ((inv >> (2 * y3)) & 2u) != 0;
    }
    uint32_t w[16];
#pragma unroll
    for (int y2 = 0; y2 < 4; ++y2) {
        const uint4 u = row[(inv >> (2 * y2)) & 3u];
        const uint32_t ux = u.x, uy = u.y, uz = u.z, uw = u.w;
#pragma unroll
        for (int y3 = 0; y3 < 4; ++y3) {
            const uint32_t xy = odd[y3] ? uy : ux, zw = odd[y3] ? uw : uz;
            w[4 * y2 + y3] = high[y3] ? zw : xy;
        }
    }
    uint32_t c[PAT_CLASSES];
#pragma unroll
    for (int i = 0; i < PAT_CLASSES; ++i) c[i] = 0;
    pattern_add_renamed<0>(c, w);
    // a row with x0 == x1 reaches the classes 00.. only (0..4), any other row the classes 01.. only (5..14)
    constexpr int FIRST_DIFF = pattern_class(0, 1, 0, 0);
    uint32_t total = 0;
#pragma unroll
    for (int i = 0; i < PAT_CLASSES; ++i) {
        c[i] = ((i < FIRST_DIFF) == same) ? c[i] : 0u;
        c[i] = pattern_row_sum(c[i]);
        total += c[i];
    }
    if (live && l == 0) {
        uint4 *out = reinterpret_cast<uint4 *>(classes + (size_t)q * PAT_ROW);
        out[0] = make_uint4(c[0], c[1], c[2], c[3]);
        out[1] = make_uint4(c[4], c[5], c[6], c[7]);
        out[2] = make_uint4(c[8], c[9], c[10], c[11]);
        out[3] = make_uint4(c[12], c[13], c[14], total);
    }
}

// One replicate of one test: a, b = the ABBA and BABA counts.  acc = {n, sum of d, sum of d^2, d of this replicate};
// a + b = 0 leaves acc as it is.  Every operation is rounded once, so the host, the device and Python floats give the
// same bits: the product and the sum stay apart.  Device code contracts a * b + c into one fused multiply-add by
// default.  __dmul_rn / __dadd_rn do not prevent that: they are inline functions of plain * and +, compiled under the
// default, and the pair still came out as one v_fmac_f64.  So the operators are written here, with contraction switched
// off for this function (the kernel then holds v_mul_f64 and v_add_f64).
__host__ __device__ __forceinline__ void dstat_add(uint32_t a, uint32_t b, double *acc)
{
#pragma clang fp contract(off)
    const uint64_t den = (uint64_t)a + (uint64_t)b;
    if (den == 0) return;
    const int64_t num = (int64_t)a - (int64_t)b;
    const double d = (double)num / (double)den;
    const double p = d * d;
    acc[0] = acc[0] + 1.0;
    acc[1] = acc[1] + d;
    acc[2] = acc[2] + p;
    acc[3] = d;
}

// test t: a = classes[set_of[t]][ia[t]], b = classes[set_of[t]][ib[t]].  Indices out of range: the thread returns
// without touching memory.
__global__ __launch_bounds__(DSTAT_THREADS) void tq_dstat_kernel(const uint32_t *__restrict__ classes, int64_t n_sets,
                                                                 const uint32_t *__restrict__ set_of,
                                                                 const uint8_t *__restrict__ ia, const uint8_t *__restrict__ ib,
                                                                 int64_t N, double *__restrict__ acc)
{
    const int64_t t = (int64_t)blockIdx.x * DSTAT_THREADS + threadIdx.x;
    if (t >= N) return;
    const uint32_t s = set_of[t];
    const uint32_t ca = ia[t], cb = ib[t];
    if ((int64_t)s >= n_sets || ca >= (uint32_t)PAT_CLASSES || cb >= (uint32_t)PAT_CLASSES) return;
    const uint32_t *row = classes + (size_t)s * PAT_ROW;
    dstat_add(row[ca], row[cb], acc + 4 * t);
}

// the host execution; the caller has checked the indices
inline void dstat_add_host(const uint32_t *classes, const uint32_t *set_of, const uint8_t *ia, const uint8_t *ib, int64_t N,
                           double *acc)
{
    for (int64_t t = 0; t < N; ++t) {
        const uint32_t *row = classes + (size_t)set_of[t] * PAT_ROW;
        dstat_add(row[ia[t]], row[ib[t]], acc + 4 * t);
    }
}

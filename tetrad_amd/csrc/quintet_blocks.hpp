// quintet_blocks.hpp -- five-taxon site-pattern class counts per (set, block of sites) from the bit planes, and the
// delete-one-block jackknife on sums of slots that DFOIL and partitioned D read them with.  Part of
// the single translation unit tetrad_hip.hip (included inside its anonymous namespace, after pattern_blocks.hpp).
//
// Rule (full mode only; `quintet_class` is its one statement): a site is counted for a set (t0 < t1 < t2 < t3 < t4) when
// none of the five bases x0..x4 is missing and they take exactly two distinct values.  Its class is
// k = sum over i = 1..4 of [x_i != x_0] 2^(i - 1), in 1..15: unpolarised, so every role assignment is a relabelling on
// the host.  Invariant sites and sites with three or four bases count nowhere; option count_invariant is not read.  A
// block row is u32[16]: slot k = the count of class k (k = 1..15), slot 0 = their sum.  Blocks are the `starts` of
// pattern_blocks.hpp.
//
// tq_quintet_blocks_kernel: the shape of tq_block_rows_kernel (block_rows.hpp), written out on its own: as a rule of that
// template the kernel measured 1 % slower at B = 50 (profiles/quintets/README.md).  A work item is a (set, block) pair,
// item = set * B + block; 16 lanes per item, four items per wavefront.  Lane l takes the words w0 + l, w0 + l + 16, ...
// of the block's word range: per word five 12-byte plane records, valid = ~(OR of the missing words) & range mask, the four
// "differs from x0" words and the six pair-difference words among positions 1..4, the 15 class masks (quintet_masks),
// 15 popcount-adds.  The 16 lanes are summed with the DPP steps of pattern_row_sum and the group's lane 0 writes the
// 64-byte row.  No LDS, no atomics, no scratch; every address is 64-bit.  A taxon >= T gives a row of zeros; items past
// Q * B store nothing.
//
// tq_jackknife_kernel<MaskPairTests>: dstat_jackknife_row with a_j / b_j = the sums of the row's slots named by two
// u16 masks (JackknifeMaskPair), one thread per test.
#pragma once

constexpr int QNT_TAXA = 5;

// class 1..15 of five bases 0..3, or -1 for a site that is not counted (a base outside 0..3 is missing)
constexpr __host__ __device__ int quintet_class(int x0, int x1, int x2, int x3, int x4)
{
    const int x[QNT_TAXA] = {x0, x1, x2, x3, x4};
    int k = 0, other = -1;
    for (int i = 0; i < QNT_TAXA; ++i)
        if (x[i] < 0 || x[i] > 3) return -1;
    for (int i = 1; i < QNT_TAXA; ++i) {
        if (x[i] == x0) continue;
        if (other >= 0 && x[i] != other) return -1;     // a third base
        other = x[i];
        k |= 1 << (i - 1);
    }
    return k == 0 ? -1 : k;                             // invariant
}

// The class masks of 32 sites: m[k] for k = 1..15, m[0] = the counted sites (their union).  n_i: position i differs from
// position 0; d_ij: positions i and j (both in 1..4) differ; `on` is AND-ed into every mask.  A site is bad when two
// positions that both differ from x0 differ from each other (a third base).  One definition for the kernel and for the
// compile-time check below.
struct QuintetMasks {
    uint32_t m[PAT_ROW];
};

constexpr __host__ __device__ QuintetMasks quintet_masks(uint32_t n1, uint32_t n2, uint32_t n3, uint32_t n4, uint32_t d12,
                                                         uint32_t d13, uint32_t d14, uint32_t d23, uint32_t d24, uint32_t d34,
                                                         uint32_t on)
{
    QuintetMasks r{};
    const uint32_t bad = (n1 & n2 & d12) | (n1 & n3 & d13) | (n1 & n4 & d14) | (n2 & n3 & d23) | (n2 & n4 & d24) | (n3 & n4 & d34);
    const uint32_t counted = on & ~bad & (n1 | n2 | n3 | n4);
    r.m[0] = counted;
    const uint32_t a[2] = {counted & ~n1, counted & n1};
    for (int i = 0; i < 2; ++i) {
        const uint32_t b[2] = {a[i] & ~n2, a[i] & n2};
        for (int j = 0; j < 2; ++j) {
            const uint32_t c[2] = {b[j] & ~n3, b[j] & n3};
            for (int k = 0; k < 2; ++k) {
                const int cls = i + 2 * j + 4 * k;
                if (cls != 0) r.m[cls] = c[k] & ~n4;    // (class 0 is empty: a counted site differs somewhere)
                r.m[cls + 8] = c[k] & n4;
            }
        }
    }
    return r;
}

// every one of the 1024 patterns sets exactly the mask of its class (and the counted mask), or none
constexpr bool quintet_masks_ok()
{
    for (int p = 0; p < 1024; ++p) {
        const int x0 = p >> 8, x1 = (p >> 6) & 3, x2 = (p >> 4) & 3, x3 = (p >> 2) & 3, x4 = p & 3;
        const QuintetMasks r = quintet_masks(x1 != x0, x2 != x0, x3 != x0, x4 != x0, x1 != x2, x1 != x3, x1 != x4, x2 != x3,
                                             x2 != x4, x3 != x4, 1u);
        const int want = quintet_class(x0, x1, x2, x3, x4);
        if (want == 0 || want > 15) return false;
        if (r.m[0] != (want > 0 ? 1u : 0u)) return false;
        for (int c = 1; c < PAT_ROW; ++c)
            if (r.m[c] != (c == want ? 1u : 0u)) return false;
    }
    return true;
}
static_assert(quintet_masks_ok(), "the class masks must follow quintet_class");

__device__ __forceinline__ uint32_t qnt_diff(const PlaneRec &x, const PlaneRec &y)
{
    return (x.b0 ^ y.b0) | (x.b1 ^ y.b1);
}

// planes3 u32[T][W][3]; sets5 u32[Q][5]; starts i64[B + 1] with 0 <= starts[0] < ... < starts[B] <= 32 W (checked on the
// host), Q * B < 2^31; classes u32[Q][B][16]
__global__ __launch_bounds__(PBLK_THREADS) void tq_quintet_blocks_kernel(const uint32_t *__restrict__ planes3, int64_t W,
                                                                         uint32_t T, const uint32_t *__restrict__ sets5,
                                                                         int64_t Q, const int64_t *__restrict__ starts,
                                                                         int64_t B, uint32_t *__restrict__ classes)
{
    const int l = threadIdx.x & 15;
    const int64_t item = (int64_t)blockIdx.x * PBLK_ITEMS + (threadIdx.x >> 4);
    const bool live = item < Q * B;             // the same for the 16 lanes of a DPP row
    // one launch holds fewer than 2^31 items (the host cuts longer calls): a 32-bit division
    const uint32_t q32 = live ? (uint32_t)item / (uint32_t)B : 0u;
    const int64_t q = q32, j = live ? item - q * B : 0;
    // a 20-byte row has no 16-byte alignment: five dwords
    const uint32_t *set = sets5 + q * QNT_TAXA;
    const uint32_t t0 = set[0], t1 = set[1], t2 = set[2], t3 = set[3], t4 = set[4];
    const bool inside = live && t0 < T && t1 < T && t2 < T && t3 < T && t4 < T;
    uint32_t c[PAT_ROW];                        // c[0] stays 0 until the total is summed into it
#pragma unroll
    for (int i = 0; i < PAT_ROW; ++i) c[i] = 0;
    if (inside) {
        const int64_t s0 = starts[j], s1 = starts[j + 1];       // s0 < s1
        const int64_t w0 = s0 >> 5, w1 = (s1 - 1) >> 5;
        const uint32_t first = 0xFFFFFFFFu << (uint32_t)(s0 & 31);
        const uint32_t last = 0xFFFFFFFFu >> (31u - (uint32_t)((s1 - 1) & 31));
        const uint32_t *r0 = planes3 + (int64_t)t0 * W * 3, *r1 = planes3 + (int64_t)t1 * W * 3;
        const uint32_t *r2 = planes3 + (int64_t)t2 * W * 3, *r3 = planes3 + (int64_t)t3 * W * 3;
        const uint32_t *r4 = planes3 + (int64_t)t4 * W * 3;
        for (int64_t w = w0 + l; w <= w1; w += 16) {
            const PlaneRec x0 = pblk_load(r0, w), x1 = pblk_load(r1, w), x2 = pblk_load(r2, w), x3 = pblk_load(r3, w);
            const PlaneRec x4 = pblk_load(r4, w);
            uint32_t valid = ~(x0.miss | x1.miss | x2.miss | x3.miss | x4.miss);
            valid &= w == w0 ? first : 0xFFFFFFFFu;
            valid &= w == w1 ? last : 0xFFFFFFFFu;
            const QuintetMasks k = quintet_masks(qnt_diff(x1, x0), qnt_diff(x2, x0), qnt_diff(x3, x0), qnt_diff(x4, x0),
                                                 qnt_diff(x1, x2), qnt_diff(x1, x3), qnt_diff(x1, x4), qnt_diff(x2, x3),
                                                 qnt_diff(x2, x4), qnt_diff(x3, x4), valid);
#pragma unroll
            for (int i = 1; i < PAT_ROW; ++i) c[i] += (uint32_t)__popc(k.m[i]);
        }
    }
    // every lane of the wavefront is here: the DPP steps read lanes of the own row only, and a row is one item
#pragma unroll
    for (int i = 1; i < PAT_ROW; ++i) {
        c[i] = pattern_row_sum(c[i]);
        c[0] += c[i];
    }
    if (live && l == 0) {
        uint4 *out = reinterpret_cast<uint4 *>(classes + item * PAT_ROW);
        // (an empty statement that pins each group of four: without it the vectorizer regroups the 16 values by the
        // registers the loop left them in and the row goes out as 12 + 16 + 16 + 16 + 4 bytes, three stores unaligned)
#pragma unroll
        for (int i = 0; i < PAT_ROW; i += 4) asm volatile("" : "+v"(c[i]), "+v"(c[i + 1]), "+v"(c[i + 2]), "+v"(c[i + 3]));
        out[0] = make_uint4(c[0], c[1], c[2], c[3]);
        out[1] = make_uint4(c[4], c[5], c[6], c[7]);
        out[2] = make_uint4(c[8], c[9], c[10], c[11]);
        out[3] = make_uint4(c[12], c[13], c[14], c[15]);
    }
}

// a_j / b_j = the sums of the row's slots whose bit is set in lmask / rmask (slots 1..15: bit 0 is the total's)
struct JackknifeMaskPair {
    uint32_t lmask, rmask;
    __host__ __device__ __forceinline__ void operator()(const uint32_t *row, uint64_t &a, uint64_t &b) const
    {
        uint64_t sa = 0, sb = 0;
#pragma unroll
        for (int k = 1; k < PAT_ROW; ++k) {
            const uint64_t v = row[k];
            sa += (lmask >> k) & 1u ? v : 0u;
            sb += (rmask >> k) & 1u ? v : 0u;
        }
        a = sa;
        b = sb;
    }
};

// a test is valid when bit 0 is clear in both masks, both are non-empty and they are disjoint
constexpr __host__ __device__ bool jackknife_masks_valid(uint32_t lmask, uint32_t rmask)
{
    return ((lmask | rmask) & 1u) == 0 && lmask != 0 && rmask != 0 && (lmask & rmask) == 0;
}

// the mask form of the jackknife tests (see ClassPairTests, pattern_blocks.hpp): two u16 slot masks per test
struct MaskPairTests {
    const uint16_t *a, *b;
    static constexpr const char *refusal =
        "%s: test %lld has masks 0x%04x / 0x%04x: bit 0 must be clear, both non-empty, and disjoint";
    __host__ __device__ __forceinline__ JackknifeMaskPair operator[](int64_t t) const { return JackknifeMaskPair{a[t], b[t]}; }
    static __host__ __device__ __forceinline__ bool valid(const JackknifeMaskPair &p) { return jackknife_masks_valid(p.lmask, p.rmask); }
};

// block_rows.hpp -- the per-block class-row kernel and the counting rules it runs (DESIGN.md sections 20, 21 and 23).
// Part of the single translation unit tetrad_hip.hip (included inside its anonymous namespace, after the headers that hold
// the rules' arithmetic: pattern_blocks.hpp, species_blocks.hpp, species_quintet_blocks.hpp).  The five-taxon rows of
// quintet_blocks.hpp keep a kernel of their own in this shape: as a rule on PlaneRule it measured slower.
//
// The shape of the kernel.  A work item is a (set, block) pair, item = set * B + block.  16 lanes take one item, four
// items per wavefront (the group shape of tq_pattern_class_kernel, whose DPP row sum is re-used).  Lane l takes every
// 16th word (plane rules) or site (table rules) of the block from its l-th on and adds into Rule::SUMS u32 sums; the 16
// lanes are summed with the DPP steps of pattern_row_sum and the group's lane 0 turns the sums into the 64-byte row and
// writes it.  No LDS, no atomics, no scratch; every address is 64-bit.  A set the rule does not take (an id out of
// range, a species row beyond its range rule) gives a row of zeros; items past Q * B store nothing.
//
// A rule is a struct passed to the kernel by value.  It holds the arrays it reads and says only what differs between the
// kinds: WIDTH (ids per set), SUMS, inside(set), walk(set, s0, s1, lane, acc) and finish(acc, row).  The two walks are
// written once, as the bases PlaneRule (words of the bit planes, with the range masks of the block's first and last
// word) and TableRule (sites of the species table); a rule on top of one adds its step per word or per site.
#pragma once

template <int N>
struct BlockSet {
    uint32_t id[N];
};

template <int N>
__device__ __forceinline__ BlockSet<N> block_set_load(const uint32_t *__restrict__ sets, int64_t q)
{
    static_assert(N == 4 || N == QNT_TAXA, "sets of four or five ids");
    if constexpr (N == 4) {
        const uint4 v = reinterpret_cast<const uint4 *>(sets)[q];
        return BlockSet<4>{{v.x, v.y, v.z, v.w}};
    } else {
        // a 20-byte row has no 16-byte alignment: five dwords (row 0 is read by the lanes of a dead item: Q >= 1)
        const uint32_t *set = sets + q * QNT_TAXA;
        return BlockSet<5>{{set[0], set[1], set[2], set[3], set[4]}};
    }
}

template <int N>
__device__ __forceinline__ bool block_set_below(const BlockSet<N> &set, uint32_t bound)
{
    bool ok = true;
#pragma unroll
    for (int i = 0; i < N; ++i) ok = ok & (set.id[i] < bound);
    return ok;
}

// The plane walk: planes3 u32[T][W][3]; a set is N taxa below T.  Per word N 12-byte plane records {missing, bit 0, bit 1}
// (prepare.hpp) and valid = ~(OR of the missing words) & range mask, then Rule::word(records, valid, acc).  The range
// mask differs from all-ones only in the first and the last word of the block (both cuts in one word when the block lies
// inside it); pad sites are missing in every taxon.  0 <= s0 < s1 <= 32 W (checked on the host).
template <class Rule, int N>
struct PlaneRule {
    static constexpr int WIDTH = N, SUMS = PAT_CLASSES;
    const uint32_t *planes3;
    int64_t W;
    uint32_t T;

    __device__ __forceinline__ bool inside(const BlockSet<N> &set) const { return block_set_below(set, T); }

    __device__ __forceinline__ void walk(const BlockSet<N> &set, int64_t s0, int64_t s1, int lane, uint32_t (&acc)[SUMS]) const
    {
        const int64_t w0 = s0 >> 5, w1 = (s1 - 1) >> 5;
        const uint32_t first = 0xFFFFFFFFu << (uint32_t)(s0 & 31);
        const uint32_t last = 0xFFFFFFFFu >> (31u - (uint32_t)((s1 - 1) & 31));
        const uint32_t *row[N];
#pragma unroll
        for (int i = 0; i < N; ++i) row[i] = planes3 + (int64_t)set.id[i] * W * 3;
        for (int64_t w = w0 + lane; w <= w1; w += 16) {
            PlaneRec x[N];
            uint32_t miss = 0;
#pragma unroll
            for (int i = 0; i < N; ++i) {
                x[i] = pblk_load(row[i], w);
                miss |= x[i].miss;
            }
            uint32_t valid = ~miss;
            valid &= w == w0 ? first : 0xFFFFFFFFu;
            valid &= w == w1 ? last : 0xFFFFFFFFu;
            static_cast<const Rule *>(this)->word(x, valid, acc);
        }
    }
};

// The table walk: tab u32[K][Sp] (VALU form of the species table, current for the resident replicate), offsets i32[K + 1]
// in lineages; a set is N species below K.  Per site the N packed entries (one dword each), then Rule::site(entries, acc).
// 0 <= s0 < s1 <= S <= Sp (checked on the host).
template <class Rule, int N, int NSUMS>
struct TableRule {
    static constexpr int WIDTH = N, SUMS = NSUMS;
    const uint32_t *tab;
    int64_t Sp, S;
    uint32_t K;
    const int32_t *offsets;

    __device__ __forceinline__ void walk(const BlockSet<N> &set, int64_t s0, int64_t s1, int lane, uint32_t (&acc)[SUMS]) const
    {
        const uint32_t *row[N];
#pragma unroll
        for (int i = 0; i < N; ++i) row[i] = tab + (int64_t)set.id[i] * Sp;
        for (int64_t s = s0 + lane; s < s1; s += 16) {
            uint32_t n[N];
#pragma unroll
            for (int i = 0; i < N; ++i) n[i] = row[i][s];
            Rule::site(n, acc);
        }
    }
};

// pattern_blocks.hpp: six equality words, the 15 class masks, 15 popcount-adds; inv = 0xFFFFFFFF when invariant sites
// count, else 0, AND-ed into class 0 only.  Row = the 15 counts and their sum.
struct QuartetRule : PlaneRule<QuartetRule, 4> {
    uint32_t inv;

    __device__ __forceinline__ void word(const PlaneRec (&x)[4], uint32_t valid, uint32_t (&c)[SUMS]) const
    {
        const PatternMasks k = pattern_masks(pblk_eq(x[0], x[1]), pblk_eq(x[0], x[2]), pblk_eq(x[0], x[3]), pblk_eq(x[1], x[2]),
                                             pblk_eq(x[1], x[3]), pblk_eq(x[2], x[3]), valid);
        c[0] += (uint32_t)__popc(k.m[0] & inv);
#pragma unroll
        for (int i = 1; i < PAT_CLASSES; ++i) c[i] += (uint32_t)__popc(k.m[i]);
    }

    static __device__ __forceinline__ void finish(const uint32_t (&c)[SUMS], uint32_t (&row)[PAT_ROW])
    {
        row[PAT_CLASSES] = 0;
#pragma unroll
        for (int i = 0; i < PAT_CLASSES; ++i) {
            row[i] = c[i];
            row[PAT_CLASSES] += c[i];
        }
    }
};

// species_blocks.hpp: the 15 partition sums per site, inverted once per row.  A row that repeats species so that S x its
// own lineage product breaks the range rule (species_row_in_range, as the pooling kernels) is not taken.
struct SpeciesRule : TableRule<SpeciesRule, 4, PAT_CLASSES> {
    __device__ __forceinline__ bool inside(const BlockSet<4> &set) const
    {
        return block_set_below(set, K) && species_row_in_range(offsets, make_uint4(set.id[0], set.id[1], set.id[2], set.id[3]), S);
    }

    static __device__ __forceinline__ void site(const uint32_t (&n)[4], uint32_t (&f)[SUMS]) { pooled_site_f(n[0], n[1], n[2], n[3], f); }

    static __device__ __forceinline__ void finish(const uint32_t (&f)[SUMS], uint32_t (&row)[PAT_ROW]) { pooled_invert(f, row); }
};

// species_quintet_blocks.hpp: the quintuple dot and the 15 products per site, subtracted once per row; the range rule
// of five ids.
struct SpeciesQuintetRule : TableRule<SpeciesQuintetRule, QNT_TAXA, PAT_ROW> {
    __device__ __forceinline__ bool inside(const BlockSet<QNT_TAXA> &set) const
    {
        return block_set_below(set, K) && species_row5_in_range(offsets, set.id[0], set.id[1], set.id[2], set.id[3], set.id[4], S);
    }

    static __device__ __forceinline__ void site(const uint32_t (&n)[QNT_TAXA], uint32_t (&f)[SUMS])
    {
        pooled5_site_f(n[0], n[1], n[2], n[3], n[4], f);
    }

    static __device__ __forceinline__ void finish(const uint32_t (&f)[SUMS], uint32_t (&row)[PAT_ROW]) { pooled5_finish(f, row); }
};

// One class row out as four aligned 16-byte stores (dst is 16-byte aligned).  The empty statement pins each group of
// four: without it the vectorizer may regroup the 16 values by the registers the sums left them in, and the row then
// goes out as 12 + 16 + 16 + 16 + 4 bytes, three stores unaligned.
__device__ __forceinline__ void block_row_store(uint32_t *dst, uint32_t (&c)[PAT_ROW])
{
    uint4 *out = reinterpret_cast<uint4 *>(dst);
#pragma unroll
    for (int i = 0; i < PAT_ROW; i += 4) asm volatile("" : "+v"(c[i]), "+v"(c[i + 1]), "+v"(c[i + 2]), "+v"(c[i + 3]));
#pragma unroll
    for (int i = 0; i < PAT_ROW; i += 4) out[i / 4] = make_uint4(c[i], c[i + 1], c[i + 2], c[i + 3]);
}

// sets u32[Q][Rule::WIDTH]; starts i64[B + 1], ascending (its range is the walk's); Q * B < 2^31; classes u32[Q][B][16]
template <class Rule>
__global__ __launch_bounds__(PBLK_THREADS) void tq_block_rows_kernel(const Rule rule, const uint32_t *__restrict__ sets, int64_t Q,
                                                                     const int64_t *__restrict__ starts, int64_t B,
                                                                     uint32_t *__restrict__ classes)
{
    const int lane = threadIdx.x & 15;
    const int64_t item = (int64_t)blockIdx.x * PBLK_ITEMS + (threadIdx.x >> 4);
    const bool live = item < Q * B;             // the same for the 16 lanes of a DPP row
    // one launch holds fewer than 2^31 items (the host cuts longer calls): a 32-bit division
    const uint32_t q32 = live ? (uint32_t)item / (uint32_t)B : 0u;
    const int64_t q = q32, j = live ? item - q * B : 0;
    const BlockSet<Rule::WIDTH> set = block_set_load<Rule::WIDTH>(sets, q);
    const bool inside = live && rule.inside(set);
    uint32_t acc[Rule::SUMS];
#pragma unroll
    for (int i = 0; i < Rule::SUMS; ++i) acc[i] = 0;
    if (inside) rule.walk(set, starts[j], starts[j + 1], lane, acc);
    // every lane of the wavefront is here: the DPP steps read lanes of the own row only, and a row is one item
#pragma unroll
    for (int i = 0; i < Rule::SUMS; ++i) acc[i] = pattern_row_sum(acc[i]);
    if (live && lane == 0) {
        uint32_t row[PAT_ROW];
        Rule::finish(acc, row);
        block_row_store(classes + item * PAT_ROW, row);
    }
}

// taxdist.hpp -- all-pairs taxon counts per block of sites: shared sites, differences, transitions and transversions
// (DESIGN.md section 29).  No reference counterpart.
// Part of the single translation unit tetrad_hip.hip (included inside its anonymous namespace, behind bit_tile.hpp and
// pattern_blocks.hpp, whose block limit it shares).
//
// One rule, executed on the host and on the device, integers only.  For two taxa i, j and the sites of a block:
//   both  the sites present (not missing) in i and in j
//   diff  of those, the sites whose bases differ
//   ts    of the differing ones, the transitions: with A, C, G, T = 0..3 bit 1 differs and bit 0 does not (A<->G, C<->T)
//   tv    diff - ts, formed once at the store
// On plane words (`td_word`), with p = present, x0 = b0_i ^ b0_j, x1 = b1_i ^ b1_j: both = popc(p_i & p_j), diff =
// popc(p_i & p_j & (x0 | x1)), ts = popc(p_i & p_j & x1 & ~x0).  A pair row is u32[4] = (both, diff, ts, tv); the
// diagonal row is (sites present in i, 0, 0, 0); the matrix is symmetric.  Full mode only, every site counts (no
// count_invariant, no one-SNP-per-locus form).  Blocks are those of pattern_blocks.hpp: starts i64[B + 1], strictly
// increasing inside [0, S], B <= PBLK_MAX_BLOCKS; a site outside every block counts nowhere.  A count is at most the sites
// of a block, so u32 holds it, and integer adds are exact in any order: no result depends on the slicing, the launch
// shape or the stream.
//
// Device path, on planes3 u32[T][W][3] = {missing, bit 0, bit 1} of the natural layout:
//   tq_taxon_counts_kernel   the tile product of bit_tile.hpp with three planes, 64 taxa x 64 taxa, on u64 words made of
//                         plane records 2k and 2k + 1 (the second half absent where 2k + 1 >= W).  Plane 0 of the tile
//                         is the PRESENT word, ~missing AND the block's range mask, so rows past T and words past the
//                         slice, staged as zeros, count nothing.  Grid (upper-triangle tile pairs as `bit_tile_pair`
//                         numbers them, work items); a work item (`TdItem`, built on the host) is a slice of at most
//                         `slice_words` u64 words of ONE block with the block's first and last word and their range
//                         masks (both cuts may fall into one word).  48 u32 accumulators per thread; a thread adds its
//                         non-zero results to out[block][r][c][0..2] with the u32 integer atomicAdd (the region was
//                         zeroed on the stream first).
//   tq_taxon_finish_kernel   threads over the rows (block, r, c) of the tiles on and above the diagonal: forms tv, stores
//                         the row as one 16-byte word and, for a tile above the diagonal, its mirror [c][r] as well.  A
//                         thread reads its own row only and writes rows no other thread touches.
// Every address is 64-bit.  No float, no inline assembly, no loop that waits on another lane or workgroup; every loop is
// bounded by T, the words of a slice or a constant.
#pragma once

constexpr int TD_THREADS = BT_THREADS;
constexpr int TD_BT = BT_ROWS;              // taxa per tile side
constexpr int TD_SLICE_WORDS = 32;          // u64 words of a work item (profiles/taxdist/: the sweep 8 .. 128); a multiple of BT_KW
constexpr int TD_MAX_SLICE_WORDS = 1 << 16; // bound of option taxdist_slice_words; a u32 accumulator holds at most 64 x the words of a slice
constexpr int64_t TD_LAUNCH_ITEMS = 65535;  // work items of one launch (grid.y)
static_assert(TD_SLICE_WORDS % BT_KW == 0, "a slice is whole staged chunks");

struct TdCounts {
    uint32_t both, diff, ts;
};

// the counts of one u64 word of two taxa: present, bit 0 and bit 1 of either
constexpr __host__ __device__ TdCounts td_word(uint64_t pi, uint64_t b0i, uint64_t b1i, uint64_t pj, uint64_t b0j, uint64_t b1j)
{
    const uint64_t p = pi & pj, x0 = b0i ^ b0j, x1 = b1i ^ b1j;
    return TdCounts{(uint32_t)__builtin_popcountll(p), (uint32_t)__builtin_popcountll(p & (x0 | x1)),
                    (uint32_t)__builtin_popcountll(p & x1 & ~x0)};
}

// every pair of cells (4 = missing, else the base) gives the counts the definition in words gives, at any bit
constexpr bool td_word_ok()
{
    for (int bit = 0; bit < 64; bit += 21)
        for (int x = 0; x < 5; ++x)
            for (int y = 0; y < 5; ++y) {
                const uint64_t one = uint64_t(1) << bit;
                // a missing cell carries base bits as well here: they must not count
                const TdCounts c = td_word(x < 4 ? one : 0, (x & 1) ? one : 0, (x & 2 || x == 4) ? one : 0, y < 4 ? one : 0,
                                           (y & 1 || y == 4) ? one : 0, (y & 2) ? one : 0);
                const bool both = x < 4 && y < 4, diff = both && x != y;
                const bool ts = diff && ((x == 0 && y == 2) || (x == 2 && y == 0) || (x == 1 && y == 3) || (x == 3 && y == 1));
                if (c.both != (both ? 1u : 0u) || c.diff != (diff ? 1u : 0u) || c.ts != (ts ? 1u : 0u)) return false;
            }
    return true;
}
static_assert(td_word_ok(), "the word rule must follow the definition of both, diff and ts");

// the range masks of a block [s0, s1) in its first word s0 / 64 and its last word (s1 - 1) / 64
constexpr __host__ __device__ uint64_t td_first_mask(int64_t s0) { return ~uint64_t(0) << (uint32_t)(s0 & 63); }
constexpr __host__ __device__ uint64_t td_last_mask(int64_t s1) { return ~uint64_t(0) >> (63u - (uint32_t)((s1 - 1) & 63)); }

// A work item: the words [w_begin, w_end) of block `block`, whose first and last word are w_first and w_last.
struct TdItem {
    int32_t block, w_begin, w_end, w_first, w_last, pad;
    uint64_t first, last;
};

// The items of blocks [b0, b1): every block cut into slices of `slice_words`, in block order.  A slice never straddles
// two blocks.
inline void td_make_items(const int64_t *starts, int64_t b0, int64_t b1, int64_t slice_words, std::vector<TdItem> &items)
{
    for (int64_t b = b0; b < b1; ++b) {
        const int64_t wf = starts[b] >> 6, wl = (starts[b + 1] - 1) >> 6;
        const uint64_t first = td_first_mask(starts[b]), last = td_last_mask(starts[b + 1]);
        for (int64_t w = wf; w <= wl; w += slice_words)
            items.push_back(TdItem{(int32_t)b, (int32_t)w, (int32_t)std::min(wl + 1, w + slice_words), (int32_t)wf, (int32_t)wl, 0,
                                   first, last});
    }
}

// Host execution: the same rule on u64 words packed from tmparr u8[T][S] (a cell above 3 is missing); out u32[B][T][T][4]
inline void td_host_counts(const uint8_t *tmparr, int64_t T, int64_t S, const int64_t *starts, int64_t B, uint32_t *out)
{
    const int64_t W = (S + 63) / 64;
    std::vector<uint64_t> P((size_t)(T * 3 * W), 0);            // [T][3][W] = {present, bit 0, bit 1}
    for (int64_t t = 0; t < T; ++t) {
        uint64_t *row = P.data() + t * 3 * W;
        for (int64_t s = 0; s < S; ++s) {
            const uint8_t v = tmparr[t * S + s];
            if (v > 3) continue;
            const uint64_t bit = uint64_t(1) << (s & 63);
            row[s >> 6] |= bit;
            if (v & 1) row[W + (s >> 6)] |= bit;
            if (v & 2) row[2 * W + (s >> 6)] |= bit;
        }
    }
    for (int64_t b = 0; b < B; ++b) {
        const int64_t wf = starts[b] >> 6, wl = (starts[b + 1] - 1) >> 6;
        const uint64_t first = td_first_mask(starts[b]), last = td_last_mask(starts[b + 1]);
        for (int64_t i = 0; i < T; ++i) {
            const uint64_t *x = P.data() + i * 3 * W;
            for (int64_t j = i; j < T; ++j) {
                const uint64_t *y = P.data() + j * 3 * W;
                uint32_t both = 0, diff = 0, ts = 0;
                for (int64_t w = wf; w <= wl; ++w) {
                    const uint64_t range = (w == wf ? first : ~uint64_t(0)) & (w == wl ? last : ~uint64_t(0));
                    const TdCounts c = td_word(x[w] & range, x[W + w], x[2 * W + w], y[w], y[W + w], y[2 * W + w]);
                    both += c.both;
                    diff += c.diff;
                    ts += c.ts;
                }
                uint32_t *up = out + ((b * T + i) * T + j) * 4, *lo = out + ((b * T + j) * T + i) * 4;
                up[0] = lo[0] = both;
                up[1] = lo[1] = diff;
                up[2] = lo[2] = ts;
                up[3] = lo[3] = diff - ts;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Device path
// ---------------------------------------------------------------------------------------------
struct TdArgs {
    const uint32_t *planes3;    // [T][W][3]
    const TdItem *items;        // the items of this launch
    uint32_t *out;              // rows of block `block0`: u32 [blocks][T][T][4], zeroed
    int64_t W;                  // plane records per taxon row
    int32_t T, nt;              // taxa, tiles per side
    int32_t block0;             // the block out[0] belongs to
};

// u64 word w of plane p of taxon row `row`: records 2 w and 2 w + 1; a record past W is all missing.  Plane 0 comes out
// as the present word inside the item's block.
__device__ __forceinline__ uint64_t td_load(const TdArgs &a, const TdItem &it, int row, int p, int w)
{
    const int64_t k = 2 * (int64_t)w;
    const uint32_t *rec = a.planes3 + ((int64_t)row * a.W + k) * 3;
    const bool second = k + 1 < a.W;
    const uint32_t lo = rec[p], hi = second ? rec[3 + p] : (p == 0 ? 0xFFFFFFFFu : 0u);
    uint64_t v = (uint64_t)lo | ((uint64_t)hi << 32);
    if (p == 0) {
        v = ~v;
        if (w == it.w_first) v &= it.first;
        if (w == it.w_last) v &= it.last;
    }
    return v;
}

// grid (upper-triangle tile pairs, work items of the launch)
__global__ __launch_bounds__(TD_THREADS) void tq_taxon_counts_kernel(TdArgs a)
{
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int T = a.T;
    int bi, bj;
    if (!bit_tile_pair((int)blockIdx.x, a.nt, bi, bj)) return;
    const TdItem it = a.items[blockIdx.y];
    if (it.w_begin >= it.w_end) return;         // never with the items the host builds
    const int r0 = bi * TD_BT, c0 = bj * TD_BT;
    uint32_t both[4][4], diff[4][4], ts[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) both[i][j] = diff[i][j] = ts[i][j] = 0;
    bit_tile_product<3, 2>(
        T - r0, T - c0, it.w_begin, it.w_end, [&](int row, int p, int w) { return td_load(a, it, r0 + row, p, w); },
        [&](int row, int p, int w) { return td_load(a, it, c0 + row, p, w); },
        [&](int i, int j, const uint64_t (&x)[3], const uint64_t (&y)[3]) {
            const TdCounts c = td_word(x[0], x[1], x[2], y[0], y[1], y[2]);
            both[i][j] += c.both;
            diff[i][j] += c.diff;
            ts[i][j] += c.ts;
        });
    uint32_t *blk = a.out + (int64_t)(it.block - a.block0) * T * T * 4;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int r = r0 + ty + 16 * i;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int c = c0 + tx + 16 * j;
            if (r >= T || c >= T) continue;
            uint32_t *o = blk + ((int64_t)r * T + c) * 4;
            if (both[i][j]) atomicAdd(o, both[i][j]);           // integer adds: exact in any order
            if (diff[i][j]) atomicAdd(o + 1, diff[i][j]);
            if (ts[i][j]) atomicAdd(o + 2, ts[i][j]);
        }
    }
}

// threads over the rows (block, r, c) of `blocks` blocks; out is 16-byte aligned
__global__ __launch_bounds__(TD_THREADS) void tq_taxon_finish_kernel(uint4 *out, int64_t blocks, int32_t T)
{
    const int64_t idx = (int64_t)blockIdx.x * TD_THREADS + threadIdx.x;
    const int64_t TT = (int64_t)T * T;
    if (idx >= blocks * TT) return;
    const int64_t b = idx / TT, rem = idx - b * TT;
    const int r = (int)(rem / T), c = (int)(rem - (int64_t)r * T);
    if (r / TD_BT > c / TD_BT) return;          // written as the mirror of [c][r]
    uint4 v = out[idx];
    v.w = v.y - v.z;
    out[idx] = v;
    if (r / TD_BT < c / TD_BT) out[b * TT + (int64_t)c * T + r] = v;
}

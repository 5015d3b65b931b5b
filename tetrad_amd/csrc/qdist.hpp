// qdist.hpp -- all-pairs quartet distances of a set of trees.  No reference counterpart.
// Part of the single translation unit tetrad_hip.hip (included inside its anonymous namespace, behind treedist.hpp and
// fit.hpp, whose tables it reuses).
//
// One rule, executed on the host and on the device, integers only:
//   table     D(x, y) = the depth of the lowest common ancestor of tips x and y in the prepared tree, u16 [T][T], as
//             `fit_host_table` / `tq_fit_table_kernel` (fit.hpp, unchanged) give it.
//   code      of four distinct taxa (a, b, c, d) in a tree (`qd_code`): with m0 = D(a,b) + D(c,d), m1 = D(a,c) + D(b,d),
//             m2 = D(a,d) + D(b,c) the code is 0, 1 or 2 when m0, m1 or m2 is strictly the largest and 3 (unresolved)
//             when the largest is not unique.  `fit_row`'s comparison, but it says which topology holds.
//   planes    for a chunk of quartets tree i owns three bit rows P0, P1, P2: bit q of Pk is set iff the code of quartet q
//             is k; an unresolved or padding quartet sets no bit.  R = P0 | P1 | P2.
//   word      `qd_word` (`qd_word_r` with R of both sides at hand): same = popc(x0 & y0) + popc(x1 & y1) + popc(x2 & y2),
//             both = popc(Rx & Ry).
//   results   same[i][j] and both[i][j], u64 sums of the word counts over all quartets scored so far.
// A permutation of the taxa inside a quartet renames the codes 0..2 in every tree alike, so neither sum moves; any
// chunking of quartets, any split of the words and any order of score calls add the same integers.
//
// Device layout (all of it allocated at create): tables u16 [max_trees][T][T], same / both u64 [max_trees^2] (row pitch =
// the trees held), one chunk of quartets as uint4 and the plane rows u64 [trees][3][words of the chunk].
//   tq_qd_encode_kernel<LDS_TABLE>  grid (quartet slices, trees).  A wave takes 64 consecutive quartets, one per lane; the
//                         tree's table is copied to LDS for T <= FIT_T_LDS (as tq_fit_kernel) and read through L2 above.
//                         Three wave ballots (code == k) are the three plane words; lanes 0..2 store one each with a
//                         plain store.  Lanes past the chunk's end vote in no ballot.  Every word of the chunk belongs
//                         to one wave: no atomics, nothing to clear.
//   tq_qd_gemm_kernel     the tile product of bit_tile.hpp, 64 trees x 64 trees, with three planes per side, `qd_word`
//                         as the word rule (R is made once per staged word in registers), two u32 accumulators per pair,
//                         and a grid of (upper-triangle tile pairs as `bit_tile_pair` numbers them, k slices): a workgroup
//                         walks only its slice of the chunk's words.  With one slice a thread adds to same / both with a
//                         plain read-modify-write (it alone owns the pair; launches follow each other on the stream);
//                         with more it uses the integer atomicAdd on u64 and skips zeros.
//   tq_qd_final_kernel    at a read: the tiles below the diagonal mirrored from the ones above.
// A u32 accumulator holds at most 64 x the words of one chunk, which create keeps below 2^24.
// No float, no inline assembly, no loop that waits on another lane or workgroup; every loop is bounded by T, N, the
// words of a chunk or a constant.
#pragma once

constexpr int QD_THREADS = BT_THREADS;
constexpr int QD_BT = BT_ROWS;              // trees per tile side
constexpr int64_t QD_MAX_TREES = 8192;
constexpr int64_t QD_MAX_CHUNK_WORDS = int64_t(1) << 24;
constexpr int QD_ENC_WORDS_PER_BLOCK = 256; // plane words (of 64 quartets) an encode workgroup is sized for (unmeasured)
constexpr int QD_GRID_PER_CU = 4;           // auto k split: workgroups per compute unit aimed at (unmeasured)
constexpr int64_t QD_HOST_CHUNK_WORDS = 1024;

struct QdCounts {
    uint32_t same, both;
};

// which of the three pairings of four distinct taxa the tree displays, 3 = none
template <class TAB>
__host__ __device__ __forceinline__ uint32_t qd_code(const TAB *D, uint32_t T, uint32_t a, uint32_t b, uint32_t c, uint32_t d)
{
    const uint32_t m0 = (uint32_t)D[a * T + b] + (uint32_t)D[c * T + d];
    const uint32_t m1 = (uint32_t)D[a * T + c] + (uint32_t)D[b * T + d];
    const uint32_t m2 = (uint32_t)D[a * T + d] + (uint32_t)D[b * T + c];
    if (m0 > m1 && m0 > m2) return 0;
    if (m1 > m0 && m1 > m2) return 1;
    if (m2 > m0 && m2 > m1) return 2;
    return 3;
}

// the quartets of one word two trees resolve alike, and the ones both resolve; xr = x0 | x1 | x2, yr likewise
__host__ __device__ __forceinline__ QdCounts qd_word_r(uint64_t x0, uint64_t x1, uint64_t x2, uint64_t xr, uint64_t y0, uint64_t y1,
                                                       uint64_t y2, uint64_t yr)
{
    QdCounts c;
    c.same = (uint32_t)(__builtin_popcountll(x0 & y0) + __builtin_popcountll(x1 & y1) + __builtin_popcountll(x2 & y2));
    c.both = (uint32_t)__builtin_popcountll(xr & yr);
    return c;
}

__host__ __device__ __forceinline__ QdCounts qd_word(uint64_t x0, uint64_t x1, uint64_t x2, uint64_t y0, uint64_t y1, uint64_t y2)
{
    return qd_word_r(x0, x1, x2, x0 | x1 | x2, y0, y1, y2, y0 | y1 | y2);
}

// Host execution: the planes of one tree over `nq` quartets (u32 [nq][4]); P points at 3 rows of `cw` words
inline void qd_host_encode(const uint16_t *D, uint32_t T, const uint32_t *q, int64_t nq, int64_t cw, uint64_t *P)
{
    for (int64_t w = 0; w < 3 * cw; ++w) P[w] = 0;
    for (int64_t i = 0; i < nq; ++i) {
        const uint32_t code = qd_code(D, T, q[4 * i], q[4 * i + 1], q[4 * i + 2], q[4 * i + 3]);
        if (code < 3) P[code * cw + (i >> 6)] |= uint64_t(1) << (i & 63);
    }
}

// Host execution: same / both (row pitch N) += the word counts of every pair i <= j and its mirror
inline void qd_host_product(const uint64_t *P, int64_t N, int64_t cw, uint64_t *same, uint64_t *both)
{
    for (int64_t i = 0; i < N; ++i) {
        const uint64_t *x = P + i * 3 * cw;
        for (int64_t j = i; j < N; ++j) {
            const uint64_t *y = P + j * 3 * cw;
            uint64_t s = 0, b = 0;
            for (int64_t w = 0; w < cw; ++w) {
                const QdCounts c = qd_word(x[w], x[cw + w], x[2 * cw + w], y[w], y[cw + w], y[2 * cw + w]);
                s += c.same;
                b += c.both;
            }
            same[i * N + j] += s;
            both[i * N + j] += b;
            if (j != i) {
                same[j * N + i] += s;
                both[j * N + i] += b;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Device path
// ---------------------------------------------------------------------------------------------
struct QdEncodeArgs {
    const uint4 *quartets;      // [nq] four distinct taxa < T each
    const uint16_t *tab;        // [trees][T][T]
    uint64_t *planes;           // [trees][3][cw]
    int64_t nq;                 // quartets of the chunk
    int32_t cw;                 // words of the chunk, (nq + 63) / 64
    uint32_t T;
};

// grid (quartet slices, trees).  LDS_TABLE: the tree's table is copied to LDS (T <= FIT_T_LDS), otherwise read through L2.
template <bool LDS_TABLE>
__global__ __launch_bounds__(QD_THREADS) void tq_qd_encode_kernel(QdEncodeArgs a)
{
    __shared__ uint16_t s_tab[LDS_TABLE ? FIT_T_LDS * FIT_T_LDS : 2];
    const uint32_t T = a.T;
    const uint16_t *D = a.tab + (size_t)blockIdx.y * T * T;
    constexpr int WAVES = QD_THREADS / 64;
    if ((int64_t)blockIdx.x * WAVES >= a.cw) return;                // the same for every thread: no barrier is left behind
    if (LDS_TABLE) {
        const uint32_t *src = (const uint32_t *)D;                  // T * T is even (T >= 4); a table starts 4-byte aligned
        uint32_t *dst = (uint32_t *)s_tab;
        for (uint32_t i = threadIdx.x; i < T * T / 2; i += QD_THREADS) dst[i] = src[i];
        __syncthreads();
    }
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint64_t *P = a.planes + (size_t)blockIdx.y * 3 * (size_t)a.cw;
    for (int64_t w = (int64_t)blockIdx.x * WAVES + wave; w < a.cw; w += (int64_t)gridDim.x * WAVES) {
        const int64_t q = w * 64 + lane;
        uint32_t code = 3;                                          // a lane past the chunk's end votes in no ballot
        if (q < a.nq) {
            const uint4 t = a.quartets[q];
            code = LDS_TABLE ? qd_code(s_tab, T, t.x, t.y, t.z, t.w) : qd_code(D, T, t.x, t.y, t.z, t.w);
        }
        const uint64_t p0 = __ballot(code == 0), p1 = __ballot(code == 1), p2 = __ballot(code == 2);
        if (lane < 3) P[(size_t)lane * a.cw + w] = lane == 0 ? p0 : lane == 1 ? p1 : p2;
    }
}

struct QdGemmArgs {
    const uint64_t *planes;     // [N][3][cw]
    unsigned long long *same, *both;    // [N][N]
    int32_t N, cw, nt;          // trees, words of the chunk, tiles per side
    int32_t slice_words;        // words a k slice walks, a multiple of BT_KW
    int32_t atomic;             // more than one k slice
};

// grid (upper-triangle tile pairs, k slices)
__global__ __launch_bounds__(QD_THREADS) void tq_qd_gemm_kernel(QdGemmArgs a)
{
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int N = a.N;
    int bi, bj;
    if (!bit_tile_pair((int)blockIdx.x, a.nt, bi, bj)) return;
    const int wbeg = (int)blockIdx.y * a.slice_words;
    const int wend = min(a.cw, wbeg + a.slice_words);
    if (wbeg >= wend) return;                   // never with the slices the host counts
    const int r0 = bi * QD_BT, c0 = bj * QD_BT;
    uint32_t same[4][4], both[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) same[i][j] = both[i][j] = 0;
    // rows past N and words past the slice are zero: they count nothing.  The k loop is unrolled twice: 159 VGPRs, 3
    // waves per SIMD; a full unroll held 255 and left 2 (profiles/qdist/)
    bit_tile_product<3, 2>(
        N - r0, N - c0, wbeg, wend,
        [&](int row, int p, int w) { return a.planes[((int64_t)(r0 + row) * 3 + p) * a.cw + w]; },
        [&](int row, int p, int w) { return a.planes[((int64_t)(c0 + row) * 3 + p) * a.cw + w]; },
        [&](int i, int j, const uint64_t (&x)[3], const uint64_t (&y)[3]) {
            const QdCounts c = qd_word(x[0], x[1], x[2], y[0], y[1], y[2]);
            same[i][j] += c.same;
            both[i][j] += c.both;
        });
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int r = r0 + ty + 16 * i;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int c = c0 + tx + 16 * j;
            if (r >= N || c >= N) continue;
            const int64_t o = (int64_t)r * N + c;
            if (a.atomic) {                     // integer adds: exact in any order
                if (same[i][j]) atomicAdd(&a.same[o], (unsigned long long)same[i][j]);
                if (both[i][j]) atomicAdd(&a.both[o], (unsigned long long)both[i][j]);
            } else {                            // this thread alone owns (r, c)
                a.same[o] += same[i][j];
                a.both[o] += both[i][j];
            }
        }
    }
}

// threads over (r, c): an entry of a tile below the diagonal tiles takes [c][r], which no thread of this kernel writes
__global__ __launch_bounds__(QD_THREADS) void tq_qd_final_kernel(unsigned long long *same, unsigned long long *both, int32_t N)
{
    const int64_t idx = (int64_t)blockIdx.x * QD_THREADS + threadIdx.x;
    if (idx >= (int64_t)N * N) return;
    const int r = (int)(idx / N), c = (int)(idx % N);
    if (r / QD_BT <= c / QD_BT) return;
    const int64_t up = (int64_t)c * N + r;
    same[idx] = same[up];
    both[idx] = both[up];
}

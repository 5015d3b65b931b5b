// bit_tile.hpp -- the tile product on bit rows that tq_tbe_kernel (tbe.hpp), tq_rf_gemm_kernel (treedist.hpp) and
// tq_qd_gemm_kernel (qdist.hpp) share.
// Part of the single translation unit tetrad_hip.hip (included inside its anonymous namespace, ahead of the three).
//
// A binary GEMM: C[r][c] (+)= the sum over the words w of word(A[r][w], B[c][w]), where `word` is a popcount rule on one
// u64 word of each side (or on PLANES words of each side that belong together).  A workgroup of 256 threads as 16 x 16
// owns a tile of 64 rows of A times 64 rows of B; thread (tx, ty) owns the 4 x 4 results of rows ty + 16 i of A and
// tx + 16 j of B.  The words are walked in chunks of BT_KW: both operand tiles of a chunk are staged in LDS row-major
// at a pitch of BT_PITCH = BT_KW + 1 words (thread t stages rows t / 8 and t / 8 + 32, word t % 8, of every plane),
// rows past the operand's end and words past w_end as zeros, which every word rule here counts as nothing.  Then each
// thread reads 4 + 4 rows per word and applies the rule to the 16 pairs.
// Sizes: 2 sides x PLANES x 64 x 9 x 8 bytes of LDS (9 216 with one plane: no limit on the workgroups of a CU; 27 648
// with three) and 16 results per thread and accumulator.  Per word and plane a thread issues 8 ds_read_b64 for 16 rule
// applications (64 VALU operations with one popcount pair each), so the vector ALU, not the LDS, sets the pace.  The
// pitch of 9 words puts the 16 rows tx + 16 j a half-wave reads (bytes 72 tx) on 16 different even bank pairs; the rows
// ty + 16 i of a wave are 4 broadcasts.
// No float, no loop that waits on another lane or workgroup, every loop bounded by its arguments or a constant.
#pragma once

constexpr int BT_THREADS = 256;
constexpr int BT_ROWS = 64;                 // rows of either operand per tile
constexpr int BT_KW = 8;                    // words per staged chunk
constexpr int BT_PITCH = BT_KW + 1;         // words per LDS row
constexpr int BT_PLANE = BT_ROWS * BT_PITCH;    // words of one staged plane

// The tile pair (bi, bj >= bi) of workgroup `b` in a grid of the nt (nt + 1) / 2 pairs on and above the diagonal: row
// bi of the triangle holds the pairs (bi, bi .. nt - 1), found in a loop of at most nt steps.  False for a workgroup
// past the triangle (never with that grid).
__device__ __forceinline__ bool bit_tile_pair(int b, int nt, int &bi, int &bj)
{
    int rest = b;
    bi = 0;
    for (int width = nt; bi < nt - 1 && rest >= width; --width) { rest -= width; ++bi; }
    bj = bi + rest;
    return bj < nt;
}

// One tile over the words w_begin .. w_end - 1.  The tile holds rows_a / rows_b rows of the operands (64 or more: a full
// tile); `load_a(row, plane, w)` / `load_b(row, plane, w)` give word w of tile row `row` below that; `word(i, j, x, y)`
// takes the PLANES words x of row ty + 16 i of A and y of row tx + 16 j of B and adds to the caller's accumulators.
// The k loop of a full chunk is unrolled UNROLL times (BT_KW = completely), that of the last, partial chunk is
// counted.  May be called again by the same workgroup: every chunk starts behind a barrier.
template <int PLANES, int UNROLL, class LoadA, class LoadB, class Word>
__device__ __forceinline__ void bit_tile_product(int rows_a, int rows_b, int w_begin, int w_end, LoadA load_a, LoadB load_b,
                                                 Word word)
{
    __shared__ uint64_t sA[PLANES * BT_PLANE], sB[PLANES * BT_PLANE];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int lr = tid >> 3, lk = tid & 7;      // staging: rows lr and lr + 32, word lk of the chunk
    const uint64_t *rowA = sA + ty * BT_PITCH, *rowB = sB + tx * BT_PITCH;
    auto step = [&](int k) {
        uint64_t x[4][PLANES], y[4][PLANES];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int p = 0; p < PLANES; ++p) x[i][p] = rowA[p * BT_PLANE + 16 * i * BT_PITCH + k];
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int p = 0; p < PLANES; ++p) y[j][p] = rowB[p * BT_PLANE + 16 * j * BT_PITCH + k];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) word(i, j, x[i], y[j]);
    };
    for (int w0 = w_begin; w0 < w_end; w0 += BT_KW) {
        __syncthreads();                        // the tiles of the step before have been read
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int row = lr + 32 * h, w = w0 + lk;
#pragma unroll
            for (int p = 0; p < PLANES; ++p) {
                sA[p * BT_PLANE + row * BT_PITCH + lk] = (row < rows_a && w < w_end) ? load_a(row, p, w) : uint64_t(0);
                sB[p * BT_PLANE + row * BT_PITCH + lk] = (row < rows_b && w < w_end) ? load_b(row, p, w) : uint64_t(0);
            }
        }
        __syncthreads();
        if (w_end - w0 >= BT_KW) {
#pragma unroll UNROLL
            for (int k = 0; k < BT_KW; ++k) step(k);
        } else {
            for (int k = 0; k < w_end - w0; ++k) step(k);
        }
    }
}

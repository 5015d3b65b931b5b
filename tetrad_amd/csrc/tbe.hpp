// tbe.hpp -- transfer bootstrap supports (TBE, Lemoine et al. 2018) of the branches of one reference tree over many
// replicate trees.  No reference counterpart.
// Part of the single translation unit tetrad_hip.hip (included inside its anonymous namespace, behind consensus.hpp).
//
// One rule, executed on the host and on the device, integers only:
//   branch    the splits of the reference tree as `cons_host_splits` gives them (the side without taxon 0, W u64 words),
//             masks ascending as one integer; p = the light side's size, min(|mask|, T - |mask|) >= 2.
//   distance  of two bipartitions with masks x, y: d = popcount(x xor y) over the W words (`tbe_word_distance` summed),
//             delta = min(d, T - d) (`tbe_delta`): the taxa to move, whichever side either mask names.
//   index     phi(b, t) = the minimum of delta over every edge of replicate t.  The edge above a tip of the light side
//             gives p - 1 and no tip edge gives less, so phi = min(p - 1, min over the internal nodes of t of delta).
//             A node that stands for no split (the root: the empty side; a side of one taxon) has delta >= p - 1 and
//             may be taken or skipped alike.
//   sums      phi_sum[b] += phi(b, t), u64; ntrees += 1.  Any chunking and any order of adds give the same numbers.
//
// Device layout (all of it allocated at create): a chunk of prepared trees is staged through a page-locked buffer,
// `tq_cons_mask_kernel` (consensus.hpp, unchanged) fills the chunk's [chunk][T - 2][W] masks, and behind it on the stream
//   tq_tbe_kernel   grid (replicate of the chunk, tile of 64 branches): the tile product of bit_tile.hpp with the
//                   branches as A, the replicate's M nodes as B (M from the tree's record; rows v >= M of the scratch
//                   hold an earlier chunk's masks and are never read) and `tbe_word_distance` as the word rule.  The
//                   workgroup walks the nodes in tiles of 64; after the last word of a tile delta is folded into 4
//                   running minima, after the last node tile the minima are reduced over the 16 lanes that share the
//                   branches (shuffles), clamped to p - 1, added to phi_sum with one 64-bit integer atomic per
//                   (branch, replicate) and, when asked for, stored as u16 phi[replicate][branch].
// With the operand words of the unrolled chunk in flight the kernel takes 92 VGPRs, 5 waves per SIMD.
// No float, no loop that waits on another lane or workgroup, every loop bounded by T, W or a constant.
#pragma once

// d of one word; d of two masks is the sum over their W words
__host__ __device__ __forceinline__ uint32_t tbe_word_distance(uint64_t x, uint64_t y)
{
    return (uint32_t)__builtin_popcountll(x ^ y);
}

// delta of a summed d: the lighter way round
__host__ __device__ __forceinline__ uint32_t tbe_delta(uint32_t d, uint32_t T) { return d < T - d ? d : T - d; }

// The branches of a prepared reference tree: masks[E][W] ascending, p[E].
inline void tbe_reference(const int32_t *rec, int32_t T, int32_t W, std::vector<uint64_t> &masks, std::vector<int32_t> &p)
{
    std::vector<uint64_t> tmp, sides;
    cons_host_splits(rec, T, W, tmp, sides);
    const int64_t E = (int64_t)(sides.size() / W);
    std::vector<int64_t> order(E);
    for (int64_t e = 0; e < E; ++e) order[e] = e;
    std::sort(order.begin(), order.end(), [&](int64_t x, int64_t y) { return cons_mask_less(&sides[x * W], &sides[y * W], W); });
    masks.resize((size_t)E * W);
    p.resize((size_t)E);
    for (int64_t e = 0; e < E; ++e) {
        const uint64_t *src = &sides[order[e] * W];
        uint32_t pc = 0;
        for (int32_t w = 0; w < W; ++w) {
            masks[e * W + w] = src[w];
            pc += tbe_word_distance(src[w], 0);
        }
        p[e] = (int32_t)tbe_delta(pc, (uint32_t)T);
    }
}

// Host execution: phi[e] of one prepared replicate against the E branches; `tmp` and `sides` are scratch.
inline void tbe_host_tree(const int32_t *rec, int32_t T, int32_t W, const std::vector<uint64_t> &masks,
                          const std::vector<int32_t> &p, std::vector<uint64_t> &tmp, std::vector<uint64_t> &sides,
                          uint32_t *phi)
{
    sides.clear();
    cons_host_splits(rec, T, W, tmp, sides);
    const size_t E = p.size(), N = sides.size() / W;
    for (size_t e = 0; e < E; ++e) {
        uint32_t best = (uint32_t)p[e] - 1;
        const uint64_t *x = &masks[e * W];
        for (size_t v = 0; v < N && best; ++v) {
            const uint64_t *y = &sides[v * W];
            uint32_t d = 0;
            for (int32_t w = 0; w < W; ++w) d += tbe_word_distance(x[w], y[w]);
            best = std::min(best, tbe_delta(d, (uint32_t)T));
        }
        phi[e] = best;
    }
}

// ---------------------------------------------------------------------------------------------
// Device path
// ---------------------------------------------------------------------------------------------
struct TbeArgs {
    const int32_t *trees;           // [chunk][cons_stride(T)] prepared records
    const uint64_t *masks;          // [chunk][T - 2][W], rows 0..M-1 of a tree written by tq_cons_mask_kernel
    const uint64_t *ref;            // [E][W]
    const int32_t *p;               // [E]
    unsigned long long *phi_sum;    // [E]
    uint16_t *phi;                  // [chunk][E] or NULL
    int32_t T, W, E;
};

__global__ __launch_bounds__(BT_THREADS) void tq_tbe_kernel(TbeArgs a)
{
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int T = a.T, W = a.W, E = a.E;
    const int e0 = blockIdx.y * BT_ROWS;
    const int M = min(a.trees[(int64_t)blockIdx.x * cons_stride(T)], T - 2);
    const uint64_t *nodes = a.masks + (int64_t)blockIdx.x * (T - 2) * W;
    uint32_t best[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) best[i] = (uint32_t)T;
    for (int v0 = 0; v0 < M; v0 += BT_ROWS) {
        uint32_t acc[4][4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = 0;
        bit_tile_product<1, BT_KW>(
            E - e0, M - v0, 0, W,               // rows past E or M and words past W are zero: they add nothing to d
            [&](int row, int, int w) { return a.ref[(int64_t)(e0 + row) * W + w]; },
            [&](int row, int, int w) { return nodes[(int64_t)(v0 + row) * W + w]; },
            [&](int i, int j, const uint64_t (&x)[1], const uint64_t (&y)[1]) { acc[i][j] += tbe_word_distance(x[0], y[0]); });
        // a zero row (v >= M) gives delta = p >= p - 1: it never lowers the clamped minimum
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) best[i] = min(best[i], tbe_delta(acc[i][j], (uint32_t)T));
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
        for (int o = 8; o > 0; o >>= 1) best[i] = min(best[i], (uint32_t)__shfl_xor((int)best[i], o, 16));
    if (tx == 0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int e = e0 + ty + 16 * i;
            if (e < E) {
                const uint32_t phi = min(best[i], (uint32_t)a.p[e] - 1u);
                atomicAdd(&a.phi_sum[e], (unsigned long long)phi);
                if (a.phi) a.phi[(int64_t)blockIdx.x * E + e] = (uint16_t)phi;
            }
        }
    }
}

// treedist.hpp -- all-pairs Robinson-Foulds distances of a set of trees.  No reference counterpart.
// Part of the single translation unit tetrad_hip.hip (included inside its anonymous namespace, behind tbe.hpp).
//
// One rule, executed on the host and on the device, integers only:
//   split     of a tree as `cons_host_splits` / `tq_cons_mask_kernel` give it: the side without taxon 0 of an internal
//             edge with at least 2 taxa on both sides, W u64 words.
//   id        every distinct split of the set has one number, found by a comparison of the full mask.
//   nsplits   [i] = the splits of tree i;  shared[i][j] = the ids both trees hold, shared[i][i] = nsplits[i];
//   rf        [i][j] = nsplits[i] + nsplits[j] - 2 shared[i][j], the size of the symmetric difference.
// Any chunking of trees or columns, any order of adds and any hash width give the same numbers.
//
// Host execution: a tree is the ascending list of its ids (`rf_host_shared` merges two lists).
//
// Device layout (all of it allocated at create).  At add, per chunk of prepared trees: `tq_cons_mask_kernel` and
// `tq_cons_insert_kernel` (consensus.hpp, unchanged) on a table the accumulator owns, then
//   tq_rf_ident_kernel    G lanes per (tree, node), as tq_cons_count_kernel: finds the entry of the node's key again and
//                         compares all W words.  Equal: integer atomic add on the entry's tree count and on
//                         nsplits[tree], the entry index stored as ids[tree][node].  Different: a true collision, the item
//                         goes to the unresolved list and its id stays RF_NONE until the host has looked the mask up in
//                         its exact map.  Host ids count down from max_splits - 1; device entries count up from 0, and
//                         both together never exceed max_splits.
//   tq_rf_patch_kernel    stores the ids the host gave to the unresolved items and counts them in nsplits.
// At read: a column is an id held by at least two trees (the host numbers them from the entry counts and uploads
// id -> column).  For as many columns at a time as the bit scratch holds:
//   tq_rf_scatter_kernel  threads over (tree, node): sets bit (column - first) of row `tree` of B[N][pitch] with a 64-bit
//                         integer atomic OR.
//   tq_rf_gemm_kernel     shared += B B^T on bit rows: the tile product of bit_tile.hpp, 64 trees x 64 trees, with
//                         `rf_word_shared` = popcount(x & y) as the word rule.  The grid is the tile pairs bj >= bi only
//                         (`bit_tile_pair`).  Every (i, j) of those tiles belongs to one thread, which adds its count
//                         with a plain read-modify-write; the column chunks follow each other on the stream.  No atomics.
//   tq_rf_final_kernel    threads over (i, j): the diagonal from nsplits, the tiles below the diagonal mirrored from the
//                         ones above, rf from both.  A thread below the diagonal tiles reads [j][i], which no thread of
//                         this kernel writes.
// No float, no loop that waits on another lane or workgroup, every loop bounded by T, W, N, Cw or a constant.
#pragma once

constexpr int RF_THREADS = BT_THREADS;
constexpr int RF_BT = BT_ROWS;              // trees per tile side
constexpr uint32_t RF_NONE = ~uint32_t(0);  // id of a node that is no split; column of an id held by one tree
constexpr int64_t RF_MAX_TREES = 8192;

// the columns two bit rows share in one word; shared[i][j] is the sum over the words
__host__ __device__ __forceinline__ uint32_t rf_word_shared(uint64_t x, uint64_t y)
{
    return (uint32_t)__builtin_popcountll(x & y);
}

__host__ __device__ __forceinline__ uint32_t rf_distance(uint32_t ni, uint32_t nj, uint32_t s) { return ni + nj - 2 * s; }

// Host execution: the ids two ascending lists have in common.
inline uint32_t rf_host_shared(const std::vector<uint32_t> &a, const std::vector<uint32_t> &b)
{
    uint32_t n = 0;
    size_t i = 0, j = 0;
    while (i < a.size() && j < b.size()) {
        if (a[i] < b[j]) ++i;
        else if (b[j] < a[i]) ++j;
        else { ++n; ++i; ++j; }
    }
    return n;
}

// ---------------------------------------------------------------------------------------------
// Device path
// ---------------------------------------------------------------------------------------------
struct RfIdentArgs {
    uint32_t *ids;              // [max_trees][T - 2]
    int32_t *nsplits;           // [max_trees]
    int64_t tree_base;          // first tree of the chunk
};

__global__ __launch_bounds__(CONS_THREADS) void tq_rf_ident_kernel(ConsArgs a, RfIdentArgs r)
{
    const int G = a.G, l = threadIdx.x % G;
    const int64_t item = ((int64_t)blockIdx.x * CONS_THREADS + threadIdx.x) / G;
    const uint64_t key = item < a.items ? a.keys[item] : CONS_EMPTY;
    int32_t idx = -1;
    if (key != CONS_EMPTY) {                    // the lanes of a group probe alike (reads only)
        uint64_t s = cons_slot(key) & (uint64_t)a.slot_mask;
        for (int64_t p = 0; p <= a.slot_mask; ++p) {
            const unsigned long long k = a.slot_key[s];
            if (k == key) { idx = a.slot_idx[s]; break; }
            if (k == CONS_EMPTY) break;
            s = (s + 1) & (uint64_t)a.slot_mask;
        }
    }
    int same = 1;
    if (idx >= 0 && l < a.W) same = a.rep[(int64_t)idx * a.W + l] == a.masks[item * a.W + l];
    for (int o = G >> 1; o > 0; o >>= 1) same &= __shfl_xor(same, o, G);
    if (l != 0 || item >= a.items) return;
    const int nodes = a.T - 2;
    const int64_t tree = r.tree_base + item / nodes;
    uint32_t id = RF_NONE;
    if (key != CONS_EMPTY) {
        if (idx < 0) {
            a.ctr[CONS_CTR_OVERFLOW] = 1u;      // its key found no entry: more distinct splits than max_splits
        } else if (same) {
            atomicAdd(&a.count[idx], 1ull);
            atomicAdd(&r.nsplits[tree], 1);
            id = (uint32_t)idx;
        } else {
            const unsigned int u = atomicAdd(&a.ctr[CONS_CTR_UNRES], 1u);
            a.unres[u] = (uint32_t)item;
        }
    }
    r.ids[r.tree_base * nodes + item] = id;
}

// ids[tree_base][unres[e]] = newid[e] for e < n, one more split for the tree
__global__ __launch_bounds__(CONS_THREADS) void tq_rf_patch_kernel(const uint32_t *unres, const uint32_t *newid, int64_t n,
                                                                   RfIdentArgs r, int32_t nodes)
{
    const int64_t e = (int64_t)blockIdx.x * CONS_THREADS + threadIdx.x;
    if (e >= n) return;
    const int64_t item = unres[e];
    r.ids[r.tree_base * nodes + item] = newid[e];
    atomicAdd(&r.nsplits[r.tree_base + item / nodes], 1);
}

struct RfBitArgs {
    const uint32_t *ids;        // [N][T - 2]
    const uint32_t *colmap;     // [max_splits] id -> column or RF_NONE
    unsigned long long *bits;   // [N][pitch]
    int64_t items;              // N x (T - 2)
    int64_t pitch;              // words per row of `bits`
    uint32_t col0, ncol;        // the chunk's columns
    int32_t nodes;              // T - 2
};

__global__ __launch_bounds__(RF_THREADS) void tq_rf_scatter_kernel(RfBitArgs a)
{
    const int64_t item = (int64_t)blockIdx.x * RF_THREADS + threadIdx.x;
    if (item >= a.items) return;
    const uint32_t id = a.ids[item];
    if (id == RF_NONE) return;
    const uint32_t col = a.colmap[id];
    if (col == RF_NONE || col < a.col0 || col - a.col0 >= a.ncol) return;
    const uint32_t c = col - a.col0;
    atomicOr(&a.bits[(item / a.nodes) * a.pitch + (c >> 6)], 1ull << (c & 63));
}

struct RfGemmArgs {
    const uint64_t *bits;       // [N][pitch], words 0..Cw-1 of a row hold the chunk's columns
    uint32_t *shared;           // [N][N]
    int64_t pitch;
    int32_t N, Cw, nt;          // trees, words of the chunk, tiles per side
};

__global__ __launch_bounds__(RF_THREADS) void tq_rf_gemm_kernel(RfGemmArgs a)
{
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int N = a.N;
    int bi, bj;
    if (!bit_tile_pair((int)blockIdx.x, a.nt, bi, bj)) return;
    const int r0 = bi * RF_BT, c0 = bj * RF_BT;
    uint32_t acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0;
    bit_tile_product<1, BT_KW>(                 // rows past N and words past Cw are zero: they share nothing
        N - r0, N - c0, 0, a.Cw,
        [&](int row, int, int w) { return a.bits[(int64_t)(r0 + row) * a.pitch + w]; },
        [&](int row, int, int w) { return a.bits[(int64_t)(c0 + row) * a.pitch + w]; },
        [&](int i, int j, const uint64_t (&x)[1], const uint64_t (&y)[1]) { acc[i][j] += rf_word_shared(x[0], y[0]); });
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int r = r0 + ty + 16 * i;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int c = c0 + tx + 16 * j;
            if (r < N && c < N) a.shared[(int64_t)r * N + c] += acc[i][j];      // this thread alone owns (r, c)
        }
    }
}

__global__ __launch_bounds__(RF_THREADS) void tq_rf_final_kernel(uint32_t *shared, uint32_t *rf, const int32_t *nsplits, int32_t N)
{
    const int64_t idx = (int64_t)blockIdx.x * RF_THREADS + threadIdx.x;
    if (idx >= (int64_t)N * N) return;
    const int r = (int)(idx / N), c = (int)(idx % N);
    const bool below = r / RF_BT > c / RF_BT;   // a tile the product did not visit
    const uint32_t s = r == c ? (uint32_t)nsplits[r] : shared[below ? (int64_t)c * N + r : idx];
    if (r == c || below) shared[idx] = s;
    rf[idx] = rf_distance((uint32_t)nsplits[r], (uint32_t)nsplits[c], s);
}

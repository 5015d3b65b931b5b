// supertree.hpp -- exact quartet supertree: Quartet MaxCut level by level, integer graph weights, the quartet passes on
// the device next to the resolved rows.  Part of the single translation unit tetrad_hip.hip
// (included inside its anonymous namespace).  tq_qmc_tree (qmc.hpp) is untouched; this is a second path.
//
// Rule (one definition, a host and a device execution of it):
//   * `stree_row` turns a resolved row into a weighted split: the filters, split and weight of format.hpp's qmc_row,
//     the weight kept as the integer k = weight x 10^5 rounded as its "%.5f" text rounds.
//   * For every open node of a level the graph G (good edges a-c, a-d, b-c, b-d) and B (bad edges a-b, c-d) are sums
//     of k in u64 over the node's live quartets, upper triangle only: order-independent, so any launch shape, any row
//     order and any split of the rows over several adds give the same cells.
//   * Each node's cut is searched by one of two rules.  "f64" (default): the host runs qmc_search of qmc.hpp on cell /
//     10^5 as doubles, one generator per node keyed by (seed, level, index of the node in its level).  "exact"
//     (tq_stree_set_search): stree_search_exact, all-integer, which the device back end runs in
//     tq_stree_search_kernel with the matrices where the graph pass left them.
//   * One pass partitions the live quartets: four taxa on a side -> that child; three -> that child with the odd taxon
//     replaced by the child's artificial taxon; 2 | 2 -> dropped.
//   The level loop, the search, the forest and the newick writer are one piece of host code (`stree_build`) that talks
//   to a back end with three operations, `graphs`, `search` (rule "exact" only) and `partition`: StreeHostBackend on
//   host arrays, StreeDevBackend on the device.  All three are exact, so the two give the same newick string.
//
// Device layout: a live quartet is {four node-local taxon indices u16 packed in a u64, k u64, node id u32}.  The rows
// kept by the add kernel sit in the accumulator's root store (node 0 implied) and are never modified; the partition
// pass of level L writes work buffer L & 1.  A level's matrices are one u64 array [2][cells], node i at `toff`, cell
// (u < v) at u * n - u (u + 1) / 2 + v - u - 1.
#pragma once

constexpr int STREE_T_MAX = 1024;               // device path: 4 <= ntaxa <= 1024 (u16 indices; 3 T^2 u64 cells per level)
constexpr int STREE_THREADS = 256;
constexpr int STREE_LDS_CELLS = 8128;           // 128 * 127 / 2 u64 counters = 63.5 KiB of LDS per workgroup
constexpr int STREE_LDS_THREADS = 512;
constexpr int STREE_MAX_LEVELS = 64;            // levels the per-level statistics keep (deeper ones are still run)
constexpr uint64_t STREE_K_SCALE = 100000;      // weight = k / 10^5
constexpr uint64_t STREE_SUM_LIMIT = 1501199875790166ull;   // smallest sum of k with 6 * sum >= 2^53

// k = the integer nearest to the exact w * 10^5 (ties to even): the digits "%.5f" prints.  0 when w is not in
// (0, 4e9) or not finite, and when it rounds to 0.  w * 10^5 = p + err exactly (fma), the product is below 2^53.
__host__ __device__ __forceinline__ uint64_t stree_round_k(double w)
{
#pragma clang fp contract(off)
    if (!(w > 0.0) || !(w < 4.0e9)) return 0;
    const double p = w * 1e5;
    const double err = fma(w, 1e5, -p);
    const double n = floor(p);
    const double t = (p - n) - 0.5;
    bool up = t > -err;
    if (t == -err) up = (n - 2.0 * floor(n * 0.5)) != 0.0;
    return (uint64_t)n + (up ? 1u : 0u);
}

// One resolved row -> (split a,b|c,d, k).  false: the row is skipped (taxon >= T, repeated taxon, topology > 2, flags
// TQ_FLAG_BAD_INDEX / TQ_FLAG_INVALID_DIAGNOSTIC, nsnps < min_snps, ratio < min_ratio, k == 0).  min_snps >= 1.
__host__ __device__ __forceinline__ bool stree_row(uint32_t T, int weights, uint32_t min_snps, double min_ratio, uint32_t a,
                                                   uint32_t b, uint32_t c, uint32_t d, uint32_t topo, uint32_t nsnps,
                                                   double x0, double x1, double x2, uint32_t flags, uint32_t (&split)[4],
                                                   uint64_t &k)
{
#pragma clang fp contract(off)
    if ((flags & (4u | 16u)) || a >= T || b >= T || c >= T || d >= T || topo > 2u) return false;
    if (a == b || a == c || a == d || b == c || b == d || c == d) return false;
    if (nsnps < min_snps) return false;
    double weight = 1.0, ratio = 1.0;
    if (weights) {
        double s0 = conc_reread6(x0), s1 = conc_reread6(x1), s2 = conc_reread6(x2), tmp;
        if (s0 > s1) { tmp = s0; s0 = s1; s1 = tmp; }
        if (s1 > s2) { tmp = s1; s1 = s2; s2 = tmp; }
        if (s0 > s1) { tmp = s0; s0 = s1; s1 = tmp; }
        const double smean = (s1 + s2) / 2.0;
        ratio = s0 == 0.0 ? 1.0 : smean / s0;
        if (weights == 1) weight = smean;
        else if (weights == 2) weight = ratio;
        else weight = 1.0 - s0 / ((s0 + s1) + s2);
    }
    if (ratio < min_ratio) return false;
    k = stree_round_k(weight);
    if (k == 0) return false;
    split[0] = a; split[1] = b; split[2] = c; split[3] = d;
    if (topo == 1) { split[1] = c; split[2] = b; }
    else if (topo == 2) { split[1] = d; split[2] = b; split[3] = c; }
    return true;
}

// an open node of a level, as both back ends see it
struct StreeNode {
    uint32_t toff;              // first cell of its triangle in the level's matrices
    uint32_t moff;              // first entry of its taxa in the level's side map
    int32_t n;                  // taxa (artificial ones included)
    int32_t childA, childB;     // index in the next level, -1: the node became a star (its quartets leave)
    uint32_t nA, nB;            // real sizes of the two sides = local index of the artificial taxon in each child
    uint32_t pad;
};

__host__ __device__ __forceinline__ uint32_t stree_tri(uint32_t u, uint32_t v, uint32_t n)
{
    if (u > v) { const uint32_t t = u; u = v; v = t; }
    return u * n - u * (u + 1) / 2 + (v - u - 1);
}

// the six cells of a live quartet: bad a-b, c-d; good a-c, a-d, b-c, b-d
__host__ __device__ __forceinline__ void stree_cells(uint64_t t4, uint32_t n, uint32_t (&bad)[2], uint32_t (&good)[4])
{
    const uint32_t a = (uint32_t)(t4 & 0xFFFF), b = (uint32_t)((t4 >> 16) & 0xFFFF), c = (uint32_t)((t4 >> 32) & 0xFFFF),
                   d = (uint32_t)(t4 >> 48);
    bad[0] = stree_tri(a, b, n);
    bad[1] = stree_tri(c, d, n);
    good[0] = stree_tri(a, c, n);
    good[1] = stree_tri(a, d, n);
    good[2] = stree_tri(b, c, n);
    good[3] = stree_tri(b, d, n);
}

// where a live quartet goes under its node's cut: false = it leaves.  map entry = side << 16 | index in the child.
__host__ __device__ __forceinline__ bool stree_route(const StreeNode &nd, const uint32_t *map, uint64_t t4, uint64_t &out4,
                                                     uint32_t &child)
{
    if (nd.childA < 0) return false;
    uint32_t m[4], ones = 0;
    for (int j = 0; j < 4; ++j) {
        m[j] = map[nd.moff + (uint32_t)((t4 >> (16 * j)) & 0xFFFF)];
        ones += m[j] >> 16;
    }
    if (ones == 2) return false;
    const bool toB = ones >= 3;
    const uint32_t odd_side = ones == 1 ? 1u : (ones == 3 ? 0u : 2u);      // side of the taxon that is replaced
    const uint32_t art = toB ? nd.nB : nd.nA;
    out4 = 0;
    for (int j = 0; j < 4; ++j) {
        const uint32_t idx = (m[j] >> 16) == odd_side ? art : (m[j] & 0xFFFF);
        out4 |= (uint64_t)idx << (16 * j);
    }
    child = (uint32_t)(toB ? nd.childB : nd.childA);
    return true;
}

// ------------------------------------------------------------------------------------------------------------------
// kernels
// ------------------------------------------------------------------------------------------------------------------
enum { SC_KEPT = 0, SC_SKIPPED = 1, SC_SUM_LO = 2, SC_SUM_HI = 3, SC_LIVE0 = 4, SC_LIVE1 = 5, SC_WORDS = 8 };

// slot of this lane among the lanes of its wave that keep a row: one atomic per wave
__device__ __forceinline__ uint32_t stree_wave_slot(bool keep, unsigned long long *counter)
{
    const unsigned long long mask = __ballot(keep);
    const int lane = (int)(threadIdx.x & 63);
    const int leader = mask ? __ffsll((long long)mask) - 1 : 0;
    unsigned long long base = 0;
    if (mask && lane == leader) base = atomicAdd(counter, (unsigned long long)__popcll(mask));
    base = __shfl(base, leader);
    return (uint32_t)base + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
}

struct StreeAddArgs {
    const uint32_t *q;          // [n][4]
    const uint32_t *rstat;      // [n][2]
    const double *rscor;        // [n][3]
    const uint8_t *flags;       // [n] or null
    int64_t n;
    uint32_t T, min_snps;
    int32_t weights;
    double min_ratio;
    uint64_t *root_t, *root_k;  // the root store; the kernel appends at counters[SC_KEPT]
    int64_t capacity;
    unsigned long long *counters;
};

// rows -> live quartets at the root, one thread per row
__global__ __launch_bounds__(STREE_THREADS) void tq_stree_rows_kernel(StreeAddArgs a)
{
    __shared__ unsigned long long s_sum[2];
    __shared__ uint32_t s_skip;
    if (threadIdx.x == 0) { s_sum[0] = 0; s_sum[1] = 0; s_skip = 0; }
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * STREE_THREADS + threadIdx.x;
    bool keep = false;
    uint32_t sp[4] = {0, 0, 0, 0};
    uint64_t k = 0;
    if (i < a.n) {
        const uint4 q = ((const uint4 *)a.q)[i];
        const uint2 st = ((const uint2 *)a.rstat)[i];
        const double x0 = a.rscor[3 * i], x1 = a.rscor[3 * i + 1], x2 = a.rscor[3 * i + 2];
        const uint32_t fl = a.flags ? a.flags[i] : 0u;
        keep = stree_row(a.T, a.weights, a.min_snps, a.min_ratio, q.x, q.y, q.z, q.w, st.x, st.y, x0, x1, x2, fl, sp, k);
        if (!keep) atomicAdd(&s_skip, 1u);
    }
    const uint32_t slot = stree_wave_slot(keep, &a.counters[SC_KEPT]);
    if (keep && (int64_t)slot < a.capacity) {               // the host has checked rows against capacity before the launch
        a.root_t[slot] = (uint64_t)sp[0] | (uint64_t)sp[1] << 16 | (uint64_t)sp[2] << 32 | (uint64_t)sp[3] << 48;
        a.root_k[slot] = k;
        atomicAdd(&s_sum[0], (unsigned long long)(k & 0xFFFFFFFFull));
        atomicAdd(&s_sum[1], (unsigned long long)(k >> 32));
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (s_sum[0]) atomicAdd(&a.counters[SC_SUM_LO], s_sum[0]);
        if (s_sum[1]) atomicAdd(&a.counters[SC_SUM_HI], s_sum[1]);
        if (s_skip) atomicAdd(&a.counters[SC_SKIPPED], (unsigned long long)s_skip);
    }
}

struct StreePassArgs {
    const uint64_t *t4, *k;     // live quartets of this level
    const uint32_t *node;       // null at the root: every quartet is in node 0
    const unsigned long long *n_live;
    const StreeNode *nodes;
    int32_t n_nodes;
    int64_t cells;              // of one matrix of this level
    unsigned long long *mat;    // [2][cells]: G then B
    // partition only
    const uint32_t *map;
    uint64_t *out_t4, *out_k;
    uint32_t *out_node;
    unsigned long long *out_live;
};

// graph pass, global form: six integer atomics per live quartet straight into the level's matrices
__global__ __launch_bounds__(STREE_THREADS) void tq_stree_graph_kernel(StreePassArgs a)
{
    const int64_t n = (int64_t)*a.n_live;
    const int64_t stride = (int64_t)gridDim.x * STREE_THREADS;
    for (int64_t i = (int64_t)blockIdx.x * STREE_THREADS + threadIdx.x; i < n; i += stride) {
        const uint32_t nd = a.node ? a.node[i] : 0u;
        if (nd >= (uint32_t)a.n_nodes) continue;
        const StreeNode info = a.nodes[nd];
        if (info.n < 4) continue;
        uint32_t bad[2], good[4];
        stree_cells(a.t4[i], (uint32_t)info.n, bad, good);
        const unsigned long long k = a.k[i];
        unsigned long long *G = a.mat + info.toff, *B = a.mat + a.cells + info.toff;
        atomicAdd(&B[bad[0]], k);
        atomicAdd(&B[bad[1]], k);
        atomicAdd(&G[good[0]], k);
        atomicAdd(&G[good[1]], k);
        atomicAdd(&G[good[2]], k);
        atomicAdd(&G[good[3]], k);
    }
}

// graph pass, LDS form (cells <= STREE_LDS_CELLS): even workgroups sum G, odd ones B, of the same slice of the live
// quartets, in private u64 counters; then one integer atomic per non-zero cell and workgroup
__global__ __launch_bounds__(STREE_LDS_THREADS) void tq_stree_graph_lds_kernel(StreePassArgs a)
{
    __shared__ unsigned long long s_cell[STREE_LDS_CELLS];
    const int cells = (int)a.cells;
    for (int c = threadIdx.x; c < cells; c += STREE_LDS_THREADS) s_cell[c] = 0;
    __syncthreads();
    const int which = blockIdx.x & 1;                       // 0: G, 1: B
    const int64_t n = (int64_t)*a.n_live;
    const int64_t stride = (int64_t)(gridDim.x / 2) * STREE_LDS_THREADS;
    for (int64_t i = (int64_t)(blockIdx.x / 2) * STREE_LDS_THREADS + threadIdx.x; i < n; i += stride) {
        const uint32_t nd = a.node ? a.node[i] : 0u;
        if (nd >= (uint32_t)a.n_nodes) continue;
        const StreeNode info = a.nodes[nd];
        if (info.n < 4) continue;
        uint32_t bad[2], good[4];
        stree_cells(a.t4[i], (uint32_t)info.n, bad, good);
        const unsigned long long k = a.k[i];
        unsigned long long *S = s_cell + info.toff;
        if (which) {
            atomicAdd(&S[bad[0]], k);
            atomicAdd(&S[bad[1]], k);
        } else {
            atomicAdd(&S[good[0]], k);
            atomicAdd(&S[good[1]], k);
            atomicAdd(&S[good[2]], k);
            atomicAdd(&S[good[3]], k);
        }
    }
    __syncthreads();
    unsigned long long *M = a.mat + (which ? a.cells : 0);
    for (int c = threadIdx.x; c < cells; c += STREE_LDS_THREADS)
        if (s_cell[c]) atomicAdd(&M[c], s_cell[c]);
}

// partition pass: route every live quartet through its node's cut, survivors compacted into the other work buffer
__global__ __launch_bounds__(STREE_THREADS) void tq_stree_partition_kernel(StreePassArgs a)
{
    const int64_t n = (int64_t)*a.n_live;
    const int64_t stride = (int64_t)gridDim.x * STREE_THREADS;
    const int64_t rounds = (n + stride - 1) / stride;       // every lane of a wave runs the same number of rounds
    for (int64_t r = 0; r < rounds; ++r) {
        const int64_t i = r * stride + (int64_t)blockIdx.x * STREE_THREADS + threadIdx.x;
        bool keep = false;
        uint64_t out4 = 0;
        uint32_t child = 0;
        if (i < n) {
            const uint32_t nd = a.node ? a.node[i] : 0u;
            if (nd < (uint32_t)a.n_nodes) keep = stree_route(a.nodes[nd], a.map, a.t4[i], out4, child);
        }
        const uint32_t slot = stree_wave_slot(keep, a.out_live);
        if (keep) {
            a.out_t4[slot] = out4;
            a.out_k[slot] = a.k[i];
            a.out_node[slot] = child;
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------
// the exact cut search: a second search rule beside qmc_search, on the integer cells alone.
// One definition -- `stree_search_exact` on the host, `tq_stree_search_kernel` on the device -- whose every value is an
// integer, so the two executions are equal bit for bit whatever the launch shape or the order of a reduction.
//
// Range: with S = sum of k < STREE_SUM_LIMIT (6 S < 2^53) a node's G cells sum to at most 4 S and its B cells to at most
// 2 S, so p = good <= 4 S and q = bad <= 2 S.  A gain or an objective is a signed sum of terms q G[u][v] and p B[u][v]
// whose absolute values total at most q 4 S + p 2 S <= 16 S^2 < 2^105 (twice that inside a gain update: < 2^106), and a
// cross product good_X bad_Y is at most 8 S^2 < 2^104.  Signed 128-bit arithmetic never wraps.
// ------------------------------------------------------------------------------------------------------------------
typedef __int128 stree_i128;
typedef unsigned __int128 stree_u128;

constexpr int STREE_SEARCH_THREADS = 512;       // eight waves: the starts of a round are dealt over them
constexpr int STREE_SEARCH_LDS_CELLS = 3072;    // a node of up to 78 taxa keeps its two triangles in LDS (48 KiB)
constexpr int STREE_SEARCH_ROUNDS = 6;

__host__ __device__ __forceinline__ uint64_t stree_mix(uint64_t z)         // QmcRng{s}.next() == stree_mix(s + gamma)
{
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
constexpr uint64_t STREE_GAMMA = 0x9E3779B97F4A7C15ull;

__host__ __device__ __forceinline__ uint64_t stree_node_seed(uint64_t seed, uint64_t level, uint64_t idx)
{
    return stree_mix((seed ^ (level * 0x9E3779B97F4A7C15ull) ^ (idx * 0xD1B54A32D192ED03ull)) + STREE_GAMMA);
}

// state of the generator of start s of round r; its draw v (the (v + 1)-th next()) is stree_start_bit's argument
__host__ __device__ __forceinline__ uint64_t stree_start_seed(uint64_t node_seed, uint32_t round, uint32_t s)
{
    return stree_mix((node_seed ^ ((uint64_t)(32u * round + s + 1u) * 0xD6E8FEB86659FD93ull)) + STREE_GAMMA);
}
__host__ __device__ __forceinline__ uint32_t stree_start_bit(uint64_t state0, uint32_t v)
{
    return (uint32_t)(stree_mix(state0 + (uint64_t)(v + 1u) * STREE_GAMMA) & 1u);
}

// cut X = (gx, bx) beats cut Y: larger good / bad without a division, then larger good
__host__ __device__ __forceinline__ bool stree_better(uint64_t gx, uint64_t bx, uint64_t gy, uint64_t by)
{
    const stree_u128 l = (stree_u128)gx * by, r = (stree_u128)gy * bx;
    return l != r ? l > r : gx > gy;
}
__host__ __device__ __forceinline__ stree_i128 stree_edge(uint64_t p, uint64_t q, uint64_t g, uint64_t b)
{
    return (stree_i128)((stree_u128)q * g) - (stree_i128)((stree_u128)p * b);
}
__host__ __device__ __forceinline__ int stree_starts(int n) { return n <= 8 ? 24 : 12; }

// n = 4: the three 2|2 splits {0, k} | rest, k = 1, 2, 3 in that order; the first best valid one
__host__ __device__ __forceinline__ bool stree_search4(const uint64_t *G, const uint64_t *B, uint32_t &bits)
{
    bool have = false;
    uint64_t bg = 0, bb = 0;
    for (uint32_t k = 1; k < 4; ++k) {
        const uint32_t sb = 0xEu & ~(1u << k);                 // bit v = side of v: 0 and k on side 0
        uint64_t good = 0, bad = 0;
        for (uint32_t u = 0; u < 4; ++u)
            for (uint32_t v = u + 1; v < 4; ++v)
                if (((sb >> u) ^ (sb >> v)) & 1u) {
                    good += G[stree_tri(u, v, 4)];
                    bad += B[stree_tri(u, v, 4)];
                }
        if (good > 0 && (!have || stree_better(good, bad, bg, bb))) {
            have = true;
            bg = good;
            bb = bad;
            bits = sb;
        }
    }
    return have;
}

// the rule on the host.  G, B: the node's triangles, n >= 4; side u8[n]; rounds = Dinkelbach rounds run (0: n = 4 or no B)
inline bool stree_search_exact(const uint64_t *G, const uint64_t *B, int n, uint64_t node_seed, uint8_t *side, int &rounds)
{
    rounds = 0;
    const size_t tri = (size_t)n * (n - 1) / 2;
    uint64_t bsum = 0;
    for (size_t c = 0; c < tri; ++c) bsum |= B[c];
    if (!bsum) return false;
    if (n == 4) {
        uint32_t bits = 0;
        if (!stree_search4(G, B, bits)) return false;
        for (int v = 0; v < 4; ++v) side[v] = (uint8_t)((bits >> v) & 1u);
        return true;
    }
    std::vector<uint64_t> Gf((size_t)n * n, 0), Bf((size_t)n * n, 0);
    {
        size_t c = 0;
        for (int u = 0; u < n; ++u)
            for (int v = u + 1; v < n; ++v, ++c) {
                Gf[(size_t)u * n + v] = Gf[(size_t)v * n + u] = G[c];
                Bf[(size_t)u * n + v] = Bf[(size_t)v * n + u] = B[c];
            }
    }
    std::vector<uint8_t> cur((size_t)n), inc((size_t)n), rbest((size_t)n);
    std::vector<stree_i128> gain((size_t)n);
    uint64_t p = 1, q = 1, ig = 0, ib = 0;
    bool have = false;
    const int starts = stree_starts(n);
    for (int round = 0; round < STREE_SEARCH_ROUNDS; ++round) {
        ++rounds;
        bool rhave = false;
        uint64_t rg = 0, rb = 0;
        for (int s = 0; s <= starts; ++s) {
            if (s == 0 && have) {
                cur = inc;
            } else {
                const uint64_t st0 = stree_start_seed(node_seed, (uint32_t)round, (uint32_t)s);
                int c1 = 0;
                for (int v = 0; v < n; ++v) c1 += (cur[(size_t)v] = (uint8_t)stree_start_bit(st0, (uint32_t)v));
                if (c1 < 2 || n - c1 < 2)
                    for (int v = 0; v < n; ++v) cur[(size_t)v] = (uint8_t)(v & 1);
            }
            int cnt[2] = {0, 0};
            for (int v = 0; v < n; ++v) cnt[cur[(size_t)v]]++;
            for (int v = 0; v < n; ++v) {
                stree_i128 g = 0;
                const uint64_t *gr = &Gf[(size_t)v * n], *br = &Bf[(size_t)v * n];
                for (int u = 0; u < n; ++u) {
                    if (u == v) continue;
                    const stree_i128 w = stree_edge(p, q, gr[u], br[u]);
                    g += cur[(size_t)u] == cur[(size_t)v] ? w : -w;
                }
                gain[(size_t)v] = g;
            }
            for (int64_t pass = 0; pass < 50 * (int64_t)n; ++pass) {
                int best = -1;
                stree_i128 bg = 0;
                for (int v = 0; v < n; ++v)
                    if (gain[(size_t)v] > bg && cnt[cur[(size_t)v]] > 2) {
                        bg = gain[(size_t)v];
                        best = v;
                    }
                if (best < 0) break;
                const int v = best;
                cnt[cur[(size_t)v]]--;
                cur[(size_t)v] ^= 1;
                cnt[cur[(size_t)v]]++;
                gain[(size_t)v] = -gain[(size_t)v];
                const uint64_t *gr = &Gf[(size_t)v * n], *br = &Bf[(size_t)v * n];
                for (int u = 0; u < n; ++u) {
                    if (u == v) continue;
                    const stree_i128 w2 = 2 * stree_edge(p, q, gr[u], br[u]);
                    gain[(size_t)u] += cur[(size_t)u] == cur[(size_t)v] ? w2 : -w2;
                }
            }
            uint64_t good = 0, bad = 0;
            for (int u = 0; u < n; ++u)
                for (int v = u + 1; v < n; ++v)
                    if (cur[(size_t)u] != cur[(size_t)v]) {
                        good += Gf[(size_t)u * n + v];
                        bad += Bf[(size_t)u * n + v];
                    }
            if (!(good > 0 && cnt[0] >= 2 && cnt[1] >= 2)) continue;
            if (!rhave || stree_better(good, bad, rg, rb)) {               // strictly: the lowest s keeps a tie
                rhave = true;
                rg = good;
                rb = bad;
                rbest = cur;
            }
        }
        bool improved = false;
        if (rhave && (!have || stree_better(rg, rb, ig, ib))) {
            have = improved = true;
            ig = rg;
            ib = rb;
            inc = rbest;
        }
        if (!have) return false;
        if (!improved && round > 0) break;
        if (ib == 0) break;
        p = ig;
        q = ib;
    }
    memcpy(side, inc.data(), (size_t)n);
    return true;
}

struct StreeSearchArgs {
    const StreeNode *nodes;
    int32_t n_nodes;
    int64_t cells;                      // of one matrix of this level
    const unsigned long long *mat;      // [2][cells]: G then B, where the graph pass left them
    const uint64_t *seeds;              // a node seed per node, or null: stree_node_seed(seed, level, node)
    uint64_t seed;
    uint32_t level;
    uint8_t *side;                      // side of taxon v of node i at [nodes[i].moff + v], written when the node is cut
    uint8_t *cut;                       // [n_nodes]
    uint8_t *rounds;                    // [n_nodes] or null
};

__device__ __forceinline__ uint64_t stree_wave_sum(uint64_t x)
{
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) x += (uint64_t)__shfl_xor((unsigned long long)x, m);
    return x;
}

// one local search by one wave.  Lane l owns vertices l + 64 j, j < SLOTS: their sides in bit j of `bits`, their gains
// in registers.  The cut's good and bad are kept as they change with every flip (mod 2^64; the true values fit).
template <int SLOTS>
__device__ __forceinline__ void stree_wave_search(const unsigned long long *G, const unsigned long long *B, const uint32_t n,
                                                  const uint64_t p, const uint64_t q, uint32_t &bits, uint64_t &good,
                                                  uint64_t &bad, uint32_t &ones)
{
    const uint32_t lane = threadIdx.x & 63u;
    stree_i128 gain[SLOTS];
#pragma unroll
    for (int j = 0; j < SLOTS; ++j) gain[j] = 0;
    uint64_t pg = 0, pb = 0;
    for (uint32_t u = 0; u < n; ++u) {
        const uint32_t su = ((uint32_t)__shfl((int)bits, (int)(u & 63u)) >> (u >> 6)) & 1u;
#pragma unroll
        for (int j = 0; j < SLOTS; ++j) {
            const uint32_t v = lane + 64u * (uint32_t)j;
            if (v < n && v != u) {
                const uint32_t c = stree_tri(u, v, n);
                const uint64_t g = G[c], b = B[c];
                const stree_i128 w = stree_edge(p, q, g, b);
                if ((((bits >> j) & 1u) == su)) {
                    gain[j] += w;
                } else {
                    gain[j] -= w;
                    pg += g;
                    pb += b;
                }
            }
        }
    }
    const uint64_t good0 = stree_wave_sum(pg) >> 1, bad0 = stree_wave_sum(pb) >> 1;    // every pair was met twice
    pg = lane == 0 ? good0 : 0;
    pb = lane == 0 ? bad0 : 0;
    uint32_t cnt1 = 0;
#pragma unroll
    for (int j = 0; j < SLOTS; ++j) cnt1 += (uint32_t)__popcll(__ballot(lane + 64u * (uint32_t)j < n && ((bits >> j) & 1u)));
    uint32_t cnt0 = n - cnt1;
    const uint32_t flips = 50u * n;
    for (uint32_t pass = 0; pass < flips; ++pass) {
        stree_i128 bg = 0;
        uint32_t bv = 0xFFFFFFFFu;
#pragma unroll
        for (int j = 0; j < SLOTS; ++j) {
            const uint32_t v = lane + 64u * (uint32_t)j;
            if (v < n && gain[j] > bg && (((bits >> j) & 1u) ? cnt1 : cnt0) > 2u) {
                bg = gain[j];
                bv = v;
            }
        }
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) {
            const unsigned long long olo = __shfl_xor((unsigned long long)(stree_u128)bg, m);
            const unsigned long long ohi = __shfl_xor((unsigned long long)((stree_u128)bg >> 64), m);
            const uint32_t ov = (uint32_t)__shfl_xor((int)bv, m);
            const stree_i128 og = (stree_i128)(((stree_u128)ohi << 64) | olo);
            if (og > bg || (og == bg && ov < bv)) {
                bg = og;
                bv = ov;
            }
        }
        if (bv == 0xFFFFFFFFu) break;                                       // the same in every lane
        const uint32_t v = bv, slot = v >> 6;
        const uint32_t sv = ((uint32_t)__shfl((int)bits, (int)(v & 63u)) >> slot) & 1u, nv = sv ^ 1u;
        cnt1 += nv ? 1u : 0xFFFFFFFFu;
        cnt0 += nv ? 0xFFFFFFFFu : 1u;
        if (lane == (v & 63u)) bits ^= 1u << slot;
#pragma unroll
        for (int j = 0; j < SLOTS; ++j) {
            const uint32_t u = lane + 64u * (uint32_t)j;
            if (u == v) {
                gain[j] = -gain[j];
            } else if (u < n) {
                const uint32_t c = stree_tri(u, v, n);
                const uint64_t g = G[c], b = B[c];
                const stree_i128 w2 = 2 * stree_edge(p, q, g, b);
                if (((bits >> j) & 1u) == nv) {                             // u is now on v's side: the pair is no longer cut
                    gain[j] += w2;
                    pg -= g;
                    pb -= b;
                } else {
                    gain[j] -= w2;
                    pg += g;
                    pb += b;
                }
            }
        }
    }
    good = stree_wave_sum(pg);
    bad = stree_wave_sum(pb);
    ones = cnt1;
}

// the rounds of one node by one workgroup: wave w runs starts w, w + waves, ...; two barriers per round
template <int SLOTS>
__device__ void stree_block_search(const unsigned long long *G, const unsigned long long *B, const uint32_t n,
                                   const uint64_t node_seed, unsigned long long *s_good, unsigned long long *s_bad, int *s_s,
                                   uint32_t *s_inc, uint32_t &out_bits, bool &out_cut, uint32_t &out_rounds)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
    const uint32_t starts = (uint32_t)stree_starts((int)n);
    uint64_t p = 1, q = 1, ig = 0, ib = 0;
    bool have = false;
    uint32_t ibits = 0, rounds = 0;
    for (uint32_t round = 0; round < (uint32_t)STREE_SEARCH_ROUNDS; ++round) {
        ++rounds;
        uint64_t wg = 0, wb = 0;
        int ws = -1;
        uint32_t wbits = 0;
        for (uint32_t s = wave; s <= starts; s += waves) {
            uint32_t bits = 0;
            if (s == 0 && have) {
                bits = ibits;
            } else {
                const uint64_t st0 = stree_start_seed(node_seed, round, s);
                uint32_t c1 = 0;
#pragma unroll
                for (int j = 0; j < SLOTS; ++j) {
                    const uint32_t v = lane + 64u * (uint32_t)j;
                    const uint32_t bit = v < n ? stree_start_bit(st0, v) : 0u;
                    bits |= bit << j;
                    c1 += (uint32_t)__popcll(__ballot(bit != 0u));
                }
                if (c1 < 2u || n - c1 < 2u) {
                    bits = 0;
#pragma unroll
                    for (int j = 0; j < SLOTS; ++j)
                        if (lane + 64u * (uint32_t)j < n) bits |= (lane & 1u) << j;
                }
            }
            uint64_t good, bad;
            uint32_t ones;
            stree_wave_search<SLOTS>(G, B, n, p, q, bits, good, bad, ones);
            if (good > 0 && ones >= 2u && n - ones >= 2u && (ws < 0 || stree_better(good, bad, wg, wb))) {
                wg = good;
                wb = bad;
                ws = (int)s;
                wbits = bits;
            }
        }
        if (lane == 0) {
            s_good[wave] = wg;
            s_bad[wave] = wb;
            s_s[wave] = ws;
        }
        __syncthreads();
        int win = -1;
        for (uint32_t w = 0; w < waves; ++w) {
            if (s_s[w] < 0) continue;
            if (win < 0 || stree_better(s_good[w], s_bad[w], s_good[win], s_bad[win]) ||
                (s_good[w] == s_good[win] && s_bad[w] == s_bad[win] && s_s[w] < s_s[win]))
                win = (int)w;
        }
        const bool improved = win >= 0 && (!have || stree_better(s_good[win], s_bad[win], ig, ib));
        if (improved) {
            have = true;
            ig = s_good[win];
            ib = s_bad[win];
            if ((int)wave == win) s_inc[lane] = wbits;
        }
        __syncthreads();                                                    // every value above is the same in all threads
        if (improved) ibits = s_inc[lane];
        if (!have) break;
        if (!improved && round > 0) break;
        if (ib == 0) break;
        p = ig;
        q = ib;
    }
    out_bits = ibits;
    out_cut = have;
    out_rounds = rounds;
}

// the cut search of a level: one workgroup per open node.  No loop waits on another lane, wave or workgroup; every
// loop has a fixed bound (6 rounds, starts + 1 searches, n vertices, 50 n flips).
__global__ __launch_bounds__(STREE_SEARCH_THREADS) void tq_stree_search_kernel(StreeSearchArgs a)
{
    __shared__ unsigned long long s_mat[2 * STREE_SEARCH_LDS_CELLS];
    __shared__ unsigned long long s_good[16], s_bad[16];
    __shared__ int s_s[16];
    __shared__ uint32_t s_inc[64];
    const uint32_t node = blockIdx.x;
    if (node >= (uint32_t)a.n_nodes) return;
    const StreeNode nd = a.nodes[node];
    const uint32_t lane = threadIdx.x & 63u;
    bool cut = false;
    uint32_t bits = 0, rounds = 0;
    if (nd.n >= 4 && nd.n <= STREE_T_MAX) {                                 // the same for every thread of the workgroup
        const uint32_t n = (uint32_t)nd.n, tri = n * (n - 1) / 2;
        const unsigned long long *G = a.mat + nd.toff, *B = a.mat + a.cells + nd.toff;
        int any = 0;
        for (uint32_t c = threadIdx.x; c < tri; c += blockDim.x) any |= B[c] != 0;
        any = __syncthreads_or(any);
        if (any && n == 4) {
            cut = stree_search4((const uint64_t *)G, (const uint64_t *)B, bits);
        } else if (any) {
            if (tri <= (uint32_t)STREE_SEARCH_LDS_CELLS) {
                for (uint32_t c = threadIdx.x; c < tri; c += blockDim.x) {
                    s_mat[c] = G[c];
                    s_mat[tri + c] = B[c];
                }
                __syncthreads();
                G = s_mat;
                B = s_mat + tri;
            }
            const uint64_t ns = a.seeds ? a.seeds[node] : stree_node_seed(a.seed, a.level, node);
            if (n <= 64) stree_block_search<1>(G, B, n, ns, s_good, s_bad, s_s, s_inc, bits, cut, rounds);
            else if (n <= 128) stree_block_search<2>(G, B, n, ns, s_good, s_bad, s_s, s_inc, bits, cut, rounds);
            else if (n <= 256) stree_block_search<4>(G, B, n, ns, s_good, s_bad, s_s, s_inc, bits, cut, rounds);
            else if (n <= 512) stree_block_search<8>(G, B, n, ns, s_good, s_bad, s_s, s_inc, bits, cut, rounds);
            else stree_block_search<16>(G, B, n, ns, s_good, s_bad, s_s, s_inc, bits, cut, rounds);
        }
        if (cut && threadIdx.x < 64u) {
            if (n == 4) {
                if (lane < 4u) a.side[nd.moff + lane] = (uint8_t)((bits >> lane) & 1u);
            } else {
                for (uint32_t j = 0; lane + 64u * j < n; ++j) a.side[nd.moff + lane + 64u * j] = (uint8_t)((bits >> j) & 1u);
            }
        }
    }
    if (threadIdx.x == 0) {
        a.cut[node] = cut ? 1 : 0;
        if (a.rounds) a.rounds[node] = (uint8_t)rounds;
    }
}

// ------------------------------------------------------------------------------------------------------------------
// the driver (host): level loop, search, forest, newick -- once, for both back ends
// ------------------------------------------------------------------------------------------------------------------
struct StreeLevelStat {
    int64_t nodes = 0, live = 0, cells = 0;
    double graph_ms = 0, search_ms = 0, part_ms = 0;
};

struct StreeBackend {
    virtual ~StreeBackend() {}
    // working state := the rows added so far; returns the live quartets at the root
    virtual int begin(int64_t &live, std::string &err) = 0;
    // the level's matrices u64 [2][cells] (G then B), valid until the next call
    virtual int graphs(const std::vector<StreeNode> &nodes, int64_t cells, int level, const uint64_t *&mat,
                       std::string &err) = 0;
    // rule "exact" only: the cut search of the level whose matrices `graphs` just made.  sides[nodes[i].moff + v] = side
    // of taxon v of node i where cuts[i] != 0.  With `exact` set, `graphs` may leave the matrices where this reads them
    // and hand out no host pointer.
    virtual int search(const std::vector<StreeNode> &nodes, int64_t cells, int level, uint64_t seed,
                       std::vector<uint8_t> &sides, std::vector<uint8_t> &cuts, std::string &err) = 0;
    bool exact = false;
    // routes the live quartets through the cuts (children, nA, nB in `nodes`; side and new index in `map`)
    virtual int partition(const std::vector<StreeNode> &nodes, const std::vector<uint32_t> &map, int level, int64_t &live,
                          std::string &err) = 0;
};

inline double stree_ms_since(const std::chrono::steady_clock::time_point &t0)
{
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// the exact search of a level on host matrices (StreeHostBackend, and the device back end's A/B leg)
inline void stree_search_level_host(const std::vector<StreeNode> &nodes, const uint64_t *mat, int64_t cells, int level,
                                    uint64_t seed, std::vector<uint8_t> &sides, std::vector<uint8_t> &cuts)
{
    for (size_t i = 0; i < nodes.size(); ++i) {
        const int n = nodes[i].n;
        cuts[i] = 0;
        if (n < 4) continue;
        int rounds;
        cuts[i] = stree_search_exact(mat + nodes[i].toff, mat + cells + nodes[i].toff, n,
                                     stree_node_seed(seed, (uint64_t)level, (uint64_t)i), &sides[nodes[i].moff], rounds);
    }
}

inline int stree_build(StreeBackend &be, int64_t ntaxa, uint64_t seed, std::string &newick, int64_t &levels,
                       std::vector<StreeLevelStat> &stats, std::string &err)
{
    newick.clear();
    levels = 0;
    stats.clear();
    if (ntaxa == 1) {
        newick = "0;";
        return TQ_OK;
    }
    int64_t live = 0;
    if (int rc = be.begin(live, err)) return rc;
    QmcForest F;
    int32_t next_label = (int32_t)ntaxa;
    std::vector<std::vector<int32_t>> open(1), next;
    open[0].resize((size_t)ntaxa);
    for (int64_t i = 0; i < ntaxa; ++i) open[0][(size_t)i] = (int32_t)i;
    std::vector<std::pair<int32_t, int32_t>> joins;            // the two artificial leaves of every cut
    std::vector<StreeNode> nodes;
    std::vector<uint32_t> map;
    std::vector<double> Gd, Bd;
    std::vector<uint8_t> side, sides, cuts;
    int level = 0;
    while (!open.empty()) {
        const size_t nn = open.size();
        nodes.assign(nn, StreeNode{});
        uint64_t cells = 0, moff = 0;
        for (size_t i = 0; i < nn; ++i) {
            const uint64_t n = open[i].size();
            nodes[i].toff = (uint32_t)cells;
            nodes[i].moff = (uint32_t)moff;
            nodes[i].n = (int32_t)n;
            nodes[i].childA = nodes[i].childB = -1;
            if (n > 3) cells += n * (n - 1) / 2;
            moff += n;
        }
        if (cells > 0xFFFFFFFFull) { err = "a level's matrices exceed 2^32 cells"; return TQ_ERR_INVALID_ARG; }
        StreeLevelStat st;
        st.nodes = (int64_t)nn;
        st.live = live;
        st.cells = (int64_t)cells;
        const uint64_t *mat = nullptr;
        const bool have_graph = live > 0 && cells > 0;
        if (have_graph) {
            const auto t0 = std::chrono::steady_clock::now();
            if (int rc = be.graphs(nodes, (int64_t)cells, level, mat, err)) return rc;
            st.graph_ms = stree_ms_since(t0);
        }
        const auto t1 = std::chrono::steady_clock::now();
        map.assign((size_t)moff, 0);
        next.clear();
        bool any_cut = false;
        if (be.exact && have_graph) {
            sides.assign((size_t)moff, 0);
            cuts.assign(nn, 0);
            if (int rc = be.search(nodes, (int64_t)cells, level, seed, sides, cuts, err)) return rc;
        }
        for (size_t i = 0; i < nn; ++i) {
            const int n = nodes[i].n;
            bool cut = false;
            if (be.exact) {
                if (n > 3 && have_graph && cuts[i]) {
                    cut = true;
                    side.assign(sides.begin() + nodes[i].moff, sides.begin() + nodes[i].moff + n);
                }
            } else if (n > 3 && mat) {
                const uint64_t *G = mat + nodes[i].toff, *B = mat + cells + nodes[i].toff;
                const size_t tri = (size_t)n * (n - 1) / 2;
                uint64_t bsum = 0;
                for (size_t c = 0; c < tri; ++c) bsum += B[c];
                if (bsum) {                                            // every live quartet adds k to two bad cells
                    Gd.assign((size_t)n * n, 0.0);
                    Bd.assign((size_t)n * n, 0.0);
                    size_t c = 0;
                    for (int u = 0; u < n; ++u)
                        for (int v = u + 1; v < n; ++v, ++c) {
                            Gd[(size_t)u * n + v] = Gd[(size_t)v * n + u] = (double)G[c] / 1e5;
                            Bd[(size_t)u * n + v] = Bd[(size_t)v * n + u] = (double)B[c] / 1e5;
                        }
                    QmcRng rng{stree_node_seed(seed, (uint64_t)level, (uint64_t)i)};
                    cut = qmc_search(Gd, Bd, (double)(bsum / 2) / 1e5, n, rng, side);
                }
            }
            if (!cut) {
                qmc_star(F, open[i]);
                continue;
            }
            any_cut = true;
            const int32_t artA = next_label++, artB = next_label++;    // artA stands for side 0, artB for side 1
            std::vector<int32_t> A, Bt;
            for (int j = 0; j < n; ++j) {
                std::vector<int32_t> &dst = side[j] ? Bt : A;
                map[nodes[i].moff + j] = (uint32_t)side[j] << 16 | (uint32_t)dst.size();
                dst.push_back(open[i][j]);
            }
            nodes[i].nA = (uint32_t)A.size();
            nodes[i].nB = (uint32_t)Bt.size();
            A.push_back(artB);
            Bt.push_back(artA);
            nodes[i].childA = (int32_t)next.size();
            next.push_back(std::move(A));
            nodes[i].childB = (int32_t)next.size();
            next.push_back(std::move(Bt));
            joins.emplace_back(artB, artA);
        }
        st.search_ms = stree_ms_since(t1);
        if (any_cut && live > 0) {
            const auto t2 = std::chrono::steady_clock::now();
            if (int rc = be.partition(nodes, map, level, live, err)) return rc;
            st.part_ms = stree_ms_since(t2);
        } else {
            live = 0;
        }
        if ((int)stats.size() < STREE_MAX_LEVELS) stats.push_back(st);
        open.swap(next);
        ++level;
    }
    for (const auto &j : joins) {                                      // each join links the parents of two artificial leaves
        const int32_t la = F.leaf_of[j.first], lb = F.leaf_of[j.second];
        const int32_t pa = F.adj[la][0], pb = F.adj[lb][0];
        F.unlink(la, pa);
        F.unlink(lb, pb);
        F.link(pa, pb);
    }
    levels = level;
    const int32_t root = F.adj[F.leaf_of[0]][0];                       // the node taxon 0 hangs on
    qmc_newick(F, root, -1, newick);
    newick += ';';
    return TQ_OK;
}

// ------------------------------------------------------------------------------------------------------------------
// host back end
// ------------------------------------------------------------------------------------------------------------------
struct StreeHostBackend : StreeBackend {
    const std::vector<uint64_t> *root_t = nullptr, *root_k = nullptr;
    std::vector<uint64_t> t4[2], k[2];
    std::vector<uint32_t> node[2];
    std::vector<uint64_t> mat;
    int64_t n_live = 0;
    int cur = -1;                                                      // -1: the live quartets are the root store

    int begin(int64_t &live, std::string &) override
    {
        cur = -1;
        live = n_live = (int64_t)root_t->size();
        return TQ_OK;
    }
    int graphs(const std::vector<StreeNode> &nodes, int64_t cells, int, const uint64_t *&out, std::string &) override
    {
        mat.assign((size_t)(2 * cells), 0);
        const uint64_t *T4 = cur < 0 ? root_t->data() : t4[cur].data(), *K = cur < 0 ? root_k->data() : k[cur].data();
        const uint32_t *N = cur < 0 ? nullptr : node[cur].data();
        for (int64_t i = 0; i < n_live; ++i) {
            const StreeNode &info = nodes[N ? N[i] : 0];
            if (info.n < 4) continue;
            uint32_t bad[2], good[4];
            stree_cells(T4[i], (uint32_t)info.n, bad, good);
            uint64_t *G = &mat[info.toff], *B = &mat[(size_t)cells + info.toff];
            B[bad[0]] += K[i];
            B[bad[1]] += K[i];
            for (int j = 0; j < 4; ++j) G[good[j]] += K[i];
        }
        out = mat.data();
        return TQ_OK;
    }
    int search(const std::vector<StreeNode> &nodes, int64_t cells, int level, uint64_t seed, std::vector<uint8_t> &sides,
               std::vector<uint8_t> &cuts, std::string &) override
    {
        stree_search_level_host(nodes, mat.data(), cells, level, seed, sides, cuts);
        return TQ_OK;
    }
    int partition(const std::vector<StreeNode> &nodes, const std::vector<uint32_t> &map, int, int64_t &live,
                  std::string &) override
    {
        const uint64_t *T4 = cur < 0 ? root_t->data() : t4[cur].data(), *K = cur < 0 ? root_k->data() : k[cur].data();
        const uint32_t *N = cur < 0 ? nullptr : node[cur].data();
        const int dst = cur < 0 ? 0 : cur ^ 1;
        t4[dst].clear();
        k[dst].clear();
        node[dst].clear();
        for (int64_t i = 0; i < n_live; ++i) {
            uint64_t out4;
            uint32_t child;
            if (!stree_route(nodes[N ? N[i] : 0], map.data(), T4[i], out4, child)) continue;
            t4[dst].push_back(out4);
            k[dst].push_back(K[i]);
            node[dst].push_back(child);
        }
        cur = dst;
        live = n_live = (int64_t)t4[dst].size();
        return TQ_OK;
    }
};

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
//   * The host searches each node's cut (qmc_search of qmc.hpp on cell / 10^5 as doubles, one generator per node keyed
//     by (seed, level, index of the node in its level)).
//   * One pass partitions the live quartets: four taxa on a side -> that child; three -> that child with the odd taxon
//     replaced by the child's artificial taxon; 2 | 2 -> dropped.
//   The level loop, the search, the forest and the newick writer are one piece of host code (`stree_build`) that talks
//   to a back end with two operations, `graphs` and `partition`: StreeHostBackend on host arrays, StreeDevBackend on
//   the device.  Both operations are exact, so the two give the same newick string.
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
    // routes the live quartets through the cuts (children, nA, nB in `nodes`; side and new index in `map`)
    virtual int partition(const std::vector<StreeNode> &nodes, const std::vector<uint32_t> &map, int level, int64_t &live,
                          std::string &err) = 0;
};

inline uint64_t stree_node_seed(uint64_t seed, uint64_t level, uint64_t idx)
{
    QmcRng r{seed ^ (level * 0x9E3779B97F4A7C15ull) ^ (idx * 0xD1B54A32D192ED03ull)};
    return r.next();
}

inline double stree_ms_since(const std::chrono::steady_clock::time_point &t0)
{
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
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
    std::vector<uint8_t> side;
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
        if (live > 0 && cells > 0) {
            const auto t0 = std::chrono::steady_clock::now();
            if (int rc = be.graphs(nodes, (int64_t)cells, level, mat, err)) return rc;
            st.graph_ms = stree_ms_since(t0);
        }
        const auto t1 = std::chrono::steady_clock::now();
        map.assign((size_t)moff, 0);
        next.clear();
        bool any_cut = false;
        for (size_t i = 0; i < nn; ++i) {
            const int n = nodes[i].n;
            bool cut = false;
            if (n > 3 && mat) {
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

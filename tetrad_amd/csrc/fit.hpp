// fit.hpp -- quartet fit of trees against the rows of a supertree accumulator: the weight of the kept quartets a tree
// displays, contradicts and leaves unresolved.  Part of the single translation unit
// tetrad_hip.hip (included inside its anonymous namespace, after concordance.hpp and supertree.hpp).
//
// Rule (one definition, `fit_row`, a host and a device execution of it): with D(x, y) = the depth of the lowest common
// ancestor of tips x and y in the prepared tree (`conc_prepare_tree`), a kept row a,b|c,d has
//   m0 = D(a,b) + D(c,d),  m1 = D(a,c) + D(b,d),  m2 = D(a,d) + D(b,c)
// and is satisfied when m0 is strictly the largest, violated when m1 or m2 is, unresolved when the largest value is
// not unique (the four taxa meet in a polytomy).  This is the four-point condition on unit edge lengths; every value
// is an integer, every sum a u64 sum, so any launch shape and any order give the same six numbers per tree.
//
// Tables: D as u16 [T][T] per tree (depths stay below 2 T <= 2048 on the device, below 65535 on the host).  The host
// uploads only the prepared parent arrays, one record of FIT stride 2 T i32 per tree (the parents of the N <= 2 T - 2
// nodes, N in the last word); `tq_fit_table_kernel` computes the node depths and walks every taxon pair up to its
// meeting node with the parents and depths in LDS.  `fit_host_table` is the same walk on the host.
#pragma once

constexpr int FIT_THREADS = 256;
constexpr int FIT_T_LDS = 128;                  // up to here the table of a tree is copied to LDS: 128 * 128 u16 = 32 KiB
constexpr int FIT_ROWS_PER_BLOCK = 4096;        // rows a workgroup of the fit kernel is sized for
constexpr int FIT_MAX_SLICES = 1024;
constexpr int FIT_MAX_CHUNK_TREES = 65535;      // grid y
constexpr int FIT_TABLE_BLOCKS = 64;            // workgroups per tree of the table kernel, at most
enum { FIT_K_SAT = 0, FIT_K_VIO = 1, FIT_K_UNR = 2, FIT_N_SAT = 3, FIT_N_VIO = 4, FIT_N_UNR = 5, FIT_WORDS = 6 };

// class of one kept row against a table: 0 satisfied, 1 violated, 2 unresolved.  The row's taxa are distinct and < T.
template <class TAB>
__host__ __device__ __forceinline__ int fit_row(const TAB *D, uint32_t T, uint64_t t4)
{
    const uint32_t a = (uint32_t)(t4 & 0xFFFF), b = (uint32_t)((t4 >> 16) & 0xFFFF), c = (uint32_t)((t4 >> 32) & 0xFFFF),
                   d = (uint32_t)(t4 >> 48);
    const uint32_t m0 = (uint32_t)D[a * T + b] + (uint32_t)D[c * T + d];
    const uint32_t m1 = (uint32_t)D[a * T + c] + (uint32_t)D[b * T + d];
    const uint32_t m2 = (uint32_t)D[a * T + d] + (uint32_t)D[b * T + c];
    if (m0 > m1 && m0 > m2) return 0;
    if ((m1 > m0 && m1 > m2) || (m2 > m0 && m2 > m1)) return 1;
    return 2;
}

// pair number i of [0, fit_pairs_span(T)) -> taxa x < y, each pair once: row r = i / (T - 1) shares its T - 1 slots with
// row T - 1 - r (r and T - 1 - r entries above the diagonal).  false: the slot is unused (the middle row of an odd T).
__host__ __device__ __forceinline__ uint32_t fit_pairs_span(uint32_t T) { return ((T + 1) / 2) * (T - 1); }
__host__ __device__ __forceinline__ bool fit_pair(uint32_t i, uint32_t T, uint32_t &x, uint32_t &y)
{
    const uint32_t r = i / (T - 1), j = i - r * (T - 1), own = T - 1 - r;
    if (j < own) {
        x = r;
        y = r + 1 + j;
        return true;
    }
    if (own == r) return false;
    x = own;
    y = T - r + (j - own);
    return true;
}

// depth of the meeting node of tips x != y: both walk up, the deeper one first.  `par` / `dep` of a prepared tree.
template <class PAR, class DEP>
__host__ __device__ __forceinline__ uint32_t fit_meet_depth(const PAR *par, const DEP *dep, uint32_t N, uint32_t x, uint32_t y)
{
    uint32_t u = (uint32_t)par[x], v = (uint32_t)par[y];
    for (uint32_t step = 0; step < 2 * N && u != v; ++step) {      // the bound only guards a record that is no tree
        const uint32_t du = dep[u], dv = dep[v];
        if (du >= dv) u = (uint32_t)par[u];
        if (dv >= du) v = (uint32_t)par[v];
        if (u >= N || v >= N) return 0;
    }
    return dep[u];
}

// the table of one prepared tree on the host; `dep` is scratch
inline void fit_host_table(const std::vector<int32_t> &par, uint32_t T, std::vector<uint32_t> &dep, uint16_t *D)
{
    const uint32_t N = (uint32_t)par.size();
    dep.assign(N, 0);
    for (uint32_t v = T + 1; v < N; ++v) dep[v] = dep[(size_t)par[v]] + 1;     // internal nodes are in BFS order, root = T
    for (uint32_t v = 0; v < T; ++v) dep[v] = dep[(size_t)par[v]] + 1;
    for (uint32_t x = 0; x < T; ++x) D[(size_t)x * T + x] = (uint16_t)dep[x];
    const uint32_t span = fit_pairs_span(T);
    for (uint32_t i = 0; i < span; ++i) {
        uint32_t x, y;
        if (!fit_pair(i, T, x, y)) continue;
        const uint16_t m = (uint16_t)fit_meet_depth(par.data(), dep.data(), N, x, y);
        D[(size_t)x * T + y] = D[(size_t)y * T + x] = m;
    }
}

// the six sums of one tree over host rows
inline void fit_host_rows(const uint16_t *D, uint32_t T, const uint64_t *t4, const uint64_t *k, int64_t n, uint64_t *out)
{
    for (int j = 0; j < FIT_WORDS; ++j) out[j] = 0;
    for (int64_t i = 0; i < n; ++i) {
        const int cls = fit_row(D, T, t4[i]);
        out[FIT_K_SAT + cls] += k[i];
        out[FIT_N_SAT + cls] += 1;
    }
}

// ------------------------------------------------------------------------------------------------------------------
// kernels
// ------------------------------------------------------------------------------------------------------------------
struct FitTableArgs {
    const int32_t *rec;         // [trees][2 T]: parents of the prepared tree, its node count in the last word
    uint16_t *tab;              // [trees][T][T]
    uint32_t T;
};

// grid (workgroups of a tree, trees).  No loop waits on another lane; every loop has a fixed bound.
__global__ __launch_bounds__(FIT_THREADS) void tq_fit_table_kernel(FitTableArgs a)
{
    __shared__ int32_t s_par[2 * STREE_T_MAX];
    __shared__ uint16_t s_dep[2 * STREE_T_MAX];
    const uint32_t T = a.T, S = 2 * T;
    const int32_t *rec = a.rec + (size_t)blockIdx.y * S;
    uint32_t N = (uint32_t)rec[S - 1];
    if (N > S - 1) N = S - 1;                                       // the host never sends this; keeps LDS indices in range
    for (uint32_t v = threadIdx.x; v < N; v += FIT_THREADS) {
        const int32_t p = rec[v];
        s_par[v] = (p >= 0 && (uint32_t)p < N) ? p : (int32_t)T;    // the root's -1: it is never followed (depth 0 ends a walk)
    }
    __syncthreads();
    for (uint32_t v = threadIdx.x; v < N; v += FIT_THREADS) {       // depth = edges up to the root, node T
        uint32_t u = v, d = 0;
        while (u != T && d < N) {
            u = (uint32_t)s_par[u];
            ++d;
        }
        s_dep[v] = (uint16_t)d;
    }
    __syncthreads();
    uint16_t *D = a.tab + (size_t)blockIdx.y * T * T;
    const uint32_t span = fit_pairs_span(T);
    for (uint32_t i = blockIdx.x * FIT_THREADS + threadIdx.x; i < span; i += gridDim.x * FIT_THREADS) {
        uint32_t x, y;
        if (!fit_pair(i, T, x, y)) continue;
        const uint16_t m = (uint16_t)fit_meet_depth(s_par, s_dep, N, x, y);
        D[x * T + y] = m;
        D[y * T + x] = m;
    }
    if (blockIdx.x == 0)
        for (uint32_t x = threadIdx.x; x < T; x += FIT_THREADS) D[x * T + x] = s_dep[x];
}

struct FitArgs {
    const uint64_t *t4, *k;             // the root store
    const unsigned long long *n_rows;   // kept rows, on the device
    const uint16_t *tab;                // [trees][T][T]
    unsigned long long *out;            // [trees][6]
    uint32_t T;
};

__device__ __forceinline__ uint32_t fit_wave_sum32(uint32_t x)
{
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) x += (uint32_t)__shfl_xor((int)x, m);
    return x;
}

// grid (row slices, trees).  LDS_TABLE: the tree's table is copied to LDS (T <= FIT_T_LDS), otherwise read through L2.
template <bool LDS_TABLE>
__global__ __launch_bounds__(FIT_THREADS) void tq_fit_kernel(FitArgs a)
{
    __shared__ uint16_t s_tab[LDS_TABLE ? FIT_T_LDS * FIT_T_LDS : 2];
    __shared__ unsigned long long s_part[FIT_THREADS / 64][FIT_WORDS];
    const uint32_t T = a.T;
    const uint16_t *D = a.tab + (size_t)blockIdx.y * T * T;
    const int64_t n = (int64_t)*a.n_rows;
    const int64_t stride = (int64_t)gridDim.x * FIT_THREADS;
    if ((int64_t)blockIdx.x * FIT_THREADS >= n) return;             // the same for every thread: no barrier is left behind
    if (LDS_TABLE) {
        const uint32_t *src = (const uint32_t *)D;                  // T * T is even (T >= 4); a table starts 4-byte aligned
        uint32_t *dst = (uint32_t *)s_tab;
        for (uint32_t i = threadIdx.x; i < T * T / 2; i += FIT_THREADS) dst[i] = src[i];
        __syncthreads();
    }
    uint64_t ks[3] = {0, 0, 0};
    uint32_t ns[3] = {0, 0, 0};
    for (int64_t i = (int64_t)blockIdx.x * FIT_THREADS + threadIdx.x; i < n; i += stride) {
        const uint64_t t4 = a.t4[i], k = a.k[i];
        const int cls = LDS_TABLE ? fit_row(s_tab, T, t4) : fit_row(D, T, t4);
        ks[0] += cls == 0 ? k : 0;
        ks[1] += cls == 1 ? k : 0;
        ks[2] += cls == 2 ? k : 0;
        ns[0] += cls == 0;
        ns[1] += cls == 1;
        ns[2] += cls == 2;
    }
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const uint64_t sk = stree_wave_sum(ks[j]);
        const uint32_t sn = fit_wave_sum32(ns[j]);
        if (lane == 0) {
            s_part[wave][FIT_K_SAT + j] = sk;
            s_part[wave][FIT_N_SAT + j] = sn;
        }
    }
    __syncthreads();
    if (threadIdx.x < FIT_WORDS) {
        unsigned long long s = 0;
        for (int w = 0; w < FIT_THREADS / 64; ++w) s += s_part[w][threadIdx.x];
        if (s) atomicAdd(&a.out[(size_t)blockIdx.y * FIT_WORDS + threadIdx.x], s);
    }
}

// scf.hpp -- site concordance factors per branch of a fixed tree (sCF / sDF1 / sDF2 / sN of Minh, Hahn & Lanfear 2020),
// accumulated next to the site-pattern class rows (patterns.hpp) on the tree machinery of concordance.hpp.
// Part of the single translation unit tetrad_hip.hip (included inside its anonymous namespace, after concordance.hpp).
//
// Tree: `ConcTree` from `conc_build_tree` -- limits, unrooting, unary suppression, polytomy rule, edge numbering and
// masks are those of concordance.hpp.
//
// Row (one function, `scf_row`, on the host and on the device): a set (a, b, c, d) and the three class counts of its
// class row that support a resolution: n0 = class 3 (0011), n1 = class 6 (0101), n2 = class 8 (0110), by position in
// the row as given.  The geometric half restates `conc_row`'s: the three pair sums give the tree's resolution r, the
// row is induced on an edge iff its internal path is one edge long.  With inf = n0 + n1 + n2:
//   conc = n_r, d1 = n of the lower of the two other indices, d2 = n of the remaining one;
//   inf == 0: the edge's nq_zero += 1 and nothing else;
//   otherwise nq += 1, sum_x += x and fx_x += floor(x * 2^32 / inf) for x = conc, d1, d2 (x < 2^32: x << 32 fits u64).
// Every sum is a u64, so device = host = any order of addition, bit for bit.
//
// Device layout: `tq_scf_kernel` strides over the rows with per-workgroup counters in LDS (u32 row counts, u64 sums),
// the LCA table in LDS up to T = SCF_T_LDS_B and read through L2 above, where the edges are counted in passes of
// SCF_EDGE_TILE.  Each workgroup writes its counters to its own slab; `tq_scf_fold_kernel` adds the slabs in workgroup
// order.  No atomic touches global memory.
#pragma once

constexpr int SCF_THREADS = 256;
constexpr int SCF_EDGE_WORDS = 8;           // per edge, all u64: nq, nq_zero, sum conc / d1 / d2, fx conc / d1 / d2
constexpr int SCF_T_LDS_A = 128;            // LCA table in LDS, small form:  32 KiB table +  7 KiB counters
constexpr int SCF_T_LDS_B = 256;            // LCA table in LDS, large form: 128 KiB table + 14 KiB counters
constexpr int SCF_EDGE_TILE = 2048;         // edges per pass of the global-table form: 112 KiB of counters
constexpr int64_t SCF_ROWS_PER_LAUNCH = CONC_ROWS_PER_LAUNCH;   // keeps the u32 LDS row counts below 2^32
enum { SW_NQ = 0, SW_NQ_ZERO = 1, SW_SUM_CONC = 2, SW_SUM_D1 = 3, SW_SUM_D2 = 4, SW_FX_CONC = 5, SW_FX_D1 = 6, SW_FX_D2 = 7 };

// One row against the tree.  Returns -1 (skipped: taxon >= T or repeated taxon), 0 (induced on no edge) or 1: induced
// on `edge`, with v = {conc, d1, d2, fx_conc, fx_d1, fx_d2}; `zero` says inf == 0 (then v is all zero).
template <class LCA, class DEP, class EID>
__host__ __device__ __forceinline__ int scf_row(const LCA *lca, const DEP *dep, const EID *eid, uint32_t T, uint32_t a,
                                                uint32_t b, uint32_t c, uint32_t d, uint32_t n0, uint32_t n1, uint32_t n2,
                                                int &edge, bool &zero, uint64_t v[6])
{
    if (a >= T || b >= T || c >= T || d >= T) return -1;
    if (a == b || a == c || a == d || b == c || b == d || c == d) return -1;
    const uint32_t lab = lca[a * T + b], lcd = lca[c * T + d], lac = lca[a * T + c], lbd = lca[b * T + d],
                   lad = lca[a * T + d], lbc = lca[b * T + c];
    const int dsum = (int)dep[a] + (int)dep[b] + (int)dep[c] + (int)dep[d];
    const int s0 = dsum - 2 * ((int)dep[lab] + (int)dep[lcd]);
    const int s1 = dsum - 2 * ((int)dep[lac] + (int)dep[lbd]);
    const int s2 = dsum - 2 * ((int)dep[lad] + (int)dep[lbc]);
    int r, l1, l2, smin, sother;
    if (s0 < s1 && s0 < s2) { r = 0; l1 = lab; l2 = lcd; smin = s0; sother = s1; }
    else if (s1 < s0 && s1 < s2) { r = 1; l1 = lac; l2 = lbd; smin = s1; sother = s0; }
    else if (s2 < s0 && s2 < s1) { r = 2; l1 = lad; l2 = lbc; smin = s2; sother = s0; }
    else return 0;                               // star: the four taxa meet at one node
    if (sother - smin != 2) return 0;            // internal path longer than one edge
    edge = (int)eid[dep[l1] > dep[l2] ? l1 : l2];
    if (edge < 0) return 0;
    const uint64_t conc = r == 0 ? n0 : r == 1 ? n1 : n2;
    const uint64_t d1 = r == 0 ? n1 : n0;        // the lower of the two other indices
    const uint64_t d2 = r == 2 ? n1 : n2;        // the remaining one
    const uint64_t inf = (uint64_t)n0 + n1 + n2;
    zero = inf == 0;
    v[0] = conc; v[1] = d1; v[2] = d2;
    v[3] = zero ? 0 : (conc << 32) / inf;
    v[4] = zero ? 0 : (d1 << 32) / inf;
    v[5] = zero ? 0 : (d2 << 32) / inf;
    return 1;
}

struct ScfArgs {
    const uint32_t *sets;       // [n][4]
    const uint32_t *classes;    // [n][16]
    int64_t n;
    const uint16_t *lca, *dep;
    const int32_t *eid;
    int32_t T, N, E;
    int32_t e_lo, e_n;          // edges counted by this pass
    int32_t first;              // 1: this pass also counts the skipped rows
    uint64_t *slab;             // [gridDim.x][words]
    int64_t words;              // 8 E + 1
};

// LDS_TABLE: lca / dep / eid copied to LDS (T <= TMAX); otherwise read from global memory through L2.
// EMAX: edges per pass.
template <bool LDS_TABLE, int TMAX, int EMAX>
__global__ __launch_bounds__(SCF_THREADS) void tq_scf_kernel(ScfArgs a)
{
    __shared__ uint16_t s_lca[LDS_TABLE ? TMAX * TMAX : 1];
    __shared__ uint16_t s_dep[LDS_TABLE ? 2 * TMAX : 1];
    __shared__ int16_t s_eid[LDS_TABLE ? 2 * TMAX : 1];
    __shared__ unsigned long long s_sum[EMAX * 6];
    __shared__ uint32_t s_cnt[EMAX * 2];
    __shared__ uint32_t s_skip;
    const int tid = threadIdx.x;
    const int T = a.T;
    if (LDS_TABLE) {
        const uint32_t *src = (const uint32_t *)a.lca;           // T * T is even (T >= 4)
        uint32_t *dst = (uint32_t *)s_lca;
        for (int i = tid; i < T * T / 2; i += SCF_THREADS) dst[i] = src[i];
        for (int i = tid; i < a.N; i += SCF_THREADS) { s_dep[i] = a.dep[i]; s_eid[i] = (int16_t)a.eid[i]; }
    }
    for (int i = tid; i < a.e_n * 6; i += SCF_THREADS) s_sum[i] = 0;
    for (int i = tid; i < a.e_n * 2; i += SCF_THREADS) s_cnt[i] = 0;
    if (tid == 0) s_skip = 0;
    __syncthreads();
    const uint4 *q4 = (const uint4 *)a.sets;
    const int64_t stride = (int64_t)gridDim.x * SCF_THREADS;
    for (int64_t i = (int64_t)blockIdx.x * SCF_THREADS + tid; i < a.n; i += stride) {
        const uint4 q = q4[i];
        const uint32_t *cl = a.classes + 16 * i;
        const uint32_t n0 = cl[3], n1 = cl[6], n2 = cl[8];      // byte offsets 12, 24 and 32 of the 64-byte row
        int edge = -1;
        bool zero = false;
        uint64_t v[6];
        const int res = LDS_TABLE ? scf_row(s_lca, s_dep, s_eid, (uint32_t)T, q.x, q.y, q.z, q.w, n0, n1, n2, edge, zero, v)
                                  : scf_row(a.lca, a.dep, a.eid, (uint32_t)T, q.x, q.y, q.z, q.w, n0, n1, n2, edge, zero, v);
        if (res < 0) {
            if (a.first) atomicAdd(&s_skip, 1u);
            continue;
        }
        if (res == 0) continue;
        const int le = edge - a.e_lo;
        if (le < 0 || le >= a.e_n) continue;
        if (zero) {
            atomicAdd(&s_cnt[2 * le + SW_NQ_ZERO], 1u);
            continue;
        }
        atomicAdd(&s_cnt[2 * le + SW_NQ], 1u);
#pragma unroll
        for (int k = 0; k < 6; ++k) atomicAdd(&s_sum[6 * le + k], (unsigned long long)v[k]);
    }
    __syncthreads();
    uint64_t *out = a.slab + (int64_t)blockIdx.x * a.words;
    for (int i = tid; i < a.e_n; i += SCF_THREADS) {
        uint64_t *o = out + (int64_t)(a.e_lo + i) * SCF_EDGE_WORDS;
        o[SW_NQ] = s_cnt[2 * i + SW_NQ];
        o[SW_NQ_ZERO] = s_cnt[2 * i + SW_NQ_ZERO];
#pragma unroll
        for (int k = 0; k < 6; ++k) o[SW_SUM_CONC + k] = s_sum[6 * i + k];
    }
    if (a.first && tid == 0) out[(int64_t)a.E * SCF_EDGE_WORDS] = s_skip;
}

// totals[i] += slab[0][i] + slab[1][i] + ... in workgroup order, every word a u64
__global__ __launch_bounds__(SCF_THREADS) void tq_scf_fold_kernel(const uint64_t *slab, int nslab, int64_t words,
                                                                   uint64_t *totals)
{
    const int64_t i = (int64_t)blockIdx.x * SCF_THREADS + threadIdx.x;
    if (i >= words) return;
    uint64_t s = totals[i];
    for (int w = 0; w < nslab; ++w) s += slab[(int64_t)w * words + i];
    totals[i] = s;
}

// Host accumulation on the same row function into tot[8 E + 1].
inline void scf_add_host(const ConcTree &t, const uint32_t *sets, const uint32_t *classes, int64_t n,
                         std::vector<uint64_t> &tot)
{
    for (int64_t i = 0; i < n; ++i) {
        const uint32_t *r = sets + 4 * i, *cl = classes + 16 * i;
        int edge = -1;
        bool zero = false;
        uint64_t v[6];
        const int res = scf_row(t.lca.data(), t.dep.data(), t.eid.data(), (uint32_t)t.T, r[0], r[1], r[2], r[3], cl[3], cl[6],
                                cl[8], edge, zero, v);
        if (res < 0) { tot[(size_t)t.E * SCF_EDGE_WORDS] += 1; continue; }
        if (res == 0) continue;
        uint64_t *e = &tot[(size_t)edge * SCF_EDGE_WORDS];
        if (zero) { e[SW_NQ_ZERO] += 1; continue; }
        e[SW_NQ] += 1;
        for (int k = 0; k < 6; ++k) e[SW_SUM_CONC + k] += v[k];
    }
}

// scf.hpp -- site concordance factors per branch of a fixed tree (sCF / sDF1 / sDF2 / sN of Minh, Hahn & Lanfear 2020),
// accumulated next to the site-pattern class rows (patterns.hpp) on the tree machinery of concordance.hpp.
// Part of the single translation unit tetrad_hip.hip (included inside its anonymous namespace, after concordance.hpp).
//
// Tree: `ConcTree` from `conc_build_tree` -- limits, unrooting, unary suppression, polytomy rule, edge numbering and
// masks are those of concordance.hpp.
//
// Row (one function, `scf_row`, on the host and on the device): a set (a, b, c, d) and the three class counts of its
// class row that support a resolution: n0 = class 3 (0011), n1 = class 6 (0101), n2 = class 8 (0110), by position in
// the row as given.  `conc_geometry` gives the tree's resolution r and the edge the row is induced on.  With
// inf = n0 + n1 + n2:
//   conc = n_r, d1 = n of the lower of the two other indices, d2 = n of the remaining one;
//   inf == 0: the edge's nq_zero += 1 and nothing else;
//   otherwise nq += 1, sum_x += x and fx_x += floor(x * 2^32 / inf) for x = conc, d1, d2 (x < 2^32: x << 32 fits u64).
// Every sum is a u64, so device = host = any order of addition, bit for bit.
//
// Device layout: `tq_scf_kernel` strides over the rows with per-workgroup counters in LDS (u32 row counts, u64 sums),
// the tree tables (`ConcTables`) in LDS up to T = SCF_T_LDS_B and read through L2 above, where the edges are counted in
// passes of SCF_EDGE_TILE.  Each workgroup writes its counters to its own slab; `tq_conc_fold_kernel` adds the slabs in
// workgroup order (no f64 words here).  No atomic touches global memory.
#pragma once

constexpr int SCF_EDGE_WORDS = 8;           // per edge, all u64: nq, nq_zero, sum conc / d1 / d2, fx conc / d1 / d2
constexpr int SCF_T_LDS_A = 128;            // LCA table in LDS, small form:  32 KiB table +  7 KiB counters
constexpr int SCF_T_LDS_B = 256;            // LCA table in LDS, large form: 128 KiB table + 14 KiB counters
constexpr int SCF_EDGE_TILE = 2048;         // edges per pass of the global-table form: 112 KiB of counters
// the launch loop the two accumulators share changes form at the CONC_ values (and takes at most
// CONC_ROWS_PER_LAUNCH rows a launch, which keeps the u32 LDS row counts below 2^32)
static_assert(SCF_T_LDS_A == CONC_T_LDS_A && SCF_T_LDS_B == CONC_T_LDS_B && SCF_EDGE_TILE == CONC_EDGE_TILE, "form sizes");
enum { SW_NQ = 0, SW_NQ_ZERO = 1, SW_SUM_CONC = 2, SW_SUM_D1 = 3, SW_SUM_D2 = 4, SW_FX_CONC = 5, SW_FX_D1 = 6, SW_FX_D2 = 7 };

// One row against the tree.  Returns -1 (skipped: taxon >= T or repeated taxon), 0 (induced on no edge) or 1: induced
// on `edge`, with v = {conc, d1, d2, fx_conc, fx_d1, fx_d2}; `zero` says inf == 0 (then v is all zero).
template <class LCA, class DEP, class EID>
__host__ __device__ __forceinline__ int scf_row(const LCA *lca, const DEP *dep, const EID *eid, uint32_t T, uint32_t a,
                                                uint32_t b, uint32_t c, uint32_t d, uint32_t n0, uint32_t n1, uint32_t n2,
                                                int &edge, bool &zero, uint64_t v[6])
{
    int r = 0;
    const int geo = conc_geometry(lca, dep, eid, T, a, b, c, d, r, edge);
    if (geo <= 0) return geo;
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

// LDS_TABLE, TMAX: see ConcTables.  EMAX: edges per pass.
template <bool LDS_TABLE, int TMAX, int EMAX>
__global__ __launch_bounds__(CONC_THREADS) void tq_scf_kernel(ScfArgs a)
{
    __shared__ ConcTables<LDS_TABLE, TMAX> s_tab;
    __shared__ unsigned long long s_sum[EMAX * 6];
    __shared__ uint32_t s_cnt[EMAX * 2];
    __shared__ uint32_t s_skip;
    const int tid = threadIdx.x;
    const int T = a.T;
    if (LDS_TABLE) s_tab.load(a.lca, a.dep, a.eid, T, a.N);
    for (int i = tid; i < a.e_n * 6; i += CONC_THREADS) s_sum[i] = 0;
    for (int i = tid; i < a.e_n * 2; i += CONC_THREADS) s_cnt[i] = 0;
    if (tid == 0) s_skip = 0;
    __syncthreads();
    const uint4 *q4 = (const uint4 *)a.sets;
    const int64_t stride = (int64_t)gridDim.x * CONC_THREADS;
    for (int64_t i = (int64_t)blockIdx.x * CONC_THREADS + tid; i < a.n; i += stride) {
        const uint4 q = q4[i];
        const uint32_t *cl = a.classes + 16 * i;
        const uint32_t n0 = cl[3], n1 = cl[6], n2 = cl[8];      // byte offsets 12, 24 and 32 of the 64-byte row
        int edge = -1;
        bool zero = false;
        uint64_t v[6];
        const int res = LDS_TABLE
            ? scf_row(s_tab.lca, s_tab.dep, s_tab.eid, (uint32_t)T, q.x, q.y, q.z, q.w, n0, n1, n2, edge, zero, v)
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
    for (int i = tid; i < a.e_n; i += CONC_THREADS) {
        uint64_t *o = out + (int64_t)(a.e_lo + i) * SCF_EDGE_WORDS;
        o[SW_NQ] = s_cnt[2 * i + SW_NQ];
        o[SW_NQ_ZERO] = s_cnt[2 * i + SW_NQ_ZERO];
#pragma unroll
        for (int k = 0; k < 6; ++k) o[SW_SUM_CONC + k] = s_sum[6 * i + k];
    }
    if (a.first && tid == 0) out[(int64_t)a.E * SCF_EDGE_WORDS] = s_skip;
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

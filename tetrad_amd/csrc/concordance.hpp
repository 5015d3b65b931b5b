// concordance.hpp -- quartet concordance statistics on a fixed tree, accumulated next to the resolved rows
// (the counts behind QC / QD / QI / QF of the reference's `tetrad concordance`, tetrad/src/concordance.py).
// Part of the single translation unit tetrad_hip.hip (included inside its anonymous namespace).
//
// Tree (host, once per accumulator): a parent array whose tips 0..T-1 are the taxa is made unrooted the way
// toytree's .unroot() does it (a root of degree 2 is dissolved into one edge) and its unary nodes are suppressed.
// The result is held rooted at a node of degree >= 3, so that every internal non-root node v stands for exactly
// one nontrivial edge (v, parent(v)); that node carries the edge id.  With unit edge lengths the kernel needs
//   lca  u16 [T][T]   the lowest common ancestor of every taxon pair (x on the diagonal),
//   dep  u16 [N]      edges from the root,
//   eid  i32 [N]      edge id of an internal non-root node, -1 elsewhere.
//
// Geometry (`conc_geometry`, on the host and on the device; the row function of scf.hpp calls it): the three pair sums
//   s_r = d(pairing r) with d(x, y) = dep[x] + dep[y] - 2 dep[lca(x, y)]
// give the tree's resolution r of four taxa (four-point condition: the smallest sum; the two others are equal).
// They are induced on an edge iff their internal path is one edge long, (s_other - s_min) / 2 == 1; the edge is
// the deeper of the two LCAs of the winning pairing.  On a polytomy (all three sums equal) they are induced on none.
// Row (one function, `conc_row`, on the host and on the device): the same geometry, written out in place because
// the call measured 1-2 % slower per device add (profiles/concordance/README.md), then the scores.  They are rounded
// to 6 decimals exactly as the TSV reads back (`conc_reread6`, bit-equal to format.hpp's reread6) and sorted
// numerically; weight = (s1 + s2) / 2, score = weight / s0 (0 when s0 == 0).
//
// Device layout: `tq_conc_kernel` strides over the rows with per-workgroup counters in LDS (u32 class counts,
// u64 nsnps sum, f64 weight / score sums, u32 QFc / QFd per taxon), the LCA table in LDS up to T = 256 and read
// through L2 above (`ConcTables`, shared with scf.hpp).  Each workgroup writes its counters to its own slab;
// `tq_conc_fold_kernel` (also the fold of scf.hpp) adds the slabs in fixed workgroup order to the u64 / f64 totals.
// No float atomic touches global memory.
#pragma once

constexpr int CONC_T_MAX = 4096;            // u16 LCA table of T * T entries: 32 MiB at the limit
constexpr int CONC_THREADS = 256;           // of every kernel here and in scf.hpp
constexpr int CONC_T_LDS_A = 128;           // LCA table in LDS, small form:  32 KiB table
constexpr int CONC_T_LDS_B = 256;           // LCA table in LDS, large form: 128 KiB table
constexpr int CONC_EDGE_WORDS = 7;          // per edge: conc, disc1, disc2, nu, nsnps sum (u64), weight sum, score sum (f64)
constexpr int CONC_EDGE_TILE = 2048;        // edges per pass of the global-table kernel (LDS counters of one pass)
constexpr int64_t CONC_ROWS_PER_LAUNCH = int64_t(1) << 31;   // keeps every u32 LDS counter of a workgroup below 2^32
enum { CW_CONC = 0, CW_DISC1 = 1, CW_DISC2 = 2, CW_NU = 3, CW_NSNPS = 4, CW_WEIGHT = 5, CW_SCORE = 6 };

struct ConcTree {
    int32_t T = 0, N = 0, E = 0, W = 0;         // taxa, nodes, nontrivial edges, 64-bit words of a split mask
    std::vector<uint16_t> lca, dep;
    std::vector<int32_t> eid;
    std::vector<uint64_t> masks;                // [E][W] taxa on the child side of each edge
    std::vector<uint64_t> nqrts;                // [E] quartets the edge induces
};

// The preparation every tree goes through (shared with consensus.hpp): a parent array whose tips 0..T-1 are the taxa
// (no children), nodes >= T internal (at least one child), parent[root] = -1, is validated, its unary nodes are
// suppressed and a root of degree 2 is dissolved.  Out: `par` / `nch` of the prepared tree, root = node T, internal
// nodes T..N-1 in BFS order.  Returns an empty string or what is wrong.
inline std::string conc_prepare_tree(const int32_t *parent, int64_t n, int64_t T, std::vector<int32_t> &par,
                                     std::vector<std::vector<int32_t>> &nch)
{
    if (T < 4) return "a tree needs at least 4 taxa";
    if (T > CONC_T_MAX) return "T exceeds the LCA table limit of 4096 taxa";
    if (n < T || n > 64 * CONC_T_MAX) return "node count must be between T and 64 * 4096";
    std::vector<int32_t> nkids(n, 0);
    int64_t root = -1;
    for (int64_t v = 0; v < n; ++v) {
        const int32_t p = parent[v];
        if (p == -1) {
            if (root >= 0) return "more than one root (parent == -1)";
            root = v;
        } else if (p < 0 || p >= n || p == v) {
            return "parent index out of range";
        } else {
            ++nkids[p];
        }
    }
    if (root < 0) return "no root (parent == -1)";
    for (int64_t v = 0; v < n; ++v) {
        if (v < T && nkids[v]) return "a taxon (node < T) has children: taxa must be tips";
        if (v >= T && !nkids[v]) return "a node >= T has no children: every tip must be a taxon";
    }
    std::vector<int32_t> first(n + 1, 0), kids(n > 0 ? n - 1 : 0);
    for (int64_t v = 0; v < n; ++v) first[v + 1] = first[v] + nkids[v];
    std::vector<int32_t> fill(first.begin(), first.end() - 1);
    for (int64_t v = 0; v < n; ++v)
        if (parent[v] >= 0) kids[fill[parent[v]]++] = (int32_t)v;
    std::vector<int32_t> order;                 // BFS from the root: parents before children
    order.reserve(n);
    order.push_back((int32_t)root);
    for (size_t i = 0; i < order.size(); ++i)
        for (int32_t k = first[order[i]]; k < first[order[i] + 1]; ++k) order.push_back(kids[k]);
    if ((int64_t)order.size() != n) return "the parent array has a cycle";
    // suppress unary nodes: rep[v] = the node v stands for; internal nodes of the suppressed tree get ids >= T
    std::vector<int32_t> rep(n, -1);
    std::vector<std::vector<int32_t>> ch;       // children of suppressed internal node T + i
    for (int64_t i = n - 1; i >= 0; --i) {
        const int32_t v = order[i];
        if (v < T) { rep[v] = v; continue; }
        if (nkids[v] == 1) { rep[v] = rep[kids[first[v]]]; continue; }
        std::vector<int32_t> c;
        for (int32_t k = first[v]; k < first[v + 1]; ++k) c.push_back(rep[kids[k]]);
        rep[v] = (int32_t)(T + ch.size());
        ch.push_back(std::move(c));
    }
    int32_t r = rep[root];
    if (r < T) return "the tree has fewer than 4 tips";
    if (ch[r - T].size() == 2) {                // unroot: dissolve the degree-2 root into one edge
        int32_t a = ch[r - T][0], b = ch[r - T][1];
        if (a < T) std::swap(a, b);             // a is internal (both tips would mean T == 2)
        ch[a - T].push_back(b);
        ch[r - T].clear();
        r = a;
    }
    // renumber: root = T, internal nodes in BFS order
    std::vector<int32_t> newid(T + ch.size(), -1), bfs{r};
    for (size_t i = 0; i < bfs.size(); ++i)
        if (bfs[i] >= T)
            for (int32_t c : ch[bfs[i] - T]) bfs.push_back(c);
    int32_t next = (int32_t)T;
    for (int32_t v : bfs) newid[v] = v < T ? v : next++;
    const int32_t N = next;
    par.assign(N, -1);
    nch.assign(N, std::vector<int32_t>());
    for (int32_t v : bfs)
        if (v >= T)
            for (int32_t c : ch[v - T]) { par[newid[c]] = newid[v]; nch[newid[v]].push_back(newid[c]); }
    return std::string();
}

// Tree from a parent array (`conc_prepare_tree`) with the tables of the concordance kernel.  Returns an empty string
// or what is wrong.
inline std::string conc_build_tree(const int32_t *parent, int64_t n, int64_t T, ConcTree &t)
{
    std::vector<int32_t> par;
    std::vector<std::vector<int32_t>> nch;
    const std::string err = conc_prepare_tree(parent, n, T, par, nch);
    if (!err.empty()) return err;
    const int32_t N = (int32_t)par.size();
    t.T = (int32_t)T; t.N = N; t.W = (int32_t)((T + 63) / 64);
    t.dep.assign(N, 0);
    std::vector<int32_t> pre{(int32_t)T}, stack{(int32_t)T};   // preorder: the tips of a subtree are contiguous
    pre.clear();
    while (!stack.empty()) {
        const int32_t v = stack.back();
        stack.pop_back();
        pre.push_back(v);
        for (auto it = nch[v].rbegin(); it != nch[v].rend(); ++it) {
            t.dep[*it] = (uint16_t)(t.dep[v] + 1);
            stack.push_back(*it);
        }
    }
    std::vector<int32_t> lo(N, 0), hi(N, 0), tip_at;
    for (int32_t v : pre)
        if (v < T) { lo[v] = (int32_t)tip_at.size(); tip_at.push_back(v); hi[v] = lo[v] + 1; }
    for (auto it = pre.rbegin(); it != pre.rend(); ++it)
        if (*it >= T) { lo[*it] = lo[nch[*it].front()]; hi[*it] = hi[nch[*it].back()]; }
    t.lca.assign((size_t)T * T, 0);
    for (int32_t x = 0; x < T; ++x) t.lca[(size_t)x * T + x] = (uint16_t)x;
    for (int32_t v = (int32_t)T; v < N; ++v) {
        const auto &c = nch[v];
        for (size_t i = 0; i < c.size(); ++i)
            for (size_t j = i + 1; j < c.size(); ++j)
                for (int32_t p = lo[c[i]]; p < hi[c[i]]; ++p)
                    for (int32_t q = lo[c[j]]; q < hi[c[j]]; ++q) {
                        const int32_t x = tip_at[p], y = tip_at[q];
                        t.lca[(size_t)x * T + y] = t.lca[(size_t)y * T + x] = (uint16_t)v;
                    }
    }
    auto pairsum = [](const std::vector<uint64_t> &s) {
        uint64_t a = 0, b = 0;
        for (uint64_t x : s) { a += x; b += x * x; }
        return (a * a - b) / 2;
    };
    t.eid.assign(N, -1);
    t.E = 0;
    for (int32_t v = (int32_t)T + 1; v < N; ++v) {
        t.eid[v] = t.E++;
        t.masks.resize((size_t)t.E * t.W, 0);
        uint64_t *m = &t.masks[(size_t)(t.E - 1) * t.W];
        for (int32_t p = lo[v]; p < hi[v]; ++p) m[tip_at[p] >> 6] |= uint64_t(1) << (tip_at[p] & 63);
        std::vector<uint64_t> below, above;     // subtrees off v (not through the edge) and off its parent
        for (int32_t c : nch[v]) below.push_back((uint64_t)(hi[c] - lo[c]));
        const int32_t u = par[v];
        for (int32_t c : nch[u])
            if (c != v) above.push_back((uint64_t)(hi[c] - lo[c]));
        if (par[u] >= 0) above.push_back((uint64_t)(T - (hi[u] - lo[u])));
        t.nqrts.push_back(pairsum(below) * pairsum(above));
    }
    return std::string();
}

// The double that "%.6f" text of x reads back as (format.hpp's reread6), without text: the integer nearest to the
// exact x * 10^6 (ties to even, as glibc's printf rounds the exact binary value), divided by 10^6 -- one correctly
// rounded division, which is what strtod returns for that decimal string.  x * 10^6 = p + err exactly (fma), so
// the tie decision is exact for |x| < 9e9 (product below 2^53); beyond that (and for NaN / inf) x is returned.
__host__ __device__ __forceinline__ double conc_reread6(double x)
{
    const double ax = fabs(x);
    if (!(ax < 9.0e9)) return x;
    const double p = ax * 1e6;
    const double err = fma(ax, 1e6, -p);
    const double n = floor(p);
    const double t = (p - n) - 0.5;           // exact whenever it matters (p - n >= 0.25, or p a multiple of 0.5)
    bool up = t > -err;
    if (t == -err) up = (n - 2.0 * floor(n * 0.5)) != 0.0;     // exact tie: to even
    const double v = (n + (up ? 1.0 : 0.0)) / 1e6;
    return x < 0 ? -v : v;
}

// Four taxa against the tree.  Returns -1 (a taxon >= T or a repeated taxon), 0 (induced on no edge) or 1: the tree
// resolves them as pairing `r` (0 = ab|cd, 1 = ac|bd, 2 = ad|bc) and they are induced on edge `edge`.  What a new
// statistic on a fixed tree calls; `conc_row` below holds the same lines in place (see the head of this file).
template <class LCA, class DEP, class EID>
__host__ __device__ __forceinline__ int conc_geometry(const LCA *lca, const DEP *dep, const EID *eid, uint32_t T, uint32_t a,
                                                      uint32_t b, uint32_t c, uint32_t d, int &r, int &edge)
{
    if (a >= T || b >= T || c >= T || d >= T) return -1;
    if (a == b || a == c || a == d || b == c || b == d || c == d) return -1;
    const uint32_t lab = lca[a * T + b], lcd = lca[c * T + d], lac = lca[a * T + c], lbd = lca[b * T + d],
                   lad = lca[a * T + d], lbc = lca[b * T + c];
    const int dsum = (int)dep[a] + (int)dep[b] + (int)dep[c] + (int)dep[d];
    const int s0 = dsum - 2 * ((int)dep[lab] + (int)dep[lcd]);
    const int s1 = dsum - 2 * ((int)dep[lac] + (int)dep[lbd]);
    const int s2 = dsum - 2 * ((int)dep[lad] + (int)dep[lbc]);
    int l1, l2, smin, sother;
    if (s0 < s1 && s0 < s2) { r = 0; l1 = lab; l2 = lcd; smin = s0; sother = s1; }
    else if (s1 < s0 && s1 < s2) { r = 1; l1 = lac; l2 = lbd; smin = s1; sother = s0; }
    else if (s2 < s0 && s2 < s1) { r = 2; l1 = lad; l2 = lbc; smin = s2; sother = s0; }
    else return 0;                               // star: the four taxa meet at one node
    if (sother - smin != 2) return 0;            // internal path longer than one edge
    edge = (int)eid[dep[l1] > dep[l2] ? l1 : l2];
    return 1;
}

// One row against the tree.  Returns -1 (not counted: taxon >= T, repeated taxon, topology > 2, or flags
// TQ_FLAG_BAD_INDEX / TQ_FLAG_INVALID_DIAGNOSTIC), 0 (induced on no edge) or 1: induced on edge `edge`, counted
// in class `cls` (CW_CONC / CW_DISC1 / CW_DISC2 / CW_NU) with its weight and score.  `min_snps` >= 1.
template <class LCA, class DEP, class EID>
__host__ __device__ __forceinline__ int conc_row(const LCA *lca, const DEP *dep, const EID *eid, uint32_t T,
                                                 uint32_t min_snps, double min_ratio, uint32_t a, uint32_t b, uint32_t c,
                                                 uint32_t d, uint32_t topo, uint32_t nsnps, double x0, double x1, double x2,
                                                 uint32_t flags, int &edge, int &cls, double &weight, double &score)
{
    if ((flags & (4u | 16u)) || a >= T || b >= T || c >= T || d >= T || topo > 2u) return -1;
    if (a == b || a == c || a == d || b == c || b == d || c == d) return -1;
    const uint32_t lab = lca[a * T + b], lcd = lca[c * T + d], lac = lca[a * T + c], lbd = lca[b * T + d],
                   lad = lca[a * T + d], lbc = lca[b * T + c];
    const int da = dep[a], db = dep[b], dc = dep[c], dd = dep[d];
    const int s0 = da + db + dc + dd - 2 * ((int)dep[lab] + (int)dep[lcd]);
    const int s1 = da + db + dc + dd - 2 * ((int)dep[lac] + (int)dep[lbd]);
    const int s2 = da + db + dc + dd - 2 * ((int)dep[lad] + (int)dep[lbc]);
    int r, l1, l2, smin, sother;
    if (s0 < s1 && s0 < s2) { r = 0; l1 = lab; l2 = lcd; smin = s0; sother = s1; }
    else if (s1 < s0 && s1 < s2) { r = 1; l1 = lac; l2 = lbd; smin = s1; sother = s0; }
    else if (s2 < s0 && s2 < s1) { r = 2; l1 = lad; l2 = lbc; smin = s2; sother = s0; }
    else return 0;                               // star: the four taxa meet at one node
    if (sother - smin != 2) return 0;            // internal path longer than one edge
    edge = (int)eid[dep[l1] > dep[l2] ? l1 : l2];
    // scores as the TSV reads back, sorted numerically (deviation 1 of DESIGN section 11)
    double y0 = conc_reread6(x0), y1 = conc_reread6(x1), y2 = conc_reread6(x2), tmp;
    if (y0 > y1) { tmp = y0; y0 = y1; y1 = tmp; }
    if (y1 > y2) { tmp = y1; y1 = y2; y2 = tmp; }
    if (y0 > y1) { tmp = y0; y0 = y1; y1 = tmp; }
    weight = (y1 + y2) / 2.0;
    score = y0 == 0.0 ? 0.0 : weight / y0;
    if (score < min_ratio || nsnps < min_snps) { cls = CW_NU; return 1; }
    if ((int)topo == r) { cls = CW_CONC; return 1; }
    const int lower = r == 0 ? 1 : 0;            // the lower of the two other topology indices
    cls = (int)topo == lower ? CW_DISC1 : CW_DISC2;
    return 1;
}

struct ConcArgs {
    const uint32_t *q;          // [n][4]
    const uint32_t *rstat;      // [n][2]
    const double *rscor;        // [n][3]
    const uint8_t *flags;       // [n] or null
    int64_t n;
    const uint16_t *lca, *dep;
    const int32_t *eid;
    int32_t T, N, E;
    uint32_t min_snps;
    double min_ratio;
    int32_t e_lo, e_n;          // edges counted by this pass
    int32_t tips;               // 1: this pass also counts QFc / QFd and the skipped rows
    uint64_t *slab;             // [gridDim.x][words]
    int64_t words;              // 7 E + 2 T + 1
};

// The tree tables of a workgroup: with LDS_TABLE, lca / dep / eid copied to LDS (T <= TMAX); otherwise nothing, and
// the kernel reads them from global memory through L2.  Declared `__shared__` by tq_conc_kernel and tq_scf_kernel.
template <bool LDS_TABLE, int TMAX>
struct ConcTables {
    uint16_t lca[LDS_TABLE ? TMAX * TMAX : 1];
    uint16_t dep[LDS_TABLE ? 2 * TMAX : 1];
    int16_t eid[LDS_TABLE ? 2 * TMAX : 1];
    // every thread of the workgroup calls it; the caller's __syncthreads() follows
    __device__ __forceinline__ void load(const uint16_t *g_lca, const uint16_t *g_dep, const int32_t *g_eid, int T, int N)
    {
        const int tid = threadIdx.x;
        const uint32_t *src = (const uint32_t *)g_lca;           // T * T is even (T >= 4)
        uint32_t *dst = (uint32_t *)lca;
        for (int i = tid; i < T * T / 2; i += CONC_THREADS) dst[i] = src[i];
        for (int i = tid; i < N; i += CONC_THREADS) { dep[i] = g_dep[i]; eid[i] = (int16_t)g_eid[i]; }
    }
};

// LDS_TABLE, TMAX: see ConcTables.
// EMAX: edges per pass; QF counters for TMAX taxa.
template <bool LDS_TABLE, int TMAX, int EMAX>
__global__ __launch_bounds__(CONC_THREADS) void tq_conc_kernel(ConcArgs a)
{
    __shared__ ConcTables<LDS_TABLE, TMAX> s_tab;
    __shared__ uint32_t s_cnt[EMAX * 4];
    __shared__ unsigned long long s_nsn[EMAX];
    __shared__ double s_ws[EMAX * 2];
    __shared__ uint32_t s_qf[TMAX * 2];
    __shared__ uint32_t s_skip;
    const int tid = threadIdx.x;
    const int T = a.T;
    if (LDS_TABLE) s_tab.load(a.lca, a.dep, a.eid, T, a.N);
    for (int i = tid; i < a.e_n * 4; i += CONC_THREADS) s_cnt[i] = 0;
    for (int i = tid; i < a.e_n; i += CONC_THREADS) { s_nsn[i] = 0; s_ws[2 * i] = 0.0; s_ws[2 * i + 1] = 0.0; }
    for (int i = tid; i < 2 * T; i += CONC_THREADS) s_qf[i] = 0;
    if (tid == 0) s_skip = 0;
    __syncthreads();
    const uint4 *q4 = (const uint4 *)a.q;
    const uint2 *st2 = (const uint2 *)a.rstat;
    const int64_t stride = (int64_t)gridDim.x * CONC_THREADS;
    for (int64_t i = (int64_t)blockIdx.x * CONC_THREADS + tid; i < a.n; i += stride) {
        const uint4 q = q4[i];
        const uint2 st = st2[i];
        const double x0 = a.rscor[3 * i], x1 = a.rscor[3 * i + 1], x2 = a.rscor[3 * i + 2];
        const uint32_t fl = a.flags ? a.flags[i] : 0u;
        int edge = -1, cls = 0;
        double w = 0.0, s = 0.0;
        const int res = LDS_TABLE
            ? conc_row(s_tab.lca, s_tab.dep, s_tab.eid, (uint32_t)T, a.min_snps, a.min_ratio, q.x, q.y, q.z, q.w, st.x, st.y,
                       x0, x1, x2, fl, edge, cls, w, s)
            : conc_row(a.lca, a.dep, a.eid, (uint32_t)T, a.min_snps, a.min_ratio, q.x, q.y, q.z, q.w, st.x, st.y, x0, x1,
                       x2, fl, edge, cls, w, s);
        if (res < 0) {
            if (a.tips) atomicAdd(&s_skip, 1u);
            continue;
        }
        if (res == 0) continue;
        const int le = edge - a.e_lo;
        if (le >= 0 && le < a.e_n) {
            atomicAdd(&s_cnt[le * 4 + cls], 1u);
            atomicAdd(&s_nsn[le], (unsigned long long)st.y);
            atomicAdd(&s_ws[2 * le], w);
            atomicAdd(&s_ws[2 * le + 1], s);
        }
        if (a.tips && cls != CW_NU) {
            const int k = cls == CW_CONC ? 0 : 1;
            atomicAdd(&s_qf[2 * q.x + k], 1u);
            atomicAdd(&s_qf[2 * q.y + k], 1u);
            atomicAdd(&s_qf[2 * q.z + k], 1u);
            atomicAdd(&s_qf[2 * q.w + k], 1u);
        }
    }
    __syncthreads();
    uint64_t *out = a.slab + (int64_t)blockIdx.x * a.words;
    for (int i = tid; i < a.e_n; i += CONC_THREADS) {
        uint64_t *o = out + (int64_t)(a.e_lo + i) * CONC_EDGE_WORDS;
        o[CW_CONC] = s_cnt[4 * i + CW_CONC];
        o[CW_DISC1] = s_cnt[4 * i + CW_DISC1];
        o[CW_DISC2] = s_cnt[4 * i + CW_DISC2];
        o[CW_NU] = s_cnt[4 * i + CW_NU];
        o[CW_NSNPS] = s_nsn[i];
        o[CW_WEIGHT] = (uint64_t)__double_as_longlong(s_ws[2 * i]);
        o[CW_SCORE] = (uint64_t)__double_as_longlong(s_ws[2 * i + 1]);
    }
    if (a.tips) {
        uint64_t *o = out + (int64_t)a.E * CONC_EDGE_WORDS;
        for (int i = tid; i < 2 * T; i += CONC_THREADS) o[i] = s_qf[i];
        if (tid == 0) o[2 * T] = s_skip;
    }
}

// totals[i] += slab[0][i] + slab[1][i] + ... in workgroup order: f64 for the weight / score words of the first
// `f64_edges` records of CONC_EDGE_WORDS words (the concordance edges; scf.hpp passes 0), u64 otherwise
__global__ __launch_bounds__(CONC_THREADS) void tq_conc_fold_kernel(const uint64_t *slab, int nslab, int64_t words,
                                                                    int32_t f64_edges, uint64_t *totals)
{
    const int64_t i = (int64_t)blockIdx.x * CONC_THREADS + threadIdx.x;
    if (i >= words) return;
    const bool is_f64 = i < (int64_t)f64_edges * CONC_EDGE_WORDS && (i % CONC_EDGE_WORDS) >= CW_WEIGHT;
    if (is_f64) {
        double s = __longlong_as_double((long long)totals[i]);
        for (int w = 0; w < nslab; ++w) s += __longlong_as_double((long long)slab[(int64_t)w * words + i]);
        totals[i] = (uint64_t)__double_as_longlong(s);
    } else {
        uint64_t s = totals[i];
        for (int w = 0; w < nslab; ++w) s += slab[(int64_t)w * words + i];
        totals[i] = s;
    }
}

// Host accumulation on the same row function: integer words in `ti`, weight / score sums in `tf` (row order).
inline void conc_add_host(const ConcTree &t, uint32_t min_snps, double min_ratio, const uint32_t *q, const uint32_t *rstat,
                          const double *rscor, const uint8_t *flags, int64_t n, std::vector<uint64_t> &ti,
                          std::vector<double> &tf)
{
    const int64_t tips = (int64_t)t.E * CONC_EDGE_WORDS;
    for (int64_t i = 0; i < n; ++i) {
        int edge = -1, cls = 0;
        double w = 0.0, s = 0.0;
        const uint32_t *r = q + 4 * i;
        const int res = conc_row(t.lca.data(), t.dep.data(), t.eid.data(), (uint32_t)t.T, min_snps, min_ratio, r[0], r[1],
                                 r[2], r[3], rstat[2 * i], rstat[2 * i + 1], rscor[3 * i], rscor[3 * i + 1],
                                 rscor[3 * i + 2], flags ? flags[i] : 0u, edge, cls, w, s);
        if (res < 0) { ti[tips + 2 * t.T] += 1; continue; }
        if (res == 0) continue;
        uint64_t *e = &ti[(int64_t)edge * CONC_EDGE_WORDS];
        e[cls] += 1;
        e[CW_NSNPS] += rstat[2 * i + 1];
        tf[(int64_t)edge * CONC_EDGE_WORDS + CW_WEIGHT] += w;
        tf[(int64_t)edge * CONC_EDGE_WORDS + CW_SCORE] += s;
        if (cls != CW_NU)
            for (int k = 0; k < 4; ++k) ti[tips + 2 * r[k] + (cls == CW_CONC ? 0 : 1)] += 1;
    }
}

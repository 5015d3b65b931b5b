// nni.hpp -- nearest-neighbour interchanges of a tree scored on the quartet fit, every move in one pass over the kept
// rows of a supertree accumulator, and the local search built on that pass.  Part of the single
// translation unit tetrad_hip.hip (included inside its anonymous namespace, after fit.hpp).
//
// Tree: a parent array made ready by `conc_prepare_tree` and then put in canonical form (`nni_canonical`): the prepared
// rooting, the children of every node ordered by their smallest taxon, internal nodes T..N-1 in BFS order, root = T.
// Edge e = v - T - 1 is the edge above internal non-root node v; with u = parent(v) it is eligible when v has two
// children and u three neighbours.  Its corners: X1, X2 below the children of v, Y1, Y2 the two other subtrees at u,
// within a side the corner with the smaller smallest taxon first.
//
// Rule (one definition, `nni_row`, a host and a device execution of it): with L(x, y) = the lowest common ancestor
// node of tips x and y and dep = node depths, the geometry of `conc_geometry` (six lookups, the pairing whose LCA
// depths sum strictly highest, an internal path of one edge, v = the deeper LCA of that pairing) says whether a kept
// row a,b|c,d has one taxon in every corner of an edge.  Then k goes to w[e][0] when the tree pairs a with b.  Otherwise
// a and b sit on different sides, and two more lookups against the edge's record place them: a taxon x below v is in
// X1 iff L(x, rx) != v for the record's taxon rx of X1; a taxon z beyond u is in the corner of the record's taxon ry
// (the sibling of v) iff dep[L(z, ry)] > dep[u].  Equal corner numbers give w[e][1], unequal ones w[e][2].  Every value
// is an integer and every sum a u64 sum, so any launch shape and any row order give the same numbers.
#pragma once

constexpr int NNI_THREADS = 256;
constexpr int NNI_T_LDS = 128;                  // up to here the LCA table is copied to LDS: 128 * 128 u16 = 32 KiB
constexpr int NNI_ROWS_PER_BLOCK = 4096;        // rows a workgroup of the scan kernel is sized for
constexpr int NNI_MAX_SLICES = 1024;
constexpr int NNI_TABLE_BLOCKS = 64;            // workgroups of the table kernel, at most
constexpr int64_t NNI_MAX_ROUNDS = 65536;
// edge record: bits 0-15 a taxon of X1, bits 16-31 a taxon of the sibling's corner, then the two flags
constexpr uint64_t NNI_REC_ELIGIBLE = uint64_t(1) << 32, NNI_REC_SIB_Y2 = uint64_t(1) << 33;

// One kept row against the tree.  true: its taxa lie one in each corner of eligible edge `edge`, and it displays the
// edge's current split (cls 0), alternative 1 (X1 Y1 | X2 Y2) or alternative 2 (X1 Y2 | X2 Y1).  The row's taxa are
// distinct and < T; `L` holds nodes < N, `dep` N depths, `rec` E records.
template <class TAB, class DEP>
__host__ __device__ __forceinline__ bool nni_row(const TAB *L, const DEP *dep, const uint64_t *rec, uint32_t T, uint32_t E,
                                                 uint64_t t4, uint32_t &edge, uint32_t &cls)
{
    const uint32_t a = (uint32_t)(t4 & 0xFFFF), b = (uint32_t)((t4 >> 16) & 0xFFFF), c = (uint32_t)((t4 >> 32) & 0xFFFF),
                   d = (uint32_t)(t4 >> 48);
    const uint32_t lab = L[a * T + b], lcd = L[c * T + d], lac = L[a * T + c], lbd = L[b * T + d], lad = L[a * T + d],
                   lbc = L[b * T + c];
    const uint32_t m0 = (uint32_t)dep[lab] + (uint32_t)dep[lcd];
    const uint32_t m1 = (uint32_t)dep[lac] + (uint32_t)dep[lbd];
    const uint32_t m2 = (uint32_t)dep[lad] + (uint32_t)dep[lbc];
    uint32_t r, l1, l2, top, other;             // the tree's pairing, its two LCAs (l1 is a's), its sum and another one
    if (m0 > m1 && m0 > m2) { r = 0; l1 = lab; l2 = lcd; top = m0; other = m1; }
    else if (m1 > m0 && m1 > m2) { r = 1; l1 = lac; l2 = lbd; top = m1; other = m0; }
    else if (m2 > m0 && m2 > m1) { r = 2; l1 = lad; l2 = lbc; top = m2; other = m0; }
    else return false;                          // the four taxa meet at one node
    if (top - other != 1) return false;         // internal path longer than one edge
    const bool a_below = (uint32_t)dep[l1] > (uint32_t)dep[l2];
    const uint32_t v = a_below ? l1 : l2;
    const uint32_t e = v - T - 1;               // v is internal and no root; anything else wraps past E
    if (e >= E) return false;
    const uint64_t rc = rec[e];
    if (!(rc & NNI_REC_ELIGIBLE)) return false;
    edge = e;
    if (r == 0) {
        cls = 0;
        return true;
    }
    const uint32_t x = a_below ? a : b, z = a_below ? b : a;        // of a and b: the one below v, the one beyond u
    const uint32_t rx = (uint32_t)(rc & 0xFFFF), ry = (uint32_t)((rc >> 16) & 0xFFFF);
    const uint32_t i = (uint32_t)L[x * T + rx] != v ? 0u : 1u;
    const uint32_t sib = (rc & NNI_REC_SIB_Y2) ? 1u : 0u;
    const uint32_t j = (uint32_t)dep[L[z * T + ry]] >= (uint32_t)dep[v] ? sib : sib ^ 1u;
    cls = i == j ? 1u : 2u;
    return true;
}

// meeting node of tips x != y: both walk up, the deeper one first (`fit_meet_depth`, returning the node)
template <class PAR, class DEP>
__host__ __device__ __forceinline__ uint32_t nni_meet_node(const PAR *par, const DEP *dep, uint32_t N, uint32_t T, uint32_t x,
                                                           uint32_t y)
{
    uint32_t u = (uint32_t)par[x], v = (uint32_t)par[y];
    for (uint32_t step = 0; step < 2 * N && u != v; ++step) {      // the bound only guards a record that is no tree
        const uint32_t du = dep[u], dv = dep[v];
        if (du >= dv) u = (uint32_t)par[u];
        if (dv >= du) v = (uint32_t)par[v];
        if (u >= N || v >= N) return T;
    }
    return u == v ? u : T;
}

// ------------------------------------------------------------------------------------------------------------------
// host: the canonical tree, its edges, the move selection and application, the newick -- once, for both back ends
// ------------------------------------------------------------------------------------------------------------------
struct NniTree {
    int32_t T = 0, N = 0, E = 0, W = 0;
    std::vector<int32_t> par, mintax;           // [N]
    std::vector<std::vector<int32_t>> nch;      // children, by smallest taxon
    std::vector<int32_t> lo, hi, tip_at;        // preorder: the tips of a subtree are tip_at[lo .. hi)
    std::vector<int32_t> up_min;                // [N] smallest taxon not below the node (T for the root)
    // per edge
    std::vector<uint8_t> elig;
    std::vector<uint64_t> rec;
    std::vector<int32_t> corner;                // [E][4] nodes of X1, X2, Y1, Y2; -1 = everything not below u
};

// `par` / `nch` of any rooted tree on tips 0..T-1 whose root is `root` -> canonical numbering in `t.par` / `t.nch`,
// with the preorder intervals, the smallest taxa and the edges
inline void nni_canonical(const std::vector<std::vector<int32_t>> &nch_in, int32_t root, int32_t T, NniTree &t)
{
    const int32_t N = (int32_t)nch_in.size();
    std::vector<int32_t> order{root}, mt(N, 0);
    order.reserve(N);
    for (size_t i = 0; i < order.size(); ++i)
        for (int32_t c : nch_in[order[i]]) order.push_back(c);
    for (auto it = order.rbegin(); it != order.rend(); ++it) {
        const int32_t v = *it;
        if (v < T) { mt[v] = v; continue; }
        int32_t m = T;
        for (int32_t c : nch_in[v]) m = std::min(m, mt[c]);
        mt[v] = m;
    }
    std::vector<int32_t> bfs{root}, newid(N, -1);
    bfs.reserve(N);
    std::vector<int32_t> kids;
    for (size_t i = 0; i < bfs.size(); ++i) {
        kids = nch_in[bfs[i]];
        std::sort(kids.begin(), kids.end(), [&](int32_t p, int32_t q) { return mt[p] < mt[q]; });
        for (int32_t c : kids) bfs.push_back(c);
    }
    int32_t next = T;
    for (int32_t v : bfs) newid[v] = v < T ? v : next++;
    t.T = T; t.N = N; t.E = N - T - 1; t.W = (T + 63) / 64;
    t.par.assign(N, -1);
    t.mintax.assign(N, 0);
    t.nch.assign(N, std::vector<int32_t>());
    for (int32_t v : bfs) {
        t.mintax[newid[v]] = mt[v];
        if (v < T) continue;
        kids = nch_in[v];
        std::sort(kids.begin(), kids.end(), [&](int32_t p, int32_t q) { return mt[p] < mt[q]; });
        for (int32_t c : kids) { t.par[newid[c]] = newid[v]; t.nch[newid[v]].push_back(newid[c]); }
    }
    // preorder intervals
    t.lo.assign(N, 0); t.hi.assign(N, 0); t.tip_at.clear();
    std::vector<int32_t> pre, stack{T};
    pre.reserve(N);
    while (!stack.empty()) {
        const int32_t v = stack.back();
        stack.pop_back();
        pre.push_back(v);
        for (auto it = t.nch[v].rbegin(); it != t.nch[v].rend(); ++it) stack.push_back(*it);
    }
    for (int32_t v : pre)
        if (v < T) { t.lo[v] = (int32_t)t.tip_at.size(); t.tip_at.push_back(v); t.hi[v] = t.lo[v] + 1; }
    for (auto it = pre.rbegin(); it != pre.rend(); ++it)
        if (*it >= T) { t.lo[*it] = t.lo[t.nch[*it].front()]; t.hi[*it] = t.hi[t.nch[*it].back()]; }
    std::vector<int32_t> pmin(T + 1, T), smin(T + 1, T);           // smallest taxon of tip_at[0 .. i) and of tip_at[i .. T)
    for (int32_t i = 0; i < T; ++i) pmin[i + 1] = std::min(pmin[i], t.tip_at[i]);
    for (int32_t i = T - 1; i >= 0; --i) smin[i] = std::min(smin[i + 1], t.tip_at[i]);
    t.up_min.assign(N, T);
    for (int32_t v = 0; v < N; ++v) t.up_min[v] = std::min(pmin[t.lo[v]], smin[t.hi[v]]);
    // edges
    const int32_t E = t.E;
    t.elig.assign(E, 0);
    t.rec.assign(E, 0);
    t.corner.assign((size_t)E * 4, -1);
    for (int32_t e = 0; e < E; ++e) {
        const int32_t v = T + 1 + e, u = t.par[v];
        const bool u_root = t.par[u] < 0;
        if (t.nch[v].size() != 2 || t.nch[u].size() != (u_root ? 3u : 2u)) continue;
        int32_t *c = &t.corner[(size_t)e * 4];
        c[0] = t.nch[v][0];
        c[1] = t.nch[v][1];
        int32_t sib = -1, k = 2;
        for (int32_t s : t.nch[u])
            if (s != v) { c[k++] = s; if (sib < 0) sib = s; }      // a root: the two others, already in order
        bool sib_y2 = false;
        if (!u_root) {
            c[3] = -1;
            if (t.up_min[u] < t.mintax[sib]) { c[2] = -1; c[3] = sib; sib_y2 = true; }
        }
        t.elig[e] = 1;
        t.rec[e] = (uint64_t)t.mintax[c[0]] | (uint64_t)t.mintax[sib] << 16 | NNI_REC_ELIGIBLE | (sib_y2 ? NNI_REC_SIB_Y2 : 0);
    }
}

// the canonical tree of a parent array: empty string, or what is wrong with it (the words of `conc_prepare_tree`)
inline std::string nni_prepare(const int32_t *parent, int64_t n, int64_t T, NniTree &t)
{
    std::vector<int32_t> par;
    std::vector<std::vector<int32_t>> nch;
    const std::string err = conc_prepare_tree(parent, n, T, par, nch);
    if (!err.empty()) return err;
    if ((int64_t)par.size() > 2 * T - 2) return "internal error: a prepared tree of T taxa has at most 2 T - 2 nodes";
    nni_canonical(nch, (int32_t)T, (int32_t)T, t);
    return std::string();
}

// corner masks u64[E][4][W] of the canonical tree (zeros where an edge is not eligible)
inline void nni_corner_masks(const NniTree &t, uint64_t *out)
{
    const int32_t W = t.W;
    memset(out, 0, (size_t)t.E * 4 * W * 8);
    for (int32_t e = 0; e < t.E; ++e) {
        if (!t.elig[e]) continue;
        const int32_t u = t.par[t.T + 1 + e];
        for (int j = 0; j < 4; ++j) {
            uint64_t *m = out + ((size_t)e * 4 + j) * W;
            const int32_t c = t.corner[(size_t)e * 4 + j];
            if (c >= 0) {
                for (int32_t p = t.lo[c]; p < t.hi[c]; ++p) m[t.tip_at[p] >> 6] |= uint64_t(1) << (t.tip_at[p] & 63);
            } else {
                for (int32_t p = 0; p < t.lo[u]; ++p) m[t.tip_at[p] >> 6] |= uint64_t(1) << (t.tip_at[p] & 63);
                for (int32_t p = t.hi[u]; p < t.T; ++p) m[t.tip_at[p] >> 6] |= uint64_t(1) << (t.tip_at[p] & 63);
            }
        }
    }
}

// the LCA-node table and the depths of the canonical tree on the host: every pair once, from the preorder intervals
inline void nni_host_table(const NniTree &t, std::vector<uint16_t> &L, std::vector<uint16_t> &dep)
{
    const int32_t T = t.T, N = t.N;
    L.assign((size_t)T * T, 0);
    dep.assign(N, 0);
    for (int32_t v = T + 1; v < N; ++v) dep[v] = (uint16_t)(dep[t.par[v]] + 1);    // BFS order: the parent comes first
    for (int32_t x = 0; x < T; ++x) {
        dep[x] = (uint16_t)(dep[t.par[x]] + 1);
        L[(size_t)x * T + x] = (uint16_t)x;
    }
    for (int32_t v = T; v < N; ++v) {
        const auto &c = t.nch[v];
        for (size_t i = 0; i < c.size(); ++i)
            for (size_t j = i + 1; j < c.size(); ++j)
                for (int32_t p = t.lo[c[i]]; p < t.hi[c[i]]; ++p)
                    for (int32_t q = t.lo[c[j]]; q < t.hi[c[j]]; ++q) {
                        const int32_t x = t.tip_at[p], y = t.tip_at[q];
                        L[(size_t)x * T + y] = L[(size_t)y * T + x] = (uint16_t)v;
                    }
    }
}

// the 3 E sums of the canonical tree over host rows
inline void nni_host_rows(const NniTree &t, const uint64_t *t4, const uint64_t *k, int64_t n, std::vector<uint64_t> &w)
{
    w.assign((size_t)t.E * 3, 0);
    if (t.E == 0 || n == 0) return;
    std::vector<uint16_t> L, dep;
    nni_host_table(t, L, dep);
    for (int64_t i = 0; i < n; ++i) {
        uint32_t e, cls;
        if (nni_row(L.data(), dep.data(), t.rec.data(), (uint32_t)t.T, (uint32_t)t.E, t4[i], e, cls))
            w[(size_t)e * 3 + cls] += k[i];
    }
}

// One round on the sums `w` of the canonical tree `t`: the candidates, the accepted moves applied to the tree (which is
// put back in canonical form).  Returns the moves applied; `gain` = the sum of their gains.
inline int64_t nni_round(NniTree &t, const std::vector<uint64_t> &w, uint64_t &gain)
{
    struct Cand { uint64_t gain; int32_t e; int alt; };
    std::vector<Cand> cand;
    for (int32_t e = 0; e < t.E; ++e) {
        if (!t.elig[e]) continue;
        const uint64_t w0 = w[(size_t)e * 3], w1 = w[(size_t)e * 3 + 1], w2 = w[(size_t)e * 3 + 2];
        const int alt = w2 > w1 ? 2 : 1;
        const uint64_t wa = alt == 1 ? w1 : w2;
        if (wa > w0) cand.push_back({wa - w0, e, alt});
    }
    gain = 0;
    if (cand.empty()) return 0;
    std::sort(cand.begin(), cand.end(),
              [](const Cand &p, const Cand &q) { return p.gain != q.gain ? p.gain > q.gain : p.e < q.e; });
    std::vector<uint8_t> used(t.N, 0);
    std::vector<std::vector<int32_t>> nch = t.nch;
    auto exchange = [&](int32_t v, int32_t cv, int32_t u, int32_t cu) {        // child cv of v <-> child cu of u
        *std::find(nch[v].begin(), nch[v].end(), cv) = cu;
        *std::find(nch[u].begin(), nch[u].end(), cu) = cv;
    };
    int64_t moves = 0;
    for (const Cand &c : cand) {
        const int32_t v = t.T + 1 + c.e, u = t.par[v];
        if (used[u] || used[v]) continue;
        used[u] = used[v] = 1;
        const int32_t *cn = &t.corner[(size_t)c.e * 4];
        const int32_t target = cn[c.alt == 1 ? 2 : 3], rest = cn[c.alt == 1 ? 3 : 2];
        if (target >= 0) exchange(v, cn[1], u, target);                         // X2 <-> the Y corner it joins X1's partner for
        else exchange(v, cn[0], u, rest);                                       // that corner is "up": X1 <-> the sibling instead
        gain += c.gain;
        ++moves;
    }
    NniTree next;
    nni_canonical(nch, t.T, t.T, next);
    t = std::move(next);
    return moves;
}

inline void nni_newick_node(const NniTree &t, int32_t v, std::string &out)
{
    if (v < t.T) {
        out += std::to_string(v);
        return;
    }
    out += '(';
    for (size_t i = 0; i < t.nch[v].size(); ++i) {
        if (i) out += ',';
        nni_newick_node(t, t.nch[v][i], out);
    }
    out += ')';
}

// newick of the canonical tree: numeric tips, children by smallest taxon
inline std::string nni_newick(const NniTree &t)
{
    std::string out;
    nni_newick_node(t, t.T, out);
    out += ';';
    return out;
}

// ------------------------------------------------------------------------------------------------------------------
// kernels
// ------------------------------------------------------------------------------------------------------------------
struct NniTableArgs {
    const int32_t *rec;         // [2 T]: parents of the canonical tree, its node count in the last word
    uint16_t *tab;              // [T][T] LCA nodes, then [2 T] node depths
    uint32_t T;
};

// grid (workgroups).  `tq_fit_table_kernel` for one tree, keeping the meeting node of every pair and the depths.
// No loop waits on another lane; every loop has a fixed bound.
__global__ __launch_bounds__(NNI_THREADS) void tq_nni_table_kernel(NniTableArgs a)
{
    __shared__ int32_t s_par[2 * STREE_T_MAX];
    __shared__ uint16_t s_dep[2 * STREE_T_MAX];
    const uint32_t T = a.T, S = 2 * T;
    uint32_t N = (uint32_t)a.rec[S - 1];
    if (N > S - 1) N = S - 1;                                       // the host never sends this; keeps LDS indices in range
    for (uint32_t v = threadIdx.x; v < N; v += NNI_THREADS) {
        const int32_t p = a.rec[v];
        s_par[v] = (p >= 0 && (uint32_t)p < N) ? p : (int32_t)T;    // the root's -1: it is never followed (depth 0 ends a walk)
    }
    __syncthreads();
    for (uint32_t v = threadIdx.x; v < N; v += NNI_THREADS) {       // depth = edges up to the root, node T
        uint32_t u = v, d = 0;
        while (u != T && d < N) {
            u = (uint32_t)s_par[u];
            ++d;
        }
        s_dep[v] = (uint16_t)d;
    }
    __syncthreads();
    uint16_t *L = a.tab;
    const uint32_t span = fit_pairs_span(T);
    for (uint32_t i = blockIdx.x * NNI_THREADS + threadIdx.x; i < span; i += gridDim.x * NNI_THREADS) {
        uint32_t x, y;
        if (!fit_pair(i, T, x, y)) continue;
        const uint16_t m = (uint16_t)nni_meet_node(s_par, s_dep, N, T, x, y);
        L[x * T + y] = m;
        L[y * T + x] = m;
    }
    if (blockIdx.x == 0) {
        for (uint32_t x = threadIdx.x; x < T; x += NNI_THREADS) L[x * T + x] = (uint16_t)x;
        uint16_t *dep = a.tab + (size_t)T * T;
        for (uint32_t v = threadIdx.x; v < S; v += NNI_THREADS) dep[v] = v < N ? s_dep[v] : (uint16_t)0;
    }
}

struct NniArgs {
    const uint64_t *t4, *k;             // the root store
    const unsigned long long *n_rows;   // kept rows, on the device
    const uint16_t *tab;                // [T][T] LCA nodes, then [2 T] depths
    const uint64_t *rec;                // [E] edge records
    unsigned long long *w;              // [E][3]
    uint32_t T, N, E;
};

// grid (row slices).  LDS_TABLE: the LCA table is copied to LDS (T <= NNI_T_LDS), otherwise read through L2.  Depths,
// edge records and the 3 E sums of the workgroup are in LDS either way.  No loop waits on another lane or workgroup;
// every loop has a fixed bound.
template <bool LDS_TABLE>
__global__ __launch_bounds__(NNI_THREADS) void tq_nni_kernel(NniArgs a)
{
    constexpr int TMAX = LDS_TABLE ? NNI_T_LDS : STREE_T_MAX;
    constexpr int EMAX = TMAX - 3;
    __shared__ uint16_t s_tab[LDS_TABLE ? NNI_T_LDS * NNI_T_LDS : 2];
    __shared__ uint16_t s_dep[2 * TMAX];
    __shared__ uint64_t s_rec[EMAX];
    __shared__ unsigned long long s_w[3 * EMAX];
    const uint32_t T = a.T;
    const uint32_t N = a.N < 2u * TMAX ? a.N : 2u * TMAX, E = a.E < (uint32_t)EMAX ? a.E : (uint32_t)EMAX;
    const int64_t n = (int64_t)*a.n_rows;
    const int64_t stride = (int64_t)gridDim.x * NNI_THREADS;
    if ((int64_t)blockIdx.x * NNI_THREADS >= n) return;             // the same for every thread: no barrier is left behind
    if (LDS_TABLE) {
        // whole u32 words, rounded up: `nni_row` reads the diagonal too, and for an odd T its last entry L[T-1][T-1] is
        // the low half of the last word (the high half is dep[0], inside the buffer; s_tab has room: T * T < 128 * 128)
        const uint32_t *src = (const uint32_t *)a.tab;
        uint32_t *dst = (uint32_t *)s_tab;
        for (uint32_t i = threadIdx.x; i < (T * T + 1) / 2; i += NNI_THREADS) dst[i] = src[i];
    }
    const uint16_t *g_dep = a.tab + (size_t)T * T;
    for (uint32_t i = threadIdx.x; i < N; i += NNI_THREADS) s_dep[i] = g_dep[i];
    for (uint32_t i = threadIdx.x; i < E; i += NNI_THREADS) s_rec[i] = a.rec[i];
    for (uint32_t i = threadIdx.x; i < 3 * E; i += NNI_THREADS) s_w[i] = 0;
    __syncthreads();
    for (int64_t i = (int64_t)blockIdx.x * NNI_THREADS + threadIdx.x; i < n; i += stride) {
        const uint64_t t4 = a.t4[i];
        uint32_t e, cls;
        const bool hit = LDS_TABLE ? nni_row(s_tab, s_dep, s_rec, T, E, t4, e, cls)
                                   : nni_row(a.tab, s_dep, s_rec, T, E, t4, e, cls);
        if (hit) atomicAdd(&s_w[3 * e + cls], (unsigned long long)a.k[i]);
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < 3 * E; i += NNI_THREADS) {
        const unsigned long long s = s_w[i];
        if (s) atomicAdd(&a.w[i], s);
    }
}

// consensus.hpp -- exact split counts over many trees and the majority-rule consensus built from them (what the
// reference's `tetrad consensus` gets from toytree).
// Part of the single translation unit tetrad_hip.hip (included inside its anonymous namespace).
//
// One rule, executed on the host and on the device:
//   tree    a parent array (tips 0..T-1 = the taxa) goes through `conc_prepare_tree` (validated, unary nodes suppressed,
//           a root of degree 2 dissolved), so that every internal non-root node stands for one edge.  `cons_prepare`
//           then numbers the internal nodes by height (a tip has height 0, a node 1 + its highest child) and writes one
//           flat i32 record: node count, height count, the first node of every height, a child list.
//   mask    of a node = the OR of its children's masks, u64 words, bit x of word x / 64 = taxon x; heights bottom-up.
//   split   the canonical side is the one without taxon 0: a mask with bit 0 set is complemented under the T-bit tail
//           mask.  Sides of fewer than 2 or more than T - 2 taxa (tips, the root) are no splits.
//   count   one per tree and split, after a comparison of the full mask.  Integers only.
//
// Device layout (all of it allocated at create): a chunk of prepared trees is staged through a page-locked buffer;
//   tq_cons_mask_kernel    one workgroup per tree: heights bottom-up with a workgroup barrier between them, threads over
//                          (node of the height, word); then every mask is made canonical, and its key (a 64-bit hash cut
//                          to `cons_hash_bits`, CONS_EMPTY for a side that is no split) is written beside it.
//   tq_cons_insert_kernel  open addressing keyed by the hash: one 64-bit compare-and-swap per probed slot, no retry on a
//                          foreign key (the probe moves on).  The claimer draws the entry index with an integer atomic add
//                          and stores its mask as the entry's representative.
//   tq_cons_count_kernel   (after the insert kernel has finished) finds each split's entry again and compares all W words
//                          with the representative: equal -> integer atomic add on the entry's count; different -> a true
//                          collision, the split goes to the unresolved list, which has room for every split of the chunk.
//   tq_cons_gather_kernel  packs the unresolved masks for the host, which counts them in the map of the host back end.
// No loop of these kernels waits for another lane or workgroup: every probe loop is bounded by the slot count.  A count
// only goes up behind a full-mask match, so the hash decides where the time goes and never what the result is.
#pragma once

constexpr int CONS_T_MAX = CONC_T_MAX;
constexpr int CONS_THREADS = 256;
constexpr uint64_t CONS_EMPTY = ~uint64_t(0);
constexpr int64_t CONS_CHUNK_MAX = 65536;           // trees per chunk at most
constexpr int64_t CONS_GATHER_BYTES = int64_t(4) << 20;   // unresolved masks fetched per round
enum { CONS_CTR_CLAIMS = 0, CONS_CTR_OVERFLOW = 1, CONS_CTR_UNRES = 2, CONS_CTR_WORDS = 4 };

// record of one prepared tree, i32 words: [0] M internal nodes, [1] H heights, [4 ..] first node of height 1..H and the
// end (H + 1 words), [4 + T ..] first child of node 0..M-1 and the end, [4 + 2T ..] children: a taxon, or T + node
__host__ __device__ constexpr int64_t cons_stride(int64_t T) { return 4 * T + 4; }

__host__ __device__ __forceinline__ uint64_t cons_mix(uint64_t x)
{
    x ^= x >> 33; x *= 0xff51afd7ed558ccdull;
    x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ull;
    return x ^ (x >> 33);
}

// the hash of a mask is the (wrapping) sum of these over its words, so it can be summed across lanes in any order
__host__ __device__ __forceinline__ uint64_t cons_word_hash(uint64_t word, int w)
{
    return cons_mix(word + (uint64_t)(w + 1) * 0x9e3779b97f4a7c15ull);
}

__host__ __device__ __forceinline__ uint64_t cons_key(uint64_t hash_sum, int bits)
{
    uint64_t k = cons_mix(hash_sum);
    if (bits < 64) k &= (uint64_t(1) << bits) - 1;
    return k == CONS_EMPTY ? k - 1 : k;
}

__host__ __device__ __forceinline__ uint64_t cons_slot(uint64_t key) { return cons_mix(key ^ 0x9e3779b97f4a7c15ull); }

// Prepared record of one tree (cons_stride(T) words at `out`).  Returns an empty string or what is wrong.
inline std::string cons_prepare(const int32_t *parent, int64_t n, int64_t T, int32_t *out)
{
    std::vector<int32_t> par;
    std::vector<std::vector<int32_t>> nch;
    const std::string err = conc_prepare_tree(parent, n, T, par, nch);
    if (!err.empty()) return err;
    const int32_t N = (int32_t)par.size(), M = N - (int32_t)T;
    if (M < 1 || M > T - 2) return "internal error: a prepared tree of T taxa has 1..T-2 internal nodes";
    std::vector<int32_t> height(N, 0);
    int32_t H = 0;
    for (int32_t v = N - 1; v >= T; --v) {      // BFS numbering: the children of v have larger numbers
        int32_t h = 0;
        for (int32_t c : nch[v]) h = std::max(h, height[c]);
        height[v] = h + 1;
        H = std::max(H, h + 1);
    }
    int32_t *hstart = out + 4, *kstart = out + 4 + T, *kids = out + 4 + 2 * T;
    out[0] = M; out[1] = H; out[2] = 0; out[3] = 0;
    for (int32_t h = 0; h <= H; ++h) hstart[h] = 0;
    for (int32_t v = (int32_t)T; v < N; ++v) ++hstart[height[v]];       // hstart[h] = nodes of height h (h >= 1)
    int32_t run = 0;
    for (int32_t h = 1; h <= H; ++h) { const int32_t c = hstart[h]; hstart[h - 1] = run; run += c; }
    hstart[H] = run;                            // now hstart[h - 1] .. hstart[h] = the nodes of height h
    std::vector<int32_t> at(hstart, hstart + H), id(N, -1);
    for (int32_t v = (int32_t)T; v < N; ++v) id[v] = at[height[v] - 1]++;
    std::vector<int32_t> old(M);
    for (int32_t v = (int32_t)T; v < N; ++v) old[id[v]] = v;
    int32_t k = 0;
    for (int32_t i = 0; i < M; ++i) {
        kstart[i] = k;
        for (int32_t c : nch[old[i]]) kids[k++] = c < T ? c : (int32_t)T + id[c];
    }
    kstart[M] = k;
    return std::string();
}

// The canonical nontrivial sides of one prepared tree, appended to `out` ([.][W]); `tmp` is scratch.
inline void cons_host_splits(const int32_t *rec, int32_t T, int32_t W, std::vector<uint64_t> &tmp, std::vector<uint64_t> &out)
{
    const int32_t M = rec[0];
    const int32_t *kstart = rec + 4 + T, *kids = rec + 4 + 2 * T;
    const uint64_t tail = (T & 63) ? (uint64_t(1) << (T & 63)) - 1 : ~uint64_t(0);
    tmp.assign((size_t)M * W, 0);
    for (int32_t v = 0; v < M; ++v) {           // height order: children first
        uint64_t *m = &tmp[(size_t)v * W];
        for (int32_t k = kstart[v]; k < kstart[v + 1]; ++k) {
            const int32_t c = kids[k];
            if (c < T) {
                m[c >> 6] |= uint64_t(1) << (c & 63);
            } else {
                const uint64_t *s = &tmp[(size_t)(c - T) * W];
                for (int32_t w = 0; w < W; ++w) m[w] |= s[w];
            }
        }
    }
    for (int32_t v = 0; v < M; ++v) {
        uint64_t *m = &tmp[(size_t)v * W];
        if (m[0] & 1) {
            for (int32_t w = 0; w < W; ++w) m[w] = ~m[w];
            m[W - 1] &= tail;
        }
        int pc = 0;
        for (int32_t w = 0; w < W; ++w) pc += __builtin_popcountll(m[w]);
        if (pc >= 2 && pc <= T - 2) out.insert(out.end(), m, m + W);
    }
}

struct ConsVecHash {
    size_t operator()(const std::vector<uint64_t> &m) const
    {
        uint64_t s = 0;
        for (size_t w = 0; w < m.size(); ++w) s += cons_word_hash(m[w], (int)w);
        return (size_t)cons_mix(s);
    }
};
using ConsMap = std::unordered_map<std::vector<uint64_t>, int64_t, ConsVecHash>;

// a < b as one big integer, word W - 1 most significant
inline bool cons_mask_less(const uint64_t *a, const uint64_t *b, int32_t W)
{
    for (int32_t w = W - 1; w >= 0; --w)
        if (a[w] != b[w]) return a[w] < b[w];
    return false;
}

// The map as the canonical table: count descending, then the mask ascending.
inline void cons_sorted_table(const ConsMap &map, int32_t W, std::vector<uint64_t> &masks, std::vector<int64_t> &counts)
{
    std::vector<const ConsMap::value_type *> rows;
    rows.reserve(map.size());
    for (const auto &kv : map) rows.push_back(&kv);
    std::sort(rows.begin(), rows.end(), [W](const ConsMap::value_type *a, const ConsMap::value_type *b) {
        if (a->second != b->second) return a->second > b->second;
        return cons_mask_less(a->first.data(), b->first.data(), W);
    });
    masks.resize(rows.size() * (size_t)W);
    counts.resize(rows.size());
    for (size_t i = 0; i < rows.size(); ++i) {
        std::copy(rows[i]->first.begin(), rows[i]->first.end(), masks.begin() + i * (size_t)W);
        counts[i] = rows[i]->second;
    }
}

// Two canonical sides are compatible iff they are disjoint or one contains the other.
inline bool cons_compatible(const uint64_t *a, const uint64_t *b, int32_t W)
{
    bool meet = false, a_only = false, b_only = false;
    for (int32_t w = 0; w < W; ++w) {
        meet |= (a[w] & b[w]) != 0;
        a_only |= (a[w] & ~b[w]) != 0;
        b_only |= (b[w] & ~a[w]) != 0;
        if (meet && a_only && b_only) return false;
    }
    return true;
}

// Consensus newick of a canonical table: splits accepted greedily in table order (count >= min_count, compatible with
// every accepted one); the root holds the maximal sides and the uncovered tips, children ordered by their smallest
// taxon, every accepted side labelled with its integer percent (200 count + ntrees) / (2 ntrees).
inline std::string cons_newick(const std::vector<uint64_t> &masks, const std::vector<int64_t> &counts, int32_t T, int32_t W,
                               int64_t ntrees, int64_t min_count)
{
    std::vector<int64_t> acc;                   // accepted rows
    for (size_t i = 0; i < counts.size(); ++i) {
        if (counts[i] < min_count) break;       // the table is sorted by count
        bool ok = true;
        for (size_t j = 0; j < acc.size() && ok; ++j) ok = cons_compatible(&masks[i * W], &masks[acc[j] * (size_t)W], W);
        if (ok) acc.push_back((int64_t)i);
    }
    const int32_t A = (int32_t)acc.size();
    std::vector<int32_t> size(A), low(A), order(A);
    for (int32_t s = 0; s < A; ++s) {
        const uint64_t *m = &masks[acc[s] * (size_t)W];
        int pc = 0, lo = -1;
        for (int32_t w = 0; w < W; ++w) {
            pc += __builtin_popcountll(m[w]);
            if (lo < 0 && m[w]) lo = 64 * w + __builtin_ctzll(m[w]);
        }
        size[s] = pc; low[s] = lo; order[s] = s;
    }
    // a nested family: walking it from the largest side down, the owner of a side's taxa is its parent
    std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return size[a] > size[b]; });
    std::vector<int32_t> owner(T, -1), up(A, -1);
    for (int32_t s : order) {
        const uint64_t *m = &masks[acc[s] * (size_t)W];
        up[s] = owner[low[s]];
        for (int32_t w = 0; w < W; ++w)
            for (uint64_t x = m[w]; x; x &= x - 1) owner[64 * w + __builtin_ctzll(x)] = s;
    }
    // children of node s (index A = the root): (smallest taxon, child) with child = taxon, or T + side
    std::vector<std::vector<std::pair<int32_t, int32_t>>> kids(A + 1);
    for (int32_t s = 0; s < A; ++s) kids[up[s] < 0 ? A : up[s]].push_back({low[s], T + s});
    for (int32_t x = 0; x < T; ++x) kids[owner[x] < 0 ? A : owner[x]].push_back({x, x});
    for (auto &k : kids) std::sort(k.begin(), k.end());
    std::string out;
    std::vector<std::pair<int32_t, size_t>> stack{{A, 0}};      // (node, next child)
    out += '(';
    while (!stack.empty()) {
        auto &top = stack.back();
        const int32_t s = top.first;
        if (top.second == kids[s].size()) {
            out += ')';
            if (s < A && ntrees > 0) out += std::to_string((200 * counts[acc[s]] + ntrees) / (2 * ntrees));
            stack.pop_back();
            continue;
        }
        if (top.second) out += ',';
        const int32_t c = kids[s][top.second++].second;
        if (c < T) {
            out += std::to_string(c);
        } else {
            out += '(';
            stack.push_back({c - T, 0});
        }
    }
    out += ';';
    return out;
}

// ---------------------------------------------------------------------------------------------
// Device path
// ---------------------------------------------------------------------------------------------
struct ConsArgs {
    const int32_t *trees;       // [chunk][cons_stride(T)] prepared records
    uint64_t *masks;            // [chunk][T - 2][W]
    uint64_t *keys;             // [chunk][T - 2]
    int64_t items;              // chunk trees x (T - 2)
    int32_t T, W, G;            // G = lanes that share a mask: the power of two >= W
    int32_t hash_bits;
    uint64_t tail;              // valid bits of word W - 1
    // the table
    unsigned long long *slot_key;   // [slots] CONS_EMPTY or a key
    int32_t *slot_idx;          // [slots] entry of the slot's key, -1 until claimed within max_splits
    uint64_t *rep;              // [max_splits][W] representative mask of an entry
    unsigned long long *count;  // [max_splits]
    unsigned int *ctr;          // CONS_CTR_*
    uint32_t *unres;            // [chunk x (T - 2)] items whose mask differs from their entry's representative
    int64_t slot_mask;          // slots - 1 (a power of two)
    int64_t max_splits;
};

__global__ __launch_bounds__(CONS_THREADS) void tq_cons_mask_kernel(ConsArgs a)
{
    const int tid = threadIdx.x;
    const int T = a.T, W = a.W, G = a.G, Mmax = T - 2;
    const int32_t *rec = a.trees + (int64_t)blockIdx.x * cons_stride(T);
    const int M = rec[0], H = rec[1];
    const int32_t *hstart = rec + 4, *kstart = rec + 4 + T, *kids = rec + 4 + 2 * T;
    uint64_t *m = a.masks + (int64_t)blockIdx.x * Mmax * W;
    for (int h = 1; h <= H; ++h) {              // a node of height h has only lower children: no atomics
        const int lo = hstart[h - 1], n = (hstart[h] - lo) * W;
        for (int i = tid; i < n; i += CONS_THREADS) {
            const int v = lo + i / W, w = i % W;
            uint64_t x = 0;
            for (int k = kstart[v]; k < kstart[v + 1]; ++k) {
                const int c = kids[k];
                if (c < T) x |= (c >> 6) == w ? uint64_t(1) << (c & 63) : uint64_t(0);
                else x |= m[(int64_t)(c - T) * W + w];
            }
            m[(int64_t)v * W + w] = x;
        }
        __syncthreads();
    }
    // canonical side, size, key: G lanes share a node, lane l holds word l (every thread walks the same trip count)
    uint64_t *keys = a.keys + (int64_t)blockIdx.x * Mmax;
    const int per = CONS_THREADS / G, g = tid / G, l = tid % G;
    for (int base = 0; base < Mmax; base += per) {
        const int v = base + g;
        const bool on = v < M && l < W;
        uint64_t x = on ? m[(int64_t)v * W + l] : uint64_t(0);
        const bool flip = (__shfl(x, 0, G) & 1) != 0;
        if (on && flip) x = ~x & (l == W - 1 ? a.tail : ~uint64_t(0));
        int pc = __popcll(x);
        uint64_t hs = on ? cons_word_hash(x, l) : uint64_t(0);
        for (int o = G >> 1; o > 0; o >>= 1) {
            pc += __shfl_xor(pc, o, G);
            hs += __shfl_xor(hs, o, G);
        }
        if (on && flip) m[(int64_t)v * W + l] = x;
        if (l == 0 && v < Mmax) keys[v] = (v < M && pc >= 2 && pc <= T - 2) ? cons_key(hs, a.hash_bits) : CONS_EMPTY;
    }
}

// G lanes per item (tree, node); lane 0 of the group claims, the group stores the representative
__global__ __launch_bounds__(CONS_THREADS) void tq_cons_insert_kernel(ConsArgs a)
{
    const int G = a.G, l = threadIdx.x % G;
    const int64_t item = ((int64_t)blockIdx.x * CONS_THREADS + threadIdx.x) / G;
    const uint64_t key = item < a.items ? a.keys[item] : CONS_EMPTY;
    int32_t idx = -1;
    if (l == 0 && key != CONS_EMPTY) {
        uint64_t s = cons_slot(key) & (uint64_t)a.slot_mask;
        bool placed = false;
        for (int64_t p = 0; p <= a.slot_mask && !placed; ++p) {
            const unsigned long long old = atomicCAS(&a.slot_key[s], (unsigned long long)CONS_EMPTY, (unsigned long long)key);
            if (old == CONS_EMPTY) {            // claimed: this mask becomes the entry's representative
                const unsigned int e = atomicAdd(&a.ctr[CONS_CTR_CLAIMS], 1u);
                if ((int64_t)e < a.max_splits) {
                    idx = (int32_t)e;
                    a.slot_idx[s] = idx;
                } else {
                    a.ctr[CONS_CTR_OVERFLOW] = 1u;
                }
                placed = true;
            } else if (old == key) {
                placed = true;
            }
            s = (s + 1) & (uint64_t)a.slot_mask;
        }
        if (!placed) a.ctr[CONS_CTR_OVERFLOW] = 1u;     // every slot holds another key
    }
    idx = __shfl(idx, 0, G);
    if (idx >= 0 && l < a.W) a.rep[(int64_t)idx * a.W + l] = a.masks[item * a.W + l];
}

__global__ __launch_bounds__(CONS_THREADS) void tq_cons_count_kernel(ConsArgs a)
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
    if (l == 0 && key != CONS_EMPTY) {
        if (idx < 0) {
            a.ctr[CONS_CTR_OVERFLOW] = 1u;      // its key found no entry: more distinct splits than max_splits
        } else if (same) {
            atomicAdd(&a.count[idx], 1ull);
        } else {
            const unsigned int u = atomicAdd(&a.ctr[CONS_CTR_UNRES], 1u);
            a.unres[u] = (uint32_t)item;
        }
    }
}

// out[e][w] = masks[unres[first + e]][w] for e < n
__global__ __launch_bounds__(CONS_THREADS) void tq_cons_gather_kernel(const uint32_t *unres, int64_t first, int64_t n,
                                                                      const uint64_t *masks, int32_t W, uint64_t *out)
{
    const int64_t i = (int64_t)blockIdx.x * CONS_THREADS + threadIdx.x;
    if (i >= n * W) return;
    const int64_t e = i / W, w = i % W;
    out[i] = masks[(int64_t)unres[first + e] * W + w];
}

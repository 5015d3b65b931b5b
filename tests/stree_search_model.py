"""The exact cut search of the supertree in plain Python integers, which cannot wrap.  Written
from the rule's statement, not from the C++: it is the definition that the host execution (`tq_stree_search(NULL, ...)`)
and the device execution (`tq_stree_search_kernel`) are compared with, as bootstrap_stream_model.py is for the device
stream.  Also the graphs the CPU and the GPU test share."""
import ctypes

import numpy as np

M64 = (1 << 64) - 1
GAMMA = 0x9E3779B97F4A7C15
SUM_LIMIT = 1501199875790166            # smallest sum of k with 6 * sum >= 2^53


def mix(z):
    z &= M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def rng_next(state):
    """QmcRng: (new state, output)"""
    state = (state + GAMMA) & M64
    return state, mix(state)


def node_seed(seed, level, index):
    return rng_next((seed ^ (level * 0x9E3779B97F4A7C15) ^ (index * 0xD1B54A32D192ED03)) & M64)[1]


def start_seed(ns, r, s):
    return rng_next(ns ^ (((32 * r + s + 1) * 0xD6E8FEB86659FD93) & M64))[1]


def draw(state0, v):
    """draw v of QmcRng{state0} = its (v + 1)-th next()"""
    return mix(state0 + (v + 1) * GAMMA)


def better(x, y):
    l, r = x[0] * y[1], y[0] * x[1]
    return l > r if l != r else x[0] > y[0]


def full(tri, n):
    """upper triangle (row by row) -> symmetric u64 matrix"""
    M = np.zeros((n, n), np.uint64)
    M[np.triu_indices(n, 1)] = np.asarray(tri, np.uint64)
    return M + M.T


def cut_value(G, B, side):
    """(good, bad) as Python ints; a node's cells sum to less than 2^53, so the u64 sums are exact"""
    sep = np.triu(side[:, None] != side[None, :], 1)
    return int(G[sep].sum()), int(B[sep].sum())


def valid(val, side):
    ones = int(side.sum())
    return val[0] > 0 and ones >= 2 and len(side) - ones >= 2


def edge_weights(G, B, p, q, n):
    """w = q G - p B in Python integers (an object array).  Where 2 n max|w| < 2^62 -- checked on those integers -- no
    sum the local search forms can leave int64, and the same values are handed out as int64, which is only faster."""
    W = q * G.astype(object) - p * B.astype(object)
    if 2 * n * max(abs(int(W.max())), abs(int(W.min()))) < 1 << 62:
        return W.astype(np.int64)
    return W


def local_search(W, n, side):
    side = side.copy()
    sgn = 1 - 2 * side.astype(np.int64)                     # +1 / -1
    gain = sgn * W.dot(sgn.astype(W.dtype))                 # gain[v] = sum over u of (same side ? w : -w); w[v][v] = 0
    cnt = [n - int(side.sum()), int(side.sum())]
    for _ in range(50 * n):
        elig = np.nonzero(np.asarray(gain > 0, bool) & (np.array(cnt)[side] > 2))[0]
        if len(elig) == 0:
            break
        vals = gain[elig]
        v = int(elig[np.nonzero(np.asarray(vals == max(vals), bool))[0][0]])      # the largest gain, the lowest v
        cnt[side[v]] -= 1
        side[v] ^= 1
        cnt[side[v]] += 1
        sgn[v] = -sgn[v]
        gain[v] = -gain[v]
        gain = gain + 2 * int(sgn[v]) * (W[v] * sgn)        # + 2 w where u is now on v's side, - 2 w elsewhere
    return side


def search(Gtri, Btri, n, ns):
    """-> (cut, side list[n] (zeros without a cut), rounds)"""
    if sum(int(x) for x in Btri) == 0:
        return False, [0] * n, 0
    G, B = full(Gtri, n), full(Btri, n)
    if n == 4:
        best = None
        for k in (1, 2, 3):
            side = np.ones(4, np.int64)
            side[0] = side[k] = 0
            val = cut_value(G, B, side)
            if valid(val, side) and (best is None or better(val, best[0])):
                best = (val, side)
        return (True, best[1].tolist(), 0) if best else (False, [0] * 4, 0)
    p = q = 1
    inc = None                                  # (value, side)
    starts = 24 if n <= 8 else 12
    rounds = 0
    for r in range(6):
        rounds += 1
        W = edge_weights(G, B, p, q, n)
        rbest = None
        for s in range(starts + 1):
            if s == 0 and inc is not None:
                side = inc[1]
            else:
                st0 = start_seed(ns, r, s)
                side = np.array([draw(st0, v) & 1 for v in range(n)], np.int64)
                if side.sum() < 2 or n - side.sum() < 2:
                    side = np.arange(n, dtype=np.int64) & 1
            side = local_search(W, n, side)
            val = cut_value(G, B, side)
            if valid(val, side) and (rbest is None or better(val, rbest[0])):
                rbest = (val, side)
        improved = rbest is not None and (inc is None or better(rbest[0], inc[0]))
        if improved:
            inc = rbest
        if inc is None:
            return False, [0] * n, rounds
        if (r > 0 and not improved) or inc[0][1] == 0:
            break
        p, q = inc[0]
    return True, inc[1].tolist(), rounds


# ---------------------------------------------------------------------------------------------------------------------
# graphs
# ---------------------------------------------------------------------------------------------------------------------
def tri_index(u, v, n):
    if u > v:
        u, v = v, u
    return u * n - u * (u + 1) // 2 + v - u - 1


def graph_from_splits(splits, k, n):
    """triangles (G, B) u64 of weighted splits a,b|c,d"""
    G = np.zeros(n * (n - 1) // 2, np.uint64)
    B = np.zeros_like(G)
    for (a, b, c, d), w in zip(np.asarray(splits).tolist(), np.asarray(k).tolist()):
        w = np.uint64(w)
        B[tri_index(a, b, n)] += w
        B[tri_index(c, d, n)] += w
        for x, y in ((a, c), (a, d), (b, c), (b, d)):
            G[tri_index(x, y, n)] += w
    return G, B


def tree_graph(n, rows, wrong, seed):
    """graph of `rows` random quartets of a random generating tree on n taxa, a fraction `wrong` of them given one of
    the two other topologies, unit weights k = 10^5"""
    from supertree_model import rows_from_tree
    _, _, q, sc, st = rows_from_tree(n, rows, "random", wrong, seed=seed)
    q = np.asarray(q, np.int64)
    topo = np.asarray(st)[:, 0]
    sp = q.copy()
    sp[topo == 1] = q[topo == 1][:, [0, 2, 1, 3]]
    sp[topo == 2] = q[topo == 2][:, [0, 3, 1, 2]]
    return graph_from_splits(sp, np.full(len(sp), 100000, np.uint64), n)


def limit_graph(n, seed):
    """a tree graph with 10 % wrong rows whose weights sum to exactly SUM_LIMIT - 1 -- row i k0[i] * 2^20, the first
    row the remainder (below 2^20) more -- and the same graph with every cell divided by 2^20 (floor), which is the
    graph of the weights k0: the remainder is rounded away"""
    from supertree_model import rows_from_tree
    _, _, q, sc, st = rows_from_tree(n, 40 * n, "random", 0.1, seed=seed)
    q = np.asarray(q, np.int64)
    topo = np.asarray(st)[:, 0]
    sp = q.copy()
    sp[topo == 1] = q[topo == 1][:, [0, 2, 1, 3]]
    sp[topo == 2] = q[topo == 2][:, [0, 3, 1, 2]]
    units, rem = divmod(SUM_LIMIT - 1, 1 << 20)
    k0 = np.full(len(sp), units // len(sp), np.uint64)
    k0[:units % len(sp)] += np.uint64(1)
    k = k0 << np.uint64(20)
    k[0] += np.uint64(rem)
    assert int(k.sum()) == SUM_LIMIT - 1
    G, B = graph_from_splits(sp, k, n)
    assert int(B.sum()) == 2 * (SUM_LIMIT - 1) and int(G.sum()) == 4 * (SUM_LIMIT - 1)
    return (G, B), (G >> np.uint64(20), B >> np.uint64(20))


def tie_graph(n):
    """two disjoint quartets 0,1|2,3 and 4,5|6,7 ... of equal weight: many cuts share the best value"""
    sp = [[4 * i, 4 * i + 1, 4 * i + 2, 4 * i + 3] for i in range(n // 4)]
    if n == 4:
        sp = [[0, 1, 2, 3], [0, 2, 1, 3]]                       # two of the three splits tie
    return graph_from_splits(sp, np.full(len(sp), 100000, np.uint64), n)


def forced_start_node(n=5, tries=4000):
    """a node seed for which start 1 of round 0 draws fewer than 2 vertices on one side"""
    for ns in range(1, tries):
        st0 = start_seed(ns, 0, 1)
        ones = sum(draw(st0, v) & 1 for v in range(n))
        if ones < 2 or n - ones < 2:
            return ns
    raise AssertionError("no such seed")


def standard_cases(sizes, seed=0):
    """[(name, n, G, B, node seed)]: per size the tree graphs with 0 / 10 / 40 % wrong rows, all-zero B, all-zero G, the
    tie graph, the limit-weight graph and its 2^-20 copy (which must give the same sides)"""
    cases = []
    for n in sizes:
        rows = max(3, min(30 * n, 6000))
        for wrong in (0.0, 0.1, 0.4):
            G, B = tree_graph(n, rows, wrong, seed + n)
            cases.append((f"tree{int(wrong * 100)}", n, G, B, node_seed(seed, n, int(wrong * 10))))
        G, B = tree_graph(n, rows, 0.1, seed + n + 1)
        cases.append(("zeroB", n, G, np.zeros_like(B), node_seed(seed, n, 5)))
        cases.append(("zeroG", n, np.zeros_like(G), B, node_seed(seed, n, 6)))
        G, B = tie_graph(n)
        cases.append(("tie", n, G, B, node_seed(seed, n, 7)))
        (Gb, Bb), (Gs, Bs) = limit_graph(n, seed + n + 2)
        cases.append(("limit", n, Gb, Bb, node_seed(seed, n, 8)))
        cases.append(("limit_small", n, Gs, Bs, node_seed(seed, n, 8)))
    return cases


_MODEL_CACHE = {}


def model_batch(cases):
    """the model's answer for every case, computed once per (name, n, seed) and shared between tests"""
    out = []
    for name, n, G, B, ns in cases:
        key = (name, n, ns, int(G.sum()), int(B.sum()))
        if key not in _MODEL_CACHE:
            _MODEL_CACHE[key] = search(G, B, n, ns)
        out.append(_MODEL_CACHE[key])
    return out


def run_batch(cases, ctx=None):
    """`tq_stree_search` on the batch -> [(cut, side list, rounds)]"""
    from tetrad_amd import _lib
    lib = _lib.load()
    sizes = np.array([c[1] for c in cases], np.int32)
    G = np.ascontiguousarray(np.concatenate([c[2] for c in cases]), np.uint64)
    B = np.ascontiguousarray(np.concatenate([c[3] for c in cases]), np.uint64)
    seeds = np.array([c[4] for c in cases], np.uint64)
    side = np.full(int(sizes.sum()), 255, np.uint8)
    cut = np.full(len(cases), 255, np.uint8)
    rounds = np.full(len(cases), -1, np.int32)
    rc = lib.tq_stree_search(ctx, len(cases), sizes.ctypes.data, G.ctypes.data, B.ctypes.data, seeds.ctypes.data,
                             side.ctypes.data, cut.ctypes.data, rounds.ctypes.data)
    if rc != 0:
        raise _lib.TetradHipError(rc, lib.tq_last_error(ctx).decode())
    out, o = [], 0
    for i, n in enumerate(sizes.tolist()):
        out.append((bool(cut[i]), side[o:o + n].tolist(), int(rounds[i])))
        o += n
    return out

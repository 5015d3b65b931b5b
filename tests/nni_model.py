"""Independent model of the NNI scan and the polish search for their tests.

No LCA table and no depths: the corners of an edge are the side masks of `fit_model.side_masks` (taxa below a node, as
Python ints), a row counts on an edge when its four taxa test one into each of the four masks, and a neighbour tree is
made by exchanging two children in the parent array.  `model_round` is the round rule written out literally."""
import numpy as np

import fit_model as fm


def canonical(parent, T):
    """The prepared tree of a parent array as the library holds it: unary nodes suppressed, a root of degree 2 dissolved
    into its first internal child (children in node order), then children ordered by their smallest taxon, the root
    numbered T and the internal nodes in BFS order.  Returns the parent array of that numbering."""
    parent = [int(p) for p in parent]
    n = len(parent)
    kids = [[] for _ in range(n)]
    root = parent.index(-1)
    for v, p in enumerate(parent):
        if p >= 0:
            kids[p].append(v)

    def skip(v):                                    # through unary nodes
        while v >= T and len(kids[v]) == 1:
            v = kids[v][0]
        return v

    root = skip(root)
    ch = {}
    stack = [root]
    while stack:
        v = stack.pop()
        if v >= T:
            ch[v] = [skip(c) for c in kids[v]]
            stack.extend(ch[v])
    if len(ch[root]) == 2:
        a, b = ch[root]
        if a < T:
            a, b = b, a
        ch[a].append(b)
        del ch[root]
        root = a
    low = {}

    def smallest(v):
        order, out = [v], []
        while order:
            x = order.pop()
            out.append(x)
            order.extend(ch.get(x, ()))
        for x in reversed(out):
            low[x] = x if x < T else min(low[c] for c in ch[x])
    smallest(root)
    bfs = [root]
    for v in bfs:
        if v >= T:
            ch[v].sort(key=low.get)
            bfs.extend(ch[v])
    ids, nxt = {}, T
    for v in bfs:
        if v < T:
            ids[v] = v
        else:
            ids[v] = nxt
            nxt += 1
    par = np.full(nxt, -1, np.int32)
    for v in bfs:
        for c in ch.get(v, ()):
            par[ids[c]] = ids[v]
    return par


def low_bit(m):
    return (m & -m).bit_length() - 1


def edges(par, T):
    """Per internal non-root node v of a canonical parent array, ascending: dict(v, u, eligible, masks [X1, X2, Y1, Y2],
    nodes [the same corners as nodes, None = everything not below u])."""
    par = [int(p) for p in par]
    n = len(par)
    below = fm.side_masks(par, T)                   # root = T is left out
    mask = {v: below[v if v < T else v - 1] for v in range(n) if v != T}
    full = (1 << T) - 1
    kids = [[] for _ in range(n)]
    for v, p in enumerate(par):
        if p >= 0:
            kids[p].append(v)
    out = []
    for v in range(T + 1, n):
        u = par[v]
        others = [c for c in kids[u] if c != v]
        rec = dict(v=v, u=u, eligible=False, masks=[0, 0, 0, 0], nodes=[None] * 4)
        if len(kids[v]) == 2 and len(others) + (u != T) == 2:
            xs = sorted(kids[v], key=lambda c: low_bit(mask[c]))
            ys = [(mask[c], c) for c in others]
            if u != T:
                ys.append((full ^ mask[u], None))
            ys.sort(key=lambda mc: low_bit(mc[0]))
            rec.update(eligible=True, masks=[mask[xs[0]], mask[xs[1]], ys[0][0], ys[1][0]],
                       nodes=[xs[0], xs[1], ys[0][1], ys[1][1]])
        out.append(rec)
    return out


def model_scan(parent, T, splits, k):
    """[(eligible, [X1, X2, Y1, Y2] as Python ints, [w0, w1, w2] as Python ints)] per edge of the prepared tree."""
    par = canonical(parent, T)
    sp = np.asarray(splits, np.int64).reshape(-1, 4)
    kk = np.asarray(k, np.uint64)
    res = []
    for ed in edges(par, T):
        w = [0, 0, 0]
        if ed["eligible"] and len(sp):
            corner = np.full(T, 4, np.int64)                                 # 4: in no corner
            for j, m in enumerate(ed["masks"]):
                bits = np.unpackbits(np.frombuffer(m.to_bytes((T + 7) // 8, "little"), np.uint8), bitorder="little")[:T]
                assert (corner[bits == 1] == 4).all(), "corners overlap"
                corner[bits == 1] = j
            c = corner[sp]                                                   # [n, 4]
            inside = (1 << c).sum(axis=1) == 15                              # one taxon in each corner
            same_side = (c[:, 0] // 2) == (c[:, 1] // 2)                     # {X1, X2} or {Y1, Y2}
            alt1 = ~same_side & ((c[:, 0] % 2) == (c[:, 1] % 2))             # {X1, Y1} or {X2, Y2}
            for j, sel in enumerate((same_side, alt1, ~same_side & ~alt1)):
                w[j] = sum(int(x) for x in kk[inside & sel])
        res.append((ed["eligible"], ed["masks"], w))
    return res


def neighbour(par, T, ed, alt):
    """The parent array with the interchange of alternative `alt` (1 or 2) made on edge record `ed` of `edges(par, T)`:
    X2 changes places with Y1 (alternative 1) or Y2 (alternative 2); when that corner is the one above u, X1 changes
    places with the sibling instead -- the same unrooted tree."""
    new = np.array(par, np.int32)
    x1, x2, y1, y2 = ed["nodes"]
    target, rest = (y1, y2) if alt == 1 else (y2, y1)
    a, b = (x2, target) if target is not None else (x1, rest)
    new[a], new[b] = ed["u"], ed["v"]
    return new


def model_round(par, T, splits, k):
    """One round on a canonical parent array: (moves, sum of gains, the canonical parent array after it)."""
    eds = edges(par, T)
    scan = model_scan(par, T, splits, k)
    cand = []
    for e, (ed, (elig, _, w)) in enumerate(zip(eds, scan)):
        if not elig:
            continue
        alt = 2 if w[2] > w[1] else 1
        if w[alt] > w[0]:
            cand.append((-(w[alt] - w[0]), e, alt))
    cand.sort()
    used, new, gain, moves = set(), np.array(par, np.int32), 0, 0
    for g, e, alt in cand:
        ed = eds[e]
        if ed["u"] in used or ed["v"] in used:
            continue
        used.update((ed["u"], ed["v"]))
        new = neighbour(new, T, ed, alt)
        gain -= g
        moves += 1
    return moves, gain, canonical(new, T)


def newick(par, T):
    par = [int(p) for p in par]
    kids = [[] for _ in par]
    for v, p in enumerate(par):
        if p >= 0:
            kids[p].append(v)
    below = fm.side_masks(par, T)
    mask = {v: below[v if v < T else v - 1] for v in range(len(par)) if v != T}

    def text(v):
        if v < T:
            return str(v)
        return "(" + ",".join(text(c) for c in sorted(kids[v], key=lambda c: low_bit(mask[c]))) + ")"
    return text(T) + ";"


def model_polish(parent, T, splits, k, max_rounds=1000):
    """(newick, moves per round, gains per round, converged) as `Supertree.polish` returns them."""
    par = canonical(parent, T)
    moves, gains, converged = [], [], False
    for _ in range(max_rounds):
        m, g, par = model_round(par, T, splits, k)
        if m == 0:
            converged = True
            break
        moves.append(m)
        gains.append(g)
    return newick(par, T), moves, gains, converged


def all_neighbours(parent, T):
    """Every NNI neighbour of the tree: [(edge index, alt, parent array)], 2 per eligible edge."""
    par = canonical(parent, T)
    return [(e, alt, neighbour(par, T, ed, alt)) for e, ed in enumerate(edges(par, T)) if ed["eligible"] for alt in (1, 2)]

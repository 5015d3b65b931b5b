"""Pure-Python restatement of the reference's concordance step (tetrad/src/concordance.py) with the deviations of
DESIGN.md section 11, for tests.  Independent of the library's path: edges come from an explicit traversal of the
unrooted tree and the product of the parts around each edge (no LCA table, no distances).

    model = ConcordanceModel(parent, T, min_snps, min_ratio)
    model.add(quartets, rscor, rstat, flags)      # any number of times
    model.result()                                # dict keyed by split (frozenset of the side without taxon 0)
"""
from __future__ import annotations

from itertools import combinations, product
from math import log

import numpy as np


def reread6(x: float) -> float:
    """The value a score reads back as from the TSV ("%.6f", run_inference.py:233-234)."""
    return float("%.6f" % x)


def row_values(scores):
    """(weight, score) of one row as concordance.py:80-89 computes them, but with a numeric sort (deviation 1)."""
    s = sorted(reread6(float(x)) for x in scores)
    weight = (s[1] + s[2]) / 2
    score = 0 if not s[0] else weight / s[0]
    return weight, score


def row_values_reference(score_texts):
    """concordance.py:80-89 as written: the score strings are sorted as strings."""
    scores = np.array(sorted(score_texts), dtype=np.float64)
    weight = np.mean(sorted(scores)[1:])
    min_score = scores.min()
    score = 0 if not min_score else np.mean(scores[1:]) / scores.min()
    return float(weight), float(score)


def qc(conc, disc1, disc2) -> float:
    z = int(conc > 0) + int(disc1 > 0) + int(disc2 > 0)
    if z == 1:
        return 1.0 if conc else -1.0
    nq = conc + disc1 + disc2
    value = 0.0
    for i in (conc, disc1, disc2):
        if i:
            value += (i / nq) * log(i / nq, z)
    return 1.0 + value


def qd(disc1, disc2) -> float:
    if not disc1 + disc2:
        return 1.0
    return 1.0 - abs(disc1 - disc2) / (disc1 + disc2)


def unrooted(parent, T):
    """Adjacency sets of the unrooted tree: nodes of degree 2 (a root of degree 2, unary nodes) are dissolved."""
    adj = {v: set() for v in range(len(parent))}
    for v, p in enumerate(parent):
        if p >= 0:
            adj[v].add(p)
            adj[p].add(v)
    changed = True
    while changed:
        changed = False
        for v in list(adj):
            if v >= T and len(adj[v]) == 2:
                a, b = adj.pop(v)
                adj[a].discard(v)
                adj[b].discard(v)
                adj[a].add(b)
                adj[b].add(a)
                changed = True
            elif v >= T and len(adj[v]) == 1:       # a root with one child
                (a,) = adj.pop(v)
                adj[a].discard(v)
                changed = True
    return adj


def tips_beyond(adj, T, start, avoid):
    """Taxa reachable from `start` without passing through `avoid`."""
    seen, stack, out = {avoid, start}, [start], []
    while stack:
        v = stack.pop()
        if v < T:
            out.append(v)
        for w in adj[v]:
            if w not in seen:
                seen.add(w)
                stack.append(w)
    return out


def tree_edges(parent, T):
    """[(split, parts_u, parts_v)] for every edge between two internal nodes; split = frozenset of the side that
    does not hold taxon 0."""
    adj = unrooted(parent, T)
    out = []
    for u in adj:
        for v in adj[u]:
            if u < v and u >= T and v >= T:
                pu = [tips_beyond(adj, T, w, u) for w in adj[u] if w != v]
                pv = [tips_beyond(adj, T, w, v) for w in adj[v] if w != u]
                side = frozenset(t for p in pu for t in p)
                if 0 in side:
                    side = frozenset(t for p in pv for t in p)
                out.append((side, pu, pv))
    return out


def induced_table(parent, T):
    """prepare_fixed_tree (concordance.py:97-125) with the general rule for polytomies (deviation 6): sorted
    quartet -> (split of the edge, (pair, pair) the tree resolves it into)."""
    table = {}
    for side, pu, pv in tree_edges(parent, T):
        for (A, B), (C, D) in product(combinations(pu, 2), combinations(pv, 2)):
            for a, b, c, d in product(A, B, C, D):
                key = tuple(sorted((a, b, c, d)))
                assert key not in table, "a quartet induced on two edges"
                table[key] = (side, (frozenset((a, b)), frozenset((c, d))))
    return table


class ConcordanceModel:
    def __init__(self, parent, T, min_snps=0, min_ratio=1.0):
        self.T = T
        self.min_snps = max(1, int(min_snps))          # deviation 2
        self.min_ratio = float(min_ratio)
        self.table = induced_table(parent, T)
        self.edges = {}
        for side, pu, pv in tree_edges(parent, T):
            self.edges[side] = dict(nqrts=0, conc=0, disc1=0, disc2=0, nu=0, nsnps=[], weights=[], scores=[])
        for side, _ in self.table.values():
            self.edges[side]["nqrts"] += 1
        self.QFc = [0] * T
        self.QFd = [0] * T
        self.skipped = 0

    def add(self, quartets, rscor, rstat, flags=None):
        quartets = np.asarray(quartets).reshape(-1, 4)
        for i in range(quartets.shape[0]):
            q = [int(x) for x in quartets[i]]
            rhat, nsnps = int(rstat[i][0]), int(rstat[i][1])
            fl = 0 if flags is None else int(flags[i])
            if fl & (4 | 16) or len(set(q)) < 4 or max(q) >= self.T or rhat > 2:
                self.skipped += 1
                continue
            hit = self.table.get(tuple(sorted(q)))
            if hit is None:
                continue
            side, (p1, p2) = hit
            # the tree's resolution in the row's own positions (TSV convention, run_inference.py:264-270)
            pairs = [frozenset((q[0], q[1])), frozenset((q[0], q[2])), frozenset((q[0], q[3]))]
            r = next(k for k in range(3) if pairs[k] in (p1, p2))
            e = self.edges[side]
            weight, score = row_values(rscor[i])
            e["nsnps"].append(nsnps)
            e["weights"].append(weight)
            e["scores"].append(score)
            if score < self.min_ratio or nsnps < self.min_snps:
                e["nu"] += 1
                continue
            if rhat == r:
                e["conc"] += 1
                for t in q:
                    self.QFc[t] += 1
            else:
                for t in q:
                    self.QFd[t] += 1
                lower = min(k for k in range(3) if k != r)
                e["disc1" if rhat == lower else "disc2"] += 1

    def result(self):
        out = {}
        for side, e in self.edges.items():
            n = e["conc"] + e["disc1"] + e["disc2"] + e["nu"]
            out[side] = dict(
                nqrts=e["nqrts"], conc=e["conc"], disc1=e["disc1"], disc2=e["disc2"], nu=e["nu"],
                nsnps_sum=sum(e["nsnps"]), weight_sum=float(np.sum(e["weights"])) if n else 0.0,
                score_sum=float(np.sum(e["scores"])) if n else 0.0,
                QC=qc(e["conc"], e["disc1"], e["disc2"]), QD=qd(e["disc1"], e["disc2"]),
                QI=(1 - e["nu"] / n) if n else float("nan"),
                nsnps=float(np.mean(e["nsnps"])) if n else float("nan"),
                weights=float(np.mean(e["weights"])) if n else float("nan"),
                scores=float(np.mean(e["scores"])) if n else float("nan"))
        qf = [c / (c + d) if c + d else float("nan") for c, d in zip(self.QFc, self.QFd)]
        return dict(edges=out, QFc=list(self.QFc), QFd=list(self.QFd), QF=qf, skipped=self.skipped)


def random_tree(T, rng, multifurcate=0.0, rooted=True):
    """A random parent array over taxa 0..T-1 (tips) built by random joins; with probability `multifurcate` a join
    takes three subtrees; `rooted=False` ends with a root of degree 3 when possible; a unary node is inserted
    now and then (the library must suppress it)."""
    roots = list(range(T))
    parent = [-1] * T
    while len(roots) > (1 if rooted else 3):
        k = 3 if (len(roots) >= 3 + (0 if rooted else 3) and rng.random() < multifurcate) else 2
        picks = sorted(rng.choice(len(roots), size=k, replace=False).tolist(), reverse=True)
        v = len(parent)
        parent.append(-1)
        for p in picks:
            parent[roots[p]] = v
            roots.pop(p)
        if rng.random() < 0.1:                       # a unary node above v
            u = len(parent)
            parent.append(-1)
            parent[v] = u
            v = u
        roots.append(v)
    if len(roots) > 1:
        v = len(parent)
        parent.append(-1)
        for r in roots:
            parent[r] = v
    return np.array(parent, np.int32)


def side_of(mask_row, T):
    """A bool split row (library) -> the model's key (frozenset of the side without taxon 0)."""
    side = frozenset(int(t) for t in np.flatnonzero(mask_row))
    return side if 0 not in side else frozenset(range(T)) - side

"""Quartet frequencies of a set of trees and the leaf stability of its taxa: which taxa the trees disagree about.

Consensus supports, transfer supports and the two distance matrices say how much a set of replicate trees disagrees;
this says where.  The leaf stability index of Thorley & Wilkinson (1999) scores a taxon by how often the trees agree on
the small subtrees that hold it -- quartets here, because the trees are unrooted.  A rogue taxon, which sits somewhere
else in every replicate, has the lowest index.

Per quartet row the trees are counted by the topology they show (`tq_ls_*`, tetrad_amd/csrc/stability.hpp), exactly, as
integers, on the host (`LeafStability(ntaxa, max_trees)`) or on the device (`engine=...`: the bit planes of `qdist`
summed along the trees by a HIP kernel).  Both give identical arrays.  The table of counts is useful on its own: it is
the quartet-support table of a tree set and, through `dominant_splits`, the weighted quartet input of a summary tree
(`qmc.qmc_tree`).  No reference counterpart.

Definitions, over the N trees held, for a quartet row (a, b, c, d) as given:
  counts      u16 (n_0, n_1, n_2, n_3): the trees that show ab|cd, ac|bd, ad|bc, and the ones that leave it unresolved
  top         max(n_0, n_1, n_2)         second  the second largest of the three (= top when the largest is tied)
  dif         top - second               res     n_0 + n_1 + n_2
  raw()       u64 [T, 4] = (quartets, res, top, dif) summed over every scored row that holds the taxon
  stability   ls_res = res / (N quartets), ls_max = top / (N quartets), ls_dif = dif / (N quartets); 0.0 where the taxon is
              in no scored row or there are no trees (the only floats of this module)
"""
from __future__ import annotations

import numpy as np

from .concordance import newick_to_parent
from .qdist import QuartetScoring

KINDS = {"res": 1, "max": 2, "dif": 3}     # the column of raw() a kind of stability divides


class LeafStability(QuartetScoring):
    """Quartet frequencies and leaf stability over all trees added, on the taxa 0..ntaxa-1.

    ntaxa       4..1024
    max_trees   1..8192: the room for trees (the device back end allocates their tables at create)
    samples     names of the taxa for `add_newick` and `rogues`
    engine      a `QuartetEngine`: the work is done on its device; None: on the host

    Every `score*` method of `qdist.QuartetDistances` is here with the same meaning; with `counts=True` it returns the
    table of counts of the rows it scored (u16 [Q, 4]) and waits for it.
    """

    _prefix = "tq_ls"
    _row_counts = True

    # -- reading --------------------------------------------------------------------------------------------
    def raw(self) -> np.ndarray:
        """u64 [ntaxa, 4] = (quartets, res, top, dif) per taxon, as the library returns it; waits for the device."""
        out = np.zeros((self.ntaxa, 4), np.uint64)
        self._check(self._lib.tq_ls_read(self._h, out.ctypes.data))
        return out

    def quartets_per_taxon(self) -> np.ndarray:
        """[t] the scored rows that hold taxon t (i64)."""
        return self.raw()[:, 0].astype(np.int64)

    def stability(self, kind: str = "dif") -> np.ndarray:
        """ls_dif, ls_max or ls_res as f64 [ntaxa]; 0.0 where the taxon is in no scored row, and without trees."""
        if kind not in KINDS:
            raise ValueError(f"no stability of kind {kind!r}: one of {sorted(KINDS)}")
        raw = self.raw()
        den = raw[:, 0].astype(np.float64) * self.ntrees
        out = np.zeros(self.ntaxa, np.float64)
        np.divide(raw[:, KINDS[kind]].astype(np.float64), den, out=out, where=den != 0)
        return out

    def ranking(self, kind: str = "dif") -> np.ndarray:
        """The taxa from the least to the most stable (i64 [ntaxa]); ties go to the lower index."""
        return np.argsort(self.stability(kind), kind="stable").astype(np.int64)

    def rogues(self, k: int, kind: str = "dif") -> list:
        """The `k` least stable taxa: their names when `samples` was given at create, their numbers otherwise."""
        first = [int(t) for t in self.ranking(kind)[:max(0, int(k))]]
        return [self.samples[t] for t in first] if self.samples is not None else first

    def stats(self) -> dict:
        """Counters: quartets per chunk, quartet chunks launched and tree tables built since create / reset, the table
        form (0 host, 1 LDS, 2 through L2), plane words per chunk, the workgroups of the last count launch (0 on the
        host) and the trees the count kernel stages per pass."""
        out = np.zeros(7, np.int64)
        self._check(self._lib.tq_ls_stats(self._h, out.ctypes.data))
        keys = ("chunk_quartets", "chunks", "tables", "table_form", "chunk_words", "workgroups", "tree_tile")
        return {k: int(v) for k, v in zip(keys, out)}


def quartet_frequencies(newicks, quartets=None, samples=None, engine=None):
    """(quartets i32 [Q, 4], counts u16 [Q, 4]) of trees given as newick text, in one call: per row of `quartets` -- or,
    with None, per 4-combination of the taxa in rank order -- how many trees show each of its three pairings and how many
    leave it unresolved.  Tips are taxon numbers, or names through `samples`."""
    newicks = [newicks] if isinstance(newicks, str) else list(newicks)
    if not newicks:
        raise ValueError("no trees")
    _, T, _ = newick_to_parent(newicks[0], samples)
    with LeafStability(T, len(newicks), samples=samples, engine=engine) as acc:
        acc.add_newick(newicks)
        if quartets is None:
            from itertools import combinations
            q = np.array(list(combinations(range(T), 4)), np.int32).reshape(-1, 4)
            return q, acc.score_all(counts=True)
        q = np.ascontiguousarray(quartets, dtype=np.int32).reshape(-1, 4)
        return q, acc.score(q, counts=True)


def dominant_splits(quartets, counts, min_count: int = 1):
    """(splits u32 [n, 4], weights f64 [n]) in the form `qmc.qmc_tree` takes: per row the pairing that strictly more trees
    show than either other, written a,b|c,d -- (a, b, c, d), (a, c, b, d) or (a, d, b, c) for code 0, 1 or 2 -- weighted
    by that count.  A row whose largest count is tied or below `min_count` is left out.
    `qmc_tree(*dominant_splits(*quartet_frequencies(trees)), ntaxa=T)` is a summary tree of the set."""
    q = np.asarray(quartets, dtype=np.int64).reshape(-1, 4)
    n = np.asarray(counts, dtype=np.int64).reshape(-1, 4)[:, :3]
    if len(q) != len(n):
        raise ValueError("quartets and counts must have one row each per quartet")
    code = np.argmax(n, axis=1)
    top = n[np.arange(len(n)), code]
    keep = ((n == top[:, None]).sum(axis=1) == 1) & (top >= int(min_count))
    order = np.array([[0, 1, 2, 3], [0, 2, 1, 3], [0, 3, 1, 2]])[code[keep]]
    splits = np.take_along_axis(q[keep], order, axis=1).astype(np.uint32)
    return splits, top[keep].astype(np.float64)

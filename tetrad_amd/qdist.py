"""All-pairs quartet distances of a set of trees -- what tqDist's `all_pairs_quartet_distance` reports: for every pair of
trees the number of quartets of taxa the two resolve differently.  The supertrees of this package optimise quartet fit,
so this is the ruler that matches them; and where one misplaced taxon breaks every split on its path (and with it the
Robinson-Foulds distance of `treedist`), it changes only the quartets that hold it.

Tree is compared with tree (`tq_qd_*`, tetrad_amd/csrc/qdist.hpp) exactly, as integers, on the host
(`QuartetDistances(ntaxa, max_trees)`) or on the device (`engine=...`: a HIP kernel writes three bit planes per tree
over a chunk of quartets, one bit per quartet and topology, and a tiled binary GEMM multiplies the planes).  Both give
identical arrays.  The quartets are all C(ntaxa, 4), a range of their ranks, a sample, or an explicit list.
No reference counterpart.

Definitions, per pair of trees (i, j) over the quartets scored so far (`nquartets`):
  same       both trees resolve the quartet, alike          both   both trees resolve it
  A = same   B = both - same (resolved differently)         C = both[i][i] - both[i][j] (only i resolves it)
  D = C^T    E = nquartets - both[i][i] - both[j][j] + both[i][j] (neither resolves it)
  resolved   [i] = both[i][i]
  distance   B + C + D, tqDist's quartet distance
  normalized distance / nquartets, 0.0 before anything is scored (the only float of this module)
"""
from __future__ import annotations

import ctypes
from math import comb

import numpy as np

from ._handle import Handle, mean_pairs, medoid
from .concordance import TreeSetInput, newick_to_parent

RANGE_STEP = 1 << 24        # ranks per call of score_range / score_all


class QuartetScoring(TreeSetInput, Handle):
    """What the accumulators over the quartets of a tree set share (`QuartetDistances` here, `stability.LeafStability`):
    create, adding trees, every way of naming the quartets to score, and the shape.  A family sets `_prefix`; one whose
    library calls return a table of counts per quartet row sets `_row_counts`, and then `counts=True` makes a score
    method return that table (u16 [Q, 4])."""

    _row_counts = False

    def __init__(self, ntaxa: int, max_trees: int, samples=None, engine=None):
        self.ntaxa, self.max_trees, self.engine, self.samples = int(ntaxa), int(max_trees), engine, samples
        self._create(self.ntaxa, self.max_trees, self._ctx())
        self.total_quartets = comb(self.ntaxa, 4)

    def clear(self):
        """Zeroes the counts and keeps the trees."""
        self._check(self._fn("clear")(self._h))

    def reset(self):
        """Forgets the trees and the counts."""
        super().reset()

    # -- adding trees ---------------------------------------------------------------------------------------
    def _add(self, block, n_nodes, stride, stream):
        """Refused once quartets have been scored, until `clear` or `reset`."""
        self._check(self._fn("add")(self._h, block.ctypes.data, n_nodes.ctypes.data, len(n_nodes), stride, stream))

    # -- scoring quartets -----------------------------------------------------------------------------------
    def _table(self, Q: int, counts: bool):
        """The array a score call fills ([Q, 4] u16; zero rows stay where the library has nothing to score), or None."""
        if not counts:
            return None
        if not self._row_counts:
            raise ValueError(f"{type(self).__name__} has no counts per quartet")
        return np.zeros((Q, 4), np.uint16)

    def _call(self, name, *args, table=None, offset=0, stream=0):
        """tq_<family>_<name>(handle, *args[, the rows of `table` from `offset`], stream)."""
        if isinstance(stream, bool):        # score(quartets, True) meant counts=True: never hand 1 to the device as a stream
            raise TypeError("stream is a hipStream_t address; counts is given by keyword")
        if self._row_counts:
            args += (table[offset:].ctypes.data if table is not None and offset < len(table) else None,)
        self._check(self._fn(name)(self._h, *args, stream or None))

    def score(self, quartets, stream: int = 0, *, counts: bool = False):
        """Quartets as an integer array [Q, 4]: four distinct taxa each, in any order.  All are checked first."""
        q = np.ascontiguousarray(quartets, dtype=np.int32)
        if q.size == 0:
            return self._table(0, counts)
        if q.ndim != 2 or q.shape[1] != 4:
            raise ValueError("quartets must have the shape [Q, 4]")
        table = self._table(q.shape[0], counts)
        self._call("score", q.ctypes.data, q.shape[0], table=table, stream=stream)
        return table

    def score_ranks(self, ranks, stream: int = 0, *, counts: bool = False):
        """Quartets as lexicographic ranks of 4-combinations of the taxa, each below C(ntaxa, 4)."""
        r = np.ascontiguousarray(ranks, dtype=np.uint64).reshape(-1)
        table = self._table(r.shape[0], counts)
        if r.size:
            self._call("score_ranks", r.ctypes.data, 0, r.shape[0], table=table, stream=stream)
        return table

    def score_range(self, first: int, count: int, stream: int = 0, *, counts: bool = False):
        """The `count` consecutive ranks from `first`, issued in ranges of at most 2^24.  Checked as a whole first."""
        first, count = int(first), int(count)
        if first < 0 or count < 0 or first + count > self.total_quartets:
            raise ValueError(f"rank range [{first},+{count}) exceeds C({self.ntaxa},4) = {self.total_quartets}")
        table = self._table(count, counts)
        for lo in range(first, first + count, RANGE_STEP):
            n = min(RANGE_STEP, first + count - lo)
            self._call("score_ranks", None, lo, n, table=table, offset=lo - first, stream=stream)
        return table

    def score_all(self, stream: int = 0, *, counts: bool = False):
        """All C(ntaxa, 4) quartets."""
        return self.score_range(0, self.total_quartets, stream, counts=counts)

    def sample_ranks(self, n: int, seed) -> np.ndarray:
        """`n` distinct ranks drawn with numpy.random.default_rng(seed), ascending."""
        n = int(n)
        if n < 0 or n > self.total_quartets:
            raise ValueError(f"cannot draw {n} distinct quartets of C({self.ntaxa},4) = {self.total_quartets}")
        ranks = np.random.default_rng(seed).choice(self.total_quartets, size=n, replace=False)
        return np.sort(ranks).astype(np.uint64)

    def score_sample(self, n: int, seed, stream: int = 0, *, counts: bool = False):
        """Scores `n` distinct sampled quartets (see `sample_ranks`) and returns their ranks; with `counts=True`
        (ranks, the table of their counts)."""
        ranks = self.sample_ranks(n, seed)
        table = self.score_ranks(ranks, stream, counts=counts)
        return (ranks, table) if counts else ranks

    # -- reading --------------------------------------------------------------------------------------------
    def _shape(self):
        T, n, q = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_uint64()
        self._check(self._fn("shape")(self._h, ctypes.byref(T), ctypes.byref(n), ctypes.byref(q)))
        return T.value, n.value, q.value

    @property
    def ntrees(self) -> int:
        return self._shape()[1]

    @property
    def nquartets(self) -> int:
        """Quartets scored since create, `clear` or `reset`."""
        return self._shape()[2]


class QuartetDistances(QuartetScoring):
    """Quartet distances between all trees added, on the taxa 0..ntaxa-1.

    ntaxa       4..1024
    max_trees   1..8192: the room for trees (the device back end allocates their tables and two max_trees^2 matrices at
                create)
    samples     names of the taxa for `add_newick`
    engine      a `QuartetEngine`: the work is done on its device; None: on the host
    """

    _prefix = "tq_qd"

    def raw(self):
        """(same u64[N, N], both u64[N, N]) as the library returns them; waits for the device."""
        N = self.ntrees
        same = np.zeros((N, N), np.uint64)
        both = np.zeros((N, N), np.uint64)
        self._check(self._lib.tq_qd_read(self._h, same.ctypes.data, both.ctypes.data))
        return same, both

    def counts(self):
        """The five classes (A, B, C, D, E) of Estabrook / tqDist as i64 [N, N] each."""
        same, both = (a.astype(np.int64) for a in self.raw())
        res = np.diag(both)
        A = same
        B = both - same
        C = res[:, None] - both
        D = C.T.copy()
        E = self.nquartets - res[:, None] - res[None, :] + both
        return A, B, C, D, E

    def resolved(self) -> np.ndarray:
        """[i] the scored quartets tree i resolves (i64)."""
        return np.diag(self.raw()[1]).astype(np.int64)

    def distance(self) -> np.ndarray:
        """B + C + D: the quartets the two trees do not treat alike, i64 [N, N]."""
        _, B, C, D, _ = self.counts()
        return B + C + D

    def normalized(self) -> np.ndarray:
        """distance / nquartets as f64 [N, N]; 0.0 before anything is scored."""
        d, q = self.distance(), self.nquartets
        return d / q if q else np.zeros(d.shape, np.float64)

    def medoid(self):
        """(index, row sum) of the tree with the smallest sum of distances to all others; ties go to the lowest index."""
        return medoid(self.distance())

    def mean_distance(self) -> float:
        """The mean distance over the pairs i < j; 0.0 for fewer than 2 trees."""
        return mean_pairs(self.distance())

    def stats(self) -> dict:
        """Counters: quartets per chunk, quartet chunks launched and tree tables built since create / reset, the k
        slices of the last product launch (0 on the host), the table form (0 host, 1 LDS, 2 through L2), plane words
        per chunk."""
        out = np.zeros(6, np.int64)
        self._check(self._lib.tq_qd_stats(self._h, out.ctypes.data))
        keys = ("chunk_quartets", "chunks", "kslices", "tables", "table_form", "chunk_words")
        return {k: int(v) for k, v in zip(keys, out)}


def quartet_distance_matrix(newicks, quartets=None, samples=None, engine=None) -> np.ndarray:
    """The quartet distance matrix (i64 [N, N]) of trees given as newick text, in one call, over `quartets` ([Q, 4]) or,
    with None, over all C(ntaxa, 4); tips are taxon numbers, or names through `samples`."""
    newicks = [newicks] if isinstance(newicks, str) else list(newicks)
    if not newicks:
        raise ValueError("no trees")
    _, T, _ = newick_to_parent(newicks[0], samples)
    with QuartetDistances(T, len(newicks), samples=samples, engine=engine) as acc:
        acc.add_newick(newicks)
        if quartets is None:
            acc.score_all()
        else:
            acc.score(quartets)
        return acc.distance()

"""All-pairs Robinson-Foulds distances of a set of trees -- what `booster`, RAxML-NG's `--rfdist` or toytree report
beside branch supports: do the bootstrap replicates (or N restarts, or two search rules) form one cloud or several
islands, which tree is closest to all others, how far apart they are on average.

`consensus.Consensus` and `tbe.TransferSupport` speak per split; here tree is compared with tree (`tq_rf_*`,
tetrad_amd/csrc/treedist.hpp): exactly, as integers, on the host (`TreeDistances(ntaxa, max_trees)`) or on the device
(`engine=...`: the split table of the consensus kernels numbers the distinct splits, a tree becomes a row of bits, and
a HIP kernel multiplies the bit rows).  Both give identical arrays.  No reference counterpart.

Definitions:
  split      an internal edge with at least 2 taxa on both sides, named by the side without taxon 0
  nsplits    [i] the splits of tree i (0 for a star, ntaxa - 3 for a binary tree)
  shared     [i][j] the splits both trees hold; shared[i][i] = nsplits[i]
  rf         [i][j] = nsplits[i] + nsplits[j] - 2 shared[i][j], the size of the symmetric difference
  normalised rf / (nsplits[i] + nsplits[j]), 0 where both trees are stars (the only float of this module)
"""
from __future__ import annotations

import ctypes

import numpy as np

from .concordance import newick_to_parent


class TreeDistances:
    """Robinson-Foulds distances between all trees added, on the taxa 0..ntaxa-1.

    ntaxa       4..4096
    max_trees   1..8192: the room for trees (the device back end allocates two max_trees^2 matrices at create)
    max_splits  the room for distinct splits; default min(max_trees (ntaxa - 3), 2^26), at least 1
    samples     names of the taxa for `add_newick`
    engine      a `QuartetEngine`: the work is done on its device; None: on the host
    """

    def __init__(self, ntaxa: int, max_trees: int, max_splits=None, samples=None, engine=None):
        from . import _lib
        self._lib = _lib.load()
        self.ntaxa, self.max_trees, self.engine, self.samples = int(ntaxa), int(max_trees), engine, samples
        self._h = None
        if max_splits is None:
            max_splits = max(1, min(self.max_trees * (self.ntaxa - 3), 2 ** 26))
        self.max_splits = int(max_splits)
        h = ctypes.c_void_p()
        self._check(self._lib.tq_rf_create(ctypes.byref(h), self.ntaxa, self.max_trees, self.max_splits,
                                           engine._h if engine is not None else None))
        self._h = h
        self.mask_words = (self.ntaxa + 63) // 64

    # -- lifecycle ------------------------------------------------------------------------------------------
    def _check(self, rc: int):
        if rc != 0:
            from ._lib import TetradHipError
            ctx = self.engine._h if self.engine is not None else None
            raise TetradHipError(rc, self._lib.tq_last_error(ctx).decode())

    def close(self):
        if getattr(self, "_h", None):
            self._lib.tq_rf_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self):
        """Forgets the trees and their splits."""
        self._check(self._lib.tq_rf_reset(self._h))

    # -- adding trees ---------------------------------------------------------------------------------------
    def add_parents(self, parents, stream: int = 0):
        """Trees as parent arrays (nodes 0..ntaxa-1 the taxa, parent[root] = -1), each with its own node count.  All of
        them are validated before any is added.  With an engine the kernels run on `stream` (a hipStream_t)."""
        arrs = [np.ascontiguousarray(p, dtype=np.int32).reshape(-1) for p in parents]
        if not arrs:
            return
        n = np.array([a.shape[0] for a in arrs], np.int64)
        stride = int(n.max())
        block = np.full((len(arrs), stride), -1, np.int32)
        for i, a in enumerate(arrs):
            block[i, :a.shape[0]] = a
        self._check(self._lib.tq_rf_add(self._h, block.ctypes.data, n.ctypes.data, len(arrs), stride, stream or None))

    def add_newick(self, strings, samples=None, stream: int = 0):
        """Trees as newick text: tips are taxon numbers, or names through `samples` (default: those given at create)."""
        if isinstance(strings, str):
            strings = [strings]
        if samples is None:
            samples = self.samples
        parents = []
        for i, s in enumerate(strings):
            try:
                par, T, _ = newick_to_parent(s, samples)
            except ValueError as e:
                raise ValueError(f"tree {i}: {e}") from None
            if T != self.ntaxa:
                raise ValueError(f"tree {i}: {T} taxa, the accumulator compares trees of {self.ntaxa}")
            parents.append(par)
        self.add_parents(parents, stream)

    # -- reading --------------------------------------------------------------------------------------------
    def _shape(self, which: int) -> int:
        out = [ctypes.c_int64() for _ in range(5)]
        args = [ctypes.byref(o) if i == which else None for i, o in enumerate(out)]
        self._check(self._lib.tq_rf_shape(self._h, *args))
        return out[which].value

    @property
    def ntrees(self) -> int:
        return self._shape(2)

    @property
    def ndistinct(self) -> int:
        """Distinct splits over all trees added (waits for the device)."""
        return self._shape(3)

    def raw(self):
        """(nsplits i32[N], shared u32[N, N], rf u32[N, N]) as the library returns them; waits for the device."""
        N = self.ntrees
        nsplits = np.zeros(N, np.int32)
        shared = np.zeros((N, N), np.uint32)
        rf = np.zeros((N, N), np.uint32)
        self._check(self._lib.tq_rf_read(self._h, nsplits.ctypes.data, shared.ctypes.data, rf.ctypes.data))
        return nsplits, shared, rf

    def nsplits(self) -> np.ndarray:
        N = self.ntrees
        out = np.zeros(N, np.int32)
        self._check(self._lib.tq_rf_read(self._h, out.ctypes.data, None, None))
        return out.astype(np.int64)

    def shared(self) -> np.ndarray:
        N = self.ntrees
        out = np.zeros((N, N), np.uint32)
        self._check(self._lib.tq_rf_read(self._h, None, out.ctypes.data, None))
        return out.astype(np.int64)

    def rf(self) -> np.ndarray:
        N = self.ntrees
        out = np.zeros((N, N), np.uint32)
        self._check(self._lib.tq_rf_read(self._h, None, None, out.ctypes.data))
        return out.astype(np.int64)

    def rf_normalized(self) -> np.ndarray:
        """rf / (nsplits[i] + nsplits[j]) as f64 [N, N]; 0 where both trees have no split."""
        n = self.nsplits()
        den = n[:, None] + n[None, :]
        out = np.zeros(den.shape, np.float64)
        np.divide(self.rf(), den, out=out, where=den > 0)
        return out

    def medoid(self):
        """(index, row sum) of the tree with the smallest sum of distances to all others; ties go to the lowest index."""
        rf = self.rf()
        if not len(rf):
            raise ValueError("no trees")
        sums = [sum(int(x) for x in row) for row in rf]
        best = min(range(len(sums)), key=lambda i: (sums[i], i))
        return best, sums[best]

    def mean_rf(self) -> float:
        """The mean distance over the pairs i < j; 0.0 for fewer than 2 trees."""
        rf = self.rf()
        N = len(rf)
        if N < 2:
            return 0.0
        total = sum(int(x) for x in rf[np.triu_indices(N, 1)])
        return total / (N * (N - 1) // 2)

    def stats(self) -> dict:
        """Counters: trees per chunk, tree chunks launched since create / reset, and of the last read the columns
        (distinct splits held by at least two trees), the column words per chunk and the column chunks multiplied; the
        splits resolved on the host after a hash collision, the hash bits in use, the entries of the device table."""
        out = np.zeros(8, np.int64)
        self._check(self._lib.tq_rf_stats(self._h, out.ctypes.data))
        keys = ("chunk_trees", "chunks", "columns", "col_words_chunk", "col_chunks", "unresolved", "hash_bits", "dev_entries")
        return {k: int(v) for k, v in zip(keys, out)}


def rf_matrix(newicks, samples=None, engine=None) -> np.ndarray:
    """The Robinson-Foulds matrix (i64 [N, N]) of trees given as newick text, in one call; tips are taxon numbers, or
    names through `samples`."""
    newicks = [newicks] if isinstance(newicks, str) else list(newicks)
    if not newicks:
        raise ValueError("no trees")
    _, T, _ = newick_to_parent(newicks[0], samples)
    with TreeDistances(T, len(newicks), samples=samples, engine=engine) as acc:
        acc.add_newick(newicks)
        return acc.rf()

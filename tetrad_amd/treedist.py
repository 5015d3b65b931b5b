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

from ._handle import Handle, mean_pairs, medoid
from .concordance import TreeSetInput, newick_to_parent


class TreeDistances(TreeSetInput, Handle):
    """Robinson-Foulds distances between all trees added, on the taxa 0..ntaxa-1.

    ntaxa       4..4096
    max_trees   1..8192: the room for trees (the device back end allocates two max_trees^2 matrices at create)
    max_splits  the room for distinct splits; default min(max_trees (ntaxa - 3), 2^26), at least 1
    samples     names of the taxa for `add_newick`
    engine      a `QuartetEngine`: the work is done on its device; None: on the host
    """

    _prefix = "tq_rf"

    def __init__(self, ntaxa: int, max_trees: int, max_splits=None, samples=None, engine=None):
        self.ntaxa, self.max_trees, self.engine, self.samples = int(ntaxa), int(max_trees), engine, samples
        if max_splits is None:
            max_splits = max(1, min(self.max_trees * (self.ntaxa - 3), 2 ** 26))
        self.max_splits = int(max_splits)
        self._create(self.ntaxa, self.max_trees, self.max_splits, self._ctx())
        self.mask_words = (self.ntaxa + 63) // 64

    def reset(self):
        """Forgets the trees and their splits."""
        super().reset()

    def _add(self, block, n_nodes, stride, stream):
        self._check(self._lib.tq_rf_add(self._h, block.ctypes.data, n_nodes.ctypes.data, len(n_nodes), stride, stream))

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
        return medoid(self.rf())

    def mean_rf(self) -> float:
        """The mean distance over the pairs i < j; 0.0 for fewer than 2 trees."""
        return mean_pairs(self.rf())

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

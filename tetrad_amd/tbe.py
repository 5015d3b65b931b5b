"""Transfer bootstrap supports (TBE; Lemoine et al. 2018, Nature 556:452) of the branches of one tree over a set of
replicate trees -- the support that `booster` and RAxML-NG's `--bs-metric tbe` report beside Felsenstein's frequency.

`consensus.Consensus` counts a replicate for a branch only when it contains the branch exactly.  Here a replicate
contributes the number of taxa that must be moved to turn the branch's bipartition into the closest bipartition of the
replicate (`tq_tbe_*`, tetrad_amd/csrc/tbe.hpp): exactly, as integers, on the host (`TransferSupport(ntaxa, tree)`) or on
the device (`engine=...`: a HIP kernel takes the all-pairs Hamming distances of the branch masks against every node's
mask of every replicate).  Both give identical arrays.  No reference counterpart.

Definitions:
  branch    a split of the reference tree (an internal edge with at least 2 taxa on both sides), its mask the side without
            taxon 0, the branches ordered by mask ascending as one integer (the order of `Consensus.support_of`);
            p = the size of the lighter side
  delta     of two bipartitions with sides A, B: min(|A xor B|, T - |A xor B|)
  phi       of a branch in a replicate: the minimum of delta over every edge of the replicate, tip edges included
            (hence at most p - 1; 0 when the replicate contains the branch)
  TBE       1 - phi_sum / (ntrees (p - 1)); the label is its percent rounded half up, taken in integers
"""
from __future__ import annotations

import ctypes

import numpy as np

from ._handle import Handle, mask_bits
from .concordance import TreeSetInput, newick_to_parent, tree_to_parent, trees_to_parents
from .consensus import write_split_labels


def percent(phi_sum: int, p: int, ntrees: int) -> int:
    """The TBE label of a branch with light side `p` and `phi_sum` over `ntrees` replicates: the percent rounded half
    up, in integers; 0 without replicates."""
    nq = int(ntrees) * (int(p) - 1)
    return (200 * (nq - int(phi_sum)) + nq) // (2 * nq) if nq else 0


def _parent_to_newick(parent, T: int) -> str:
    """Newick text (numeric tips, children in node order) of a parent array."""
    kids = {}
    root = -1
    for v, p in enumerate(parent):
        if p < 0:
            root = v
        else:
            kids.setdefault(int(p), []).append(v)
    order = [root]
    for v in order:
        order.extend(kids.get(v, ()))
    text = {}
    for v in reversed(order):
        text[v] = str(v) if v < T else "(" + ",".join(text.pop(k) for k in kids[v]) + ")"
    return text[root] + ";"


class TransferSupport(TreeSetInput, Handle):
    """Transfer indices of the branches of `tree` summed over replicate trees on the taxa 0..ntaxa-1.

    ntaxa    4..4096
    tree     the reference tree: newick text (tips are taxon numbers, or names through `samples`) or a parent array
    engine   a `QuartetEngine`: the distances are taken on its device; None: on the host
    """

    _prefix = "tq_tbe"

    def __init__(self, ntaxa: int, tree, samples=None, engine=None):
        self.ntaxa, self.engine, self.samples = int(ntaxa), engine, samples
        self._newick = tree if isinstance(tree, str) else None
        self._parent = par = tree_to_parent(tree, self.ntaxa, samples)[0]
        self._create(self.ntaxa, par.ctypes.data, par.shape[0], self._ctx())
        self.mask_words = (self.ntaxa + 63) // 64
        e = ctypes.c_int64()
        self._check(self._lib.tq_tbe_shape(self._h, None, None, ctypes.byref(e), None))
        self.nbranches = e.value

    def reset(self):
        """Forgets the replicates, keeps the reference tree."""
        super().reset()

    # -- adding trees ---------------------------------------------------------------------------------------
    def _add(self, block, n_nodes, stride, stream, phi=None):
        self._check(self._lib.tq_tbe_add(self._h, block.ctypes.data, n_nodes.ctypes.data, len(n_nodes), stride, stream,
                                         None if phi is None else phi.ctypes.data))

    def add_parents(self, parents, stream: int = 0, per_tree: bool = False):
        """Replicates as parent arrays (nodes 0..ntaxa-1 the taxa, parent[root] = -1), each with its own node count.
        All of them are validated before any is added.  With an engine the kernels run on `stream` (a hipStream_t).
        `per_tree`: returns phi as u16 [R, E] (the call then waits for the device)."""
        parents = list(parents)
        phi = np.zeros((len(parents), self.nbranches), np.uint16) if per_tree else None
        self._add_trees(parents, stream, phi)
        return phi

    def add_newick(self, strings, samples=None, stream: int = 0, per_tree: bool = False):
        """Replicates as newick text: tips are taxon numbers, or names through `samples`."""
        return self.add_parents(trees_to_parents(strings, self.ntaxa, samples), stream, per_tree)

    # -- reading --------------------------------------------------------------------------------------------
    @property
    def ntrees(self) -> int:
        n = ctypes.c_int64()
        self._check(self._lib.tq_tbe_shape(self._h, None, None, None, ctypes.byref(n)))
        return n.value

    def raw(self):
        """(masks bool[E, ntaxa] = the side without taxon 0, p i64[E], phi_sum u64[E]) in branch order; waits for the
        device."""
        E = self.nbranches
        masks = np.zeros((E, self.mask_words), np.uint64)
        p = np.zeros(E, np.int64)
        phi_sum = np.zeros(E, np.uint64)
        self._check(self._lib.tq_tbe_read(self._h, masks.ctypes.data, p.ctypes.data, phi_sum.ctypes.data))
        return mask_bits(masks, self.ntaxa), p, phi_sum

    def stats(self) -> dict:
        """Counters of the device path: trees per chunk, chunks launched since create / reset."""
        out = np.zeros(2, np.int64)
        self._check(self._lib.tq_tbe_stats(self._h, out.ctypes.data))
        return {"chunk_trees": int(out[0]), "chunks": int(out[1])}

    def supports(self) -> np.ndarray:
        """TBE per branch, f64[E] (the only float of this module); 0 without replicates."""
        _, p, phi_sum = self.raw()
        n = self.ntrees
        if not n:
            return np.zeros(len(p), np.float64)
        return 1.0 - phi_sum.astype(np.float64) / (n * (p - 1).astype(np.float64))

    def percents(self) -> np.ndarray:
        """The integer percent of every branch, i64[E]."""
        _, p, phi_sum = self.raw()
        n = self.ntrees
        return np.array([percent(int(s), int(q), n) for s, q in zip(phi_sum, p)], np.int64)

    def map_supports(self, newick: str | None = None, samples=None) -> str:
        """The reference tree with the TBE percent of each branch as the label of the node where
        `Consensus.map_supports` puts its percent.  `newick` (with `samples`) is another text of the same tree -- its
        shape, rooting, child order and tip labels are kept; default: the text (and `samples`) given at create, or
        numeric tips for a parent array."""
        if newick is None:
            newick = self._newick if self._newick is not None else _parent_to_newick(self._parent, self.ntaxa)
            samples = self.samples if self._newick is not None else None
        masks, _, _ = self.raw()
        with TransferSupport(self.ntaxa, newick, samples) as other:
            if not np.array_equal(other.raw()[0], masks):
                raise ValueError("the tree to write on does not have the branches of the reference tree")
        return write_split_labels(newick, samples, masks, [str(x) for x in self.percents()])


def transfer_supports(tree: str, newicks, samples=None, engine=None) -> str:
    """`tree` with the transfer bootstrap percents of `newicks` on its branches, in one call; tips carry the names of
    `samples` when given (in `tree` and in `newicks`)."""
    newicks = [newicks] if isinstance(newicks, str) else list(newicks)
    if not newicks:
        raise ValueError("no trees")
    _, T, _ = newick_to_parent(tree, samples)
    with TransferSupport(T, tree, samples, engine=engine) as acc:
        acc.add_newick(newicks, samples)
        return acc.map_supports()

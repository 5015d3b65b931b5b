"""Majority-rule consensus with split supports: what `tetrad consensus` reports (tetrad/src/cli_consensus.py:87-132).

The reference re-infers a supertree per bootstrap replicate, lets toytree count in how many trees each split occurs and
returns the majority-rule tree with edge supports, or maps the supports onto a tree the user names.  Here the splits
are counted by the library (`tq_cons_*`, tetrad_amd/csrc/consensus.hpp): exactly, as integers, on the host
(`Consensus(ntaxa)`) or on the device (`Consensus(ntaxa, engine=...)`: HIP kernels build every tree's split masks and
count them in a hash table; every count follows a comparison of the full mask).  Both give identical tables and trees.

Definitions:
  split      an internal edge with at least 2 taxa on both sides; its side is the one without taxon 0
  table      count descending, then the side ascending as one integer (taxon T-1 most significant)
  consensus  walking the table, a split is accepted when count >= min_count and it is compatible with every accepted
             split; min_count = max(1, ceil(min_freq x ntrees)) with min_freq read as its shortest decimal text, and
             min_freq = 0.5 additionally requires 2 x count > ntrees (strict majority)
  newick     root = the maximal sides and the uncovered tips, children by smallest taxon, numeric tips, an accepted
             split labelled with its integer percent (200 count + ntrees) // (2 ntrees), no branch lengths

Deviations from the reference: the byte format of toytree's consensus newick (float supports, branch lengths) is not
reproduced; ties between conflicting splits below 50 % are broken by the fixed table order, not by toytree's dict order.
"""
from __future__ import annotations

import ctypes
from fractions import Fraction
from pathlib import Path

import numpy as np

from ._handle import Handle, grow_text, mask_bits
from .concordance import TreeSetInput, newick_to_parent, parse_newick, tree_to_parent


def min_count_for(min_freq: float, ntrees: int) -> int:
    """The integer threshold of `min_freq` over `ntrees` trees (module docstring, "consensus")."""
    f = Fraction(repr(float(min_freq)))
    if not 0 <= f <= 1:
        raise ValueError("min_freq must be within 0..1")
    need = f * int(ntrees)
    k = max(1, -((-need.numerator) // need.denominator))
    if f == Fraction(1, 2):
        k = max(k, int(ntrees) // 2 + 1)
    return k


def percent(count: int, ntrees: int) -> int:
    """The support label of a split seen in `count` of `ntrees` trees: the percent rounded half up, in integers."""
    return (200 * int(count) + int(ntrees)) // (2 * int(ntrees)) if ntrees else 0


class Consensus(TreeSetInput, Handle):
    """Split counts over a set of trees on the taxa 0..ntaxa-1, and the consensus built from them.

    ntaxa       4..4096
    max_splits  distinct splits the table may hold (default max(1024, 16 x ntaxa)); more is an error until `reset`
    engine      a `QuartetEngine`: the splits are counted on its device; None: on the host
    """

    _prefix = "tq_cons"

    def __init__(self, ntaxa: int, max_splits: int | None = None, engine=None):
        self.ntaxa, self.engine = int(ntaxa), engine
        self.max_splits = int(max_splits) if max_splits is not None else max(1024, 16 * self.ntaxa)
        self._create(self.ntaxa, self.max_splits, self._ctx())
        self.mask_words = (self.ntaxa + 63) // 64

    def _add(self, block, n_nodes, stride, stream):
        self._check(self._lib.tq_cons_add(self._h, block.ctypes.data, n_nodes.ctypes.data, len(n_nodes), stride, stream))

    # -- reading --------------------------------------------------------------------------------------------
    @property
    def ntrees(self) -> int:
        n = ctypes.c_int64()
        self._check(self._lib.tq_cons_shape(self._h, None, None, ctypes.byref(n), None))
        return n.value

    def raw(self):
        """(masks u64[n, W], counts i64[n], ntrees) in table order; waits for the device."""
        nt, ns = ctypes.c_int64(), ctypes.c_int64()
        self._check(self._lib.tq_cons_shape(self._h, None, None, ctypes.byref(nt), ctypes.byref(ns)))
        masks = np.zeros((ns.value, self.mask_words), np.uint64)
        counts = np.zeros(ns.value, np.int64)
        self._check(self._lib.tq_cons_read(self._h, masks.ctypes.data, counts.ctypes.data))
        return masks, counts, nt.value

    def splits(self):
        """(masks bool[n, ntaxa] = the side without taxon 0, counts i64[n], ntrees) in table order."""
        masks, counts, ntrees = self.raw()
        return mask_bits(masks, self.ntaxa), counts, ntrees

    def frequencies(self) -> np.ndarray:
        """count / ntrees per split of the table (the only float of this module besides `min_freq`)."""
        _, counts, ntrees = self.raw()
        return counts / ntrees if ntrees else counts.astype(np.float64)

    def stats(self) -> dict:
        """Counters of the device path since create / reset: trees per chunk, chunks launched, entries of the device
        table, entries of the host map, splits that lost a hash collision (counted on the host), hash bits."""
        out = np.zeros(6, np.int64)
        self._check(self._lib.tq_cons_stats(self._h, out.ctypes.data))
        keys = ("chunk_trees", "chunks", "device_entries", "host_entries", "unresolved", "hash_bits")
        return dict(zip(keys, (int(x) for x in out)))

    def tree_min_count(self, min_count: int) -> str:
        """The consensus newick for an integer threshold."""
        return grow_text(lambda out, cap, written: self._lib.tq_cons_tree(self._h, int(min_count), out, cap, written),
                         16 * self.ntaxa + 64, self._check)

    def tree(self, min_freq: float = 0.5) -> str:
        """The consensus newick (numeric tips; `qmc.relabel_tree` gives names and leaves the supports alone):
        majority rule at the default 0.5, the greedy extended rule with the fixed table order below it."""
        return self.tree_min_count(min_count_for(min_freq, self.ntrees))

    def support_of(self, newick_or_parent, samples=None):
        """(counts i64[E], masks bool[E, ntaxa]) of the splits of one given tree (newick text or a parent array), masks
        ascending: in how many added trees each occurs, 0 for a split seen in none."""
        par = tree_to_parent(newick_or_parent, self.ntaxa, samples)[0]
        cap = max(1, self.ntaxa - 3)
        counts = np.zeros(cap, np.int64)
        masks = np.zeros((cap, self.mask_words), np.uint64)
        e = ctypes.c_int64()
        self._check(self._lib.tq_cons_support(self._h, par.ctypes.data, par.shape[0], counts.ctypes.data,
                                              masks.ctypes.data, ctypes.byref(e)))
        return counts[:e.value].copy(), mask_bits(masks[:e.value], self.ntaxa)

    def map_supports(self, newick: str, samples=None) -> str:
        """The given tree (its own shape, rooting, child order and tip labels) with the percent support of each of its
        splits as the label of the first node in preorder whose clade is one side of the edge (where
        `Concordance.to_newick` puts its comments).  Branch lengths and labels of internal nodes are dropped."""
        counts, masks = self.support_of(newick, samples)           # validates; the writer walks the text's own order
        ntrees = self.ntrees
        return write_split_labels(newick, samples, masks, [str(percent(c, ntrees)) for c in counts])


def write_split_labels(newick: str, samples, masks, labels) -> str:
    """`newick` (its own shape, rooting, child order and tip labels) with `labels[e]` written behind the first node in
    preorder whose clade is one side of split `e` (`masks` bool[E, ntaxa]).  Branch lengths and labels of internal nodes
    are dropped.  The writer of `Consensus.map_supports` and `tbe.TransferSupport.map_supports`."""
    _, T, names = newick_to_parent(newick, samples)
    par, label, nkids = parse_newick(newick)                       # node 0 = the root, children in order of appearance
    n = len(par)
    taxon_of = {str(name): t for t, name in enumerate(names)}
    kids = [[] for _ in range(n)]
    for v in range(1, n):
        kids[par[v]].append(v)
    root = 0
    clade = [0] * n
    for v in range(n - 1, -1, -1):                                 # a child always follows its parent
        if not nkids[v]:
            clade[v] = 1 << taxon_of[label[v]]
        if v:
            clade[par[v]] |= clade[v]
    full = (1 << T) - 1
    where = {}
    for e in range(len(labels)):
        m = sum(1 << int(t) for t in np.flatnonzero(masks[e]))
        where[m] = where[full ^ m] = e
    placed, used = {}, set()
    for v in range(n):                                             # order of appearance = preorder
        e = where.get(clade[v])
        if nkids[v] and e is not None and e not in used:
            placed[v] = e
            used.add(e)

    def name(v):
        s = str(label[v])
        return "'" + s.replace("'", "''") + "'" if any(ch in s for ch in " (),:;[]'") else s

    out, stack = [], [(root, 0)]
    while stack:
        v, i = stack.pop()
        if not nkids[v]:
            out.append(name(v))
            continue
        if i == 0:
            out.append("(")
        if i == len(kids[v]):
            out.append(")")
            if v in placed:
                out.append(labels[placed[v]])
            continue
        if i:
            out.append(",")
        stack.append((v, i + 1))
        stack.append((kids[v][i], 0))
    return "".join(out) + ";"


def consensus_tree(newicks, min_freq: float = 0.5, samples=None, engine=None) -> str:
    """The consensus of newick trees in one call; tips carry the names of `samples` when given (in and out)."""
    from .qmc import relabel_tree
    newicks = [newicks] if isinstance(newicks, str) else list(newicks)
    if not newicks:
        raise ValueError("no trees")
    _, T, _ = newick_to_parent(newicks[0], samples)
    with Consensus(T, engine=engine) as acc:
        acc.add_newick(newicks, samples)
        nwk = acc.tree(min_freq)
    return relabel_tree(nwk, samples) if samples is not None else nwk


def run_consensus(qrt_files, ntaxa: int, weights: int = 0, min_snps: int = 0, min_ratio: float = 1.0, tree=None,
                  min_freq: float = 0.5, samples=None, engine=None) -> str:
    """cli_consensus.py:87-132 on explicit paths instead of a Project: one supertree per quartets TSV of `qrt_files`
    (`qmc.infer_supertree_exact` under `weights`, `min_snps`, `min_ratio`; seed = the file's index), their splits
    counted, and either the consensus tree at `min_freq` or, when `tree` (newick text or a path to it) is given, that
    tree with the supports mapped onto its edges.  Tips are sample names when `samples` is given (`tree` then carries
    names too), taxon numbers otherwise."""
    from .qmc import infer_supertree_exact, relabel_tree
    from .qmc_format import read_quartets_tsv
    if isinstance(qrt_files, (str, Path)):
        qrt_files = [qrt_files]
    with Consensus(ntaxa, engine=engine) as acc:
        trees = []
        for i, f in enumerate(qrt_files):
            rqrts, rscor, rstat = read_quartets_tsv(f)
            trees.append(infer_supertree_exact(rqrts, rscor, rstat, ntaxa, weights, min_snps, min_ratio, seed=i))
        acc.add_newick(trees)
        if tree is not None:
            text = str(tree)
            if not text.lstrip().startswith("("):
                text = Path(text).read_text()
            return acc.map_supports(text, samples)
        nwk = acc.tree(min_freq)
    return relabel_tree(nwk, samples) if samples is not None else nwk

"""Quartet supertree: the step right after the hot path (second half).

The reference writes the wQMC input file and shells out to a prebuilt binary
(tetrad/src/run_inference.py:146-166 `run_qmc`, :330-357 `infer_supertree`).  Here the tree comes from the
library's own weighted Quartet MaxCut (`tq_qmc_tree`, host C++, written from the published method -- the
reference's binary has no source and is never executed; parity with it is unpinned by construction).
Tip labels are the taxon numbers, as in the file the reference's `relabel_tree` (:169-181) post-processes.
"""
from __future__ import annotations

import collections
import ctypes
from pathlib import Path

import numpy as np

from ._handle import Handle, grow_text
from .concordance import parent_block, tree_to_parent, trees_to_parents


def qmc_tree(splits: np.ndarray, weights=None, ntaxa: int | None = None, seed: int = 0) -> str:
    """Newick of the supertree of quartets `splits` u32[n,4] ("a,b|c,d" per row) with optional weights."""
    from . import _lib
    lib = _lib.load()
    sp = np.ascontiguousarray(splits, dtype=np.uint32).reshape(-1, 4)
    n = sp.shape[0]
    if ntaxa is None:
        ntaxa = int(sp.max()) + 1 if n else 1
    w = None if weights is None else np.ascontiguousarray(weights, dtype=np.float64).reshape(-1)
    if w is not None and w.shape[0] != n:
        raise ValueError("weights must have one entry per quartet")

    def fail(rc):
        raise _lib.TetradHipError(rc, "tq_qmc_tree")

    return grow_text(lambda out, cap, written: lib.tq_qmc_tree(sp.ctypes.data, None if w is None else w.ctypes.data, n,
                                                               int(ntaxa), int(seed) & (2**64 - 1), out, cap, written),
                     16 * int(ntaxa) + 64, fail)


def qmc_splits(rqrts, rscor, rstat, weights: int = 0, min_snps: int = 0, min_ratio: float = 1.0):
    """The rows `qmc_format.qmc_lines` would write, as arrays: (splits u32[n,4], weights f64[n]) -- same filters, same
    weight strategies, the weight as its "%.5f" text reads back -- without producing or parsing text."""
    from . import _lib
    lib = _lib.load()
    if weights not in (0, 1, 2, 3):
        raise ValueError(f"no weight strategy {weights}")
    q = np.ascontiguousarray(rqrts, dtype=np.uint32).reshape(-1, 4)
    st = np.ascontiguousarray(rstat, dtype=np.uint32).reshape(-1, 2)
    sc = np.ascontiguousarray(rscor, dtype=np.float64).reshape(-1, 3)
    n = q.shape[0]
    sp = np.empty((n, 4), np.uint32)
    w = np.empty(n, np.float64)
    kept = ctypes.c_int64()
    rc = lib.tq_qmc_splits(q.ctypes.data, st.ctypes.data, sc.ctypes.data, n, int(weights), int(min_snps), float(min_ratio),
                           sp.ctypes.data, w.ctypes.data, ctypes.byref(kept))
    if rc != 0:
        raise _lib.TetradHipError(rc, "tq_qmc_splits")
    return sp[:kept.value], w[:kept.value]


def parse_qmc_lines(lines) -> tuple[np.ndarray, np.ndarray]:
    """"a,b|c,d:w" lines (run_inference.py:305) -> (splits u32[n,4], weights f64[n])."""
    sp, w = [], []
    for ln in lines:
        ln = ln.decode() if isinstance(ln, bytes) else ln
        ln = ln.strip()
        if not ln:
            continue
        left, _, weight = ln.partition(":")
        ab, cd = left.split("|")
        sp.append([int(x) for x in ab.split(",")] + [int(x) for x in cd.split(",")])
        w.append(float(weight) if weight else 1.0)
    return np.array(sp, dtype=np.uint32).reshape(-1, 4), np.array(w, dtype=np.float64)


def run_qmc(qmc_in_file: Path, qmc_out_file: Path, use_weights: bool, ntaxa: int | None = None, seed: int = 0) -> None:
    """run_inference.py:146-166 without the external binary: reads the wQMC input file, writes the newick."""
    with open(qmc_in_file) as f:
        splits, weights = parse_qmc_lines(f)
    nwk = qmc_tree(splits, weights if use_weights else None, ntaxa, seed)
    Path(qmc_out_file).write_text(nwk + "\n")


def infer_supertree_from_arrays(rqrts, rscor, rstat, ntaxa: int, weights: int = 0, min_snps: int = 0,
                                min_ratio: float = 1.0, seed: int = 0) -> str:
    """run_inference.py:330-357 straight from the result arrays of a replicate: the wQMC lines of
    `tq_format_qmc` (same filters and weight strategies as :254-305), then the tree."""
    splits, w = qmc_splits(rqrts, rscor, rstat, weights, min_snps, min_ratio)
    return qmc_tree(splits, w if weights else None, ntaxa, seed)


#: one record of `Supertree.fit` per tree: the six integers of `tq_stree_fit`, and k_satisfied / (k_satisfied + k_violated)
FIT_DTYPE = np.dtype([("k_satisfied", np.uint64), ("k_violated", np.uint64), ("k_unresolved", np.uint64),
                      ("n_satisfied", np.uint64), ("n_violated", np.uint64), ("n_unresolved", np.uint64),
                      ("fraction", np.float64)])
LastFit = collections.namedtuple("LastFit", "results chosen seeds")
#: what `Supertree.polish` did: interchanges applied and sum of gains (Python ints) per round that moved, and whether the
#: last scan found no candidate
PolishTrace = collections.namedtuple("PolishTrace", "moves gains converged")


class Supertree(Handle):
    """Exact quartet supertree accumulator (`tq_stree_*`): Quartet MaxCut level by level on
    integer graph weights.  Rows are added on the host (`add`) or where the engine wrote them (`add_dev_ptrs`, needs
    `engine`); `tree(seed)` gives the newick with numeric tips.  The host and the device execution give the same
    string for the same rows, in any order and over any number of adds.

    ntaxa     taxa 0..ntaxa-1 (with an engine: 4..1024)
    capacity  rows that may be added between two resets
    weights, min_snps, min_ratio   as `qmc_splits`
    search    rule of the cut search: "f64" (default) = the multi-start search on the cells as doubles, on the host;
              "exact" = the all-integer rule of DESIGN.md section 16, which device rows run in a kernel.  Each rule
              gives one string from both back ends; the two rules draw different starts and may differ from each other.
    """

    SEARCH = {"f64": 0, "exact": 1}
    _prefix = "tq_stree"

    def __init__(self, ntaxa: int, capacity: int, weights: int = 0, min_snps: int = 0, min_ratio: float = 1.0, engine=None,
                 search: str = "f64"):
        if weights not in (0, 1, 2, 3):
            raise ValueError(f"no weight strategy {weights}")
        if search not in self.SEARCH:
            raise ValueError(f"search must be 'f64' or 'exact', got {search!r}")
        self.ntaxa, self.capacity, self.engine = int(ntaxa), int(capacity), engine
        self.levels = 0
        self.last_fit = None
        self.last_polish = None
        self._chosen_stats = None
        self._create(self.ntaxa, self.capacity, int(weights), int(min_snps), float(min_ratio), self._ctx())
        self.search = "f64"
        if search != "f64":
            self.set_search(search)

    def set_search(self, search: str):
        """The rule of the following `tree` calls: "f64" or "exact"."""
        if search not in self.SEARCH:
            raise ValueError(f"search must be 'f64' or 'exact', got {search!r}")
        self._check(self._lib.tq_stree_set_search(self._h, self.SEARCH[search]))
        self.search = search

    def add(self, rqrts, rscor, rstat, flags=None):
        """Host rows: quartets u32[n,4], scores f64[n,3], rstat u32[n,2] = {topology, nsnps}, flags u8[n] or None."""
        q = np.ascontiguousarray(rqrts, dtype=np.uint32).reshape(-1, 4)
        sc = np.ascontiguousarray(rscor, dtype=np.float64).reshape(-1, 3)
        st = np.ascontiguousarray(rstat, dtype=np.uint32).reshape(-1, 2)
        n = q.shape[0]
        if sc.shape[0] != n or st.shape[0] != n:
            raise ValueError("quartets, scores and rstat must have one row per quartet")
        fl = None
        if flags is not None:
            fl = np.ascontiguousarray(flags, dtype=np.uint8).reshape(-1)
            if fl.shape[0] != n:
                raise ValueError("flags must have one entry per quartet")
        self._check(self._lib.tq_stree_add(self._h, q.ctypes.data, st.ctypes.data, sc.ctypes.data,
                                           None if fl is None else fl.ctypes.data, n))

    def add_dev_ptrs(self, d_quartets: int, d_rstat: int, d_rscor: int, d_flags: int, n: int, stream: int = 0):
        """Device rows by address, enqueued on `stream` (a hipStream_t as int)."""
        self._check(self._lib.tq_stree_add_dev(self._h, d_quartets, d_rstat, d_rscor, d_flags or None, int(n),
                                               stream or None))

    def counts(self):
        """(kept rows, skipped rows, sum of the integer weights k) of everything added so far."""
        kept, skipped, sum_k = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_uint64()
        self._check(self._lib.tq_stree_graph(self._h, None, None, ctypes.byref(kept), ctypes.byref(skipped),
                                             ctypes.byref(sum_k)))
        return kept.value, skipped.value, sum_k.value

    def graph(self):
        """The root graph: (G u64[T,T], B u64[T,T], kept, skipped, sum_k)."""
        G = np.empty((self.ntaxa, self.ntaxa), np.uint64)
        B = np.empty((self.ntaxa, self.ntaxa), np.uint64)
        kept, skipped, sum_k = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_uint64()
        self._check(self._lib.tq_stree_graph(self._h, G.ctypes.data, B.ctypes.data, ctypes.byref(kept),
                                             ctypes.byref(skipped), ctypes.byref(sum_k)))
        return G, B, kept.value, skipped.value, sum_k.value

    def rows(self):
        """The kept rows: (splits u32[n,4] = "a,b|c,d", k u64[n]); weight = k / 10^5."""
        n = ctypes.c_int64()
        self._check(self._lib.tq_stree_rows(self._h, None, None, ctypes.byref(n)))
        sp = np.empty((n.value, 4), np.uint32)
        k = np.empty(n.value, np.uint64)
        self._check(self._lib.tq_stree_rows(self._h, sp.ctypes.data, k.ctypes.data, ctypes.byref(n)))
        return sp, k

    def _build(self, seed: int, stream: int) -> str:
        levels = ctypes.c_int64()
        nwk = grow_text(lambda out, cap, written: self._lib.tq_stree_build(self._h, int(seed) & (2**64 - 1), stream or None,
                                                                           out, cap, written, ctypes.byref(levels)),
                        16 * self.ntaxa + 64, self._check)
        self.levels = levels.value
        return nwk

    def tree(self, seed: int = 0, stream: int = 0, restarts: int = 1, polish: bool = False) -> str:
        """Newick of the rows added so far (numeric tips); `self.levels` = levels of the recursion.  Device rows: the
        passes run on `stream`.
        `restarts=N` > 1: builds with the seeds seed, seed + 1, ..., seed + N - 1, fits the N trees to the rows in one
        `tq_stree_fit` and returns the tree with the largest k_satisfied (ties: the smaller k_violated, then the lowest
        seed).  `self.last_fit` then holds `LastFit(results, chosen, seeds)`; `levels` and `level_stats()` describe the
        chosen seed's build.
        `polish=True`: every build goes through `polish` (its default rounds) before the fit that chooses among the
        restarts; `self.last_polish` holds the returned tree's `PolishTrace` (None after a call without polish).  Off, the
        calls are the ones above."""
        restarts = int(restarts)
        if restarts < 1:
            raise ValueError("restarts must be at least 1")
        self._chosen_stats = None
        self.last_polish = None
        if polish and self.ntaxa < 4:
            raise ValueError("polish needs a tree of at least 4 taxa")
        if restarts == 1:
            nwk = self._build(seed, stream)
            if polish:
                nwk, self.last_polish = self.polish(nwk, stream=stream)
            return nwk
        if self.ntaxa < 4:
            raise ValueError("restarts need a tree of at least 4 taxa to score")
        seeds = [int(seed) + i for i in range(restarts)]
        builds = []
        for s in seeds:
            nwk, trace = self._build(s, stream), None
            if polish:
                nwk, trace = self.polish(nwk, stream=stream)
            builds.append((nwk, self.levels, self.level_stats(), trace))
        res = self.fit([b[0] for b in builds], stream=stream)
        chosen = min(range(restarts), key=lambda i: (-int(res["k_satisfied"][i]), int(res["k_violated"][i]), i))
        self.last_fit = LastFit(res, chosen, seeds)
        nwk, self.levels, self._chosen_stats, trace = builds[chosen]
        if polish:
            self.last_polish = trace
        return nwk

    def _parent_of(self, tree, samples):
        """One tree as `fit` takes it -> parent array i32."""
        return tree_to_parent(tree, self.ntaxa, samples)[0]

    def nni_scan(self, tree, samples=None, stream: int = 0) -> np.ndarray:
        """The quartet-fit weights of every nearest-neighbour interchange of `tree` (a newick string or a parent array,
        as `fit` takes one) in one pass over the kept rows (`tq_stree_nni_scan`).  One record
        per internal edge of the prepared tree: `eligible`; `corners` u64[4, W] = the taxon masks X1, X2, Y1, Y2 (bit x
        of word x // 64; `corner_ints` turns a record's into Python ints); `w0`, `w1`, `w2` = the weight of the kept
        rows with a taxon in every corner that display the tree's split X1 X2 | Y1 Y2, X1 Y1 | X2 Y2 and X1 Y2 | X2 Y1.
        The neighbour of alternative j scores k_satisfied - w0 + wj.  Device rows: the kernels run on `stream`."""
        par = self._parent_of(tree, samples)
        W = (self.ntaxa + 63) // 64
        cap = max(self.ntaxa - 3, 1)
        n = ctypes.c_int64()
        elig = np.zeros(cap, np.uint8)
        corners = np.zeros((cap, 4, W), np.uint64)
        w = np.zeros((cap, 3), np.uint64)
        self._check(self._lib.tq_stree_nni_scan(self._h, par.ctypes.data, len(par), stream or None, ctypes.byref(n),
                                                elig.ctypes.data, corners.ctypes.data, w.ctypes.data))
        E = n.value
        out = np.zeros(E, np.dtype([("eligible", np.bool_), ("corners", np.uint64, (4, W)), ("w0", np.uint64),
                                    ("w1", np.uint64), ("w2", np.uint64)]))
        out["eligible"] = elig[:E] != 0
        out["corners"] = corners[:E]
        out["w0"], out["w1"], out["w2"] = w[:E, 0], w[:E, 1], w[:E, 2]
        return out

    @staticmethod
    def corner_ints(record) -> list:
        """The four corner masks of one `nni_scan` record as Python ints (bit x = taxon x)."""
        return [sum(int(word) << (64 * i) for i, word in enumerate(m)) for m in record["corners"]]

    def polish(self, tree, max_rounds: int = 1000, samples=None, stream: int = 0):
        """Local search from `tree` on the quartet fit (`tq_stree_polish`): rounds of one
        `nni_scan` each, after which every interchange that raises k_satisfied and shares no node with a better one is
        applied, until none does or `max_rounds` rounds have moved.  Returns (newick with numeric tips,
        `PolishTrace(moves, gains, converged)`).  The rows stay as they are."""
        par = self._parent_of(tree, samples)
        max_rounds = int(max_rounds)
        if not 0 <= max_rounds <= 65536:
            raise ValueError("max_rounds must be 0..65536")
        rounds, conv = ctypes.c_int64(), ctypes.c_int()
        trace = np.zeros((max(max_rounds, 1), 2), np.uint64)
        nwk = grow_text(lambda out, cap, written: self._lib.tq_stree_polish(
            self._h, par.ctypes.data, len(par), max_rounds, stream or None, out, cap, written, trace.ctypes.data,
            ctypes.byref(rounds), ctypes.byref(conv)), 16 * self.ntaxa + 64, self._check)
        r = rounds.value
        return nwk, PolishTrace([int(x) for x in trace[:r, 0]], [int(x) for x in trace[:r, 1]], bool(conv.value))

    def fit(self, trees, samples=None, stream: int = 0) -> np.ndarray:
        """Quartet fit of `trees` against the kept rows (`tq_stree_fit`).  `trees`: a newick string,
        a list of newick strings, or parent arrays (one int32 array with tips 0..ntaxa-1 = the taxa and parent[root] =
        -1, or a list of them).  Tips are taxon numbers, or names through `samples` (as `concordance.newick_to_parent`).
        Returns one record per tree (`FIT_DTYPE`; a single newick string or parent array gives a single record): the
        weight k and the number n of the kept rows the tree displays (satisfied), contradicts (violated) and leaves in
        a polytomy (unresolved), and fraction = k_satisfied / (k_satisfied + k_violated), NaN when that is 0 / 0.
        Device rows: the kernels run on `stream`."""
        single = isinstance(trees, str) or (isinstance(trees, np.ndarray) and trees.ndim == 1) or (
            isinstance(trees, (list, tuple)) and len(trees) > 0 and np.isscalar(trees[0]) and not isinstance(trees[0], str))
        parents, n_nodes, stride = parent_block(trees_to_parents([trees] if single else trees, self.ntaxa, samples), 1)
        R = len(n_nodes)
        raw = np.zeros((R, 6), np.uint64)
        self._check(self._lib.tq_stree_fit(self._h, parents.ctypes.data, n_nodes.ctypes.data, R, stride,
                                           stream or None, raw.ctypes.data))
        out = np.zeros(R, FIT_DTYPE)
        for j, name in enumerate(FIT_DTYPE.names[:6]):
            out[name] = raw[:, j]
        den = out["k_satisfied"].astype(np.float64) + out["k_violated"].astype(np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            out["fraction"] = np.where(den > 0, out["k_satisfied"].astype(np.float64) / den, np.nan)
        return out[0] if single else out

    def level_stats(self) -> np.ndarray:
        """Of the last `tree` (with restarts: of the chosen seed's build): f64[levels,6] = {open nodes, live quartets,
        cells, graph ms, search ms, partition ms}."""
        if getattr(self, "_chosen_stats", None) is not None:
            return self._chosen_stats
        n = ctypes.c_int64()
        out = np.zeros((64, 6), np.float64)
        self._check(self._lib.tq_stree_level_stats(self._h, ctypes.byref(n), out.ctypes.data))
        return out[:n.value]


def infer_supertree_exact(rqrts, rscor, rstat, ntaxa: int, weights: int = 0, min_snps: int = 0, min_ratio: float = 1.0,
                          seed: int = 0, flags=None, search: str = "f64", restarts: int = 1, polish: bool = False) -> str:
    """`infer_supertree_from_arrays` on the exact path (host back end): the tree does not depend on the row order.
    `search`: the rule of the cut search, as `Supertree`; `restarts`, `polish`: as `Supertree.tree`."""
    n = np.asarray(rqrts).reshape(-1, 4).shape[0]
    with Supertree(ntaxa, n, weights, min_snps, min_ratio, search=search) as st:
        st.add(rqrts, rscor, rstat, flags)
        return st.tree(seed, restarts=restarts, polish=polish)


def relabel_tree(newick: str, samples) -> str:
    """The tree with the numeric tip labels replaced by sample names -- what run_inference.py:169-181 does with
    toytree.  `samples` maps the taxon number to its name (a dict, or a sequence indexed by taxon number)."""
    import re
    names = samples if hasattr(samples, "get") else dict(enumerate(samples))

    def sub(m):
        name = names.get(int(m.group(2)))
        if name is None:
            raise KeyError(f"no sample name for taxon {m.group(2)}")
        name = str(name)
        if re.search(r"[\s(),:;\[\]']", name):
            name = "'" + name.replace("'", "''") + "'"
        return m.group(1) + name

    return re.sub(r"([(,])(\d+)(?=[,):])", sub, newick)


def infer_supertree(qrts_file: Path, qmc_in_file: Path, qmc_out_file: Path, ntaxa: int, weights: int = 0, min_snps: int = 0,
                    min_ratio: float = 1.0, samples=None, seed: int = 0) -> str:
    """run_inference.py:330-357 on explicit paths instead of a Project: the quartets TSV -> shuffled wQMC input file
    (`qmc_format.write_qmc_format`) -> tree file (`run_qmc`) -> newick with sample names when `samples` is given
    (`relabel_tree`), numeric tips otherwise."""
    from .qmc_format import write_qmc_format
    write_qmc_format(qrts_file, qmc_in_file, weights, min_snps, min_ratio, seed=seed)      # :347
    run_qmc(qmc_in_file, qmc_out_file, bool(weights), ntaxa=ntaxa, seed=seed)              # :350
    nwk = Path(qmc_out_file).read_text().strip()
    return relabel_tree(nwk, samples) if samples is not None else nwk                      # :353

"""Quartet concordance statistics on a fixed tree: what `tetrad concordance` reports (tetrad/src/concordance.py).

For every nontrivial edge of a fixed tree (usually the species tree or a consensus tree) the resolved quartets it
induces are counted as concordant, as one of the two discordant resolutions, or as uninformative; per tip the
concordant and discordant informative quartets that contain it are counted.  From those counts come QC (quartet
concordance), QD (skew of the two discordant resolutions), QI (share of informative quartets), the means of
nsnps / weight / score of the induced quartets, and QF (quartet fidelity) per tip (Pease et al. 2018).

The reference parses every quartets TSV line by line in Python (concordance.py:74-94, :165-230).  Here the rows are
counted by the library (`tq_conc_*`, tetrad_amd/csrc/concordance.hpp): on host arrays (`Concordance.add`, no device
needed) or on device arrays right where the engine wrote them (`Concordance.add_dev`, a HIP kernel, asynchronous;
`replicates.ReplicateRunner(concordance=...)` feeds every replicate this way without any D2H).

Deviations from the reference (DESIGN.md section 11 has the reasons):
  1. the three scores are sorted numerically (the reference sorts their strings, :82, which picks the wrong
     numerator of `score` when the scores have different numbers of integer digits);
  2. `min_snps` is taken as max(1, min_snps): rows without data are uninformative;
  3. several replicates are plain sums over all rows (the reference adds one tree object to itself, :238-244, :293);
  4. QF is credited to the taxon itself (the reference indexes `tree[tip]` by taxon number, :199, :206);
  5. QI and QF are NaN where their denominator is zero (the reference raises ZeroDivisionError for QF);
  6. multifurcations use the general edge rule: a quartet is induced on edge (u, v) when one pair lies in two
     different subtrees off u and the other pair in two different subtrees off v (other than through the edge);
     quartets whose four taxa meet at one node are induced on no edge.
Rows with a taxon >= T, a repeated taxon, a topology > 2 or the flags TQ_FLAG_BAD_INDEX / TQ_FLAG_INVALID_DIAGNOSTIC
are counted in `skipped` only.
"""
from __future__ import annotations

import ctypes
from math import log
from pathlib import Path

import numpy as np

from ._handle import Handle, mask_bits

STATS = ["QC", "QD", "QI", "nsnps", "weights", "scores", "conc", "disc1", "disc2", "nu", "nqrts"]


# -- newick ----------------------------------------------------------------------------------------------------
def parse_newick(text: str):
    """Newick text -> (parent list, label list): node 0 is the root, labels of internal nodes are kept (support
    values) but not interpreted.  Quoted labels ('' = a quote), branch lengths and [comments] are handled."""
    s = text.strip()
    parent, label, nkids = [-1], [None], [0]
    cur, i, n = 0, 0, len(s)

    def new(p):
        parent.append(p)
        label.append(None)
        nkids.append(0)
        nkids[p] += 1
        return len(parent) - 1

    while i < n:
        ch = s[i]
        if ch.isspace():
            i += 1
        elif ch == "[":
            j = s.find("]", i)
            if j < 0:
                raise ValueError("newick: unterminated [comment]")
            i = j + 1
        elif ch == "(":
            cur = new(cur)
            i += 1
        elif ch == ",":
            if parent[cur] < 0:
                raise ValueError("newick: ',' outside parentheses")
            cur = new(parent[cur])
            i += 1
        elif ch == ")":
            if parent[cur] < 0:
                raise ValueError("newick: unbalanced ')'")
            cur = parent[cur]
            i += 1
        elif ch == ":":
            i += 1
            while i < n and s[i] not in ",():;[":
                i += 1
        elif ch == ";":
            break
        elif ch == "'":
            j, out = i + 1, []
            while True:
                k = s.find("'", j)
                if k < 0:
                    raise ValueError("newick: unterminated quoted label")
                out.append(s[j:k])
                if k + 1 < n and s[k + 1] == "'":
                    out.append("'")
                    j = k + 2
                    continue
                break
            label[cur] = "".join(out)
            i = k + 1
        else:
            j = i
            while j < n and s[j] not in ",():;[" and not s[j].isspace():
                j += 1
            label[cur] = s[i:j]
            i = j
    if cur != 0:
        raise ValueError("newick: unbalanced '('")
    return parent, label, nkids


def newick_to_parent(text: str, samples=None):
    """Newick text -> (parent int32[n], T, tip_names): nodes 0..T-1 are the taxa, internal nodes follow in order of
    appearance, parent[root] = -1.  Tip labels are taxon numbers, or names through `samples` (taxon number -> name:
    a dict or a sequence indexed by taxon number, as `qmc.relabel_tree` takes it).  Every taxon must be a tip
    exactly once; T >= 4."""
    parent, label, nkids = parse_newick(text)
    tips = [v for v in range(len(parent)) if nkids[v] == 0]
    if samples is not None:
        names = dict(samples) if hasattr(samples, "items") else dict(enumerate(samples))
        T = len(names)
        index = {str(name): int(t) for t, name in names.items()}
        if len(index) != T or sorted(index.values()) != list(range(T)):
            raise ValueError("samples must map the taxon numbers 0..T-1 to distinct names")

        def taxon(lab):
            if lab not in index:
                raise ValueError(f"tip {lab!r} is not a sample name")
            return index[lab]
    else:
        T = len(tips)

        def taxon(lab):
            if lab is None or not lab.isdigit():
                raise ValueError(f"tip label {lab!r} is not a taxon number (give `samples` for names)")
            return int(lab)
    taxa = [taxon(label[v]) for v in tips]
    if len(set(taxa)) != len(taxa):
        raise ValueError("a taxon appears more than once in the tree")
    if any(t >= T for t in taxa) or len(taxa) != T:
        missing = sorted(set(range(T)) - set(taxa))
        raise ValueError(f"the tree's tips must be exactly the taxa 0..{T - 1} (missing {missing[:10]}, "
                         f"out of range {[t for t in taxa if t >= T][:10]})")
    if T < 4:
        raise ValueError("a tree needs at least 4 taxa")
    new = {}
    for v, t in zip(tips, taxa):
        new[v] = t
    nxt = T
    for v in range(len(parent)):
        if nkids[v]:
            new[v] = nxt
            nxt += 1
    par = np.full(len(parent), -1, np.int32)
    for v, p in enumerate(parent):
        par[new[v]] = -1 if p < 0 else new[p]
    names = [None] * T
    for v, t in zip(tips, taxa):
        names[t] = label[v]
    return par, T, names


def tree_to_parent(tree, ntaxa=None, samples=None):
    """One tree, newick text or a parent array -> (parent i32[n], T, tip names).  Text of another taxon count than
    `ntaxa` is refused (None: the text decides); a parent array needs `ntaxa`."""
    if isinstance(tree, str):
        par, T, names = newick_to_parent(tree, samples)
        if ntaxa is not None and T != ntaxa:
            raise ValueError(f"{T} taxa, the accumulator has {ntaxa}")
        return par, T, names
    if ntaxa is None:
        raise ValueError("a parent array needs `ntaxa`")
    return np.ascontiguousarray(tree, dtype=np.int32).reshape(-1), int(ntaxa), [str(t) for t in range(int(ntaxa))]


def trees_to_parents(trees, ntaxa: int, samples=None) -> list:
    """Trees as `tree_to_parent` takes one (a single newick string stands for a list of one) -> their parent arrays;
    what is wrong with tree i is reported as "tree {i}: ..."."""
    parents = []
    for i, t in enumerate([trees] if isinstance(trees, str) else trees):
        try:
            parents.append(tree_to_parent(t, ntaxa, samples)[0])
        except ValueError as e:
            raise ValueError(f"tree {i}: {e}") from None
    return parents


def parent_block(parents, min_stride: int = 0):
    """Parent arrays of any lengths (a list or a generator) -> (block i32[R, stride] padded with -1, n_nodes i64[R],
    stride): how the library takes a set of trees."""
    arrs = [np.ascontiguousarray(p, dtype=np.int32).reshape(-1) for p in parents]
    n = np.array([a.shape[0] for a in arrs], np.int64)
    stride = max(int(n.max(initial=0)), min_stride)
    block = np.full((len(arrs), stride), -1, np.int32)
    for i, a in enumerate(arrs):
        block[i, :a.shape[0]] = a
    return block, n, stride


class TreeSetInput:
    """`add_parents` / `add_newick` of the accumulators over sets of trees on the taxa 0..`ntaxa`-1.  A class supplies
    `_add(block, n_nodes, stride, stream)`, the call of its tq_*_add on a block that is not empty, and may keep the
    `samples` given at create as the default of `add_newick`."""

    samples = None

    def _add_trees(self, parents, stream, *extra):
        block, n, stride = parent_block(parents)
        if len(n):
            self._add(block, n, stride, stream or None, *extra)

    def add_parents(self, parents, stream: int = 0):
        """Trees as parent arrays (nodes 0..ntaxa-1 the taxa, parent[root] = -1), each with its own node count.  All of
        them are validated before any is added.  With an engine the kernels run on `stream` (a hipStream_t)."""
        self._add_trees(parents, stream)

    def add_newick(self, strings, samples=None, stream: int = 0):
        """Trees as newick text: tips are taxon numbers, or names through `samples` (`newick_to_parent`; default: those
        given at create, where the accumulator takes them there)."""
        self.add_parents(trees_to_parents(strings, self.ntaxa, self.samples if samples is None else samples), stream)


# -- statistics (concordance.py:37-71, :246-281) ---------------------------------------------------------------------
def qc(conc, disc1, disc2) -> float:
    """QC as concordance.py:37-57: +-1 with one non-zero class, 1 + sum p log_z p for z = 2 or 3, 1.0 for none."""
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
    """QD as concordance.py:60-71."""
    if not disc1 + disc2:
        return 1.0
    return 1.0 - (abs(disc1 - disc2) / (disc1 + disc2))


def _div(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    out = np.full(np.broadcast(a, b).shape, np.nan)
    np.divide(a, b, out=out, where=b != 0)
    return out


class _TreeAccumulator(Handle):
    """What the accumulators of the library on one fixed tree share (`Concordance`, `scf.SiteConcordance`): the tree,
    the checks of device rows, the split masks and the annotated newick.  A subclass names its family of library
    functions in `_prefix` and passes `tq_*_create` its own arguments."""

    def __init__(self, tree, samples, ntaxa, engine, *create_args):
        self.newick = tree if isinstance(tree, str) else None
        par, T, names = tree_to_parent(tree, ntaxa if self.newick is None else None, samples)     # text decides its own T
        self.parent, self.T, self.names = par, T, names
        self.engine = engine
        self._create(par.ctypes.data, par.shape[0], T, *create_args, self._ctx())
        t, e, w = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
        self._check(self._fn("shape")(self._h, ctypes.byref(t), ctypes.byref(e), ctypes.byref(w)))
        self.n_edges, self.mask_words = e.value, w.value

    # -- helpers of the subclasses ------------------------------------------------------------------------------
    def _need_engine(self):
        if self.engine is None:
            raise ValueError("add_dev needs an accumulator created with an engine")

    def _dev_stream(self, rows, n: int, stream) -> int:
        """Checks device rows -- (tensor, elements per row, bytes per element) each, n rows -- and returns the handle
        of `stream` (default: the current stream of their device)."""
        import torch
        for t, width, size in rows:
            if not t.is_cuda or not t.is_contiguous() or t.element_size() != size or t.numel() != n * width:
                raise ValueError("device rows must be contiguous GPU tensors of matching shape and dtype")
        if stream is None:
            stream = torch.cuda.current_stream(rows[0][0].device)
        return stream.cuda_stream if hasattr(stream, "cuda_stream") else int(stream)

    def _annotated_newick(self, split, edge_comment, tip_comment) -> str:
        """The input tree (as given: rooted or not) with `edge_comment(e)` after the node of each edge (the first
        node, in preorder, whose clade is one side of the edge; `split` bool [E,T]) and `tip_comment(t)`, which may be
        empty, after each tip; tips carry their names."""
        T, par = self.T, self.parent
        n = par.shape[0]
        kids = [[] for _ in range(n)]
        root = -1
        for v in range(n):
            if par[v] < 0:
                root = v
            else:
                kids[par[v]].append(v)
        clade = [0] * n
        order = [root]
        for v in order:
            order.extend(kids[v])
        for v in reversed(order):
            clade[v] = (1 << v) if v < T else 0
            for k in kids[v]:
                clade[v] |= clade[k]
        full = (1 << T) - 1
        where = {}
        for e in range(self.n_edges):
            m = int(sum(1 << int(t) for t in np.flatnonzero(split[e])))
            where[m] = where[full ^ m] = e
        placed, used = {}, set()
        for v in order:
            e = where.get(clade[v])
            if v >= T and e is not None and e not in used:
                placed[v] = e
                used.add(e)

        def name(t):
            s = str(self.names[t])
            return "'" + s.replace("'", "''") + "'" if any(ch in s for ch in " (),:;[]'") else s

        # children before parents, without recursion (a caterpillar of 4096 taxa is 4095 levels deep)
        text = {}
        for v in reversed(order):
            if v < T:
                text[v] = name(v) + tip_comment(v)
                continue
            s = "(" + ",".join(text.pop(k) for k in kids[v]) + ")"
            if v in placed:
                s += edge_comment(placed[v])
            text[v] = s
        return text[root] + ";"


class Concordance(_TreeAccumulator):
    """Concordance counters of resolved quartet rows on one fixed tree.

    tree      newick text (tips = taxon numbers, or names through `samples`), or a parent array with `ntaxa`
    engine    a `QuartetEngine` for device adds (`add_dev`); None: host adds only
    """

    _prefix = "tq_conc"

    def __init__(self, tree, *, samples=None, ntaxa: int | None = None, min_snps: int = 0, min_ratio: float = 1.0,
                 engine=None):
        self.min_snps, self.min_ratio = int(min_snps), float(min_ratio)
        super().__init__(tree, samples, ntaxa, engine, self.min_snps, self.min_ratio)
        self._carry = None                         # totals merged from other ranks (`reduce`)

    def reset(self):
        super().reset()
        self._carry = None

    # -- adding rows ------------------------------------------------------------------------------------------
    def add(self, rqrts, rscor, rstat, flags=None):
        """Host rows: quartets u32[n,4], scores f64[n,3], rstat u32[n,2] = {topology, nsnps}, flags u8[n] or None."""
        q = np.ascontiguousarray(rqrts, dtype=np.uint32).reshape(-1, 4)
        sc = np.ascontiguousarray(rscor, dtype=np.float64).reshape(-1, 3)
        st = np.ascontiguousarray(rstat, dtype=np.uint32).reshape(-1, 2)
        n = q.shape[0]
        if sc.shape[0] != n or st.shape[0] != n:
            raise ValueError("quartets, scores and rstat must have the same number of rows")
        fl = None if flags is None else np.ascontiguousarray(flags, dtype=np.uint8).reshape(-1)
        if fl is not None and fl.shape[0] != n:
            raise ValueError("flags must have one entry per row")
        self._check(self._lib.tq_conc_add(self._h, q.ctypes.data, st.ctypes.data, sc.ctypes.data,
                                          None if fl is None else fl.ctypes.data, n))

    def add_dev_ptrs(self, d_quartets: int, d_rstat: int, d_rscor: int, d_flags: int, n: int, stream: int = 0):
        """Device rows by address, enqueued on `stream` (a hipStream_t as int)."""
        self._check(self._lib.tq_conc_add_dev(self._h, d_quartets, d_rstat, d_rscor, d_flags or None, int(n),
                                              stream or None))

    def add_dev(self, quartets, rstat, rscor, flags=None, stream=None):
        """Device rows as torch tensors on the engine's device: quartets int32/uint32 [n,4], rstat int32 [n,2],
        rscor float64 [n,3], flags uint8 [n] or None; enqueued on `stream` (default: the current stream)."""
        self._need_engine()
        n = int(quartets.shape[0]) if quartets.dim() == 2 else int(quartets.numel()) // 4
        rows = [(quartets, 4, 4), (rstat, 2, 4), (rscor, 3, 8)] + ([(flags, 1, 1)] if flags is not None else [])
        handle = self._dev_stream(rows, n, stream)
        self.add_dev_ptrs(quartets.data_ptr(), rstat.data_ptr(), rscor.data_ptr(),
                          flags.data_ptr() if flags is not None else 0, n, handle)

    # -- reading -----------------------------------------------------------------------------------------------
    def raw(self) -> dict:
        """The summed counters (waits for the device adds): edge_counts i64[E,6] = {nqrts, conc, disc1, disc2, nu,
        nsnps sum}, edge_sums f64[E,2] = {weight sum, score sum}, masks u64[E,W], tip_counts i64[T,2] = {QFc, QFd},
        skipped."""
        E, W, T = self.n_edges, self.mask_words, self.T
        counts = np.zeros((E, 6), np.int64)
        sums = np.zeros((E, 2), np.float64)
        masks = np.zeros((E, W), np.uint64)
        tips = np.zeros((T, 2), np.int64)
        skipped = ctypes.c_int64()
        self._check(self._lib.tq_conc_read(self._h, counts.ctypes.data, sums.ctypes.data, masks.ctypes.data,
                                           tips.ctypes.data, ctypes.byref(skipped)))
        out = dict(edge_counts=counts, edge_sums=sums, masks=masks, tip_counts=tips, skipped=int(skipped.value))
        if self._carry is not None:
            c = self._carry
            out["edge_counts"][:, 1:] += c["edge_counts"][:, 1:]
            out["edge_sums"] = c["edge_sums"] + out["edge_sums"]
            out["tip_counts"] += c["tip_counts"]
            out["skipped"] += c["skipped"]
        return out

    def reduce(self, group=None, dst: int = 0):
        """Sum the counters of every rank of `group` into rank `dst` (integer counters exactly, the float sums
        added in rank order); the other ranks are reset.  A process group of one rank is left as it is."""
        import torch
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) == 1:
            return
        world, rank = dist.get_world_size(group), dist.get_rank(group)
        r = self.raw()
        ints = np.concatenate([r["edge_counts"][:, 1:].ravel(), r["tip_counts"].ravel(), [r["skipped"]]]).astype(np.int64)
        flts = r["edge_sums"].ravel().copy()
        dev = torch.device("cuda", torch.cuda.current_device()) if dist.get_backend(group) == "nccl" else torch.device("cpu")
        ti, tf = torch.from_numpy(ints).to(dev), torch.from_numpy(flts).to(dev)
        gi = [torch.zeros_like(ti) for _ in range(world)] if rank == dst else None
        gf = [torch.zeros_like(tf) for _ in range(world)] if rank == dst else None
        dist.gather(ti, gi, dst=dst, group=group)
        dist.gather(tf, gf, dst=dst, group=group)
        self.reset()
        if rank != dst:
            return
        E, T = self.n_edges, self.T
        si = sum(g.cpu().numpy() for g in gi)
        sf = gf[0].cpu().numpy().copy()
        for g in gf[1:]:
            sf = sf + g.cpu().numpy()
        counts = np.zeros((E, 6), np.int64)
        counts[:, 1:] = si[:5 * E].reshape(E, 5)
        self._carry = dict(edge_counts=counts, edge_sums=sf.reshape(E, 2),
                           tip_counts=si[5 * E:5 * E + 2 * T].reshape(T, 2).copy(), skipped=int(si[-1]))

    def split_masks(self) -> np.ndarray:
        """bool [E, T]: the taxa on one side of each edge."""
        return mask_bits(self.raw()["masks"], self.T)

    def stats(self) -> dict:
        """Per edge: split (bool [E,T]), nqrts, conc, disc1, disc2, nu, QC, QD, QI and the means nsnps, weights,
        scores of the induced quartets; per tip: QFc, QFd, QF; and `skipped` (concordance.py:246-281)."""
        r = self.raw()
        c = r["edge_counts"]
        nq, conc, d1, d2, nu, nsn = (c[:, k] for k in range(6))
        induced = conc + d1 + d2 + nu
        qfc, qfd = r["tip_counts"][:, 0], r["tip_counts"][:, 1]
        return dict(
            split=mask_bits(r["masks"], self.T), nqrts=nq, conc=conc, disc1=d1, disc2=d2, nu=nu,
            QC=np.array([qc(int(a), int(b), int(d)) for a, b, d in zip(conc, d1, d2)], np.float64),
            QD=np.array([qd(int(a), int(b)) for a, b in zip(d1, d2)], np.float64),
            QI=1.0 - _div(nu, induced),
            nsnps=_div(nsn, induced), weights=_div(r["edge_sums"][:, 0], induced), scores=_div(r["edge_sums"][:, 1], induced),
            QFc=qfc, QFd=qfd, QF=_div(qfc, qfc + qfd), skipped=r["skipped"])

    def to_newick(self) -> str:
        """The input tree (as given: rooted or not) with the statistics as comments: "[&QC=..,QD=..,...]" after the
        node of each edge (the first node, in preorder, whose clade is one side of the edge), "[&QF=..]" after each
        tip; tips carry their names.  The byte format of toytree's write(features=...) is not reproduced."""
        st = self.stats()

        def fmt(k, e):
            return "%.6g" % float(st[k][e]) if k in ("QC", "QD", "QI", "nsnps", "weights", "scores") else str(int(st[k][e]))

        return self._annotated_newick(st["split"], lambda e: "[&" + ",".join(f"{k}={fmt(k, e)}" for k in STATS) + "]",
                                      lambda t: "[&QF=%.6g]" % float(st["QF"][t]))


def run_quartet_concordance(newick_file, qrt_files, min_snps: int = 0, min_ratio: float = 1.0, samples=None,
                            engine=None) -> Concordance:
    """concordance.py:284-301 on explicit paths instead of a Project: the fixed tree from `newick_file`, the rows of
    every quartets TSV in `qrt_files` (one path or a list; read with `qmc_format.read_quartets_tsv`) summed into one
    accumulator.  Returns the `Concordance` (`.stats()`, `.to_newick()`)."""
    from .qmc_format import read_quartets_tsv
    if isinstance(qrt_files, (str, Path)):
        qrt_files = [qrt_files]
    acc = Concordance(Path(newick_file).read_text(), samples=samples, min_snps=min_snps, min_ratio=min_ratio,
                      engine=engine)
    for f in qrt_files:
        rqrts, rscor, rstat = read_quartets_tsv(f)
        acc.add(rqrts, rscor, rstat)
    return acc

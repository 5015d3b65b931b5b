"""Species-tree mode: quartets of species resolved from pooled lineages.

The reference plans a sample-to-clade table (`imap`: schema.py:50-51, cli.py:8 `-i IMAP.txt`, parsed at
write_database.py:198-201) but would only use it to select samples.  Here it defines species: each species quartet is
resolved from the count matrices of all its lineage quartets, summed (`QuartetEngine.resolve_species`), and the
species tree comes from those rows through the same supertree step as a sample tree.  Full mode only.
"""
from __future__ import annotations

from itertools import combinations
from math import comb

import numpy as np

from . import qmc


def read_imap(path) -> dict[str, list[str]]:
    """The reference's imap file (write_database.py:198-201): whitespace-separated `clade sample` lines ->
    {clade: [samples in file order]}.  Blank lines and lines starting with '#' are skipped."""
    imap: dict[str, list[str]] = {}
    with open(path) as f:
        for n, line in enumerate(f, 1):
            parts = line.split()
            if not parts or parts[0].startswith("#"):
                continue
            if len(parts) != 2:
                raise ValueError(f"{path}:{n}: expected 'clade sample', got {line.strip()!r}")
            imap.setdefault(parts[0], []).append(parts[1])
    return imap


class SpeciesMap:
    """Sample -> species ids: `species_of` i32[T] (-1 = sample left out), `names` = clade names by species id."""

    def __init__(self, species_of, names):
        self.species_of = np.ascontiguousarray(species_of, dtype=np.int32)
        self.names = list(names)
        if len(self.names) < 4:
            raise ValueError(f"a species tree needs at least 4 clades, got {len(self.names)}")

    @property
    def K(self) -> int:
        return len(self.names)

    @property
    def sizes(self) -> np.ndarray:
        """Lineages per species."""
        sp = self.species_of[self.species_of >= 0]
        return np.bincount(sp, minlength=self.K)

    @classmethod
    def from_imap(cls, imap: dict, samples) -> "SpeciesMap":
        """Species ids in sorted clade-name order (what pandas groupby gives); samples not listed get -1."""
        samples = list(samples)
        index = {s: i for i, s in enumerate(samples)}
        if len(index) != len(samples):
            raise ValueError("sample names are not unique")
        names = sorted(imap)
        species_of = np.full(len(samples), -1, np.int32)
        owner: dict[str, str] = {}
        for k, clade in enumerate(names):
            for s in imap[clade]:
                if s not in index:
                    raise ValueError(f"imap clade {clade!r} lists unknown sample {s!r}")
                if s in owner and owner[s] != clade:
                    raise ValueError(f"sample {s!r} is in two clades: {owner[s]!r} and {clade!r}")
                owner[s] = clade
                species_of[index[s]] = k
        return cls(species_of, names)


def pooled_range_ok(S: int, sizes, alleles: bool = False) -> bool:
    """The library's range rule: pooled bins and nsnps are u32, so S x (product of the four largest species sizes)
    must stay below 2^32 (and no species may hold more than 255 lineages).  `sizes` are samples per species; with
    `alleles` (option ``species_alleles``) every sample is two lineages, so the sizes count double."""
    lin = 2 if alleles else 1
    top = sorted((lin * int(n) for n in sizes), reverse=True)[:4]
    return len(top) == 4 and top[0] <= 255 and int(S) * top[0] * top[1] * top[2] * top[3] < 2**32


def species_quartets(K: int, nquartets: int = 0, seed: int = 0) -> np.ndarray:
    """All C(K,4) species quartets in lexicographic order, or (nquartets > 0) that many distinct ones drawn
    uniformly, in lexicographic order."""
    total = comb(K, 4)
    if nquartets <= 0 or nquartets >= total:
        return np.array(list(combinations(range(K), 4)), dtype=np.uint32).reshape(-1, 4)
    from .combinations import unrank
    rng = np.random.default_rng(seed)
    ranks = np.sort(rng.choice(total, size=int(nquartets), replace=False)).astype(np.uint64)
    return np.ascontiguousarray(unrank(ranks, K), dtype=np.uint32)


def infer_species_tree(engine, species_map: SpeciesMap, nquartets: int = 0, weights: int = 0, min_snps: int = 0,
                       min_ratio: float = 1.0, seed: int = 0, return_rows: bool = False, alleles: bool = False):
    """Species tree (newick, clade names as tips) from the engine's resident replicate: the map is set on the engine,
    all C(K,4) species quartets (or `nquartets` sampled) are resolved from pooled lineages, then the weighted
    supertree of those rows is built and relabelled.  With `return_rows`, also (squartets, rstat, rscor, flags).

    With `alleles` the call runs under option ``species_alleles`` = 1: every sample is two
    haplotype lineages read from the IUPAC source, a heterozygote counting once for each of its bases.  The resident
    replicate must then come from `engine.bootstrap` (`bootstrap.identity_replicate` for the original matrix); the
    library's refusal is raised as it is.  The option is off again when the call returns."""
    if engine.S and not pooled_range_ok(engine.S, species_map.sizes, alleles):
        raise ValueError(f"pooled counts of {engine.S} sites exceed u32 for species sizes {sorted(species_map.sizes)[-4:]}"
                         " (S x product of the four largest must stay below 2^32, at most 255 lineages per species"
                         + ("; two lineages per sample)" if alleles else ")"))
    engine.set_species(species_map.species_of, species_map.K)
    sq = species_quartets(species_map.K, nquartets, seed)
    engine.set_option("species_alleles", int(bool(alleles)))
    try:
        rstat, rscor, flags = engine.resolve_species(sq)
    finally:
        engine.set_option("species_alleles", 0)
    nwk = qmc.infer_supertree_from_arrays(sq, rscor, rstat, species_map.K, weights=weights, min_snps=min_snps,
                                          min_ratio=min_ratio, seed=seed)
    tree = qmc.relabel_tree(nwk, species_map.names)
    return (tree, (sq, rstat, rscor, flags)) if return_rows else tree


def bootstrap_species_trees(engine, seqarr, spans, species_map: SpeciesMap, nboots: int, *, nquartets: int = 0,
                            alleles: bool = True, weights: int = 0, min_snps: int = 0, min_ratio: float = 1.0, seed=None,
                            rng=None, supertree: str = "device", consensus=None, include_original: bool = False,
                            search: str = "f64") -> list[str]:
    """Bootstrap species trees: `nboots` replicates of the loci of `seqarr` u8[T,S0] (ASCII, IUPAC codes) / `spans`
    i64[nloci,2], each built on the device, resolved in species mode and turned into a tree by the exact supertree
    (DESIGN.md sections 13 and 15).  Returns the newick strings in replicate order with the species numbers as tips
    (`qmc.relabel_tree(nwk, species_map.names)` names them); with `include_original` the tree of the original matrix
    (`bootstrap.identity_replicate`, no draw, supertree seed 0) comes first.

    Per replicate k the draws on one Generator (`rng`, else `default_rng(seed)`) are those of
    `bootstrap.draw_replicate`, in the reference's order, followed -- only when `nquartets` species quartets are
    sampled out of C(K,4) -- by one integer seed for `species_quartets`.  Then `engine.bootstrap` on a stream,
    `resolve_species_dev` into device buffers allocated once, and one of two back ends of the same exact rule, so both
    return the same string: ``supertree="device"`` feeds a `qmc.Supertree(K, Q, engine=engine)` where the rows were
    written, ``"host"`` copies the rows back for `qmc.infer_supertree_exact`; the supertree seed is k = 0..nboots-1.

    `alleles` (default) runs the species calls under option ``species_alleles``: both alleles of every genotype
    count, and `seed_ambig` has no influence.  With `alleles=False` the replicate's coin-resolved rows are pooled.
    `search` ("f64" or "exact") is the rule of the supertree's cut search, as `qmc.Supertree`; both back ends take it.
    `consensus` (a `consensus.Consensus(K)`) receives all trees through `add_newick` once they are in.  One rank,
    one plain loop: a species replicate is a few milliseconds.

    Per-sample trees: a map with `species_of = arange(T)` makes every sample a species of its own two alleles, which
    gives heterozygote-aware bootstrap trees of the samples themselves with no code of their own."""
    import torch
    from .bootstrap import draw_replicate, identity_replicate
    if supertree not in ("device", "host"):
        raise ValueError(f"supertree must be 'device' or 'host', got {supertree!r}")
    if search not in ("f64", "exact"):
        raise ValueError(f"search must be 'f64' or 'exact', got {search!r}")
    rng = np.random.default_rng(seed) if rng is None else np.random.default_rng(rng)
    K = species_map.K
    sampled = 0 < nquartets < comb(K, 4)
    Q = int(nquartets) if sampled else comb(K, 4)
    dev = torch.device(f"cuda:{engine.device_id}")
    stream = torch.cuda.Stream(dev)
    sid = stream.cuda_stream
    engine.set_source(seqarr, spans)
    mapped = False                  # the map goes in behind the first replicate: its T is checked against the resident data
    sq_all = None if sampled else species_quartets(K)
    with torch.cuda.stream(stream):
        dq = torch.empty((Q, 4), dtype=torch.int32, device=dev)
        if not sampled:
            dq.copy_(torch.from_numpy(sq_all.view(np.int32)))
        drs = torch.empty((Q, 2), dtype=torch.int32, device=dev)
        dsc = torch.empty((Q, 3), dtype=torch.float64, device=dev)
        dfl = torch.empty(Q, dtype=torch.uint8, device=dev)
    acc = qmc.Supertree(K, Q, weights, min_snps, min_ratio, engine=engine, search=search) if supertree == "device" else None
    trees = []
    engine.set_option("species_alleles", int(bool(alleles)))
    try:
        for k in ([None] if include_original else []) + list(range(nboots)):
            if k is None:
                identity_replicate(engine)
                sq = sq_all if not sampled else species_quartets(K, nquartets, 0)
                k = 0
            else:
                lidxs, seed_shuffle, seed_ambig = draw_replicate(engine.nloci, rng)
                sq = sq_all if not sampled else species_quartets(K, nquartets, int(rng.integers(2**31)))
                engine.bootstrap(lidxs, seed_shuffle, seed_ambig, sid)
            if not mapped:
                engine.set_species(species_map.species_of, K)
                mapped = True
            with torch.cuda.stream(stream):
                if sampled:
                    dq.copy_(torch.from_numpy(sq.view(np.int32)))
                engine.resolve_species_dev(dq.data_ptr(), Q, drs.data_ptr(), dsc.data_ptr(), dfl.data_ptr(), sid)
                if acc is not None:
                    acc.reset()
                    acc.add_dev_ptrs(dq.data_ptr(), drs.data_ptr(), dsc.data_ptr(), dfl.data_ptr(), Q, sid)
                    trees.append(acc.tree(seed=k, stream=sid))
                else:
                    rstat, rscor, flags = drs.cpu().numpy().view(np.uint32), dsc.cpu().numpy(), dfl.cpu().numpy()
                    trees.append(qmc.infer_supertree_exact(sq, rscor, rstat, K, weights, min_snps, min_ratio, seed=k,
                                                           flags=flags, search=search))
    finally:
        stream.synchronize()
        engine.set_option("species_alleles", 0)
        if acc is not None:
            acc.close()
    if consensus is not None:
        consensus.add_newick(trees)
    return trees

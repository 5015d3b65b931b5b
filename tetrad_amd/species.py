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


def pooled_range_ok(S: int, sizes) -> bool:
    """The library's range rule: pooled bins and nsnps are u32, so S x (product of the four largest species sizes)
    must stay below 2^32 (and no species may hold more than 255 lineages)."""
    top = sorted((int(n) for n in sizes), reverse=True)[:4]
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
                       min_ratio: float = 1.0, seed: int = 0, return_rows: bool = False):
    """Species tree (newick, clade names as tips) from the engine's resident replicate: the map is set on the engine,
    all C(K,4) species quartets (or `nquartets` sampled) are resolved from pooled lineages, then the weighted
    supertree of those rows is built and relabelled.  With `return_rows`, also (squartets, rstat, rscor, flags)."""
    if engine.S and not pooled_range_ok(engine.S, species_map.sizes):
        raise ValueError(f"pooled counts of {engine.S} sites exceed u32 for species sizes {sorted(species_map.sizes)[-4:]}"
                         " (S x product of the four largest must stay below 2^32, at most 255 lineages per species)")
    engine.set_species(species_map.species_of, species_map.K)
    sq = species_quartets(species_map.K, nquartets, seed)
    rstat, rscor, flags = engine.resolve_species(sq)
    nwk = qmc.infer_supertree_from_arrays(sq, rscor, rstat, species_map.K, weights=weights, min_snps=min_snps,
                                          min_ratio=min_ratio, seed=seed)
    tree = qmc.relabel_tree(nwk, species_map.names)
    return (tree, (sq, rstat, rscor, flags)) if return_rows else tree

"""Five-taxon site patterns per block of sites; DFOIL and partitioned D with a block jackknife.

A biallelic site of five taxa (t0 < t1 < t2 < t3 < t4) with no missing base has one of 15 unpolarised patterns: its
class is k = sum over i = 1..4 of [x_i != x_0] 2^(i-1).  `QuartetEngine.patterns_quintet_blocks` returns u32[Q,B,16]
rows per (set, block of sites): slot k = the count of class k, slot 0 their sum.  Sites with three or four bases and
invariant sites count nowhere.

A statistic is (L - R) / (L + R) with L and R sums of patterns.  A pattern is written as five letters A/B in role order
(P1, P2, P3, P4, O) with O's letter 'A' (the outgroup polarises).  The engine counts every taxon set once, in ascending
order, and a role assignment is a relabelling: `quintet_tests` turns tests in role order into the unique ascending sets
and, per test and statistic, two u16 slot masks.  The jackknife is the one of the four-taxon D test
(`patterns.run_dstat_jackknife`), with a block's a_j and b_j the sums of the row's slots under the two masks.

With a species map the same rows exist for five species, pooled over one lineage per species
(`QuartetEngine.patterns_quintet_blocks_species`), and `run_quintet_jackknife(species_of=...)` runs
the tests between populations.

`DFOIL` (Pease & Hahn 2015) is defined on the tree ((P1,P2),(P3,P4)),O; `PARTITIONED_D` (Eaton & Ree 2013) reads the
roles as (P1, P2, P3_1, P3_2, O).
"""
from __future__ import annotations

import numpy as np

from . import _lib
from ._lib import TetradHipError
from .engine import QuartetEngine, _ptr
from .patterns import _ascending_sets, _jackknife_host, _jackknife_starts, _run_block_jackknife, jackknife_moments, jackknife_z


class QuintetStats(tuple):
    """A sequence of (left patterns, right patterns) with a name per statistic."""

    def __new__(cls, names, pairs):
        self = super().__new__(cls, tuple((tuple(left), tuple(right)) for left, right in pairs))
        self.names = tuple(names)
        if len(self.names) != len(self):
            raise ValueError("one name per statistic")
        return self


DFOIL = QuintetStats(("DFO", "DIL", "DFI", "DOL"), (
    (("BABAA", "BBBAA", "ABABA", "AAABA"), ("BAABA", "BBABA", "ABBAA", "AABAA")),
    (("ABBAA", "BBBAA", "BAABA", "AAABA"), ("ABABA", "BBABA", "BABAA", "AABAA")),
    (("BABAA", "BABBA", "ABABA", "ABAAA"), ("ABBAA", "ABBBA", "BAABA", "BAAAA")),
    (("BAABA", "BABBA", "ABBAA", "ABAAA"), ("ABABA", "ABBBA", "BABAA", "BAAAA")),
))

PARTITIONED_D = QuintetStats(("D1", "D2", "D12"), (
    (("ABBAA",), ("BABAA",)),
    (("ABABA",), ("BAABA",)),
    (("ABBBA",), ("BABBA",)),
))


def class_table() -> np.ndarray:
    """u8[1024]: the class (1..15, 0 = not counted) of the pattern with index 256 x0 + 64 x1 + 16 x2 + 4 x3 + x4, from
    the library's rule."""
    out = np.zeros(1024, np.uint8)
    rc = _lib.load().tq_quintet_class_table(_ptr(out))
    if rc != 0:
        raise TetradHipError(rc, "tq_quintet_class_table failed")
    return out


def pattern_slot(pattern: str, rank) -> int:
    """The slot 1..15 of a pattern in role order when role i sits at ascending position rank[i]: the ascending
    positions that hold 'B'; if position 0 is among them, the complement; shifted right by one."""
    if len(pattern) != 5 or set(pattern) - {"A", "B"}:
        raise ValueError(f"pattern {pattern!r}: five letters A / B in the order (P1, P2, P3, P4, O)")
    if pattern[4] != "A":
        raise ValueError(f"pattern {pattern!r}: the outgroup's letter must be 'A'")
    bits = 0
    for i, letter in enumerate(pattern):
        if letter == "B":
            bits |= 1 << int(rank[i])
    if bits & 1:
        bits ^= 31
    if bits == 0:
        raise ValueError(f"pattern {pattern!r} is invariant")
    return bits >> 1


def _stat_names(stats):
    names = getattr(stats, "names", None)
    return tuple(names) if names is not None else tuple(f"s{i}" for i in range(len(stats)))


def quintet_tests(tests, stats=DFOIL):
    """tests int[N,5] in the order (P1, P2, P3, P4, O), five distinct taxa in any order; `stats` a sequence of
    (left patterns, right patterns) ->
    (sets5 u32[M,5] unique and ascending, set_of u32[N], masks u16[N, len(stats), 2]): statistic s of test t reads
    L as the sum of the slots in masks[t, s, 0] and R as that in masks[t, s, 1] of the block rows of sets5[set_of[t]]."""
    sets, set_of, rank = _ascending_sets(tests, 5, "(P1, P2, P3, P4, O)")
    stats = [(tuple(left), tuple(right)) for left, right in stats]
    masks = np.zeros((rank.shape[0], len(stats), 2), np.uint16)
    cache: dict = {}
    for t, p in enumerate(map(tuple, rank.tolist())):
        if p not in cache:
            row = np.zeros((len(stats), 2), np.uint16)
            for s, sides in enumerate(stats):
                for side, pats in enumerate(sides):
                    for pat in pats:
                        row[s, side] |= np.uint16(1 << pattern_slot(pat, p))
                if not row[s, 0] or not row[s, 1] or (row[s, 0] & row[s, 1]):
                    raise ValueError(f"statistic {s}: both sides need a pattern and they must not share one")
            cache[p] = row
        masks[t] = cache[p]
    return sets, set_of, masks


def dstat_jackknife_masks(bclasses, set_of, lmask, rmask) -> np.ndarray:
    """The host execution of the mask jackknife (`tq_dstat_jackknife_masks`, no GPU): block rows u32[M,B,16] ->
    f64[N,4] = {blocks with a count, D, jackknife D, jackknife variance} per test, a_j / b_j the sums of the slots under
    lmask / rmask u16[N]."""
    return _jackknife_host("tq_dstat_jackknife_masks", np.uint16, "lmask and rmask", bclasses, set_of, lmask, rmask)


def result_dtype(stats) -> np.dtype:
    """The structured type `run_quintet_jackknife` returns: nsites, then per statistic NAME_left, NAME_right (u64),
    NAME_D, NAME_jk_blocks, NAME_jk_mean, NAME_jk_se, NAME_Z."""
    fields = [("nsites", np.uint64)]
    for name in _stat_names(stats):
        fields += [(f"{name}_left", np.uint64), (f"{name}_right", np.uint64), (f"{name}_D", np.float64),
                   (f"{name}_jk_blocks", np.int64), (f"{name}_jk_mean", np.float64), (f"{name}_jk_se", np.float64),
                   (f"{name}_Z", np.float64)]
    return np.dtype(fields)


def run_quintet_jackknife(engine: QuartetEngine, tmparr, tmpmap, tests, stats=DFOIL, nblocks: int = 50, block_starts=None,
                          chunk: int = 1 << 16, *, resident: bool = False, species_of=None) -> np.ndarray:
    """Five-taxon tests with a block jackknife, full mode.  `set_data(tmparr, tmpmap)`, then the unique sets of `tests`
    int[N,5] = (P1, P2, P3, P4, O) in chunks of `chunk`: the block rows of the chunk (`patterns_quintet_blocks_dev`, torch
    memory of chunk x B x 64 bytes, re-used) and one jackknife launch per statistic on the chunk's tests
    (`dstat_jackknife_masks_dev`), all on the current stream; one device-to-host copy at the end.  Blocks, `resident`
    and `tmpmap` as in `patterns.run_dstat_jackknife`.  With `species_of` (i32[T], see `QuartetEngine.set_species`) the
    tests name species and the block rows are those of the pooled lineages (`patterns_quintet_blocks_species_dev`,
    DESIGN.md section 23); the map is set after `set_data` or, with `resident=True`, on the resident replicate (the way to
    allele mode, as in `patterns.run_dstat_jackknife`).
    Returns a structured array per test (`result_dtype(stats)`): nsites (slot 0 summed over the blocks) and per
    statistic left, right (sums over the blocks), D, jk_blocks, jk_mean, jk_se, Z = D / jk_se; NaN where undefined."""
    if int(chunk) < 1:
        raise ValueError("chunk must be positive")
    names = _stat_names(stats)
    sets, set_of, masks = quintet_tests(tests, stats)
    if not resident:
        engine.set_data(tmparr, tmpmap)
    if species_of is not None:
        engine.set_species(species_of)
    block_rows_dev = engine.patterns_quintet_blocks_dev if species_of is None else engine.patterns_quintet_blocks_species_dev
    starts = _jackknife_starts(engine, tmpmap, nblocks, block_starts)
    N, K = len(set_of), len(names)
    res = np.zeros(N, result_dtype(stats))
    if N == 0 or K == 0:
        return res
    sums, jk = _run_block_jackknife(engine, block_rows_dev, engine.dstat_jackknife_masks_dev, sets, set_of, masks.transpose(1, 2, 0),
                                    starts, chunk)
    rows = sums[set_of.astype(np.int64)].astype(np.uint64)                       # [N, 16]
    slot = np.arange(16, dtype=np.uint16)
    res["nsites"] = rows[:, 0]
    for s, name in enumerate(names):
        for side, field in enumerate(("left", "right")):
            on = (masks[:, s, side, None] >> slot) & 1
            res[f"{name}_{field}"] = (rows * on).sum(axis=1, dtype=np.uint64)
        res[f"{name}_D"] = jk[s, :, 1]
        res[f"{name}_jk_blocks"], res[f"{name}_jk_mean"], res[f"{name}_jk_se"] = jackknife_moments(jk[s])
        res[f"{name}_Z"] = jackknife_z(res[f"{name}_D"], res[f"{name}_jk_se"])
    return res

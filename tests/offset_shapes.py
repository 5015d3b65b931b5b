"""Inputs for the scans at 32-bit row offsets past 2^31 and at the switch to 64-bit addressing (a plain helper module
for tests/test_offset_shapes_cpu.py and tests/test_gpu_offset_range.py).

The cooperative scan kernels address the resident matrix with u32 byte offsets and the host keeps a batch on them only
while T * pitch < 0xFFFF0000.  One host matrix of 3 067 rows x 1 400 000 sites serves four shapes, each the contiguous
slice ``matrix[:T]``:

    T      T * Sp
    1600   2 241 331 200   past 2^31, inside the limit, T^3 <= 2^32 (the joint-histogram scan is eligible);
                           row 1533 starts 8 192 bytes below 2^31 and straddles it
    3065   4 293 550 080   1 351 680 bytes below 0xFFFF0000; the packed set lies past the limit
    3066   4 294 950 912   past 0xFFFF0000, below 2^32: only the host comparison protects the kernels
    3067   4 296 351 744   past 2^32

A few HOT rows hold simulated tree-like data; every other row is a copy of one further simulated row (the DECOY), so a
read that lands on a wrong row returns well-formed but different data.  The expected rows come from the oracle on the
nine-row submatrix of a shape's hot rows, so the oracle never sees the 4 GB matrix.
"""
from __future__ import annotations

from functools import lru_cache
from itertools import combinations

import numpy as np

S = 1_400_000
TILE = 2048                                  # sites per step of a scan: rows are padded to a multiple of it
SP = -(-S // TILE) * TILE                    # 1 400 832 bytes per resident row, 684 steps
T_ROWS = 3067
SHAPES = (1600, 3065, 3066, 3067)
COMMON_HOT = (0, 1, 1532, 1533, 1534)        # 1533 straddles byte 2^31 of the resident rows
SEED = 20261
# per-branch substitution probability of the simulation: at the simulator's default of 0.05 two sister rows differ at
# about a quarter of the sites only; at 0.5 every pair of rows differs at more than 0.6 of them, whatever the tree
P_BRANCH = 0.5
PERM_SEED = 7


def hot_rows(T: int) -> tuple[int, ...]:
    """The nine hot rows of shape T: the common ones and its last four."""
    return COMMON_HOT + tuple(range(T - 4, T))


ALL_HOT = tuple(sorted(set().union(*(hot_rows(T) for T in SHAPES))))


@lru_cache(maxsize=None)
def simulated():
    """(hot u8[len(ALL_HOT), S] in the order of ALL_HOT, decoy u8[S], tmpmap u32[S,2]): one simulation, its last row the
    decoy; loci are runs of 5 sites, so subsample mode counts something and the packed layout is padded (six loci per
    32-site word)."""
    from tetrad_amd import synth
    rows, tmpmap = synth.simulate_tmparr(len(ALL_HOT) + 1, S, SEED, p=P_BRANCH, missing=0.1)
    tmpmap[:, 0] = np.arange(S, dtype=np.uint32) // 5
    rows.setflags(write=False)
    tmpmap.setflags(write=False)
    return rows[:-1], rows[-1], tmpmap


def build_matrix() -> np.ndarray:
    """The host matrix u8[T_ROWS, S] (4.3 GB): the decoy in every row by a broadcast copy, then the hot rows."""
    hot, decoy, _ = simulated()
    m = np.empty((T_ROWS, S), np.uint8)
    m[:] = decoy
    m[list(ALL_HOT)] = hot
    return m


@lru_cache(maxsize=None)
def quartets(T: int):
    """(quartets u32[252,4], index i64[252] into the 126 four-subsets): all four-subsets of the shape's hot rows, once
    in lexicographic order (neighbours share a and b) and once under a seeded permutation."""
    lex = np.array(list(combinations(hot_rows(T), 4)), np.uint32)
    idx = np.concatenate([np.arange(len(lex)), np.random.default_rng(PERM_SEED).permutation(len(lex))])
    q = np.ascontiguousarray(lex[idx])
    q.setflags(write=False)
    return q, idx


@lru_cache(maxsize=None)
def expected(T: int, subsample: bool):
    """Oracle rows of quartets(T): (rstat, rscor, debug dict, exact ranks i32[252,3]) from the nine-row submatrix with
    remapped indices, computed once per shape and mode."""
    from oracle import oracle as orc
    from exact_ties import exact_rank
    hot, _, tmpmap = simulated()
    rows = hot_rows(T)
    sub = np.ascontiguousarray(hot[[ALL_HOT.index(r) for r in rows]])
    lex = np.array(list(combinations(range(len(rows)), 4)), np.uint32)
    _, rstat, rscor, dbg = orc.new_infer_resolved_quartets(sub, tmpmap, lex, subsample, debug=True)
    exact = np.zeros((len(lex), 3), np.int32)
    live = rstat[:, 1] > 0
    exact[live] = exact_rank(dbg["cmats"][live])
    _, idx = quartets(T)
    out = (rstat[idx], rscor[idx], {k: v[idx] for k, v in dbg.items()}, exact[idx])
    for a in (out[0], out[1], out[3], *out[2].values()):
        a.setflags(write=False)
    return out

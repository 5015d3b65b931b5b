"""Site-pattern classes of quartets and ABBA-BABA D tests with bootstrap Z.

A site pattern of a quartet is four bases in the order of its taxa.  Its class is its restricted-growth string:
position 0 gets label 0 and every base not seen before gets the next label.  The 15 strings in lexicographic order
(`CLASS_STRINGS`) number the classes; `QuartetEngine.patterns` returns u32[Q,16] rows with the 15 class counts and
their sum.  With roles (P1, P2, P3, O) in positions 0..3, BBAA is class 3, BABA class 6 and ABBA class 8.

Permuting the four positions only permutes the classes (`permute_classes`), so the engine scans every taxon set once,
as its ascending quartet, and every role assignment is read off that row: `dstat_tests` turns tests in role order
into the unique ascending sets and, per test, the row and the two class indices that play ABBA and BABA.

`run_dstat_jackknife` is the same test with the error estimate everyone else uses: the sites
are cut into contiguous blocks (`locus_blocks`), one pass writes the class rows of every (set, block)
(`QuartetEngine.patterns_blocks_dev`) and one kernel per chunk of sets runs the delete-one-block jackknife of every
test (`dstat_jackknife_dev`) -- no replicate is built and nothing is rescanned.  With `species_of` the tests name
species and the block rows are the pooled ones of `patterns_blocks_species_dev`.

`run_dstat` is the whole bootstrap test: observed counts from the given matrix, then locus-bootstrap replicates built on the
device, each followed on the same stream by the class rows of the unique sets and one accumulation kernel.  Nothing
returns to the host before the end.
"""
from __future__ import annotations

from itertools import combinations
from typing import Optional

import numpy as np

from . import _lib, bootstrap
from ._lib import TetradHipError
from .engine import QuartetEngine, _ptr

CLASS_STRINGS = ("0000", "0001", "0010", "0011", "0012", "0100", "0101", "0102", "0110", "0111", "0112", "0120",
                 "0121", "0122", "0123")
NCLASS = 15
BBAA, BABA, ABBA = 3, 6, 8

JACKKNIFE_DTYPE = np.dtype([("abba", np.uint32), ("baba", np.uint32), ("bbaa", np.uint32), ("nsites", np.uint32),
                            ("D", np.float64), ("jk_blocks", np.int64), ("jk_mean", np.float64), ("jk_se", np.float64),
                            ("Z", np.float64)])
MAX_BLOCKS = 4096

DSTAT_DTYPE = np.dtype([("abba", np.uint32), ("baba", np.uint32), ("bbaa", np.uint32), ("nsites", np.uint32),
                        ("D", np.float64), ("boot_n", np.int64), ("boot_mean", np.float64), ("boot_std", np.float64),
                        ("Z", np.float64)])


def class_table() -> np.ndarray:
    """u8[256]: the class of the pattern with slab index 64 x0 + 16 x1 + 4 x2 + x3, from the library's rule."""
    out = np.zeros(256, np.uint8)
    rc = _lib.load().tq_pattern_class_table(_ptr(out))
    if rc != 0:
        raise TetradHipError(rc, "tq_pattern_class_table failed")
    return out


def _class_of_labels(labels) -> int:
    """The class of four symbols (any hashables) in position order."""
    seen: dict = {}
    s = "".join(str(seen.setdefault(x, len(seen))) for x in labels)
    return CLASS_STRINGS.index(s)


def class_permutation(perm) -> np.ndarray:
    """i64[15]: new class of each class when the positions are reordered so that new position i holds what position
    perm[i] held."""
    perm = [int(p) for p in perm]
    if sorted(perm) != [0, 1, 2, 3]:
        raise ValueError("perm must be a permutation of 0..3")
    return np.array([_class_of_labels([s[p] for p in perm]) for s in CLASS_STRINGS], np.int64)


def permute_classes(classes: np.ndarray, perm) -> np.ndarray:
    """Class rows [..., 16] (or [..., 15]) of quartets (t0, t1, t2, t3) -> the rows of (t[perm[0]], .., t[perm[3]]).
    The sum slot stays."""
    classes = np.asarray(classes)
    out = classes.copy()
    out[..., class_permutation(perm)] = classes[..., :NCLASS]
    return out


def dstat_tests(tests):
    """tests int[N,4] in the order (P1, P2, P3, O), distinct taxa in any order ->
    (sets u32[M,4] unique and ascending, set_of u32[N], ia u8[N], ib u8[N]): test t reads ABBA at
    classes[set_of[t], ia[t]] and BABA at classes[set_of[t], ib[t]] of the class rows of `sets`.  The three D tests of
    one taxon set share one row."""
    sets, set_of, idx = _role_classes(tests, (ABBA, BABA))
    return sets, set_of, idx[:, 0].copy(), idx[:, 1].copy()


def _ascending_sets(tests, width: int, roles: str):
    """tests int[N,width] in the order `roles`, distinct taxa in any order -> (sets u32[M,width] unique and ascending,
    set_of u32[N], rank i64[N,width]): role position i of test t holds ascending position rank[t, i] of
    sets[set_of[t]]."""
    tests = np.asarray(tests)
    if tests.ndim != 2 or tests.shape[1] != width:
        raise ValueError(f"tests must be [N, {width}] in the order {roles}")
    if tests.size and tests.min() < 0:
        raise ValueError("taxon indices must not be negative")
    tests = tests.astype(np.int64)
    order = np.argsort(tests, axis=1, kind="stable")
    asc = np.take_along_axis(tests, order, axis=1)
    if tests.shape[0] and (asc[:, 1:] == asc[:, :-1]).any():
        raise ValueError(f"the {('four', 'five')[width - 4]} taxa of a test must be distinct")
    rank = np.argsort(order, axis=1, kind="stable")
    if tests.shape[0]:
        sets, set_of = np.unique(asc, axis=0, return_inverse=True)
    else:
        sets, set_of = asc, np.zeros(0, np.int64)
    return (np.ascontiguousarray(sets, dtype=np.uint32), np.ascontiguousarray(set_of.reshape(-1), dtype=np.uint32), rank)


def _role_classes(tests, role_classes):
    sets, set_of, rank = _ascending_sets(tests, 4, "(P1, P2, P3, O)")
    idx = np.zeros((rank.shape[0], len(role_classes)), np.uint8)
    cache: dict = {}
    for t, p in enumerate(map(tuple, rank.tolist())):
        if p not in cache:
            inv = np.argsort(class_permutation(p))          # inv[role class] = class of the ascending row
            cache[p] = [int(inv[c]) for c in role_classes]
        idx[t] = cache[p]
    return sets, set_of, idx


def tests_with_outgroup(ntaxa: int, outgroup: int) -> np.ndarray:
    """i64[3 C(ntaxa - 1, 3), 4]: every test (P1, P2, P3, O) with O = outgroup -- for each three other taxa a < b < c
    the three choices of P3: (a, b, c), (a, c, b), (b, c, a)."""
    if not 0 <= outgroup < ntaxa:
        raise ValueError("outgroup must be a taxon index")
    rows = []
    for a, b, c in combinations([t for t in range(ntaxa) if t != outgroup], 3):
        rows += [(a, b, c, outgroup), (a, c, b, outgroup), (b, c, a, outgroup)]
    return np.array(rows, np.int64).reshape(-1, 4)


def dstat_moments(D: np.ndarray, acc: np.ndarray):
    """(boot_n, boot_mean, boot_std, Z) from the observed D and the accumulator f64[N,4] = {n, s1, s2, last}:
    boot_mean = s1 / n, boot_std = sqrt(max(0, s2 / n - (s1 / n)^2)), Z = D / boot_std; NaN where a denominator is 0."""
    acc = np.asarray(acc, np.float64).reshape(-1, 4)
    n, s1, s2 = acc[:, 0], acc[:, 1], acc[:, 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        mean = np.where(n > 0, s1 / n, np.nan)
        std = np.where(n > 0, np.sqrt(np.maximum(0.0, s2 / n - mean * mean)), np.nan)
        Z = np.where(std > 0, np.asarray(D, np.float64) / std, np.nan)
    return n.astype(np.int64), mean, std, Z


def observed_dstat(classes: np.ndarray, set_of, ia, ib, ibbaa) -> np.ndarray:
    """The observed columns of the result from the class rows of the unique sets (the bootstrap columns empty)."""
    rows = np.asarray(classes)[np.asarray(set_of, np.int64)]
    take = lambda col: rows[np.arange(rows.shape[0]), np.asarray(col, np.int64)]
    out = np.zeros(rows.shape[0], DSTAT_DTYPE)
    out["abba"], out["baba"], out["bbaa"], out["nsites"] = take(ia), take(ib), take(ibbaa), rows[:, NCLASS]
    a, b = out["abba"].astype(np.int64), out["baba"].astype(np.int64)
    with np.errstate(divide="ignore", invalid="ignore"):
        out["D"] = np.where(a + b > 0, (a - b) / (a + b), np.nan)
    out["boot_mean"] = out["boot_std"] = out["Z"] = np.nan
    return out


def run_dstat(engine: QuartetEngine, tmparr, tmpmap, seqarr, spans, tests, nboots: int, *, subsample_snps: bool = False,
              seed=None, rng: Optional[np.random.Generator] = None, species_of=None) -> np.ndarray:
    """D tests with a locus bootstrap.  The observed counts are those of the resident matrix after
    `set_data(tmparr, tmpmap)`; then `nboots` replicates of (seqarr, spans) are built on the device
    (`bootstrap.draw_replicate` on one Generator, `engine.bootstrap` on the current stream), each followed on that
    stream by the class rows of the unique sets and the accumulation of every test's D.  One device-to-host copy at
    the end.  `tests` int[N,4] = (P1, P2, P3, O).  With `species_of` (i32[T], see `QuartetEngine.set_species`) the
    tests name species and the counts are those of the pooled lineages (full mode only).
    Returns a structured array per test: abba, baba, bbaa, nsites, D, boot_n, boot_mean, boot_std, Z."""
    import torch
    species = species_of is not None
    if species and subsample_snps:
        raise ValueError("species mode counts every site: subsample_snps must be False")
    rng = rng if rng is not None else np.random.default_rng(seed)
    sets, set_of, idx = _role_classes(tests, (ABBA, BABA, BBAA))
    ia, ib = idx[:, 0].copy(), idx[:, 1].copy()
    engine.set_data(tmparr, tmpmap)
    if species:
        engine.set_species(species_of)
        obs = engine.patterns_species(sets)
    else:
        obs = engine.patterns(sets, subsample_snps)
    out = observed_dstat(obs, set_of, ia, ib, idx[:, 2])
    N, M = len(set_of), len(sets)
    if nboots <= 0 or N == 0:
        return out
    engine.set_source(seqarr, spans)
    nloci = int(np.asarray(spans).reshape(-1, 2).shape[0])
    dev = torch.device("cuda", engine.device_id)
    with torch.cuda.device(dev):
        cur = torch.cuda.current_stream(dev)
        d_sets = torch.from_numpy(sets.view(np.int32)).to(dev)
        d_set_of = torch.from_numpy(set_of.view(np.int32)).to(dev)
        d_ia, d_ib = torch.from_numpy(ia).to(dev), torch.from_numpy(ib).to(dev)
        d_classes = torch.empty((M, 16), dtype=torch.int32, device=dev)
        d_acc = torch.zeros((N, 4), dtype=torch.float64, device=dev)
        for _ in range(int(nboots)):
            lidxs, s1, s2 = bootstrap.draw_replicate(nloci, rng)
            engine.bootstrap(lidxs, s1, s2, stream=cur.cuda_stream)
            if species:
                engine.patterns_species_dev(d_sets.data_ptr(), M, d_classes.data_ptr(), cur.cuda_stream)
            else:
                engine.patterns_dev(d_sets.data_ptr(), M, subsample_snps, d_classes.data_ptr(), cur.cuda_stream)
            engine.dstat_accumulate_dev(d_classes.data_ptr(), M, d_set_of.data_ptr(), d_ia.data_ptr(), d_ib.data_ptr(), N,
                                        d_acc.data_ptr(), cur.cuda_stream)
        acc = d_acc.cpu().numpy()
    out["boot_n"], out["boot_mean"], out["boot_std"], out["Z"] = dstat_moments(out["D"], acc)
    return out


def dstat_accumulate(classes, set_of, ia, ib, acc) -> np.ndarray:
    """The host execution of the accumulation kernel (`tq_dstat_accumulate`, no GPU): one replicate's class rows
    u32[M,16] added to acc f64[N,4] in place."""
    classes = np.ascontiguousarray(classes, dtype=np.uint32).reshape(-1, 16)
    set_of = np.ascontiguousarray(set_of, dtype=np.uint32)
    ia, ib = np.ascontiguousarray(ia, dtype=np.uint8), np.ascontiguousarray(ib, dtype=np.uint8)
    if not (isinstance(acc, np.ndarray) and acc.dtype == np.float64 and acc.flags.c_contiguous
            and acc.size == 4 * set_of.shape[0]):
        raise ValueError("acc must be a C-contiguous float64 array [N, 4]")
    if not (ia.shape == ib.shape == set_of.shape):
        raise ValueError("set_of, ia and ib must have one entry per test")
    lib = _lib.load()
    rc = lib.tq_dstat_accumulate(_ptr(classes), classes.shape[0], _ptr(set_of), _ptr(ia), _ptr(ib), set_of.shape[0],
                                 _ptr(acc))
    if rc != 0:
        raise TetradHipError(rc, lib.tq_last_error(None).decode())
    return acc


def locus_blocks(tmpmap, nblocks: int) -> np.ndarray:
    """i64[B + 1] block starts that cut [0, S) at locus boundaries only, B = min(nblocks, number of loci).  Cut k sits
    at the locus boundary nearest to k S / B (the lower one of two equally near) among those that leave a locus for
    every block before and after it, so the blocks hold as equal site counts as the loci allow.  `tmpmap` is u32[S,2]
    (column 0 used) or the 1-D locus column; a locus is a run of equal ids."""
    tm = np.asarray(tmpmap)
    locus = tm[:, 0] if tm.ndim == 2 else tm.reshape(-1)
    S = int(locus.shape[0])
    if S < 1:
        raise ValueError("the matrix has no sites")
    if not 1 <= int(nblocks) <= MAX_BLOCKS:
        raise ValueError(f"nblocks must be 1..{MAX_BLOCKS}")
    bnd = np.flatnonzero(locus[1:] != locus[:-1]).astype(np.int64) + 1       # interior locus boundaries, ascending
    B = min(int(nblocks), bnd.shape[0] + 1)
    starts = np.zeros(B + 1, np.int64)
    starts[B] = S
    lo = 0                                                                     # first boundary index still free
    for k in range(1, B):
        hi = bnd.shape[0] - (B - 1 - k)                                        # leave one boundary per later cut
        num = k * S                                                            # target = num / B, compared exactly
        i = int(np.searchsorted(bnd[lo:hi] * B, num, side="left")) + lo        # first boundary >= target
        if i >= hi:
            i = hi - 1
        elif i > lo and num - int(bnd[i - 1]) * B <= int(bnd[i]) * B - num:
            i -= 1
        starts[k] = bnd[i]
        lo = i + 1
    return starts


def jackknife_moments(out: np.ndarray):
    """(jk_blocks, jk_mean, jk_se) from the rows f64[N,4] = {g, theta, theta_J, var} the jackknife calls write:
    jk_mean = theta_J, jk_se = sqrt(var); both NaN where fewer than two blocks hold a count."""
    out = np.asarray(out, np.float64).reshape(-1, 4)
    with np.errstate(invalid="ignore"):
        se = np.sqrt(out[:, 3])
    return out[:, 0].astype(np.int64), out[:, 2].copy(), se


def jackknife_z(D, se) -> np.ndarray:
    """Z = D / jk_se; NaN where the standard error is 0 or undefined."""
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(se > 0, D / se, np.nan)


def _jackknife_host(entry: str, dtype, names: str, bclasses, set_of, a, b) -> np.ndarray:
    """The host execution of a jackknife kernel (library entry point `entry`, no GPU) on block rows u32[M,B,16] and the
    per-test arrays a, b of `dtype`."""
    bclasses = np.ascontiguousarray(bclasses, dtype=np.uint32)
    if bclasses.ndim != 3 or bclasses.shape[2] != 16:
        raise ValueError("bclasses must be [M, B, 16]")
    set_of = np.ascontiguousarray(set_of, dtype=np.uint32)
    a, b = np.ascontiguousarray(a, dtype=dtype), np.ascontiguousarray(b, dtype=dtype)
    if not (a.shape == b.shape == set_of.shape):
        raise ValueError(f"set_of, {names} must have one entry per test")
    out = np.zeros((set_of.shape[0], 4), np.float64)
    lib = _lib.load()
    rc = getattr(lib, entry)(_ptr(bclasses), bclasses.shape[0], bclasses.shape[1], _ptr(set_of), _ptr(a), _ptr(b),
                             set_of.shape[0], _ptr(out))
    if rc != 0:
        raise TetradHipError(rc, lib.tq_last_error(None).decode())
    return out


def dstat_jackknife(bclasses, set_of, ia, ib) -> np.ndarray:
    """The host execution of the jackknife kernel (`tq_dstat_jackknife`, no GPU): block rows u32[M,B,16] ->
    f64[N,4] = {blocks with a count, D, jackknife D, jackknife variance} per test."""
    return _jackknife_host("tq_dstat_jackknife", np.uint8, "ia and ib", bclasses, set_of, ia, ib)


def _jackknife_starts(engine: QuartetEngine, tmpmap, nblocks: int, block_starts) -> np.ndarray:
    """i64[B + 1]: `block_starts`, or without it `locus_blocks` of `tmpmap` (None: the resident locus column)."""
    if block_starts is None:
        if tmpmap is None:
            tmpmap = engine.get_data()[1]
        block_starts = locus_blocks(tmpmap, nblocks)
    return np.ascontiguousarray(block_starts, dtype=np.int64).reshape(-1)


def _run_block_jackknife(engine: QuartetEngine, block_rows_dev, jackknife_dev, sets, set_of, per_test, starts, chunk: int):
    """The chunked device loop of the block-jackknife drivers, all on the current stream.  `sets` u32[M,width] and
    `set_of` u32[N] (N > 0) as `_ascending_sets` gives them; `per_test` [K,2,N] (u8 or u16, K > 0) holds the two
    per-test arrays of each of K statistics.  Per chunk of `chunk` >= 1 sets: the block rows (`block_rows_dev`, torch memory
    of chunk x B x 64 bytes, re-used), their sums over the blocks, and one `jackknife_dev` launch per statistic on the
    chunk's tests.  One device-to-host copy at the end.
    Returns (u32[M,16] block sums per set, f64[K,N,4] jackknife rows in test order)."""
    import torch
    B = starts.shape[0] - 1
    (M, width), N, K = sets.shape, len(set_of), per_test.shape[0]
    chunk = min(int(chunk), M)
    # the tests in the order of their sets: the tests of a chunk of sets are then one contiguous run
    order = np.argsort(set_of, kind="stable")
    s_sorted = set_of[order].astype(np.int64)
    item = per_test.dtype.itemsize
    dev = torch.device("cuda", engine.device_id)
    with torch.cuda.device(dev):
        cur = torch.cuda.current_stream(dev)
        d_sets = torch.from_numpy(sets.view(np.int32)).to(dev)
        d_rel = torch.from_numpy((s_sorted % chunk).astype(np.uint32).view(np.int32)).to(dev)
        d_per = torch.from_numpy(np.ascontiguousarray(per_test[:, :, order]).view(np.uint8)).to(dev)
        d_rows = torch.empty((chunk, B, 16), dtype=torch.int32, device=dev)
        # u32 sums: a set counts at most S < 2^32 sites (a species set: below 2^32 by the range rule of species mode)
        d_sum = torch.empty((M, 16), dtype=torch.int32, device=dev)
        d_out = torch.empty((K, N, 4), dtype=torch.float64, device=dev)
        for q0 in range(0, M, chunk):
            n = min(chunk, M - q0)
            block_rows_dev(d_sets.data_ptr() + 4 * width * q0, n, starts, d_rows.data_ptr(), cur.cuda_stream)
            torch.sum(d_rows[:n], dim=1, dtype=torch.int32, out=d_sum[q0:q0 + n])
            t0, t1 = (int(v) for v in np.searchsorted(s_sorted, [q0, q0 + n], side="left"))
            for s in range(K if t1 > t0 else 0):
                jackknife_dev(d_rows.data_ptr(), n, B, d_rel.data_ptr() + 4 * t0, d_per.data_ptr() + item * (2 * s * N + t0),
                              d_per.data_ptr() + item * ((2 * s + 1) * N + t0), t1 - t0, d_out.data_ptr() + 32 * (s * N + t0),
                              cur.cuda_stream)
        sums = d_sum.cpu().numpy().view(np.uint32)
        jk = np.empty((K, N, 4), np.float64)
        jk[:, order] = d_out.cpu().numpy()
    return sums, jk


def run_dstat_jackknife(engine: QuartetEngine, tmparr, tmpmap, tests, nblocks: int = 50, block_starts=None,
                        chunk: int = 1 << 16, *, resident: bool = False, species_of=None) -> np.ndarray:
    """D tests with a block jackknife, full mode.  `set_data(tmparr, tmpmap)`, then the unique sets of `tests`
    int[N,4] = (P1, P2, P3, O) in chunks of `chunk`: the block rows of the chunk (`patterns_blocks_dev`, torch memory of
    chunk x B x 64 bytes, re-used) and the jackknife of the chunk's tests (`dstat_jackknife_dev`), all on the current
    stream; one device-to-host copy at the end.  The blocks are `block_starts` i64[B + 1] or, without it,
    `locus_blocks(tmpmap, nblocks)`.  With `resident=True` nothing is loaded: the tests run on the replicate the engine
    holds (after `engine.bootstrap`, say); `tmparr` is not read, and `tmpmap` may be None when `block_starts` is given
    (else the resident locus column is fetched for the cuts).  With `species_of` (i32[T], see
    `QuartetEngine.set_species`) the tests name species and the block rows are those of the pooled lineages
    (`patterns_blocks_species_dev`); the map is set after `set_data` or, with `resident=True`, on the resident replicate
    (the way to allele mode: `set_source`, `bootstrap`, option "species_alleles", then `resident=True`).
    Returns a structured array per test: abba, baba, bbaa, nsites (sums over the blocks), D, jk_blocks, jk_mean,
    jk_se, Z = D / jk_se; NaN where undefined."""
    if int(chunk) < 1:
        raise ValueError("chunk must be positive")
    sets, set_of, idx = _role_classes(tests, (ABBA, BABA, BBAA))
    if not resident:
        engine.set_data(tmparr, tmpmap)
    if species_of is not None:
        engine.set_species(species_of)
    block_rows_dev = engine.patterns_blocks_dev if species_of is None else engine.patterns_blocks_species_dev
    starts = _jackknife_starts(engine, tmpmap, nblocks, block_starts)
    N = len(set_of)
    res = np.zeros(N, JACKKNIFE_DTYPE)
    if N == 0:
        return res
    sums, jk = _run_block_jackknife(engine, block_rows_dev, engine.dstat_jackknife_dev, sets, set_of, idx[:, :2].T[None], starts,
                                    chunk)
    rows = sums[set_of.astype(np.int64)]
    take = lambda col: rows[np.arange(N), np.asarray(col, np.int64)]
    res["abba"], res["baba"], res["bbaa"], res["nsites"] = take(idx[:, 0]), take(idx[:, 1]), take(idx[:, 2]), rows[:, NCLASS]
    res["D"] = jk[0, :, 1]
    res["jk_blocks"], res["jk_mean"], res["jk_se"] = jackknife_moments(jk[0])
    res["Z"] = jackknife_z(res["D"], res["jk_se"])
    return res

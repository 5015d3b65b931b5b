"""CPU-only: the host execution of the taxon counts, the derived quantities and neighbour joining
against the independent model of tests/taxdist_model.py."""
import ctypes
import math

import numpy as np
import pytest

from conftest import GOLDEN_FULL_CASES, load_golden
import taxdist_model as tm
from tetrad_amd import _lib, distance, synth
from tetrad_amd._lib import TetradHipError


@pytest.fixture(scope="module")
def lib():
    _lib.build()
    return _lib.load()


def last_error(lib):
    return lib.tq_last_error(None).decode()


# -- counts ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GOLDEN_FULL_CASES)
def test_goldens_host_equals_model(lib, name):
    tmparr = load_golden(name)["tmparr"]
    T, S = tmparr.shape
    starts = tm.tiling(S)
    tiled = distance.taxon_counts_host(tmparr, starts)
    whole = distance.taxon_counts_host(tmparr)
    assert tiled.dtype == np.uint32 and tiled.shape == (len(starts) - 1, T, T, 4) and whole.shape == (1, T, T, 4)
    assert np.array_equal(tiled, tm.counts(tmparr, starts))
    assert np.array_equal(whole, tm.counts(tmparr))
    # identities
    assert np.array_equal(tiled, tiled.transpose(0, 2, 1, 3))
    assert np.array_equal(tiled[..., 1], tiled[..., 2] + tiled[..., 3])
    assert np.array_equal(tiled.astype(np.int64).sum(axis=0), whole[0].astype(np.int64))
    idx = np.arange(T)
    assert np.array_equal(whole[0, idx, idx, 0], (tmparr <= 3).sum(axis=1))
    assert not whole[0, idx, idx, 1:].any()


def test_blocks_with_gaps_count_only_their_sites(lib):
    tmparr = load_golden("sparse_T10_S257")["tmparr"]
    starts = np.array([2, 70, 200, 257], np.int64)
    got = distance.taxon_counts_host(tmparr, starts)
    assert np.array_equal(got, tm.counts(tmparr, starts))
    inner = np.array([3, 60, 66, 67, 130, 190], np.int64)          # sites 0..2, 60..65, 67..129 and 190.. count nowhere
    got = distance.taxon_counts_host(tmparr, inner)
    assert np.array_equal(got, tm.counts(tmparr, inner))
    for j in range(len(inner) - 1):
        assert np.array_equal(got[j], tm.counts(tmparr[:, inner[j]:inner[j + 1]])[0])


def test_particular_inputs(lib):
    rng = np.random.default_rng(5)
    a = rng.integers(0, 4, size=(6, 333), dtype=np.uint8)
    full = distance.taxon_counts_host(a)                           # no missing cell
    assert (full[0, :, :, 0] == 333).all() and np.array_equal(full, tm.counts(a))
    b = a.copy()
    b[2] = 78                                                      # a taxon that is all missing
    got = distance.taxon_counts_host(b)
    assert not got[0, 2].any() and not got[0, :, 2].any() and np.array_equal(got, tm.counts(b))
    c = a.copy()
    hole = rng.random(a.shape) < 0.3
    want = None
    for code in (4, 78, 255):                                      # every value above 3 is missing
        c[hole] = code
        got = distance.taxon_counts_host(c)
        assert np.array_equal(got, tm.counts(c))
        want = got if want is None else want
        assert np.array_equal(got, want)


def test_counts_refusals(lib):
    a = np.zeros((3, 10), np.uint8)
    out = np.zeros((4100, 3, 3, 4), np.uint32)
    one = np.array([0, 10], np.int64)

    def call(arr, T, S, starts, B, o):
        p = lambda x: None if x is None else x.ctypes.data
        return lib.tq_taxon_counts_host(p(arr), T, S, p(starts), B, p(o))

    assert call(a, 3, 10, one, 1, out) == 0
    for args in ((None, 3, 10, one, 1, out), (a, 3, 10, None, 1, out), (a, 3, 10, one, 1, None)):
        assert call(*args) == -1 and "NULL" in last_error(lib)
    assert call(a, 1, 10, one, 1, out) == -1 and "T >= 2" in last_error(lib)
    assert call(a, 3, 0, one, 1, out) == -1 and "S >= 1" in last_error(lib)
    assert call(a, 3, 10, one, 0, out) == -1 and "B=0" in last_error(lib)
    many = np.arange(4098, dtype=np.int64)
    big = np.zeros((3, 5000), np.uint8)
    assert call(big, 3, 5000, many, 4097, out) == -1 and "B=4097" in last_error(lib)
    assert call(big, 3, 5000, many, 4096, out) == 0
    assert call(a, 3, 10, np.array([0, 5, 5, 10], np.int64), 3, out) == -1 and "not above" in last_error(lib)
    assert call(a, 3, 10, np.array([0, 7, 5, 10], np.int64), 3, out) == -1 and "not above" in last_error(lib)
    assert call(a, 3, 10, np.array([-1, 10], np.int64), 1, out) == -1 and "negative" in last_error(lib)
    assert call(a, 3, 10, np.array([0, 11], np.int64), 1, out) == -1 and "past" in last_error(lib)
    with pytest.raises(TetradHipError, match="past"):
        distance.taxon_counts_host(a, [0, 11])


# -- distances -----------------------------------------------------------------------------------------------------
def pair_counts(both, ts, tv, n0=None, n1=None):
    c = np.zeros((2, 2, 4), np.int64)
    c[0, 1] = c[1, 0] = (both, ts + tv, ts, tv)
    c[0, 0, 0] = both if n0 is None else n0
    c[1, 1, 0] = both if n1 is None else n1
    return c


def test_distances_by_hand():
    c = pair_counts(100, 6, 4)
    assert distance.distances(c, "p")[0, 1] == 0.1
    assert distance.distances(c, "jc")[0, 1] == pytest.approx(-0.75 * math.log(1.0 - 4.0 * 0.1 / 3.0), rel=1e-15)
    k = -0.5 * math.log((1.0 - 2.0 * 0.06 - 0.04) * math.sqrt(1.0 - 2.0 * 0.04))
    assert distance.distances(c, "kimura")[0, 1] == pytest.approx(k, rel=1e-15)
    for model in distance.MODELS:
        d = distance.distances(c.astype(np.uint32), model)
        assert d.shape == (2, 2) and d[0, 0] == 0.0 and d[1, 1] == 0.0 and d[0, 1] == d[1, 0]
        assert distance.distances(pair_counts(50, 0, 0), model)[0, 1] == 0.0
    stacked = distance.distances(np.stack([c, pair_counts(10, 1, 1)]), "p")        # leading shape
    assert stacked.shape == (2, 2, 2) and stacked[1, 0, 1] == 0.2
    with pytest.raises(ValueError):
        distance.distances(c, "logdet")


def test_distances_undefined_and_saturated():
    empty = pair_counts(0, 0, 0, 5, 7)
    for model in distance.MODELS:
        d = distance.distances(empty, model)
        assert math.isnan(d[0, 1]) and math.isnan(d[1, 0]) and d[0, 0] == 0.0
    assert distance.distances(pair_counts(100, 40, 35), "p")[0, 1] == 0.75
    assert distance.distances(pair_counts(100, 40, 35), "jc")[0, 1] == math.inf                # p = 0.75
    assert distance.distances(pair_counts(100, 40, 40), "jc")[0, 1] == math.inf                # p > 0.75
    assert math.isfinite(distance.distances(pair_counts(100, 40, 34), "jc")[0, 1])
    assert distance.distances(pair_counts(100, 10, 50), "kimura")[0, 1] == math.inf            # 1 - 2Q = 0
    assert distance.distances(pair_counts(100, 50, 0), "kimura")[0, 1] == math.inf             # 1 - 2P - Q = 0
    assert distance.distances(pair_counts(100, 60, 0), "kimura")[0, 1] == math.inf             # 1 - 2P - Q < 0
    d = np.array([[0.0, 1.0, np.nan], [1.0, 0.0, 3.0], [np.nan, 3.0, 0.0]])
    f = distance.fill_undefined(d)
    assert f[0, 2] == 6.0 and f[2, 0] == 6.0 and f[0, 1] == 1.0 and np.isnan(d[0, 2])
    assert distance.fill_undefined(np.where(np.isnan(d), np.inf, d), factor=1.5)[0, 2] == 4.5


def test_sharing_and_pool_counts_against_loops(lib):
    tmparr = load_golden("sparse_T10_S257")["tmparr"]
    c = distance.taxon_counts_host(tmparr, [0, 100, 257])
    T = tmparr.shape[0]
    both, jac = distance.sharing(c)
    assert both.dtype == np.int64 and both.shape == (2, T, T)
    for b in range(2):
        for i in range(T):
            for j in range(T):
                n = int(c[b, i, i, 0]) + int(c[b, j, j, 0]) - int(c[b, i, j, 0])
                assert both[b, i, j] == c[b, i, j, 0]
                assert jac[b, i, j] == (int(c[b, i, j, 0]) / n if n else 0.0)
    z = np.zeros((2, 2, 4), np.uint32)
    assert not distance.sharing(z)[1].any()
    species_of = np.array([0, 1, 0, 2, -1, 1, 0, 3, 2, 0])
    K = 4
    pooled = distance.pool_counts(c, species_of)
    assert pooled.dtype == np.int64 and pooled.shape == (2, K, K, 4)
    want = np.zeros((2, K, K, 4), np.int64)
    for b in range(2):
        for i in range(T):
            for j in range(T):
                A, Bs = species_of[i], species_of[j]
                if A < 0 or Bs < 0 or (A == Bs and not i < j):
                    continue
                want[b, A, Bs] += c[b, i, j]
    assert np.array_equal(pooled, want)
    assert not pooled[:, 3, 3].any()                               # a single member
    assert np.array_equal(distance.pool_counts(c[0], species_of, K=5)[:K, :K], want[0])


# -- neighbour joining ---------------------------------------------------------------------------------------------
def dyadic_tree(T, seed):
    """(dist f64[T, T], parent, length) of a random binary tree whose edge lengths are multiples of 1/8."""
    rng = np.random.default_rng(seed)
    children, root = synth.random_tree_children(T, rng)
    parent = tm.children_to_parent(children, root, T)
    length = [0.0 if p < 0 else float(rng.integers(1, 17)) / 8.0 for p in parent]
    anc = []
    for t in range(T):
        path, v, acc = {}, t, 0.0
        while v >= 0:
            path[v] = acc
            acc += length[v]
            v = parent[v]
        anc.append(path)
    d = np.zeros((T, T))
    for i in range(T):
        for j in range(i + 1, T):
            d[i, j] = d[j, i] = min(anc[i][v] + anc[j][v] for v in anc[i] if v in anc[j])
    return d, parent, length


@pytest.mark.parametrize("T", [3, 4, 5, 12, 33, 128])
def test_nj_recovers_additive_trees_exactly(lib, T):
    d, parent, length = dyadic_tree(T, 100 + T)
    got_parent, got_length = distance.nj(d)
    assert got_parent.dtype == np.int32 and got_parent.shape == (2 * T - 2,) and got_length.shape == (2 * T - 2,)
    assert got_parent[2 * T - 3] == -1 and got_length[2 * T - 3] == 0.0 and (got_parent[:2 * T - 3] >= T).all()
    assert tm.splits(got_parent, T) == tm.splits(parent, T)
    assert tm.split_lengths(got_parent, got_length, T) == tm.split_lengths(parent, length, T)


@pytest.mark.parametrize("T", [4, 7, 33])
def test_nj_equals_the_model_bit_for_bit(lib, T):
    rng = np.random.default_rng(T)
    for trial in range(3):
        d = rng.random((T, T)) * (10.0 ** trial)
        if trial == 2:
            d -= 20.0                                              # negative entries are allowed
        d = np.triu(d, 1)
        d = d + d.T
        np.fill_diagonal(d, rng.random(T))                         # the diagonal is ignored
        parent, length = distance.nj(d)
        m_parent, m_length = tm.nj(d.tolist())
        assert parent.tolist() == m_parent
        assert length.tobytes() == np.array(m_length, np.float64).tobytes()


def test_nj_tie_rule_on_the_all_equal_matrix(lib):
    T = 6
    d = np.ones((T, T)) - np.eye(T)
    parent, length = distance.nj(d)
    # every Q ties in every round: the lowest pair of the active list is joined, the new node goes to its end
    assert parent.tolist() == [6, 6, 7, 7, 8, 8, 9, 9, 9, -1]
    assert parent.tolist() == tm.nj(d.tolist())[0]
    newick, p2, l2 = distance.nj_tree(d, samples=list("abcdef"))
    assert np.array_equal(p2, parent) and np.array_equal(l2, length) and np.array_equal(distance.nj_parents(d), parent)
    assert newick.startswith("((a:0.5,b:0.5):") and newick.endswith(";") and newick.count(":") == 2 * T - 3


def test_nj_refusals(lib):
    with pytest.raises(TetradHipError, match="at least 3"):
        distance.nj(np.zeros((2, 2)))
    d = np.ones((5, 5)) - np.eye(5)
    for bad in (np.nan, np.inf, -np.inf):
        e = d.copy()
        e[1, 3] = e[3, 1] = bad
        with pytest.raises(TetradHipError, match=r"pair \(1, 3\) is not finite"):
            distance.nj(e)
    e = d.copy()
    e[4, 2] = 1.5
    with pytest.raises(TetradHipError, match=r"not symmetric at the pair \(2, 4\)"):
        distance.nj(e)
    e = d.copy()
    e[0, 0] = np.nan                                               # the diagonal is ignored
    assert np.array_equal(distance.nj(e)[0], distance.nj(d)[0])
    parent = np.zeros(8, np.int32)
    assert lib.tq_nj_tree(None, 5, parent.ctypes.data, None) == -1


# -- recovery of the generating tree ---------------------------------------------------------------------------------
_SIM = {}


def simulated(T, S, seed):
    """(tmparr, tmpmap, host counts of one block, splits of the generating tree), computed once per input."""
    key = (T, S, seed)
    if key not in _SIM:
        tmparr, tmpmap = synth.simulate_tmparr(T, S, seed, p=0.05, missing=0.10)
        children, root = synth.random_tree_children(T, np.random.default_rng(seed))
        true = tm.splits(tm.children_to_parent(children, root, T), T)
        _SIM[key] = (tmparr, tmpmap, distance.taxon_counts_host(tmparr), true)
    return _SIM[key]


@pytest.mark.parametrize("model", ["p", "jc"])
@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("T,S", [(12, 4000), (33, 8000)])
def test_nj_recovers_the_generating_tree(lib, T, S, seed, model):
    _, _, c, true = simulated(T, S, seed)
    assert tm.splits(distance.nj_parents(distance.distances(c[0], model)), T) == true


# -- jackknife trees ---------------------------------------------------------------------------------------------------
def test_jackknife_trees_against_the_model(lib):
    tmparr, tmpmap, _, _ = simulated(12, 4000, 0)
    starts = np.linspace(0, 4000, 9).astype(np.int64)
    c = distance.taxon_counts_host(tmparr, starts)
    trees = distance.jackknife_nj_trees(c, "jc")
    assert len(trees) == 8
    mc = tm.counts(tmparr, starts).astype(np.int64)
    for j, parent in enumerate(trees):
        rest = mc.sum(axis=0) - mc[j]
        p = rest[..., 1] / rest[..., 0]
        d = -0.75 * np.log(1.0 - 4.0 * p / 3.0)
        np.fill_diagonal(d, 0.0)
        assert parent.tolist() == tm.nj(d.tolist())[0]


class HostEngine:
    """What `run_distance_tree` asks of an engine, on the host execution (the consensus then counts on the host too)."""
    _h = None

    def set_data(self, tmparr, tmpmap):
        self.tmparr = tmparr

    def taxon_counts(self, block_starts=None):
        return distance.taxon_counts_host(self.tmparr, block_starts)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_run_distance_tree_supports(lib, monkeypatch, seed):
    from tetrad_amd import consensus, patterns
    from tetrad_amd.concordance import newick_to_parent
    T, S = 12, 4000
    tmparr, tmpmap, _, true = simulated(T, S, seed)
    real = consensus.Consensus
    monkeypatch.setattr(consensus, "Consensus", lambda ntaxa, engine=None: real(ntaxa))        # host back end
    newick, counts = distance.run_distance_tree(HostEngine(), tmparr, tmpmap, model="jc", nblocks=50)
    starts = patterns.locus_blocks(tmpmap, 50)
    assert np.array_equal(counts, tm.counts(tmparr, starts))
    parent, T2, _ = newick_to_parent(newick)
    assert T2 == T and tm.splits(parent, T) == true
    # what the model gives: the share of the delete-one-block trees that hold each branch of the tree
    mc = tm.counts(tmparr, starts).astype(np.int64)
    held = {s: 0 for s in true}
    for j in range(len(starts) - 1):
        rest = mc.sum(axis=0) - mc[j]
        d = -0.75 * np.log(1.0 - 4.0 * (rest[..., 1] / rest[..., 0]) / 3.0)
        np.fill_diagonal(d, 0.0)
        for s in tm.splits(tm.nj(d.tolist())[0], T):
            if s in held:
                held[s] += 1
    B = len(starts) - 1
    labels = sorted(int(x) for x in __import__("re").findall(r"\)(\d+):", newick))
    assert labels == sorted((200 * n + B) // (2 * B) for n in held.values())
    assert labels == [100] * (T - 3)

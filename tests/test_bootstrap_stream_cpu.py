"""CPU: the model of the device bootstrap's random stream (tests/bootstrap_stream_model.py) -- that the NumPy restatement
is the arithmetic it claims to be (against plain Python integers and splitmix64's published outputs), that what it
returns is a valid replicate, and the statistics of the stream.  tests/test_gpu_bootstrap_layout.py pins the device to
the model bit for bit, so what is shown here holds for the device and is not repeated there.

Every statistic is a chi-square against its exact expectation, accepted when |stat - dof| < 5 sqrt(2 dof) (the bar of
tests/test_gpu_replicates.py); every expected cell holds at least 20.  The seeds are fixed, so the outcome is
deterministic; none had to be changed to pass."""
import numpy as np
import pytest

import bootstrap_stream_model as M

MASK = (1 << 64) - 1


def ok(stat, dof):
    return abs(stat - dof) < 5 * np.sqrt(2 * dof)


def chi2_uniform(counts):
    counts = np.asarray(counts, float).ravel()
    e = counts.sum() / counts.size
    assert e >= 20, e
    return float(((counts - e) ** 2 / e).sum()), counts.size - 1


def py_mix64(x):
    x = (x + 0x9E3779B97F4A7C15) & MASK
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & MASK
    return x ^ (x >> 31)


def test_mix64_is_splitmix64():
    # the first three outputs of splitmix64 seeded with 0 (Steele, Lea & Flood 2014; the values every port quotes)
    want = [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]
    got = [int(M.mix64(np.uint64((k * 0x9E3779B97F4A7C15) & MASK))) for k in range(3)]
    assert got == want
    xs = [0, 1, 2**31 - 1, 2**32, 2**63, MASK, 0x0123456789ABCDEF]
    assert [int(v) for v in M.mix64(np.array(xs, np.uint64))] == [py_mix64(x) for x in xs]


@pytest.mark.parametrize("seeds", [(0, 0), (2**31 - 1, 7), (2**40 + 12345, 2**63 + 99)])
def test_model_equals_plain_integer_arithmetic(seeds):
    """The vectorised model against the same stream written cell by cell with Python integers."""
    s1, s2 = seeds
    rng = np.random.default_rng(1)
    widths = [1, 2, 3, 33, 7, 64]
    starts = np.concatenate([[0], np.cumsum(widths)])
    spans = np.stack([starts[:-1], starts[1:]], axis=1)
    seqarr = rng.choice(np.frombuffer(b"ACGTNRKSYWM-", np.uint8), size=(4, int(starts[-1])))
    lidxs = np.array([3, 3, 0, 5, 1, 2, 4, 3])
    tmparr, tmpmap = M.replicate(seqarr, spans, lidxs, s1, s2)
    cols, locus = [], []
    for i, l in enumerate(lidxs):
        a, b = int(spans[l, 0]), int(spans[l, 1])
        p = list(range(a, b))
        state = py_mix64(s1 ^ ((i * 0xD1342543DE82EF95) & MASK))
        for j in range(b - a, 1, -1):
            state = py_mix64(state)
            r = ((state >> 32) * j) >> 32
            p[j - 1], p[r] = p[r], p[j - 1]
        cols += p
        locus += [i] * (b - a)
    res = {a: (one, zero) for a, one, zero in M.GETCONS}
    code = {65: 0, 67: 1, 71: 2, 84: 3}
    want = np.zeros((4, len(cols)), np.uint8)
    for t in range(4):
        for s, c in enumerate(cols):
            v = int(seqarr[t, c])
            coin = py_mix64(s2 ^ ((t * 0x9E3779B97F4A7C15) & MASK) ^ ((s * 0xC2B2AE3D27D4EB4F) & MASK)) >> 63
            if v in res:
                v = res[v][0] if coin else res[v][1]
            want[t, s] = code.get(v, 78)
    np.testing.assert_array_equal(tmparr, want)
    np.testing.assert_array_equal(tmpmap[:, 0], locus)
    np.testing.assert_array_equal(tmpmap[:, 1], np.arange(len(cols)))


def test_model_output_is_a_valid_replicate():
    from conftest import load_golden
    from oracle import resample as R
    g = load_golden("resample_T7_S300")
    tmparr, tmpmap = M.replicate(g["seqarr"], g["spans"], g["lidxs"], 111, 222)
    R.check_replicate(g["seqarr"], g["spans"], g["lidxs"], tmparr, tmpmap)


# ---- the coin ---------------------------------------------------------------------------------------------------------
def resolved_R(T, S, seed_ambig):
    """T taxa that are R at each of S sites (loci of one site, drawn in order): 1 where R became G, 0 where it became A."""
    spans = np.stack([np.arange(S), np.arange(S) + 1], axis=1)
    tmparr, _ = M.replicate(np.full((T, S), 82, np.uint8), spans, np.arange(S), 5, seed_ambig)
    assert set(np.unique(tmparr)) <= {0, 2}
    return tmparr >> 1


def assert_independent_coins(a, b, what):
    """Two coin sequences: they agree in half of the cells (2 cells), and the four outcomes are equally likely (4 cells)."""
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    s, d = chi2_uniform(np.bincount((a == b).astype(np.int64), minlength=2))
    assert ok(s, d), (what, "agreement", s, d)
    s, d = chi2_uniform(np.bincount(2 * a + b, minlength=4))
    assert ok(s, d), (what, "joint", s, d)


N_COIN = 40_000


@pytest.mark.parametrize("seed", [0, 9, 2**31 - 1, 2**45 + 3])
def test_coin_versus_taxon(seed):
    c = resolved_R(2, N_COIN, seed)
    assert_independent_coins(c[0], c[1], ("taxa 0 and 1", seed))


@pytest.mark.parametrize("seed", [0, 9, 2**31 - 1, 2**45 + 3])
@pytest.mark.parametrize("lag", [1, 32, 2048])
def test_coin_versus_site(seed, lag):
    c = resolved_R(1, N_COIN + lag, seed)[0]
    assert_independent_coins(c[:-lag], c[lag:], ("sites s and s+%d" % lag, seed))


@pytest.mark.parametrize("seed", [0, 9, 2**31 - 2, 2**45 + 3])
def test_coin_versus_seed(seed):
    a, b = resolved_R(1, N_COIN, seed)[0], resolved_R(1, N_COIN, seed + 1)[0]
    assert_independent_coins(a, b, ("seeds s and s+1", seed))


# ---- the shuffle ------------------------------------------------------------------------------------------------------
def drawn_orders(w, n, seed_shuffle):
    """One locus of w sites drawn n times, through the whole model: i64[n,w], entry [i,j] = the source column at position
    j of the draw at ordinal i.  The column number is written in the bases of four taxa (base-4 digits), so that it can be
    read back from the replicate."""
    assert w <= 256
    col = np.arange(w)
    seqarr = np.frombuffer(b"ACGT", np.uint8)[np.stack([(col >> (2 * k)) & 3 for k in range(4)])]
    tmparr, tmpmap = M.replicate(seqarr, np.array([[0, w]]), np.zeros(n, np.int64), seed_shuffle, 1)
    np.testing.assert_array_equal(tmpmap[:, 0], np.repeat(np.arange(n), w))
    got = sum(tmparr[k].astype(np.int64) << (2 * k) for k in range(4)).reshape(n, w)
    np.testing.assert_array_equal(np.sort(got, axis=1), np.tile(col, (n, 1)))       # every draw is a permutation
    return got


def landing(orders):
    """Position at which source column 0 lands, per draw."""
    return np.argmax(orders == 0, axis=1)


@pytest.mark.parametrize("seed", [0, 7, 2**31 - 1, 2**52 + 1])
@pytest.mark.parametrize("w", [2, 5, 33, 100])
def test_shuffle_lands_column_0_uniformly(w, seed):
    n = 60 * w
    pos = landing(drawn_orders(w, n, seed))
    s, d = chi2_uniform(np.bincount(pos, minlength=w))
    assert ok(s, d), (w, seed, s, d)
    # and the last column, the first one Fisher-Yates moves
    last = np.argmax(drawn_orders(w, n, seed) == w - 1, axis=1)
    s, d = chi2_uniform(np.bincount(last, minlength=w))
    assert ok(s, d), (w, seed, "last column", s, d)


@pytest.mark.parametrize("seed", [0, 7, 2**31 - 1, 2**52 + 1])
def test_shuffle_of_width_5_is_uniform_over_the_120_permutations(seed):
    o = drawn_orders(5, 120 * 50, seed)
    key = (o * 5 ** np.arange(5)).sum(axis=1)
    keys, counts = np.unique(key, return_counts=True)
    assert len(keys) == 120
    s, d = chi2_uniform(counts)
    assert ok(s, d), (seed, s, d)


@pytest.mark.parametrize("seed", [0, 7, 2**31 - 1, 2**52 + 1])
def test_shuffle_versus_ordinal(seed):
    """The same locus at ordinals i and i+1 (disjoint pairs): the joint landing position of column 0 is uniform on 5 x 5."""
    pos = landing(drawn_orders(5, 2 * 25 * 60, seed))
    s, d = chi2_uniform(np.bincount(5 * pos[0::2] + pos[1::2], minlength=25))
    assert ok(s, d), (seed, s, d)
    # neighbours the other way round (i odd), and ordinals 32 apart
    s, d = chi2_uniform(np.bincount(5 * pos[1:-1:2] + pos[2::2], minlength=25))
    assert ok(s, d), (seed, "odd", s, d)
    k = (len(pos) // 64) * 64
    blocks = pos[:k].reshape(-1, 2, 32)
    s, d = chi2_uniform(np.bincount((5 * blocks[:, 0] + blocks[:, 1]).ravel(), minlength=25))
    assert ok(s, d), (seed, "32 apart", s, d)


@pytest.mark.parametrize("seed", [0, 7, 2**31 - 2, 2**52 + 1])
def test_shuffle_versus_seed(seed):
    a, b = landing(drawn_orders(5, 25 * 60, seed)), landing(drawn_orders(5, 25 * 60, seed + 1))
    s, d = chi2_uniform(np.bincount(5 * a + b, minlength=25))
    assert ok(s, d), (seed, s, d)

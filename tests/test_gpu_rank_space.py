"""GPU: the kernels that turn a rank in [0, C(T,4)) into four taxa and an order -- `tq_sample_kernel` (keyed Feistel
permutation, cycle walk, unrank), `tq_unrank_kernel` (tq_unrank_dev, tq_resolve_range_dev, the `*_score_ranks` calls of the
quartet-distance and leaf-stability accumulators) and `tq_key_kernel` with the radix sort of make_order / make_units --
against the exact model of tests/rank_model.py, over the whole 64-bit rank space: T from 4 to
145 056, ranks on both sides of 2^32, 2^53 and 2^63, every half_bits of the sampler up to its 32-bit branch, and the three
regimes of the sort key.  Every comparison is exact: there are no tolerances here."""
from functools import lru_cache

import numpy as np
import pytest

import consensus_model as cm
import rank_model as rm
from exact_ties import check_rows
from tetrad_amd import _lib, synth
from tetrad_amd._lib import TetradHipError
from tetrad_amd.qdist import QuartetDistances
from tetrad_amd.stability import LeafStability

pytestmark = pytest.mark.gpu

SEEDS = (0, 12345, 2**63, 2**64 - 1)
SPACE_MSG = r"C\(%d,4\) does not fit 64 bits"


def torch_():
    import torch
    return torch


@pytest.fixture(scope="module")
def engine():
    from tetrad_amd.engine import QuartetEngine
    with QuartetEngine(0) as e:
        yield e


@pytest.fixture(scope="module")
def last_engine():
    """The last T whose rank space fits: about 1 GB on the device, uploaded once for every case that runs there."""
    from tetrad_amd.engine import QuartetEngine
    with QuartetEngine(0) as e:
        only_t(e, rm.T_MAX)
        yield e


def only_t(eng, T):
    """Data of which only T matters: one locus, every base A."""
    if eng.T != T or eng.S != 64 or getattr(eng, "_only_t", None) != eng.data_generation:
        eng.set_data(np.zeros((T, 64), np.uint8), np.zeros((64, 2), np.uint32))
        eng._only_t = eng.data_generation
    return eng


def pick(engine, last_engine, T):
    return last_engine if T == rm.T_MAX else only_t(engine, T)


def to_dev_u64(values):
    torch = torch_()
    return torch.from_numpy(np.array(values, np.uint64).view(np.int64)).to("cuda:0")


def u64(t):
    return t.cpu().numpy().view(np.uint64)


def u32(t):
    return t.cpu().numpy().view(np.uint32)


def dev_full(shape, dtype, value):
    torch = torch_()
    return torch.full(shape, value, dtype=dtype, device="cuda:0")


def stream():
    return torch_().cuda.current_stream().cuda_stream


@lru_cache(maxsize=None)
def unrank_case(T):
    ranks = rm.rank_list(T)
    return ranks, rm.unrank_many(ranks, T)


# ---- unranking --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("T", rm.T_LIST)
def test_unrank_dev_equals_the_model(engine, last_engine, T):
    torch = torch_()
    eng = pick(engine, last_engine, T)
    ranks, want = unrank_case(T)
    d_r = to_dev_u64(ranks)
    d_q = dev_full((len(ranks), 4), torch.int32, -1)
    eng.unrank_dev(d_r.data_ptr(), len(ranks), d_q.data_ptr(), stream())
    torch.cuda.synchronize()
    np.testing.assert_array_equal(u32(d_q), want)
    assert u64(d_r).tolist() == ranks                           # read back as uint64: the ranks reach 2^64 - 1.6e14


# ---- the sampler ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("T", rm.T_LIST)
def test_sampler_equals_the_model(engine, last_engine, T):
    """Which rank (seed, i) must give, and its quartet -- not only that the ranks are distinct and look uniform."""
    torch = torch_()
    eng = pick(engine, last_engine, T)
    total = rm.choose4(T)
    Q = total if T <= 27 else min(total, 4096)
    for seed in SEEDS:
        want_r = rm.sampler(seed, total, Q)
        want_q = rm.unrank_many(want_r, T)
        d_q, d_r = dev_full((Q, 4), torch.int32, -1), dev_full((Q,), torch.int64, -1)
        eng.sample_quartets_dev(seed, Q, d_q.data_ptr(), d_r.data_ptr(), stream())
        torch.cuda.synchronize()
        assert u64(d_r).tolist() == want_r, f"ranks, seed {seed}"
        np.testing.assert_array_equal(u32(d_q), want_q, err_msg=f"quartets, seed {seed}")
        d_q2 = dev_full((Q, 4), torch.int32, -1)
        eng.sample_quartets_dev(seed, Q, d_q2.data_ptr(), 0, stream())                      # no rank array
        torch.cuda.synchronize()
        np.testing.assert_array_equal(u32(d_q2), want_q, err_msg=f"quartets without ranks, seed {seed}")
        P = Q // 3
        if P:
            d_q3, d_r3 = dev_full((Q, 4), torch.int32, -1), dev_full((Q,), torch.int64, -1)
            eng.sample_quartets_dev(seed, P, d_q3.data_ptr(), d_r3.data_ptr(), stream())
            torch.cuda.synchronize()
            assert u64(d_r3)[:P].tolist() == want_r[:P] and (d_r3[P:] == -1).all(), f"prefix ranks, seed {seed}"
            np.testing.assert_array_equal(u32(d_q3)[:P], want_q[:P], err_msg=f"prefix quartets, seed {seed}")
            assert (d_q3[P:] == -1).all(), "rows past Q written"


# ---- ranges of ranks across 2^32 ----------------------------------------------------------------------------------------

def range_outputs(Q):
    torch = torch_()
    return (dev_full((Q, 4), torch.int32, -1), dev_full((Q, 2), torch.int32, -1),
            dev_full((Q, 3), torch.float64, -1.0), dev_full((Q,), torch.uint8, 255))


@pytest.mark.parametrize("where", ["across 2^32", "the last 200"])
def test_resolve_range_across_the_32_bit_boundary(engine, where):
    torch = torch_()
    T, Q = 569, 200
    total = rm.choose4(T)
    first = 2**32 - 100 if where == "across 2^32" else total - Q
    tmparr, tmpmap = synth.simulate_tmparr(T, 64, seed=569)
    engine.set_data(tmparr, tmpmap)
    quartets = rm.unrank_many(range(first, first + Q), T)
    assert first < 2**32 < first + Q or quartets[-1].tolist() == [565, 566, 567, 568]
    for sub in (False, True):
        want = engine.resolve(quartets, sub)
        for with_quartets in (True, False):
            d_q, d_rs, d_sc, d_fl = range_outputs(Q)
            engine.resolve_range_dev(first, Q, sub, d_q.data_ptr() if with_quartets else 0, d_rs.data_ptr(), d_sc.data_ptr(),
                                     d_fl.data_ptr(), stream())
            torch.cuda.synchronize()
            if with_quartets:
                np.testing.assert_array_equal(u32(d_q), quartets)
            for got, w in zip((u32(d_rs), d_sc.cpu().numpy(), d_fl.cpu().numpy()), want):
                np.testing.assert_array_equal(got, w, err_msg=f"sub={sub} with_quartets={with_quartets}")


# ---- the accumulators' rank calls across 2^32 ---------------------------------------------------------------------------

ACC_T, ACC_FIRST, ACC_Q = 569, 2**32 - 200, 400


@lru_cache(maxsize=None)
def acc_case():
    trees = [cm.caterpillar(ACC_T), cm.balanced(ACC_T), cm.random_binary(ACC_T, np.random.default_rng(ACC_T))]
    ranks = np.arange(ACC_FIRST, ACC_FIRST + ACC_Q, dtype=np.uint64)
    quartets = rm.unrank_many(ranks.tolist(), ACC_T).astype(np.int32)
    return trees, ranks, quartets


def test_quartet_distance_ranks_across_the_32_bit_boundary(engine):
    trees, ranks, quartets = acc_case()
    raws = []
    for eng in (engine, None):
        for how in ("quartets", "ranks", "range"):
            with QuartetDistances(ACC_T, 3, engine=eng) as acc:
                acc.add_parents(trees)
                if how == "quartets":
                    acc.score(quartets)
                elif how == "ranks":
                    acc.score_ranks(ranks)
                else:
                    acc.score_range(ACC_FIRST, ACC_Q)
                assert acc.nquartets == ACC_Q
                raws.append(acc.raw())
    assert raws[0][1].diagonal().tolist() == [ACC_Q] * 3            # binary trees resolve every quartet
    for other in raws[1:]:
        for a, b in zip(other, raws[0]):
            np.testing.assert_array_equal(a, b)


def test_leaf_stability_ranks_across_the_32_bit_boundary(engine):
    trees, ranks, quartets = acc_case()
    out = []
    for eng in (engine, None):
        for how in ("quartets", "ranks", "range"):
            with LeafStability(ACC_T, 3, engine=eng) as acc:
                acc.add_parents(trees)
                if how == "quartets":
                    table = acc.score(quartets, counts=True)
                elif how == "ranks":
                    table = acc.score_ranks(ranks, counts=True)
                else:
                    table = acc.score_range(ACC_FIRST, ACC_Q, counts=True)
                assert acc.nquartets == ACC_Q
                out.append((table, acc.raw()))
    assert (out[0][0].sum(axis=1) == 3).all() and out[0][1][:, 0].sum() == 4 * ACC_Q
    for table, raw in out[1:]:
        np.testing.assert_array_equal(table, out[0][0])
        np.testing.assert_array_equal(raw, out[0][1])


# ---- refusals -----------------------------------------------------------------------------------------------------------

def one_range(eng, first, Q, rows=None):
    """tq_resolve_range_dev of Q ranks from `first` into arrays of `rows` rows; returns (quartets, flags)."""
    torch = torch_()
    d_q, d_rs, d_sc, d_fl = range_outputs(rows or Q)
    eng.resolve_range_dev(first, Q, False, d_q.data_ptr(), d_rs.data_ptr(), d_sc.data_ptr(), d_fl.data_ptr(), stream())
    torch.cuda.synchronize()
    return u32(d_q), d_fl.cpu().numpy()


@pytest.mark.parametrize("T", [8, 569, 102_571, rm.T_MAX])
def test_resolve_range_refuses_ranges_past_the_space(engine, last_engine, T):
    eng = pick(engine, last_engine, T)
    total = rm.choose4(T)
    last = [[T - 4, T - 3, T - 2, T - 1]]
    for first, Q in ((2**64 - 1, 2), (total, 1), (total - 1, 2)):
        with pytest.raises(TetradHipError, match=r"TQ_ERR_INVALID_ARG.*rank range \[%d,\+%d\) exceeds C\(%d,4\)=%d" % (first, Q, T, total)):
            one_range(eng, first, Q, rows=2)
        q, fl = one_range(eng, total - 1, 1)                        # the next valid call, and the last rank of the space
        np.testing.assert_array_equal(q, last)
        assert fl.tolist() == [_lib.FLAG_ZERO_DATA]                 # every base alike: no variable site


def test_sampler_refuses_more_than_the_space_holds(engine):
    """At T = 102 571 the product C(T,3) (T-3) passes 2^64: the refusal must quote the true C(T,4)."""
    torch = torch_()
    T = 102_571
    eng = only_t(engine, T)
    total = rm.choose4(T)
    d_q, d_r = dev_full((4, 4), torch.int32, -1), dev_full((4,), torch.int64, -1)
    with pytest.raises(TetradHipError, match=r"TQ_ERR_INVALID_ARG.*C\(%d,4\)=%d$" % (T, total)):
        eng.sample_quartets_dev(1, total + 1, d_q.data_ptr(), d_r.data_ptr(), stream())
    eng.sample_quartets_dev(1, 4, d_q.data_ptr(), d_r.data_ptr(), stream())
    torch.cuda.synchronize()
    assert u64(d_r).tolist() == rm.sampler(1, total, 4)


def test_every_rank_call_refuses_a_space_past_64_bits(engine):
    torch = torch_()
    T = rm.T_MAX + 1
    eng = only_t(engine, T)
    d_q, d_r = dev_full((4, 4), torch.int32, -1), dev_full((4,), torch.int64, 0)
    d_rs, d_sc, d_fl = dev_full((4, 2), torch.int32, -1), dev_full((4, 3), torch.float64, -1.0), dev_full((4,), torch.uint8, 255)
    calls = {
        "tq_unrank_dev": lambda: eng.unrank_dev(d_r.data_ptr(), 4, d_q.data_ptr(), stream()),
        "tq_sample_quartets_dev": lambda: eng.sample_quartets_dev(1, 4, d_q.data_ptr(), d_r.data_ptr(), stream()),
        "tq_resolve_range_dev": lambda: eng.resolve_range_dev(0, 4, False, d_q.data_ptr(), d_rs.data_ptr(), d_sc.data_ptr(),
                                                              d_fl.data_ptr(), stream()),
    }
    for name, call in calls.items():
        with pytest.raises(TetradHipError, match=r"TQ_ERR_INVALID_ARG: %s: " % name + SPACE_MSG % T):
            call()
        torch.cuda.synchronize()
        assert (d_q == -1).all(), f"{name} wrote quartets"
        rstat, rscor, flags = eng.resolve(np.array([[0, 1, T - 2, T - 1]], np.uint32), False)      # the next valid call
        assert flags.tolist() == [_lib.FLAG_ZERO_DATA]


# ---- ordering: the three regimes of the sort key ------------------------------------------------------------------------

ORDER_Q, ORDER_CHUNK, ORDER_POOL, ORDER_SAMPLE = 33_000, 8_000, 3_000, 300


@lru_cache(maxsize=2)
def order_case(T):
    """Unsorted rows with taxa over the whole range (keys with their high bits set), ORDER_POOL rows from 40 taxa in
    rising order (workgroups share (a,b), and (a,b,c) repeats so that the joint-histogram scan pairs), 5 bad rows."""
    rng = np.random.default_rng(T)
    tmparr, tmpmap = synth.simulate_tmparr(T, 64, seed=T, missing=0.20)
    wide = rng.integers(0, T, (ORDER_Q - ORDER_POOL, 4), dtype=np.int64)
    wide[:200] = np.array([T - 1, T - 2, T - 3, T - 4]) - rng.integers(0, 30, (200, 1)) * 4         # the highest keys
    while True:
        s = np.sort(wide, axis=1)
        again = (np.diff(s, axis=1) == 0).any(axis=1)
        if not again.any():
            break
        wide[again] = rng.integers(0, T, (int(again.sum()), 4))
    pool = np.sort(rng.choice(T, 40, replace=False))
    small = np.stack([np.sort(rng.choice(pool, 4, replace=False)) for _ in range(ORDER_POOL)])
    assert len(np.unique(small[:, :3], axis=0)) < ORDER_POOL - 500          # many rows share (a,b,c)
    q = np.concatenate([wide, small])[rng.permutation(ORDER_Q)].astype(np.uint32)
    bad_rows = np.sort(rng.choice(ORDER_Q, 5, replace=False))
    bad = q.copy()
    bad[bad_rows, [0, 1, 2, 3, 0]] = [T, T + 3, 0xFFFFFFFF, 0x80000000, max(T, 65_536)]
    for a in (tmparr, tmpmap, q, bad, bad_rows):
        a.setflags(write=False)
    return tmparr, tmpmap, q, bad, bad_rows


def resolve_dev_rows(eng, d_q, lo, hi, sub):
    torch = torch_()
    n = hi - lo
    d_rs, d_sc, d_fl = dev_full((n, 2), torch.int32, -1), dev_full((n, 3), torch.float64, -1.0), dev_full((n,), torch.uint8, 255)
    eng.resolve_dev(d_q[lo:hi].data_ptr(), n, sub, d_rs.data_ptr(), d_sc.data_ptr(), d_fl.data_ptr(), stream())
    torch.cuda.synchronize()
    return u32(d_rs), d_sc.cpu().numpy(), d_fl.cpu().numpy(), eng.last_scan()[0]


@pytest.mark.parametrize("T", [1625, 1626, 65_535, 65_536])
def test_one_sorted_call_equals_chunks_in_natural_order(engine, oracle, T):
    """T <= 1625: key (a,b,c); up to 65 535: key (a,b), all 32 bits of it at 65 535; above: no sort.  Chunks of 8 000 are
    below the sort's threshold of 32 768 quartets, so they run in natural order: chunk invariance
    makes them the expectation, bit for bit."""
    torch = torch_()
    tmparr, tmpmap, q, bad, bad_rows = order_case(T)
    engine.set_data(tmparr, tmpmap)
    d_bad = torch.from_numpy(bad.view(np.int32).copy()).to("cuda:0")
    d_good = torch.from_numpy(q.view(np.int32).copy()).to("cuda:0")
    good = np.setdiff1d(np.arange(ORDER_Q), bad_rows)
    rows = np.sort(np.random.default_rng(T + 1).choice(good, ORDER_SAMPLE, replace=False))
    for sub in (False, True):
        whole = resolve_dev_rows(engine, d_bad, 0, ORDER_Q, sub)
        if not sub:
            assert (whole[3] == "dp") == (T == 1625), f"full-mode kernel form {whole[3]} at T = {T}"
        parts = [resolve_dev_rows(engine, d_bad, lo, min(lo + ORDER_CHUNK, ORDER_Q), sub) for lo in range(0, ORDER_Q, ORDER_CHUNK)]
        assert all(p[3] != "dp" for p in parts)
        for k, what in enumerate(("rstat", "rscor", "flags")):
            np.testing.assert_array_equal(whole[k], np.concatenate([p[k] for p in parts]), err_msg=f"{what}, sub={sub}")
        # the bad rows are flagged, zero-data rows; the others do not know about them
        rstat, rscor, flags = whole[:3]
        assert (flags[bad_rows] & _lib.FLAG_BAD_INDEX).all() and not (flags[good] & _lib.FLAG_BAD_INDEX).any()
        assert (rstat[bad_rows, 1] == 0).all()
        clean = resolve_dev_rows(engine, d_good, 0, ORDER_Q, sub)
        for k, what in enumerate(("rstat", "rscor", "flags")):
            np.testing.assert_array_equal(whole[k][good], clean[k][good], err_msg=f"{what} beside bad rows, sub={sub}")
        # sampled rows against the oracle, ties judged exactly; the debug call (natural order) equals the sorted call
        d_rstat, d_rscor, d_flags, dbg = engine.resolve(q[rows], sub, debug=True)
        for a, b in zip((rstat[rows], rscor[rows], flags[rows]), (d_rstat, d_rscor, d_flags)):
            np.testing.assert_array_equal(a, b, err_msg=f"sorted call != debug call, sub={sub}")
        _, o_rstat, o_rscor, o = oracle.new_infer_resolved_quartets(tmparr, tmpmap, q[rows], sub, debug=True)
        n = check_rows((rstat[rows], rscor[rows], flags[rows]), dbg, (o_rstat, o_rscor, o))
        assert n["rows"] == ORDER_SAMPLE and n["zero"] < ORDER_SAMPLE // 2, n

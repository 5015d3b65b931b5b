"""GPU: the resident layout and the random stream of a device-built bootstrap replicate (tq_bootstrap, csrc/bootstrap.hpp).

tq_boot_build_kernel writes every array of the resident layout itself -- byte rows, nib, nib5, the 16-byte plane records,
the 12-byte plane records and the shared run-begin word -- beside tq_prepare_rows (csrc/prepare.hpp), which writes the same
arrays for tq_set_data.  tq_get_data shows the byte rows and the 16-byte records only.  So:

* ROUND TRIP.  Engine A builds a replicate, exports it, engine B takes the export through tq_set_data; both resolve the
  same quartets under every form of the scan (each reads another subset of the arrays) and must agree BITWISE in rstat,
  rscor, flags and the count matrices; B's counts must be the oracle's.  Replicate lengths sit on and next to the 2048-site
  step and the 32-site word, loci are wider than a word and than a step with their counted sites deep inside, one locus
  repeats under successive ordinals, and one engine walks through the life cycle of its buffers: reuse of tq_set_data's
  allocation under a stale packed set, a short replicate over a long one, the head-room of tq_bootstrap's own allocation
  and the replicates that outgrow it, another number of taxa, tq_set_data again.  (The shared run-begin word is the one
  array this cannot reach: no kernel reads DevData::runbeg, the scans take the bits from the 16-byte records.)
* STREAM.  The exported replicate equals, bit for bit, what tests/bootstrap_stream_model.py computes from the same source,
  draws and seeds (tests/test_bootstrap_stream_cpu.py checks that model's statistics on the CPU).
"""
import numpy as np
import pytest

import bootstrap_stream_model as model

pytestmark = pytest.mark.gpu

TILE = 2048                      # sites per scan step: replicates are padded to a multiple (csrc/common.hpp)
SPECIAL = [1, 2, 3, 31, 32, 33, 63, 64, 65, 100, 2047, 2048, 2100]
L = {w: i for i, w in enumerate(SPECIAL)}          # locus index of each special width
DEAD = 7                         # the all-missing taxon

DEFAULTS = {"wg_min_quartets": 0, "dp_min_quartets": 0, "scan_f4": -1, "scan_dp": 1, "scan_method": -1, "scan_pair": 0,
            "share_c": 0, "park_t": 1, "scan_wg": 0, "order": 1}


def option_sets(sub):
    """(wg_min_quartets, options): the one-wave kernel, then every cooperative form at a batch of 64 or more."""
    return [(0, {})] + [(64, o) for o in (
        {}, {"dp_min_quartets": 2}, {"scan_f4": 0}, {"scan_f4": 1}, {"scan_dp": 0}, {"scan_method": 6},
        {"scan_method": 1 - int(sub)}, {"scan_pair": 1}, {"share_c": 1}, {"park_t": 0}, {"scan_wg": 8}, {"order": 0})]


def padded(S):
    return -(-S // TILE) * TILE


def capacity_of_new_allocation(S):
    """tq_bootstrap_async: capSp = align_up(Sp + Sp / 8, TILE)."""
    return padded(padded(S) + padded(S) // 8)


def layout_source(T, seed):
    """(seqarr u8[T,S0] ASCII, spans): the SPECIAL widths, then 60 loci of 1 + Poisson(3) sites; ~15 % N, ~3 % IUPAC
    two-base codes, taxon DEAD all N; in the loci wider than a word every taxon misses a random number of the first sites."""
    from tetrad_amd import synth
    rng = np.random.default_rng(seed)
    widths = np.array(SPECIAL + (1 + rng.poisson(3, size=60)).tolist())
    ends = np.cumsum(widths)
    spans = np.stack([ends - widths, ends], axis=1).astype(np.int64)
    tmparr, _ = synth.simulate_tmparr(T, int(ends[-1]), seed=seed, missing=0.15)
    seqarr = np.where(tmparr <= 3, np.frombuffer(b"ACGT", np.uint8)[np.minimum(tmparr, 3)], 78).astype(np.uint8)
    amb = rng.random(seqarr.shape) < 0.03
    seqarr[amb] = rng.choice(np.frombuffer(b"RKSYWM", np.uint8), size=int(amb.sum()))
    for (a, b), n in zip(spans, widths):
        if n > 32:
            for t in range(T):
                seqarr[t, a:a + int(rng.integers(0, n))] = 78
    seqarr[DEAD] = 78
    return seqarr, spans


def draws(spans, first, target):
    """nloci locus indices that give exactly `target` sites: the hand-picked `first`, then the loci of at most 100 sites
    taken in turn, skipping one after which the remaining draws could no longer add up to the target; dealt out so that
    the wide loci do not sit in a row."""
    widths = (spans[:, 1] - spans[:, 0]).tolist()
    n = len(widths)
    small = [i for i, w in enumerate(widths) if w <= 100]
    picked = list(first)
    m, rest = n - len(picked), target - sum(widths[i] for i in picked)
    assert m <= rest <= 100 * m, (m, rest)
    reach = np.zeros((m + 1, rest + 1), bool)                # reach[k, r]: k draws of small loci can add up to r sites
    reach[0, 0] = True
    for k in range(1, m + 1):
        for w in {widths[i] for i in small}:
            reach[k, w:] |= reach[k - 1, :rest + 1 - w]
    assert reach[m, rest]
    turn = 0
    for left in range(m - 1, -1, -1):                        # draws still to come after this one
        while widths[small[turn % len(small)]] > rest or not reach[left, rest - widths[small[turn % len(small)]]]:
            turn += 1
        picked.append(small[turn % len(small)])
        rest -= widths[picked[-1]]
        turn += 1
    assert rest == 0 and len(picked) == n
    lidxs = np.array([picked[(k * 31) % n] for k in range(n)], np.int64)         # n = 73 is prime: a permutation
    assert sorted(lidxs.tolist()) == sorted(picked)
    assert int((spans[lidxs, 1] - spans[lidxs, 0]).sum()) == target
    return lidxs


def quartet_sets(T, seed=3):
    """All quartets of T taxa, sorted and permuted; at least 64 rows (the cooperative kernels take 64 or more)."""
    from tetrad_amd import synth
    q = np.ascontiguousarray(synth.all_quartets(T), dtype=np.uint32)
    if len(q) < 64:
        q = np.concatenate([q] * -(-64 // len(q)))
    return [q, np.ascontiguousarray(q[np.random.default_rng(seed).permutation(len(q))])]


def resolve_under(eng, q, sub, wg, opts):
    eng.set_option("wg_min_quartets", wg)
    for k, v in opts.items():
        eng.set_option(k, v)
    try:
        rstat, rscor, flags, dbg = eng.resolve(q, sub, debug=True)
    finally:
        for k in ("wg_min_quartets", *opts):
            eng.set_option(k, DEFAULTS[k])
    return [("rstat", np.array(rstat)), ("rscor", np.array(rscor)), ("flags", np.array(flags)), ("cmats", dbg["cmats"])]


def round_trip(A, B, qsets, oracle, what):
    """What A holds (however it got there) against tq_set_data of its export on B, under every scan form; B against the
    oracle.  Returns the export."""
    tmparr, tmpmap = A.get_data()
    B.set_data(tmparr, tmpmap)
    assert B.site_pack_state() == (0, False)
    for sub in (True, False):
        _, o_rstat, _, o = oracle.new_infer_resolved_quartets(tmparr, tmpmap, qsets[0], sub, debug=True)
        for qi, q in enumerate(qsets):
            for wg, opts in option_sets(sub):
                a, b = resolve_under(A, q, sub, wg, opts), resolve_under(B, q, sub, wg, opts)
                for (name, x), (_, y) in zip(a, b):
                    assert x.dtype == y.dtype and x.shape == y.shape
                    np.testing.assert_array_equal(x.view(np.uint8), y.view(np.uint8),
                                                  err_msg=f"{what}: replicate vs set_data of its export, {name}, sub={sub}, "
                                                          f"wg_min_quartets={wg} {opts}, quartet set {qi}")
                if qi == 0 and not opts:
                    got = dict(b)
                    np.testing.assert_array_equal(got["cmats"], o["cmats"], err_msg=f"{what}: oracle counts, sub={sub}")
                    np.testing.assert_array_equal(got["rstat"][:, 1], o_rstat[:, 1], err_msg=f"{what}: oracle nsnps")
    return tmparr, tmpmap


def replicate_and_check(A, B, src, lidxs, seeds, S, qsets, oracle, what):
    seqarr, spans = src
    assert len(lidxs) == len(spans)
    assert A.bootstrap(lidxs, *seeds) == S == int((spans[lidxs, 1] - spans[lidxs, 0]).sum())
    assert not A.site_pack_state()[1]
    tmparr, tmpmap = round_trip(A, B, qsets, oracle, what)
    m_arr, m_map = model.replicate(seqarr, spans, lidxs, *seeds)
    np.testing.assert_array_equal(tmparr, m_arr, err_msg=f"{what}: stream model, tmparr")
    np.testing.assert_array_equal(tmpmap, m_map, err_msg=f"{what}: stream model, tmpmap")


@pytest.fixture(scope="module")
def source10():
    src = layout_source(10, seed=12)
    assert len(src[1]) == 73
    return src


@pytest.fixture(scope="module")
def engines():
    from tetrad_amd.engine import QuartetEngine
    with QuartetEngine(0) as A, QuartetEngine(0) as B:
        B.set_option("site_pack", 0)
        yield A, B


# name -> (hand-picked first draws, number of sites).  73 draws each; the rest of the draws is filled in by `draws`.
LENGTHS = {
    "one step, no padding": ([L[65], L[64], L[63], L[33], L[32], L[31]], 2048),
    "three steps, no padding": ([L[2100], L[2048], L[65], L[33]], 3 * 2048),
    "one step + 1": ([L[100], L[100], L[65], L[33]], 2048 + 1),                     # = 1 modulo 32 as well
    "two steps - 1": ([L[2047], L[64], L[63], L[33]], 2 * 2048 - 1),               # = 31 modulo 32 as well
    "31 modulo 32": ([L[2048], L[2047], L[100], L[65]], 3 * 2048 + 31),
    "1 modulo 32": ([L[2100], L[2100], L[33]], 2 * 2048 + 1024 + 1),
}


@pytest.mark.parametrize("name", list(LENGTHS))
def test_round_trip_at_step_and_word_edges(engines, source10, oracle, name):
    A, B = engines
    first, S = LENGTHS[name]
    A.set_source(*source10)
    lidxs = draws(source10[1], first, S)
    replicate_and_check(A, B, source10, lidxs, (41, 43), S, quartet_sets(10), oracle, name)


@pytest.mark.parametrize("w", [65, 2100])
def test_round_trip_one_wide_locus_under_every_ordinal(engines, source10, oracle, w):
    """The same source columns 73 times: a run begins at every offset inside a word (65) and steps apart (2100)."""
    A, B = engines
    A.set_source(*source10)
    lidxs = np.full(73, L[w], np.int64)
    replicate_and_check(A, B, source10, lidxs, (5, 6), 73 * w, quartet_sets(10), oracle, f"73 x width {w}")


def test_round_trip_every_site_a_locus(engines, source10, oracle):
    A, B = engines
    A.set_source(*source10)
    spans = source10[1]
    ones = np.flatnonzero(spans[:, 1] - spans[:, 0] == 1)
    assert len(ones) >= 2
    lidxs = ones[np.arange(73) % len(ones)]
    replicate_and_check(A, B, source10, lidxs, (8, 9), 73, quartet_sets(10), oracle, "width-1 loci only")


def test_round_trip_one_site(engines, oracle):
    """A source of one locus of one site: S = 1 (the shape of the golden case one_site_T5_S1)."""
    A, B = engines
    src = (np.frombuffer(b"ACRNG", np.uint8).reshape(5, 1).copy(), np.array([[0, 1]], np.int64))
    A.set_source(*src)
    replicate_and_check(A, B, src, np.zeros(1, np.int64), (1, 2), 1, quartet_sets(5), oracle, "one site")


@pytest.mark.parametrize("seeds", [(0, 2**31 - 1), (2**31 - 1, 0), (2**32 + 5, 2**63 + 11)])
def test_device_stream_equals_the_model(engines, source10, seeds):
    """tq_bootstrap's replicate, array against array, for seeds at the ends of the reference's range (it draws them from
    [0, 2^31)) and beyond 32 bits (the C ABI takes uint64_t)."""
    A, _ = engines
    seqarr, spans = source10
    A.set_source(seqarr, spans)
    lidxs = draws(spans, [L[2100], L[2048], L[2047], L[100], L[65], L[3], L[2]], 3 * 2048 + 777)
    assert A.bootstrap(lidxs, *seeds) == 3 * 2048 + 777
    tmparr, tmpmap = A.get_data()
    m_arr, m_map = model.replicate(seqarr, spans, lidxs, *seeds)
    np.testing.assert_array_equal(tmparr, m_arr)
    np.testing.assert_array_equal(tmpmap, m_map)
    assert set(np.unique(tmparr)) == {0, 1, 2, 3, 78}


def test_round_trip_through_the_buffer_life_cycle(source10, oracle):
    """One engine; after every step what it holds must resolve like tq_set_data of its export."""
    from tetrad_amd import synth
    from tetrad_amd.engine import QuartetEngine
    seqarr, spans = source10
    q10, q12 = quartet_sets(10), quartet_sets(12)
    assert len(q12[0]) == 495
    with QuartetEngine(0) as A, QuartetEngine(0) as B:
        B.set_option("site_pack", 0)
        A.set_option("site_pack", 1)
        # (a) tq_set_data sizes the buffers: capacity 5 steps (320 plane words per row), and a packed set
        big = synth.simulate_tmparr(10, 5 * TILE, seed=31, missing=0.15)
        A.set_data(*big)
        assert A.site_pack_state()[1]
        cap = padded(5 * TILE)
        A.set_source(seqarr, spans)

        def step(first, S, reallocates, what):
            nonlocal cap
            assert (padded(S) > cap) == reallocates, (what, S, cap)
            if reallocates:
                cap = capacity_of_new_allocation(S)
            replicate_and_check(A, B, source10, draws(spans, first, S), (S, S + 1), S, q10, oracle, what)

        # capacity 10 240 from tq_set_data: reused, W = 256 < the 320 words of the allocation, the packed set is stale
        step([L[2100], L[2048], L[65]], 3 * TILE + 1, False, "a: after a packed tq_set_data")
        # (b) short after long: the long replicate's words lie behind Sp = 4 096
        step([L[100], L[65], L[33]], TILE + 1, False, "b: short after long")
        # (c) capacity 10 240 still (tq_set_data leaves no head-room): filled to the last site, W = the allocation's 320 words again
        step([L[2100]] * 3 + [L[2048]], 5 * TILE, False, "c: fills the allocation of tq_set_data")
        # (d) one site more: Sp = 12 288 > 10 240 -> new allocation of align(12 288 + 1 536) = 14 336
        step([L[2100]] * 4, 5 * TILE + 1, True, "d: outgrows the allocation of tq_set_data")
        assert cap == 14336
        # (c) Sp = 14 336: the last step of the head-room of that allocation, no new one
        step([L[2100]] * 5 + [L[2048]], 7 * TILE, False, "c: inside the head-room")
        step([L[2047], L[65]], 2 * TILE - 1, False, "b: short after the longest")
        # (d) Sp = 16 384 > 14 336 -> new allocation of align(16 384 + 2 048) = 18 432
        step([L[2100]] * 6, 7 * TILE + 1, True, "d: beyond the head-room")
        assert cap == 18432
        # (e) another number of taxa: new allocation although the replicate is short (align(4 096 + 512) = 6 144)
        src12 = layout_source(12, seed=13)
        assert len(src12[1]) == 73
        A.set_source(*src12)
        S = TILE + 33
        replicate_and_check(A, B, src12, draws(src12[1], [L[100], L[65], L[33]], S), (3, 4), S, q12, oracle, "e: 12 taxa")
        # (f) tq_set_data again takes a fresh packed set
        A.set_data(*big)
        assert A.site_pack_state()[1]
        tmparr, tmpmap = round_trip(A, B, q10, oracle, "f: tq_set_data after the replicates")
        np.testing.assert_array_equal(tmparr, np.where(big[0] <= 3, big[0], 78))


def test_round_trip_at_the_natural_thresholds(oracle):
    """32 taxa, all 35 960 quartets, default options: the device sort, tq_scan_f4_kernel (subsample mode) and
    tq_scan_dp_kernel with its unit list (full mode, 32 768 quartets and more) on a drawn replicate."""
    from tetrad_amd import bootstrap, synth
    from tetrad_amd.engine import QuartetEngine
    seqarr, _, spans = synth.make_c5_source(T=32, S=4000, seed=19, ambiguous=0.03)
    seqarr[11] = 78
    q = np.ascontiguousarray(synth.all_quartets(32), dtype=np.uint32)
    assert len(q) == 35960
    rows = np.linspace(0, len(q) - 1, 300).astype(np.int64)
    with QuartetEngine(0) as A, QuartetEngine(0) as B:
        B.set_option("site_pack", 0)
        A.set_source(seqarr, spans)
        lidxs, s1, s2 = bootstrap.draw_replicate(len(spans), np.random.default_rng(77))
        A.bootstrap(lidxs, s1, s2)
        tmparr, tmpmap = A.get_data()
        np.testing.assert_array_equal(tmparr, model.replicate(seqarr, spans, lidxs, s1, s2)[0])
        B.set_data(tmparr, tmpmap)
        for sub in (True, False):
            a, b = A.resolve(q, sub), B.resolve(q, sub)
            for x, y, name in zip(a, b, ("rstat", "rscor", "flags")):
                np.testing.assert_array_equal(np.array(x).view(np.uint8), np.array(y).view(np.uint8), err_msg=f"{name} sub={sub}")
            _, o_rstat, _, o = oracle.new_infer_resolved_quartets(tmparr, tmpmap, q[rows], sub, debug=True)
            rstat, flags = np.array(a[0])[rows], np.array(a[2])[rows]
            np.testing.assert_array_equal(rstat[:, 1], o_rstat[:, 1])
            ok = ((flags | o["flags"]) & 3) == 0
            assert ok.sum() > 200
            np.testing.assert_array_equal(rstat[ok, 0], o_rstat[ok, 0])

"""CPU: the packed site order of option ``site_pack`` (csrc/pack.hpp) through the exported packer tq_pack_sites.

The subsample-mode count matrix is a histogram over loci (one counted site per locus run), so the device may hold the
sites in any order that keeps every locus together and in its own order.  Checked here, without a GPU:

* the map is a permutation of the sites plus pads, and the layout rules hold (a locus stays adjacent and ordered, one
  of <= 32 sites never straddles a lane word, a longer one starts a word and fills consecutive words, a pad follows the
  run it belongs to and the length is a multiple of 2048);
* the sites a quartet counts are the same set in both layouts (the reference's rule, resolve_quartets.py:58-64,
  applied to the packed arrays with pads missing and without a run-begin);
* the walk-trip model (sum over 2048-site steps of the largest number of counted sites in one of the 64 lane words,
  200 random quartets) falls to <= 0.80 of the natural layout's on c3 and c4 at no more than 2 / 5 extra steps;
* the automatic rule takes the packed layout on c3 and leaves the sparse rad60 matrix alone."""
import numpy as np
import pytest

from tetrad_amd import synth
from tetrad_amd.engine import PACK_PAD, pack_sites

TILE = 2048


def check_rules(src, locus):
    """Rules 1-3 and 5 of the layout + permutation; returns the number of steps."""
    S = len(locus)
    assert src.dtype == np.uint32 and len(src) % TILE == 0 and len(src) >= TILE
    pad = src == PACK_PAD
    real = src[~pad].astype(np.int64)
    assert np.array_equal(np.sort(real), np.arange(S)), "not a permutation of the sites"
    pos = np.empty(S, np.int64)
    pos[real] = np.flatnonzero(~pad)
    starts = np.flatnonzero(np.r_[True, locus[1:] != locus[:-1]])
    ends = np.r_[starts[1:], S]
    # rule 1: inside a locus, consecutive sites sit at consecutive positions
    same = locus[1:] == locus[:-1]
    assert np.all(pos[1:][same] == pos[:-1][same] + 1), "a locus is split or reordered"
    lens = ends - starts
    first, last = pos[starts], pos[ends - 1]
    short = lens <= 32
    # rule 2: a locus of <= 32 sites lies inside one word
    assert np.all(first[short] >> 5 == last[short] >> 5), "a short locus straddles a word"
    # rule 3: a longer locus starts a word (consecutive words follow from rule 1)
    assert np.all(first[~short] & 31 == 0), "a long locus does not start a word"
    # rule 5: a pad never starts a word that a locus continues into, i.e. every pad is followed, inside its word, by
    # pads only (it belongs to the run before it); the first position of every word that holds sites is a site
    w = src.reshape(-1, 32) == PACK_PAD
    assert not np.any(w[:, :-1] & ~w[:, 1:]), "a site follows a pad inside a word"
    return len(src) // TILE


def packed_arrays(src, tmparr, locus):
    """The packed matrix as the device builds it: pads missing, a pad's locus = that of the run before it."""
    pad = src == PACK_PAD
    take = np.where(pad, 0, src).astype(np.int64)
    parr = np.where(pad[None, :], np.uint8(78), tmparr[:, take])
    last = np.maximum.accumulate(np.where(pad, -1, np.arange(len(src))))
    ploc = np.where(last >= 0, locus.astype(np.int64)[take[np.maximum(last, 0)]], -1)
    return parr, ploc


def counted_sites(arr4, locus):
    """resolve_quartets.py:58-64, 216-218: unmasked = no taxon missing and the four bases not all equal; counted = unmasked
    and its locus differs from the locus of the previous unmasked site."""
    idx = np.flatnonzero((arr4 <= 3).all(axis=0) & (arr4 != arr4[0]).any(axis=0))
    if not len(idx):
        return idx
    loc = locus[idx]
    return idx[np.r_[True, loc[1:] != loc[:-1]]]


def trips(sites, nsites):
    words = -(-nsites // TILE) * 64
    return int(np.bincount(sites >> 5, minlength=words).reshape(-1, 64).max(axis=1).sum())


def trip_model(tmparr, tmpmap, src, nq=200, seed=1):
    locus = tmpmap[:, 0]
    parr, ploc = packed_arrays(src, tmparr, locus)
    nat = pk = 0
    for row in synth.random_quartets(tmparr.shape[0], nq, seed=seed):
        cn, cp = counted_sites(tmparr[row], locus), counted_sites(parr[row], ploc)
        assert np.array_equal(np.sort(src[cp]), cn), "the layouts count different sites"
        nat += trips(cn, tmparr.shape[1])
        pk += trips(cp, len(src))
    return nat / nq, pk / nq


@pytest.mark.parametrize("cfg", ["c1", "c2", "c3", "c4"])
def test_rules_on_benchmark_shapes(cfg):
    T, S, _ = synth.CONFIGS[cfg]
    tmparr, tmpmap = synth.simulate_tmparr(T, S, synth.CONFIG_SEEDS[cfg])
    src = pack_sites(tmpmap)
    steps = check_rules(src, tmpmap[:, 0])
    assert steps <= -(-S // TILE) + 5
    np.testing.assert_array_equal(src, pack_sites(tmpmap[:, 0].copy()))          # 1-D locus column, deterministic


@pytest.mark.parametrize("lens", [[1, 32, 33, 100], [100, 33, 32, 1], [5000], [1], [64], [31, 2, 2100, 7, 32, 32, 65, 1, 1, 1],
                                  [3] * 700 + [40] * 30 + [1] * 500])
def test_rules_on_designed_maps(lens):
    locus = np.repeat(np.arange(len(lens), dtype=np.uint32) * 3 + 7, lens)      # ids with gaps
    src = pack_sites(locus)
    check_rules(src, locus)
    rng = np.random.default_rng(len(lens))
    T = 6
    tmparr = rng.integers(0, 4, size=(T, len(locus)), dtype=np.uint8)
    tmparr[rng.random(tmparr.shape) < 0.5] = 78          # counted sites deep inside the long loci
    src2, pays, est = pack_sites(np.stack([locus, np.arange(len(locus), dtype=np.uint32)], axis=1), tmparr)
    np.testing.assert_array_equal(src, src2)
    assert pays in (True, False) and len(est) == 5
    trip_model(tmparr, locus[:, None], src, nq=15)      # asserts that both layouts count the same sites


def test_locus_runs_must_be_contiguous():
    from tetrad_amd._lib import TetradHipError
    with pytest.raises(TetradHipError):
        pack_sites(np.array([1, 1, 2, 1], np.uint32))
    with pytest.raises(TetradHipError):
        pack_sites(np.array([1, 0xFFFFFFFF], np.uint32))


@pytest.mark.parametrize("cfg,extra_steps", [("c3", 2), ("c4", 5)])
def test_trip_model(cfg, extra_steps):
    T, S, _ = synth.CONFIGS[cfg]
    tmparr, tmpmap = synth.simulate_tmparr(T, S, synth.CONFIG_SEEDS[cfg])
    src, pays, est = pack_sites(tmpmap, tmparr)
    steps = check_rules(src, tmpmap[:, 0])
    nat, pk = trip_model(tmparr, tmpmap, src)
    print(f"{cfg}: steps {-(-S // TILE)} -> {steps}, trips per quartet {nat:.1f} -> {pk:.1f} ({pk / nat:.3f}); "
          f"library estimate {est[2]:.1f} -> {est[3]:.1f}, instructions {est[0]:.0f} -> {est[1]:.0f}")
    assert pk <= 0.80 * nat
    assert steps <= -(-S // TILE) + extra_steps
    # the library's own estimate (24 quartets of its own) agrees with the 200-quartet model to a few per cent
    assert abs(est[2] - nat) <= 0.03 * nat and abs(est[3] - pk) <= 0.03 * pk


def test_automatic_rule():
    T, S, _ = synth.CONFIGS["c3"]
    tmparr, tmpmap = synth.simulate_tmparr(T, S, synth.CONFIG_SEEDS["c3"])
    _, pays, est = pack_sites(tmpmap, tmparr)
    print("c3 estimate", est)
    assert pays and est[1] < est[0] and est[4] >= 0.03
    tmparr, tmpmap = synth.radseq_profile("rad60")
    _, pays, est = pack_sites(tmpmap, tmparr)
    print("rad60 estimate", est)
    assert not pays and est[4] < 0.03

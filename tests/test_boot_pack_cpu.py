"""CPU: what option ``boot_pack`` is expected to buy -- the packed site order (csrc/pack.hpp, through tq_pack_sites) on
bootstrap replicates of the c5 source.  No device: a replicate is taken here as its locus runs only (the spans of the drawn
loci one after the other, locus id = ordinal of the draw, bases recoded with a two-base IUPAC code taken as present; the
shuffle inside a locus and the ambiguity coin move single counted sites, not the statistics).

A replicate draws the source's loci with replacement, so its locus lengths and its missing-data pattern are the source's:
the packer keeps the natural number of 2048-site steps and the modelled walk trips (test_site_packing_cpu.trip_model: per
step the largest number of counted sites in one of the 64 lane words) fall as they do on the original matrix.  Bound: the
mean ratio packed / natural over 4 replicates x 60 quartets stays below 0.85 (a locus-level restatement of the planner gave
0.778-0.805 per replicate; a 60-quartet mean scatters by about +-0.015).  Figures: profiles/boot_pack/README.md."""
import numpy as np
import pytest

from tetrad_amd import synth
from tetrad_amd.engine import pack_sites
from test_site_packing_cpu import TILE, check_rules, trip_model

CODE = np.full(256, 78, np.uint8)
CODE[[65, 67, 71, 84]] = [0, 1, 2, 3]
CODE[[82, 75, 83, 89, 87, 77]] = [0, 3, 1, 1, 0, 0]          # R K S Y W M: present (their first base)


def host_replicate(seqarr, spans, lidxs):
    """(tmparr, tmpmap) of the replicate that draws `lidxs`, columns unshuffled."""
    widths = spans[lidxs, 1] - spans[lidxs, 0]
    start = np.repeat(spans[lidxs, 0], widths)
    first = np.repeat(np.cumsum(widths) - widths, widths)
    cols = start + np.arange(int(widths.sum())) - first
    locus = np.repeat(np.arange(len(lidxs), dtype=np.uint32), widths)
    return CODE[seqarr[:, cols]], np.stack([locus, np.arange(len(cols), dtype=np.uint32)], axis=1)


@pytest.fixture(scope="module")
def c5_source():
    seqarr, _, spans = synth.make_c5_source()
    return seqarr, spans


def test_replicates_of_the_c5_source_keep_their_steps_and_lose_trips(c5_source):
    seqarr, spans = c5_source
    rng = np.random.default_rng(2024)
    nat_sum = pk_sum = 0.0
    for rep in range(4):
        lidxs = rng.integers(0, len(spans), size=len(spans))
        tmparr, tmpmap = host_replicate(seqarr, spans, lidxs)
        S = tmparr.shape[1]
        src = pack_sites(tmpmap)
        steps = check_rules(src, tmpmap[:, 0])
        nat, pk = trip_model(tmparr, tmpmap, src, nq=60, seed=rep)
        print(f"replicate {rep}: {S} sites, steps {-(-S // TILE)} -> {steps}, trips per quartet {nat:.1f} -> {pk:.1f} "
              f"({pk / nat:.3f})")
        assert steps == -(-S // TILE)
        nat_sum += nat
        pk_sum += pk
    print(f"4 replicates: trips per quartet {nat_sum / 4:.1f} -> {pk_sum / 4:.1f} ({pk_sum / nat_sum:.3f})")
    assert pk_sum < 0.85 * nat_sum


def test_repeated_draws_are_runs_of_their_own():
    """Two consecutive draws of the same locus are two runs: each is placed as a whole, and neither is merged."""
    spans = np.array([[0, 20], [20, 37]], np.int64)
    seqarr = np.full((4, 37), 65, np.uint8)
    lidxs = np.array([1, 1, 0, 1, 1], np.int64)
    _, tmpmap = host_replicate(seqarr, spans, lidxs)
    src = pack_sites(tmpmap)
    check_rules(src, tmpmap[:, 0])
    # 17 + 17 does not fit a 32-site word, 20 + 17 neither: five words, one locus each
    words = src[:5 * 32].reshape(5, 32)
    assert sorted((words != 0xFFFFFFFF).sum(axis=1).tolist()) == [17, 17, 17, 17, 20]

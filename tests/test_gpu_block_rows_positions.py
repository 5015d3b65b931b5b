"""GPU: the range test of the block-row kernels (`tq_block_rows_kernel<Rule>`, `tq_quintet_blocks_kernel`) at every
position of a set.  The device forms do not check rows, and the
other device-form tests put an id out of range in the last position only.  Here, for each of the four kinds, every
position in turn holds the bound itself (T, or K under the identity species map) and 0xFFFFFFFF: those rows come back all
zero, the valid rows beside them equal the model of the kind's own test file bit for bit, and a canary row behind the
output is untouched.  The quartet kind runs once more with count_invariant = 1 for slot 0."""
from itertools import combinations

import numpy as np
import pytest

from conftest import load_golden
import blocks_model as bm
import quintets_model as qm
import species_blocks_model as sbm
import species_quintets_model as sqm
from species_model import species_counts

pytestmark = pytest.mark.gpu

GOLDEN, T, STARTS = "edge_T7_S130", 7, np.array([0, 50, 130], np.int64)
KINDS = {   # width, species, the engine's device form
    "quartets": (4, False, "patterns_blocks_dev"),
    "species": (4, True, "patterns_blocks_species_dev"),
    "quintets": (5, False, "patterns_quintet_blocks_dev"),
    "species_quintets": (5, True, "patterns_quintet_blocks_species_dev"),
}


@pytest.fixture(scope="module")
def engine():
    from tetrad_amd.engine import QuartetEngine
    g = load_golden(GOLDEN)
    assert g["tmparr"].shape == (T, 130)
    with QuartetEngine(0) as eng:
        eng.set_data(g["tmparr"], g["tmpmap"])
        eng.set_species(np.arange(T, dtype=np.int32), T)
        yield eng


def rows_of(width):
    """(sets u32[6 + 2 width][width], valid mask): six valid sets, then per position p a row with the bound at p and a row
    with 0xFFFFFFFF at p, on two different valid sets, interleaved with the valid ones.  Taxon 3 of the golden is missing
    at every site: the valid sets leave it out, so that none of their rows is empty."""
    valid = np.array(list(combinations((0, 1, 2, 4, 5, 6), width)), np.uint32)
    valid = valid[np.linspace(0, len(valid) - 1, 6).astype(int)]
    rows, ok = [], []
    for p in range(width):
        for base, bad in ((valid[p % 6], T), (valid[(p + 3) % 6], 0xFFFFFFFF)):
            row = base.copy()
            row[p] = bad
            rows.append(row)
            ok.append(False)
        rows.append(valid[p])
        ok.append(True)
    for v in valid[width:]:
        rows.append(v)
        ok.append(True)
    return np.array(rows, np.uint32), np.array(ok)


_MODEL = {}


def model(kind, sets, inv=0):
    """The model rows of the valid sets, by the model of the kind's own test file; computed once."""
    key = (kind, inv)
    if key not in _MODEL:
        tmparr = load_golden(GOLDEN)["tmparr"]
        cnt = species_counts(tmparr, np.arange(T, dtype=np.int32), T)
        _MODEL[key] = {"quartets": lambda: bm.block_rows(tmparr, sets, STARTS, inv),
                       "species": lambda: sbm.factored_rows(cnt, sets, STARTS),
                       "quintets": lambda: qm.block_rows(tmparr, sets, STARTS),
                       "species_quintets": lambda: sqm.factored_rows(cnt, sets, STARTS)}[kind]()
        _MODEL[key].setflags(write=False)
    return _MODEL[key]


def device_rows(engine, kind, sets):
    """The device form on canary-filled output with one row to spare: (rows u32[Q][2][16], the spare rows)."""
    import torch
    Q = len(sets)
    d_sets = torch.from_numpy(sets.view(np.int32).reshape(-1)).cuda()
    d_out = torch.full((Q * 2 + 1, 16), -1, dtype=torch.int32, device="cuda")
    getattr(engine, KINDS[kind][2])(d_sets.data_ptr(), Q, STARTS, d_out.data_ptr(), torch.cuda.current_stream().cuda_stream)
    out = d_out.cpu().numpy().view(np.uint32)
    return out[:Q * 2].reshape(Q, 2, 16), out[Q * 2:]


@pytest.mark.parametrize("kind", list(KINDS))
def test_a_bad_id_at_every_position(engine, kind):
    width = KINDS[kind][0]
    sets, ok = rows_of(width)
    assert len(sets) == 6 + 2 * width and ok.sum() == 6
    for p in range(width):                                               # every position holds each bad id once
        assert sorted(sets[~ok][:, p][sets[~ok][:, p] >= T].tolist()) == [T, 0xFFFFFFFF]
    want = model(kind, sets[ok])
    assert want[:, :, 0 if width == 5 else 15].all()                     # no valid row is empty
    rows, spare = device_rows(engine, kind, sets)
    assert not rows[~ok].any()
    assert np.array_equal(rows[ok], want)
    assert (spare == 0xFFFFFFFF).all()


def test_quartet_slot_0_with_invariant_sites(engine):
    sets, ok = rows_of(4)
    want = model("quartets", sets[ok], 1)
    assert want[:, :, 0].any() and not model("quartets", sets[ok], 0)[:, :, 0].any()
    engine.set_option("count_invariant", 1)
    try:
        rows, spare = device_rows(engine, "quartets", sets)
    finally:
        engine.set_option("count_invariant", 0)
    assert np.array_equal(rows[ok][:, :, 0], want[:, :, 0]) and rows[ok][:, :, 0].any()
    assert np.array_equal(rows[ok], want) and not rows[~ok].any() and (spare == 0xFFFFFFFF).all()

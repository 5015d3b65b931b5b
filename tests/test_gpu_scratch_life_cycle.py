"""GPU: the life cycle of the grow-only device buffers that the layout and packing life-cycle tests do not walk -- the
host-API scratch, the count slab with its ordering scratch, the singular-value scratch, the species table and the
block-boundary array.

One engine ``E`` goes through every step; after each step its rows are compared BITWISE (rstat, rscor, flags, and the
count matrices of the debug call) with those of a fresh engine that was given only that step's data and options.  A
buffer that was regrown wrongly, kept a stale capacity, or is read at an offset of its old size shows as a difference:

1. 64 quartets, both modes;
2. all 495 quartets: the count slab, the ordering scratch and the result scratch grow;
3. 64 again: a short batch inside the long allocations;
4. ``svd_chunk`` 64, then 256, on the 495: chunks shorter than the singular-value scratch, and a scratch that grows;
5. a species map and the 15 species quartets;
6. a longer matrix (S = 4 * TILE + 1): the species table grows;
7. the short matrix again: a short table inside the long allocation;
8. block rows (B = 3) of 20 sets before and after a ``set_data`` of another length."""
import numpy as np
import pytest

from test_gpu_bootstrap_layout import TILE

pytestmark = pytest.mark.gpu

T = 12
SPECIES_OF = np.arange(T) // 2


def rows(eng, quartets, species=False):
    """Every array a resolve hands out: the plain call and the debug call (count matrices), both modes (species: full)."""
    out = []
    for sub in ((False,) if species else (True, False)):
        call = (lambda debug: eng.resolve_species(quartets, debug=debug)) if species else \
               (lambda debug: eng.resolve(quartets, sub, debug=debug))
        rstat, rscor, flags = call(False)
        d_rstat, d_rscor, d_flags, dbg = call(True)
        out += [(f"sub={sub} {name}", np.array(a)) for name, a in
                (("rstat", rstat), ("rscor", rscor), ("flags", flags), ("debug rstat", d_rstat), ("debug rscor", d_rscor),
                 ("debug flags", d_flags), ("cmats", dbg["cmats"]))]
    return out


def assert_bitwise(got, want, step):
    assert len(got) == len(want)
    for (name, a), (_, b) in zip(got, want):
        assert a.dtype == b.dtype and a.shape == b.shape, f"{step}: {name}"
        np.testing.assert_array_equal(a.view(np.uint8), b.view(np.uint8), err_msg=f"{step}: {name}")


def fresh_rows(data, quartets, step, options=(), species=False):
    """The rows of a new engine that sees only this step's data and options (one resolve per entry of `options`)."""
    from tetrad_amd.engine import QuartetEngine
    out = []
    with QuartetEngine(0) as F:
        F.set_data(*data)
        if species:
            F.set_species(SPECIES_OF, 6)
        for opt in options or (None,):
            if opt:
                F.set_option(*opt)
            out.append(rows(F, quartets, species))
    return out


def test_grow_only_buffers_through_their_life_cycle():
    from tetrad_amd import synth
    from tetrad_amd.engine import QuartetEngine
    short = synth.simulate_tmparr(T, 2 * TILE + 5, seed=71, missing=0.15)
    long_ = synth.simulate_tmparr(T, 4 * TILE + 1, seed=72, missing=0.15)
    allq = synth.all_quartets(T)
    assert len(allq) == 495
    few = np.ascontiguousarray(allq[100:164])
    squartets = synth.all_quartets(6)
    assert len(squartets) == 15
    with QuartetEngine(0) as E:
        E.set_data(*short)
        for step, q in (("1: 64 quartets", few), ("2: 495 quartets", allq), ("3: 64 after 495", few)):
            assert_bitwise(rows(E, q), fresh_rows(short, q, step)[0], step)

        chunks = (("svd_chunk", 64), ("svd_chunk", 256))
        want = fresh_rows(short, allq, "4", options=chunks)
        for opt, w in zip(chunks, want):
            E.set_option(*opt)
            assert_bitwise(rows(E, allq), w, f"4: svd_chunk {opt[1]}")
        E.set_option("svd_chunk", 0)                                # the default again

        E.set_species(SPECIES_OF, 6)
        for step, data, reload in (("5: species", short, False), ("6: species, longer matrix", long_, True),
                                   ("7: species, short matrix again", short, True)):
            if reload:
                E.set_data(*data)
            assert_bitwise(rows(E, squartets, species=True), fresh_rows(data, squartets, step, species=True)[0], step)

        sets = allq[:20]
        for step, data, reload in (("8: block rows before set_data", short, False), ("8: block rows after set_data", long_, True)):
            S = data[0].shape[1]
            starts = [3, TILE - 1, S - TILE + 7, S]
            if reload:
                E.set_data(*data)
            got = E.patterns_blocks(sets, starts)
            with QuartetEngine(0) as F:
                F.set_data(*data)
                want_rows = F.patterns_blocks(sets, starts)
            assert got.shape == (20, 3, 16)
            np.testing.assert_array_equal(got, want_rows, err_msg=step)
            assert got[:, :, 15].sum() > 0, step

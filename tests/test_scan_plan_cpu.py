"""CPU-only: `choose_scan` (csrc/scan_plan.hpp, through tq_scan_plan) names, field by field, the launch that the
dispatch code it replaced made (tests/scan_plan_model.py), over the whole option lattice and over the shape limits;
every plan has a kernel in the library's table, and the lattice reaches every kernel of the table and every form."""
from itertools import product

import numpy as np
import pytest

import scan_plan_model as M
from tetrad_amd import _lib
from tetrad_amd.engine import scan_plan

LIMIT = 0xFFFF0000
ORDINARY = dict(T=128, pitch=51200, Sp=51200)


def rows_of(knob_dicts_and_shapes):
    return np.array([[k[f] for f in M.KNOB_FIELDS] + [s[f] for f in M.SHAPE_FIELDS] for k, s in knob_dicts_and_shapes],
                    dtype=np.int64)


def option_lattice():
    """Full product of every option that the choice reads and both modes, at the batch sizes either side of each
    threshold (64, wg_min_quartets 4096, dp_min_quartets = the sort threshold 32768) and at one ordinary size.  No value
    of the issue's axes is dropped."""
    shapes = {(Q, sub, insorted): dict(ORDINARY, Q=Q, subsample=sub, input_sorted=insorted)
              for Q in (63, 64, 4095, 4096, 32767, 32768, 100_000) for sub in (0, 1) for insorted in (0, 1)}
    out = []
    for pair, wg, method, f4, dp, park, shc, inv, wpc, order in product(
            (0, 1), (1, 2, 3, 4, 6, 8, 16), range(-1, 7), (-1, 0, 1), (0, 1), (0, 1), (0, 1), (0, 1), (0, 2), (0, 1)):
        k = dict(M.DEFAULT_KNOBS, scan_pair=pair, scan_wg=wg, scan_method=method, scan_f4=f4, scan_dp=dp, park_t=park,
                 share_c=shc, count_invariant=inv, waves_per_cu=wpc, order=order)
        # sortedness: `order` holds, the quartets arrive sorted, or neither (both at once adds no clause)
        out += [(k, s) for (Q, sub, insorted), s in shapes.items() if not (order and insorted)]
    return out


#: option sets that between them reach every form (and the one-wave form through count_invariant and scan_wg 1)
REDUCED = [{}, {"scan_f4": 0}, {"scan_f4": 1}, {"scan_pair": 1}, {"scan_method": 6}, {"scan_method": 6, "scan_wg": 8},
           {"scan_wg": 8}, {"scan_wg": 2, "scan_f4": 0}, {"scan_wg": 3}, {"scan_wg": 6, "scan_method": 1}, {"scan_wg": 16},
           {"scan_wg": 1}, {"scan_wg": 1, "scan_method": 0}, {"scan_wg": 1, "scan_method": 1}, {"count_invariant": 1}, {"share_c": 1}, {"scan_wg": 4, "waves_per_cu": 2, "scan_f4": 0},
           {"scan_wg": 16, "waves_per_cu": 2}, {"scan_dp": 0, "scan_f4": 0}, {"order": 0}]

SHAPES = [
    ORDINARY,
    dict(T=128, pitch=49152, Sp=51200),                         # a packed set, shorter than the natural one
    dict(T=1, pitch=LIMIT - 1, Sp=LIMIT - 1),                   # T * pitch one below the 32-bit offset limit
    dict(T=1, pitch=LIMIT, Sp=LIMIT),                           # and at it
    dict(T=65535, pitch=63488, Sp=63488),                       # the same with many taxa: one step below the limit
    dict(T=65535, pitch=65536, Sp=65536),                       # = 0xFFFF0000
    dict(T=1, pitch=2048, Sp=LIMIT),                            # only the natural set is out of range
    dict(T=1, pitch=LIMIT, Sp=2048),                            # only the set the scan reads
    dict(T=16, pitch=1023 * 2048, Sp=1023 * 2048),              # pitch / TILE at PB_MAX_TILES
    dict(T=16, pitch=1024 * 2048, Sp=1024 * 2048),              # and past it
    dict(T=1625, pitch=4096, Sp=4096),                          # T^3 = 4 291 015 625 <= 2^32 - 1
    dict(T=1626, pitch=4096, Sp=4096),                          # T^3 = 4 298 942 376
    dict(T=1 << 22, pitch=1, Sp=1),                             # T^3 = 2^66 wraps to 0 in the 64-bit product
]


def limit_lattice():
    """The reduced option sets x batch sizes (1, 2, block counts 63 / 64 for every workgroup size, the thresholds) x
    pb_ok x nrep x xcd_remap x the shape limits x default and non-default wg_min_quartets / dp_min_quartets."""
    sizes = {1, 2, 4096, 32768, 100_000}
    for qpw in (2, 3, 4, 6, 8, 16):                             # quartets per workgroup: nblk = 63, 64, 64
        sizes |= {63 * qpw, 63 * qpw + 1, 64 * qpw}
    shapes = [dict(shape, Q=Q, subsample=sub, input_sorted=0) for shape in SHAPES for Q in sorted(sizes) for sub in (0, 1)]
    out = []
    for opts, pb_ok, nrep, remap, (wg_min, dp_min) in product(
            REDUCED, (1, -1), (1, 2, 4, 8, 16, 32), (0, 1), ((4096, 32768), (64, 64), (100, 2))):
        k = dict(M.DEFAULT_KNOBS, pb_ok=pb_ok, nrep=nrep, xcd_remap=remap, wg_min_quartets=wg_min, dp_min_quartets=dp_min)
        k.update(opts)
        out += [(k, s) for s in shapes]
    return out


@pytest.fixture(scope="module")
def lattice():
    """(cases, the library's plans i64[n, 12], the model's plans i64[n, 11], rows of the library's table)."""
    _lib.build()
    cases = option_lattice() + limit_lattice()
    got, want, n_kernels = [], [], 0
    for i in range(0, len(cases), 1 << 16):                     # in pieces: the rows of a million cases are large as lists
        plans, n_kernels = scan_plan(rows_of(cases[i:i + (1 << 16)]))
        got.append(plans)
        want.append(np.array([M.plan(k, s) for k, s in cases[i:i + (1 << 16)]], dtype=np.int64))
    got, want = np.concatenate(got), np.concatenate(want)
    return cases, got, want, n_kernels


def test_library_plan_equals_the_parent_rule(lattice):
    cases, got, want, _ = lattice
    assert got.shape == (len(cases), 12) and want.shape == (len(cases), len(M.PLAN_FIELDS))
    for col, name in enumerate(M.PLAN_FIELDS):
        bad = np.flatnonzero(got[:, col] != want[:, col])
        assert bad.size == 0, (f"{name}: {bad.size} of {len(cases)} rows differ; first: {cases[bad[0]]} "
                               f"library {dict(zip(M.PLAN_FIELDS, got[bad[0]]))} model {M.Plan(*want[bad[0]])._asdict()}")


def test_every_plan_has_a_kernel_and_every_kernel_and_form_is_reached(lattice):
    cases, got, _, n_kernels = lattice
    assert (got[:, 11] >= 0).all(), f"no kernel in the table for {cases[int(np.argmin(got[:, 11]))]}"
    built = M.built_kernels()
    assert n_kernels == len(built) == 83
    assert set(np.unique(got[:, 11]).tolist()) == set(range(n_kernels))
    reached = set(map(tuple, np.unique(got[:, :7], axis=0).tolist()))
    assert reached == built
    assert len(set(map(tuple, np.unique(got[:, [0, 1, 2, 3, 4, 5, 6, 11]], axis=0).tolist()))) == n_kernels     # one row each
    assert set(np.unique(got[:, 0]).tolist()) == set(M.FORM_NAMES)


def test_named_cases():
    """What a reader asks first.  Defaults: F4 in subsample mode, DP in full mode from 32 768 sorted quartets, WG with the
    transposed park below that, one wave below 4096.  scan_wg 6 / park_t 1 / scan_method 3 / full mode: the WG form,
    SUB = true, METHOD = 3, six waves, no PARK_T."""
    def lib(shape, **opts):
        k = dict(M.DEFAULT_KNOBS, **opts)
        s = dict(ORDINARY, input_sorted=0, **shape)
        got = scan_plan(rows_of([(k, s)]))[0][0]
        assert tuple(got[:11]) == tuple(M.plan(k, s))
        return tuple(got[:7])
    assert lib(dict(Q=100_000, subsample=1)) == (M.F4, 1, 0, 4, 0, 0, 0)
    assert lib(dict(Q=100_000, subsample=0)) == (M.DP, 0, 0, 4, 0, 0, 0)
    assert lib(dict(Q=20_000, subsample=0)) == (M.WG, 0, 0, 4, 0, 0, 0)
    assert lib(dict(Q=20_000, subsample=0), scan_method=1) == (M.WG, 0, 1, 4, 0, 1, 0)
    assert lib(dict(Q=4000, subsample=1), nrep=8) == (M.ONE_WAVE, 1, 1, 1, 0, 0, 8)
    assert lib(dict(Q=100_000, subsample=0), scan_wg=6, park_t=1, scan_method=3) == (M.WG, 1, 3, 6, 0, 0, 0)


def test_bad_arguments_are_refused():
    lib = _lib.load()
    assert lib.tq_scan_plan(None, 1, None, None) == -1
    assert lib.tq_scan_plan(None, -1, None, None) == -1
    assert lib.tq_scan_plan(None, 0, None, None) == 0

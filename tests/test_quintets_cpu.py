"""CPU: the five-taxon class rule, the relabelling of A/B patterns with the symmetries of DFOIL, the host execution of the
jackknife on sums of slots against Python floats bit for bit and against the class-index form, and the refusals
(DESIGN.md section 22)."""
import ctypes
from itertools import permutations

import numpy as np
import pytest

import blocks_model as bm
import quintets_model as qm


@pytest.fixture(scope="module")
def quintets():
    from tetrad_amd import _lib, quintets
    _lib.build()
    return quintets


# ---- the class rule ----

def test_class_table_equals_the_model(quintets):
    got, want = quintets.class_table(), qm.class_table()
    assert got.dtype == np.uint8 and got.shape == (1024,)
    assert np.array_equal(got, want)
    assert int((got != 0).sum()) == 4 * 3 * 15 == 180
    assert np.bincount(got, minlength=16)[1:].tolist() == [12] * 15
    from tetrad_amd import _lib
    assert _lib.load().tq_quintet_class_table(None) == -1


# ---- the relabelling ----

TAXA = (2, 5, 7, 11, 13)


def role_orders():
    return np.array(list(permutations(TAXA)), np.int64)


def test_relabelling_equals_the_model_for_all_role_orders(quintets):
    tests = role_orders()
    assert len(tests) == 120
    for stats in (quintets.DFOIL, quintets.PARTITIONED_D):
        sets, set_of, masks = quintets.quintet_tests(tests, stats)
        assert sets.dtype == np.uint32 and sets.tolist() == [list(TAXA)]
        assert set_of.dtype == np.uint32 and not set_of.any()
        assert masks.dtype == np.uint16 and masks.shape == (120, len(stats), 2)
        assert np.array_equal(masks, qm.masks(tests, stats))


def test_the_example_of_the_rule(quintets):
    # roles already ascending: BABAA -> positions {0, 2} -> complement {1, 3, 4} -> k = 13
    assert quintets.pattern_slot("BABAA", (0, 1, 2, 3, 4)) == 13
    assert qm.relabel("BABAA", (0, 1, 2, 3, 4)) == 13
    assert quintets.pattern_slot("ABBAA", (0, 1, 2, 3, 4)) == 3


def popcount(v):
    return bin(int(v)).count("1")


def test_dfoil_sides_are_eight_distinct_slots(quintets):
    _, _, masks = quintets.quintet_tests(role_orders(), quintets.DFOIL)
    for t in range(120):
        for s in range(4):
            left, right = int(masks[t, s, 0]), int(masks[t, s, 1])
            assert popcount(left) == 4 and popcount(right) == 4 and not left & right and not (left | right) & 1


def swapped(tests, i, j):
    out = tests.copy()
    out[:, [i, j]] = out[:, [j, i]]
    return out


def test_dfoil_symmetries(quintets):
    """What the eight patterns of each statistic give when two sister taxa change places (read off the definitions:
    exchange the two letters in every pattern).  P1 <-> P2 maps DFO's left side onto DIL's left side and its right side
    onto DIL's right side, and maps each side of DFI and of DOL onto the other side of the same statistic (D changes
    sign).  P3 <-> P4 does the same with the pairs exchanged: DFI <-> DOL with their sides kept, DFO and DIL negated."""
    DFO, DIL, DFI, DOL = range(4)
    tests = role_orders()
    _, _, m = quintets.quintet_tests(tests, quintets.DFOIL)
    _, _, m12 = quintets.quintet_tests(swapped(tests, 0, 1), quintets.DFOIL)
    _, _, m34 = quintets.quintet_tests(swapped(tests, 2, 3), quintets.DFOIL)
    assert np.array_equal(m12[:, DFO], m[:, DIL]) and np.array_equal(m12[:, DIL], m[:, DFO])
    assert np.array_equal(m12[:, DFI], m[:, DFI, ::-1]) and np.array_equal(m12[:, DOL], m[:, DOL, ::-1])
    assert np.array_equal(m34[:, DFI], m[:, DOL]) and np.array_equal(m34[:, DOL], m[:, DFI])
    assert np.array_equal(m34[:, DFO], m[:, DFO, ::-1]) and np.array_equal(m34[:, DIL], m[:, DIL, ::-1])
    # and the model says the same of the definitions themselves
    assert np.array_equal(m12, qm.masks(swapped(tests, 0, 1), quintets.DFOIL))
    assert np.array_equal(m34, qm.masks(swapped(tests, 2, 3), quintets.DFOIL))


def test_partitioned_d_symmetries(quintets):
    """P1 <-> P2 negates D1, D2 and D12; P3_1 <-> P3_2 exchanges D1 and D2 and keeps D12."""
    tests = role_orders()
    _, _, m = quintets.quintet_tests(tests, quintets.PARTITIONED_D)
    _, _, m12 = quintets.quintet_tests(swapped(tests, 0, 1), quintets.PARTITIONED_D)
    _, _, m34 = quintets.quintet_tests(swapped(tests, 2, 3), quintets.PARTITIONED_D)
    assert np.array_equal(m12, m[:, :, ::-1])
    assert np.array_equal(m34[:, 0], m[:, 1]) and np.array_equal(m34[:, 1], m[:, 0]) and np.array_equal(m34[:, 2], m[:, 2])


def test_quintet_tests_shares_sets_and_refuses_bad_input(quintets):
    tests = np.array([[0, 1, 2, 3, 9], [1, 0, 3, 2, 9], [4, 5, 6, 7, 9], [3, 2, 1, 0, 9]], np.int64)
    sets, set_of, masks = quintets.quintet_tests(tests, quintets.DFOIL)
    assert sets.tolist() == [[0, 1, 2, 3, 9], [4, 5, 6, 7, 9]] and set_of.tolist() == [0, 0, 1, 0]
    sets0, set_of0, masks0 = quintets.quintet_tests(np.zeros((0, 5), np.int64), quintets.DFOIL)
    assert sets0.shape == (0, 5) and set_of0.shape == (0,) and masks0.shape == (0, 4, 2)
    for bad in ([[0, 1, 2, 3]], [[0, 1, 2, 2, 4]], [[0, 1, 2, 3, -1]]):
        with pytest.raises(ValueError):
            quintets.quintet_tests(np.array(bad), quintets.DFOIL)
    for stats in ([(("ABBAB",), ("BABAA",))], [(("AAAAA",), ("BABAA",))], [(("ABBAA",), ("ABBAA",))], [(("ABBA",), ("BABAA",))],
                  [((), ("BABAA",))]):
        with pytest.raises(ValueError):
            quintets.quintet_tests(tests, stats)


# ---- the host jackknife ----

@pytest.mark.parametrize("B", [1, 2, 3, 50, 4096])
@pytest.mark.parametrize("N", [1, 64, 65])
def test_host_equals_python_floats(quintets, N, B):
    rows, set_of, lmask, rmask = qm.jackknife_case(N, B)
    got = quintets.dstat_jackknife_masks(rows, set_of, lmask, rmask)
    want = qm.jackknife_masks_model(rows, set_of, lmask, rmask)
    assert got.shape == (N, 4)
    assert np.array_equal(bm.bits(got), bm.bits(want))
    # the designed tests are what their names say
    nl, nr = popcount(lmask[0]), popcount(rmask[0])
    assert got[0, 0] == B and got[0, 1] == (nl - nr) / (nl + nr)         # 2^32 - 1 in every slot
    if N > 1:
        assert got[1, 1] < 0                                            # left < right everywhere
    if N > 2:
        assert got[2, 0] == 0 and np.isnan(got[2, 1:]).all()            # every block empty
    if N > 3:
        assert got[3, 0] == 1 and np.isfinite(got[3, 1]) and np.isnan(got[3, 2:]).all()      # g = 1


@pytest.mark.parametrize("B", [1, 3, 50])
def test_single_bit_masks_equal_the_class_index_form(quintets, B):
    """The same counts in the slots the masks name: the two instantiations of the rule give the same bits."""
    from tetrad_amd import patterns
    rows, set_of, ia, ib = bm.jackknife_case(65, B)
    shifted = np.zeros_like(rows)
    shifted[:, :, 1:] = rows[:, :, :15]                                 # class c of the quartet rows -> slot c + 1
    lmask = (1 << (ia.astype(np.uint16) + 1)).astype(np.uint16)
    rmask = (1 << (ib.astype(np.uint16) + 1)).astype(np.uint16)
    got = quintets.dstat_jackknife_masks(shifted, set_of, lmask, rmask)
    assert np.array_equal(bm.bits(got), bm.bits(patterns.dstat_jackknife(rows, set_of, ia, ib)))


def test_refusals_leave_out_untouched(quintets):
    from tetrad_amd import _lib
    lib = _lib.load()
    rows, set_of, lmask, rmask = qm.jackknife_case(8, 3)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)

    def call(rows_, n_sets, B, set_of_, lm, rm, N):
        out = np.full((8, 4), -7.0)
        rc = lib.tq_dstat_jackknife_masks(p(rows_), n_sets, B, p(set_of_), p(lm), p(rm), N, p(out))
        return rc, out

    rc, out = call(rows, rows.shape[0], 3, set_of, lmask, rmask, 8)
    assert rc == 0 and not (out == -7.0).any()

    def changed(a, t, v):
        b = a.copy()
        b[t] = v
        return b

    M = rows.shape[0]
    # the full texts, as the library gave them before the checks of the two test forms became one
    rule = b": bit 0 must be clear, both non-empty, and disjoint"
    for args, text in [((rows, M, 3, set_of, changed(lmask, 7, lmask[7] | 1), rmask, 8), b"test 7 has masks 0x8b63 / 0x7098" + rule),
                       ((rows, M, 3, set_of, lmask, changed(rmask, 0, rmask[0] | 1), 8), b"test 0 has masks 0x4f20 / 0x90cf" + rule),
                       ((rows, M, 3, set_of, changed(lmask, 3, 0), rmask, 8), b"test 3 has masks 0x0000 / 0xa4e0" + rule),
                       ((rows, M, 3, set_of, lmask, changed(rmask, 4, 0), 8), b"test 4 has masks 0x4720 / 0x0000" + rule),
                       ((rows, M, 3, set_of, changed(lmask, 2, lmask[2] | rmask[2]), rmask, 8),
                        b"test 2 has masks 0x7bfa / 0x3910" + rule),
                       ((rows, M, 3, changed(set_of, 5, M), lmask, rmask, 8), b"test 5 has set_of=4 >= n_sets=4"),
                       ((rows, M, 0, set_of, lmask, rmask, 8), b"B=0 blocks, must be 1..4096"),
                       ((rows, M, 4097, set_of, lmask, rmask, 8), b"B=4097 blocks, must be 1..4096"),
                       ((rows, -1, 3, set_of, lmask, rmask, 8), b"NULL pointer or negative size"),
                       ((rows, M, 3, set_of, lmask, rmask, -1), b"NULL pointer or negative size")]:
        rc, out = call(*args)
        assert rc == -1 and (out == -7.0).all(), text
        assert lib.tq_last_error(None) == b"tq_dstat_jackknife_masks: " + text
    out = np.full((8, 4), -7.0)
    assert lib.tq_dstat_jackknife_masks(None, M, 3, p(set_of), p(lmask), p(rmask), 8, p(out)) == -1 and (out == -7.0).all()
    assert lib.tq_dstat_jackknife_masks(p(rows), M, 3, p(set_of), p(lmask), p(rmask), 8, None) == -1
    assert lib.tq_dstat_jackknife_masks(None, 0, 3, None, None, None, 0, None) == 0      # N = 0 is valid
    with pytest.raises(ValueError):
        quintets.dstat_jackknife_masks(rows[:, :, :15], set_of, lmask, rmask)
    with pytest.raises(ValueError):
        quintets.dstat_jackknife_masks(rows, set_of, lmask[:3], rmask)


def test_result_dtype_names_every_statistic(quintets):
    dt = quintets.result_dtype(quintets.PARTITIONED_D)
    assert dt.names[0] == "nsites" and dt["D12_left"] == np.uint64 and dt["D1_Z"] == np.float64
    assert len(dt.names) == 1 + 3 * 7
    assert quintets.result_dtype([(("ABBAA",), ("BABAA",))]).names[1] == "s0_left"

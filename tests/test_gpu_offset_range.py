"""GPU: the scans at 32-bit row offsets with bit 31 set, on both sides of the host's limit for the cooperative kernels
(T * pitch < 0xFFFF0000) and past 2^32, at the four shapes of tests/offset_shapes.py.  `QuartetEngine.last_scan()` says
which kernel form took a batch, so a case meant for a cooperative kernel fails when the one-wave kernel ran instead.

Every case compares the whole row set with the oracle: count matrices and nsnps exactly, the rest under the bar of
tests/exact_ties.py (flagged rows included); the plain call equals the debug call; all forms of one shape and mode
give bitwise the same rows.  One engine is resident at a time (device memory peaks near 30 GB at T = 3 065 with the
packed set); the tests are ordered by shape so that each shape is uploaded once."""
import time

import numpy as np
import pytest

import offset_shapes as osh
from exact_ties import check_rows

pytestmark = pytest.mark.gpu

TWO31 = 2147483648
LIMIT = 0xFFFF0000            # written out: the bound the host applies before it selects a cooperative kernel
TWO32 = 4294967296

DEFAULTS = {"park_t": 1, "scan_pair": 0, "share_c": 0, "scan_wg": 0, "scan_method": -1, "scan_dp": 1, "scan_f4": -1,
            "dp_min_quartets": 0}
# option sets of test_scan_kernel_variants_agree_on_sorted_batches -> the cooperative form they ask for in
# (subsample, full) mode.  By default subsample mode streams plane records (f4) and full mode runs the nibble-code
# kernel (wg); f4 needs the transposed park and has no form that shares row c; scan_wg = 8 keeps the mode's kernel
# with 8 waves; the joint histogram (dp) is a full-mode kernel
OPTION_SETS = {
    "default": ({}, "f4", "wg"),
    "scan_f4=0": ({"scan_f4": 0}, "wg", "wg"),
    "scan_f4=1": ({"scan_f4": 1}, "f4", "f4"),
    "scan_pair=1": ({"scan_pair": 1}, "wg2", "wg2"),
    "scan_method=6": ({"scan_method": 6}, "pb", "pb"),
    "scan_wg=8": ({"scan_wg": 8}, "f4", "wg"),
    "share_c=1": ({"share_c": 1}, "wg", "wg"),
    "park_t=0": ({"park_t": 0}, "wg", "wg"),
    "scan_dp=1": ({"scan_dp": 1, "dp_min_quartets": 2}, None, "dp"),
}
CASES = [(mode, name) for mode in ("sub", "full") for name, (_, s, f) in OPTION_SETS.items()
         if (s if mode == "sub" else f) is not None]
CASES_NO_DP = [c for c in CASES if c[1] != "scan_dp=1"]
PACKED_SHAPES = (1600, 3065)      # uploaded with site_pack = 1; site_pack = 0 afterwards reads the natural set again


class Resident:
    """The host matrix and the one engine that is resident: asking for another shape closes it first."""

    def __init__(self):
        t0 = time.perf_counter()
        self.matrix = osh.build_matrix()
        self.tmpmap = osh.simulated()[2]
        print(f"\n[offset_range] host matrix {self.matrix.shape} built in {time.perf_counter() - t0:.1f} s")
        self.T = None
        self.eng = None
        self.base = {}

    def engine(self, T):
        from tetrad_amd.engine import QuartetEngine
        if self.T != T:
            self.close()
            self.eng = QuartetEngine(0)
            self.T = T
            self.eng.set_option("wg_min_quartets", 64)
            self.eng.set_option("site_pack", 1 if T in PACKED_SHAPES else 0)
            t0 = time.perf_counter()
            self.eng.set_data(self.matrix[:T], self.tmpmap)
            print(f"\n[offset_range] set_data T={T} site_pack={int(T in PACKED_SHAPES)}: {time.perf_counter() - t0:.1f} s")
        return self.eng

    def close(self):
        if self.eng is not None:
            self.eng.close()
        self.eng, self.T = None, None

    def run(self, T, mode, opts, site_pack=0):
        """Rows of the shape's quartets under `opts` (restored afterwards), checked against the oracle and the debug
        call: ((rstat, rscor, flags), last_scan())."""
        eng = self.engine(T)
        sub = mode == "sub"
        q = osh.quartets(T)[0]
        eng.set_option("site_pack", site_pack)
        for k, v in opts.items():
            eng.set_option(k, v)
        try:
            plain = eng.resolve(q, sub)
            scan = eng.last_scan()
            rstat, rscor, flags, dbg = eng.resolve(q, sub, debug=True)
            assert eng.last_scan() == scan
        finally:
            for k in opts:
                eng.set_option(k, DEFAULTS[k])
        what = f"T={T} {mode} {opts} site_pack={site_pack} {scan}"
        for a, b in zip(plain, (rstat, rscor, flags)):
            np.testing.assert_array_equal(a, b, err_msg=f"plain call != debug call: {what}")
        o_rstat, o_rscor, o, exact = osh.expected(T, sub)
        assert len(rstat) == len(q) == len(o_rstat)                     # no row is skipped
        np.testing.assert_array_equal(dbg["cmats"], o["cmats"], err_msg=f"count matrices: {what}")
        np.testing.assert_array_equal(rstat[:, 1], o_rstat[:, 1], err_msg=f"nsnps: {what}")
        check_rows((rstat, rscor, flags), dbg, (o_rstat, o_rscor, o), exact=exact)
        return tuple(np.array(a) for a in plain), scan

    def same_as_base(self, T, mode, rows, what):
        """Bitwise the rows of the default options on the natural set."""
        if (T, mode) not in self.base:
            self.base[T, mode] = self.run(T, mode, {})[0]
        for a, b, name in zip(self.base[T, mode], rows, ("rstat", "rscor", "flags")):
            np.testing.assert_array_equal(a, b, err_msg=f"{name} differs from the default form: {what}")


@pytest.fixture(scope="module")
def resident(oracle):
    r = Resident()
    hot, decoy, _ = osh.simulated()
    assert np.array_equal(r.matrix[list(osh.ALL_HOT)], hot)
    for row in (2, 1531, 1535, 1595, 3060):
        assert np.array_equal(r.matrix[row], decoy)
    yield r
    r.close()


def form_asked(mode, name):
    _, s, f = OPTION_SETS[name]
    return s if mode == "sub" else f


# ---- T = 1600: bit 31 set, inside the limit ---------------------------------------------------------------------------

@pytest.mark.parametrize("mode,name", CASES)
def test_cooperative_forms_with_bit_31_set(resident, mode, name):
    """T * Sp = 2 241 331 200: rows 1533 and up start past 2^31 (1533 straddles it); they occur as shared rows a, b and
    as own rows c, d, and in the permuted half of the batch most wavefronts read a, b at their own byte-row offsets."""
    rows, (form, t_pitch, packed) = resident.run(1600, mode, OPTION_SETS[name][0])
    assert (form, t_pitch, packed) == (form_asked(mode, name), 2_241_331_200, False)
    assert TWO31 < t_pitch < LIMIT
    resident.same_as_base(1600, mode, rows, f"{mode} {name}")


@pytest.mark.parametrize("name", ["default", "scan_f4=0"])
def test_packed_set_with_bit_31_set(resident, name):
    """site_pack = 1, subsample mode, the plane-record and the nibble-code form: the packed set's own pitch (about 1.07
    times the natural one) puts bit 31 into other rows' offsets; the same rows, bit for bit."""
    rows, (form, t_pitch, packed) = resident.run(1600, "sub", OPTION_SETS[name][0], site_pack=1)
    assert form == form_asked("sub", name) and packed
    assert t_pitch == 1600 * resident.eng.site_pack_state()[0] and TWO31 < t_pitch < LIMIT and t_pitch > 2_241_331_200
    resident.same_as_base(1600, "sub", rows, f"packed {name}")


def test_export_returns_the_input_at_1600(resident):
    """tq_export_kernel indexes up to T * S = 2.24e9."""
    eng = resident.engine(1600)
    arr, tmap = eng.get_data()
    assert arr.shape == (1600, osh.S)
    assert np.array_equal(arr, resident.matrix[:1600])
    assert np.array_equal(tmap, resident.tmpmap)


def test_species_table_reads_high_rows_at_1600(resident):
    """tq_species_table_kernel's members[m] * (Sp / 2) at rows past 1532: pooled count matrices of both forms against
    the factored model on the member rows.  No species has more than 6 samples (here 3), so 6^4 * S < 2^32."""
    from species_model import pooled_factored
    species = [(0, 1, 1532), (1533, 1534, 1596), (1597, 1598), (1599, 2), (3, 1535), (1000,)]
    K = len(species)
    assert max(len(s) for s in species) <= 6 and 6 ** 4 * osh.S < TWO32
    sp = np.full(1600, -1, np.int32)
    for k, mem in enumerate(species):
        sp[list(mem)] = k
    used = np.flatnonzero(sp >= 0)
    squartets = np.array([(0, 1, 2, 3), (1, 0, 3, 2), (0, 1, 2, 4), (1, 2, 3, 5), (0, 2, 4, 5), (3, 1, 4, 0)], np.uint32)
    want = pooled_factored(resident.matrix[used], sp[used], K, squartets)
    eng = resident.engine(1600)
    eng.set_species(sp, K)
    try:
        for method in (0, 1):
            eng.set_option("species_method", method)
            _, _, _, dbg = eng.resolve_species(squartets, debug=True)
            np.testing.assert_array_equal(dbg["cmats"], want, err_msg=f"species_method={method}")
    finally:
        eng.set_option("species_method", -1)


# ---- T = 3065: just inside the limit ------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode,name", CASES_NO_DP)
def test_cooperative_forms_just_inside_the_limit(resident, mode, name):
    """T * Sp = 4 293 550 080 = 0xFFFF0000 - 1 351 680: the last rows' offsets come within 1.4 MB of the bound."""
    rows, (form, t_pitch, packed) = resident.run(3065, mode, OPTION_SETS[name][0])
    assert (form, t_pitch, packed) == (form_asked(mode, name), 4_293_550_080, False)
    assert LIMIT - t_pitch == 1_351_680
    resident.same_as_base(3065, mode, rows, f"{mode} {name}")


@pytest.mark.parametrize("mode", ["sub", "full"])
def test_forced_packed_set_past_the_limit(resident, mode):
    """site_pack = 1 bypasses the rule that drops a packed set whose pitch is past the limit while the natural one is
    inside: the subsample scan must take the long pitch to the one-wave kernel; full mode reads the natural set."""
    rows, (form, t_pitch, packed) = resident.run(3065, mode, {}, site_pack=1)
    if mode == "sub":
        assert form == "one_wave" and packed
        assert t_pitch == 3065 * resident.eng.site_pack_state()[0] and t_pitch >= LIMIT
    else:
        assert (form, t_pitch, packed) == ("wg", 4_293_550_080, False)
    resident.same_as_base(3065, mode, rows, f"forced pack {mode}")


# ---- T = 3066 and 3067: the band below 2^32 and beyond ----------------------------------------------------------------

@pytest.mark.parametrize("mode,name", CASES)
@pytest.mark.parametrize("T", [3066, 3067])
def test_past_the_limit_every_option_set_takes_the_one_wave_kernel(resident, T, mode, name):
    """T = 3066: 0xFFFF0000 <= T * Sp < 2^32, where a cooperative kernel's u32 offsets would still not wrap and only the
    host comparison keeps it out; T = 3067: past 2^32."""
    rows, (form, t_pitch, packed) = resident.run(T, mode, OPTION_SETS[name][0])
    assert (form, t_pitch, packed) == ("one_wave", T * 1_400_832, False)
    assert (LIMIT <= t_pitch < TWO32) if T == 3066 else t_pitch >= TWO32
    resident.same_as_base(T, mode, rows, f"T={T} {mode} {name}")

"""GPU: `tq_set_option` name by name -- the legal range of every option, the value just outside each end with its code and
full message, the listed values of `nrep` and `scan_wg`, the flags, the clamp of `batch`, an unknown name, `bdsqr_stats`
on and off, and what "0 = default" gives where it shows without data (the chunk sizes of two accumulators).  One
context, no data."""
import pytest

from tetrad_amd._lib import TetradHipError

pytestmark = pytest.mark.gpu

I64_MAX = 2**63 - 1

#: name, lowest legal value, highest legal value (None: the largest int64), the message of a value outside them
RANGES = [
    ("waves_per_cu", 0, 2**20, "waves_per_cu must be 0..2^20"),
    ("scan_f4", -1, 1, "scan_f4 must be -1 (subsample mode only), 0 or 1"),
    ("site_pack", -1, 1, "site_pack must be -1 (automatic), 0 or 1"),
    ("boot_pack", -1, 1, "boot_pack must be -1 (automatic), 0 or 1"),
    ("scan_dp", 0, 1, "scan_dp must be 0 or 1"),
    ("dp_min_quartets", 0, None, "dp_min_quartets must be >= 0"),
    ("wg_min_quartets", 0, None, "wg_min_quartets must be >= 0"),
    ("bidiag_layout", -1, 1, "bidiag_layout must be -1 (default), 0 or 1"),
    ("cons_hash_bits", 0, 64, "cons_hash_bits must be 1..64 (0 = default 64)"),
    ("cons_scratch_bytes", 0, None, "cons_scratch_bytes must be >= 0 (0 = default 256 MiB)"),
    ("stree_search_dev", 0, 1, "stree_search_dev must be 0 or 1"),
    ("fit_scratch_bytes", 1, None, "fit_scratch_bytes must be at least 1"),
    ("qdist_scratch_bytes", 0, None, "qdist_scratch_bytes must be >= 0 (0 = default 256 MiB)"),
    ("qdist_kslices", 0, 65535, "qdist_kslices must be 0 (auto) .. 65535"),
    ("stree_lds", 0, 1, "stree_lds must be 0 or 1"),
    ("svd_wpc", 0, 2**20, "svd_wpc must be 0..2^20"),
    ("svd_chunk", 0, None, "svd_chunk must be >= 0"),
    ("svd_streams", 0, 2, "svd_streams must be 0 (default), 1 or 2"),
    ("bdsqr_maxit", 0, 1000, "bdsqr_maxit must be 0..1000"),
    ("svd_method", 0, 1, "svd_method must be 0 (Jacobi) or 1 (HQR)"),
    ("order", 0, 1, "order must be 0 or 1"),
    ("scan_method", -1, 6, "scan_method must be -1 (auto), 0, 1, 6 (or 2..5: timing diagnostics)"),
    ("batch", 0, None, "batch must be >= 0"),
    ("species_method", -1, 1, "species_method must be -1 (auto), 0 (VALU form) or 1 (MFMA form)"),
    ("species_alleles", 0, 1, "species_alleles must be 0 (one lineage per sample) or 1 (two: both alleles)"),
    ("phases", 0, 3, "phases must be 1, 2 or 3"),
]
#: name, the values it takes, the message of any other
LISTED = [
    ("nrep", (0, 1, 2, 4, 8, 16, 32), "nrep must be 1,2,4,8,16 or 32"),
    ("scan_wg", (0, 1, 2, 3, 4, 6, 8, 16), "scan_wg must be 0 (default), 1, 2, 3, 4, 6, 8 or 16"),
]
FLAGS = ["xcd_remap", "count_invariant", "scan_pair", "park_t", "share_c"]

CONS_T, QD_T, QD_TREES = 1025, 8, 4     # shapes at which 256 MiB of scratch, not a cap, decide the chunk


def cons_chunk(engine):
    from tetrad_amd.consensus import Consensus
    with Consensus(CONS_T, engine=engine) as c:
        return c.stats()["chunk_trees"]


def qd_chunk(engine):
    from tetrad_amd.qdist import QuartetDistances
    with QuartetDistances(QD_T, QD_TREES, engine=engine) as q:
        return q.stats()["chunk_words"]


@pytest.fixture(scope="module")
def fresh():
    """The one context, and the chunk sizes it gives before any option has been set."""
    from tetrad_amd.engine import QuartetEngine
    with QuartetEngine(0) as e:
        yield e, cons_chunk(e), qd_chunk(e)


@pytest.fixture
def engine(fresh):
    return fresh[0]


def refused(engine, name, value, message):
    with pytest.raises(TetradHipError) as err:
        engine.set_option(name, value)
    assert err.value.code == -1, (name, value)
    assert str(err.value) == "TQ_ERR_INVALID_ARG: " + message, (name, value)


def test_all_options_are_covered():
    names = [r[0] for r in RANGES] + [r[0] for r in LISTED] + FLAGS + ["bdsqr_stats"]
    assert len(names) == len(set(names)) == 34


@pytest.mark.parametrize("name,lo,hi,message", RANGES, ids=[r[0] for r in RANGES])
def test_range_ends(engine, name, lo, hi, message):
    refused(engine, name, lo - 1, message)
    if hi is not None:
        refused(engine, name, hi + 1, message)
    engine.set_option(name, I64_MAX if hi is None else hi)
    engine.set_option(name, lo)


@pytest.mark.parametrize("name,values,message", LISTED, ids=[r[0] for r in LISTED])
def test_listed_values(engine, name, values, message):
    for v in range(-1, max(values) + 2):
        if v in values:
            engine.set_option(name, v)
        else:
            refused(engine, name, v, message)
    engine.set_option(name, 0)


@pytest.mark.parametrize("name", FLAGS)
def test_flags_take_any_value(engine, name):
    for v in (1, -1, 2, 2**40, -2**63, I64_MAX, 0):
        engine.set_option(name, v)
    engine.set_option(name, 1 if name in ("xcd_remap", "park_t") else 0)


def test_batch_takes_two_to_the_forty(engine):
    engine.set_option("batch", 2**40)
    engine.set_option("batch", 0)


def test_unknown_name(engine):
    refused(engine, "x", 0, "unknown option 'x'")
    refused(engine, "x", 1, "unknown option 'x'")


def test_bdsqr_stats_on_and_off_twice(engine):
    for _ in range(2):
        engine.set_option("bdsqr_stats", 1)
        engine.set_option("bdsqr_stats", 0)


def test_zero_is_the_default_scratch(fresh):
    engine, cons_default, qd_default = fresh
    engine.set_option("cons_scratch_bytes", 1 << 20)
    engine.set_option("qdist_scratch_bytes", 1 << 20)
    assert cons_chunk(engine) < cons_default            # the options are read, and at these shapes they decide
    assert qd_chunk(engine) < qd_default
    engine.set_option("cons_scratch_bytes", 0)
    engine.set_option("qdist_scratch_bytes", 0)
    assert cons_chunk(engine) == cons_default
    assert qd_chunk(engine) == qd_default

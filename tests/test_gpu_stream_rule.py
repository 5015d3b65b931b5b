"""GPU: the stream rule of include/tetrad_hip.h, asserted as an ORDER and not only as data.

"The *_dev entry points of one context share its device scratch; the library orders them in call order whatever their
streams; a host-buffer call waits for every *_dev call made before it", and the accumulators promise the same for their
device adds, builds and scores.  Every case here is one `stream_hold.ordered(...)`: the first call sits on stream A behind
a hold, the second goes to stream B (or is a host-buffer call, or an accumulator read), and the case fails

* when the second call ENDS INSIDE THE HOLD -- it did not wait for the first (no sibling test can see that: a second
  call that runs to completion before the first starts is a legal serial order with right results), and
* when any output differs BITWISE from the same calls made one at a time on a fresh engine -- the second call touched
  shared state before its wait (tq_resolve_range_dev did: it unranked into the shared scratch, then waited).

The entry points that touch only caller memory promise nothing beyond their own stream: their cases assert the opposite,
that they end inside the hold (no device-wide synchronisation crept in).

No case regrows a library buffer under queued work: every engine is first driven once through the calls of its case
(with other inputs behind them, so that stale scratch never equals the expected one), the second call never needs more
than the first, and a replicate is never longer than the one resident before it.

Shapes: T = 16 (1820 ranks), S = 2 * TILE + 5 sites, 15 % missing, 20 sets for the block rows; the 10-taxon, 73-locus
source of test_gpu_bootstrap_layout.py for replicates; 12 trees of 12 taxa for the tree-set accumulators."""
from itertools import combinations

import numpy as np
import pytest

import blocks_model as bm
import patterns_model as pm
import quintets_model as qm
from stream_hold import Streams, assert_bitwise, ordered, runs_while_held, streams      # noqa: F401  (streams: the fixture)
from test_gpu_bootstrap_layout import TILE, layout_source
from test_gpu_staging_rings import five_draws

pytestmark = pytest.mark.gpu

T, S = 16, 2 * TILE + 5
STARTS_A = [3, TILE - 1, S - TILE + 7, S]                 # B = 3
STARTS_B = [1, 40, TILE, TILE + 33, S - 1]                # B = 4
SPECIES_OF_16 = np.arange(T) % 6                          # K = 6: species of 3, 3, 3, 3, 2, 2 samples
SPECIES_OF_10 = np.arange(10) % 5                         # K = 5, two samples each


# ---- inputs, made once ---------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def data():
    from tetrad_amd import synth
    return synth.simulate_tmparr(T, S, seed=81, missing=0.15)


@pytest.fixture(scope="module")
def other_data():
    from tetrad_amd import synth
    return synth.simulate_tmparr(T, S, seed=82, missing=0.15)


@pytest.fixture(scope="module")
def source():
    """(seqarr, spans), and two draws of its loci: the longer replicate first, so that the second needs no larger buffer."""
    src = layout_source(10, seed=12)
    reps = five_draws(src[1], seed=5)
    return src, reps[0], reps[1]


def ranks_to_quartets(lo, hi, ntaxa=T):
    from tetrad_amd import synth
    return np.ascontiguousarray(synth.all_quartets(ntaxa)[lo:hi], dtype=np.uint32)


def sets5(ntaxa, n):
    return np.array(list(combinations(range(ntaxa), 5))[:n], dtype=np.uint32)


# ---- calls: one entry point, inputs and outputs of its own -----------------------------------------------------------

def dev_u32(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).cuda()


class Call:
    """`run(engine, stream_address)` enqueues; `outs` are the device tensors it writes, filled with a sentinel before."""

    def __init__(self, name, run, outs=(), keep=(), sentinel=-1):
        self.name, self.run, self.outs, self.keep, self.sentinel = name, run, list(outs), keep, sentinel

    def fill(self):
        import torch
        for t in self.outs:
            t.fill_(self.sentinel & 255 if t.dtype == torch.uint8 else self.sentinel)

    def rows(self):
        return [t.cpu().numpy() for t in self.outs]


def row_outputs(Q):
    import torch
    return [torch.empty((Q, 2), dtype=torch.int32, device="cuda"), torch.empty((Q, 3), dtype=torch.float64, device="cuda"),
            torch.empty((Q,), dtype=torch.uint8, device="cuda")]


def resolve_call(q, sub):
    d_q, o = dev_u32(q), row_outputs(len(q))
    return Call(f"resolve_dev(Q={len(q)}, sub={sub})",
                lambda e, s: e.resolve_dev(d_q.data_ptr(), len(q), sub, o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), s), o)


def range_call(first, Q, sub):
    o = row_outputs(Q)
    return Call(f"resolve_range_dev([{first}, +{Q}), sub={sub}, d_quartets=0)",
                lambda e, s: e.resolve_range_dev(first, Q, sub, 0, o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), s), o)


def species_call(sq):
    d_q, o = dev_u32(sq), row_outputs(len(sq))
    return Call(f"resolve_species_dev(Q={len(sq)})",
                lambda e, s: e.resolve_species_dev(d_q.data_ptr(), len(sq), o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), s), o)


def scan_call(q, sub):
    d_q = dev_u32(q)
    return Call(f"scan_dev(Q={len(q)}, sub={sub})", lambda e, s: e.scan_dev(d_q.data_ptr(), len(q), sub, s), [], keep=(d_q,))


def svd_call(q0, n):
    o = row_outputs(n)
    return Call(f"svd_dev([{q0}, +{n}))",
                lambda e, s: e.svd_dev(q0, n, o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), s), o)


def patterns_call(sets, sub):
    import torch
    d_s, out = dev_u32(sets), torch.empty((len(sets), 16), dtype=torch.int32, device="cuda")
    return Call(f"patterns_dev(sub={sub})", lambda e, s: e.patterns_dev(d_s.data_ptr(), len(sets), sub, out.data_ptr(), s), [out])


def blocks_call(form, sets, starts):
    """form: the engine method, 'patterns_blocks_dev', 'patterns_quintet_blocks_dev' or one of their species forms."""
    import torch
    d_s, out = dev_u32(sets), torch.empty((len(sets), len(starts) - 1, 16), dtype=torch.int32, device="cuda")
    return Call(f"{form}(B={len(starts) - 1})",
                lambda e, s: getattr(e, form)(d_s.data_ptr(), len(sets), starts, out.data_ptr(), s), [out])


def taxon_call(starts, ntaxa=T):
    import torch
    out = torch.empty((len(starts) - 1, ntaxa, ntaxa, 4), dtype=torch.int32, device="cuda")
    return Call(f"taxon_counts_dev(B={len(starts) - 1})", lambda e, s: e.taxon_counts_dev(starts, out.data_ptr(), s), [out])


def bootstrap_call(rep):
    lidxs, s1, s2 = rep
    return Call("bootstrap(stream)", lambda e, s: e.bootstrap(lidxs, s1, s2, stream=s))


# ---- the two executions of a case -------------------------------------------------------------------------------------

def one_at_a_time(prepare, calls):
    """The reference: a fresh engine, every call alone on one stream, the device idle in between; the rows of each."""
    import torch
    from tetrad_amd.engine import QuartetEngine
    st = torch.cuda.Stream()
    want = []
    with QuartetEngine(0) as F:
        prepare(F)
        for c in calls:
            if isinstance(c, Call):
                c.fill()
                torch.cuda.synchronize()
                c.run(F, st.cuda_stream)
                torch.cuda.synchronize()
                want.append(c.rows())
            else:
                want.append(list(c(F)))
        torch.cuda.synchronize()
    return want


def decoy(eng, ntaxa):
    """Other rows through the scratch every resolve shares, so that what a case finds there when it does not wait is never
    what it expects: a range call without a quartet array over ranks no case uses, full mode."""
    import torch
    first, Q = (800, 1000) if ntaxa == T else (140, 70)
    o = row_outputs(Q)
    eng.resolve_range_dev(first, Q, False, 0, o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), 0)
    torch.cuda.synchronize()


def run_ordered(streams, prepare, first, second, ntaxa=T, warm=None, second_kind="enqueue", expect_wait=True, different=True):
    """One case: reference, a warmed engine, `ordered`, every output compared bitwise.  `second` is a Call, or with
    second_kind "host" a function of the engine that returns host arrays.  `warm`: the calls that size the engine's buffers
    (default: the two of the case)."""
    import torch
    from tetrad_amd.engine import QuartetEngine
    calls = [first, second]
    want = one_at_a_time(prepare, calls)
    assert all(any(np.asarray(a).any() for a in rows) for rows in want if rows), "the reference rows of a call are all zero"
    if different and want[0] and want[1] and len(want[0]) == len(want[1]):
        assert any(a.shape != b.shape or not np.array_equal(a, b) for a, b in zip(want[0], want[1])), "the two calls give the same rows"
    with QuartetEngine(0) as E:
        prepare(E)
        for c in (calls if warm is None else warm):
            if isinstance(c, Call):
                c.run(E, 0)
                torch.cuda.synchronize()
            else:
                c(E)
        decoy(E, ntaxa)
        for c in calls:
            if isinstance(c, Call):
                c.fill()
        got = [None, None]

        def run_second(s):
            if second_kind == "host":
                got[1] = list(second(E))
            else:
                second.run(E, s)

        def check():
            got[0] = first.rows()
            if second_kind != "host":
                got[1] = second.rows()
            assert_bitwise(got[0], want[0], f"first call, {first.name}")
            assert_bitwise(got[1], want[1], f"second call, {getattr(second, 'name', 'host call')}")

        ordered(streams, lambda s: first.run(E, s), run_second, check, second_kind, expect_wait)
    return want


def with_data(data, species=None):
    def prepare(eng):
        eng.set_data(*data)
        if species is not None:
            eng.set_species(species)
    return prepare


# ---- 1. the range call without a quartet array: it unranks into the shared scratch ----------------------------------------

@pytest.mark.parametrize("sub", [True, False])
def test_two_range_calls_without_a_quartet_array(streams, data, sub):
    """Ranks [0, 1000), then [700, 1300): before the fix the second call's unrank ran ahead of its wait, the first call's
    unrank then overwrote the scratch, and the second call's scan read the quartets of ranks [0, 600)."""
    run_ordered(streams, with_data(data), range_call(0, 1000, sub), range_call(700, 600, sub))


@pytest.mark.parametrize("order", ["range first", "range second"])
def test_range_call_and_resolve_dev(streams, data, order):
    a, b = range_call(0, 1000, True), resolve_call(ranks_to_quartets(700, 1300), False)
    run_ordered(streams, with_data(data), *((a, b) if order == "range first" else (b, a)))


# ---- 2. two resolves: count slab, ordering and singular-value scratch ----------------------------------------------------

def test_two_resolve_dev_calls(streams, data):
    run_ordered(streams, with_data(data), resolve_call(ranks_to_quartets(0, 1000)[::-1], True),
                resolve_call(ranks_to_quartets(900, 1700), False))


@pytest.mark.parametrize("order", ["species first", "species second"])
def test_species_resolve_and_resolve_dev(streams, data, order):
    a, b = species_call(ranks_to_quartets(0, 15, 6)), resolve_call(ranks_to_quartets(300, 315), False)
    run_ordered(streams, with_data(data, SPECIES_OF_16), *((a, b) if order == "species first" else (b, a)))


# ---- 3. the two halves of a resolve: the consumer reads the slab the producer writes ---------------------------------------

@pytest.mark.parametrize("sub", [True, False])
def test_scan_dev_then_svd_dev(streams, data, sub):
    run_ordered(streams, with_data(data), scan_call(ranks_to_quartets(100, 1100), sub), svd_call(200, 700), different=False)


# ---- 4. a replicate built on A, its consumers on B ---------------------------------------------------------------------------

def consumer(name, smin):
    starts = [0, 40, smin // 2, smin - 3]
    q = ranks_to_quartets(70, 134, 10)
    return {
        "resolve_dev": lambda: resolve_call(q, True),
        "patterns_dev": lambda: patterns_call(q[:20], True),
        "patterns_blocks_dev": lambda: blocks_call("patterns_blocks_dev", q[:20], starts),
        "patterns_quintet_blocks_dev": lambda: blocks_call("patterns_quintet_blocks_dev", sets5(10, 20), starts),
        "taxon_counts_dev": lambda: taxon_call(starts, 10),
        "resolve_species_dev": lambda: species_call(ranks_to_quartets(0, 5, 5)),
        "patterns_blocks_species_dev": lambda: blocks_call("patterns_blocks_species_dev", ranks_to_quartets(0, 5, 5), starts),
        "patterns_quintet_blocks_species_dev": lambda: blocks_call("patterns_quintet_blocks_species_dev", sets5(5, 1), starts),
    }[name]()


CONSUMERS = ["resolve_dev", "patterns_dev", "patterns_blocks_dev", "patterns_quintet_blocks_dev", "taxon_counts_dev",
             "resolve_species_dev", "patterns_blocks_species_dev", "patterns_quintet_blocks_species_dev"]


@pytest.mark.parametrize("boot_pack", [0, 1])
@pytest.mark.parametrize("name", CONSUMERS)
def test_consumer_behind_a_replicate_built_on_another_stream(streams, source, name, boot_pack):
    """tq_bootstrap_async on the held A, the consumer on B: the library orders it behind the build (the header's comment
    at tq_bootstrap_async once asked the caller to).  Another replicate is resident before, so a consumer that does not
    wait reads that one and gets other rows."""
    src, rep0, rep1 = source
    spans = src[1]
    smin = min(int((spans[r[0], 1] - spans[r[0], 0]).sum()) for r in (rep0, rep1))

    def prepare(eng):
        eng.set_option("boot_pack", boot_pack)
        eng.set_source(*src)
        eng.bootstrap(*rep0)
        if "species" in name:
            eng.set_species(SPECIES_OF_10)

    second = consumer(name, smin)
    stale = one_at_a_time(prepare, [second])[0]                        # the consumer's rows on the replicate resident before
    want = run_ordered(streams, prepare, bootstrap_call(rep1), second, ntaxa=10, warm=[second])
    assert any(not np.array_equal(a, b) for a, b in zip(stale, want[1])), "the two replicates give the same rows"


# ---- 5. block rows and taxon counts: the boundaries and the work items in one device array each -------------------------

def block_pair(kind):
    sets = ranks_to_quartets(0, 20)
    return {"blocks, blocks": lambda: (blocks_call("patterns_blocks_dev", sets, STARTS_B), blocks_call("patterns_blocks_dev", sets, STARTS_A)),
            "counts, counts": lambda: (taxon_call(STARTS_B), taxon_call(STARTS_A)),
            "blocks, counts": lambda: (blocks_call("patterns_blocks_dev", sets, STARTS_B), taxon_call(STARTS_A)),
            "counts, blocks": lambda: (taxon_call(STARTS_B), blocks_call("patterns_blocks_dev", sets, STARTS_A))}[kind]()


@pytest.mark.parametrize("kind", ["blocks, blocks", "counts, counts", "blocks, counts", "counts, blocks"])
def test_block_rows_and_taxon_counts(streams, data, kind):
    run_ordered(streams, with_data(data), *block_pair(kind))


# ---- 6. a host-buffer call behind a *_dev call -----------------------------------------------------------------------------

def host_call(name, other_data):
    q = ranks_to_quartets(900, 1700)
    return {"resolve": lambda e: e.resolve(q, True),
            "patterns": lambda e: (e.patterns(q[:20], True),),
            "patterns_blocks": lambda e: (e.patterns_blocks(q[:20], STARTS_A),),
            "taxon_counts": lambda e: (e.taxon_counts(STARTS_A),),
            "get_data": lambda e: e.get_data(),
            "set_data": lambda e: (e.set_data(*other_data), e.get_data())[1]}[name]


@pytest.mark.parametrize("first", ["resolve_dev", "range without a quartet array"])
@pytest.mark.parametrize("name", ["resolve", "patterns", "patterns_blocks", "taxon_counts", "get_data", "set_data"])
def test_host_call_behind_a_device_call(streams, data, other_data, name, first):
    """When the host call returns the hold is over; the device call's rows are those of the data resident when it was made
    (set_data replaces them only behind it), the host call's are the reference's."""
    dev = resolve_call(ranks_to_quartets(0, 1000), True) if first == "resolve_dev" else range_call(0, 1000, True)
    host = host_call(name, other_data)
    warm = [dev, host] if name != "set_data" else [dev, host, lambda e: e.set_data(*data)]
    run_ordered(streams, with_data(data), dev, host, warm=warm, second_kind="host", different=False)


# ---- 7. three calls, the third on the first call's stream: the "same stream as the last call" shortcut --------------------

def test_three_calls_A_B_A(streams, data):
    """A held, B, then A again; and the mirror image that can fail on time as well: one call on A, then B held with the
    second call behind it, then A again -- the third call enters on the stream of the FIRST call, which is not the stream
    of the last one, and has to wait for B."""
    import torch
    from tetrad_amd.engine import QuartetEngine
    calls = [range_call(0, 1000, True), range_call(700, 600, False), range_call(1200, 500, True)]
    want = one_at_a_time(with_data(data), calls)
    for held_first in (True, False):
        with QuartetEngine(0) as E:
            E.set_data(*data)
            for c in calls:
                c.run(E, 0)
            decoy(E, T)
            for c in calls:
                c.fill()

            def check():
                for c, w in zip(calls, want):
                    assert_bitwise(c.rows(), w, f"{c.name}, A held first: {held_first}")

            if held_first:
                def second(s):
                    calls[1].run(E, s)
                    calls[2].run(E, streams.A.cuda_stream)
                ordered(streams, lambda s: calls[0].run(E, s), second, check)
            else:
                if not runs_while_held(streams.B, streams.A):       # the fixture showed the pair the other way round only
                    pytest.fail("A does not run while B is held: the mirror image would pass its timing assertion vacuously")
                torch.cuda.synchronize()
                calls[0].run(E, streams.A.cuda_stream)
                ordered(Streams(streams.B, streams.A, 0), lambda s: calls[1].run(E, s), lambda s: calls[2].run(E, s), check)


# ---- entry points that touch only caller memory: they do NOT wait ----------------------------------------------------------

def caller_memory_call(name):
    import torch
    if name == "unrank_dev":
        ranks = np.arange(300, 1300, dtype=np.int64)
        d_r, out = torch.from_numpy(ranks).cuda(), torch.empty((1000, 4), dtype=torch.int32, device="cuda")
        want = [ranks_to_quartets(300, 1300).view(np.int32)]
        return Call(name, lambda e, s: e.unrank_dev(d_r.data_ptr(), 1000, out.data_ptr(), s), [out]), want
    if name == "sample_quartets_dev":
        out, d_r = torch.empty((1000, 4), dtype=torch.int32, device="cuda"), torch.empty((1000,), dtype=torch.int64, device="cuda")
        return Call(name, lambda e, s: e.sample_quartets_dev(7, 1000, out.data_ptr(), d_r.data_ptr(), s), [out, d_r]), None
    if name == "dstat_accumulate_dev":
        reps, set_of, ia, ib = pm.dstat_case(65)
        d = [dev_u32(reps[0]), dev_u32(set_of), torch.from_numpy(ia).cuda(), torch.from_numpy(ib).cuda()]
        acc = torch.zeros((65, 4), dtype=torch.float64, device="cuda")           # added to: its "sentinel" is zero
        return Call(name, lambda e, s: e.dstat_accumulate_dev(d[0].data_ptr(), len(reps[0]), d[1].data_ptr(), d[2].data_ptr(),
                                                              d[3].data_ptr(), 65, acc.data_ptr(), s), [acc], sentinel=0), \
            [np.array(pm.dstat_model(reps[:1], set_of, ia, ib))]
    if name == "dstat_jackknife_dev":
        rows, set_of, ia, ib = bm.jackknife_case(65, 3)
        d = [dev_u32(rows), dev_u32(set_of), torch.from_numpy(ia).cuda(), torch.from_numpy(ib).cuda()]
        out = torch.empty((65, 4), dtype=torch.float64, device="cuda")
        return Call(name, lambda e, s: e.dstat_jackknife_dev(d[0].data_ptr(), rows.shape[0], 3, d[1].data_ptr(), d[2].data_ptr(),
                                                             d[3].data_ptr(), 65, out.data_ptr(), s), [out]), \
            [bm.jackknife_model(rows, set_of, ia, ib)]
    rows, set_of, lmask, rmask = qm.jackknife_case(65, 3)
    d = [dev_u32(rows), dev_u32(set_of), torch.from_numpy(lmask.view(np.int16)).cuda(), torch.from_numpy(rmask.view(np.int16)).cuda()]
    out = torch.empty((65, 4), dtype=torch.float64, device="cuda")
    return Call(name, lambda e, s: e.dstat_jackknife_masks_dev(d[0].data_ptr(), rows.shape[0], 3, d[1].data_ptr(), d[2].data_ptr(),
                                                               d[3].data_ptr(), 65, out.data_ptr(), s), [out]), \
        [qm.jackknife_masks_model(rows, set_of, lmask, rmask)]


@pytest.mark.parametrize("name", ["unrank_dev", "sample_quartets_dev", "dstat_accumulate_dev", "dstat_jackknife_dev",
                                  "dstat_jackknife_masks_dev"])
def test_caller_memory_calls_do_not_wait(streams, data, name):
    """Queued on B behind a resolve on the held A, the call ends inside the hold; its rows are the model's."""
    second, model = caller_memory_call(name)
    want = run_ordered(streams, with_data(data), resolve_call(ranks_to_quartets(0, 1000), True), second, expect_wait=False,
                       different=False)
    if model is not None:
        assert_bitwise(want[1], model, f"{name} against its model")


# ---- accumulators: an enqueue on another stream first waits, a read or reset synchronises (StreamOrder) ---------------------

def same_result(got, want, what):
    """Results of a read, whatever their form: arrays bit for bit, everything else equal."""
    if isinstance(want, dict):
        assert got.keys() == want.keys(), what
        for k in want:
            same_result(got[k], want[k], f"{what}[{k}]")
    elif isinstance(want, (list, tuple)) and not (want and np.isscalar(want[0])):
        assert len(got) == len(want), what
        for i, (g, w) in enumerate(zip(got, want)):
            same_result(g, w, f"{what}[{i}]")
    elif isinstance(want, np.ndarray):
        assert_bitwise([got], [want], what)
    else:
        assert got == want, what


def nonzero(result):
    """Whether a read holds any count at all (a tree or a trace in text form counts as one)."""
    if isinstance(result, dict):
        return any(nonzero(v) for v in result.values())
    if isinstance(result, (list, tuple)):
        return any(nonzero(v) for v in result)
    if isinstance(result, np.ndarray):
        return bool(result.view(np.uint8).any()) if result.dtype.names else bool(np.asarray(result).any())
    return bool(result)


def run_accumulator(streams, make, first, second, after=None, host=None):
    """`make(engine)` creates the accumulator (engine None: its host back end); `first(acc, stream)` queues device work
    on the held A; `second(acc, stream)` makes the second call on B and reads, or reads or resets straight away, and
    returns what it read.  When it returns the hold must be over; what it read must equal, bit for bit, a fresh
    accumulator that was fed one call at a time, `host(acc)` of the host back end, and `after(acc)` checks the model."""
    import torch
    from tetrad_amd.engine import QuartetEngine
    with QuartetEngine(0) as F, make(F) as ref:
        st = torch.cuda.Stream()
        first(ref, st.cuda_stream)
        torch.cuda.synchronize()
        want = second(ref, st.cuda_stream)
        torch.cuda.synchronize()
    assert nonzero(want), "the reference read is all zero: the case would compare nothing"
    if host is not None:
        with make(None) as h:
            same_result(host(h), want, "host back end")
    with QuartetEngine(0) as E, make(E) as acc:
        got = ordered(streams, lambda s: first(acc, s), lambda s: second(acc, s), lambda: None, second_kind="host")
        same_result(got, want, "read behind the held add")
        if after is not None:
            after(acc)


# -- rows on a fixed tree: concordance and site concordance

@pytest.fixture(scope="module")
def fixed_tree_rows():
    """A random tree of 16 taxa; 2 rows aimed at every edge and 128 mixed rows; scores whose f64 sums are exact in any
    order (test_gpu_scf.py: multiples of 1/8 up to 64)."""
    from concordance_model import random_tree
    from scf_model import ScfModel, scf_rows
    rng = np.random.default_rng([T, 29])
    parent = random_tree(T, rng)
    sets, classes = scf_rows(ScfModel(parent, T), 2, 128, rng)
    n = len(sets)
    sc = np.stack([2.0 ** rng.integers(0, 3, n), rng.integers(4, 65, n), rng.integers(4, 65, n)], axis=1)
    sc = rng.permuted(sc.astype(np.float64), axis=1)
    st = np.stack([rng.integers(0, 3, n), rng.integers(0, 40, n)], axis=1).astype(np.uint32)
    return parent, np.array(sets, np.uint32), np.array(classes, np.uint32), st, sc


READS = ["add on B, read", "read", "reset, add on B, read"]


def in_turn(how, add1, add2, read, reset):
    """first and second of a case from the two adds, the read and the reset of an accumulator."""
    def second(acc, s):
        if how.startswith("reset"):
            reset(acc)
        if "add on B" in how:
            add2(acc, s)
        return read(acc)
    return add1, second


@pytest.mark.parametrize("how", READS)
def test_concordance_add_dev(streams, fixed_tree_rows, how):
    import torch
    from tetrad_amd.concordance import Concordance
    parent, sets, _, st, sc = fixed_tree_rows
    h = len(sets) // 3
    d_q, d_st, d_sc = dev_u32(sets), dev_u32(st), torch.from_numpy(sc).cuda()
    first, second = in_turn(how, lambda a, s: a.add_dev(d_q[:h], d_st[:h], d_sc[:h], None, stream=s),
                            lambda a, s: a.add_dev(d_q[h:], d_st[h:], d_sc[h:], None, stream=s),
                            lambda a: a.raw(), lambda a: a.reset())

    def host(a):
        lo, hi = {"add on B, read": (0, len(sets)), "read": (0, h), "reset, add on B, read": (h, len(sets))}[how]
        a.add(sets[lo:hi], sc[lo:hi], st[lo:hi])
        return a.raw()

    run_accumulator(streams, lambda e: Concordance(parent, ntaxa=T, min_snps=3, min_ratio=1.25, engine=e), first, second, host=host)


@pytest.mark.parametrize("how", READS)
def test_site_concordance_add_dev(streams, fixed_tree_rows, how):
    from scf_model import ScfModel, assert_matches
    from tetrad_amd.scf import SiteConcordance
    parent, sets, classes, _, _ = fixed_tree_rows
    h = len(sets) // 3
    d_s, d_c = dev_u32(sets), dev_u32(classes)
    first, second = in_turn(how, lambda a, s: a.add_dev(d_s[:h], d_c[:h], stream=s), lambda a, s: a.add_dev(d_s[h:], d_c[h:], stream=s),
                            lambda a: a.raw(), lambda a: a.reset())
    lo, hi = {"add on B, read": (0, len(sets)), "read": (0, h), "reset, add on B, read": (h, len(sets))}[how]

    def after(acc):
        model = ScfModel(parent, T)
        model.add(sets[lo:hi], classes[lo:hi])
        assert_matches(acc, model)

    run_accumulator(streams, lambda e: SiteConcordance(parent, ntaxa=T, engine=e), first, second, after=after,
                    host=lambda a: (a.add(sets[lo:hi], classes[lo:hi]), a.raw())[1])


# -- the supertree: rows added on A; a second add, a build, a fit, an NNI scan and a polish on B

@pytest.mark.parametrize("how", ["add on B, build", "build", "fit", "nni_scan", "polish", "reset, add on B, build"])
def test_supertree_behind_a_queued_add(streams, how):
    import torch
    from supertree_model import rows_from_tree
    from tetrad_amd.qmc import Supertree
    n = 600
    _, _, q, sc, st = rows_from_tree(T, n, "random", 0.2, seed=31)
    h = n // 2
    d_q, d_st, d_sc = dev_u32(q), dev_u32(st), torch.from_numpy(sc).cuda()
    with Supertree(T, n, 1) as hb:                                  # a tree to fit, scan and polish: the host build of half the rows
        hb.add(q[h:], sc[h:], st[h:])
        other = hb.tree(3)

    def add(lo, hi):
        return lambda a, s: a.add_dev_ptrs(d_q[lo:hi].data_ptr(), d_st[lo:hi].data_ptr(), d_sc[lo:hi].data_ptr(), 0, hi - lo, s)

    def second(acc, s):
        if how.startswith("reset"):
            acc.reset()
        if "add on B" in how:
            add(h, n)(acc, s)
        if how.endswith("build"):
            return acc.tree(9, stream=s), acc.levels
        if how == "fit":
            return acc.fit([other, "(" + ",".join(str(t) for t in range(T)) + ");"], stream=s)
        if how == "nni_scan":
            return acc.nni_scan(other, stream=s)
        nwk, trace = acc.polish(other, stream=s)
        return nwk, trace.moves, trace.gains, trace.converged

    lo, hi = {"add on B, build": (0, n), "reset, add on B, build": (h, n)}.get(how, (0, h))

    def host(a):
        a.add(q[lo:hi], sc[lo:hi], st[lo:hi])
        return second_on_host(a)

    def second_on_host(a):
        if how.endswith("build"):
            return a.tree(9), a.levels
        if how == "fit":
            return a.fit([other, "(" + ",".join(str(t) for t in range(T)) + ");"])
        if how == "nni_scan":
            return a.nni_scan(other)
        nwk, trace = a.polish(other)
        return nwk, trace.moves, trace.gains, trace.converged

    run_accumulator(streams, lambda e: Supertree(T, n, 1, engine=e), add(0, h), second, host=host)


# -- tree sets: 12 trees of 12 taxa

TREES_T = 12


@pytest.fixture(scope="module")
def trees12():
    import consensus_model as cm
    return cm.tree_set(TREES_T, seed=TREES_T)[:12]


def tree_set_case(how, read, trees):
    """Six trees on A; six more on B and a read, a read straight away, or a reset and six on B; the trees the read sees."""
    first, second = in_turn(how, lambda a, s: a.add_parents(trees[:6], stream=s), lambda a, s: a.add_parents(trees[6:], stream=s),
                            read, lambda a: a.reset())
    seen = {"add on B, read": slice(0, 12), "read": slice(0, 6), "reset, add on B, read": slice(6, 12)}[how]
    return first, second, seen


@pytest.mark.parametrize("how", READS)
def test_consensus_add(streams, trees12, how):
    import consensus_model as cm
    from tetrad_amd.consensus import Consensus
    first, second, seen = tree_set_case(how, lambda a: a.raw(), trees12)
    run_accumulator(streams, lambda e: Consensus(TREES_T, engine=e), first, second,
                    after=lambda a: cm.assert_matches(a, *cm.model_of(trees12[seen], TREES_T), TREES_T),
                    host=lambda a: (a.add_parents(trees12[seen]), a.raw())[1])


@pytest.mark.parametrize("how", READS)
def test_transfer_support_add(streams, trees12, how):
    import tbe_model as tm
    from tetrad_amd.tbe import TransferSupport
    first, second, seen = tree_set_case(how, lambda a: a.raw(), trees12)
    run_accumulator(streams, lambda e: TransferSupport(TREES_T, trees12[0], engine=e), first, second,
                    after=lambda a: tm.assert_matches(a, *tm.expected(trees12[0], trees12[seen], TREES_T)),
                    host=lambda a: (a.add_parents(trees12[seen]), a.raw())[1])


@pytest.mark.parametrize("how", READS)
def test_tree_distances_add(streams, trees12, how):
    import treedist_model as dm
    from tetrad_amd.treedist import TreeDistances
    first, second, seen = tree_set_case(how, lambda a: (a.nsplits(), a.shared(), a.rf()), trees12)
    run_accumulator(streams, lambda e: TreeDistances(TREES_T, 12, engine=e), first, second,
                    after=lambda a: dm.assert_matches(a, *dm.expected(trees12[seen], TREES_T)[:3]),
                    host=lambda a: (a.add_parents(trees12[seen]), (a.nsplits(), a.shared(), a.rf()))[1])


SCORES = ["add on B, score on B, read", "score on A; score on B, read", "score on A; read", "score on A; clear, score on B, read"]


def scoring_case(how, trees, read):
    """`tq_*_add` and `tq_*_score` on the held A, then a score on B and a read.  Returns first, second, the trees and the
    quartet ranks [lo, hi) the read sees."""
    Q = 495                                                             # C(12, 4)
    if how == SCORES[0]:
        return (lambda a, s: a.add_parents(trees[:6], stream=s),
                lambda a, s: (a.add_parents(trees[6:], stream=s), a.score_range(0, Q, stream=s), read(a))[2], trees, (0, Q))

    def first(a, s):
        a.add_parents(trees, stream=s)
        a.score_range(0, 300, stream=s)

    if how == SCORES[1]:
        return first, lambda a, s: (a.score_range(300, Q - 300, stream=s), read(a))[1], trees, (0, Q)
    if how == SCORES[2]:
        return first, lambda a, s: read(a), trees, (0, 300)
    return first, lambda a, s: (a.clear(), a.score_range(300, Q - 300, stream=s), read(a))[2], trees, (300, Q)


@pytest.mark.parametrize("how", SCORES)
def test_quartet_distances_add_and_score(streams, trees12, how):
    import qdist_model as qm
    from tetrad_amd.qdist import QuartetDistances
    first, second, trees, (lo, hi) = scoring_case(how, trees12, lambda a: a.raw())
    quartets = qm.all_quartets(TREES_T)[lo:hi]
    run_accumulator(streams, lambda e: QuartetDistances(TREES_T, 12, engine=e), first, second,
                    after=lambda a: qm.assert_matches(a, qm.expected(trees, TREES_T, quartets), hi - lo),
                    host=lambda a: (a.add_parents(trees), a.score_range(lo, hi - lo), a.raw())[2])


@pytest.mark.parametrize("how", SCORES)
def test_leaf_stability_add_and_score(streams, trees12, how):
    import qdist_model as qm
    import stability_model as sm
    from tetrad_amd.stability import LeafStability
    first, second, trees, (lo, hi) = scoring_case(how, trees12, lambda a: a.raw())
    quartets = qm.all_quartets(TREES_T)[lo:hi]
    run_accumulator(streams, lambda e: LeafStability(TREES_T, 12, engine=e), first, second,
                    after=lambda a: sm.assert_matches(a, None, *sm.expected(trees, TREES_T, quartets), len(trees)),
                    host=lambda a: (a.add_parents(trees), a.score_range(lo, hi - lo), a.raw())[2])


# -- the context must outlive its accumulators: closing the engine closes them first

def test_closing_an_engine_closes_its_accumulators_first(trees12):
    """The library's accumulators select their context's device and wait for their own work when they go, so the context
    has to be there: an engine that is closed with accumulators still open -- here one with an add queued, and one that
    nothing refers to but a reference cycle -- closes them before its context, and their own close is then a no-op."""
    import gc
    import consensus_model as cm
    from tetrad_amd.consensus import Consensus
    from tetrad_amd.engine import QuartetEngine
    from tetrad_amd.treedist import TreeDistances
    gc.collect()
    E = QuartetEngine(0)
    used = Consensus(TREES_T, engine=E)
    used.add_parents(trees12[:6])
    cycle = [TreeDistances(TREES_T, 12, engine=E)]
    cycle.append(cycle)                                   # only the collector frees it
    forgotten = cycle[0]
    del cycle
    E.close()
    assert used._h is None and forgotten._h is None and E._h is None
    used.close()
    del forgotten
    gc.collect()
    with QuartetEngine(0) as N, Consensus(TREES_T, engine=N) as acc:        # the device is as it was
        acc.add_parents(trees12)
        cm.assert_matches(acc, *cm.model_of(trees12, TREES_T), TREES_T)

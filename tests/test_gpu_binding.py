"""GPU: the shared handle base and tree-input path with an engine -- every tree-set accumulator and the supertree fed
three 8-taxon trees on the device equal their host twins, an invalid third tree is refused by the library's host-side
validation with a message read from the engine's context, and every accumulator is closed before the engine."""
import numpy as np
import pytest

from tetrad_amd._lib import TetradHipError
from tetrad_amd.concordance import newick_to_parent
from tetrad_amd.consensus import Consensus
from tetrad_amd.qdist import QuartetDistances
from tetrad_amd.qmc import Supertree
from tetrad_amd.tbe import TransferSupport
from tetrad_amd.treedist import TreeDistances

pytestmark = pytest.mark.gpu

T = 8
TREES = ["(((0,1),(2,3)),((4,5),(6,7)));", "(((0,2),(1,3)),((4,6),(5,7)));", "((0,(1,(2,3))),((4,5),(6,7)));"]


@pytest.fixture(scope="module")
def engine():
    from tetrad_amd.engine import QuartetEngine
    with QuartetEngine(0) as e:
        yield e
        assert e._h                                  # still open after every accumulator of this module has closed


def parents_with_a_cycle():
    """The three trees as parent arrays, the last two internal nodes of the third made each other's parent."""
    parents = [newick_to_parent(t)[0] for t in TREES]
    bad = parents[2].copy()
    bad[-1], bad[-2] = len(bad) - 2, len(bad) - 1
    return parents[:2] + [bad]


def same(got, want):
    for a, b in zip(got, want):
        np.testing.assert_array_equal(a, b)


TREE_SETS = {
    "Consensus": (lambda engine=None: Consensus(T, engine=engine), "tq_cons_add"),
    "TransferSupport": (lambda engine=None: TransferSupport(T, TREES[0], engine=engine), "tq_tbe_add"),
    "TreeDistances": (lambda engine=None: TreeDistances(T, 4, engine=engine), "tq_rf_add"),
    "QuartetDistances": (lambda engine=None: QuartetDistances(T, 4, engine=engine), "tq_qd_add"),
}


@pytest.mark.parametrize("name", TREE_SETS)
def test_tree_sets_equal_the_host_and_refuse_a_bad_tree(engine, name):
    create, add_call = TREE_SETS[name]
    with create(engine) as dev, create() as host:
        assert dev.engine is engine and host.engine is None
        with pytest.raises(TetradHipError, match=f"{add_call}: tree 2") as info:
            dev.add_parents(parents_with_a_cycle())
        assert info.value.code == -1 and dev.ntrees == 0
        dev.add_newick(TREES)
        host.add_newick(TREES)
        if name == "QuartetDistances":
            dev.score_all()
            host.score_all()
        assert dev.ntrees == host.ntrees == 3
        same(dev.raw(), host.raw())
        dev.reset()
        assert dev.ntrees == 0
    assert dev._h is None and host._h is None and engine._h


def test_supertree_equals_the_host_and_refuses_a_bad_tree(engine):
    import torch
    q = np.array([[0, 1, 2, 3], [0, 2, 4, 6], [1, 3, 5, 7], [0, 1, 4, 5], [2, 3, 6, 7]], np.uint32)
    sc = np.tile(np.array([0.1, 0.5, 0.9]), (len(q), 1))
    st = np.array([[0, 10], [1, 12], [2, 9], [0, 30], [0, 7]], np.uint32)
    dq, dst, dsc = torch.tensor(q.view(np.int32)).cuda(), torch.tensor(st.view(np.int32)).cuda(), torch.tensor(sc).cuda()
    with Supertree(T, len(q), 1, engine=engine) as dev, Supertree(T, len(q), 1) as host:
        dev.add_dev_ptrs(dq.data_ptr(), dst.data_ptr(), dsc.data_ptr(), 0, len(q), torch.cuda.current_stream().cuda_stream)
        host.add(q, sc, st)
        assert dev.counts() == host.counts() and dev.counts()[0] == len(q)
        with pytest.raises(TetradHipError, match="tq_stree_fit: tree 2") as info:
            dev.fit(parents_with_a_cycle())
        assert info.value.code == -1
        got, want = dev.fit(TREES), host.fit(TREES)
        assert got.dtype == want.dtype and len(got) == 3
        for field in got.dtype.names:
            np.testing.assert_array_equal(got[field], want[field])
        assert dev.tree(3) == host.tree(3)
        torch.cuda.synchronize()
    assert dev._h is None and host._h is None and engine._h

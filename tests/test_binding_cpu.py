"""CPU-only: what the Python classes over a library handle share -- the life cycle of `_handle.Handle` on the host
path of every accumulator, the one tree-input path (`concordance.parent_block`, `trees_to_parents`, `TreeSetInput`)
and its one wording of a wrong taxon count."""
import gc
import sys

import numpy as np
import pytest

from tetrad_amd import _lib
from tetrad_amd.concordance import Concordance, newick_to_parent, parent_block
from tetrad_amd.consensus import Consensus
from tetrad_amd.qdist import QuartetDistances
from tetrad_amd.qmc import Supertree
from tetrad_amd.scf import SiteConcordance
from tetrad_amd.tbe import TransferSupport
from tetrad_amd.treedist import TreeDistances

T = 8
TREE = "(((0,1),(2,3)),((4,5),(6,7)));"
OTHER = "(((0,2),(1,3)),((4,6),(5,7)));"
SEVEN = "(((0,1),(2,3)),((4,5),6));"
STAR3 = np.array([3, 3, 3, -1], np.int32)           # three tips under one root: no tree for the library


@pytest.fixture(scope="module", autouse=True)
def lib():
    _lib.build()
    return _lib.load()


def rows():
    """Two resolved quartet rows as `Concordance.add` / `Supertree.add` take them."""
    q = np.array([[0, 1, 2, 3], [0, 2, 4, 6]], np.uint32)
    return q, np.array([[0.1, 0.5, 0.9]] * 2), np.array([[0, 10], [1, 12]], np.uint32)


def _use_conc(a):
    a.add(*rows())
    return int(a.raw()["edge_counts"][:, 0].sum())


def _use_scf(a):
    a.add(np.array([[0, 2, 4, 6]], np.uint32), np.arange(16, dtype=np.uint32)[None, :])
    return int(a.raw()["edge_counts"][:, 0].sum())


def _use_stree(a):
    a.add(*rows())
    return a.counts()[0]


def _use_trees(a):
    a.add_newick([TREE, OTHER])
    return a.ntrees


#: name -> (create on 8 taxa, a create the library refuses, what it says, add something and read a count that is > 0)
#: The refused create has ntaxa = 3, except for the supertree: its host back end takes 1..65535 taxa, so it gets 0.
CLASSES = {
    "Concordance": (lambda: Concordance(TREE), lambda: Concordance(STAR3, ntaxa=3), "tq_conc_create", _use_conc),
    "SiteConcordance": (lambda: SiteConcordance(TREE), lambda: SiteConcordance(STAR3, ntaxa=3), "tq_scf_create", _use_scf),
    "Supertree": (lambda: Supertree(T, 16), lambda: Supertree(0, 16), "tq_stree_create", _use_stree),
    "Consensus": (lambda: Consensus(T), lambda: Consensus(3), "tq_cons_create", _use_trees),
    "TransferSupport": (lambda: TransferSupport(T, TREE), lambda: TransferSupport(3, STAR3), "tq_tbe_create", _use_trees),
    "TreeDistances": (lambda: TreeDistances(T, 4), lambda: TreeDistances(3, 4), "tq_rf_create", _use_trees),
    "QuartetDistances": (lambda: QuartetDistances(T, 4), lambda: QuartetDistances(3, 4), "tq_qd_create", _use_trees),
}
TREE_SETS = ("Consensus", "TransferSupport", "TreeDistances", "QuartetDistances")


@pytest.mark.parametrize("name", CLASSES)
def test_close_twice_and_context_manager(name):
    create = CLASSES[name][0]
    acc = create()
    assert acc._h and acc.engine is None
    acc.close()
    assert acc._h is None
    acc.close()
    with create() as acc:
        assert acc._h
    assert acc._h is None


@pytest.mark.parametrize("name", CLASSES)
def test_failed_create_raises_the_librarys_message_and_dies_silently(name, monkeypatch):
    create, refused, said = CLASSES[name][:3]
    unraisable = []
    monkeypatch.setattr(sys, "unraisablehook", unraisable.append)
    with pytest.raises(_lib.TetradHipError, match=said) as info:
        refused()
    assert info.value.code == -1
    del info
    gc.collect()                                     # the half-made object dies here at the latest
    assert not unraisable
    with create() as made:
        half = type(made).__new__(type(made))        # what an __init__ that failed before create leaves behind
    assert half._h is None
    half.close()
    half.__del__()


@pytest.mark.parametrize("name", CLASSES)
def test_a_method_after_reset_still_works(name):
    create, _, _, use = CLASSES[name]
    with create() as acc:
        first = use(acc)
        assert first > 0
        acc.reset()
        assert use(acc) == first


# -- the tree block ---------------------------------------------------------------------------------------------
def ragged():
    return [np.arange(7, dtype=np.int32), np.arange(10, dtype=np.int64), list(range(9))]


def test_parent_block_pads_ragged_arrays_with_minus_one():
    block, n_nodes, stride = parent_block(ragged())
    assert block.dtype == np.int32 and block.shape == (3, 10) and stride == 10
    assert n_nodes.dtype == np.int64 and n_nodes.tolist() == [7, 10, 9]
    for row, n in zip(block, (7, 10, 9)):
        assert row[:n].tolist() == list(range(n)) and (row[n:] == -1).all()
    from_generator = parent_block(p for p in ragged())
    assert np.array_equal(from_generator[0], block) and np.array_equal(from_generator[1], n_nodes)
    empty, n0, stride0 = parent_block([])
    assert empty.shape == (0, 0) and n0.dtype == np.int64 and len(n0) == 0 and stride0 == 0
    assert parent_block([], 1)[0].shape == (0, 1)


@pytest.mark.parametrize("name", TREE_SETS)
def test_a_generator_of_parents_adds_and_nothing_makes_no_library_call(name):
    parents = [newick_to_parent(t)[0] for t in (TREE, OTHER)]
    with CLASSES[name][0]() as acc:
        acc.add_parents(p for p in parents)
        assert acc.ntrees == 2

        def no_call(*a):
            raise AssertionError("an empty add reached the library")

        acc._add = no_call
        assert acc.add_parents([]) is None and acc.add_parents(iter(())) is None and acc.add_newick([]) is None
        assert acc.ntrees == 2


def test_transfer_support_per_tree_goes_through_the_same_hook():
    parents = [newick_to_parent(t)[0] for t in (TREE, OTHER)]
    with TransferSupport(T, TREE) as acc:
        phi = acc.add_parents((p for p in parents), per_tree=True)
        assert phi.dtype == np.uint16 and phi.shape == (2, acc.nbranches)
        assert not phi[0].any() and phi[1].any()
        assert np.array_equal(acc.add_newick([TREE, OTHER], per_tree=True), phi)
        none = acc.add_parents([], per_tree=True)
        assert none.dtype == np.uint16 and none.shape == (0, acc.nbranches)
        assert acc.ntrees == 4


# -- one wording ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", TREE_SETS)
def test_wrong_taxon_count_and_malformed_text_name_the_tree(name):
    with CLASSES[name][0]() as acc:
        with pytest.raises(ValueError, match="tree 1: 7 taxa"):
            acc.add_newick([TREE, SEVEN])
        with pytest.raises(ValueError, match="tree 0"):
            acc.add_newick(["((0,1),(2,3);", TREE])
        assert acc.ntrees == 0                       # nothing is added when one tree is refused


def test_samples_default_to_those_of_create_only_where_they_did():
    names = list("abcdefgh")
    named = "(((a,b),(c,d)),((e,f),(g,h)));"
    for cls in (TreeDistances, QuartetDistances):
        with cls(T, 4, samples=names) as acc:
            acc.add_newick([named])
            assert acc.ntrees == 1
    with TransferSupport(T, named, samples=names) as acc:
        with pytest.raises(ValueError, match="tree 0"):
            acc.add_newick([named])
        acc.add_newick([named], samples=names)
        assert acc.ntrees == 1

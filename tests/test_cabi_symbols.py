"""CPU-only: the C-ABI library builds, loads and exports every symbol the header declares."""
import ctypes
import re

import pytest

from tetrad_amd import _lib


@pytest.fixture(scope="module")
def lib():
    _lib.build()
    return _lib.load()


def header_symbols():
    text = _lib.HEADER.read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(tq_[a-z_]+)\s*\(", text)))


def test_header_and_binding_agree():
    assert header_symbols() == sorted(_lib.SYMBOLS)


def header_declarations():
    """{name: (result type text, number of parameters)} of every function the header declares.  The header has no
    function-pointer parameters, so the parameter list splits at its commas."""
    text = re.sub(r"/\*.*?\*/", "", _lib.HEADER.read_text(), flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    decls = {}
    for result, name, params in re.findall(r"([A-Za-z_][\w \t\*]*?)\b(tq_[a-z_0-9]+)\s*\(([^()]*)\)\s*;", text):
        params = params.strip()
        decls[name] = (" ".join(result.split()), 0 if params in ("", "void") else len(params.split(",")))
    return decls


def test_prototypes_match_the_header():
    """Every declared function has one prototype with the header's number of parameters, and no result type exactly
    where the header says void: a missing or short prototype would pass 64-bit values through ctypes' int default."""
    decls = header_declarations()
    assert sorted(decls) == header_symbols()
    assert sorted(decls) == sorted(_lib.PROTOTYPES)
    for name, (result, nparams) in decls.items():
        argtypes, restype = _lib.PROTOTYPES[name]
        assert len(argtypes) == nparams, f"{name}: {len(argtypes)} argument types, the header declares {nparams}"
        assert (restype is None) == (result == "void"), f"{name}: result {restype}, the header says {result!r}"


def test_load_declares_every_prototype(lib):
    for name, (argtypes, restype) in _lib.PROTOTYPES.items():
        fn = getattr(lib, name)
        assert list(fn.argtypes) == argtypes and fn.restype is restype, name


def test_every_declared_symbol_is_exported(lib):
    for name in header_symbols():
        assert hasattr(lib, name), f"{name} not exported by {_lib.LIB_PATH}"


def test_no_device_is_a_clean_error(lib):
    """Without a GPU tq_create must fail with an error code and a message, never crash."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    h = ctypes.c_void_p()
    rc = lib.tq_create(ctypes.byref(h), 0)
    assert rc == -2 and not h.value
    assert b"HIP device" in lib.tq_last_error(None)


def test_null_context_is_rejected(lib):
    assert lib.tq_set_option(None, b"nrep", 8) == -1
    assert lib.tq_timing_enable(None, 1) == -1
    lib.tq_destroy(None)  # no-op


def test_product_does_not_import_oracle():
    """The product package must never reach into oracle/ (test infrastructure)."""
    from pathlib import Path
    for p in Path(_lib.CSRC).parent.rglob("*.py"):
        src = p.read_text()
        assert "import oracle" not in src and "from oracle" not in src, p

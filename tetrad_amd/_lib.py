"""ctypes binding of libtetrad_hip.so (the C ABI declared in include/tetrad_hip.h).

There is no CPU fallback: if the HIP library is missing or cannot be loaded the
import-time helper raises, and every compute entry point raises TetradHipError
on a non-zero return code (message from the library's last-error text).
"""
from __future__ import annotations

import ctypes
import os
import sys
import shutil
import subprocess
from pathlib import Path

CSRC = Path(__file__).resolve().parent / "csrc"
LIB_PATH = CSRC / "libtetrad_hip.so"
SRC_PATH = CSRC / "tetrad_hip.hip"
HEADER = Path(__file__).resolve().parents[1] / "include" / "tetrad_hip.h"

TQ_OK = 0
ERR_NAMES = {
    -1: "TQ_ERR_INVALID_ARG", -2: "TQ_ERR_NO_DEVICE", -3: "TQ_ERR_HIP",
    -4: "TQ_ERR_NO_DATA", -5: "TQ_ERR_LOCUS_ORDER", -6: "TQ_ERR_OOM",
}
FLAG_ZERO_DATA, FLAG_DEGENERATE, FLAG_BAD_INDEX, FLAG_NO_CONVERGENCE, FLAG_INVALID_DIAGNOSTIC = 1, 2, 4, 8, 16

vp, text, f64 = ctypes.c_void_p, ctypes.c_char_p, ctypes.c_double
i32, i64, u32, u64 = ctypes.c_int, ctypes.c_int64, ctypes.c_uint32, ctypes.c_uint64
P = ctypes.POINTER


def _sig(*argtypes, ret=i32):
    return list(argtypes), ret


#: every function include/tetrad_hip.h declares, in its order: the argument types and, where it is not int, the result
#: type (None = void).  `load()` declares exactly these; tests/test_cabi_symbols.py compares names, arity and void
#: results with the header.  Array and handle arguments are plain addresses (vp); P(...) marks a by-reference scalar.
PROTOTYPES = {
    # -- context, resident data, bootstrap replicates
    "tq_create": _sig(P(vp), i32),
    "tq_destroy": _sig(vp, ret=None),
    "tq_last_error": _sig(vp, ret=text),
    "tq_set_data": _sig(vp, vp, i64, i64, vp, i64),
    "tq_set_source": _sig(vp, vp, i64, i64, vp, i64),
    "tq_bootstrap": _sig(vp, vp, i64, u64, u64, P(i64)),
    "tq_bootstrap_async": _sig(vp, vp, i64, u64, u64, P(i64), vp),
    "tq_get_data": _sig(vp, vp, vp),
    "tq_data_shape": _sig(vp, P(i64), P(i64)),
    # -- resolving quartets: host rows, the pinned pool, device rows, the two halves, ranks
    "tq_resolve": _sig(vp, vp, i64, i32, vp, vp, vp),
    "tq_host_alloc": _sig(i64, P(vp)),
    "tq_host_free": _sig(vp),
    "tq_resolve_to_host": _sig(vp, vp, i64, i32, vp, vp, vp),
    "tq_resolve_dev": _sig(vp, vp, i64, i32, vp, vp, vp, vp),
    "tq_resolve_range_dev": _sig(vp, u64, i64, i32, vp, vp, vp, vp, vp),
    "tq_scan_dev": _sig(vp, vp, i64, i32, vp),
    "tq_svd_dev": _sig(vp, i64, i64, vp, vp, vp, vp),
    "tq_unrank_dev": _sig(vp, vp, i64, vp, vp),
    "tq_sample_quartets_dev": _sig(vp, u64, i64, vp, vp, vp),
    "tq_resolve_debug": _sig(vp, vp, i64, i32, vp, vp, vp, vp, vp, vp),
    # -- timing, options, test hooks
    "tq_timing_enable": _sig(vp, i32),
    "tq_timing_read": _sig(vp, P(f64), P(i64)),
    "tq_timing_read_split": _sig(vp, P(f64), P(f64), P(f64), P(i64)),
    "tq_timing_read_kernels": _sig(vp, P(f64), i32, P(i64)),
    "tq_set_option": _sig(vp, text, i64),
    "tq_debug_fetch": _sig(vp, i32, vp, i64),
    "tq_scan_plan": _sig(vp, i64, vp, P(i64)),
    "tq_debug_bdsqr": _sig(vp, vp, i64, vp, vp, i32, P(f64)),
    # -- host helpers without a context: formats, site packing, ranks, Quartet MaxCut
    "tq_format_tsv": _sig(vp, vp, vp, i64, vp, i64, P(i64)),
    "tq_format_qmc": _sig(vp, vp, vp, i64, i32, i64, f64, vp, i64, P(i64), P(i64)),
    "tq_pack_sites": _sig(vp, i64, i64, vp, i64, vp, i64, P(i64), P(i32), vp),
    "tq_numpy_choice_tail": _sig(vp, u64, i64, vp),
    "tq_unrank": _sig(vp, u64, i64, i64, vp),
    "tq_qmc_splits": _sig(vp, vp, vp, i64, i32, i64, f64, vp, vp, P(i64)),
    "tq_qmc_tree": _sig(vp, vp, i64, i64, u64, vp, i64, P(i64)),
    # -- quartet concordance on a fixed tree
    "tq_conc_create": _sig(P(vp), vp, i64, i64, i64, f64, vp),
    "tq_conc_destroy": _sig(vp, ret=None),
    "tq_conc_reset": _sig(vp),
    "tq_conc_add": _sig(vp, vp, vp, vp, vp, i64),
    "tq_conc_add_dev": _sig(vp, vp, vp, vp, vp, i64, vp),
    "tq_conc_shape": _sig(vp, P(i64), P(i64), P(i64)),
    "tq_conc_read": _sig(vp, vp, vp, vp, vp, P(i64)),
    # -- exact supertree
    "tq_stree_create": _sig(P(vp), i64, i64, i32, i64, f64, vp),
    "tq_stree_destroy": _sig(vp, ret=None),
    "tq_stree_reset": _sig(vp),
    "tq_stree_add": _sig(vp, vp, vp, vp, vp, i64),
    "tq_stree_add_dev": _sig(vp, vp, vp, vp, vp, i64, vp),
    "tq_stree_graph": _sig(vp, vp, vp, P(i64), P(i64), P(u64)),
    "tq_stree_rows": _sig(vp, vp, vp, P(i64)),
    "tq_stree_build": _sig(vp, u64, vp, vp, i64, P(i64), P(i64)),
    "tq_stree_level_stats": _sig(vp, P(i64), vp),
    "tq_stree_set_search": _sig(vp, i32),
    "tq_stree_fit": _sig(vp, vp, vp, i64, i64, vp, vp),
    "tq_stree_nni_scan": _sig(vp, vp, i64, vp, P(i64), vp, vp, vp),
    "tq_stree_polish": _sig(vp, vp, i64, i64, vp, vp, i64, P(i64), vp, P(i64), P(i32)),
    "tq_stree_search": _sig(vp, i64, vp, vp, vp, vp, vp, vp, vp),
    # -- consensus: split counts of tree sets
    "tq_cons_create": _sig(P(vp), i64, i64, vp),
    "tq_cons_destroy": _sig(vp, ret=None),
    "tq_cons_reset": _sig(vp),
    "tq_cons_add": _sig(vp, vp, vp, i64, i64, vp),
    "tq_cons_shape": _sig(vp, P(i64), P(i64), P(i64), P(i64)),
    "tq_cons_read": _sig(vp, vp, vp),
    "tq_cons_tree": _sig(vp, i64, vp, i64, P(i64)),
    "tq_cons_support": _sig(vp, vp, i64, vp, vp, P(i64)),
    "tq_cons_stats": _sig(vp, vp),
    # -- transfer bootstrap supports
    "tq_tbe_create": _sig(P(vp), i64, vp, i64, vp),
    "tq_tbe_destroy": _sig(vp, ret=None),
    "tq_tbe_reset": _sig(vp),
    "tq_tbe_add": _sig(vp, vp, vp, i64, i64, vp, vp),
    "tq_tbe_shape": _sig(vp, P(i64), P(i64), P(i64), P(i64)),
    "tq_tbe_read": _sig(vp, vp, vp, vp),
    "tq_tbe_stats": _sig(vp, vp),
    # -- Robinson-Foulds distances
    "tq_rf_create": _sig(P(vp), i64, i64, i64, vp),
    "tq_rf_destroy": _sig(vp, ret=None),
    "tq_rf_reset": _sig(vp),
    "tq_rf_add": _sig(vp, vp, vp, i64, i64, vp),
    "tq_rf_shape": _sig(vp, P(i64), P(i64), P(i64), P(i64), P(i64)),
    "tq_rf_read": _sig(vp, vp, vp, vp),
    "tq_rf_stats": _sig(vp, vp),
    "tq_rf_word_shared": _sig(u64, u64, ret=u32),
    # -- quartet distances
    "tq_qd_create": _sig(P(vp), i64, i64, vp),
    "tq_qd_destroy": _sig(vp, ret=None),
    "tq_qd_reset": _sig(vp),
    "tq_qd_clear": _sig(vp),
    "tq_qd_add": _sig(vp, vp, vp, i64, i64, vp),
    "tq_qd_score": _sig(vp, vp, i64, vp),
    "tq_qd_score_ranks": _sig(vp, vp, u64, i64, vp),
    "tq_qd_shape": _sig(vp, P(i64), P(i64), P(u64)),
    "tq_qd_read": _sig(vp, vp, vp),
    "tq_qd_stats": _sig(vp, vp),
    "tq_qd_word_counts": _sig(u64, u64, u64, u64, u64, u64, P(u32), P(u32), ret=None),
    # -- quartet frequencies and leaf stability
    "tq_ls_create": _sig(P(vp), i64, i64, vp),
    "tq_ls_destroy": _sig(vp, ret=None),
    "tq_ls_reset": _sig(vp),
    "tq_ls_clear": _sig(vp),
    "tq_ls_add": _sig(vp, vp, vp, i64, i64, vp),
    "tq_ls_score": _sig(vp, vp, i64, vp, vp),
    "tq_ls_score_ranks": _sig(vp, vp, u64, i64, vp, vp),
    "tq_ls_shape": _sig(vp, P(i64), P(i64), P(u64)),
    "tq_ls_read": _sig(vp, vp),
    "tq_ls_stats": _sig(vp, vp),
    # -- species mode
    "tq_set_species": _sig(vp, vp, i64, i64),
    "tq_resolve_species": _sig(vp, vp, i64, vp, vp, vp),
    "tq_resolve_species_dev": _sig(vp, vp, i64, vp, vp, vp, vp),
    "tq_resolve_species_debug": _sig(vp, vp, i64, vp, vp, vp, vp, vp, vp),
    # -- site-pattern classes and D tests: whole rows, per block, pooled by species
    "tq_pattern_class_table": _sig(vp),
    "tq_patterns": _sig(vp, vp, i64, i32, vp),
    "tq_patterns_dev": _sig(vp, vp, i64, i32, vp, vp),
    "tq_patterns_species": _sig(vp, vp, i64, vp),
    "tq_patterns_species_dev": _sig(vp, vp, i64, vp, vp),
    "tq_dstat_accumulate": _sig(vp, i64, vp, vp, vp, i64, vp),
    "tq_dstat_accumulate_dev": _sig(vp, vp, i64, vp, vp, vp, i64, vp, vp),
    "tq_patterns_blocks": _sig(vp, vp, i64, vp, i64, vp),
    "tq_patterns_blocks_dev": _sig(vp, vp, i64, vp, i64, vp, vp),
    "tq_dstat_jackknife": _sig(vp, i64, i64, vp, vp, vp, i64, vp),
    "tq_dstat_jackknife_dev": _sig(vp, vp, i64, i64, vp, vp, vp, i64, vp, vp),
    "tq_patterns_blocks_species": _sig(vp, vp, i64, vp, i64, vp),
    "tq_patterns_blocks_species_dev": _sig(vp, vp, i64, vp, i64, vp, vp),
    "tq_pooled_site_classes": _sig(vp, vp),
    # -- five-taxon patterns
    "tq_quintet_class_table": _sig(vp),
    "tq_patterns_quintet_blocks": _sig(vp, vp, i64, vp, i64, vp),
    "tq_patterns_quintet_blocks_dev": _sig(vp, vp, i64, vp, i64, vp, vp),
    "tq_dstat_jackknife_masks": _sig(vp, i64, i64, vp, vp, vp, i64, vp),
    "tq_dstat_jackknife_masks_dev": _sig(vp, vp, i64, i64, vp, vp, vp, i64, vp, vp),
    "tq_patterns_quintet_blocks_species": _sig(vp, vp, i64, vp, i64, vp),
    "tq_patterns_quintet_blocks_species_dev": _sig(vp, vp, i64, vp, i64, vp, vp),
    "tq_pooled_quintet_site_classes": _sig(vp, vp),
    # -- site concordance on a fixed tree
    "tq_scf_create": _sig(P(vp), vp, i64, i64, vp),
    "tq_scf_destroy": _sig(vp, ret=None),
    "tq_scf_reset": _sig(vp),
    "tq_scf_add": _sig(vp, vp, vp, i64),
    "tq_scf_add_dev": _sig(vp, vp, vp, i64, vp),
    "tq_scf_shape": _sig(vp, P(i64), P(i64), P(i64)),
    "tq_scf_read": _sig(vp, vp, vp, P(i64)),
    # -- taxon counts per block of sites, neighbour joining
    "tq_taxon_counts": _sig(vp, vp, i64, vp),
    "tq_taxon_counts_dev": _sig(vp, vp, i64, vp, vp),
    "tq_taxon_counts_host": _sig(vp, i64, i64, vp, i64, vp),
    "tq_taxon_counts_stats": _sig(vp, vp),
    "tq_nj_tree": _sig(vp, i64, vp, vp),
    "tq_device_info": _sig(vp, P(i32), P(i32), P(i64)),
}
#: the names alone
SYMBOLS = list(PROTOTYPES)


class TetradHipError(RuntimeError):
    def __init__(self, code: int, message: str):
        self.code = code
        super().__init__(f"{ERR_NAMES.get(code, code)}: {message}")


def build(force: bool = False, verbose: bool = False) -> Path:
    """Compile the HIP library in-tree for gfx950 (hipcc cross-compiles without a GPU)."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    sources = [SRC_PATH, HEADER, *CSRC.glob("*.hpp")]
    newest_src = max(p.stat().st_mtime for p in sources)
    if not force and LIB_PATH.exists() and LIB_PATH.stat().st_mtime >= newest_src:
        return LIB_PATH
    # -Wno-inline-asm: scan.hpp's park stores set M0 (ds_write_addtid_b32) and say so in their clobber list; the
    # compiler warns that it will not preserve a reserved register across the statement (nothing else in the unit uses M0)
    cmd = [hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "-fPIC", "-shared", "-Wno-inline-asm",
           "-o", str(LIB_PATH), str(SRC_PATH)]
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    _stamp_commit()
    return LIB_PATH


def _stamp_commit() -> None:
    """Remember which commit the library was built from (bench.py quotes it; the GPU box has no .git)."""
    repo = CSRC.parents[1]
    try:
        head = subprocess.check_output(["git", "-C", str(repo), "rev-parse", "--short", "HEAD"],
                                       stderr=subprocess.DEVNULL).decode().strip()
        dirty = subprocess.check_output(["git", "-C", str(repo), "status", "--porcelain", "--untracked-files=no"],
                                        stderr=subprocess.DEVNULL).decode().strip()
        (repo / ".build_commit").write_text(head + ("+uncommitted" if dirty else "") + "\n")
    except Exception:
        pass


_lib = None
LOADED_PATH = None      # the file load() mapped (bench.py records it: an inherited TQ_LIB_PATH must show in the line)


def load() -> ctypes.CDLL:
    """Load libtetrad_hip.so and declare every prototype.  Raises if it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not LIB_PATH.exists():
        raise ImportError(
            f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc, gfx950).  tetrad_amd has no CPU fallback.")
    # One HIP runtime per process: PyTorch-ROCm ships its own libamdhip64.so.7 and must be the
    # first to load it, otherwise torch.cuda (device buffers, streams, RCCL) finds no GPU.
    try:
        import torch  # noqa: F401
    except ImportError:  # torch is plumbing, not a requirement of the host-buffer API
        pass
    # developer knob for A/B runs of alternative builds of the same source (tools/ab/*.so): never a fallback --
    # a path that does not exist fails exactly like a missing library
    alt = os.environ.get("TQ_LIB_PATH")
    if alt:
        print(f"tetrad_amd: TQ_LIB_PATH is set -- loading {alt} instead of {LIB_PATH}", file=sys.stderr)
    global LOADED_PATH
    LOADED_PATH = alt if alt else str(LIB_PATH)
    lib = ctypes.CDLL(LOADED_PATH)
    for name, (argtypes, restype) in PROTOTYPES.items():
        fn = getattr(lib, name)
        fn.argtypes, fn.restype = argtypes, restype
    _lib = lib
    return lib

"""ctypes binding of libtetrad_hip.so (the C ABI declared in include/tetrad_hip.h).

There is no CPU fallback: if the HIP library is missing or cannot be loaded the
import-time helper raises, and every compute entry point raises TetradHipError
on a non-zero return code (message from tq_last_error).
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

#: every symbol include/tetrad_hip.h declares (checked by tests/test_cabi_symbols.py)
SYMBOLS = [
    "tq_create", "tq_destroy", "tq_last_error", "tq_set_data", "tq_resolve",
    "tq_set_source", "tq_bootstrap", "tq_bootstrap_async", "tq_sample_quartets_dev", "tq_get_data", "tq_data_shape",
    "tq_host_alloc", "tq_host_free", "tq_resolve_to_host", "tq_scan_dev", "tq_svd_dev",
    "tq_resolve_dev", "tq_resolve_range_dev", "tq_unrank_dev", "tq_resolve_debug",
    "tq_timing_enable", "tq_timing_read", "tq_timing_read_split", "tq_timing_read_kernels",
    "tq_set_option", "tq_device_info", "tq_debug_fetch", "tq_scan_plan", "tq_debug_bdsqr",
    "tq_format_tsv", "tq_format_qmc", "tq_qmc_tree", "tq_qmc_splits", "tq_unrank", "tq_numpy_choice_tail",
    "tq_conc_create", "tq_conc_destroy", "tq_conc_reset", "tq_conc_add", "tq_conc_add_dev", "tq_conc_shape", "tq_conc_read",
    "tq_stree_create", "tq_stree_destroy", "tq_stree_reset", "tq_stree_add", "tq_stree_add_dev", "tq_stree_graph",
    "tq_stree_rows", "tq_stree_build", "tq_stree_level_stats", "tq_stree_set_search", "tq_stree_search", "tq_stree_fit",
    "tq_stree_nni_scan", "tq_stree_polish",
    "tq_cons_create", "tq_cons_destroy", "tq_cons_reset", "tq_cons_add", "tq_cons_shape", "tq_cons_read", "tq_cons_tree",
    "tq_cons_support", "tq_cons_stats",
    "tq_tbe_create", "tq_tbe_destroy", "tq_tbe_reset", "tq_tbe_add", "tq_tbe_shape", "tq_tbe_read", "tq_tbe_stats",
    "tq_rf_create", "tq_rf_destroy", "tq_rf_reset", "tq_rf_add", "tq_rf_shape", "tq_rf_read", "tq_rf_stats",
    "tq_rf_word_shared",
    "tq_qd_create", "tq_qd_destroy", "tq_qd_reset", "tq_qd_clear", "tq_qd_add", "tq_qd_score", "tq_qd_score_ranks",
    "tq_qd_shape", "tq_qd_read", "tq_qd_stats", "tq_qd_word_counts",
    "tq_set_species", "tq_resolve_species", "tq_resolve_species_dev", "tq_resolve_species_debug",
    "tq_pack_sites",
    "tq_pattern_class_table", "tq_patterns", "tq_patterns_dev", "tq_patterns_species", "tq_patterns_species_dev",
    "tq_dstat_accumulate", "tq_dstat_accumulate_dev",
    "tq_patterns_blocks", "tq_patterns_blocks_dev", "tq_dstat_jackknife", "tq_dstat_jackknife_dev",
    "tq_patterns_blocks_species", "tq_patterns_blocks_species_dev", "tq_pooled_site_classes",
    "tq_quintet_class_table", "tq_patterns_quintet_blocks", "tq_patterns_quintet_blocks_dev",
    "tq_dstat_jackknife_masks", "tq_dstat_jackknife_masks_dev",
    "tq_patterns_quintet_blocks_species", "tq_patterns_quintet_blocks_species_dev", "tq_pooled_quintet_site_classes",
    "tq_scf_create", "tq_scf_destroy", "tq_scf_reset", "tq_scf_add", "tq_scf_add_dev", "tq_scf_shape", "tq_scf_read",
]


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
    c = ctypes
    vp, i64, i32 = c.c_void_p, c.c_int64, c.c_int
    lib.tq_create.argtypes = [c.POINTER(vp), i32]
    lib.tq_create.restype = i32
    lib.tq_destroy.argtypes = [vp]
    lib.tq_destroy.restype = None
    lib.tq_last_error.argtypes = [vp]
    lib.tq_last_error.restype = c.c_char_p
    lib.tq_set_data.argtypes = [vp, vp, i64, i64, vp, i64]
    lib.tq_set_data.restype = i32
    lib.tq_set_source.argtypes = [vp, vp, i64, i64, vp, i64]
    lib.tq_set_source.restype = i32
    lib.tq_bootstrap.argtypes = [vp, vp, i64, c.c_uint64, c.c_uint64, c.POINTER(i64)]
    lib.tq_bootstrap.restype = i32
    lib.tq_bootstrap_async.argtypes = [vp, vp, i64, c.c_uint64, c.c_uint64, c.POINTER(i64), vp]
    lib.tq_bootstrap_async.restype = i32
    lib.tq_sample_quartets_dev.argtypes = [vp, c.c_uint64, i64, vp, vp, vp]
    lib.tq_sample_quartets_dev.restype = i32
    lib.tq_get_data.argtypes = [vp, vp, vp]
    lib.tq_get_data.restype = i32
    lib.tq_data_shape.argtypes = [vp, c.POINTER(i64), c.POINTER(i64)]
    lib.tq_data_shape.restype = i32
    lib.tq_resolve.argtypes = [vp, vp, i64, i32, vp, vp, vp]
    lib.tq_resolve.restype = i32
    lib.tq_host_alloc.argtypes = [i64, c.POINTER(vp)]
    lib.tq_host_alloc.restype = i32
    lib.tq_host_free.argtypes = [vp]
    lib.tq_host_free.restype = i32
    lib.tq_resolve_to_host.argtypes = [vp, vp, i64, i32, vp, vp, vp]
    lib.tq_resolve_to_host.restype = i32
    lib.tq_scan_dev.argtypes = [vp, vp, i64, i32, vp]
    lib.tq_scan_dev.restype = i32
    lib.tq_svd_dev.argtypes = [vp, i64, i64, vp, vp, vp, vp]
    lib.tq_svd_dev.restype = i32
    lib.tq_timing_read_kernels.argtypes = [vp, c.POINTER(c.c_double), i32, c.POINTER(i64)]
    lib.tq_timing_read_kernels.restype = i32
    lib.tq_resolve_dev.argtypes = [vp, vp, i64, i32, vp, vp, vp, vp]
    lib.tq_resolve_dev.restype = i32
    lib.tq_resolve_range_dev.argtypes = [vp, c.c_uint64, i64, i32, vp, vp, vp, vp, vp]
    lib.tq_resolve_range_dev.restype = i32
    lib.tq_unrank_dev.argtypes = [vp, vp, i64, vp, vp]
    lib.tq_unrank_dev.restype = i32
    lib.tq_resolve_debug.argtypes = [vp, vp, i64, i32, vp, vp, vp, vp, vp, vp]
    lib.tq_resolve_debug.restype = i32
    lib.tq_timing_enable.argtypes = [vp, i32]
    lib.tq_timing_enable.restype = i32
    lib.tq_timing_read.argtypes = [vp, c.POINTER(c.c_double), c.POINTER(i64)]
    lib.tq_timing_read.restype = i32
    lib.tq_timing_read_split.argtypes = [vp, c.POINTER(c.c_double), c.POINTER(c.c_double),
                                         c.POINTER(c.c_double), c.POINTER(i64)]
    lib.tq_timing_read_split.restype = i32
    lib.tq_debug_fetch.argtypes = [vp, i32, vp, i64]
    lib.tq_debug_fetch.restype = i32
    lib.tq_scan_plan.argtypes = [vp, i64, vp, c.POINTER(i64)]
    lib.tq_scan_plan.restype = i32
    lib.tq_debug_bdsqr.argtypes = [vp, vp, i64, vp, vp, i32, c.POINTER(c.c_double)]
    lib.tq_debug_bdsqr.restype = i32
    lib.tq_set_option.argtypes = [vp, c.c_char_p, i64]
    lib.tq_set_option.restype = i32
    lib.tq_format_tsv.argtypes = [vp, vp, vp, i64, vp, i64, c.POINTER(i64)]
    lib.tq_format_tsv.restype = i32
    lib.tq_format_qmc.argtypes = [vp, vp, vp, i64, i32, i64, c.c_double, vp, i64, c.POINTER(i64), c.POINTER(i64)]
    lib.tq_format_qmc.restype = i32
    lib.tq_qmc_splits.argtypes = [vp, vp, vp, i64, i32, i64, c.c_double, vp, vp, c.POINTER(i64)]
    lib.tq_qmc_splits.restype = i32
    lib.tq_numpy_choice_tail.argtypes = [vp, c.c_uint64, i64, vp]
    lib.tq_numpy_choice_tail.restype = i32
    lib.tq_unrank.argtypes = [vp, c.c_uint64, i64, i64, vp]
    lib.tq_unrank.restype = i32
    lib.tq_qmc_tree.argtypes = [vp, vp, i64, i64, c.c_uint64, vp, i64, c.POINTER(i64)]
    lib.tq_qmc_tree.restype = i32
    lib.tq_conc_create.argtypes = [c.POINTER(vp), vp, i64, i64, i64, c.c_double, vp]
    lib.tq_conc_create.restype = i32
    lib.tq_conc_destroy.argtypes = [vp]
    lib.tq_conc_destroy.restype = None
    lib.tq_conc_reset.argtypes = [vp]
    lib.tq_conc_reset.restype = i32
    lib.tq_conc_add.argtypes = [vp, vp, vp, vp, vp, i64]
    lib.tq_conc_add.restype = i32
    lib.tq_conc_add_dev.argtypes = [vp, vp, vp, vp, vp, i64, vp]
    lib.tq_conc_add_dev.restype = i32
    lib.tq_conc_shape.argtypes = [vp, c.POINTER(i64), c.POINTER(i64), c.POINTER(i64)]
    lib.tq_conc_shape.restype = i32
    lib.tq_conc_read.argtypes = [vp, vp, vp, vp, vp, c.POINTER(i64)]
    lib.tq_conc_read.restype = i32
    lib.tq_stree_create.argtypes = [c.POINTER(vp), i64, i64, i32, i64, c.c_double, vp]
    lib.tq_stree_create.restype = i32
    lib.tq_stree_destroy.argtypes = [vp]
    lib.tq_stree_destroy.restype = None
    lib.tq_stree_reset.argtypes = [vp]
    lib.tq_stree_reset.restype = i32
    lib.tq_stree_add.argtypes = [vp, vp, vp, vp, vp, i64]
    lib.tq_stree_add.restype = i32
    lib.tq_stree_add_dev.argtypes = [vp, vp, vp, vp, vp, i64, vp]
    lib.tq_stree_add_dev.restype = i32
    lib.tq_stree_graph.argtypes = [vp, vp, vp, c.POINTER(i64), c.POINTER(i64), c.POINTER(c.c_uint64)]
    lib.tq_stree_graph.restype = i32
    lib.tq_stree_rows.argtypes = [vp, vp, vp, c.POINTER(i64)]
    lib.tq_stree_rows.restype = i32
    lib.tq_stree_build.argtypes = [vp, c.c_uint64, vp, vp, i64, c.POINTER(i64), c.POINTER(i64)]
    lib.tq_stree_build.restype = i32
    lib.tq_stree_level_stats.argtypes = [vp, c.POINTER(i64), vp]
    lib.tq_stree_level_stats.restype = i32
    lib.tq_stree_set_search.argtypes = [vp, i32]
    lib.tq_stree_set_search.restype = i32
    lib.tq_stree_search.argtypes = [vp, i64, vp, vp, vp, vp, vp, vp, vp]
    lib.tq_stree_search.restype = i32
    lib.tq_stree_fit.argtypes = [vp, vp, vp, i64, i64, vp, vp]
    lib.tq_stree_fit.restype = i32
    lib.tq_stree_nni_scan.argtypes = [vp, vp, i64, vp, c.POINTER(i64), vp, vp, vp]
    lib.tq_stree_nni_scan.restype = i32
    lib.tq_stree_polish.argtypes = [vp, vp, i64, i64, vp, vp, i64, c.POINTER(i64), vp, c.POINTER(i64), c.POINTER(i32)]
    lib.tq_stree_polish.restype = i32
    lib.tq_cons_create.argtypes = [c.POINTER(vp), i64, i64, vp]
    lib.tq_cons_create.restype = i32
    lib.tq_cons_destroy.argtypes = [vp]
    lib.tq_cons_destroy.restype = None
    lib.tq_cons_reset.argtypes = [vp]
    lib.tq_cons_reset.restype = i32
    lib.tq_cons_add.argtypes = [vp, vp, vp, i64, i64, vp]
    lib.tq_cons_add.restype = i32
    lib.tq_cons_shape.argtypes = [vp, c.POINTER(i64), c.POINTER(i64), c.POINTER(i64), c.POINTER(i64)]
    lib.tq_cons_shape.restype = i32
    lib.tq_cons_read.argtypes = [vp, vp, vp]
    lib.tq_cons_read.restype = i32
    lib.tq_cons_tree.argtypes = [vp, i64, vp, i64, c.POINTER(i64)]
    lib.tq_cons_tree.restype = i32
    lib.tq_cons_support.argtypes = [vp, vp, i64, vp, vp, c.POINTER(i64)]
    lib.tq_cons_support.restype = i32
    lib.tq_cons_stats.argtypes = [vp, vp]
    lib.tq_cons_stats.restype = i32
    lib.tq_tbe_create.argtypes = [c.POINTER(vp), i64, vp, i64, vp]
    lib.tq_tbe_create.restype = i32
    lib.tq_tbe_destroy.argtypes = [vp]
    lib.tq_tbe_destroy.restype = None
    lib.tq_tbe_reset.argtypes = [vp]
    lib.tq_tbe_reset.restype = i32
    lib.tq_tbe_add.argtypes = [vp, vp, vp, i64, i64, vp, vp]
    lib.tq_tbe_add.restype = i32
    lib.tq_tbe_shape.argtypes = [vp, c.POINTER(i64), c.POINTER(i64), c.POINTER(i64), c.POINTER(i64)]
    lib.tq_tbe_shape.restype = i32
    lib.tq_tbe_read.argtypes = [vp, vp, vp, vp]
    lib.tq_tbe_read.restype = i32
    lib.tq_tbe_stats.argtypes = [vp, vp]
    lib.tq_tbe_stats.restype = i32
    lib.tq_rf_create.argtypes = [c.POINTER(vp), i64, i64, i64, vp]
    lib.tq_rf_create.restype = i32
    lib.tq_rf_destroy.argtypes = [vp]
    lib.tq_rf_destroy.restype = None
    lib.tq_rf_reset.argtypes = [vp]
    lib.tq_rf_reset.restype = i32
    lib.tq_rf_add.argtypes = [vp, vp, vp, i64, i64, vp]
    lib.tq_rf_add.restype = i32
    lib.tq_rf_shape.argtypes = [vp, c.POINTER(i64), c.POINTER(i64), c.POINTER(i64), c.POINTER(i64), c.POINTER(i64)]
    lib.tq_rf_shape.restype = i32
    lib.tq_rf_read.argtypes = [vp, vp, vp, vp]
    lib.tq_rf_read.restype = i32
    lib.tq_rf_stats.argtypes = [vp, vp]
    lib.tq_rf_stats.restype = i32
    lib.tq_rf_word_shared.argtypes = [c.c_uint64, c.c_uint64]
    lib.tq_rf_word_shared.restype = c.c_uint32
    lib.tq_qd_create.argtypes = [c.POINTER(vp), i64, i64, vp]
    lib.tq_qd_create.restype = i32
    lib.tq_qd_destroy.argtypes = [vp]
    lib.tq_qd_destroy.restype = None
    lib.tq_qd_reset.argtypes = [vp]
    lib.tq_qd_reset.restype = i32
    lib.tq_qd_clear.argtypes = [vp]
    lib.tq_qd_clear.restype = i32
    lib.tq_qd_add.argtypes = [vp, vp, vp, i64, i64, vp]
    lib.tq_qd_add.restype = i32
    lib.tq_qd_score.argtypes = [vp, vp, i64, vp]
    lib.tq_qd_score.restype = i32
    lib.tq_qd_score_ranks.argtypes = [vp, vp, c.c_uint64, i64, vp]
    lib.tq_qd_score_ranks.restype = i32
    lib.tq_qd_shape.argtypes = [vp, c.POINTER(i64), c.POINTER(i64), c.POINTER(c.c_uint64)]
    lib.tq_qd_shape.restype = i32
    lib.tq_qd_read.argtypes = [vp, vp, vp]
    lib.tq_qd_read.restype = i32
    lib.tq_qd_stats.argtypes = [vp, vp]
    lib.tq_qd_stats.restype = i32
    lib.tq_qd_word_counts.argtypes = [c.c_uint64] * 6 + [c.POINTER(c.c_uint32), c.POINTER(c.c_uint32)]
    lib.tq_qd_word_counts.restype = None
    lib.tq_set_species.argtypes = [vp, vp, i64, i64]
    lib.tq_set_species.restype = i32
    lib.tq_resolve_species.argtypes = [vp, vp, i64, vp, vp, vp]
    lib.tq_resolve_species.restype = i32
    lib.tq_resolve_species_dev.argtypes = [vp, vp, i64, vp, vp, vp, vp]
    lib.tq_resolve_species_dev.restype = i32
    lib.tq_resolve_species_debug.argtypes = [vp, vp, i64, vp, vp, vp, vp, vp, vp]
    lib.tq_resolve_species_debug.restype = i32
    lib.tq_pack_sites.argtypes = [vp, i64, i64, vp, i64, vp, i64, c.POINTER(i64), c.POINTER(c.c_int32), vp]
    lib.tq_pack_sites.restype = i32
    lib.tq_pattern_class_table.argtypes = [vp]
    lib.tq_pattern_class_table.restype = i32
    lib.tq_patterns.argtypes = [vp, vp, i64, i32, vp]
    lib.tq_patterns.restype = i32
    lib.tq_patterns_dev.argtypes = [vp, vp, i64, i32, vp, vp]
    lib.tq_patterns_dev.restype = i32
    lib.tq_patterns_species.argtypes = [vp, vp, i64, vp]
    lib.tq_patterns_species.restype = i32
    lib.tq_patterns_species_dev.argtypes = [vp, vp, i64, vp, vp]
    lib.tq_patterns_species_dev.restype = i32
    lib.tq_dstat_accumulate.argtypes = [vp, i64, vp, vp, vp, i64, vp]
    lib.tq_dstat_accumulate.restype = i32
    lib.tq_dstat_accumulate_dev.argtypes = [vp, vp, i64, vp, vp, vp, i64, vp, vp]
    lib.tq_dstat_accumulate_dev.restype = i32
    lib.tq_patterns_blocks.argtypes = [vp, vp, i64, vp, i64, vp]
    lib.tq_patterns_blocks.restype = i32
    lib.tq_patterns_blocks_dev.argtypes = [vp, vp, i64, vp, i64, vp, vp]
    lib.tq_patterns_blocks_dev.restype = i32
    lib.tq_dstat_jackknife.argtypes = [vp, i64, i64, vp, vp, vp, i64, vp]
    lib.tq_dstat_jackknife.restype = i32
    lib.tq_dstat_jackknife_dev.argtypes = [vp, vp, i64, i64, vp, vp, vp, i64, vp, vp]
    lib.tq_dstat_jackknife_dev.restype = i32
    lib.tq_patterns_blocks_species.argtypes = [vp, vp, i64, vp, i64, vp]
    lib.tq_patterns_blocks_species.restype = i32
    lib.tq_patterns_blocks_species_dev.argtypes = [vp, vp, i64, vp, i64, vp, vp]
    lib.tq_patterns_blocks_species_dev.restype = i32
    lib.tq_pooled_site_classes.argtypes = [vp, vp]
    lib.tq_pooled_site_classes.restype = i32
    lib.tq_quintet_class_table.argtypes = [vp]
    lib.tq_quintet_class_table.restype = i32
    lib.tq_patterns_quintet_blocks.argtypes = [vp, vp, i64, vp, i64, vp]
    lib.tq_patterns_quintet_blocks.restype = i32
    lib.tq_patterns_quintet_blocks_dev.argtypes = [vp, vp, i64, vp, i64, vp, vp]
    lib.tq_patterns_quintet_blocks_dev.restype = i32
    lib.tq_dstat_jackknife_masks.argtypes = [vp, i64, i64, vp, vp, vp, i64, vp]
    lib.tq_dstat_jackknife_masks.restype = i32
    lib.tq_dstat_jackknife_masks_dev.argtypes = [vp, vp, i64, i64, vp, vp, vp, i64, vp, vp]
    lib.tq_dstat_jackknife_masks_dev.restype = i32
    lib.tq_patterns_quintet_blocks_species.argtypes = [vp, vp, i64, vp, i64, vp]
    lib.tq_patterns_quintet_blocks_species.restype = i32
    lib.tq_patterns_quintet_blocks_species_dev.argtypes = [vp, vp, i64, vp, i64, vp, vp]
    lib.tq_patterns_quintet_blocks_species_dev.restype = i32
    lib.tq_pooled_quintet_site_classes.argtypes = [vp, vp]
    lib.tq_pooled_quintet_site_classes.restype = i32
    lib.tq_scf_create.argtypes = [c.POINTER(vp), vp, i64, i64, vp]
    lib.tq_scf_create.restype = i32
    lib.tq_scf_destroy.argtypes = [vp]
    lib.tq_scf_destroy.restype = None
    lib.tq_scf_reset.argtypes = [vp]
    lib.tq_scf_reset.restype = i32
    lib.tq_scf_add.argtypes = [vp, vp, vp, i64]
    lib.tq_scf_add.restype = i32
    lib.tq_scf_add_dev.argtypes = [vp, vp, vp, i64, vp]
    lib.tq_scf_add_dev.restype = i32
    lib.tq_scf_shape.argtypes = [vp, c.POINTER(i64), c.POINTER(i64), c.POINTER(i64)]
    lib.tq_scf_shape.restype = i32
    lib.tq_scf_read.argtypes = [vp, vp, vp, c.POINTER(i64)]
    lib.tq_scf_read.restype = i32
    lib.tq_device_info.argtypes = [vp, c.POINTER(c.c_int32), c.POINTER(c.c_int32), c.POINTER(i64)]
    lib.tq_device_info.restype = i32
    _lib = lib
    return lib

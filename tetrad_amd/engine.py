"""QuartetEngine: one HIP context on one GPU (thin object wrapper over the C ABI).

Holds one replicate's genotype matrix resident in HBM (`set_data`, once per
replicate) and resolves quartet chunks against it.  Mirrors the state an
ipyparallel engine has in the reference while it runs
`infer_resolved_quartets` (tetrad/src/resolve_quartets.py:17-39) -- minus the
per-chunk HDF5 re-read.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _lib
from ._handle import Handle
from ._lib import TetradHipError


def _ptr(a):
    return ctypes.c_void_p(a.ctypes.data) if a is not None else None


class _PinnedBlock:
    """One block of the library's page-locked host pool (tq_host_alloc); returned to the pool when the
    last NumPy view of it is garbage-collected."""
    __slots__ = ("ptr", "nbytes", "_free", "__weakref__")

    def __init__(self, nbytes: int):
        lib = _lib.load()
        p = ctypes.c_void_p()
        rc = lib.tq_host_alloc(int(nbytes), ctypes.byref(p))
        if rc != 0 or not p.value:
            raise TetradHipError(rc or -6, f"tq_host_alloc({nbytes}) failed")
        self.ptr, self.nbytes, self._free = p.value, int(nbytes), lib.tq_host_free

    @property
    def __array_interface__(self):
        return {"shape": (self.nbytes,), "typestr": "|u1", "data": (self.ptr, False), "version": 3}

    def __del__(self):
        try:
            self._free(ctypes.c_void_p(self.ptr))
        except Exception:  # interpreter shutdown
            pass


def pinned_empty(shape, dtype) -> np.ndarray:
    """An uninitialised NumPy array in page-locked host memory from the library's pool: the copy engine
    reads / writes it directly, asynchronously under the kernels (no staging, no extra host pass)."""
    dtype = np.dtype(dtype)
    shape = (shape,) if np.isscalar(shape) else tuple(shape)
    n = int(np.prod(shape, dtype=np.int64)) * dtype.itemsize
    raw = np.asarray(_PinnedBlock(max(n, 1)))           # .base keeps the block alive
    return raw[:n].view(dtype).reshape(shape)


def scan_plan(rows) -> tuple[np.ndarray, int]:
    """Test hook (tq_scan_plan; host code, no GPU needed): for rows i64[n, 22] of scan options and batch shape, the kernel
    the library would launch as i64[n, 12], and the number of scan instantiations it is built with.  Columns:
    include/tetrad_hip.h."""
    rows = np.ascontiguousarray(rows, dtype=np.int64).reshape(-1, 22)
    plans = np.zeros((len(rows), 12), np.int64)
    n_kernels = ctypes.c_int64()
    rc = _lib.load().tq_scan_plan(_ptr(rows), len(rows), _ptr(plans), ctypes.byref(n_kernels))
    if rc != 0:
        raise TetradHipError(rc, "tq_scan_plan failed")
    return plans, n_kernels.value


PACK_PAD = 0xFFFFFFFF


def pack_sites(tmpmap: np.ndarray, tmparr: np.ndarray | None = None):
    """The site order of the packed layout (option ``site_pack``, csrc/pack.hpp; host code, no GPU needed):
    ``src`` u32[S'] with ``src[p]`` = the site packed position p holds or PACK_PAD, S' a multiple of 2048.  With
    ``tmparr`` also what the automatic rule of ``set_data`` decides: returns (src, pays, estimate) with estimate =
    (predicted instructions per quartet natural, packed, walk trips per quartet natural, packed, relative gain in
    instructions lowered by two standard errors of the sample -- the rule takes the packed layout from 0.03 on)."""
    lib = _lib.load()
    tm = np.asarray(tmpmap)
    stride = tm.shape[1] if tm.ndim == 2 else 1
    tm = np.ascontiguousarray(tm, dtype=np.uint32)
    S = tm.shape[0]
    arr = None
    if tmparr is not None:
        arr = np.ascontiguousarray(tmparr, dtype=np.uint8)
        if arr.ndim != 2 or arr.shape[1] != S:
            raise ValueError("tmparr must be [ntaxa, nsites] with one column per tmpmap row")
    T = arr.shape[0] if arr is not None else 0
    n = ctypes.c_int64()
    pays = ctypes.c_int32(-1)
    est = np.zeros(5, np.float64)

    def call(src, cap):
        rc = lib.tq_pack_sites(_ptr(arr), T, S, _ptr(tm), stride, _ptr(src), cap, ctypes.byref(n), ctypes.byref(pays),
                               _ptr(est))
        if rc != 0:
            raise TetradHipError(rc, "tq_pack_sites failed")

    call(None, 0)
    src = np.empty(n.value, np.uint32)
    call(src, src.shape[0])
    if arr is None:
        return src
    return src, bool(pays.value), tuple(est.tolist())


class QuartetEngine(Handle):
    _prefix = "tq"

    def __init__(self, device_id: int = 0):
        self._create(int(device_id))
        self.device_id = int(device_id)
        self.T = self.S = 0
        #: bumped whenever the resident replicate is replaced (set_data / bootstrap); lets the API
        #: mirrors notice that what they uploaded is no longer what the device holds
        self.data_generation = 0

    def _ctx(self):
        return self._h                  # the engine's errors are in its own context (NULL while it is being created)

    # -- data --------------------------------------------------------------
    def set_data(self, tmparr: np.ndarray, tmpmap: np.ndarray):
        """tmparr u8[T,S]; tmpmap u32[S,2] (column 0 used) or a 1-D locus column."""
        tmparr = np.ascontiguousarray(tmparr, dtype=np.uint8)
        if tmparr.ndim != 2:
            raise ValueError("tmparr must be 2-D [ntaxa, nsites]")
        tmpmap = np.asarray(tmpmap)
        if tmpmap.ndim == 2:
            tm = np.ascontiguousarray(tmpmap, dtype=np.uint32)
            stride = tm.shape[1]
        else:
            tm = np.ascontiguousarray(tmpmap, dtype=np.uint32)
            stride = 1
        if tm.shape[0] != tmparr.shape[1]:
            raise ValueError("tmpmap rows must equal tmparr columns")
        T, S = tmparr.shape
        self.data_generation += 1
        self._check(self._lib.tq_set_data(self._h, _ptr(tmparr), T, S, _ptr(tm), stride))
        self.T, self.S = T, S

    # -- bootstrap replicates on the device -------------------------------------
    def set_source(self, seqarr: np.ndarray, spans: np.ndarray):
        """seqarr u8[T,S0] (ASCII, IUPAC codes allowed); spans i64[nloci,2] ([start,end) per locus)."""
        seqarr = np.ascontiguousarray(seqarr, dtype=np.uint8)
        spans = np.ascontiguousarray(spans, dtype=np.int64).reshape(-1, 2)
        T, S0 = seqarr.shape
        self._check(self._lib.tq_set_source(self._h, _ptr(seqarr), T, S0, _ptr(spans), spans.shape[0]))
        self.nloci = spans.shape[0]

    def bootstrap(self, lidxs: np.ndarray, seed_shuffle: int, seed_ambig: int, stream: int | None = None) -> int:
        """Build the replicate for resampled loci `lidxs` on the device; returns its number of sites.
        With `stream` (a hipStream_t address, 0 = default stream) the call only enqueues."""
        lidxs = np.ascontiguousarray(lidxs, dtype=np.int64)
        S = ctypes.c_int64()
        self.data_generation += 1
        if stream is None:
            self._check(self._lib.tq_bootstrap(self._h, _ptr(lidxs), lidxs.shape[0], int(seed_shuffle),
                                               int(seed_ambig), ctypes.byref(S)))
        else:
            self._check(self._lib.tq_bootstrap_async(self._h, _ptr(lidxs), lidxs.shape[0], int(seed_shuffle),
                                                     int(seed_ambig), ctypes.byref(S), stream or None))
        T = ctypes.c_int64()
        self._check(self._lib.tq_data_shape(self._h, ctypes.byref(T), None))
        self.T, self.S = T.value, S.value
        return S.value

    def get_data(self):
        """Resident replicate in the reference layout: (tmparr u8[T,S] 0..3/78, tmpmap u32[S,2])."""
        T, S = ctypes.c_int64(), ctypes.c_int64()
        self._check(self._lib.tq_data_shape(self._h, ctypes.byref(T), ctypes.byref(S)))
        tmparr = np.zeros((T.value, S.value), np.uint8)
        tmpmap = np.zeros((S.value, 2), np.uint32)
        self._check(self._lib.tq_get_data(self._h, _ptr(tmparr), _ptr(tmpmap)))
        return tmparr, tmpmap

    def set_option(self, name: str, value: int) -> int:
        self._check(self._lib.tq_set_option(self._h, name.encode(), int(value)))
        return int(value)

    # -- host-buffer API -----------------------------------------------------
    def resolve(self, quartets: np.ndarray, subsample_snps: bool = True, debug: bool = False):
        """Returns (rstat u32[Q,2], rscor f64[Q,3], flags u8[Q]) and, with ``debug``,
        a dict with cmats u32[Q,3,16,16], svds f64[Q,3,16], ranks i32[Q,3].
        The result arrays live in page-locked memory of the library's pool (ordinary NumPy arrays to the
        caller), so the result D2H runs under the kernels."""
        q = quartets
        if not (isinstance(q, np.ndarray) and q.dtype == np.uint32 and q.flags.c_contiguous):
            src = np.asarray(quartets)
            q = pinned_empty((src.size // 4, 4), np.uint32)      # the conversion copy lands in pinned memory
            q[...] = src.reshape(-1, 4)
        q = q.reshape(-1, 4)
        Q = q.shape[0]
        rstat = pinned_empty((Q, 2), np.uint32)
        rscor = pinned_empty((Q, 3), np.float64)
        flags = pinned_empty(Q, np.uint8)
        if debug:
            cm = np.zeros((Q, 3, 16, 16), np.uint32)
            sv = np.zeros((Q, 3, 16), np.float64)
            rk = np.zeros((Q, 3), np.int32)
            self._check(self._lib.tq_resolve_debug(
                self._h, _ptr(q), Q, int(bool(subsample_snps)), _ptr(rstat), _ptr(rscor),
                _ptr(flags), _ptr(cm), _ptr(sv), _ptr(rk)))
            return rstat, rscor, flags, dict(cmats=cm, svds=sv, ranks=rk)
        self._check(self._lib.tq_resolve(
            self._h, _ptr(q), Q, int(bool(subsample_snps)), _ptr(rstat), _ptr(rscor), _ptr(flags)))
        return rstat, rscor, flags

    def resolve_to_host(self, d_quartets: int, Q: int, subsample_snps: bool = True, out=None):
        """Quartets on the device (address), results to host arrays: (rstat, rscor, flags).  ``out`` may
        hold the three arrays to fill (any NumPy arrays of the right shape; pinned ones are written by the
        copy engine directly)."""
        if out is None:
            out = (pinned_empty((Q, 2), np.uint32), pinned_empty((Q, 3), np.float64), pinned_empty(Q, np.uint8))
        rstat, rscor, flags = out
        self._check(self._lib.tq_resolve_to_host(
            self._h, d_quartets, Q, int(bool(subsample_snps)), _ptr(rstat), _ptr(rscor), _ptr(flags)))
        return rstat, rscor, flags

    # -- species-tree mode ------------------------------------------
    def set_species(self, species_of, K: int | None = None):
        """species_of i32[T]: species id in [0, K) per sample, -1 = left out; K defaults to max id + 1."""
        sp = np.ascontiguousarray(species_of, dtype=np.int32).reshape(-1)
        if K is None:
            K = int(sp.max()) + 1 if sp.size else 0
        self._check(self._lib.tq_set_species(self._h, _ptr(sp), sp.shape[0], int(K)))

    def resolve_species(self, squartets: np.ndarray, debug: bool = False):
        """Species quartets u32[Q,4] resolved from pooled lineages (full mode): (rstat, rscor, flags) as `resolve`,
        and with ``debug`` a dict with the pooled cmats u32[Q,3,16,16], svds f64[Q,3,16], ranks i32[Q,3]."""
        q = squartets
        if not (isinstance(q, np.ndarray) and q.dtype == np.uint32 and q.flags.c_contiguous):
            src = np.asarray(squartets)
            q = pinned_empty((src.size // 4, 4), np.uint32)
            q[...] = src.reshape(-1, 4)
        q = q.reshape(-1, 4)
        Q = q.shape[0]
        rstat = pinned_empty((Q, 2), np.uint32)
        rscor = pinned_empty((Q, 3), np.float64)
        flags = pinned_empty(Q, np.uint8)
        if debug:
            cm = np.zeros((Q, 3, 16, 16), np.uint32)
            sv = np.zeros((Q, 3, 16), np.float64)
            rk = np.zeros((Q, 3), np.int32)
            self._check(self._lib.tq_resolve_species_debug(self._h, _ptr(q), Q, _ptr(rstat), _ptr(rscor), _ptr(flags),
                                                           _ptr(cm), _ptr(sv), _ptr(rk)))
            return rstat, rscor, flags, dict(cmats=cm, svds=sv, ranks=rk)
        self._check(self._lib.tq_resolve_species(self._h, _ptr(q), Q, _ptr(rstat), _ptr(rscor), _ptr(flags)))
        return rstat, rscor, flags

    def resolve_species_dev(self, d_squartets: int, Q: int, d_rstat: int, d_rscor: int, d_flags: int = 0,
                            stream: int = 0):
        """Species quartets on the device, results to device arrays, enqueued on `stream`."""
        self._check(self._lib.tq_resolve_species_dev(self._h, d_squartets, Q, d_rstat, d_rscor, d_flags or None,
                                                     stream or None))

    # -- site-pattern classes and D tests (tetrad_amd/patterns.py) ----
    @staticmethod
    def _sets(sets) -> np.ndarray:
        s = np.asarray(sets)
        if s.size and (s.min() < 0 or s.max() > 0xFFFFFFFF):
            raise ValueError("set indices must fit an unsigned 32-bit integer")
        return np.ascontiguousarray(s, dtype=np.uint32).reshape(-1, 4)

    def patterns(self, sets, subsample_snps: bool = True) -> np.ndarray:
        """Class rows u32[Q,16] of strictly ascending quartets `sets` [Q,4]: the 15 site-pattern class counts
        (patterns.CLASS_STRINGS) and their sum, the number of counted sites."""
        s = self._sets(sets)
        classes = np.zeros((s.shape[0], 16), np.uint32)
        self._check(self._lib.tq_patterns(self._h, _ptr(s), s.shape[0], int(bool(subsample_snps)), _ptr(classes)))
        return classes

    def patterns_dev(self, d_sets: int, Q: int, subsample_snps: bool, d_classes: int, stream: int = 0):
        """The same with device pointers (u32[Q,4] in, u32[Q,16] out), enqueued on `stream`; the rows are the
        caller's responsibility."""
        self._check(self._lib.tq_patterns_dev(self._h, d_sets, Q, int(bool(subsample_snps)), d_classes, stream or None))

    def patterns_species(self, ssets) -> np.ndarray:
        """Class rows u32[Q,16] of strictly ascending SPECIES quartets: the counts of the pooled lineage combinations."""
        s = self._sets(ssets)
        classes = np.zeros((s.shape[0], 16), np.uint32)
        self._check(self._lib.tq_patterns_species(self._h, _ptr(s), s.shape[0], _ptr(classes)))
        return classes

    def patterns_species_dev(self, d_ssets: int, Q: int, d_classes: int, stream: int = 0):
        self._check(self._lib.tq_patterns_species_dev(self._h, d_ssets, Q, d_classes, stream or None))

    def dstat_accumulate_dev(self, d_classes: int, n_sets: int, d_set_of: int, d_ia: int, d_ib: int, N: int, d_acc: int,
                             stream: int = 0):
        """One replicate of N D tests added to d_acc f64[N,4] = {n, sum, sum of squares, last} on `stream`: test t reads
        ABBA at d_classes[d_set_of[t]][d_ia[t]] and BABA at [d_ib[t]] (u32 / u8 / u8 arrays on the device)."""
        self._check(self._lib.tq_dstat_accumulate_dev(self._h, d_classes, n_sets, d_set_of, d_ia, d_ib, N, d_acc,
                                                      stream or None))

    # -- class rows per block of sites and the block jackknife ----
    @staticmethod
    def _block_starts(block_starts) -> np.ndarray:
        b = np.ascontiguousarray(block_starts, dtype=np.int64).reshape(-1)
        if b.shape[0] < 2:
            raise ValueError("block_starts must hold B + 1 >= 2 boundaries")
        return b

    def _blocks_host(self, entry, s: np.ndarray, block_starts) -> np.ndarray:
        b = self._block_starts(block_starts)
        B = b.shape[0] - 1
        classes = np.zeros((s.shape[0], B, 16), np.uint32)
        self._check(entry(self._h, _ptr(s), s.shape[0], _ptr(b), B, _ptr(classes)))
        return classes

    def _blocks_dev(self, entry, d_sets: int, Q: int, block_starts, d_classes: int, stream: int):
        b = self._block_starts(block_starts)
        self._check(entry(self._h, d_sets, Q, _ptr(b), b.shape[0] - 1, d_classes, stream or None))

    def patterns_blocks(self, sets, block_starts) -> np.ndarray:
        """Block rows u32[Q,B,16] of strictly ascending quartets `sets` [Q,4], full mode: block j holds the class
        counts (and their sum) of sites [block_starts[j], block_starts[j+1]) of the resident replicate."""
        return self._blocks_host(self._lib.tq_patterns_blocks, self._sets(sets), block_starts)

    def patterns_blocks_dev(self, d_sets: int, Q: int, block_starts, d_classes: int, stream: int = 0):
        """The same with device pointers (u32[Q,4] in, u32[Q,B,16] out), enqueued on `stream`; `block_starts` is a host
        array, read before the call returns.  The rows are the caller's responsibility."""
        self._blocks_dev(self._lib.tq_patterns_blocks_dev, d_sets, Q, block_starts, d_classes, stream)

    def patterns_blocks_species(self, ssets, block_starts) -> np.ndarray:
        """Block rows u32[Q,B,16] of strictly ascending SPECIES quartets: per block the pooled
        class counts of the lineage combinations, class 0 always 0, slot 15 the sum.  Needs `set_species`."""
        return self._blocks_host(self._lib.tq_patterns_blocks_species, self._sets(ssets), block_starts)

    def patterns_blocks_species_dev(self, d_ssets: int, Q: int, block_starts, d_classes: int, stream: int = 0):
        """The same with device pointers (u32[Q,4] in, u32[Q,B,16] out), enqueued on `stream`; `block_starts` is a host
        array, read before the call returns.  The rows are the caller's responsibility (an id >= K gives zeros)."""
        self._blocks_dev(self._lib.tq_patterns_blocks_species_dev, d_ssets, Q, block_starts, d_classes, stream)

    def dstat_jackknife_dev(self, d_bclasses: int, n_sets: int, B: int, d_set_of: int, d_ia: int, d_ib: int, N: int,
                            d_out: int, stream: int = 0):
        """The delete-one-block jackknife of N D tests on `stream`: test t reads ABBA at d_bclasses[d_set_of[t]][j][d_ia[t]]
        and BABA at [d_ib[t]] of every block j and overwrites d_out f64[N,4] = {blocks used, D, jackknife D, variance}."""
        self._check(self._lib.tq_dstat_jackknife_dev(self._h, d_bclasses, n_sets, B, d_set_of, d_ia, d_ib, N, d_out,
                                                     stream or None))

    # -- five-taxon class rows per block and the jackknife on sums of slots ----
    @staticmethod
    def _sets5(sets5) -> np.ndarray:
        s = np.ascontiguousarray(sets5, dtype=np.uint32)
        if s.ndim != 2 or s.shape[1] != 5:
            raise ValueError("sets5 must be [Q, 5]")
        return s

    def patterns_quintet_blocks(self, sets5, block_starts) -> np.ndarray:
        """Block rows u32[Q,B,16] of strictly ascending five-taxon sets `sets5` [Q,5], full mode: slot k = 1..15 of
        block j counts the sites of [block_starts[j], block_starts[j+1]) with no missing base, exactly two distinct
        bases and class k = sum of [x_i != x_0] 2^(i-1); slot 0 is their sum."""
        return self._blocks_host(self._lib.tq_patterns_quintet_blocks, self._sets5(sets5), block_starts)

    def patterns_quintet_blocks_dev(self, d_sets5: int, Q: int, block_starts, d_classes: int, stream: int = 0):
        """The same with device pointers (u32[Q,5] in, 4-byte aligned; u32[Q,B,16] out, 16-byte aligned), enqueued on
        `stream`; `block_starts` is a host array, read before the call returns.  The rows are the caller's
        responsibility (an index >= T gives zeros)."""
        self._blocks_dev(self._lib.tq_patterns_quintet_blocks_dev, d_sets5, Q, block_starts, d_classes, stream)

    def dstat_jackknife_masks_dev(self, d_bclasses: int, n_sets: int, B: int, d_set_of: int, d_lmask: int, d_rmask: int,
                                  N: int, d_out: int, stream: int = 0):
        """The delete-one-block jackknife of N tests on `stream`: test t reads, of every block row j of set d_set_of[t],
        a_j = the sum of the slots set in d_lmask[t] and b_j = that of d_rmask[t] (u16 arrays) and overwrites d_out
        f64[N,4] = {blocks used, D, jackknife D, variance}.  An invalid test is skipped."""
        self._check(self._lib.tq_dstat_jackknife_masks_dev(self._h, d_bclasses, n_sets, B, d_set_of, d_lmask, d_rmask, N,
                                                           d_out, stream or None))

    # -- pooled five-taxon class rows of species sets per block ----
    def patterns_quintet_blocks_species(self, ssets5, block_starts) -> np.ndarray:
        """Block rows u32[Q,B,16] of strictly ascending five-SPECIES sets `ssets5` [Q,5]: slot k = 1..15 of block j counts
        the lineage quintets (one lineage per species) that show class k at a site of [block_starts[j], block_starts[j+1]),
        summed over its sites; slot 0 is their sum.  Needs `set_species`."""
        return self._blocks_host(self._lib.tq_patterns_quintet_blocks_species, self._sets5(ssets5), block_starts)

    def patterns_quintet_blocks_species_dev(self, d_ssets5: int, Q: int, block_starts, d_classes: int, stream: int = 0):
        """The same with device pointers (u32[Q,5] in, 4-byte aligned; u32[Q,B,16] out, 16-byte aligned), enqueued on
        `stream`; `block_starts` is a host array, read before the call returns.  The rows are the caller's
        responsibility (an id >= K gives zeros)."""
        self._blocks_dev(self._lib.tq_patterns_quintet_blocks_species_dev, d_ssets5, Q, block_starts, d_classes, stream)

    # -- all-pairs taxon counts per block of sites (tetrad_amd/distance.py) ----
    def taxon_counts(self, block_starts=None) -> np.ndarray:
        """Pair rows u32[B,T,T,4] = (both, diff, ts, tv) of the resident replicate, full mode: the sites of block j present
        in both taxa, of those the differing ones, of those the transitions, and the transversions.  `block_starts` None
        means one block [0, S)."""
        from .distance import block_starts_of
        b = block_starts_of(block_starts, self.S)
        B = b.shape[0] - 1
        out = np.zeros((B, self.T, self.T, 4), np.uint32)
        self._check(self._lib.tq_taxon_counts(self._h, _ptr(b), B, _ptr(out)))
        return out

    def taxon_counts_dev(self, block_starts, d_out: int, stream: int = 0):
        """The same into a device pointer (u32[B,T,T,4], 16-byte aligned), enqueued on `stream`; `block_starts` is a host
        array (None: one block), read before the call returns."""
        from .distance import block_starts_of
        b = block_starts_of(block_starts, self.S)
        self._check(self._lib.tq_taxon_counts_dev(self._h, _ptr(b), b.shape[0] - 1, d_out, stream or None))

    def taxon_counts_stats(self) -> dict:
        """Of the last counts call: tile pairs, work items, u64 words of a work item, blocks per chunk, chunks."""
        out = np.zeros(5, np.int64)
        self._check(self._lib.tq_taxon_counts_stats(self._h, _ptr(out)))
        return dict(zip(("tile_pairs", "work_items", "slice_words", "chunk_blocks", "chunks"), (int(x) for x in out)))

    # -- device-pointer API (addresses as ints, e.g. torch.Tensor.data_ptr()) -------
    def resolve_dev(self, d_quartets: int, Q: int, subsample_snps: bool, d_rstat: int,
                    d_rscor: int, d_flags: int = 0, stream: int = 0):
        self._check(self._lib.tq_resolve_dev(
            self._h, d_quartets, Q, int(bool(subsample_snps)), d_rstat, d_rscor,
            d_flags or None, stream or None))

    def resolve_range_dev(self, first_rank: int, Q: int, subsample_snps: bool, d_quartets: int,
                          d_rstat: int, d_rscor: int, d_flags: int = 0, stream: int = 0):
        self._check(self._lib.tq_resolve_range_dev(
            self._h, first_rank, Q, int(bool(subsample_snps)), d_quartets or None, d_rstat,
            d_rscor, d_flags or None, stream or None))

    def scan_dev(self, d_quartets: int, Q: int, subsample_snps: bool, stream: int = 0):
        """Stage 1 (ordering + site scan) of quartets [0,Q) into the context's count slab."""
        self._check(self._lib.tq_scan_dev(self._h, d_quartets, Q, int(bool(subsample_snps)), stream or None))

    def svd_dev(self, q0: int, n: int, d_rstat: int, d_rscor: int, d_flags: int = 0, stream: int = 0):
        """Stage 2 for rows [q0, q0+n) of the scanned batch; the pointers are the outputs OF ROW q0."""
        self._check(self._lib.tq_svd_dev(self._h, q0, n, d_rstat, d_rscor, d_flags or None, stream or None))

    def sample_quartets_dev(self, seed: int, Q: int, d_quartets: int, d_ranks: int = 0, stream: int = 0):
        """Q distinct quartets drawn uniformly from C(T,4) on the device (opt-in sampler, not the project Generator's stream)."""
        self._check(self._lib.tq_sample_quartets_dev(self._h, int(seed) & (2**64 - 1), Q, d_ranks or None, d_quartets,
                                                     stream or None))

    def unrank_dev(self, d_ranks: int, Q: int, d_quartets: int, stream: int = 0):
        self._check(self._lib.tq_unrank_dev(self._h, d_ranks, Q, d_quartets, stream or None))

    # -- measurement -----------------------------------------------------------
    def timing_enable(self, on: bool = True):
        self._check(self._lib.tq_timing_enable(self._h, int(on)))

    def timing_read(self):
        ms = ctypes.c_double()
        n = ctypes.c_int64()
        self._check(self._lib.tq_timing_read(self._h, ctypes.byref(ms), ctypes.byref(n)))
        return ms.value, n.value

    def timing_read_split(self):
        """(total_ms, scan_ms, svd_ms, resolve_calls) since the last read."""
        tot, a, b = ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
        n = ctypes.c_int64()
        self._check(self._lib.tq_timing_read_split(
            self._h, ctypes.byref(tot), ctypes.byref(a), ctypes.byref(b), ctypes.byref(n)))
        return tot.value, a.value, b.value, n.value

    KERNEL_TAGS = ("order", "scan", "bidiag", "bdsqr", "score")

    def timing_read_kernels(self):
        """({"order","scan","bidiag","bdsqr","score"} -> summed ms, resolve_calls) since the last read."""
        ms = (ctypes.c_double * 5)()
        n = ctypes.c_int64()
        self._check(self._lib.tq_timing_read_kernels(self._h, ms, 5, ctypes.byref(n)))
        return dict(zip(self.KERNEL_TAGS, list(ms))), n.value

    def debug_fetch(self, which: str, n: int) -> np.ndarray:
        """Scratch of the last resolve call (test hook): 'cm' u32[n,256], 'de' f64[3n,32], 'sv' f64[3n,16]."""
        shape, dt, code = {"cm": ((n, 256), np.uint32, 0), "de": ((3 * n, 32), np.float64, 1),
                           "sv": ((3 * n, 16), np.float64, 2), "bdsqr_stats": ((8,), np.uint64, 3)}[which]
        out = np.zeros(shape, dt)
        self._check(self._lib.tq_debug_fetch(self._h, code, _ptr(out), out.nbytes))
        return out

    def site_pack_state(self):
        """Test hook: (padded site count of the packed layout set or 0, whether the subsample scans read it now)."""
        out = np.zeros(2, np.int64)
        self._check(self._lib.tq_debug_fetch(self._h, 4, _ptr(out), out.nbytes))
        return int(out[0]), bool(out[1])

    SCAN_FORMS = ("none", "one_wave", "wg", "wg2", "f4", "pb", "dp")

    def last_scan(self):
        """Test hook: (kernel form, T * pitch of the layout set it read, whether that was the packed set) of the most
        recent scan launch; the form is one of SCAN_FORMS ('one_wave' = tq_scan_kernel, the others the cooperative
        kernels tq_scan_<form>_kernel; 'none' before the first scan)."""
        out = np.zeros(3, np.int64)
        self._check(self._lib.tq_debug_fetch(self._h, 6, _ptr(out), out.nbytes))
        return self.SCAN_FORMS[int(out[0])], int(out[1]), bool(out[2])

    def boot_pack_map(self) -> np.ndarray:
        """Test hook: the site order of the packed set the current device-built replicate carries (option ``boot_pack``):
        u32[S'] as `pack_sites` returns it for the replicate's tmpmap.  Refused when the replicate was not packed."""
        out = np.zeros(self.site_pack_state()[0], np.uint32)
        self._check(self._lib.tq_debug_fetch(self._h, 5, _ptr(out), out.nbytes))
        return out

    def debug_bdsqr(self, de: np.ndarray, reps: int = 5):
        """Test hook: the bidiagonal-QR kernel alone on `de` f64[nmat,32] in the given order ->
        (sv f64[nmat,16], rotation steps u32[nmat], sweeps u32[nmat], ms per launch)."""
        de = np.ascontiguousarray(de, dtype=np.float64)
        nmat = de.shape[0]
        sv = np.zeros((nmat, 16), np.float64)
        work = np.zeros(nmat, np.uint32)
        ms = ctypes.c_double()
        self._check(self._lib.tq_debug_bdsqr(self._h, _ptr(de), nmat, _ptr(sv), _ptr(work), reps, ctypes.byref(ms)))
        return sv, work & 0xFFFF, work >> 16, ms.value

    def device_info(self):
        cu = ctypes.c_int32()
        w = ctypes.c_int32()
        pitch = ctypes.c_int64()
        self._check(self._lib.tq_device_info(self._h, ctypes.byref(cu), ctypes.byref(w), ctypes.byref(pitch)))
        return dict(num_cu=cu.value, waves_per_cu=w.value, row_pitch=pitch.value)

"""What the classes over a handle of the library share: the life cycle of the handle, and the small conversions
between the library's arrays and Python that several of them need."""
from __future__ import annotations

import ctypes
import weakref

import numpy as np

from . import _lib
from ._lib import TetradHipError


class Handle:
    """One handle of the library (`_h`) and its life cycle.  A class names its family of functions in `_prefix`
    (`tq_cons` -> tq_cons_create / tq_cons_destroy / tq_cons_reset) and sets `engine` before `_create` when it reports
    through an engine's context.  The library asks that the context outlive such a handle (its destructor selects the
    context's device and waits for its own work).  The reference to the engine is kept, so the engine OBJECT outlives the
    handle; an engine that is CLOSED first (a `with` block, a fixture) closes the handles made on it before its context
    goes, whether they are still in use, waiting in a reference cycle for the collector, or forgotten.  A handle whose
    engine is gone all the same (both were collected in one sweep, the engine first) is dropped without a call."""

    _prefix = ""
    _h = None
    engine = None
    _dependants = None              # weak set of the open handles made on this one (an engine's accumulators)

    def _fn(self, name):
        return getattr(self._lib, f"{self._prefix}_{name}")

    def _ctx(self):
        """The context whose last error describes a failed call: the engine's, or NULL without one."""
        return self.engine._h if self.engine is not None else None

    def _create(self, *args):
        """tq_<family>_create(&handle, *args).  On failure `_h` stays None and TetradHipError is raised."""
        self._lib = _lib.load()
        self._h = None
        h = ctypes.c_void_p()
        self._check(self._fn("create")(ctypes.byref(h), *args))
        self._h = h
        if self.engine is not None:
            if self.engine._dependants is None:
                self.engine._dependants = weakref.WeakSet()
            self.engine._dependants.add(self)

    def _check(self, rc: int):
        if rc != 0:
            raise TetradHipError(rc, self._lib.tq_last_error(self._ctx()).decode())

    def close(self):
        if self._dependants:
            for dependant in list(self._dependants):
                dependant.close()
            self._dependants = None
        if self._h:
            if self.engine is None or self.engine._h:           # else the context is gone: its destructor would read it
                self._fn("destroy")(self._h)
            self._h = None
            if self.engine is not None and self.engine._dependants is not None:
                self.engine._dependants.discard(self)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self):
        """tq_<family>_reset, for the families that have one (every accumulator; the engine has none)."""
        self._check(self._fn("reset")(self._h))


def mask_bits(masks: np.ndarray, ntaxa: int) -> np.ndarray:
    """Mask words u64[E, W] -> bool[E, ntaxa]."""
    E, W = masks.shape
    bits = np.unpackbits(masks.view(np.uint8).reshape(E, 8 * W), axis=1, bitorder="little")
    return bits[:, :ntaxa].astype(bool)


def grow_text(call, cap: int, check) -> str:
    """The ASCII text a library function writes: `call(buffer address, cap, byref(written))` -> return code.  Where
    the buffer was too small (TQ_ERR_OOM with the needed size in `written`) it is called once more with that size;
    every other failure goes to `check(rc)`, which raises."""
    written = ctypes.c_int64()
    for _ in range(2):
        buf = np.empty(cap, dtype=np.uint8)
        rc = call(buf.ctypes.data, cap, ctypes.byref(written))
        if rc == 0:
            return buf[:written.value].tobytes().decode("ascii")
        if rc != -6 or written.value <= cap:
            break
        cap = written.value
    check(rc)


def medoid(dist: np.ndarray):
    """(index, row sum) of the row of an integer distance matrix with the smallest sum; ties go to the lowest index."""
    if not len(dist):
        raise ValueError("no trees")
    sums = [sum(int(x) for x in row) for row in dist]
    best = min(range(len(sums)), key=lambda i: (sums[i], i))
    return best, sums[best]


def mean_pairs(dist: np.ndarray) -> float:
    """The mean of an integer distance matrix over the pairs i < j; 0.0 for fewer than 2 rows."""
    N = len(dist)
    if N < 2:
        return 0.0
    total = sum(int(x) for x in dist[np.triu_indices(N, 1)])
    return total / (N * (N - 1) // 2)

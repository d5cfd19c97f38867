"""What the wrappers of every context share (hector.py, gmapping.py, plicp.py, undistort.py and the Karto stages'): the
error check, the context's lifetime, the kernel timing calls and the ctypes helpers.  A subclass names its C prefix
(`_PREFIX = "kl"`), sets `self.L` and `self.h`, and mirrors its entry points.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import Slam2dError


def hp(a):
    """A host array's address."""
    return a.ctypes.data_as(C.c_void_p)


def dp(addr):
    """A device address (or a stream) given as an int; 0 is NULL."""
    return C.c_void_p(int(addr) or None)


def params_from(L, Struct, fn_name: str, **kw):
    """A parameter struct filled by the library's `fn_name`, then overridden by keywords."""
    p = Struct()
    getattr(L, fn_name)(C.byref(p))
    for k, v in kw.items():
        if k not in [f for f, _ in Struct._fields_]:
            raise TypeError(f"unknown parameter {k}")
        setattr(p, k, v)
    return p


class Stage:
    """A context handle `h` of the library `L` with the C prefix `_PREFIX`."""

    _PREFIX = ""
    L = None
    h = None

    def _check(self, rc, what):
        if rc != 0:
            text = getattr(self.L, f"{self._PREFIX}_last_error")().decode(errors="replace")
            err = Slam2dError(f"{what} failed with code {rc}: {text}")
            err.code = rc
            raise err

    def close(self):
        if self.h:
            getattr(self.L, f"{self._PREFIX}_destroy")(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class TimedStage(Stage):
    """A stage with the xx_set_timing / xx_num_kernels / xx_kernel_name / xx_get_kernel_times calls.  The two oldest
    wrappers override both methods only to keep their signatures (`on`, reset=True); hector.py, gmapping.py and plicp.py,
    whose C-ABI has no kernel-name calls, keep their own pair on `Stage`."""

    def set_timing(self, enable: bool):
        p = self._PREFIX
        self._check(getattr(self.L, f"{p}_set_timing")(self.h, int(bool(enable))), f"{p}_set_timing")

    def kernel_times(self, reset: bool = False) -> dict:
        """{kernel name: (milliseconds, launches)} since the last reset; waits for the device."""
        p = self._PREFIX
        n = getattr(self.L, f"{p}_num_kernels")()
        ms, cnt = np.zeros(n, np.float64), np.zeros(n, np.int64)
        self._check(getattr(self.L, f"{p}_get_kernel_times")(self.h, hp(ms), hp(cnt), int(bool(reset))),
                    f"{p}_get_kernel_times")
        name = getattr(self.L, f"{p}_kernel_name")
        return {name(k).decode(): (float(ms[k]), int(cnt[k])) for k in range(n)}


def library(declare):
    """The loaded library with a module's prototypes declared."""
    L = _lib.lib()
    declare(L)
    return L

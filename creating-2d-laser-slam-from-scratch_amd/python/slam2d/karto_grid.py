"""Karto occupancy-grid rebuild over the MI355X C-ABI (include/slam2d/karto_grid.h).

Reference: karto::OccupancyGrid::CreateFromScans (lesson6/lib/open_karto/include/open_karto/Karto.h:5659-5673), the
producer of SlamKarto::updateMap's /map (lesson6/src/karto_slam.cc:507-581).  `OccupancyGridBuilder.create_from_scans`
mirrors one CreateFromScans call plus the translation to nav_msgs/OccupancyGrid bytes.  open_karto needs boost and is
not built here: results are checked against tests/ref/karto_grid_ref.c (parity unpinned against open_karto itself).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import Slam2dError
from ._stage import TimedStage, dp as _dp, hp as _hp, library
from .karto import KtLaser

KG_OK, KG_EINVAL, KG_ERANGE = 0, -1, -5


class KgParams(C.Structure):
    _fields_ = [("resolution", C.c_double), ("maximum_range", C.c_double), ("occupancy_threshold", C.c_double),
                ("min_pass_through", C.c_uint32), ("pad_", C.c_int)]


class KgInfo(C.Structure):
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("offset_x", C.c_double), ("offset_y", C.c_double),
                ("status", C.c_int), ("pad_", C.c_int)]


class MapTooLarge(Slam2dError):
    """kg_build returned KG_ERANGE: the map has more cells than max_cells.  `width`, `height` and `offset` are the
    map's, so the caller can create a larger builder."""

    def __init__(self, msg, width, height, offset):
        super().__init__(msg)
        self.width, self.height, self.offset = width, height, offset


def _declare(L):
    if getattr(L, "_kg_declared", False):
        return
    vp, i = C.c_void_p, C.c_int
    L.kg_last_error.restype = C.c_char_p
    L.kg_default_params.restype = None
    L.kg_default_params.argtypes = [C.POINTER(KgParams)]
    L.kg_create.argtypes = [C.POINTER(vp), C.POINTER(KtLaser), C.POINTER(KgParams), i, C.c_size_t]
    L.kg_destroy.argtypes = [vp]
    L.kg_build.argtypes = [vp, i, vp, vp, C.POINTER(KgInfo)]
    L.kg_build_device.argtypes = [vp, i, vp, vp, C.POINTER(KgInfo), vp]
    L.kg_get_map.argtypes = [vp, vp, vp, vp, vp]
    L.kg_device_planes.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]
    L.kg_set_timing.argtypes = [vp, i]
    L.kg_kernel_name.restype = C.c_char_p
    L.kg_kernel_name.argtypes = [i]
    L.kg_get_kernel_times.argtypes = [vp, vp, vp, i]
    L._kg_declared = True


def default_params(maximum_range: float, resolution: float | None = None) -> KgParams:
    """kg_default_params (resolution 0.05, occupancy threshold 0.1, min pass-through 2) with the laser's maximum
    range, which has no default (scan->range_max, karto_slam.cc:389-395)."""
    L = _lib.lib()
    _declare(L)
    p = KgParams()
    L.kg_default_params(C.byref(p))
    p.maximum_range = float(maximum_range)
    if resolution is not None:
        p.resolution = float(resolution)
    return p


def _dev(x):
    """A device address from an int or a torch tensor (data_ptr)."""
    if hasattr(x, "data_ptr"):
        return C.c_void_p(x.data_ptr())
    return C.c_void_p(int(x))


class OccupancyGridBuilder(TimedStage):
    """OccupancyGrid::CreateFromScans for up to `max_scans` scans of `laser` and maps of up to `max_cells` cells."""

    _PREFIX = "kg"

    def __init__(self, laser: KtLaser, params: KgParams, max_scans: int = 64, max_cells: int = 1 << 20):
        self.L = library(_declare)
        self.laser, self.params = laser, params
        self.max_scans, self.max_cells = int(max_scans), int(max_cells)
        self.width = self.height = 0
        self.offset = np.zeros(2)
        self.h = C.c_void_p()
        self._check(self.L.kg_create(C.byref(self.h), C.byref(laser), C.byref(params), self.max_scans, self.max_cells),
                    "kg_create")

    def _built(self, rc, info, what):
        off = np.array([info.offset_x, info.offset_y])
        if rc == KG_ERANGE:
            self.width = self.height = 0
            raise MapTooLarge(f"{what}: {self.L.kg_last_error().decode(errors='replace')}", info.width, info.height, off)
        self._check(rc, what)
        self.width, self.height, self.offset = info.width, info.height, off

    def get_map(self) -> dict:
        """The last build: width, height, offset and the dense [height, width] planes state (0 / 100 / 255), ros
        (-1 / 100 / 0), pass, hits."""
        w, h = self.width, self.height
        st, ro = np.zeros((h, w), np.uint8), np.zeros((h, w), np.int8)
        ps, ht = np.zeros((h, w), np.uint32), np.zeros((h, w), np.uint32)
        self._check(self.L.kg_get_map(self.h, _hp(st), _hp(ro), _hp(ps), _hp(ht)), "kg_get_map")
        return {"width": w, "height": h, "offset": self.offset.copy(), "state": st, "ros": ro, "pass": ps, "hits": ht}

    def create_from_scans(self, ranges, poses) -> dict:
        """CreateFromScans(scans, resolution) from host arrays [count, n_readings] and [count, 3]."""
        n = self.laser.n_readings
        r = np.ascontiguousarray(ranges, np.float64).reshape(-1, n)
        p = np.ascontiguousarray(poses, np.float64).reshape(-1, 3)
        if r.shape[0] != p.shape[0]:
            raise ValueError("ranges and poses disagree on the scan count")
        info = KgInfo()
        rc = self.L.kg_build(self.h, r.shape[0], _hp(r), _hp(p), C.byref(info))
        self._built(rc, info, "kg_build")
        return self.get_map()

    def create_from_scans_device(self, count: int, d_ranges, d_poses, hip_stream: int = 0, fetch: bool = True):
        """CreateFromScans from device arrays (addresses or torch tensors), stream-ordered.  Returns the map as
        create_from_scans does, or with fetch=False only (width, height, offset): read device_planes() then."""
        info = KgInfo()
        rc = self.L.kg_build_device(self.h, int(count), _dev(d_ranges), _dev(d_poses), C.byref(info), _dp(hip_stream))
        self._built(rc, info, "kg_build_device")
        return self.get_map() if fetch else (self.width, self.height, self.offset.copy())

    def device_planes(self) -> dict:
        """Device addresses of the context's planes (dense width x height of the last build)."""
        ptrs = [C.c_void_p() for _ in range(4)]
        self._check(self.L.kg_device_planes(self.h, *[C.byref(p) for p in ptrs]), "kg_device_planes")
        return {k: int(p.value or 0) for k, p in zip(("state", "ros", "pass", "hits"), ptrs)}

    def set_timing(self, on: bool):
        super().set_timing(on)

    def kernel_times(self, reset: bool = True) -> dict:
        return super().kernel_times(reset)

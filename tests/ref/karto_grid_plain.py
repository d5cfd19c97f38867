"""A plain Python float64 model of karto::OccupancyGrid::CreateFromScans, written from the reference text and not
from tests/ref/karto_grid_ref.c, to check that restatement's geometry (the box, the offset, the cell rounding, the
clip at range_threshold) against something other than itself.

  scan_box                LocalizedRangeScan::Update's bounding box, Karto.h:5379-5424 (InRange: Math.h:172)
  dimensions              ComputeDimensions, Karto.h:5804-5822 (BoundingBox2: :2765, :2805-2819; Round: Math.h:87-90)
  world_to_grid           CoordinateConverter::WorldToGrid, Karto.h:4237-4252, scale 1 / resolution (:5635)
  trace_line              Grid<T>::TraceLine, Karto.h:4680-4745, the loop as written
  create_from_scans       AddScan's reading rules and clip (Karto.h:5852-5899), RayTrace's end point (:5910-5945),
                          Update / UpdateCell (:5953-5990) and karto_slam.cc:553-567's bytes

Trigonometry is math.sin / math.cos -- deliberately not csrc/detmath.h, which the kernels and the restatement share.
The two may differ in the last place, which moves a point by about 1e-11 cells at the tests' ranges and scales, so
the model also reports how far its inputs are from every decision such a difference could flip:

  margin            the smallest distance, in cells, of any traced end point, any scan position and the two map
                    extents from a rounding boundary k + 0.5
  threshold_margin  the smallest distance, in cells, of a traced reading from range_threshold and from
                    range_threshold - 1e-6 (comparisons of the input itself, which no arithmetic precedes)

Test infrastructure: nothing here is imported by the package.
"""
from __future__ import annotations

import math

import numpy as np

KT_TOLERANCE = 1e-06
BOX_INIT = 999999999999999999.99999


def _round(v: float) -> float:
    return math.floor(v + 0.5) if v >= 0.0 else math.ceil(v - 0.5)


def _boundary_distance(v: float) -> float:
    """The distance of v from the nearest k + 0.5."""
    return abs(v - math.floor(v) - 0.5)


class _Box:
    def __init__(self):
        self.lo = [BOX_INIT, BOX_INIT]
        self.hi = [-BOX_INIT, -BOX_INIT]

    def add(self, x, y):
        self.lo = [min(self.lo[0], x), min(self.lo[1], y)]
        self.hi = [max(self.hi[0], x), max(self.hi[1], y)]


def _beam_point(lz, pose, i, r):
    angle = pose[2] + lz["minimum_angle"] + i * lz["angular_resolution"]
    return pose[0] + (r * math.cos(angle)), pose[1] + (r * math.sin(angle))


def scan_box(lz, ranges, pose) -> _Box:
    """The sensor position and every reading within [minimum_range, range_threshold]."""
    b = _Box()
    b.add(pose[0], pose[1])
    for i, r in enumerate(ranges):
        if r >= lz["minimum_range"] and r <= lz["range_threshold"]:
            b.add(*_beam_point(lz, pose, i, r))
    return b


def dimensions(case):
    """width, height, offset (the box minimum) and the extents' distance from a rounding boundary."""
    lz = case["laser"]
    box = _Box()
    for ranges, pose in zip(case["ranges"].tolist(), case["poses"].tolist()):
        b = scan_box(lz, ranges, pose)
        box.add(*b.lo)
        box.add(*b.hi)
    scale = 1.0 / case["resolution"]
    ex, ey = (box.hi[0] - box.lo[0]) * scale, (box.hi[1] - box.lo[1]) * scale
    return int(_round(ex)), int(_round(ey)), box.lo, min(_boundary_distance(ex), _boundary_distance(ey))


def trace_line(x0, y0, x1, y1):
    """The points of TraceLine in its order, valid or not."""
    steep = abs(y1 - y0) > abs(x1 - x0)
    if steep:
        x0, y0, x1, y1 = y0, x0, y1, x1
    if x0 > x1:
        x0, y0, x1, y1 = x1, y1, x0, y0
    delta_x, delta_y = x1 - x0, abs(y1 - y0)
    error, y = 0, y0
    ystep = 1 if y0 < y1 else -1
    points = []
    for x in range(x0, x1 + 1):
        points.append((y, x) if steep else (x, y))
        error += delta_y
        if 2 * error >= delta_x:
            y += ystep
            error -= delta_x
    return points


def create_from_scans(case) -> dict:
    """width, height, offset[2], pass, hits, state, ros [height, width], margin, threshold_margin."""
    lz = case["laser"]
    thr, lo, hi = lz["range_threshold"], lz["minimum_range"], lz["maximum_range"]
    width, height, offset, margin = dimensions(case)
    scale = 1.0 / case["resolution"]
    threshold_margin = math.inf
    ps = np.zeros((height, width), np.uint32)
    ht = np.zeros((height, width), np.uint32)

    def world_to_grid(wx, wy):
        nonlocal margin
        gx, gy = (wx - offset[0]) * scale, (wy - offset[1]) * scale
        margin = min(margin, _boundary_distance(gx), _boundary_distance(gy))
        return int(_round(gx)), int(_round(gy))

    def valid(x, y):
        return 0 <= x < width and 0 <= y < height

    for ranges, pose in zip(case["ranges"].tolist(), case["poses"].tolist()):
        for i, r in enumerate(ranges):
            end_valid = r < (thr - KT_TOLERANCE)
            if r <= lo or r >= hi or math.isnan(r):
                continue
            threshold_margin = min(threshold_margin, abs(r - thr) * scale, abs(r - (thr - KT_TOLERANCE)) * scale)
            px, py = _beam_point(lz, pose, i, r)
            if r >= thr:
                ratio = thr / r
                dx, dy = px - pose[0], py - pose[1]
                px, py = pose[0] + ratio * dx, pose[1] + ratio * dy
            x0, y0 = world_to_grid(pose[0], pose[1])
            x1, y1 = world_to_grid(px, py)
            for x, y in trace_line(x0, y0, x1, y1):
                if valid(x, y):
                    ps[y, x] += 1
            if end_valid and valid(x1, y1):
                ps[y1, x1] += 1
                ht[y1, x1] += 1

    st = np.zeros((height, width), np.uint8)
    known = ps > case["min_pass_through"]
    with np.errstate(divide="ignore", invalid="ignore"):
        occupied = known & (ht.astype(np.float64) / ps.astype(np.float64) > case["occupancy_threshold"])
    st[known] = 255
    st[occupied] = 100
    ro = np.where(st == 0, -1, np.where(st == 100, 100, 0)).astype(np.int8)
    return {"width": width, "height": height, "offset": np.array(offset), "pass": ps, "hits": ht, "state": st,
            "ros": ro, "margin": margin, "threshold_margin": threshold_margin}

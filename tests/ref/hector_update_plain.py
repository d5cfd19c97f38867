"""OccGridMapBase::updateByScan of one level, stated plainly beam by beam (CPU, numpy + a Python dict walk).

Independent of oracle/hector_oracle.c's update: the end cells are numpy float32 in the documented order
m + (c px + (-s) py), then + 0.5, truncated by int(); the cells of a beam come from make_golden.py_ray_cells (the
pure-Python Bresenham the oracle's walk is already pinned to); the cell rules (bresenhamCellFree / bresenhamCellOcc,
OccGridMapBase.h:302-330, with updateSetFree / updateUnsetFree / updateSetOccupied of GridMapLogOdds.h:108-129) are
a walk over a Python dict of the touched cells.  Only cos and sin are shared with the oracle (ho_det_cosf /
ho_det_sinf, pinned to libm within 1 ulp by tests/test_oracle_cpu.py).

PlainMap mirrors MapRepMultiMap: level i has the level-0 size >> i, twice the cell length, and draws the
DataContainer of the last matchData scaled by 1 / 2^i (MapRepMultiMap.h:161, :187); level 0 draws the scan it is
given.  Every update records, per level, what tests/ref/hector_update_cases.reach() needs: the begin cell, every
beam's end cell (None: nothing drawn), and per touched cell the first beam that freed it and the first that hit it.
"""
import numpy as np

import oracle as O
from make_golden import py_ray_cells

F = np.float32
I32_LO, I32_HI = -2147483648.0, 2147483648.0


def cell_of(v):
    """(int)v for v inside the int range, else (NaN included) -1, which the bounds test cancels."""
    v = float(v)
    return int(v) if (v > I32_LO and v < I32_HI) else -1


def prob_to_logodds(p):
    """GridMapLogOddsFunctions::probToLogOdds: float odds, double log, rounded to float."""
    p = F(p)
    odds = p / (F(1.0) - p)
    return F(np.log(np.float64(odds)))


class Level:
    def __init__(self, res, sx, sy, mid_x, mid_y, i):
        self.sx, self.sy = sx, sy
        self.cell_len = F(res)
        self.scale = F(1.0) / self.cell_len
        self.tx, self.ty = self.scale * F(mid_x), self.scale * F(mid_y)
        self.f = F(1.0 / 2.0 ** i)
        self.l = np.zeros(sx * sy, F)
        self.u = np.full(sx * sy, -1, np.int32)
        self.cur = 0        # currUpdateIndex
        self.last = -1      # lastUpdateIndex
        self.rec = None     # the last update's record


class PlainMap:
    def __init__(self, res, sx, sy, start, levels, free_factor=0.4, occ_factor=0.6):
        res = F(res)
        mid_x = (res * F(sx)) * F(start[0])
        mid_y = (res * F(sy)) * F(start[1])
        self.lv = []
        for i in range(levels):
            self.lv.append(Level(res, sx >> i, sy >> i, mid_x, mid_y, i))
            res = res * F(2.0)
        self.lf, self.lo = prob_to_logodds(free_factor), prob_to_logodds(occ_factor)
        self.mc = (np.zeros((0, 2), F), (0.0, 0.0))   # dataContainers of the last matchData
        self.cells = self.rays = self.touched = 0

    def store_container(self, pts, origo=(0.0, 0.0)):
        self.mc = (np.ascontiguousarray(pts, F).reshape(-1, 2).copy(), origo)

    def set_level(self, lvl, l, u):
        L = self.lv[lvl]
        L.l = np.ascontiguousarray(l, F).reshape(-1).copy()
        L.u = np.ascontiguousarray(u, np.int32).reshape(-1).copy()

    def level(self, lvl):
        L = self.lv[lvl]
        return L.l.reshape(L.sy, L.sx), L.u.reshape(L.sy, L.sx)

    def publish(self, lvl):
        l, _ = self.level(lvl)
        with np.errstate(all="ignore"):
            return np.where(l < 0, 0, np.where(l > 0, 100, -1)).astype(np.int8)

    # ------------------------------------------------------------------------------------------------
    def end_cells(self, lvl, pts, pose, origo=(0.0, 0.0)):
        """(begin cell, [end cell of every beam]) of level lvl: float32 throughout, one rounding per operation."""
        L = self.lv[lvl]
        pts = np.ascontiguousarray(pts, F).reshape(-1, 2)
        w = [F(v) for v in pose]
        with np.errstate(all="ignore"):
            mx = L.tx + (L.scale * w[0] + F(0.0) * w[1])      # getMapCoordsPose
            my = L.ty + (F(0.0) * w[0] + L.scale * w[1])
            cs, sn = F(O.hector_lib().ho_det_cosf(w[2])), F(O.hector_lib().ho_det_sinf(w[2]))
            nsn = -sn
            ox, oy = F(origo[0]) * L.f, F(origo[1]) * L.f
            bx = mx + (cs * ox + nsn * oy)
            by = my + (sn * ox + cs * oy)
            begin = (cell_of(bx + F(0.5)), cell_of(by + F(0.5)))
            px, py = pts[:, 0] * L.f, pts[:, 1] * L.f
            ex = mx + (cs * px + nsn * py)
            ey = my + (sn * px + cs * py)
            ex = ex + F(0.5)
            ey = ey + F(0.5)
        return begin, [(cell_of(a), cell_of(b)) for a, b in zip(ex.tolist(), ey.tolist())]

    def update_level(self, lvl, pts, pose, origo=(0.0, 0.0)):
        L = self.lv[lvl]
        lf, lo = self.lf, self.lo
        mf, mo = L.cur + 1, L.cur + 2
        begin, ends = self.end_cells(lvl, pts, pose, origo)
        cells = {}                 # offset -> [log-odds, updateIndex]
        first_free, first_hit = {}, {}
        drawn = []
        sum_l = 0
        with np.errstate(all="ignore"):
            for b, end in enumerate(ends):
                walk = py_ray_cells(L.sx, L.sy, begin[0], begin[1], end[0], end[1]) if end != begin else []
                if not walk:
                    drawn.append(None)
                    continue
                drawn.append(end)
                sum_l += len(walk)
                for off in walk[:-1]:                     # bresenhamCellFree
                    c = cells.get(off)
                    if c is None:
                        c = cells[off] = [L.l[off], int(L.u[off])]
                    first_free.setdefault(off, b)
                    if c[1] < mf:
                        c[0] = c[0] + lf
                        c[1] = mf
                off = walk[-1]                            # bresenhamCellOcc
                c = cells.get(off)
                if c is None:
                    c = cells[off] = [L.l[off], int(L.u[off])]
                if c[1] < mo:
                    if c[1] == mf:
                        c[0] = c[0] - lf
                    if c[0] < F(50.0):
                        c[0] = c[0] + lo
                    c[1] = mo
                first_hit.setdefault(off, b)
        touched = 0
        for off, (l, u) in cells.items():
            touched += int(u != int(L.u[off]))
            L.l[off] = l
            L.u[off] = u
        L.last += 1
        L.cur += 3
        L.rec = dict(begin=begin, ends=drawn, first_free=first_free, first_hit=first_hit, n=len(ends))
        self.cells += sum_l
        self.rays += sum(e is not None for e in drawn)
        self.touched += touched

    def update_by_scan(self, pts, pose, origo=(0.0, 0.0)):
        """MapRepMultiMap::updateByScan: the counters are those of this call."""
        self.cells = self.rays = self.touched = 0
        for lvl in range(len(self.lv)):
            if lvl == 0:
                self.update_level(0, pts, pose, origo)
            else:
                self.update_level(lvl, self.mc[0], pose, self.mc[1])

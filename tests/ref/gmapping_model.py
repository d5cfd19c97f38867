"""Exact-integer model of gm_compute_kernel's raster (gmapping_kernels.hip: gm_line, gm_clip and the closed form
q(i) = floor((2 db i + da) / (2 da))): which cells of which 64 x 32 tile a beam's line frees.  Python integers, so no
quotient is estimated and nothing rounds: where the model equals GridLineTraversal::gridLine (the oracle's
gmo_grid_line) the formula is right, and a GPU mismatch on the same line is the device arithmetic's (gm_udiv, the
packed walk, the LDS hand-offs)."""
import numpy as np

TILE_W, TILE_H = 64, 32


def line(x0, y0, x1, y1):
    """gm_line: the line in (major a, minor b) coordinates from its smaller-major end; steps [ilo, ihi] are freed."""
    dx, dy = abs(x1 - x0), abs(y1 - y0)
    xm = dy <= dx
    a0, b0, a1, b1 = (x0, y0, x1, y1) if xm else (y0, x0, y1, x1)
    rev = a1 < a0                       # p1 is the walk's start
    a_s, b_s, b_e = (a1, b1, b0) if rev else (a0, b0, b1)
    da, db = (dx, dy) if xm else (dy, dx)
    return dict(a_s=a_s, b_s=b_s, sb=1 if b_e > b_s else -1, da=da, db=db, xm=xm, ilo=1 if rev else 0,
                ihi=da if rev else da - 1)


def clip(l, A0, A1, B0, B1, numerators=None):
    """gm_clip: the steps of l inside [A0, A1) x [B0, B1), or None; the two division numerators go to `numerators`."""
    lo, hi = max(l["ilo"], A0 - l["a_s"]), min(l["ihi"], A1 - 1 - l["a_s"])
    if lo > hi:
        return None
    tlo, thi = (B0 - l["b_s"], B1 - 1 - l["b_s"]) if l["sb"] > 0 else (l["b_s"] - (B1 - 1), l["b_s"] - B0)
    if thi < 0:
        return None
    if l["db"] == 0:
        return (lo, hi) if tlo <= 0 else None
    da, db = l["da"], l["db"]
    if tlo > 0:                         # smallest i with q(i) >= tlo
        x = 2 * da * tlo - da + 2 * db - 1
        lo = max(lo, x // (2 * db))
    y = 2 * da * (thi + 1) - da - 1     # largest i with q(i) <= thi
    hi = min(hi, y // (2 * db))
    if numerators is not None:
        numerators.append((y, lo <= hi))
    return (lo, hi) if lo <= hi else None


def free_cells(x0, y0, x1, y1, sx, sy, numerators=None):
    """The cells [k, 2] of the map that the beam p0 -> p1 frees, gathered tile by tile as the kernel does."""
    l = line(x0, y0, x1, y1)
    out = []
    for ty in range(max(min(y0, y1), 0) // TILE_H, min(max(y0, y1), sy - 1) // TILE_H + 1):
        for tx in range(max(min(x0, x1), 0) // TILE_W, min(max(x0, x1), sx - 1) // TILE_W + 1):
            X0, Y0 = tx * TILE_W, ty * TILE_H
            X1, Y1 = min(X0 + TILE_W, sx), min(Y0 + TILE_H, sy)
            r = clip(l, X0, X1, Y0, Y1, numerators) if l["xm"] else clip(l, Y0, Y1, X0, X1, numerators)
            if r is None:
                continue
            i = np.arange(r[0], r[1] + 1, dtype=np.int64)
            q = (2 * l["db"] * i + l["da"]) // (2 * l["da"]) if l["da"] else 0 * i
            a, b = l["a_s"] + i, l["b_s"] + l["sb"] * q
            x, y = (a, b) if l["xm"] else (b, a)
            assert ((x >= X0) & (x < X1) & (y >= Y0) & (y < Y1)).all(), (x0, y0, x1, y1, tx, ty)
            out.append(np.stack([x, y], axis=1))
    return np.concatenate(out) if out else np.zeros((0, 2), np.int64)

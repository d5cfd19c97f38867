#!/usr/bin/env python3
"""CPU model of the duplicate rays hs_update_kernel's ray setup drops (no GPU).

A ray is its end cell (all rays of a scan share the begin cell), so two beams with the same end cell walk the same
cells.  For the bench's scans (python/slam2d/synth.py: 8 paths x 4 poses, 2048^2 x 3 levels at 20 cells/m, the ray
construction of tools/visit_model.py) this prints, per level and per scan:
  valid rays; rays left when a beam equal to its predecessor is dropped (what the kernel does); distinct rays;
  walk steps (sum of da + 1) of all valid rays -> of the kept ones;
  (tile, fan group) box visits with the beams in their 64-beam groups as they come (invalid ones keep their slot)
  -> with the kept rays packed in beam order into consecutive groups;
  the sum over tiles of the busiest wave's visits (wave w draws the groups w, w + 4, ...; the per-tile barrier
  makes the busiest wave the tile's path), before -> after.
    python3 tools/dedup_model.py [paths [poses]]
"""
import sys

import numpy as np

from visit_model import TILE, TILE_H, level_rays, synth


def visits(x0, y0, x1, y1, drawn, nslots):
    """(tile, group) box visits and the sum over tiles of the busiest wave's, for rays in slots 0 .. nslots - 1
    (drawn: which slots hold a ray; group = slot // 64, its box = begin cell + its rays' end cells)."""
    per_tile = {}
    total = 0
    for g0 in range(0, nslots, 64):
        idx = np.arange(g0, min(g0 + 64, nslots))
        idx = idx[drawn[idx]]
        gx0, gx1, gy0, gy1 = x0, x0, y0, y0
        if len(idx):
            gx0, gx1 = min(x0, x1[idx].min()), max(x0, x1[idx].max())
            gy0, gy1 = min(y0, y1[idx].min()), max(y0, y1[idx].max())
        for tx in range(gx0 // TILE, gx1 // TILE + 1):
            for ty in range(gy0 // TILE_H, gy1 // TILE_H + 1):
                per_tile.setdefault((tx, ty), np.zeros(4, int))[(g0 // 64) % 4] += 1
                total += 1
    return total, sum(int(w.max()) for w in per_tile.values())


def main():
    paths = int(sys.argv[1]) if len(sys.argv) > 1 else 8
    poses = int(sys.argv[2]) if len(sys.argv) > 2 else 4
    ss = synth.make_streams(paths, poses, distinct_paths=paths)
    acc = np.zeros((3, 9))
    for k in range(paths):
        for t in range(poses):
            pts = ss.points[k, t, :ss.counts[k, t]]
            for lvl in range(3):
                size = 2048 >> lvl
                x0, y0, x1, y1 = level_rays(pts, ss.gt[k, t], lvl)
                valid = ~((x1 == x0) & (y1 == y0)) & (x1 >= 0) & (x1 < size) & (y1 >= 0) & (y1 < size)
                same = np.zeros(len(x1), bool)
                same[1:] = (x1[1:] == x1[:-1]) & (y1[1:] == y1[:-1])
                keep = valid & ~same
                L = np.maximum(abs(x1 - x0), abs(y1 - y0)) + 1
                anyd = len({(a, b) for a, b in zip(x1[valid].tolist(), y1[valid].tolist())})
                v0, b0 = visits(x0, y0, x1, y1, valid, len(x1))
                v1, b1 = visits(x0, y0, x1[keep], y1[keep], np.ones(int(keep.sum()), bool), int(keep.sum()))
                acc[lvl] += [valid.sum(), keep.sum(), anyd, L[valid].sum(), L[keep].sum(), v0, v1, b0, b1]
    acc /= paths * poses
    print(f"{paths} paths x {poses} poses; per scan:")
    print("| level | valid rays | kept (neighbour differs) | distinct (any) | walk steps: all -> kept | "
          "(tile, group) box visits: today -> packed | sum over tiles of the busiest wave's visits |")
    print("|---|---|---|---|---|---|---|")
    rows = [(str(lvl), acc[lvl]) for lvl in range(3)] + [("all", acc.sum(0))]
    for name, a in rows:
        print(f"| {name} | {a[0]:.0f} | {a[1]:.0f} | {a[2]:.0f} | {a[3] / 1e3:.1f} k -> {a[4] / 1e3:.1f} k "
              f"({100 * a[4] / a[3]:.0f} %) | {a[5]:.0f} -> {a[6]:.0f} | {a[7]:.1f} -> {a[8]:.1f} "
              f"({100 * (a[8] / a[7] - 1):+.1f} %) |")
    g = [int(np.ceil(acc[lvl][1] / 64)) for lvl in range(3)]
    print(f"fan groups per level: 17 today -> about {g[0]}, {g[1]}, {g[2]} packed")


if __name__ == "__main__":
    main()

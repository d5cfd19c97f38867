"""Why hs_update_kernel may raster each distinct ray once (numpy model, no GPU).

The kernel's tile raster leaves, per cell, the minimum event word over all beams -- beam b frees the cells of its
walk with the event 2 b + 1 and marks its end cell with 2 b -- and a hit bit per end cell.  The apply reads a
word as: marked or not, and (where the hit bit is set) its parity.  The ray setup drops every beam that is
invalid or whose ray (its end cell: all rays share the begin cell) equals its predecessor's, and numbers the
survivors 0 .. nu - 1 in beam order.  This test builds both mark sets on random small scans and compares them as
(marked, parity where hit, hit).
"""
import numpy as np

INVALID = None


def walk(x0, y0, x1, y1):
    """Cells of bresenham2D in the kernel's closed form: step i of the major axis, minor q(i) = (e0 + i db) // da."""
    dx, dy = x1 - x0, y1 - y0
    adx, ady = abs(dx), abs(dy)
    sx, sy = (1 if dx > 0 else -1), (1 if dy > 0 else -1)
    xm = adx >= ady
    da, db = (adx, ady) if xm else (ady, adx)
    e0 = da // 2
    cells = []
    for i in range(da + 1):
        q = (e0 + i * db) // da
        cells.append((x0 + sx * i, y0 + sy * q) if xm else (x0 + sx * q, y0 + sy * i))
    return cells  # steps 0 .. da - 1 are freed, step da is the end cell


def marks(begin, rays):
    """cell -> minimum event, and the set of hit cells, from rays numbered by their position in the list."""
    ev, hit = {}, set()
    for b, r in enumerate(rays):
        if r is INVALID:
            continue
        cells = walk(begin[0], begin[1], r[0], r[1])
        for c in cells[:-1]:
            ev[c] = min(ev.get(c, 1 << 40), 2 * b + 1)
        ev[cells[-1]] = min(ev.get(cells[-1], 1 << 40), 2 * b)
        hit.add(cells[-1])
    return ev, hit


def survivors(rays):
    return [r for b, r in enumerate(rays) if r is not INVALID and (b == 0 or r != rays[b - 1])]


def outcome(ev, hit):
    """What the apply reads: the marked cells, the parity of the hit cells' words, the hit cells."""
    return set(ev), {c: ev[c] & 1 for c in hit}, hit


def check(begin, rays):
    kept = survivors(rays)
    assert outcome(*marks(begin, rays)) == outcome(*marks(begin, kept))
    return len(kept)


def random_scan(rng, n, size=48):
    """n beams from the centre of a size^2 map: runs of equal end cells, invalid beams, short and long rays."""
    begin = (size // 2, size // 2)
    rays = []
    while len(rays) < n:
        kind = rng.integers(0, 10)
        if kind == 0:
            r = INVALID                       # NaN / out of map
        elif kind == 1:
            r = begin                         # begin == end: updateByScan skips it
        elif kind <= 3 and rays and rays[-1] not in (INVALID, begin):
            # a neighbour of the last end cell (dense coarse-level beams): often on the last ray's own walk
            r = (int(np.clip(rays[-1][0] + rng.integers(-1, 2), 0, size - 1)),
                 int(np.clip(rays[-1][1] + rng.integers(-1, 2), 0, size - 1)))
        else:
            r = (int(rng.integers(0, size)), int(rng.integers(0, size)))
        run = int(rng.integers(1, 5)) if rng.integers(0, 2) else 1
        rays += [INVALID if r == begin else r] * run
    return begin, rays[:n]


def test_random_scans():
    rng = np.random.default_rng(20260)
    dropped = 0
    for _ in range(300):
        n = int(rng.integers(1, 80))
        begin, rays = random_scan(rng, n)
        dropped += sum(r is not INVALID for r in rays) - check(begin, rays)
    assert dropped > 1000  # the scans did hold duplicates


def test_duplicated_end_cell_freed_by_a_lower_beam():
    """The run's end cell lies on an earlier beam's walk: its word is that beam's odd free event before and after."""
    begin = (10, 10)
    far, near = (30, 10), (20, 10)
    for rays in ([far, near, near, near], [far, INVALID, near, near], [near, near, far, near, near],
                 [far, near, near, far, far, near]):
        ev, hit = marks(begin, rays)
        if rays[0] == far:
            assert ev[near] == 1 and near in hit  # freed by beam 0 first, then hit
        check(begin, rays)
    # and freed by a later beam only: the word stays the first hit's even event
    ev, hit = marks(begin, survivors([near, near, near, far]))
    assert ev[near] == 0 and ev[far] == 2 and hit == {near, far}
    check(begin, [near, near, near, far])


def test_a_b_a_is_kept_and_exact():
    begin = (10, 10)
    a, b = (25, 14), (25, 15)
    rays = [a, b, a, b, b, a]
    assert survivors(rays) == [a, b, a, b, a]
    check(begin, rays)


def test_edges():
    begin = (5, 5)
    assert check(begin, []) == 0
    assert check(begin, [INVALID, INVALID]) == 0
    assert check(begin, [(9, 9)] * 70) == 1
    assert check(begin, [INVALID, (9, 9), INVALID, (9, 9), (9, 9), INVALID]) == 2

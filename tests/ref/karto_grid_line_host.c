/* tests/ref/karto_grid_line_host.c -- csrc/karto_grid_line.h compiled for the host, for
 * tests/test_karto_grid_cpu.py: the closed form's cells, and the cells kg_trace_kernel's per-tile walk emits
 * (clip to each tile, carries and error at the first step, then the incremental loop). */
#include "karto_grid_line.h"

/* every major step by the closed form; cells holds dx + 1 pairs */
int kglh_cells(int x0, int y0, int x1, int y1, int *cells)
{
    const kgl_line L = kgl_setup(x0, y0, x1, y1);
    for (int i = 0; i <= L.dx; i++) kgl_cell(&L, i, &cells[2 * i], &cells[2 * i + 1]);
    return L.dx + 1;
}

static int floordiv(int a, int b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }

/* one tile [tx0, tx1] x [ty0, ty1] as kg_trace_ray walks it: appends to cells[2 * n ..], returns the new count,
 * or -1 if a walked cell lies outside the tile */
static int walk_tile(const kgl_line *L, int tx0, int ty0, int tx1, int ty1, int *cells, int n)
{
    int ia, ib;
    if (!kgl_clip(L, tx0, ty0, tx1, ty1, &ia, &ib)) return n;
    int c = kgl_carry(L, ia);
    int err = kgl_error(L, ia, c);
    for (int k = ia; k <= ib; k++) {
        const int a = L->x0 + k, b = L->y0 + L->ystep * c;
        const int x = L->steep ? b : a, y = L->steep ? a : b;
        if (x < tx0 || x > tx1 || y < ty0 || y > ty1) return -1;
        cells[2 * n] = x;
        cells[2 * n + 1] = y;
        n++;
        err += L->dy;
        if (2 * err >= L->dx) {
            ++c;
            err -= L->dx;
        }
    }
    return n;
}

/* the cells of all tile x tile squares the ends' box meets, each walked as the kernel walks it; returns the
 * count, or -1 if a walked cell lies outside its tile */
int kglh_tiled_cells(int x0, int y0, int x1, int y1, int tile, int *cells)
{
    const kgl_line L = kgl_setup(x0, y0, x1, y1);
    const int bx0 = x0 < x1 ? x0 : x1, bx1 = x0 < x1 ? x1 : x0;
    const int by0 = y0 < y1 ? y0 : y1, by1 = y0 < y1 ? y1 : y0;
    int n = 0;
    for (int ty = floordiv(by0, tile); ty <= floordiv(by1, tile); ty++)
        for (int tx = floordiv(bx0, tile); tx <= floordiv(bx1, tile); tx++) {
            n = walk_tile(&L, tx * tile, ty * tile, tx * tile + tile - 1, ty * tile + tile - 1, cells, n);
            if (n < 0) return -1;
        }
    return n;
}

/* the cells kg_trace_kernel adds for one ray on a width x height map: the map's own tiles (the last ones cut at
 * the map's edge) with kg_trace_ray's box cull, for rays whose ends lie far off the map; cells holds
 * width + height pairs; returns the count or -1 as above */
int kglh_map_cells(int x0, int y0, int x1, int y1, int tile, int width, int height, int *cells)
{
    const kgl_line L = kgl_setup(x0, y0, x1, y1);
    const int bx0 = x0 < x1 ? x0 : x1, bx1 = x0 < x1 ? x1 : x0;
    const int by0 = y0 < y1 ? y0 : y1, by1 = y0 < y1 ? y1 : y0;
    int n = 0;
    for (int ty0 = 0; ty0 < height; ty0 += tile)
        for (int tx0 = 0; tx0 < width; tx0 += tile) {
            const int tx1 = (tx0 + tile < width ? tx0 + tile : width) - 1;
            const int ty1 = (ty0 + tile < height ? ty0 + tile : height) - 1;
            if (bx0 > tx1 || bx1 < tx0 || by0 > ty1 || by1 < ty0) continue;
            n = walk_tile(&L, tx0, ty0, tx1, ty1, cells, n);
            if (n < 0) return -1;
        }
    return n;
}

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
            const int tx0 = tx * tile, ty0 = ty * tile, tx1 = tx0 + tile - 1, ty1 = ty0 + tile - 1;
            int ia, ib;
            if (!kgl_clip(&L, tx0, ty0, tx1, ty1, &ia, &ib)) continue;
            int c = kgl_carry(&L, ia);
            int err = kgl_error(&L, ia, c);
            for (int k = ia; k <= ib; k++) {
                const int a = L.x0 + k, b = L.y0 + L.ystep * c;
                const int x = L.steep ? b : a, y = L.steep ? a : b;
                if (x < tx0 || x > tx1 || y < ty0 || y > ty1) return -1;
                cells[2 * n] = x;
                cells[2 * n + 1] = y;
                n++;
                err += L.dy;
                if (2 * err >= L.dx) {
                    ++c;
                    err -= L.dx;
                }
            }
        }
    return n;
}

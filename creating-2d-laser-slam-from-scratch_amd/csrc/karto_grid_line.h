/* karto_grid_line.h -- the integer line of open_karto's Grid<T>::TraceLine (Karto.h:4680-4745) in closed
 * form, for the host and the device (kg_trace_kernel, karto_grid_kernels.hip).
 *
 * TraceLine swaps the axes of a steep line, then the ends so that the major coordinate grows, and walks
 *     error += deltaY; if (2 * error >= deltaX) { y += ystep; error -= deltaX; }
 * AFTER it has emitted the point.  With c(i) the number of carries before major step i,
 *     -deltaX <= 2 * (i * deltaY - c(i) * deltaX) < deltaX
 * holds after every step, so c(i) = floor((2 * i * deltaY + deltaX) / (2 * deltaX)) and step i emits
 * (x0 + i, y0 + ystep * c(i)) in the swapped frame; deltaX == 0 is the single cell (x0, y0).
 * tests/test_karto_grid_cpu.py compares every function here with the literal loop.
 *
 * Arithmetic: the products reach 2 * deltaX^2.  Lines of at most KGL_SMALL major steps use 32-bit
 * unsigned division (2 * 32767 * 32768 < 2^32), longer ones 64-bit.  Callers keep |coordinate| < 2^30.
 */
#ifndef SLAM2D_CSRC_KARTO_GRID_LINE_H
#define SLAM2D_CSRC_KARTO_GRID_LINE_H

#if defined(__HIPCC__)
#define KGL_FN __host__ __device__ static inline
#else
#define KGL_FN static inline
#endif

#define KGL_SMALL 32767

typedef struct kgl_line {
    int x0, y0;    /* start in the swapped frame: major, minor */
    int dx, dy;    /* deltaX >= deltaY >= 0 */
    int ystep;     /* +1 / -1 */
    int steep;     /* the frame is (y, x) */
} kgl_line;

/* TraceLine's set-up up to the loop (:4682-4707) */
KGL_FN kgl_line kgl_setup(int x0, int y0, int x1, int y1)
{
    kgl_line L;
    const int adx = x1 > x0 ? x1 - x0 : x0 - x1, ady = y1 > y0 ? y1 - y0 : y0 - y1;
    int t;
    L.steep = ady > adx;
    if (L.steep) {
        t = x0, x0 = y0, y0 = t;
        t = x1, x1 = y1, y1 = t;
    }
    if (x0 > x1) {
        t = x0, x0 = x1, x1 = t;
        t = y0, y0 = y1, y1 = t;
    }
    L.x0 = x0;
    L.y0 = y0;
    L.dx = x1 - x0;
    L.dy = y1 > y0 ? y1 - y0 : y0 - y1;
    L.ystep = y0 < y1 ? 1 : -1;
    return L;
}

/* floor(a / b) for 0 <= a, 0 < b; `small` promises a, b < 2^32 */
KGL_FN long long kgl_div(long long a, long long b, int small)
{
    return small ? (long long)((unsigned)a / (unsigned)b) : a / b;
}

/* carries before major step i, 0 <= i <= dx */
KGL_FN int kgl_carry(const kgl_line *L, int i)
{
    if (L->dx == 0) return 0;
    return (int)kgl_div(2LL * i * L->dy + L->dx, 2LL * L->dx, L->dx <= KGL_SMALL);
}

/* the grid cell of major step i */
KGL_FN void kgl_cell(const kgl_line *L, int i, int *px, int *py)
{
    const int a = L->x0 + i, b = L->y0 + L->ystep * kgl_carry(L, i);
    *px = L->steep ? b : a;
    *py = L->steep ? a : b;
}

/* i * dy - c(i) * dx, the loop's `error` before step i */
KGL_FN int kgl_error(const kgl_line *L, int i, int c)
{
    return (int)((long long)i * L->dy - (long long)c * L->dx);
}

/* The major steps [*ia, *ib] whose cells lie in the rectangle [tx0, tx1] x [ty0, ty1] (grid frame,
 * inclusive): c(i) does not decrease with i, so they are one interval.  Returns 0 if there is none. */
KGL_FN int kgl_clip(const kgl_line *L, int tx0, int ty0, int tx1, int ty1, int *ia, int *ib)
{
    const long long M0 = L->steep ? ty0 : tx0, M1 = L->steep ? ty1 : tx1;
    const long long m0 = L->steep ? tx0 : ty0, m1 = L->steep ? tx1 : ty1;
    long long a = M0 - L->x0, b = M1 - L->x0;
    if (a < 0) a = 0;
    if (b > L->dx) b = L->dx;
    if (a > b) return 0;
    if (L->dy == 0) {
        if (L->y0 < m0 || L->y0 > m1) return 0;
    } else {
        /* y0 + ystep * c in [m0, m1]  <=>  c in [clo, chi] */
        long long clo = L->ystep > 0 ? m0 - L->y0 : L->y0 - m1;
        long long chi = L->ystep > 0 ? m1 - L->y0 : L->y0 - m0;
        const int small = L->dx <= KGL_SMALL;
        const long long dx = L->dx, dy2 = 2LL * L->dy;
        if (chi < 0 || clo > L->dy) return 0;
        if (chi > L->dy) chi = L->dy;
        if (clo > 0) { /* c(i) >= clo  <=>  2 i dy >= 2 dx clo - dx */
            const long long lo = kgl_div(2 * dx * clo - dx + dy2 - 1, dy2, small);
            if (lo > a) a = lo;
        }
        { /* c(i) <= chi  <=>  2 i dy < 2 dx (chi + 1) - dx */
            const long long hi = kgl_div(2 * dx * (chi + 1) - dx + dy2 - 1, dy2, small) - 1;
            if (hi < b) b = hi;
        }
        if (a > b) return 0;
    }
    *ia = (int)a;
    *ib = (int)b;
    return 1;
}

#endif

/* oracle/gmapping_overflow_check.c -- TEST INFRASTRUCTURE ONLY.
 *
 * Stand-alone host check of gmo_compute_map's point buffer (`make -C oracle asan-check` builds this file and
 * gmapping_oracle.c with -fsanitize=address and runs it): a 96 x 64-cell map and one 20 m beam, a 400-cell line
 * that leaves the map.  A point buffer sized from the map (2 (sx + sy + 8) points) was overrun by it in
 * gmo_grid_line.  Prints the counts and exits 0 when the sanitizer saw nothing. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

long long gmo_compute_map(double px, double py, double ct, double st, const float *ranges, int nbeams,
                          const double *a_cos, const double *a_sin, double max_range, double max_urange,
                          double xmin, double ymin, double xmax, double ymax, double delta, int32_t *n_out,
                          int32_t *visits_out, float *acc_out, int *num_hits, int *oob);

int main(void)
{
    const int sx = 96, sy = 64;
    float r[1] = {20.0f};
    double c[1] = {1.0}, s[1] = {0.0};
    int nh = 0, oob = 0;
    int32_t *n = calloc((size_t)sx * sy, sizeof(int32_t)), *v = calloc((size_t)sx * sy, sizeof(int32_t));
    float *a = calloc(2 * (size_t)sx * sy, sizeof(float));
    long long f = gmo_compute_map(0, 0, 1, 0, r, 1, c, s, 29.99, 25.0, -2.4, -1.6, 2.4, 1.6, 0.05, n, v, a, &nh, &oob);
    printf("gmapping_overflow_check: 96 x 64 map, one 20 m beam: nfree %lld hits %d outside %d\n", f, nh, oob);
    free(n); free(v); free(a);
    return (f == 48 && nh == 1 && oob == 353) ? 0 : 1;
}

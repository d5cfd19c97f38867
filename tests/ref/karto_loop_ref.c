/* tests/ref/karto_loop_ref.c -- CPU restatement of the Karto loop-closure and near-chain candidate search
 * (include/slam2d/karto_loop.h), the sequence the GPU is held to bit for bit.  Test infrastructure only.
 *
 * Reference: lesson6/lib/open_karto/src/Mapper.cpp (FindNearLinkedScans :1278-1286, FindPossibleLoopClosure
 * :1333-1394, FindNearChains :1170-1275, GetClosestScanToPose :1054-1073, LinkChainToScan :1152-1167), Mapper.h
 * (BreadthFirstTraversal::Traverse :568-612, NearScanVisitor :619-643) and Karto.h (LocalizedRangeScan::Update
 * :5362-5416).  The traversal is the reference's own queue; the two chain searches use the run formulations of
 * karto_loop.h, which tests/test_karto_loop_cpu.py checks against the literal transcription karto_loop_plain.py.
 * Build: gcc -O2 -ffp-contract=off (no FMA), csrc/detmath.h for sin / cos.
 */
#include <float.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "detmath.h"

#define KLR_TOLERANCE 1e-06 /* KT_TOLERANCE, Math.h:41 */

typedef struct klr_laser {
    double minimum_angle, angular_resolution, minimum_range, range_threshold;
    int n_readings, pad_;
} klr_laser;

/* Update()'s point readings of one scan: ok[i] = InRange(r, minimum_range, range_threshold); px, py where ok */
void klr_points(const klr_laser *L, const double *raw, const double *pose, double *px, double *py, unsigned char *ok)
{
    for (int i = 0; i < L->n_readings; i++) {
        double r = raw[i];
        ok[i] = (r >= L->minimum_range && r <= L->range_threshold) ? 1 : 0;
        px[i] = py[i] = 0.0;
        if (!ok[i]) continue;
        double angle = pose[2] + L->minimum_angle + (double)(uint32_t)i * L->angular_resolution;
        px[i] = pose[0] + (r * sdm_cos(angle));
        py[i] = pose[1] + (r * sdm_sin(angle));
    }
}

/* pairwise: 0 the reference's sequential sum; 1 a balanced pairwise (tree) sum, which the tests show to differ */
static double klr_tree(const double *v, int n)
{
    if (n == 1) return v[0];
    int h = n / 2;
    return klr_tree(v, h) + klr_tree(v + h, n - h);
}

int klr_reference(const klr_laser *L, int use_barycenter, int pairwise, int count, const double *ranges,
                  const double *poses, double *out)
{
    int n = L->n_readings;
    double *px = (double *)malloc(sizeof(double) * (size_t)n * 2);
    unsigned char *ok = (unsigned char *)malloc((size_t)n);
    if (!px || !ok) return -3;
    double *py = px + n;
    for (int s = 0; s < count; s++) {
        const double *pose = poses + 3 * (size_t)s;
        int cnt = 0;
        double sx = 0.0, sy = 0.0;
        if (use_barycenter) {
            klr_points(L, ranges + (size_t)s * n, pose, px, py, ok);
            for (int i = 0; i < n; i++) {
                if (!ok[i]) continue;
                if (pairwise) {
                    px[cnt] = px[i];
                    py[cnt] = py[i];
                } else {
                    sx = sx + px[i];
                    sy = sy + py[i];
                }
                cnt++;
            }
            if (pairwise && cnt > 0) {
                sx = klr_tree(px, cnt);
                sy = klr_tree(py, cnt);
            }
        }
        if (cnt > 0) {
            double np = (double)cnt;
            out[2 * s] = sx / np;
            out[2 * s + 1] = sy / np;
        } else {
            out[2 * s] = pose[0];
            out[2 * s + 1] = pose[1];
        }
    }
    free(px);
    free(ok);
    return 0;
}

/* Traverse with NearScanVisitor(maxDistance): visiting order into out, membership into linked[]; returns the count.
 * adj int[][2] = other end, edge index; entries outside the prefix (edge >= ne, vertex >= n) are skipped. */
static int klr_traverse(int n, int ne, const int *adj_off, const int *adj, const double *d2, int scan, double lo,
                        int *out, unsigned char *linked, int *queue, unsigned char *seen)
{
    int head = 0, tail = 0, nv = 0;
    memset(seen, 0, (size_t)n);
    memset(linked, 0, (size_t)n);
    queue[tail++] = scan;
    seen[scan] = 1;
    do {
        int v = queue[head++];
        if (d2[v] <= lo) {
            out[nv++] = v;
            linked[v] = 1;
            for (int j = adj_off[v]; j < adj_off[v + 1]; j++) {
                int u = adj[2 * j], e = adj[2 * j + 1];
                if (e >= ne || u >= n) continue;
                if (!seen[u]) {
                    queue[tail++] = u;
                    seen[u] = 1;
                }
            }
        }
    } while (head < tail);
    return nv;
}

/* counts[9]: n_near_link, n_near_loop, n_loop_chains, n_near_chains, loop_index_total, n_near_long,
 * near_index_total, and two diagnostics of the sweep: runs dropped by a near-linked scan, end-of-scans chains
 * shorter than min_chain.  loop_chains int[][4] = begin, length, resume, 0; near_chains int[][4] = begin, length,
 * closest, flags.  Returns 0, -1 for arguments out of range, -3 without memory. */
int klr_search(int n, int ne, const int *adj_off, const int *adj, const double *ref, int scan, int start_num,
               double link, double loop, int min_chain, double *d2, int *near_link, int *near_loop, int *loop_chains,
               int *near_chains, int *counts)
{
    memset(counts, 0, sizeof(int) * 9);
    if (n < 1 || scan < 0 || scan >= n || start_num < 0 || ne < 0) return -1;
    const double link_hi = link * link + KLR_TOLERANCE, link_lo = link * link - KLR_TOLERANCE;
    const double loop_hi = loop * loop + KLR_TOLERANCE, loop_lo = loop * loop - KLR_TOLERANCE;
    int *queue = (int *)malloc(sizeof(int) * (size_t)n * 3);
    unsigned char *seen = (unsigned char *)malloc((size_t)n * 3);
    if (!queue || !seen) return -3;
    int *first_pos = queue + n, *order = queue + 2 * n;
    unsigned char *in_link = seen + n, *in_loop = seen + 2 * n;
    for (int i = 0; i < n; i++) {
        double dx = ref[2 * i] - ref[2 * scan], dy = ref[2 * i + 1] - ref[2 * scan + 1];
        d2[i] = dx * dx + dy * dy;
    }
    const int nl = klr_traverse(n, ne, adj_off, adj, d2, scan, link_lo, near_link, in_link, queue, seen);
    const int no = klr_traverse(n, ne, adj_off, adj, d2, scan, loop_lo, near_loop, in_loop, queue, seen);
    counts[0] = nl;
    counts[1] = no;

    /* loop chains: maximal runs of A = in range and not near-linked over i >= start_num */
    int nc = 0;
    for (int i = start_num; i < n;) {
        if (!(d2[i] < loop_hi) || in_loop[i]) {
            i++;
            continue;
        }
        int b = i;
        while (i < n && d2[i] < loop_hi && !in_loop[i]) i++;
        int len = i - b;
        if (i == n || (!(d2[i] < loop_hi) && len >= min_chain)) {
            loop_chains[4 * nc] = b;
            loop_chains[4 * nc + 1] = len;
            loop_chains[4 * nc + 2] = i;
            loop_chains[4 * nc + 3] = 0;
            nc++;
            counts[4] += len;
            if (i == n && len < min_chain) counts[8]++;
        } else if (d2[i] < loop_hi) {
            counts[7]++;
        }
    }
    counts[2] = nc;

    /* near chains: the R-runs holding a near-linked scan other than the query, without the query's own run, in the
     * order of their first near-linked member in near_link */
    int nruns = 0;
    for (int k = 0; k < nl; k++) {
        int v = near_link[k];
        if (v == scan) continue;
        int b = v, e = v;
        while (b > 0 && d2[b - 1] < link_hi) b--;
        while (e + 1 < n && d2[e + 1] < link_hi) e++;
        int known = 0;
        for (int r = 0; r < nruns; r++)
            if (first_pos[r] == b) known = 1;
        if (known) continue;
        first_pos[nruns] = b;
        order[nruns] = e;
        nruns++;
    }
    int nn = 0;
    for (int r = 0; r < nruns; r++) {
        int b = first_pos[r], e = order[r];
        if (b <= scan && scan <= e) continue;
        int len = e - b + 1, closest = -1;
        double best = DBL_MAX;
        for (int i = b; i <= e; i++)
            if (d2[i] < best) {
                best = d2[i];
                closest = i;
            }
        int flags = (len >= min_chain ? 1 : 0) | ((closest >= 0 && best < link_hi) ? 2 : 0);
        near_chains[4 * nn] = b;
        near_chains[4 * nn + 1] = len;
        near_chains[4 * nn + 2] = closest;
        near_chains[4 * nn + 3] = flags;
        nn++;
        if (flags & 1) {
            counts[5]++;
            counts[6] += len;
        }
    }
    counts[3] = nn;
    free(queue);
    free(seen);
    return 0;
}

/* GetClosestScanToPose over scans [begin, begin + length) against scan's reference position, and LinkChainToScan's
 * test: out[0] = closest (or -1), out[1] = linked */
int klr_closest(int n, const double *ref, int scan, int begin, int length, double link, int *out)
{
    out[0] = -1;
    out[1] = 0;
    if (scan < 0 || scan >= n || begin < 0 || length < 1 || begin >= n || length > n - begin) return -1;
    double best = DBL_MAX;
    for (int i = begin; i < begin + length; i++) {
        double dx = ref[2 * scan] - ref[2 * i], dy = ref[2 * scan + 1] - ref[2 * i + 1];
        double d = dx * dx + dy * dy;
        if (d < best) {
            best = d;
            out[0] = i;
        }
    }
    if (out[0] >= 0 && best < link * link + KLR_TOLERANCE) out[1] = 1;
    return 0;
}

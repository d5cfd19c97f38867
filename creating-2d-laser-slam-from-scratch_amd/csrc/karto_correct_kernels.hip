// karto_correct_kernels.hip -- the HIP kernel of the Karto pose-correction stage (gfx950; the C-ABI is
// include/slam2d/karto_correct.h).  The work itself runs in the contexts' kernels (kl_refresh_kernel,
// kt_refresh_kernel, spa_solve_kernel, spa_export_kernel); this turns the stages' device records into their rows.
//   kc_flatten_kernel  one lane per record: the kl_refresh_row, for the refresh calls the row kt_refresh_device
//                      takes, for the correct call the optimiser's graph, and the stage's totals.  A record that names
//                      nothing gets graph -1, which every consumer passes over.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/slam2d/karto_correct.h"

namespace s2d {

constexpr int KC_THREADS = 256;

enum KcMode : int { KC_INTAKE, KC_JOBS, KC_CORRECT };

struct KcFlatten {
    const kp_intake *intake;      // KC_INTAKE: [count], record i of graph g_first + i
    const ke_job *jobs;           // KC_JOBS, KC_CORRECT: [count]
    const ke_closure *closures;   // [count], or NULL (KC_JOBS: every job row)
    const int *pool_offset;       // [n_graphs]
    kl_refresh_row *rows;         // [count]
    kl_refresh_span *spans;       // [count]: KC_INTAKE, KC_JOBS
    int *graph;                   // [count]: KC_CORRECT
    int *info;                    // scans named, graphs corrected, records refused
    int mode, g_first, count, n_graphs, max_scans;
};

__global__ void __launch_bounds__(KC_THREADS) kc_flatten_kernel(KcFlatten F)
{
    const int i = blockIdx.x * KC_THREADS + threadIdx.x;
    int named = 0, bad = 0;
    if (i < F.count) {
        int g = -1, scan = 0, slot = 0;
        if (F.mode == KC_INTAKE) {
            const kp_intake r = F.intake[i];
            if (r.accepted && r.status == KP_OK) {  // kp_plan_vertices' rule: the scan the intake added
                g = F.g_first + i;
                scan = r.scan;
                if (g < F.n_graphs) slot = F.pool_offset[g] + scan;
            }
        } else {
            const ke_job j = F.jobs[i];
            if (!F.closures || F.closures[i].chain >= 0) {
                g = j.graph;
                scan = j.scan;
                slot = j.pool_offset + scan;
            }
        }
        if (g >= F.n_graphs || (g >= 0 && F.mode != KC_CORRECT && (scan < 0 || scan >= F.max_scans))) {
            bad = 1;
            g = -1;
        }
        named = g >= 0;
        if (F.mode == KC_CORRECT) {
            F.rows[i] = kl_refresh_row{g, 0, -1, g >= 0 ? F.pool_offset[g] : 0};  // every scan of the graph
            F.graph[i] = g;
        } else {
            F.rows[i] = kl_refresh_row{g, scan, 1, slot};
            F.spans[i] = g >= 0 ? kl_refresh_span{slot, 1} : kl_refresh_span{0, 0};
        }
    }
    // counts only: integer sums are the same in any order
    const int names = __popcll(__ballot(named)), bads = __popcll(__ballot(bad));
    if ((threadIdx.x & 63) == 0) {
        if (names) atomicAdd(&F.info[F.mode == KC_CORRECT ? 1 : 0], names);
        if (bads) atomicAdd(&F.info[2], bads);
    }
}

}  // namespace s2d

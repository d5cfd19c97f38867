// graph_edit_device.h -- device helpers shared by the graph-edit kernels of the loop-search context
// (karto_loop_kernels.hip: kl_edit_*) and of the optimiser context (spa_kernels.hip: spa_edit_*).
//
// An edit call gets `count` rows, each naming its graph in its first int, and launches one workgroup of GE_THREADS
// lanes per row.  The workgroup of the FIRST row that names a graph is that graph's leader: it applies every row of the
// graph, in row order, with its wave 0, and then rebuilds the graph's lists with all its lanes.  The other workgroups
// leave at once.  So the work on one graph is sequential inside one workgroup, no atomic decides an order, and the cost
// grows with count and with the touched graphs' sizes only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace s2d {

constexpr int GE_THREADS = 256;
constexpr int GE_WAVES = GE_THREADS / 64;

// the graph of row j: the first int of a row of `stride` bytes
__device__ __forceinline__ int ge_row_graph(const void *rows, size_t stride, int j)
{
    return *(const int *)((const char *)rows + (size_t)j * stride);
}

// true in every lane when no row before `row` names graph g (all lanes of the workgroup call it)
__device__ inline bool ge_is_leader(const void *rows, size_t stride, int row, int g)
{
    int hit = 0;
    for (int j = threadIdx.x; j < row; j += GE_THREADS) hit |= ge_row_graph(rows, stride, j) == g;
    return !__syncthreads_or(hit);
}

// writes of this workgroup's lanes to global memory, ordered before its later reads (one wave, or after a barrier)
__device__ __forceinline__ void ge_fence()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// a refused row: the count, and the first refusal in (call, row) order -- a minimum over a key, so the same whatever
// order the workgroups run in.  info[0] = refused rows, info[1] = the key (all ones: none).
__device__ __forceinline__ void ge_refuse(unsigned long long *info, unsigned seq, int row, int status)
{
    atomicAdd(info, 1ull);
    atomicMin(info + 1, ((unsigned long long)seq << 40) | ((unsigned long long)(unsigned)row << 8) |
                            (unsigned long long)(unsigned)(-status & 0xff));
}

__device__ __forceinline__ int ge_wave_inscan(int v, int lane)
{
    for (int off = 1; off < 64; off <<= 1) {
        const int t = __shfl_up(v, off, 64);
        if (lane >= off) v += t;
    }
    return v;
}

// exclusive scan of v over the workgroup's lanes (sw: GE_WAVES ints of LDS); *total is the sum
__device__ inline int ge_block_exscan(int v, int *sw, int *total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int incl = ge_wave_inscan(v, lane);
    __syncthreads();
    if (lane == 63) sw[wave] = incl;
    __syncthreads();
    int base = 0, sum = 0;
    for (int w = 0; w < GE_WAVES; ++w) {
        if (w < wave) base += sw[w];
        sum += sw[w];
    }
    *total = sum;
    return base + incl - v;
}

// In-place exclusive scan of a[0 .. n) (LDS or global, written by this workgroup before a barrier); a[n] = the sum.
// Every lane takes one contiguous slice.
__device__ inline int ge_exscan_array(int *a, int n, int *sw)
{
    const int per = (n + GE_THREADS - 1) / GE_THREADS;
    const int k0 = min((int)threadIdx.x * per, n), k1 = min(k0 + per, n);
    int sum = 0;
    for (int k = k0; k < k1; ++k) sum += a[k];
    int total;
    int base = ge_block_exscan(sum, sw, &total);
    for (int k = k0; k < k1; ++k) {
        const int c = a[k];
        a[k] = base;
        base += c;
    }
    if (threadIdx.x == 0) a[n] = total;
    __threadfence_block();
    __syncthreads();
    return total;
}

// Stable bucket fill: items x = 0 .. items - 1 in order, item x belongs to bucket bucket_of(x) < n; off_out[k] is
// the first position of bucket k (off_out[n] = items) and emit(x, pos) gets the item's position: its bucket's offset
// plus the number of earlier items of the same bucket.  cur: n + 1 ints of LDS; s_b: GE_THREADS ints of LDS.  A
// chunk of GE_THREADS items is ranked by comparing bucket numbers, so nothing depends on the order the lanes run in;
// the atomics only count.
template <class BucketOf, class Emit>
__device__ inline void ge_bucket_fill(int n, int items, int *cur, int *s_b, int *sw, int *off_out, BucketOf bucket_of,
                                      Emit emit)
{
    const int t = threadIdx.x;
    for (int k = t; k <= n; k += GE_THREADS) cur[k] = 0;
    __syncthreads();
    for (int x = t; x < items; x += GE_THREADS) atomicAdd(&cur[bucket_of(x)], 1);
    __syncthreads();
    ge_exscan_array(cur, n, sw);
    for (int k = t; k <= n; k += GE_THREADS) off_out[k] = cur[k];
    for (int base = 0; base < items; base += GE_THREADS) {
        const int x = base + t;
        const int b = x < items ? bucket_of(x) : -1;
        s_b[t] = b;
        __syncthreads();
        if (b >= 0) {
            int r = 0;
            for (int j = 0; j < t; ++j) r += s_b[j] == b;
            emit(x, cur[b] + r);
        }
        __syncthreads();
        if (b >= 0) atomicAdd(&cur[b], 1);
        __syncthreads();
    }
}

}  // namespace s2d

// What the stages that read the finished, (TRACK_ID, POSITION_T)-ordered track table share (select.hip, evaluate.hip,
// plots.hip, violin.hip): grid-stride helpers, the workspace arena, rows -> track runs, the workgroup reduction.  Like
// prim.h: static kernels and inline host functions (static, too: the library exports the C ABI alone), one copy per
// translation unit.  Every kernel here and every user of block_reduce runs 256 threads a workgroup.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "common.h"
#include "prim.h"

namespace ysmr {
namespace table {

// ---- grid-stride loops over resident grids ------------------------------------------------------------------
__device__ __forceinline__ long long gtid() { return (long long)blockIdx.x * blockDim.x + threadIdx.x; }
__device__ __forceinline__ long long gstride() { return (long long)gridDim.x * blockDim.x; }
static inline unsigned resident_grid(long long items, int max_blocks)
{
    return (unsigned)std::max<long long>(1, std::min<long long>((items + 255) / 256, max_blocks));
}

// ---- workspace ----------------------------------------------------------------------------------------------
// Bump allocator in steps of 256 bytes.  A stage carves its buffers with one function; run on a null base, the same
// function gives the size (every pointer null, bytes() the total).
struct Arena {
    char *base;
    size_t at = 0;
    explicit Arena(void *workspace) : base((char *)workspace) {}
    template <class T> T *take(size_t count)
    {
        T *p = base ? (T *)(base + at) : nullptr;
        at += align_up(std::max<size_t>(count * sizeof(T), 1), 256);
        return p;
    }
    size_t bytes() const { return at; }
};

// ---- rows -> track runs -------------------------------------------------------------------------------------
// A track is one run of equal ids.  flag[i] = 1 on a run's first row; incl = inclusive scan of flag.
__device__ __forceinline__ bool is_run_start(const uint32_t *__restrict__ id, long long i) { return i == 0 || id[i] != id[i - 1]; }

static __global__ __launch_bounds__(256) void k_run_flags(const uint32_t *__restrict__ id, long long n, uint32_t *__restrict__ flag)
{
    for (long long i = gtid(); i < n; i += gstride()) flag[i] = is_run_start(id, i) ? 1u : 0u;
}

// seg[i] = number of row i's run (seg == incl allowed: a row touches its own entry only); first / last row of every
// run below n_tracks_cap (UINT32_MAX: all of them).  Rows of the runs beyond the cap still get their seg.  last may
// be null.
static __global__ __launch_bounds__(256) void k_run_index(const uint32_t *__restrict__ flag, const uint32_t *incl, long long n,
                                                          uint32_t *seg, uint32_t *__restrict__ first, uint32_t *__restrict__ last,
                                                          uint32_t n_tracks_cap)
{
    for (long long i = gtid(); i < n; i += gstride()) {
        const uint32_t s = incl[i] - 1u;
        seg[i] = s;
        if (s >= n_tracks_cap) continue;
        if (flag[i]) first[s] = (uint32_t)i;
        if (last && (i == n - 1 || flag[i + 1])) last[s] = (uint32_t)i;
    }
}

// flags, scan, index over n >= 1 rows; seg[n - 1] + 1 is the number of runs.  scan_temp: prim::scan_temp_words(n) u32
static inline void index_runs(hipStream_t st, unsigned grid, const uint32_t *id, long long n, uint32_t *flag, uint32_t *seg,
                              uint32_t *first, uint32_t *last, uint32_t n_tracks_cap, uint32_t *scan_temp)
{
    hipLaunchKernelGGL(k_run_flags, dim3(grid), dim3(256), 0, st, id, n, flag);
    prim::inclusive_scan_u32(st, flag, seg, (size_t)n, scan_temp);
    hipLaunchKernelGGL(k_run_index, dim3(grid), dim3(256), 0, st, (const uint32_t *)flag, (const uint32_t *)seg, n, seg, first, last,
                       n_tracks_cap);
}

// ---- workgroup reduction ------------------------------------------------------------------------------------
// op over the 256 threads' values by a tree over s[256], in a fixed order (floating-point sums give the same bits on
// every run); every thread gets the result, and s is free again on return
template <class T, class Op> __device__ __forceinline__ T block_reduce(T v, T *s, Op op)
{
    s[threadIdx.x] = v;
    __syncthreads();
    for (int d = 128; d > 0; d >>= 1) {
        if ((int)threadIdx.x < d) s[threadIdx.x] = op(s[threadIdx.x], s[threadIdx.x + d]);
        __syncthreads();
    }
    const T r = s[0];
    __syncthreads();
    return r;
}
struct Sum { template <class T> __device__ T operator()(T a, T b) const { return a + b; } };
struct Min { template <class T> __device__ T operator()(T a, T b) const { return b < a ? b : a; } };
struct Max { template <class T> __device__ T operator()(T a, T b) const { return a < b ? b : a; } };

}  // namespace table
}  // namespace ysmr

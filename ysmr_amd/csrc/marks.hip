// marks.hip -- the marks of a whole annotated video built ON THE DEVICE from the columns of the evaluated table: what
// annotate.build_marks does on the host (filter, truncate, stable sort by frame, searchsorted), the same bytes, for
// ysmr_annotate_batch to paint.  marks_rule.h holds the row rule.  Four launches and a radix sort on the caller's stream:
//   k_marks_keys    a row per lane: the 64-bit key (frame above id; all ones for a row that is dropped) and the row number.
//                   "Table order" is get_data's: by track exactly when upstream's rough check on the first six ids says so --
//                   every lane reads those six ids itself (the same addresses across the launch), so no launch waits for a flag
//   radix_sort      prim.h: stable, least significant digit first, only over the bits that n_frames needs
//   k_marks_gather  output slot i takes the row whose key came i-th: its mark, or zeros behind the last kept row
//   k_marks_first   first[f] = lower bound of (f << 32) among the sorted keys, a frame per lane
// No atomics: the order comes from the keys and the row numbers alone, two calls give the same bytes.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "common.h"
#include "prim.h"
#include "csv_plan.h"
#include "marks_rule.h"

static_assert(csvp::RADIX_TILE == ysmr::prim::RADIX_TILE && csvp::SCAN_TILE == ysmr::prim::SCAN_TILE, "csv_plan.h restates prim.h");

namespace {

namespace mk = ysmr::marks;

struct TableColumns {
    const uint32_t *id;
    const int64_t *t;
    const double *x, *y;
    const int8_t *moving, *turn;
    const double *phenotype;        // NULL: every subtype
};

__global__ __launch_bounds__(256) void k_marks_keys(TableColumns c, long long n, int n_frames, int subtype, int sort_rule,
                                                    unsigned long long *__restrict__ keys, uint32_t *__restrict__ idx)
{
    const bool by_track = sort_rule == 1 || (sort_rule == 2 && mk::first_ids_distinct(c.id, n));
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const int64_t t = c.t[i];
        const bool keep = mk::kept(c.x[i], c.y[i], t, n_frames, c.phenotype != nullptr, c.phenotype ? c.phenotype[i] : 0.0, subtype);
        keys[i] = keep ? mk::sort_key(t, c.id[i], by_track) : mk::KEY_DROPPED;
        idx[i] = (uint32_t)i;
    }
}

__global__ __launch_bounds__(256) void k_marks_gather(TableColumns c, long long n, const unsigned long long *__restrict__ keys,
                                                      const uint32_t *__restrict__ idx, ysmr_mark *__restrict__ marks)
{
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        ysmr_mark m{0, 0, 0u, 0u};
        if (keys[i] != mk::KEY_DROPPED) {
            const uint32_t row = idx[i];
            m = mk::mark_of_row(c.x[row], c.y[row], c.id[row], c.moving[row], c.turn[row]);
        }
        marks[i] = m;
    }
}

// (the dropped rows' keys lie above every frame's: first[n_frames] is the number of marks)
__global__ __launch_bounds__(256) void k_marks_first(const unsigned long long *__restrict__ keys, long long n, int n_frames,
                                                     long long *__restrict__ first)
{
    for (long long f = (long long)blockIdx.x * 256 + threadIdx.x; f <= n_frames; f += (long long)gridDim.x * 256) {
        const unsigned long long bound = (unsigned long long)f << 32;
        long long lo = 0, hi = n;                                 // keys[lo - 1] < bound <= keys[hi]
        while (lo < hi) {
            const long long mid = lo + (hi - lo) / 2;
            if (keys[mid] < bound) lo = mid + 1; else hi = mid;
        }
        first[f] = lo;
    }
}

bool sizes_served(long long n_rows, int n_frames) { return n_rows >= 0 && n_rows <= csvp::MAX_ROWS && n_frames >= 1 && n_frames <= 0x7FFFFFFE; }

}  // namespace

extern "C" {

size_t ysmr_marks_workspace_bytes(long long n_rows, int n_frames)
{
    if (!sizes_served(n_rows, n_frames)) return 0;
    if (n_rows == 0) return 256;
    csvp::OrderPlan p;                  // keys and row numbers, both twice, and the radix passes' histograms: ysmr_csv_order's
    return csvp::order_plan_of(n_rows, p) ? p.total : 0;
}

int ysmr_marks_build(void *stream, long long n_rows, const uint32_t *track_id_dev, const int64_t *t_dev, const double *x_dev,
                     const double *y_dev, const int8_t *moving_dev, const int8_t *turn_points_dev, const double *phenotype_dev,
                     int subtype, int n_frames, int sort_rule, void *workspace_dev, size_t workspace_bytes, ysmr_mark *marks_dev,
                     int64_t *first_dev)
{
    if (!sizes_served(n_rows, n_frames))
        return ysmr::fail(YSMR_ERR_ARG, "n_rows must be in 0..2^31-1 and n_frames in 1..2^31-2, got %lld and %d", n_rows, n_frames);
    if (sort_rule < 0 || sort_rule > 2) return ysmr::fail(YSMR_ERR_ARG, "sort_rule must be 0 (file order), 1 (by track) or 2 (rough check), got %d", sort_rule);
    if (!first_dev) return ysmr::fail(YSMR_ERR_ARG, "first_dev must be set");
    hipStream_t st = (hipStream_t)stream;
    if (n_rows == 0) {
        YSMR_HIP_CHECK(hipMemsetAsync(first_dev, 0, sizeof(int64_t) * ((size_t)n_frames + 1), st));
        return YSMR_OK;
    }
    if (!track_id_dev || !t_dev || !x_dev || !y_dev || !moving_dev || !turn_points_dev || !marks_dev || !workspace_dev)
        return ysmr::fail(YSMR_ERR_ARG, "the six columns, marks_dev and workspace_dev must be set");
    csvp::OrderPlan p;
    if (!csvp::order_plan_of(n_rows, p)) return ysmr::fail(YSMR_ERR_ARG, "a workspace for %lld rows does not fit", n_rows);
    if (workspace_bytes < p.total) return ysmr::fail(YSMR_ERR_CAPACITY, "marks workspace too small: %zu < %zu bytes", workspace_bytes, p.total);
    if ((uintptr_t)workspace_dev & 15u) return ysmr::fail(YSMR_ERR_ARG, "workspace_dev must be 16-byte aligned");
    char *w = (char *)workspace_dev;
    auto *keys_a = (unsigned long long *)(w + p.keys_a), *keys_b = (unsigned long long *)(w + p.keys_b);
    auto *idx_a = (uint32_t *)(w + p.idx_a), *idx_b = (uint32_t *)(w + p.idx_b);
    const TableColumns c{track_id_dev, t_dev, x_dev, y_dev, moving_dev, turn_points_dev, phenotype_dev};
    const unsigned grid = (unsigned)std::min<long long>((n_rows + 255) / 256, 1024);
    hipLaunchKernelGGL(k_marks_keys, dim3(grid), dim3(256), 0, st, c, n_rows, n_frames, subtype, sort_rule, keys_a, idx_a);
    const int where = ysmr::prim::radix_sort(st, keys_a, keys_b, idx_a, idx_b, (size_t)n_rows, mk::key_bits(n_frames), w + p.temp);
    const unsigned long long *keys = where ? keys_b : keys_a;
    hipLaunchKernelGGL(k_marks_gather, dim3(grid), dim3(256), 0, st, c, n_rows, keys, (const uint32_t *)(where ? idx_b : idx_a), marks_dev);
    hipLaunchKernelGGL(k_marks_first, dim3((unsigned)std::min<long long>(((long long)n_frames + 256) / 256, 1024)), dim3(256), 0, st, keys, n_rows,
                       n_frames, (long long *)first_dev);
    YSMR_LAUNCH_CHECK();
    return YSMR_OK;
}

}  // extern "C"

// violin.hip -- the violin plots of evaluate_tracks (ysmr/plot_functions.py:260-370, track_eval.py:1151-1303): the split of
// the tracks into categories, per-violin order statistics and moments, seaborn's Gaussian kernel density estimate
// (cut=0, bw=.2, gridsize=100, scale='count', width=.95) and the painter.  The reference pays seaborn and matplotlib for
// this; here the two columns go to HBM, the numbers come from the kernels below and the canvas is painted as a function
// of the pixel.  The rules are stated as a NumPy model in tests/violin_model.py ("The figures"):
//   * every track yields two entries (value, violin): one for 'All' (violin 0), one for the LAST interval k with
//     lo_k <= c and c < hi_k (violin k + 1); an entry whose value is not finite, or that has no interval, gets violin 255
//     and sorts behind everything.  A stable radix sort by value and then by violin leaves every violin's finite values
//     as one ascending run;
//   * sums run in a fixed order -- lane l adds x_l, x_{l+256}, ... of the sorted run, then a tree over the 256 lanes --
//     and nothing is accumulated with floating-point atomics: two calls give the same bytes;
//   * the painter's only floating-point step is the profile kernel (one half width per axes row and violin, and the rows
//     of the quartiles and whiskers); the paint kernel decides every pixel from those integers.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>

#include "common.h"
#include "plot_lut.h"
#include "prim.h"
#include "table.h"

namespace {

constexpr int VI_GRID = YSMR_VIOLIN_GRID;
constexpr int VI_NONE = 255;             // the violin of an entry that counts nowhere
constexpr int VI_BLOCKS = 512;
constexpr int VI_MARKS = 8;              // per violin: kind, rows of q50, q25, q75, whisker_lo, whisker_hi, the line, spare
constexpr double VI_SQRT_2PI = 2.5066282746310002;
constexpr double VI_ROW_CLAMP = 1048576.0;   // rows are kept within 2^20 of the axes: enough to be "far outside", safe as int

__constant__ uint8_t c_fill[30] = {YSMR_VIOLIN_FILL_U8};

using namespace ysmr::table;   // (block_reduce with Sum: the 256 lanes' values in a fixed order, a tree over LDS)

using ysmr::prim::key_of;      // doubles as u64 keys of the same order: the radix sort's keys
using ysmr::prim::value_of;
using ysmr::prim::finite64;

// ---- categories --------------------------------------------------------------------------------------------------------

// counts: members[256] then values[256] (u32; integer atomics: the result does not depend on the order)
__global__ __launch_bounds__(256) void k_vi_keys(long long n, const double *__restrict__ cut, long long cut_stride,
                                                 const double *__restrict__ val, long long val_stride, int n_cuts,
                                                 const double *__restrict__ lo, const double *__restrict__ hi,
                                                 unsigned long long *__restrict__ keys, uint32_t *__restrict__ ids,
                                                 uint32_t *__restrict__ counts)
{
    __shared__ double s_lo[YSMR_VIOLIN_MAX_CUTS], s_hi[YSMR_VIOLIN_MAX_CUTS];
    __shared__ uint32_t s_cnt[512];
    for (int k = threadIdx.x; k < n_cuts; k += 256) { s_lo[k] = lo[k]; s_hi[k] = hi[k]; }
    for (int k = threadIdx.x; k < 512; k += 256) s_cnt[k] = 0;
    __syncthreads();
    // (a block meets at most 2^30 / gridDim.x tracks: the 32-bit LDS counters cannot wrap)
    for (long long t = gtid(); t < n; t += gstride()) {
        const double c = cut[t * cut_stride], v = val[t * val_stride];
        int cat = 0;
        for (int k = 0; k < n_cuts; ++k)
            if (s_lo[k] <= c && c < s_hi[k]) cat = k + 1;
        const bool fin = finite64(v);
        const unsigned long long key = key_of(v);
        keys[2 * t] = key;
        keys[2 * t + 1] = key;
        ids[2 * t] = fin ? 0u : (uint32_t)VI_NONE;
        ids[2 * t + 1] = (fin && cat) ? (uint32_t)cat : (uint32_t)VI_NONE;
        atomicAdd(&s_cnt[0], 1u);
        if (fin) atomicAdd(&s_cnt[256], 1u);
        if (cat) {
            atomicAdd(&s_cnt[cat], 1u);
            if (fin) atomicAdd(&s_cnt[256 + cat], 1u);
        }
    }
    __syncthreads();
    for (int k = threadIdx.x; k < 512; k += 256)
        if (s_cnt[k]) atomicAdd(&counts[k], s_cnt[k]);
}

// ---- summaries ---------------------------------------------------------------------------------------------------------

// one workgroup per violin; sorted: every violin's finite values ascending, the violins one after the other
__global__ __launch_bounds__(256) void k_vi_summary(const unsigned long long *__restrict__ sorted, const uint32_t *__restrict__ counts,
                                                    uint32_t *__restrict__ start_out, ysmr_violin_summary *__restrict__ out)
{
    __shared__ double s_red[256];
    const int v = blockIdx.x;
    uint32_t start = 0;
    for (int u = 0; u < v; ++u) start += counts[256 + u];
    const uint32_t n = counts[256 + v];
    const unsigned long long *x = sorted + start;

    double acc = 0.0;
    for (uint32_t i = threadIdx.x; i < n; i += 256) acc = acc + value_of(x[i]);
    const double total = block_reduce(acc, s_red, Sum());
    const double mean = n ? total / (double)n : 0.0;
    acc = 0.0;
    for (uint32_t i = threadIdx.x; i < n; i += 256) {
        const double d = value_of(x[i]) - mean;
        acc = acc + d * d;
    }
    const double ss = block_reduce(acc, s_red, Sum());
    if (threadIdx.x != 0) return;

    ysmr_violin_summary s;
    s.members = (long long)counts[v];
    s.values = (long long)n;
    s.vmin = s.vmax = s.q25 = s.q50 = s.q75 = s.whisker_lo = s.whisker_hi = s.mean = s.h = 0.0;
    if (n) {
        s.vmin = value_of(x[0]);
        s.vmax = value_of(x[n - 1]);
        double q[3];
        for (int k = 0; k < 3; ++k) {
            const double pos = (0.25 * (double)(k + 1)) * (double)(n - 1);
            const double fl = floor(pos);
            const uint32_t i0 = (uint32_t)fl, i1 = std::min(i0 + 1u, n - 1u);
            const double t = pos - fl, a = value_of(x[i0]), b = value_of(x[i1]);
            q[k] = t < 0.5 ? a + (b - a) * t : b - (b - a) * (1.0 - t);
        }
        s.q25 = q[0]; s.q50 = q[1]; s.q75 = q[2];
        const double iqr = s.q75 - s.q25;
        const double fence_lo = s.q25 - 1.5 * iqr, fence_hi = s.q75 + 1.5 * iqr;
        // the first value >= fence_lo, the last <= fence_hi (fence_lo <= q25 <= a value, fence_hi >= q75 >= a value)
        uint32_t a = 0, b = n;
        while (a < b) {
            const uint32_t mid = a + (b - a) / 2;
            if (value_of(x[mid]) >= fence_lo) b = mid; else a = mid + 1;
        }
        s.whisker_lo = value_of(x[std::min(a, n - 1u)]);
        a = 0; b = n;
        while (a < b) {
            const uint32_t mid = a + (b - a) / 2;
            if (value_of(x[mid]) <= fence_hi) a = mid + 1; else b = mid;
        }
        s.whisker_hi = value_of(x[a ? a - 1u : 0u]);
        s.mean = mean;
        s.h = n >= 2 ? 0.2 * sqrt(ss / (double)(n - 1)) : 0.0;
    }
    out[v] = s;
    start_out[v] = start;
}

// ---- density -----------------------------------------------------------------------------------------------------------

// one workgroup per (grid point, violin)
__global__ __launch_bounds__(256) void k_vi_density(const unsigned long long *__restrict__ sorted, const uint32_t *__restrict__ start,
                                                    const ysmr_violin_summary *__restrict__ sum, double *__restrict__ density)
{
    __shared__ double s_red[256];
    const int j = blockIdx.x, v = blockIdx.y;
    const ysmr_violin_summary s = sum[v];
    const uint32_t n = (uint32_t)s.values;
    if (n < 2 || !(s.h > 0.0)) {            // (the whole workgroup alike)
        if (threadIdx.x == 0) density[(size_t)v * VI_GRID + j] = 0.0;
        return;
    }
    const unsigned long long *x = sorted + start[v];
    const double step = (s.vmax - s.vmin) / (double)(VI_GRID - 1);
    const double g = j == VI_GRID - 1 ? s.vmax : s.vmin + (double)j * step;
    double acc = 0.0;
    for (uint32_t i = threadIdx.x; i < n; i += 256) {
        const double z = (g - value_of(x[i])) / s.h;
        acc = acc + exp(-0.5 * z * z);
    }
    const double total = block_reduce(acc, s_red, Sum());
    if (threadIdx.x == 0) {
        const double norm = 1.0 / ((double)n * s.h * VI_SQRT_2PI);
        density[(size_t)v * VI_GRID + j] = norm * total;
    }
}

// ---- the painter -------------------------------------------------------------------------------------------------------

struct ViView {                 // ysmr_violin_view as the kernels use it
    double y0, upp;
    int W, H, ax_x, ax_y, ax_w, ax_h, n, n_rows, line_half, box_half, dot_r2;
    int grid_rows[32], slot_x[YSMR_VIOLIN_MAX_SLOTS], slot_w[YSMR_VIOLIN_MAX_SLOTS], slot_colour[YSMR_VIOLIN_MAX_SLOTS];
};

__device__ __forceinline__ int row_of(double value, const ViView &v)
{
    double f = floor((value - v.y0) / v.upp);
    if (!(f >= -VI_ROW_CLAMP)) f = -VI_ROW_CLAMP;        // (NaN as well)
    if (f > VI_ROW_CLAMP) f = VI_ROW_CLAMP;
    return v.ax_h - 1 - (int)f;
}

// one workgroup per violin: the half width of every axes row, and the rows of the marks
__global__ __launch_bounds__(256) void k_vi_profile(const ysmr_violin_summary *__restrict__ sum, const double *__restrict__ density,
                                                    ViView v, int *__restrict__ prof, int *__restrict__ marks)
{
    const int w = blockIdx.x;
    const ysmr_violin_summary s = sum[w];
    long long max_values = 0;
    for (int u = 0; u < v.n; ++u)
        if (v.slot_w[u] > 0) max_values = std::max(max_values, sum[u].values);
    const double *d = density + (size_t)w * VI_GRID;
    double peak = 0.0;
    for (int j = 0; j < VI_GRID; ++j) peak = std::max(peak, d[j]);
    const bool drawn = v.slot_w[w] > 0 && s.values > 0;
    const bool line = drawn && (s.values == 1 || !(s.h > 0.0));
    const bool body = drawn && !line && peak > 0.0 && s.vmax > s.vmin;
    const double step = (s.vmax - s.vmin) / (double)(VI_GRID - 1);
    for (int r = threadIdx.x; r < v.ax_h; r += 256) {
        int half = -1;
        const double y = v.y0 + ((double)(v.ax_h - 1 - r) + 0.5) * v.upp;
        if (body && y >= s.vmin && y <= s.vmax) {
            const double p = (y - s.vmin) / step;
            int j = (int)floor(p);
            j = std::max(0, std::min(j, VI_GRID - 2));
            const double t = p - (double)j;
            const double dd = d[j] + (d[j + 1] - d[j]) * t;
            double a = dd / peak;
            a = a * (double)s.values;
            a = a / (double)max_values;
            a = a * 0.95;
            a = a * (double)v.slot_w[w];
            a = a / 2.0;
            a = floor(a);
            half = a >= 0.0 ? (int)std::min(a, 65536.0) : -1;
        }
        prof[(size_t)w * v.ax_h + r] = half;
    }
    if (threadIdx.x == 0) {
        int *m = marks + w * VI_MARKS;
        m[0] = body ? 1 : line ? 2 : 0;
        m[1] = row_of(s.q50, v);
        m[2] = row_of(s.q25, v);
        m[3] = row_of(s.q75, v);
        m[4] = row_of(s.whisker_lo, v);
        m[5] = row_of(s.whisker_hi, v);
        m[6] = row_of(s.vmin, v);
        m[7] = 0;
    }
}

// is axes pixel (ac, ar) of violin w's fill?  (columns and rows relative to the axes' top-left pixel)
__device__ __forceinline__ bool vi_fill(const int *__restrict__ prof, const ViView &v, int w, int ac, int ar)
{
    const int sx = v.slot_x[w] - v.ax_x;
    if (ar < 0 || ar >= v.ax_h || ac < sx || ac >= sx + v.slot_w[w]) return false;
    const int dx = ac - (sx + v.slot_w[w] / 2);
    return (dx < 0 ? -dx : dx) <= prof[(size_t)w * v.ax_h + ar];
}

__global__ __launch_bounds__(256) void k_vi_paint(const int *__restrict__ prof, const int *__restrict__ marks, ViView v,
                                                  uint8_t *__restrict__ rgb)
{
    const long long pixels = (long long)v.W * v.H;
    for (long long p = gtid(); p < pixels; p += gstride()) {
        const int row = (int)(p / v.W), col = (int)(p - (long long)row * v.W);
        const int ac = col - v.ax_x, ar = row - v.ax_y;
        int cr = 255, cg = 255, cb = 255;
        if (ac >= 0 && ac < v.ax_w && ar >= 0 && ar < v.ax_h) {
            bool grid = false;
            for (int k = 0; k < v.n_rows; ++k) grid |= v.grid_rows[k] == row;
            if (grid) cr = cg = cb = 176;
            int w = -1;
            for (int u = v.n - 1; u >= 0; --u)
                if (v.slot_w[u] > 0 && col >= v.slot_x[u] && col < v.slot_x[u] + v.slot_w[u]) w = u;     // the lowest such u
            const int kind = w >= 0 ? marks[w * VI_MARKS] : 0;
            if (kind) {
                const int *m = marks + w * VI_MARKS;
                const int dx = ac - (v.slot_x[w] - v.ax_x + v.slot_w[w] / 2), adx = dx < 0 ? -dx : dx;
                if (kind == 1) {
                    if (vi_fill(prof, v, w, ac, ar)) {
                        const bool inner = vi_fill(prof, v, w, ac - 1, ar) && vi_fill(prof, v, w, ac + 1, ar) &&
                                           vi_fill(prof, v, w, ac, ar - 1) && vi_fill(prof, v, w, ac, ar + 1);
                        if (inner) {
                            const int e = 3 * (int)((unsigned)v.slot_colour[w] % 10u);
                            cr = c_fill[e]; cg = c_fill[e + 1]; cb = c_fill[e + 2];
                        } else {
                            cr = cg = cb = 76;
                        }
                    }
                    if (adx <= v.line_half && ar >= m[5] && ar <= m[4]) cr = cg = cb = 76;
                    if (adx <= v.box_half && ar >= m[3] && ar <= m[2]) cr = cg = cb = 76;
                    const long long dy = (long long)ar - m[1];
                    if ((long long)dx * dx + dy * dy <= (long long)v.dot_r2) cr = cg = cb = 255;
                } else {
                    const int dy = ar - m[6];
                    if (adx <= v.slot_w[w] * 95 / 200 && (dy < 0 ? -dy : dy) <= v.line_half) cr = cg = cb = 76;
                }
            }
        }
        if ((ac == -1 && ar >= 0 && ar <= v.ax_h) || (ar == v.ax_h && ac >= -1 && ac < v.ax_w)) cr = cg = cb = 0;
        uint8_t *o = rgb + 3 * (size_t)p;
        o[0] = (uint8_t)cr; o[1] = (uint8_t)cg; o[2] = (uint8_t)cb;
    }
}

struct ViWork {
    unsigned long long *keys_a, *keys_b;
    uint32_t *ids_a, *ids_b, *counts, *start;
    void *temp;                 // of the radix sorts
    int *prof, *marks;
};

// ysmr_violin_stats carves (n_tracks, n_violins, 0) and uses the buffers in front of prof, ysmr_plot_violins carves
// (0, n_violins, ax_h) and uses prof and marks
ViWork vi_carve(Arena &a, long long n_tracks, int n_violins, int ax_h)
{
    ViWork k{};
    const size_t entries = 2 * (size_t)n_tracks;
    k.keys_a = a.take<unsigned long long>(entries);
    k.keys_b = a.take<unsigned long long>(entries);
    k.ids_a = a.take<uint32_t>(entries);
    k.ids_b = a.take<uint32_t>(entries);
    k.counts = a.take<uint32_t>(512);
    k.start = a.take<uint32_t>(256);
    k.temp = a.take<char>(ysmr::prim::radix_temp_bytes(entries));
    k.prof = a.take<int>((size_t)n_violins * (size_t)ax_h);
    k.marks = a.take<int>((size_t)n_violins * VI_MARKS);
    return k;
}

bool vi_sizes_ok(long long n_tracks, int n_violins, int ax_h)
{
    return n_tracks >= 0 && n_tracks <= (1ll << 30) && n_violins >= 1 && n_violins <= YSMR_VIOLIN_MAX_CUTS + 1 && ax_h >= 0 && ax_h <= 32768;
}

}  // namespace

extern "C" {

size_t ysmr_violin_workspace_bytes(long long n_tracks, int n_violins, int ax_h)
{
    if (!vi_sizes_ok(n_tracks, n_violins, ax_h)) return 0;
    Arena sizing(nullptr);
    vi_carve(sizing, n_tracks, n_violins, ax_h);
    return sizing.bytes();
}

int ysmr_violin_stats(void *stream, long long n_tracks, const double *cut_dev, long long cut_stride, const double *value_dev,
                      long long value_stride, int n_cuts, const double *lo_dev, const double *hi_dev, void *workspace_dev,
                      size_t workspace_bytes, ysmr_violin_summary *summaries_dev, double *density_dev)
{
    if (n_cuts < 0 || n_cuts > YSMR_VIOLIN_MAX_CUTS) return ysmr::fail(YSMR_ERR_ARG, "n_cuts must be in 0..%d, got %d", YSMR_VIOLIN_MAX_CUTS, n_cuts);
    if (n_tracks < 0 || n_tracks > (1ll << 30)) return ysmr::fail(YSMR_ERR_ARG, "n_tracks must be in 0..2^30, got %lld", n_tracks);
    if (!workspace_dev || !summaries_dev || !density_dev) return ysmr::fail(YSMR_ERR_ARG, "workspace_dev, summaries_dev and density_dev must not be NULL");
    if (n_tracks > 0 && (!cut_dev || !value_dev || cut_stride < 1 || value_stride < 1))
        return ysmr::fail(YSMR_ERR_ARG, "cut_dev and value_dev must not be NULL and their strides >= 1");
    if (n_cuts > 0 && (!lo_dev || !hi_dev)) return ysmr::fail(YSMR_ERR_ARG, "lo_dev and hi_dev must not be NULL");
    if (((uintptr_t)workspace_dev & 7) || ((uintptr_t)summaries_dev & 7) || ((uintptr_t)density_dev & 7))
        return ysmr::fail(YSMR_ERR_ARG, "workspace_dev, summaries_dev and density_dev must be 8-byte aligned");
    const int n_violins = n_cuts + 1;
    Arena arena(workspace_dev);
    const ViWork k = vi_carve(arena, n_tracks, n_violins, 0);
    if (workspace_bytes < arena.bytes())
        return ysmr::fail(YSMR_ERR_CAPACITY, "violin workspace too small: %zu < %zu bytes", workspace_bytes, arena.bytes());
    hipStream_t st = (hipStream_t)stream;
    unsigned long long *keys_a = k.keys_a, *keys_b = k.keys_b;
    uint32_t *ids_a = k.ids_a, *ids_b = k.ids_b, *counts = k.counts, *start = k.start;
    const size_t entries = 2 * (size_t)n_tracks;

    YSMR_HIP_CHECK(hipMemsetAsync(counts, 0, 4 * 512, st));
    const unsigned long long *sorted = keys_a;
    if (n_tracks > 0) {
        hipLaunchKernelGGL(k_vi_keys, dim3(resident_grid(n_tracks, VI_BLOCKS)), dim3(256), 0, st, n_tracks, cut_dev, cut_stride, value_dev, value_stride,
                           n_cuts, lo_dev, hi_dev, keys_a, ids_a, counts);
        // by value (eight passes: back in the a buffers), then by violin (one pass, stable: into the b buffers)
        const int where = ysmr::prim::radix_sort<unsigned long long, uint32_t>(st, keys_a, keys_b, ids_a, ids_b, entries, 64, k.temp);
        unsigned long long *k_in = where ? keys_b : keys_a, *k_out = where ? keys_a : keys_b;
        uint32_t *i_in = where ? ids_b : ids_a, *i_out = where ? ids_a : ids_b;
        const int there = ysmr::prim::radix_sort<uint32_t, unsigned long long>(st, i_in, i_out, k_in, k_out, entries, 8, k.temp);
        sorted = there ? k_out : k_in;
    }
    hipLaunchKernelGGL(k_vi_summary, dim3(n_violins), dim3(256), 0, st, sorted, (const uint32_t *)counts, start, summaries_dev);
    hipLaunchKernelGGL(k_vi_density, dim3(VI_GRID, n_violins), dim3(256), 0, st, sorted, (const uint32_t *)start,
                       (const ysmr_violin_summary *)summaries_dev, density_dev);
    YSMR_LAUNCH_CHECK();
    return YSMR_OK;
}

int ysmr_plot_violins(void *stream, int n_violins, const ysmr_violin_summary *summaries_dev, const double *density_dev,
                      const ysmr_violin_view *view, void *workspace_dev, size_t workspace_bytes, uint8_t *rgb_dev)
{
    if (!view) return ysmr::fail(YSMR_ERR_ARG, "view must not be NULL");
    if (n_violins < 1 || n_violins > YSMR_VIOLIN_MAX_SLOTS || view->n_violins != n_violins)
        return ysmr::fail(YSMR_ERR_ARG, "n_violins must be in 1..%d and equal to the view's, got %d and %d", YSMR_VIOLIN_MAX_SLOTS, n_violins,
                          view->n_violins);
    if (view->width < 1 || view->height < 1 || view->width > 32768 || view->height > 32768)
        return ysmr::fail(YSMR_ERR_ARG, "the canvas must be within 1..32768 pixels each way, got %d x %d", view->width, view->height);
    if (view->ax_w < 1 || view->ax_h < 1 || view->ax_x < 0 || view->ax_y < 0 || (long long)view->ax_x + view->ax_w > view->width ||
        (long long)view->ax_y + view->ax_h > view->height)
        return ysmr::fail(YSMR_ERR_ARG, "the axes rectangle (%d, %d, %d x %d) is not inside the %d x %d canvas", view->ax_x, view->ax_y,
                          view->ax_w, view->ax_h, view->width, view->height);
    if (!(view->units_per_pixel > 0) || !std::isfinite(view->units_per_pixel) || !std::isfinite(view->y0))
        return ysmr::fail(YSMR_ERR_ARG, "units_per_pixel must be positive and finite, y0 finite");
    if (view->n_grid_rows < 0 || view->n_grid_rows > 32) return ysmr::fail(YSMR_ERR_ARG, "at most 32 grid rows");
    if (view->line_half < 0 || view->line_half > 1024 || view->box_half < 0 || view->box_half > 1024 || view->dot_r2 < 0 ||
        view->dot_r2 > (1 << 20))
        return ysmr::fail(YSMR_ERR_ARG, "line_half and box_half must be in 0..1024, dot_r2 in 0..2^20");
    for (int k = 0; k < n_violins; ++k) {
        if (view->slot_w[k] < 0 || view->slot_colour[k] < 0 ||
            (view->slot_w[k] > 0 && (view->slot_x[k] < view->ax_x || (long long)view->slot_x[k] + view->slot_w[k] > (long long)view->ax_x + view->ax_w)))
            return ysmr::fail(YSMR_ERR_ARG, "slot %d (%d, width %d, colour %d) is not inside the axes", k, view->slot_x[k], view->slot_w[k],
                              view->slot_colour[k]);
    }
    if (!summaries_dev || !density_dev || !workspace_dev || !rgb_dev)
        return ysmr::fail(YSMR_ERR_ARG, "summaries_dev, density_dev, workspace_dev and rgb_dev must not be NULL");
    if (((uintptr_t)workspace_dev & 7) || ((uintptr_t)summaries_dev & 7) || ((uintptr_t)density_dev & 7))
        return ysmr::fail(YSMR_ERR_ARG, "workspace_dev, summaries_dev and density_dev must be 8-byte aligned");
    Arena arena(workspace_dev);
    const ViWork k = vi_carve(arena, 0, n_violins, view->ax_h);
    if (workspace_bytes < arena.bytes())
        return ysmr::fail(YSMR_ERR_CAPACITY, "violin workspace too small: %zu < %zu bytes", workspace_bytes, arena.bytes());
    ViView v{};
    v.y0 = view->y0; v.upp = view->units_per_pixel; v.W = view->width; v.H = view->height; v.ax_x = view->ax_x; v.ax_y = view->ax_y;
    v.ax_w = view->ax_w; v.ax_h = view->ax_h; v.n = n_violins; v.n_rows = view->n_grid_rows; v.line_half = view->line_half;
    v.box_half = view->box_half; v.dot_r2 = view->dot_r2;
    memcpy(v.grid_rows, view->grid_rows, sizeof v.grid_rows);
    memcpy(v.slot_x, view->slot_x, sizeof v.slot_x);
    memcpy(v.slot_w, view->slot_w, sizeof v.slot_w);
    memcpy(v.slot_colour, view->slot_colour, sizeof v.slot_colour);
    hipStream_t st = (hipStream_t)stream;
    int *prof = k.prof, *marks = k.marks;
    hipLaunchKernelGGL(k_vi_profile, dim3(n_violins), dim3(256), 0, st, summaries_dev, density_dev, v, prof, marks);
    hipLaunchKernelGGL(k_vi_paint, dim3(resident_grid((long long)v.W * v.H, VI_BLOCKS)), dim3(256), 0, st, (const int *)prof, (const int *)marks, v, rgb_dev);
    YSMR_LAUNCH_CHECK();
    return YSMR_OK;
}

}  // extern "C"

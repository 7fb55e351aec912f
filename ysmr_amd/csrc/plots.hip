// plots.hip -- the track figures of evaluate_tracks (ysmr/plot_functions.py:29-257): the overview of all tracks, the rose
// graph (every track moved to the origin) and the polar histogram of headings.  The reference hands the table to
// matplotlib, one scatter call per track; here the table stays in HBM, the canvas is painted by the device and comes
// back in one download.  The image is this project's own rendering of the same data ("The figures"); the
// rules are stated as a sequential painter in tests/plot_model.py and the kernels match it byte for byte:
//   * a track's colour value c_t = (dist_t - dmin) / (dmax - dmin), 0 for every track where that range is 0 or a
//     distance is not finite; its LUT entry min(255, (int)(c_t * 256)) of viridis_r;
//   * paint order: rank_t = number of tracks u with c_u > c_t, or c_u == c_t and u < t; the larger rank paints later,
//     so the shortest paths end up on top.  The key canvas holds 0 (nothing), 1 (a start dot) or 2 + rank, written
//     with atomicMax: "later over earlier" of the sequential painter is "largest key wins", whatever the scheduling;
//   * geometry in f64, operation for operation as written below (-ffp-contract=off): a row becomes the disc
//     dx^2 + dy^2 <= r2 around its pixel, clipped to the axes rectangle pixel by pixel.
// A table here is (TRACK_ID, POSITION_T)-ordered: the rows of a track are one contiguous run of equal ids.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>

#include "atan2_cr.h"
#include "common.h"
#include "plot_lut.h"
#include "prim.h"
#include "table.h"

namespace {

constexpr int PL_BLOCKS = 512;           // resident grids (two workgroups a compute unit); every kernel strides through its items
constexpr int PL_MAX_R2 = 4096;          // a dot's radius stays within 64 pixels
constexpr int PL_MAX_BINS = 1024;

__constant__ uint8_t c_lut[768] = {YSMR_VIRIDIS_R_U8};
const uint8_t h_lut[768] = {YSMR_VIRIDIS_R_U8};

using namespace ysmr::table;

using ysmr::prim::key_of;      // doubles as u64 keys of the same order: min and max become integer atomics
using ysmr::prim::value_of;
using ysmr::prim::finite64;
constexpr unsigned long long KEY_POS_INF = 0xFFF0000000000000ull;   // key_of(+inf)
constexpr unsigned long long KEY_NEG_INF = 0x000FFFFFFFFFFFFFull;   // key_of(-inf)

// first / last row of the run of equal ids that holds row i (binary search: "same id" is monotone on either side)
__device__ __forceinline__ long long run_first(const uint32_t *__restrict__ id, long long i)
{
    const uint32_t me = id[i];
    long long lo = 0, hi = i;
    while (lo < hi) {
        const long long mid = lo + (hi - lo) / 2;
        if (id[mid] == me) hi = mid; else lo = mid + 1;
    }
    return lo;
}
__device__ __forceinline__ long long run_last(const uint32_t *__restrict__ id, long long i, long long n)
{
    const uint32_t me = id[i];
    long long lo = i, hi = n - 1;
    while (lo < hi) {
        const long long mid = lo + (hi - lo + 1) / 2;
        if (id[mid] == me) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// ---- extent -----------------------------------------------------------------------------------------------------------

__global__ void k_extent_init(unsigned long long *keys)
{
    if (threadIdx.x < 4) keys[threadIdx.x] = (threadIdx.x & 1) ? KEY_NEG_INF : KEY_POS_INF;
}

__global__ __launch_bounds__(256) void k_extent(long long n, const uint32_t *__restrict__ id, const double *__restrict__ x,
                                                const double *__restrict__ y, int mode, double px, unsigned long long *keys)
{
    __shared__ unsigned long long s_red[256];
    unsigned long long u_lo = KEY_POS_INF, u_hi = KEY_NEG_INF, v_lo = KEY_POS_INF, v_hi = KEY_NEG_INF;
    for (long long i = gtid(); i < n; i += gstride()) {
        double u = x[i], v = y[i];
        if (mode == 1) {
            const long long f = run_first(id, i);
            u = u - x[f];
            v = v - y[f];
        }
        u = u / px;
        v = v / px;
        if (!finite64(u) || !finite64(v)) continue;
        const unsigned long long ku = key_of(u), kv = key_of(v);
        u_lo = std::min(u_lo, ku); u_hi = std::max(u_hi, ku);
        v_lo = std::min(v_lo, kv); v_hi = std::max(v_hi, kv);
    }
    u_lo = block_reduce(u_lo, s_red, Min()); u_hi = block_reduce(u_hi, s_red, Max());
    v_lo = block_reduce(v_lo, s_red, Min()); v_hi = block_reduce(v_hi, s_red, Max());
    if (threadIdx.x == 0) {
        atomicMin(&keys[0], u_lo); atomicMax(&keys[1], u_hi);
        atomicMin(&keys[2], v_lo); atomicMax(&keys[3], v_hi);
    }
}

__global__ void k_extent_finish(unsigned long long *keys)
{
    if (threadIdx.x < 4) {
        const double v = value_of(keys[threadIdx.x]);
        ((double *)keys)[threadIdx.x] = v;
    }
}

// ---- the tracks -------------------------------------------------------------------------------------------------------

struct PlTracks {
    const uint32_t *id;
    const double *x, *y, *dist;
    long long dist_stride;
    uint32_t *flag, *seg, *first, *rank, *canvas;   // seg: the row's track number; first[t]: track t's first row (t < n_tracks)
    double *c, *scal;                    // scal: dmin, dmax - dmin, 1.0 when the colour values are all 0
    uint8_t *lut_of_rank;
};

// one block: the range of the distances
__global__ __launch_bounds__(256) void k_pl_range(PlTracks r, uint32_t n_tracks)
{
    __shared__ unsigned long long s_red[256];
    unsigned long long lo = KEY_POS_INF, hi = KEY_NEG_INF, bad = 0;
    for (uint32_t t = threadIdx.x; t < n_tracks; t += 256) {
        const double d = r.dist[(long long)t * r.dist_stride];
        if (!finite64(d)) { bad = 1; continue; }
        const unsigned long long k = key_of(d);
        lo = std::min(lo, k); hi = std::max(hi, k);
    }
    lo = block_reduce(lo, s_red, Min());
    hi = block_reduce(hi, s_red, Max());
    bad = block_reduce(bad, s_red, Max());
    if (threadIdx.x == 0) {
        const double dmin = value_of(lo), span = value_of(hi) - dmin;
        const bool flat = bad || n_tracks == 0 || !(span > 0.0) || !finite64(span);
        r.scal[0] = flat ? 0.0 : dmin;
        r.scal[1] = flat ? 1.0 : span;
        r.scal[2] = flat ? 1.0 : 0.0;
    }
}

__global__ __launch_bounds__(256) void k_pl_colour(PlTracks r, uint32_t n_tracks)
{
    const double dmin = r.scal[0], span = r.scal[1];
    const bool flat = r.scal[2] != 0.0;
    for (long long t = gtid(); t < n_tracks; t += gstride())
        r.c[t] = flat ? 0.0 : (r.dist[t * r.dist_stride] - dmin) / span;
}

// rank by counting (tracks^2 comparisons: a table holds some thousands of tracks at most, and the figure is drawn once)
__global__ __launch_bounds__(256) void k_pl_rank(PlTracks r, uint32_t n_tracks)
{
    __shared__ double s_c[256];
    const long long rounds = ((long long)n_tracks + gstride() - 1) / gstride();
    for (long long k = 0; k < rounds; ++k) {
        const long long t = gtid() + k * gstride();
        const bool live = t < n_tracks;
        const double mine = live ? r.c[t] : 0.0;
        uint32_t rank = 0;
        for (uint32_t base = 0; base < n_tracks; base += 256) {
            __syncthreads();
            s_c[threadIdx.x] = base + threadIdx.x < n_tracks ? r.c[base + threadIdx.x] : -1.0;   // (c >= 0: -1 never counts)
            __syncthreads();
            const uint32_t m = std::min(256u, n_tracks - base);
            for (uint32_t j = 0; j < m; ++j) {
                const double o = s_c[j];
                rank += (o > mine || (o == mine && (long long)(base + j) < t)) ? 1u : 0u;
            }
        }
        if (live) {
            r.rank[t] = rank;
            const int idx = (int)(mine * 256.0);
            r.lut_of_rank[rank] = (uint8_t)std::min(255, idx);
        }
    }
}

struct PlView {                 // ysmr_plot_view as the kernels use it
    int mode, W, H, ax_x, ax_y, ax_w, ax_h, r2_dot, r2_start, n_cols, n_rows, bar_x, bar_y, bar_w, bar_h;
    double px, u0, v0, upp;
    int grid_cols[32], grid_rows[32];
};

__device__ __forceinline__ void paint_disc(uint32_t *__restrict__ canvas, const PlView &v, int c, int rr, int r2, uint32_t key)
{
    int rad = 0;
    while ((rad + 1) * (rad + 1) <= r2) ++rad;
    for (int dy = -rad; dy <= rad; ++dy) {
        const int py = rr + dy;
        if (py < 0 || py >= v.ax_h) continue;
        for (int dx = -rad; dx <= rad; ++dx) {
            const int pxl = c + dx;
            if (pxl < 0 || pxl >= v.ax_w || dx * dx + dy * dy > r2) continue;
            atomicMax(&canvas[(size_t)(v.ax_y + py) * v.W + (v.ax_x + pxl)], key);
        }
    }
}

__global__ __launch_bounds__(256) void k_pl_paint(PlTracks r, long long n, uint32_t n_tracks, PlView v)
{
    const double reach = 66.0;          // beyond this many pixels outside the axes no disc reaches in (PL_MAX_R2)
    for (long long i = gtid(); i < n; i += gstride()) {
        const uint32_t t = r.seg[i];
        if (t >= n_tracks) continue;
        double a = r.x[i], b = r.y[i];
        if (v.mode == 1) {
            const uint32_t f = r.first[t];
            a = a - r.x[f];
            b = b - r.y[f];
        }
        const double u = a / v.px, w = b / v.px;
        if (!finite64(u) || !finite64(w)) continue;
        const double fc = floor((u - v.u0) / v.upp), fr = floor((w - v.v0) / v.upp);
        if (!(fc >= -reach) || !(fc <= (double)v.ax_w + reach) || !(fr >= -reach) || !(fr <= (double)v.ax_h + reach)) continue;
        const int c = (int)fc, rr = v.ax_h - 1 - (int)fr;          // relative to the axes' top-left pixel
        if (v.mode == 0 && r.flag[i]) paint_disc(r.canvas, v, c, rr, v.r2_start, 1u);
        paint_disc(r.canvas, v, c, rr, v.r2_dot, 2u + r.rank[t]);
    }
}

__global__ __launch_bounds__(256) void k_pl_compose(const uint32_t *__restrict__ canvas, const uint8_t *__restrict__ lut_of_rank,
                                                    PlView v, uint8_t *__restrict__ rgb)
{
    const long long pixels = (long long)v.W * v.H;
    for (long long p = gtid(); p < pixels; p += gstride()) {
        const int row = (int)(p / v.W), col = (int)(p - (long long)row * v.W);
        int cr = 255, cg = 255, cb = 255;
        const int ac = col - v.ax_x, ar = row - v.ax_y;
        if (ac >= -1 && ac <= v.ax_w && ar >= -1 && ar <= v.ax_h) {
            if (ac == -1 || ac == v.ax_w || ar == -1 || ar == v.ax_h) {
                cr = cg = cb = 0;
            } else {
                bool grid = false;
                for (int k = 0; k < v.n_cols; ++k) grid |= v.grid_cols[k] == col;
                for (int k = 0; k < v.n_rows; ++k) grid |= v.grid_rows[k] == row;
                if (grid) cr = cg = cb = 176;
                const uint32_t key = canvas[p];
                if (key == 1u) {
                    cr = cg = cb = 0;
                } else if (key >= 2u) {
                    const int e = 3 * (int)lut_of_rank[key - 2u];
                    cr = c_lut[e]; cg = c_lut[e + 1]; cb = c_lut[e + 2];
                }
            }
        }
        if (v.bar_w > 0) {
            const int bc = col - v.bar_x, br = row - v.bar_y;
            if (bc >= -1 && bc <= v.bar_w && br >= -1 && br <= v.bar_h) {
                if (bc == -1 || bc == v.bar_w || br == -1 || br == v.bar_h) {
                    cr = cg = cb = 0;
                } else {
                    const int e = 3 * std::min(255, (int)(((long long)(v.bar_h - 1 - br) * 256) / v.bar_h));
                    cr = c_lut[e]; cg = c_lut[e + 1]; cb = c_lut[e + 2];
                }
            }
        }
        uint8_t *o = rgb + 3 * (size_t)p;
        o[0] = (uint8_t)cr; o[1] = (uint8_t)cg; o[2] = (uint8_t)cb;
    }
}

// the workspace part of r; returns the scan's scratch.  (The angle histogram carves (n, 0, 0) and uses flag and seg alone.)
uint32_t *pl_carve(Arena &a, long long n, long long n_tracks, long long pixels, PlTracks &r)
{
    r.flag = a.take<uint32_t>((size_t)n);
    r.seg = a.take<uint32_t>((size_t)n);
    uint32_t *scan_temp = a.take<uint32_t>(ysmr::prim::scan_temp_words((size_t)n));
    r.first = a.take<uint32_t>((size_t)n_tracks);
    r.rank = a.take<uint32_t>((size_t)n_tracks);
    r.c = a.take<double>((size_t)n_tracks);
    r.scal = a.take<double>(4);
    r.lut_of_rank = a.take<uint8_t>((size_t)n_tracks);
    r.canvas = a.take<uint32_t>((size_t)pixels);
    return scan_temp;
}

bool sizes_ok(long long n, long long n_tracks, int W, int H)
{
    return n >= 0 && n <= 0x7FFFFFFFll && n_tracks >= 0 && n_tracks <= 0x7FFFFFFFll && W >= 0 && H >= 0 && W <= 32768 && H <= 32768;
}

// ---- the angle histogram ----------------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void k_hist_moving(const int8_t *__restrict__ moving, uint32_t *__restrict__ out, long long n)
{
    for (long long i = gtid(); i < n; i += gstride()) out[i] = moving[i] == 1 ? 1u : 0u;
}

__global__ __launch_bounds__(256) void k_hist(long long n, const uint32_t *__restrict__ id, const double *__restrict__ x,
                                              const double *__restrict__ y, const int8_t *__restrict__ moving,
                                              const uint32_t *__restrict__ ones_incl, long long lag, int n_bins,
                                              const double *__restrict__ edges, unsigned long long *__restrict__ counts,
                                              unsigned long long *__restrict__ n_points)
{
    __shared__ double s_edges[PL_MAX_BINS + 1];
    __shared__ uint32_t s_hist[PL_MAX_BINS];
    __shared__ uint32_t s_points;
    for (int k = threadIdx.x; k <= n_bins; k += 256) s_edges[k] = edges[k];
    for (int k = threadIdx.x; k < n_bins; k += 256) s_hist[k] = 0;
    if (threadIdx.x == 0) s_points = 0;
    __syncthreads();
    // (a block meets at most 2^31 / gridDim.x rows: the 32-bit LDS counters cannot wrap)
    for (long long i = gtid(); i < n; i += gstride()) {
        if (moving[i] != 1) continue;
        const long long f = run_first(id, i), l = run_last(id, i, n);
        const uint32_t ones = ones_incl[l] - (f ? ones_incl[f - 1] : 0u);
        if (!((double)ones / (double)(l - f + 1) > 0.7)) continue;
        atomicAdd(&s_points, 1u);
        if (i - lag < f) continue;
        const double h = ysmr::atan2cr::atan2_cr(x[i] - x[i - lag], y[i] - y[i - lag]);   // correctly rounded, as k_ev_heading
        if (!(h >= s_edges[0]) || !(h <= s_edges[n_bins])) continue;
        int lo = 0, hi = n_bins;
        while (hi - lo > 1) {
            const int mid = lo + (hi - lo) / 2;
            if (h >= s_edges[mid]) lo = mid; else hi = mid;
        }
        atomicAdd(&s_hist[lo], 1u);
    }
    __syncthreads();
    for (int k = threadIdx.x; k < n_bins; k += 256)
        if (s_hist[k]) atomicAdd(&counts[k], (unsigned long long)s_hist[k]);
    if (threadIdx.x == 0 && s_points) atomicAdd(n_points, (unsigned long long)s_points);
}

// ---- the wedges -------------------------------------------------------------------------------------------------------

// Which wedge holds p = (east, north), and is p inside its bar?  -1: in no bar.
__device__ __forceinline__ int wedge_fill(long long pe, long long pn, int n_bins, const double *s_dirs, const long long *s_r2)
{
    const long long d2 = pe * pe + pn * pn;
    if (d2 == 0) return -1;
    const double e = (double)pe, nn = (double)pn;
    double prev = s_dirs[0] * nn - s_dirs[1] * e;
    for (int k = 0; k < n_bins; ++k) {
        const double next = s_dirs[2 * k + 2] * nn - s_dirs[2 * k + 3] * e;
        if (prev <= 0.0 && next > 0.0) return d2 <= s_r2[k] ? k : -1;      // the lowest such k
        prev = next;
    }
    return -1;
}

__global__ __launch_bounds__(256) void k_wedges(int W, int H, int cx, int cy, int n_bins, const double *__restrict__ dirs,
                                                const long long *__restrict__ r2, long long ring_r2, uint8_t *__restrict__ rgb)
{
    __shared__ double s_dirs[2 * (PL_MAX_BINS + 1)];
    __shared__ long long s_r2[PL_MAX_BINS];
    for (int k = threadIdx.x; k < 2 * (n_bins + 1); k += 256) s_dirs[k] = dirs[k];
    for (int k = threadIdx.x; k < n_bins; k += 256) s_r2[k] = r2[k];
    __syncthreads();
    const long long pixels = (long long)W * H;
    for (long long p = gtid(); p < pixels; p += gstride()) {
        const int row = (int)(p / W), col = (int)(p - (long long)row * W);
        const long long pe = (long long)col - cx, pn = (long long)cy - row;
        int cr = 255, cg = 255, cb = 255;
        const long long d2 = pe * pe + pn * pn;
        if (d2 <= ring_r2) {       // the ring: the disc's pixels that have a 4-neighbour outside it
            const bool edge = (pe - 1) * (pe - 1) + pn * pn > ring_r2 || (pe + 1) * (pe + 1) + pn * pn > ring_r2 ||
                              pe * pe + (pn - 1) * (pn - 1) > ring_r2 || pe * pe + (pn + 1) * (pn + 1) > ring_r2;
            if (edge) cr = cg = cb = 176;
        }
        const int k = wedge_fill(pe, pn, n_bins, s_dirs, s_r2);
        if (k >= 0) {
            const bool inner = wedge_fill(pe - 1, pn, n_bins, s_dirs, s_r2) == k && wedge_fill(pe + 1, pn, n_bins, s_dirs, s_r2) == k &&
                               wedge_fill(pe, pn - 1, n_bins, s_dirs, s_r2) == k && wedge_fill(pe, pn + 1, n_bins, s_dirs, s_r2) == k;
            if (inner) { cr = 143; cg = 187; cb = 218; } else { cr = cg = cb = 0; }
        }
        uint8_t *o = rgb + 3 * (size_t)p;
        o[0] = (uint8_t)cr; o[1] = (uint8_t)cg; o[2] = (uint8_t)cb;
    }
}

}  // namespace

extern "C" {

int ysmr_plot_colormap(uint8_t *out)
{
    if (!out) return ysmr::fail(YSMR_ERR_ARG, "out must not be NULL");
    memcpy(out, h_lut, sizeof h_lut);
    return YSMR_OK;
}

int ysmr_plot_extent(void *stream, long long n_rows, const uint32_t *track_id_dev, const double *x_dev, const double *y_dev,
                     int mode, double px, double *out_dev)
{
    if (n_rows < 0 || n_rows > 0x7FFFFFFFll) return ysmr::fail(YSMR_ERR_ARG, "n_rows must be in 0..2^31-1, got %lld", n_rows);
    if (mode != 0 && mode != 1) return ysmr::fail(YSMR_ERR_ARG, "mode must be 0 (overview) or 1 (rose), got %d", mode);
    if (!(px > 0) || !std::isfinite(px)) return ysmr::fail(YSMR_ERR_ARG, "px must be positive and finite");
    if (!out_dev) return ysmr::fail(YSMR_ERR_ARG, "out_dev must not be NULL");
    if (((uintptr_t)out_dev & 7)) return ysmr::fail(YSMR_ERR_ARG, "out_dev must be 8-byte aligned");
    if (n_rows > 0 && (!x_dev || !y_dev || (mode == 1 && !track_id_dev)))
        return ysmr::fail(YSMR_ERR_ARG, "a required device pointer is NULL");
    hipStream_t st = (hipStream_t)stream;
    unsigned long long *keys = (unsigned long long *)out_dev;
    hipLaunchKernelGGL(k_extent_init, dim3(1), dim3(64), 0, st, keys);
    if (n_rows > 0)
        hipLaunchKernelGGL(k_extent, dim3(resident_grid(n_rows, PL_BLOCKS)), dim3(256), 0, st, n_rows, track_id_dev, x_dev, y_dev, mode, px, keys);
    hipLaunchKernelGGL(k_extent_finish, dim3(1), dim3(64), 0, st, keys);
    YSMR_LAUNCH_CHECK();
    return YSMR_OK;
}

size_t ysmr_plot_workspace_bytes(long long n_rows, long long n_tracks, int width, int height)
{
    if (!sizes_ok(n_rows, n_tracks, width, height)) return 0;
    Arena sizing(nullptr);
    PlTracks r{};
    pl_carve(sizing, n_rows, n_tracks, (long long)width * height, r);
    return sizing.bytes();
}

int ysmr_plot_tracks(void *stream, long long n_rows, const uint32_t *track_id_dev, const double *x_dev, const double *y_dev,
                     long long n_tracks, const double *dist_dev, long long dist_stride, const ysmr_plot_view *view,
                     void *workspace_dev, size_t workspace_bytes, uint8_t *rgb_dev)
{
    if (!view) return ysmr::fail(YSMR_ERR_ARG, "view must not be NULL");
    if (!sizes_ok(n_rows, n_tracks, view->width, view->height) || view->width < 1 || view->height < 1)
        return ysmr::fail(YSMR_ERR_ARG, "n_rows, n_tracks must be in 0..2^31-1 and the canvas within 1..32768 (got %lld, %lld, %d x %d)",
                          n_rows, n_tracks, view->width, view->height);
    if (view->mode != 0 && view->mode != 1) return ysmr::fail(YSMR_ERR_ARG, "mode must be 0 (overview) or 1 (rose), got %d", view->mode);
    if (view->ax_w < 1 || view->ax_h < 1 || view->ax_x < 0 || view->ax_y < 0 || (long long)view->ax_x + view->ax_w > view->width ||
        (long long)view->ax_y + view->ax_h > view->height)
        return ysmr::fail(YSMR_ERR_ARG, "the axes rectangle (%d, %d, %d x %d) is not inside the %d x %d canvas", view->ax_x, view->ax_y,
                          view->ax_w, view->ax_h, view->width, view->height);
    if (view->bar_w < 0 || (view->bar_w > 0 && (view->bar_h < 1 || view->bar_x < 0 || view->bar_y < 0 ||
                                                (long long)view->bar_x + view->bar_w > view->width ||
                                                (long long)view->bar_y + view->bar_h > view->height)))
        return ysmr::fail(YSMR_ERR_ARG, "the colour bar (%d, %d, %d x %d) is not inside the %d x %d canvas", view->bar_x, view->bar_y,
                          view->bar_w, view->bar_h, view->width, view->height);
    if (!(view->px > 0) || !std::isfinite(view->px) || !(view->units_per_pixel > 0) || !std::isfinite(view->units_per_pixel) ||
        !std::isfinite(view->u0) || !std::isfinite(view->v0))
        return ysmr::fail(YSMR_ERR_ARG, "px and units_per_pixel must be positive, u0 and v0 finite");
    if (view->r2_dot < 0 || view->r2_dot > PL_MAX_R2 || view->r2_start < 0 || view->r2_start > PL_MAX_R2)
        return ysmr::fail(YSMR_ERR_ARG, "r2_dot and r2_start must be in 0..%d", PL_MAX_R2);
    if (view->n_grid_cols < 0 || view->n_grid_cols > 32 || view->n_grid_rows < 0 || view->n_grid_rows > 32)
        return ysmr::fail(YSMR_ERR_ARG, "at most 32 grid columns and 32 grid rows");
    if (!workspace_dev || !rgb_dev) return ysmr::fail(YSMR_ERR_ARG, "workspace_dev and rgb_dev must not be NULL");
    if (n_rows > 0 && (!track_id_dev || !x_dev || !y_dev)) return ysmr::fail(YSMR_ERR_ARG, "a required device pointer is NULL");
    if (n_tracks > 0 && (!dist_dev || dist_stride < 1)) return ysmr::fail(YSMR_ERR_ARG, "dist_dev must not be NULL and dist_stride >= 1");
    if (((uintptr_t)workspace_dev & 7)) return ysmr::fail(YSMR_ERR_ARG, "workspace_dev must be 8-byte aligned");
    const long long pixels = (long long)view->width * view->height;
    Arena arena(workspace_dev);
    PlTracks r{};
    uint32_t *scan_temp = pl_carve(arena, n_rows, n_tracks, pixels, r);
    if (workspace_bytes < arena.bytes())
        return ysmr::fail(YSMR_ERR_CAPACITY, "plot workspace too small: %zu < %zu bytes", workspace_bytes, arena.bytes());
    hipStream_t st = (hipStream_t)stream;
    r.id = track_id_dev; r.x = x_dev; r.y = y_dev; r.dist = dist_dev; r.dist_stride = dist_stride;
    PlView v{};
    v.mode = view->mode; v.W = view->width; v.H = view->height; v.ax_x = view->ax_x; v.ax_y = view->ax_y; v.ax_w = view->ax_w;
    v.ax_h = view->ax_h; v.r2_dot = view->r2_dot; v.r2_start = view->r2_start; v.n_cols = view->n_grid_cols; v.n_rows = view->n_grid_rows;
    v.bar_x = view->bar_x; v.bar_y = view->bar_y; v.bar_w = view->bar_w; v.bar_h = view->bar_h;
    v.px = view->px; v.u0 = view->u0; v.v0 = view->v0; v.upp = view->units_per_pixel;
    memcpy(v.grid_cols, view->grid_cols, sizeof v.grid_cols);
    memcpy(v.grid_rows, view->grid_rows, sizeof v.grid_rows);
    const uint32_t nt = (uint32_t)n_tracks;

    YSMR_HIP_CHECK(hipMemsetAsync(r.canvas, 0, 4 * (size_t)pixels, st));
    if (n_rows > 0 && nt > 0) {
        const dim3 g(resident_grid(n_rows, PL_BLOCKS)), gt(resident_grid(nt, PL_BLOCKS)), tb(256);
        // (a table with fewer tracks than n_tracks leaves the tail of first[] unused: no row refers to it; rows of tracks
        // beyond n_tracks are left out of first[] here and of the canvas later)
        index_runs(st, g.x, r.id, n_rows, r.flag, r.seg, r.first, nullptr, nt, scan_temp);
        hipLaunchKernelGGL(k_pl_range, dim3(1), tb, 0, st, r, nt);
        hipLaunchKernelGGL(k_pl_colour, gt, tb, 0, st, r, nt);
        hipLaunchKernelGGL(k_pl_rank, gt, tb, 0, st, r, nt);
        hipLaunchKernelGGL(k_pl_paint, g, tb, 0, st, r, n_rows, nt, v);
    }
    hipLaunchKernelGGL(k_pl_compose, dim3(resident_grid(pixels, PL_BLOCKS)), dim3(256), 0, st, (const uint32_t *)r.canvas,
                       (const uint8_t *)r.lut_of_rank, v, rgb_dev);
    YSMR_LAUNCH_CHECK();
    return YSMR_OK;
}

int ysmr_plot_angle_histogram(void *stream, long long n_rows, const uint32_t *track_id_dev, const double *x_dev,
                              const double *y_dev, const int8_t *moving_dev, int lag, int n_bins, const double *edges_dev,
                              void *workspace_dev, size_t workspace_bytes, long long *counts_dev, long long *n_points_dev)
{
    if (n_rows < 0 || n_rows > 0x7FFFFFFFll) return ysmr::fail(YSMR_ERR_ARG, "n_rows must be in 0..2^31-1, got %lld", n_rows);
    if (n_bins < 1 || n_bins > PL_MAX_BINS) return ysmr::fail(YSMR_ERR_ARG, "n_bins must be in 1..%d, got %d", PL_MAX_BINS, n_bins);
    if (lag < 1) return ysmr::fail(YSMR_ERR_ARG, "lag must be >= 1, got %d", lag);
    if (!edges_dev || !workspace_dev || !counts_dev || !n_points_dev)
        return ysmr::fail(YSMR_ERR_ARG, "edges_dev, workspace_dev, counts_dev and n_points_dev must not be NULL");
    if (n_rows > 0 && (!track_id_dev || !x_dev || !y_dev || !moving_dev)) return ysmr::fail(YSMR_ERR_ARG, "a required device pointer is NULL");
    if (((uintptr_t)counts_dev & 7) || ((uintptr_t)n_points_dev & 7) || ((uintptr_t)workspace_dev & 7))
        return ysmr::fail(YSMR_ERR_ARG, "workspace_dev, counts_dev and n_points_dev must be 8-byte aligned");
    Arena arena(workspace_dev);
    PlTracks r{};
    uint32_t *scan_temp = pl_carve(arena, n_rows, 0, 0, r);
    if (workspace_bytes < arena.bytes())
        return ysmr::fail(YSMR_ERR_CAPACITY, "plot workspace too small: %zu < %zu bytes", workspace_bytes, arena.bytes());
    hipStream_t st = (hipStream_t)stream;
    uint32_t *mv = r.flag, *incl = r.seg;
    YSMR_HIP_CHECK(hipMemsetAsync(counts_dev, 0, 8 * (size_t)n_bins, st));
    YSMR_HIP_CHECK(hipMemsetAsync(n_points_dev, 0, 8, st));
    if (n_rows > 0) {
        const dim3 g(resident_grid(n_rows, PL_BLOCKS)), tb(256);
        hipLaunchKernelGGL(k_hist_moving, g, tb, 0, st, moving_dev, mv, n_rows);
        ysmr::prim::inclusive_scan_u32(st, mv, incl, (size_t)n_rows, scan_temp);
        hipLaunchKernelGGL(k_hist, g, tb, 0, st, n_rows, track_id_dev, x_dev, y_dev, moving_dev, (const uint32_t *)incl, (long long)lag,
                           n_bins, edges_dev, (unsigned long long *)counts_dev, (unsigned long long *)n_points_dev);
    }
    YSMR_LAUNCH_CHECK();
    return YSMR_OK;
}

int ysmr_plot_wedges(void *stream, int width, int height, int cx, int cy, int n_bins, const double *dirs_dev,
                     const long long *r2_dev, long long ring_r2, uint8_t *rgb_dev)
{
    if (width < 1 || height < 1 || width > 32768 || height > 32768)
        return ysmr::fail(YSMR_ERR_ARG, "the canvas must be within 1..32768 pixels each way, got %d x %d", width, height);
    if (n_bins < 3 || n_bins > PL_MAX_BINS) return ysmr::fail(YSMR_ERR_ARG, "n_bins must be in 3..%d, got %d", PL_MAX_BINS, n_bins);
    if (cx < -(1 << 20) || cx > (1 << 20) || cy < -(1 << 20) || cy > (1 << 20))
        return ysmr::fail(YSMR_ERR_ARG, "the centre must lie within 2^20 pixels of the origin, got (%d, %d)", cx, cy);
    if (ring_r2 < 0) return ysmr::fail(YSMR_ERR_ARG, "ring_r2 must not be negative");
    if (!dirs_dev || !r2_dev || !rgb_dev) return ysmr::fail(YSMR_ERR_ARG, "dirs_dev, r2_dev and rgb_dev must not be NULL");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_wedges, dim3(resident_grid((long long)width * height, PL_BLOCKS)), dim3(256), 0, st, width, height, cx, cy, n_bins, dirs_dev,
                       r2_dev, ring_r2, rgb_dev);
    YSMR_LAUNCH_CHECK();
    return YSMR_OK;
}

}  // extern "C"

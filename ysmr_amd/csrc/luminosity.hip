// luminosity.hip -- the third tracking coordinate of 'include luminosity in tracking calculation' on gfx950:
// per detection  box = np.intp(cv2.boxPoints(rect));  cv2.fillPoly(mask, [box], 255);  cv2.mean(gray, mask)[0] / 100
// (ysmr/track_eval.py:290-300).  The mask is never stored: a scanline of the filled quadrilateral is ONE run of pixels
// [lo, hi] -- the four 8-connected edge lines and the 16.16 edge-table spans of OpenCV's fill overlap or touch on every
// row of a box that boxPoints can produce (verified, not assumed: tests/test_luminosity_cpu.py compares the counts and sums
// of random boxes with the set-based model, and a row of two runs would count the gap between them) -- so a lane takes a
// scanline, works [lo, hi] out in registers and adds the gray bytes under it.
//
//   * an edge's pixels on row y in closed form instead of by walking the line (quad.h, which also holds the corner
//     arithmetic: the detection view's outlines, view.hip, are the same lines);
//   * a group of 16 lanes (a DPP row) per detection, a lane per scanline, larger boxes strided; the two integer sums
//     are reduced inside the row by four DPP steps; lane 0 of the group writes the results.  No atomics, no LDS;
//   * gray bytes as aligned dwords with the ends masked off, added with v_sad_u8; BGR pixels are converted with the
//     fixed-point coefficients of the threshold kernels (common.h);
//   * the grid is a few workgroups per compute unit that stride over (frame, slice of detections): DESIGN.md 4.
//
// The arithmetic that decides a pixel is shared with ysmr_luminosity_batch_host below, which runs it on the host: the CPU
// suite compares it with the model where no GPU is present.  (cos / sin are the host's libm there and the device's here;
// both are rounded to float32, so a corner differs only if the double sits within an ulp of a rounding boundary.)
#include "common.h"
#include "quad.h"
#include <cmath>
#include <cstring>

namespace {

constexpr int LUM_THREADS = 256;
constexpr int LUM_GROUP = 16;                        // lanes per detection: one DPP row
constexpr int LUM_GROUPS = LUM_THREADS / LUM_GROUP;
constexpr int LUM_MAX_BLOCKS = 1024;                 // 4 workgroups per compute unit

// The filled pixels of row y, clipped to [0, W): false when there are none.
__host__ __device__ __forceinline__ bool lum_row(const LumBox &B, int y, int W, int &lo_out, int &hi_out)
{
    int lo = 0x7FFFFFFF, hi = -0x7FFFFFFF - 1;
    const long long none = 0x7FFFFFFFFFFFFFFFll;
    long long c0 = none, c1 = none, c2 = none, c3 = none;    // the edge table's crossings of this row
    auto take = [&](int a, int b) {
        a = max(a, 0); b = min(b, W - 1);
        if (a <= b) { lo = min(lo, a); hi = max(hi, b); }
    };
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const LumEdge &e = B.e[i];
        int a, b;
        if (lum_edge_row(e, y, a, b)) take(a, b);
        if (y >= e.yt && y < e.yb) {
            const long long x = e.xt16 + (long long)(y - e.yt) * e.dxs;
            if (i == 0) c0 = x;
            else if (i == 1) c1 = x;
            else if (i == 2) c2 = x;
            else c3 = x;
        }
    }
    // sorted crossings in pairs (inactive edges sort to the end)
    auto cswap = [](long long &p, long long &q) { const long long lo_ = p < q ? p : q, hi_ = p < q ? q : p; p = lo_; q = hi_; };
    cswap(c0, c1); cswap(c2, c3); cswap(c0, c2); cswap(c1, c3); cswap(c1, c2);
    if (c1 != none) take((int)((c0 + 0xFFFF) >> 16), (int)(c1 >> 16));
    if (c3 != none) take((int)((c2 + 0xFFFF) >> 16), (int)(c3 >> 16));
    lo_out = lo; hi_out = hi;
    return lo <= hi;
}

__host__ __device__ __forceinline__ uint32_t lum_bytes_sum(uint32_t v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_sad_u8(v, 0u, 0u);
#else
    return (v & 255u) + ((v >> 8) & 255u) + ((v >> 16) & 255u) + (v >> 24);
#endif
}

// Sum of the gray values of pixels [lo, hi] of row y of frame f.  total: bytes in the whole frames array.
template <int CH>
__host__ __device__ __forceinline__ uint32_t lum_row_sum(const uint8_t *__restrict__ frames, size_t total, size_t row_px,
                                                         int lo, int hi, const ysmr::GrayCoef &gc)
{
    uint32_t sum = 0;
    if (CH == 1) {
        const size_t a0 = row_px + (size_t)lo, a1 = row_px + (size_t)hi;
        const size_t w0 = a0 & ~(size_t)3, w1 = a1 & ~(size_t)3;
        for (size_t w = w0; w <= w1; w += 4) {
            uint32_t v;
            if (w + 4 <= total) {
#if defined(__HIP_DEVICE_COMPILE__)
                v = *(const uint32_t *)(frames + w);
#else
                memcpy(&v, frames + w, 4);
#endif
            } else {                                    // the array's last, partial dword
                v = 0;
                for (size_t k = w; k < total; ++k) v |= (uint32_t)frames[k] << (8 * (k - w));
            }
            if (w == w0) v &= 0xFFFFFFFFu << (8 * (unsigned)(a0 & 3));
            if (w == w1) v &= 0xFFFFFFFFu >> (8 * (3 - (unsigned)(a1 & 3)));
            sum += lum_bytes_sum(v);
        }
    } else {
        for (int x = lo; x <= hi; ++x) {
            const uint8_t *p = frames + (row_px + (size_t)x) * 3;
            sum += (uint32_t)(uint8_t)((p[0] * gc.b + p[1] * gc.g + p[2] * gc.r + gc.half) >> gc.shift);
        }
    }
    return sum;
}

// cv2.mean(gray, mask)[0] / 100
__host__ __device__ __forceinline__ double lum_value(uint32_t sum, uint32_t count)
{
    const double mean = count ? (double)sum * (1.0 / (double)count) : 0.0;
    return mean / 100.0;
}

__device__ __forceinline__ uint32_t row_total(uint32_t v)   // the sum over a DPP row, in every lane of it
{
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, true);    // quad_perm [1, 0, 3, 2]
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xF, 0xF, true);    // quad_perm [2, 3, 0, 1]
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x141, 0xF, 0xF, true);   // row_half_mirror
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x140, 0xF, 0xF, true);   // row_mirror
    return v;
}

template <int CH>
__global__ __launch_bounds__(LUM_THREADS) void k_luminosity(const uint8_t *__restrict__ frames, int batch, int height, int width,
                                                            const float *__restrict__ det, const int32_t *__restrict__ det_count,
                                                            int max_det, ysmr::GrayCoef gc, int parts, double *__restrict__ lum,
                                                            uint32_t *__restrict__ sum_out, uint32_t *__restrict__ count_out,
                                                            int32_t *__restrict__ corners)
{
    const int group = threadIdx.x / LUM_GROUP, l = threadIdx.x % LUM_GROUP;
    const size_t total = (size_t)batch * height * width * CH;
    for (int unit = blockIdx.x; unit < batch * parts; unit += gridDim.x) {
        const int f = unit / parts, part = unit - f * parts;
        const int n = min(max(det_count[f], 0), max_det);
        for (int d0 = part * LUM_GROUPS; d0 < n; d0 += parts * LUM_GROUPS) {     // (uniform over the workgroup)
            const int d = d0 + group;
            const bool live = d < n;
            const size_t slot = (size_t)f * max_det + (live ? d : 0);
            const float *q = det + slot * 5;
            const float cx = q[0], cy = q[1], w = q[2], h = q[3], angle = q[4];
            const double rad = lum_radians(angle);
            LumBox B;
            lum_box(cx, cy, w, h, (float)cos(rad), (float)sin(rad), B);
            uint32_t sum = 0, count = 0;
            const int y_first = max(B.ymin, 0), y_last = live ? min(B.ymax, height - 1) : -1;
            for (int y = y_first + l; y <= y_last; y += LUM_GROUP) {
                int lo, hi;
                if (!lum_row(B, y, width, lo, hi)) continue;
                count += (uint32_t)(hi - lo + 1);
                sum += lum_row_sum<CH>(frames, total, ((size_t)f * height + y) * width, lo, hi, gc);
            }
            sum = row_total(sum);
            count = row_total(count);
            if (live && l == 0) {
                lum[slot] = lum_value(sum, count);
                if (sum_out) sum_out[slot] = sum;
                if (count_out) count_out[slot] = count;
                if (corners) {
                    int4 *c = (int4 *)(corners + slot * 8);
                    c[0] = make_int4(B.px[0], B.py[0], B.px[1], B.py[1]);
                    c[1] = make_int4(B.px[2], B.py[2], B.px[3], B.py[3]);
                }
            }
        }
    }
}

int lum_check(const void *frames, int batch, int height, int width, int channels, const void *det, const void *det_count,
              int max_det, const void *lum)
{
    if (!frames || !det || !det_count || !lum) return ysmr::fail(YSMR_ERR_ARG, "luminosity: null pointer");
    if (batch < 0 || height <= 0 || width <= 0 || max_det <= 0)
        return ysmr::fail(YSMR_ERR_ARG, "luminosity: bad geometry (batch %d, %d x %d, max_det %d)", batch, height, width, max_det);
    if (channels != 1 && channels != 3) return ysmr::fail(YSMR_ERR_ARG, "channels must be 1 (gray) or 3 (BGR), got %d", channels);
    if ((size_t)height * width > ((size_t)1 << 24))
        return ysmr::fail(YSMR_ERR_ARG, "luminosity: frames of more than 2^24 pixels overflow the 32-bit sum of a box");
    if ((uintptr_t)frames & 3) return ysmr::fail(YSMR_ERR_ARG, "luminosity: frames must be 4-byte aligned");
    return YSMR_OK;
}

}  // namespace

extern "C" {

int ysmr_luminosity_batch(void *stream, const uint8_t *frames_dev, int batch, int height, int width, int channels,
                          const float *det_dev, const int32_t *det_count_dev, int max_det, int cv_flavour, double *lum_dev,
                          uint32_t *sum_dev, uint32_t *count_dev, int32_t *corners_dev)
{
    if (int rc = lum_check(frames_dev, batch, height, width, channels, det_dev, det_count_dev, max_det, lum_dev)) return rc;
    if (corners_dev && ((uintptr_t)corners_dev & 15)) return ysmr::fail(YSMR_ERR_ARG, "luminosity: corners must be 16-byte aligned");
    if (batch == 0) return YSMR_OK;
    const ysmr::GrayCoef gc = ysmr::gray_coef(cv_flavour);
    // every frame is cut into `parts` slices of its detections, a slice per workgroup visit, 16 detections in flight in each
    const int slices = (max_det + LUM_GROUPS - 1) / LUM_GROUPS;
    const int parts = std::max(1, std::min(LUM_MAX_BLOCKS / batch, slices));
    const int blocks = (int)std::min<long long>((long long)batch * parts, LUM_MAX_BLOCKS);
    if (channels == 1)
        hipLaunchKernelGGL(k_luminosity<1>, dim3(blocks), dim3(LUM_THREADS), 0, (hipStream_t)stream, frames_dev, batch, height, width,
                           det_dev, det_count_dev, max_det, gc, parts, lum_dev, sum_dev, count_dev, corners_dev);
    else
        hipLaunchKernelGGL(k_luminosity<3>, dim3(blocks), dim3(LUM_THREADS), 0, (hipStream_t)stream, frames_dev, batch, height, width,
                           det_dev, det_count_dev, max_det, gc, parts, lum_dev, sum_dev, count_dev, corners_dev);
    YSMR_LAUNCH_CHECK();
    return YSMR_OK;
}

int ysmr_luminosity_batch_host(const uint8_t *frames_host, int batch, int height, int width, int channels, const float *det_host,
                               const int32_t *det_count_host, int max_det, int cv_flavour, double *lum_host, uint32_t *sum_host,
                               uint32_t *count_host, int32_t *corners_host)
{
    if (int rc = lum_check(frames_host, batch, height, width, channels, det_host, det_count_host, max_det, lum_host)) return rc;
    const ysmr::GrayCoef gc = ysmr::gray_coef(cv_flavour);
    const size_t total = (size_t)batch * height * width * channels;
    for (int f = 0; f < batch; ++f) {
        const int n = std::min(std::max(det_count_host[f], 0), max_det);
        for (int d = 0; d < n; ++d) {
            const size_t slot = (size_t)f * max_det + d;
            const float *q = det_host + slot * 5;
            const double rad = lum_radians(q[4]);
            LumBox B;
            lum_box(q[0], q[1], q[2], q[3], (float)std::cos(rad), (float)std::sin(rad), B);
            uint32_t sum = 0, count = 0;
            for (int y = std::max(B.ymin, 0); y <= std::min(B.ymax, height - 1); ++y) {
                int lo, hi;
                if (!lum_row(B, y, width, lo, hi)) continue;
                count += (uint32_t)(hi - lo + 1);
                const size_t row_px = ((size_t)f * height + y) * width;
                sum += channels == 1 ? lum_row_sum<1>(frames_host, total, row_px, lo, hi, gc)
                                     : lum_row_sum<3>(frames_host, total, row_px, lo, hi, gc);
            }
            lum_host[slot] = lum_value(sum, count);
            if (sum_host) sum_host[slot] = sum;
            if (count_host) count_host[slot] = count;
            if (corners_host)
                for (int i = 0; i < 4; ++i) { corners_host[slot * 8 + 2 * i] = B.px[i]; corners_host[slot * 8 + 2 * i + 1] = B.py[i]; }
        }
    }
    return YSMR_OK;
}

}  // extern "C"

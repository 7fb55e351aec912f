// view.hip -- the detection view of track_bacteria: what upstream's window "... unfiltered possible detections" shows
// (ysmr/track_eval.py:306-325, 353-362: cv2.drawContours of every detection's box in blue, cv2.putText + cv2.circle of every
// live track in green), painted into stored DIB frames while the batch's frames are still on the device.  The pixel rule is
// stated in view_rule.h, which also holds the code that decides a pixel; here are the launches around it.
//   ysmr_view_boxes_batch   ysmr_annotate_batch's packing (no marks), then k_view_boxes: the outlines;
//   ysmr_view_tracks_batch  k_view_tracks: ids and dots of the rows the link emitted for those frames, a batch later.
// Between the layers the order is stream order; inside a layer all stores of a pixel carry the same three bytes, so lanes
// that meet on a pixel cannot disagree.  No atomics, no LDS.
//   * k_view_boxes: luminosity.hip's shape -- 16 lanes per detection, four per edge, a lane per row of the edge INSIDE the
//     frame, where the edge is one run in closed form (quad.h): the work is bounded by the frame, wherever the corners are;
//   * k_view_tracks: annotate.hip's shape -- a wave per row, a lane per cell of its digits and dot.  Which rows: the
//     half-open range of two counters read on the device (the pipeline's row counter before and after the batch's link).
#include "common.h"
#include "view_rule.h"
#include <algorithm>

namespace {

using namespace ysmr::view;
namespace glyph = ysmr::glyph;

constexpr int BOX_THREADS = 256, BOX_GROUP = 16, BOX_GROUPS = BOX_THREADS / BOX_GROUP;
constexpr int BOX_MAX_BLOCKS = 1024, TRACK_BLOCKS = 256;
constexpr int TRACK_ROUNDS = (10 * glyph::GLYPH_W * glyph::GLYPH_H + 1 + 63) / 64;   // ten digits and the small dot

__global__ __launch_bounds__(BOX_THREADS) void k_view_boxes(int batch, int H, int W, const float *__restrict__ det,
                                                            const int32_t *__restrict__ det_count, int max_det, int parts,
                                                            uint8_t *__restrict__ out, int stride, size_t frame_bytes, int bottom_up)
{
    const int group = threadIdx.x / BOX_GROUP, l = threadIdx.x % BOX_GROUP, edge = l & 3, sub = l >> 2;
    for (int unit = blockIdx.x; unit < batch * parts; unit += gridDim.x) {
        const int f = unit / parts, part = unit - f * parts;
        const int n = min(max(det_count[f], 0), max_det);
        uint8_t *frame = out + (size_t)f * frame_bytes;
        for (int d = part * BOX_GROUPS + group; d < n; d += parts * BOX_GROUPS) {
            LumEdge e;
            int first, last;
            edge_of(det + ((size_t)f * max_det + d) * 5, edge, e);
            edge_rows(e, H, first, last);
            for (int y = first + sub; y <= last; y += BOX_GROUP / 4) outline_row(e, y, W, dib_row(frame, H, stride, bottom_up, y));
        }
    }
}

__global__ __launch_bounds__(256) void k_view_tracks(const ysmr_row *__restrict__ rows, const long long *__restrict__ row_begin,
                                                     const long long *__restrict__ row_end, long long rows_capacity, int first,
                                                     int n, int H, int W, uint8_t *__restrict__ out, int stride, size_t frame_bytes,
                                                     int bottom_up)
{
    const int lane = threadIdx.x & 63;
    const long long begin = max(row_begin[0], 0ll), end = min(row_end[0], rows_capacity);   // (a counter past the buffer: overflow, the caller's to report)
    const long long wave0 = (long long)blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = (long long)gridDim.x * 4;
    for (long long item = begin + wave0; item < end; item += nwaves) {
        int f;
        glyph::Mark m;
        if (!mark_of_row(rows[item], first, n, f, m)) continue;
        const int total = glyph::mark_cells(m);
        uint8_t *frame = out + (size_t)f * frame_bytes;
#pragma unroll
        for (int r = 0; r < TRACK_ROUNDS; ++r)
            if (r * 64 + lane < total) paint_cell(m, r * 64 + lane, H, W, stride, bottom_up, frame);
    }
}

}  // namespace

extern "C" {

int ysmr_view_boxes_batch(void *stream, const uint8_t *frames_dev, int n_frames, int height, int width, int channels,
                          const float *det_dev, const int32_t *det_count_dev, int max_det, uint8_t *out_dev, int out_stride,
                          size_t out_frame_bytes, int bottom_up)
{
    if (!det_dev || !det_count_dev || max_det <= 0) return ysmr::fail(YSMR_ERR_ARG, "view: det_dev and det_count_dev must not be NULL, max_det positive (got %d)", max_det);
    // (the packing checks the frames and the layout of the output)
    if (int rc = ysmr_annotate_batch(stream, frames_dev, n_frames, height, width, channels, nullptr, nullptr, out_dev, out_stride,
                                     out_frame_bytes, bottom_up))
        return rc;
    // every frame is cut into `parts` slices of its detections, a slice per workgroup visit, 16 detections in flight in each
    const int slices = (max_det + BOX_GROUPS - 1) / BOX_GROUPS;
    const int parts = std::max(1, std::min(BOX_MAX_BLOCKS / n_frames, slices));
    const int blocks = (int)std::min<long long>((long long)n_frames * parts, BOX_MAX_BLOCKS);
    hipLaunchKernelGGL(k_view_boxes, dim3(blocks), dim3(BOX_THREADS), 0, (hipStream_t)stream, n_frames, height, width, det_dev,
                       det_count_dev, max_det, parts, out_dev, out_stride, out_frame_bytes, bottom_up);
    YSMR_LAUNCH_CHECK();
    return YSMR_OK;
}

int ysmr_view_tracks_batch(void *stream, const ysmr_row *rows_dev, int64_t rows_capacity, const int64_t *row_begin_dev,
                           const int64_t *row_end_dev, int32_t first_frame_index, int n_frames, int height, int width,
                           uint8_t *dib_dev, int stride, size_t frame_bytes, int bottom_up)
{
    if (const char *why = check_layout(n_frames, height, width, stride, frame_bytes, dib_dev)) return ysmr::fail(YSMR_ERR_ARG, "view: %s", why);
    if (!rows_dev || rows_capacity < 0 || !row_begin_dev || !row_end_dev)
        return ysmr::fail(YSMR_ERR_ARG, "view: rows_dev, row_begin_dev, row_end_dev must not be NULL, rows_capacity not negative");
    hipLaunchKernelGGL(k_view_tracks, dim3(TRACK_BLOCKS), dim3(256), 0, (hipStream_t)stream, rows_dev, (const long long *)row_begin_dev,
                       (const long long *)row_end_dev, (long long)rows_capacity, first_frame_index, n_frames, height, width, dib_dev,
                       stride, frame_bytes, bottom_up);
    YSMR_LAUNCH_CHECK();
    return YSMR_OK;
}

int ysmr_view_batch_host(const uint8_t *frames_host, int n_frames, int height, int width, int channels, const float *det_host,
                         const int32_t *det_count_host, int max_det, const ysmr_row *rows_host, int64_t row_begin, int64_t row_end,
                         int32_t first_frame_index, uint8_t *out_host, int out_stride, size_t out_frame_bytes, int bottom_up)
{
    if (const char *why = batch_host(frames_host, n_frames, height, width, channels, det_host, det_count_host, max_det, rows_host,
                                     row_begin, row_end, first_frame_index, out_host, out_stride, out_frame_bytes, bottom_up))
        return ysmr::fail(YSMR_ERR_ARG, "view: %s", why);
    return YSMR_OK;
}

}  // extern "C"

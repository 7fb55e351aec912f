// thrview.hip -- the threshold view of track_bacteria: what upstream's windows 'threshold' (ysmr/track_eval.py:271, the final
// mask behind binary_propagation) and 'Adaptive double threshold markers' (:210) show, and this project's composite of both
// over the frame, as stored DIB frames made from the class map and the mask a batch's detection has left on the device.  The
// pixel rule is stated in thrview_rule.h, which also holds the code that decides a pixel; here is the one launch around it.
//   k_thrview  every byte of every output frame, padding included: annotate.hip's k_pack_dib with two more inputs.
// A WAVE writes one stored row at a time (one division per 64 lanes); a lane takes 16 pixels per step -- 16 bytes of the
// mask, 16 of the class map and, in mode 2, the 16 or 48 bytes of the frame's pixels, all issued before the first is looked
// at -- and writes their 48 bytes; what is left of the row goes pixel by pixel, and the padding bytes are zeroed.  Neither end
// of a row is aligned beyond the 4 bytes of a DIB row.  Every byte is written by exactly one lane: no LDS, no atomics.
#include "common.h"
#include "thrview_rule.h"
#include <algorithm>

namespace {

using namespace ysmr::thrview;

constexpr int THRVIEW_BLOCKS = 1024;     // a resident grid (see ingest.hip)

__global__ __launch_bounds__(256) void k_thrview(const uint8_t *__restrict__ frames, const uint8_t *__restrict__ cls,
                                                 const uint8_t *__restrict__ mask, int n, int H, int W, int channels, int mode,
                                                 int bottom_up, uint8_t *__restrict__ out, int out_stride, size_t out_frame_bytes)
{
    const int lane = threadIdx.x & 63;
    const long long rows = (long long)n * H, wave0 = (long long)blockIdx.x * 4 + (threadIdx.x >> 6), nwaves = (long long)gridDim.x * 4;
    const size_t row_bytes = (size_t)W * 3;
    for (long long item = wave0; item < rows; item += nwaves) {
        const long long f = item / H;
        const int y = (int)(item - f * H);
        const size_t first = (size_t)item * W;
        uint8_t *dst = out + (size_t)f * out_frame_bytes + (size_t)(bottom_up ? H - 1 - y : y) * out_stride;
        // (mode and channels are the same for the whole launch: one of four bodies, each with its constants folded in.  A
        // pointer the mode does not read may be NULL and is not moved.)
        const uint8_t *fr = mode == MODE_CLASSES ? frames + first * (size_t)(channels == 3 ? 3 : 1) : nullptr;
        if (mode == MODE_MASK) row(MODE_MASK, 1, nullptr, cls + first, mask + first, W, lane * 16, 64 * 16, lane, dst);
        else if (mode == MODE_MARKERS) row(MODE_MARKERS, 1, nullptr, cls + first, nullptr, W, lane * 16, 64 * 16, lane, dst);
        else if (channels == 3) row(MODE_CLASSES, 3, fr, cls + first, mask + first, W, lane * 16, 64 * 16, lane, dst);
        else row(MODE_CLASSES, 1, fr, cls + first, mask + first, W, lane * 16, 64 * 16, lane, dst);
        for (size_t b = row_bytes + lane; b < (size_t)out_stride; b += 64) dst[b] = 0;
    }
}

}  // namespace

extern "C" {

int ysmr_thrview_batch(void *stream, const uint8_t *frames_dev, const uint8_t *cls_dev, const uint8_t *mask_dev, int n_frames, int height,
                       int width, int channels, int mode, uint8_t *out_dev, int out_stride, size_t out_frame_bytes, int bottom_up)
{
    if (const char *why = check_args(frames_dev, cls_dev, mask_dev, n_frames, height, width, channels, mode, out_dev, out_stride, out_frame_bytes))
        return ysmr::fail(YSMR_ERR_ARG, "thrview: %s", why);
    const size_t blocks = std::min<size_t>(((size_t)n_frames * height + 3) / 4, THRVIEW_BLOCKS);   // four rows (waves) per block
    hipLaunchKernelGGL(k_thrview, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, frames_dev, cls_dev, mask_dev, n_frames, height,
                       width, channels, mode, bottom_up, out_dev, out_stride, out_frame_bytes);
    YSMR_LAUNCH_CHECK();
    return YSMR_OK;
}

int ysmr_thrview_batch_host(const uint8_t *frames_host, const uint8_t *cls_host, const uint8_t *mask_host, int n_frames, int height,
                            int width, int channels, int mode, uint8_t *out_host, int out_stride, size_t out_frame_bytes, int bottom_up)
{
    if (const char *why = batch_host(frames_host, cls_host, mask_host, n_frames, height, width, channels, mode, out_host, out_stride,
                                     out_frame_bytes, bottom_up))
        return ysmr::fail(YSMR_ERR_ARG, "thrview: %s", why);
    return YSMR_OK;
}

}  // extern "C"

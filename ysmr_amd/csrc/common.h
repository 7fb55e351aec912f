// Shared helpers for libysmr_hip.so (host side).  gfx950 only.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <cstdarg>
#include <cstdio>
#include <cstdint>
#include "ysmr_hip.h"

namespace ysmr {

// thread-local message returned by ysmr_last_error()
char *error_buffer();
int fail(int code, const char *fmt, ...);

#define YSMR_HIP_CHECK(expr)                                                                   \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess)                                                                  \
            return ::ysmr::fail(YSMR_ERR_HIP, "%s failed: %s (%s:%d)", #expr,                  \
                                hipGetErrorString(e_), __FILE__, __LINE__);                    \
    } while (0)

#define YSMR_LAUNCH_CHECK() YSMR_HIP_CHECK(hipGetLastError())

// batch, height, width and max_det positive, 1 or 3 channels, the limits of 32-bit pixel indices (detect_plan.h:
// check_geometry): YSMR_OK, or YSMR_ERR_ARG with the message set (the mean-gray branch's does not name max_det)
int check_geometry(int batch, int H, int W, int channels, int max_det, bool names_max_det = true);
// the largest detection table the one-launch link takes (tracker_plan.h: FUSED_MAX_DET; track.hip)
int fused_max_det();

// One kernel launch; with an event given, the dispatch itself updates the two (hipExtLaunchKernelGGL).
template <class... Params, class... Args>
inline void launch(void (*kernel)(Params...), dim3 grid, dim3 block, size_t lds, hipStream_t stream, hipEvent_t ev_start,
                   hipEvent_t ev_stop, const Args &...args)
{
    if (ev_start || ev_stop) hipExtLaunchKernelGGL(kernel, grid, block, (uint32_t)lds, stream, ev_start, ev_stop, 0u, args...);
    else hipLaunchKernelGGL(kernel, grid, block, lds, stream, args...);
}

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// cv2.cvtColor(BGR2GRAY) on u8: fixed point, (B*b + G*g + R*r + half) >> shift.  OpenCV 4.x uses 15 bits
// (3735 / 19235 / 9798), OpenCV 3.x 14 bits (1868 / 9617 / 4899); both are the identity for B = G = R.
struct GrayCoef { uint32_t b, g, r, half, shift; };
inline GrayCoef gray_coef(int cv_flavour)
{
    if (cv_flavour & YSMR_CV_GRAY_3X) return GrayCoef{1868u, 9617u, 4899u, 8192u, 14u};
    return GrayCoef{3735u, 19235u, 9798u, 16384u, 15u};
}

}  // namespace ysmr

__device__ __forceinline__ uint32_t bgr2gray(const ysmr::GrayCoef &k, uint32_t b, uint32_t g, uint32_t r)
{
    return (b * k.b + g * k.g + r * k.r + k.half) >> k.shift;   // cv2 COLOR_BGR2GRAY (a1)
}

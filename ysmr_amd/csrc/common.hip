// Error reporting shared by the C ABI entry points.
#include "common.h"
#include "detect_plan.h"
#include <cstring>

namespace ysmr {

char *error_buffer()
{
    static thread_local char buf[512] = "";
    return buf;
}

int fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(error_buffer(), 512, fmt, ap);
    va_end(ap);
    return code;
}

int check_geometry(int batch, int H, int W, int channels, int max_det, bool names_max_det)
{
    switch (detect_plan::check_geometry(batch, H, W, channels, max_det)) {
    case detect_plan::Bad::none: break;
    case detect_plan::Bad::positive:
        if (!names_max_det) return fail(YSMR_ERR_ARG, "batch, height, width must be positive (got %d, %d, %d)", batch, H, W);
        return fail(YSMR_ERR_ARG, "batch, height, width, max_det must be positive (got %d, %d, %d, %d)", batch, H, W, max_det);
    case detect_plan::Bad::channels: return fail(YSMR_ERR_ARG, "channels must be 1 (gray) or 3 (BGR), got %d", channels);
    case detect_plan::Bad::too_large:
        return fail(YSMR_ERR_ARG, "batch too large (height and width are limited to 16384, batch*height*width to 2^32 - 1)");
    }
    return YSMR_OK;
}

}  // namespace ysmr

extern "C" {

int ysmr_abi_version(void) { return YSMR_ABI_VERSION; }

const char *ysmr_last_error(void) { return ysmr::error_buffer(); }

}

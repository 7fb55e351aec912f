// tiff_decode_plan.h -- the host-only part of tiff_decode.hip: the argument rules of a call, the strips of a frame and the layout
// of the workspace.  Plain C++ with no HIP in it, so that tests/tiff_plan_check.cc compiles it alone, under the host sanitizers.
#pragma once
#include <cstddef>
#include <cstdint>

namespace tfd {

// one row of strips_dev: int32 [n_strips][5]
constexpr int STRIP_WORDS = 5;      // frame, first row, rows, offset of the body in bodies_dev, bytes of the body
// the LZW table of a strip: entries 258 .. 4095, an output position each (see tiff_decode.hip)
constexpr int LZW_CODES = 4096;
constexpr int LZW_FIRST = 258;
// the last data code after a Clear that may still add an entry (entry 257 + n for the n-th code, 4095 at most)
constexpr int LZW_MAX_RUN = LZW_CODES - 1 - (LZW_FIRST - 1);
// the most workgroups a launch over strips gets; a workgroup takes the strips blockIdx.x, blockIdx.x + gridDim.x, ...
constexpr int STRIP_GRID = 4096;

struct Plan {
    int strips_per_frame, rows_per_strip;
    long long n_strips;
    long long row_bytes, frame_bytes;
    size_t strip_status;              // int32 per strip: what the strip's wave found
    size_t total;
};

inline size_t align256(size_t v) { return (v + 255) / 256 * 256; }

// false for what the call refuses.  Every product is formed in 64 bits from factors below 2^31, so none can wrap.
//   rows_per_strip: 1 .. height (a file's RowsPerStrip above the height is the height)
//   body_bytes: the bytes of all strip bodies of the call, 0 .. INT_MAX (offsets into bodies_dev are int32)
inline bool plan_of(int n_frames, int height, int width, int channels, int compression, int predictor, int photometric,
                    int rows_per_strip, long long body_bytes, Plan &p)
{
    if (n_frames <= 0 || height <= 0 || width <= 0) return false;
    if (channels != 1 && channels != 3) return false;
    if (compression != 1 && compression != 5 && compression != 32773) return false;
    if (predictor != 1 && predictor != 2) return false;
    if (photometric < 0 || photometric > 2 || (photometric == 2) != (channels == 3)) return false;
    if (rows_per_strip <= 0 || rows_per_strip > height) return false;
    if (body_bytes < 0 || body_bytes > INT32_MAX) return false;
    p.row_bytes = (long long)width * channels;                    // < 2^33
    if (p.row_bytes > INT32_MAX) return false;
    p.frame_bytes = p.row_bytes * height;                         // < 2^62
    if (p.frame_bytes > INT32_MAX) return false;                  // positions inside a strip are 32-bit
    if (p.frame_bytes > (long long)(INT64_MAX / n_frames)) return false;
    p.rows_per_strip = rows_per_strip;
    p.strips_per_frame = (int)(((long long)height + rows_per_strip - 1) / rows_per_strip);
    p.n_strips = (long long)p.strips_per_frame * n_frames;        // < 2^62
    if (p.n_strips > INT32_MAX) return false;
    p.strip_status = 0;
    p.total = align256((size_t)p.n_strips * sizeof(int32_t));
    return true;
}

// The strips of a call tile its frames: n_strips is a multiple of n_frames, and the strips of a frame are of equal height but
// for a shorter last one.  0, or the rows of a strip.
inline int rows_per_strip_of(long long n_strips, int n_frames, int height)
{
    if (n_frames <= 0 || height <= 0 || n_strips <= 0 || n_strips % n_frames) return 0;
    const long long per_frame = n_strips / n_frames;
    if (per_frame > height) return 0;
    const long long rows = (height + per_frame - 1) / per_frame;
    if ((height + rows - 1) / rows != per_frame) return 0;       // e.g. 10 rows in 4 strips: 3, 3, 3, 1 -- but in 6: no such file
    return (int)rows;
}

}  // namespace tfd

// mjpeg_decode_plan.h -- the host-only part of mjpeg_decode.hip: the geometry of a call, its argument rules and the layout of its
// workspace.  Plain C++ with no HIP in it, so that tests/mjpeg_sync_plan_check.cc compiles it alone, under the host sanitizers.
#pragma once
#include <cstddef>
#include <cstdint>
#include <initializer_list>

namespace mjd {

// ---- the geometry of a call (host and device) --------------------------------------------------------------------------------
struct Geo {
    int H, W, sampling, nc;
    int lh, lv;                       // sampling factors of the luminance
    int mx, my, mcus;                 // MCUs per row, MCU rows, MCUs per frame = the most restart intervals a frame can have
    int ycols, yrows, ccols, crows;   // blocks per plane
    int blocks_y, blocks_c, blocks;   // blocks per frame
    int ypitch, cpitch;               // bytes per row of the sample planes (whole blocks)
    size_t plane_y, plane_c, planes;  // bytes of the sample planes of a frame (0 for one component: the frame is the plane)
};

// what k_mjd_headers leaves per frame
struct FrameInfo {
    int32_t ent_start, ent_end;       // the entropy data [start, end) inside the frame's bytes
    int32_t ri, nseg;                 // restart interval in MCUs (0: none), restart intervals of the frame
    uint32_t tq, td, ta;              // per component, a byte each: quantisation table, DC and AC Huffman slot
    uint32_t defined;                 // bit 4 * class + slot: the frame's Huffman table is in the workspace
};
struct HuffRaw { uint8_t bits[16]; uint8_t vals[256]; };

struct Plan {
    size_t info, quant, huff, seg_start, coef, planes, total;
};

inline size_t align256(size_t v) { return (v + 255) / 256 * 256; }

inline Plan plan_of(int n, const Geo &g)
{
    Plan p;
    size_t at = 0;
    auto take = [&](size_t bytes) { const size_t here = at; at += align256(bytes); return here; };
    p.info = take((size_t)n * sizeof(FrameInfo));
    p.quant = take((size_t)n * 4 * 64 * sizeof(uint16_t));
    p.huff = take((size_t)n * 8 * sizeof(HuffRaw));
    p.seg_start = take((size_t)n * g.mcus * sizeof(int32_t));
    p.coef = take((size_t)n * g.blocks * 64 * sizeof(int16_t));
    p.planes = take((size_t)n * g.planes);
    p.total = at;
    return p;
}

inline bool geometry_of(int n, int H, int W, int channels, int sampling, Geo &g)
{
    if (n <= 0 || H <= 0 || W <= 0 || H > 65535 || W > 65535 || sampling < 0 || sampling > 3) return false;
    if (channels != (sampling == 0 ? 1 : 3)) return false;
    g.H = H; g.W = W; g.sampling = sampling; g.nc = channels;
    g.lh = sampling >= 2 ? 2 : 1; g.lv = sampling == 3 ? 2 : 1;
    g.mx = (W + 8 * g.lh - 1) / (8 * g.lh); g.my = (H + 8 * g.lv - 1) / (8 * g.lv); g.mcus = g.mx * g.my;
    g.ycols = g.mx * g.lh; g.yrows = g.my * g.lv; g.ccols = g.mx; g.crows = g.my;
    g.blocks_y = g.ycols * g.yrows; g.blocks_c = g.nc == 3 ? g.ccols * g.crows : 0; g.blocks = g.blocks_y + 2 * g.blocks_c;
    g.ypitch = 8 * g.ycols; g.cpitch = 8 * g.ccols;
    g.plane_y = g.nc == 3 ? (size_t)64 * g.blocks_y : 0; g.plane_c = (size_t)64 * g.blocks_c; g.planes = g.plane_y + 2 * g.plane_c;
    return true;
}

// ---- ysmr_mjpeg_decode_batch_sync: frames without restart markers, decoded by many lanes ----------------------------------------
// A frame's entropy data, freed of stuffing and fill bytes, is cut into subsequences of SYNC_SUB_BYTES; a workgroup takes
// SYNC_PASS consecutive ones at a time, a lane each.  Both are compile-time constants (ysmr_mjpeg_decode_sync_geometry reports
// them); a tuning build may set others.
#ifndef MJD_SYNC_SUB_BYTES
#define MJD_SYNC_SUB_BYTES 64
#endif
#ifndef MJD_SYNC_PASS
#define MJD_SYNC_PASS 256
#endif
constexpr int SYNC_SUB_BYTES = MJD_SYNC_SUB_BYTES;
constexpr int SYNC_PASS = MJD_SYNC_PASS;           // lanes of the workgroup: a multiple of 64, at most 1024
static_assert(SYNC_SUB_BYTES >= 1 && SYNC_PASS >= 64 && SYNC_PASS <= 1024 && SYNC_PASS % 64 == 0, "geometry of the synchronising decode");
// bit positions inside a frame's data are 32-bit numbers, with room to spare for the 32 bits a lane looks ahead
constexpr int SYNC_MAX_CHUNK = (1 << 27) - 1;

struct SyncPlan {
    Plan base;                        // what ysmr_mjpeg_decode_batch keeps, at the same places
    size_t data, data_pitch;          // the frames' entropy data without stuffing, data_pitch bytes apart
    size_t data_bytes;                // int32 per frame: bytes of it
    size_t total;
};

// false: an argument ysmr_mjpeg_decode_batch refuses, max_chunk_bytes outside 1 .. SYNC_MAX_CHUNK, or a total beyond size_t
inline bool sync_plan_of(int n, int H, int W, int channels, int sampling, int max_chunk_bytes, Geo &g, SyncPlan &p)
{
    if (!geometry_of(n, H, W, channels, sampling, g)) return false;
    if (max_chunk_bytes <= 0 || max_chunk_bytes > SYNC_MAX_CHUNK) return false;
    // the largest term first, in arithmetic that tells: blocks < 2^28, so 128 * blocks fits; times n it need not
    size_t coef, planes, seg, data;
    if (__builtin_mul_overflow((size_t)n, (size_t)g.blocks * 64 * sizeof(int16_t), &coef)) return false;
    if (__builtin_mul_overflow((size_t)n, g.planes, &planes)) return false;
    if (__builtin_mul_overflow((size_t)n, (size_t)g.mcus * sizeof(int32_t), &seg)) return false;
    p.data_pitch = align256((size_t)max_chunk_bytes + 8);                // (eight to spare: a lane's window is one load)
    if (__builtin_mul_overflow((size_t)n, p.data_pitch, &data)) return false;
    // per frame 32 + 512 + 2176 + 4 bytes of tables and counts; 255 bytes of rounding at most for each of eight parts
    size_t sum = (size_t)n * 4096 + 4096;
    for (const size_t part : {coef, planes, seg, data})
        if (__builtin_add_overflow(sum, part, &sum)) return false;
    p.base = plan_of(n, g);
    size_t at = p.base.total;
    auto take = [&](size_t bytes) { const size_t here = at; at += align256(bytes); return here; };
    p.data = take(data);
    p.data_bytes = take((size_t)n * sizeof(int32_t));
    p.total = at;
    return p.total <= sum;            // (the bound above is one: anything else is a mistake in this function)
}

}  // namespace mjd

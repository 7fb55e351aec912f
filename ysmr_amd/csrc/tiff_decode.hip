// tiff_decode.hip -- the strips of a TIFF stack decoded on the device: uncompressed, LZW (TIFF 6.0, MSB first) and PackBits, then
// the horizontal predictor, WhiteIsZero and R, G, B -> B, G, R (ysmr_tiff_decode_batch; the host side is frames.TiffVideo).
//
// A strip is independent work and a wave's: strips_dev row s = (frame, first row, rows, offset, bytes) says where its body lies in
// bodies_dev -- at ANY byte offset, so the body is only ever read a byte at a time -- and which rows * W * channels bytes of
// frames_out are its own.  No load leaves [offset, offset + bytes), no store the strip's bytes of its frame.
//
// LZW.  The string of a table entry is the string of the code before it plus one byte, and both already lie side by side in the
// strip's output: entry 258 + i is the output of the i-th data code since the last Clear and the first byte of the next.  So the
// table is not strings but the output POSITION of every data code since the Clear, P[0 .. n]: entry 258 + i starts at P[i] and is
// P[i + 1] - P[i] + 1 bytes long.  A position is 32 bits (a one-strip frame of 1228 x 922 is 1.13 MB), 4096 of them are 16 KB of
// LDS per strip, and no length is stored.  The code that IS the next free entry (i == n - 1, "KwKwK") reads the same way: P[n] is
// where this code's output starts, its last byte is its own first, which lies at P[i] -- every other byte of any copy lies below
// P[n] and was written by an earlier code.  The lanes of the wave copy a string side by side; the codes themselves are serial.
// Output written by one lane is read by another lane of the SAME wave only: a wave's vector memory operations are performed in
// order, which is what the wavefront-scope fences below tell the compiler to keep.
#include "common.h"
#include "tiff_decode_plan.h"
#include <algorithm>

namespace {

using namespace tfd;

constexpr int WINDOW = 1024;          // bytes of a strip's body held in LDS at a time

__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }

__device__ __forceinline__ void wave_order()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

struct Strip {
    uint8_t *dst;                     // the strip's bytes of its frame
    const uint8_t *src;               // its body
    uint32_t need, bytes;             // bytes to write, bytes of the body
    int frame;
    bool ok, frame_ok;
};

// Row s of the table, checked against the call's geometry: a row that fails writes and reads nothing.
__device__ __forceinline__ Strip strip_of(const uint8_t *bodies, const int32_t *strips, int s, int n_frames, int H, int row_bytes,
                                          uint8_t *out)
{
    Strip t;
    const int frame = uni(strips[STRIP_WORDS * s]), row0 = uni(strips[STRIP_WORDS * s + 1]), rows = uni(strips[STRIP_WORDS * s + 2]);
    const int off = uni(strips[STRIP_WORDS * s + 3]), bytes = uni(strips[STRIP_WORDS * s + 4]);
    t.frame = frame;
    t.frame_ok = frame >= 0 && frame < n_frames;
    t.ok = t.frame_ok && row0 >= 0 && rows > 0 && rows <= H - row0 && off >= 0 && bytes >= 0;
    t.dst = out + ((size_t)(t.ok ? frame : 0) * H + (t.ok ? row0 : 0)) * row_bytes;
    t.src = bodies + (t.ok ? off : 0);
    t.need = t.ok ? (uint32_t)rows * (uint32_t)row_bytes : 0u;        // <= frame bytes <= INT_MAX (plan_of)
    t.bytes = t.ok ? (uint32_t)bytes : 0u;
    return t;
}

__device__ __forceinline__ void report(const Strip &t, int s, int st, int *strip_status, int *status)
{
    if (threadIdx.x == 0 && blockIdx.y == 0) {
        strip_status[s] = st;
        if (st && t.frame_ok) atomicOr(&status[t.frame], st);
    }
}

// ---- LZW: a wave per strip -------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_tiff_lzw(const uint8_t *__restrict__ bodies, const int32_t *__restrict__ strips, int n_strips,
                                                 int n_frames, int H, int row_bytes, uint8_t *out, int *strip_status, int *status)
{
    __shared__ uint32_t P[LZW_CODES];
    __shared__ uint8_t win[WINDOW + 4];
    const uint32_t lane = threadIdx.x;
    for (int s = blockIdx.x; s < n_strips; s += gridDim.x) {
        const Strip t = strip_of(bodies, strips, s, n_frames, H, row_bytes, out);
        int st = t.ok ? 0 : YSMR_TIFFD_TABLE;
        if (t.ok && t.bytes >= 2 && uni(t.src[0]) == 0 && (uni(t.src[1]) & 1)) st = YSMR_TIFFD_OLD_LZW;
        uint32_t cur = 0, at = 0, base = 0;       // bytes written; byte of the body the next code begins in; first byte in win
        int bit = 0, nbits = 9, n = 0;            // bits of that byte already used; width; data codes since the Clear
        bool loaded = false;
        uint8_t *const dst = t.dst;
        while (st == 0 && cur < t.need) {
            if ((uint64_t)at * 8 + bit + nbits > (uint64_t)t.bytes * 8) break;            // the data ends: SHORT below
            if (!loaded || at + 3 > base + WINDOW) {
                base = at;
                loaded = true;
                __syncthreads();
                for (uint32_t i = lane; i < WINDOW + 4; i += 64) win[i] = base + i < t.bytes ? t.src[base + i] : (uint8_t)0;
                __syncthreads();
            }
            const uint8_t *w = win + (at - base);
            const uint32_t v = ((uint32_t)w[0] << 16) | ((uint32_t)w[1] << 8) | w[2];
            const int code = uni((int)((v >> (24 - bit - nbits)) & ((1u << nbits) - 1)));
            bit += nbits;
            at += bit >> 3;
            bit &= 7;
            if (code == 257) break;                                                      // EOI
            if (code == 256) { n = 0; nbits = 9; continue; }
            const int i = code - LZW_FIRST;
            if (i >= n || n > LZW_MAX_RUN) { st = YSMR_TIFFD_BAD_CODE; break; }    // above the next free entry; or the table is full
            P[n] = cur;                           // (every lane writes it and reads only what it wrote itself)
            if (code < 256) {
                if (lane == 0) dst[cur] = (uint8_t)code;
                cur += 1;
            } else {
                const uint32_t from = (uint32_t)uni((int)P[i]), len = (uint32_t)uni((int)P[i + 1]) - from + 1;
                const uint32_t m = min(len, t.need - cur);
                const bool kwkwk = i == n - 1;
                for (uint32_t j = lane; j < m; j += 64) dst[cur + j] = dst[kwkwk && j == len - 1 ? from : from + j];
                cur += m;
            }
            wave_order();
            n += 1;
            const int free_entry = LZW_FIRST - 1 + n;
            nbits = free_entry >= 2047 ? 12 : free_entry >= 1023 ? 11 : free_entry >= 511 ? 10 : 9;
        }
        if (st == 0 && cur < t.need) st = YSMR_TIFFD_SHORT;
        report(t, s, st, strip_status, status);
        __syncthreads();
    }
}

// ---- PackBits: a wave per strip -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_tiff_packbits(const uint8_t *__restrict__ bodies, const int32_t *__restrict__ strips, int n_strips,
                                                      int n_frames, int H, int row_bytes, uint8_t *__restrict__ out, int *strip_status,
                                                      int *status)
{
    const uint32_t lane = threadIdx.x;
    for (int s = blockIdx.x; s < n_strips; s += gridDim.x) {
        const Strip t = strip_of(bodies, strips, s, n_frames, H, row_bytes, out);
        int st = t.ok ? 0 : YSMR_TIFFD_TABLE;
        uint32_t cur = 0, at = 0;
        while (st == 0 && cur < t.need) {
            if (at >= t.bytes) { st = YSMR_TIFFD_SHORT; break; }
            const int h = (int8_t)uni(t.src[at]);
            at += 1;
            if (h == -128) continue;
            const uint32_t count = h >= 0 ? (uint32_t)h + 1 : (uint32_t)(1 - h);
            if (count > t.need - cur) { st = YSMR_TIFFD_OVERRUN; break; }
            if (h >= 0) {
                if (count > t.bytes - at) { st = YSMR_TIFFD_SHORT; break; }
                for (uint32_t j = lane; j < count; j += 64) t.dst[cur + j] = t.src[at + j];
                at += count;
            } else {
                if (at >= t.bytes) { st = YSMR_TIFFD_SHORT; break; }
                const uint8_t value = (uint8_t)uni(t.src[at]);
                at += 1;
                for (uint32_t j = lane; j < count; j += 64) t.dst[cur + j] = value;
            }
            cur += count;
        }
        report(t, s, st, strip_status, status);
    }
}

// ---- uncompressed: a gather ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_tiff_copy(const uint8_t *__restrict__ bodies, const int32_t *__restrict__ strips, int n_strips,
                                                   int n_frames, int H, int row_bytes, uint8_t *__restrict__ out, int *strip_status,
                                                   int *status)
{
    for (int s = blockIdx.x; s < n_strips; s += gridDim.x) {
        const Strip t = strip_of(bodies, strips, s, n_frames, H, row_bytes, out);
        const int st = !t.ok ? YSMR_TIFFD_TABLE : t.bytes < t.need ? YSMR_TIFFD_SHORT : 0;
        if (st == 0)
            for (uint32_t i = blockIdx.y * 256u + threadIdx.x; i < t.need; i += gridDim.y * 256u) t.dst[i] = t.src[i];
        report(t, s, st, strip_status, status);
    }
}

// ---- predictor 2, WhiteIsZero, R, G, B -> B, G, R: a wave per row, in place -------------------------------------------------------
// The running sum of a row is a scan over its pixels, 64 at a time with the carry of the pixels before; the three channels of a
// pixel ride in one word, 12 bits apart, each kept to its 8 bits after every step.
__global__ __launch_bounds__(256) void k_tiff_finish(uint8_t *frames, long long rows, int W, int channels, int predictor, int invert)
{
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int lane = threadIdx.x & 63;
    uint8_t *p = frames + (size_t)row * W * channels;
    const uint32_t keep = 0xFF0FF0FFu;
    uint32_t carry = 0;
    for (int x0 = 0; x0 < W; x0 += 64) {
        const int x = x0 + lane;
        uint32_t v = 0;
        if (x < W) {
            if (channels == 1) v = p[x];
            else v = (uint32_t)p[3 * x] | ((uint32_t)p[3 * x + 1] << 12) | ((uint32_t)p[3 * x + 2] << 24);
        }
        if (predictor == 2) {
            for (int d = 1; d < 64; d <<= 1) {
                const uint32_t up = __shfl_up(v, d, 64);
                if (lane >= d) v = (v + up) & keep;
            }
            v = (v + carry) & keep;
            carry = __shfl(v, 63, 64);
        }
        if (x < W) {
            if (channels == 1) p[x] = (uint8_t)(invert ? ~v : v);
            else {
                p[3 * x] = (uint8_t)(v >> 24);            // B
                p[3 * x + 1] = (uint8_t)(v >> 12);        // G
                p[3 * x + 2] = (uint8_t)v;                // R
            }
        }
    }
}

const char *const RULES = "n_frames, height and width must be positive, channels 1 or 3, compression 1, 5 or 32773, predictor 1 or 2, "
                          "photometric 0 or 1 with one channel and 2 with three, a frame and all bodies at most 2^31 - 1 bytes";

}  // namespace

extern "C" size_t ysmr_tiff_decode_workspace_bytes(int n_frames, int height, int width, int channels, int compression, int predictor,
                                                   int photometric, int rows_per_strip, long long body_bytes)
{
    Plan p;
    if (!plan_of(n_frames, height, width, channels, compression, predictor, photometric, rows_per_strip, body_bytes, p)) return 0;
    return p.total;
}

extern "C" int ysmr_tiff_decode_batch(void *stream, const uint8_t *bodies_dev, const int32_t *strips_dev, int n_strips, int n_frames,
                                      int height, int width, int channels, int compression, int predictor, int photometric,
                                      void *workspace_dev, size_t workspace_bytes, uint8_t *frames_out, int32_t *status_dev)
{
    const int rows_per_strip = rows_per_strip_of(n_strips, n_frames, height);
    Plan p;
    if (!rows_per_strip)
        return ysmr::fail(YSMR_ERR_ARG, "%d strips do not tile %d frames of %d rows", n_strips, n_frames, height);
    if (!plan_of(n_frames, height, width, channels, compression, predictor, photometric, rows_per_strip, 0, p) || p.n_strips != n_strips)
        return ysmr::fail(YSMR_ERR_ARG, "%s (got %d frames of %d x %d, %d channels, compression %d, predictor %d, photometric %d)", RULES,
                          n_frames, width, height, channels, compression, predictor, photometric);
    if (!bodies_dev || !strips_dev || !workspace_dev || !frames_out || !status_dev)
        return ysmr::fail(YSMR_ERR_ARG, "bodies_dev, strips_dev, workspace_dev, frames_out and status_dev must not be NULL");
    if (workspace_bytes < p.total)
        return ysmr::fail(YSMR_ERR_ARG, "workspace of %zu bytes, %zu needed (ysmr_tiff_decode_workspace_bytes)", workspace_bytes, p.total);
    if (((uintptr_t)workspace_dev & 255) || ((uintptr_t)strips_dev & 3) || ((uintptr_t)status_dev & 3))
        return ysmr::fail(YSMR_ERR_ARG, "workspace_dev must be 256-byte aligned, strips_dev and status_dev 4-byte");

    hipStream_t st = (hipStream_t)stream;
    int *strip_status = (int *)((uint8_t *)workspace_dev + p.strip_status);
    const int row_bytes = (int)p.row_bytes;
    const unsigned gx = (unsigned)std::min(n_strips, STRIP_GRID);
    YSMR_HIP_CHECK(hipMemsetAsync(status_dev, 0, (size_t)n_frames * sizeof(int32_t), st));
    if (compression == 5)
        hipLaunchKernelGGL(k_tiff_lzw, dim3(gx), dim3(64), 0, st, bodies_dev, strips_dev, n_strips, n_frames, height, row_bytes, frames_out,
                           strip_status, (int *)status_dev);
    else if (compression == 32773)
        hipLaunchKernelGGL(k_tiff_packbits, dim3(gx), dim3(64), 0, st, bodies_dev, strips_dev, n_strips, n_frames, height, row_bytes,
                           frames_out, strip_status, (int *)status_dev);
    else {
        const long long strip_bytes = (long long)rows_per_strip * row_bytes;
        const unsigned gy = (unsigned)std::max<long long>(1, std::min<long long>(64, (strip_bytes + 4095) / 4096));
        hipLaunchKernelGGL(k_tiff_copy, dim3(gx, gy), dim3(256), 0, st, bodies_dev, strips_dev, n_strips, n_frames, height, row_bytes,
                           frames_out, strip_status, (int *)status_dev);
    }
    YSMR_LAUNCH_CHECK();
    if (predictor == 2 || photometric != 1) {
        const long long rows = (long long)n_frames * height;          // < 2^62; the grid: rows / 4 must fit 2^31 - 1
        if ((rows + 3) / 4 > INT32_MAX) return ysmr::fail(YSMR_ERR_ARG, "%lld rows are more than one launch takes", rows);
        hipLaunchKernelGGL(k_tiff_finish, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, frames_out, rows, width, channels, predictor,
                           photometric == 0 ? 1 : 0);
        YSMR_LAUNCH_CHECK();
    }
    return YSMR_OK;
}

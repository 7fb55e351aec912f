// mjpeg.hip -- the annotated video as Motion-JPEG: what annotate.hip leaves on the device (stored 24-bit DIB frames, the marks
// painted) becomes finished '00dc' AVI chunks, each one baseline sequential JPEG (ITU-T T.81, SOF0; Y, Cb, Cr sampled 1 x 1).
// THE STREAM (tests/jpeg_model.py is its specification, and the kernels are tested against it byte for byte): SOI, APP0
// 'AVI1', DQT (tables 0 and 1: Annex K.1 scaled by the quality), SOF0, four DHT (the typical tables of Annex K.3), DRI, SOS,
// data, EOI.  One MCU row is one restart interval: DC predictors 0 at its start, padded with 1-bits to a byte at its end,
// RST(row mod 8) behind every interval but the last, 0x00 behind every 0xFF inside it -- so every MCU row of every frame is
// an independent piece of work.  Integers only from pixel to byte: 16-bit fixed-point JFIF colour, the DCT of T.81 A.3.3 as
// two products with the matrix round(2^16 c(u)/2 cos((2x+1) u pi/16)) (the first kept whole in 32 bits, the second summed in
// 64 and rounded to 12 fraction bits), quantisation by a division that rounds half away from zero, AC clamped to
// +-1023 and DC to [-1024, 1023].
// SIX LAUNCHES on the caller's stream, nothing between them but the workspace:
//   k_mj_blocks   a wave per MCU, a lane per pixel: colour, DCT (the eight operands of a row / a column come from the other
//                 lanes by ds_bpermute), quantise, zigzag -> int16 coef[frame][MCU row][MCU][component][64]
//   k_mj_lengths  a wave per restart interval, a lane per block: the bits of every block, their prefix sum -> where each
//                 block's code starts in the interval; the interval's words of the bit buffer are zeroed
//   k_mj_pack     a lane per block: the Huffman codes, OR-ed into the interval's bit buffer (a word is shared by the blocks
//                 whose bits meet in it; OR does not care about the order, so the bytes do not depend on scheduling)
//   k_mj_count    a wave per interval: its bytes and how many of them are 0xFF -> the interval's size in the file
//   k_mj_layout   one workgroup: sizes of the frames' chunks, offsets_dev, the status, every interval's place in out_dev
//   k_mj_write    a wave per interval: count-and-scan over the packed bytes for the stuffing, the bytes themselves, the RST /
//                 EOI behind them; the wave of a frame's first interval also writes the chunk header and the JPEG header.
// Every store into out_dev is a byte store guarded by out_capacity.  The worst case of a block is 1658 bits (20 for the DC,
// 26 for each AC coefficient); the bit buffer has 1664 per block IN THE WORKSPACE -- no kernel has a stack array.
// TWO CHOICES of ysmr_mjpeg_encode_batch (tests/jpeg_sampled_model.py is their specification; ysmr_mjpeg_batch is (1, 0)):
//   sampling 2 / 3   4:2:2 / 4:2:0: the MCU is 16 x 8 / 16 x 16 pixels, two / four luminance blocks, then Cb and Cr, each
//                    libjpeg's average of the 2 / 4 samples it covers; k_mj_blocks_sampled instead of k_mj_blocks, and the
//                    entropy kernels find a block's table and DC predecessor from its place in the MCU (block_at)
//   huffman 1        four tables per frame from the frame's own symbols.  Between k_mj_blocks and k_mj_lengths:
//     k_mj_hist      grid (x, frame), a lane per block: the frame's symbol counts, in LDS first
//     k_mj_tables    a workgroup per (table, frame): code lengths of at most 16 bits (png_codes.h, with the pseudo-symbol of
//                    T.81 K.2 so that the code of all 1-bits stays free), canonical codes, the DHT segment
//                    and k_mj_lengths / k_mj_pack run with the frame as the grid's y, the frame's codes in LDS; the header's
//                    length varies per frame (k_mj_layout, k_mj_write).
#include "common.h"
#include "png_codes.h"
#include <algorithm>

namespace {

constexpr int HEADER_BYTES = 625;            // SOI .. SOS header: 2 + 18 + 134 + 19 + 2 * (33 + 183) + 6 + 14
constexpr int HEADER_FRONT = 173;            // SOI, APP0, DQT, SOF0: what stands in front of the DHT segments
constexpr int HEADER_BACK = 20;              // DRI and the SOS header behind them
// Words of bit buffer per block.  With the Annex K.3 tables a block has at most 20 + 63 * 26 = 1658 bits: 52 words (1664
// bits).  A table built per frame may give ANY symbol a 16-bit code, the DC category 11 included: 27 + 63 * 26 = 1665 bits,
// one more than 52 words hold -- so the per-frame mode has 53.
constexpr int BLOCK_WORDS = 52, BLOCK_WORDS_BUILT = 53;
constexpr int MAX_GRID = 2048;
// One frame's codes, and its histogram, as 768 words: AC luminance [0, 256), AC chrominance [256, 512), DC luminance
// [512, 528), DC chrominance [528, 544) -- the layout of c_codes below.
constexpr int CODE_WORDS = 768;
constexpr int DHT_STRIDE = 192;              // a DHT segment of a built table: 21 + its symbols (at most 162) bytes

struct Header { uint8_t b[640]; };           // (by value into k_mj_write: 625 bytes used)
struct Quant { uint32_t q[2][64]; };         // divisors in natural order: luminance, chrominance

// ---- tables of the standard ---------------------------------------------------------------------------------------------
constexpr uint8_t K1_LUM[64] = {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
                                14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
                                49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
constexpr uint8_t K1_CHR[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
                                47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
                                99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};
// natural index (8 * row + column) of the k-th coefficient of the zigzag sequence
constexpr uint8_t ZIGZAG[64] = {0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,
                                7, 14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31,
                                39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
// Annex K.3: codes per length 1 .. 16, then the symbols in code order
constexpr uint8_t DC_LUM_BITS[16] = {0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0};
constexpr uint8_t DC_CHR_BITS[16] = {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0};
constexpr uint8_t DC_VALS[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
constexpr uint8_t AC_LUM_BITS[16] = {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7D};
constexpr uint8_t AC_LUM_VALS[162] = {
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91,
    0xA1, 0x08, 0x23, 0x42, 0xB1, 0xC1, 0x15, 0x52, 0xD1, 0xF0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0A, 0x16, 0x17, 0x18, 0x19, 0x1A,
    0x25, 0x26, 0x27, 0x28, 0x29, 0x2A, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4A, 0x53,
    0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79,
    0x7A, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9A, 0xA2, 0xA3, 0xA4, 0xA5,
    0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4, 0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3, 0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9,
    0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA, 0xE1, 0xE2, 0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF1, 0xF2,
    0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9, 0xFA};
constexpr uint8_t AC_CHR_BITS[16] = {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77};
constexpr uint8_t AC_CHR_VALS[162] = {
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14,
    0x42, 0x91, 0xA1, 0xB1, 0xC1, 0x09, 0x23, 0x33, 0x52, 0xF0, 0x15, 0x62, 0x72, 0xD1, 0x0A, 0x16, 0x24, 0x34, 0xE1, 0x25, 0xF1, 0x17,
    0x18, 0x19, 0x1A, 0x26, 0x27, 0x28, 0x29, 0x2A, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4A,
    0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78,
    0x79, 0x7A, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9A, 0xA2, 0xA3,
    0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4, 0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3, 0xC4, 0xC5, 0xC6, 0xC7,
    0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA, 0xE2, 0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF2,
    0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9, 0xFA};

// The codes of a table by T.81 Annex C, one word per symbol: (code << 8) | length; 0 where the table has no such symbol.
struct Codes { uint32_t v[256]; };
constexpr Codes codes_of(const uint8_t *bits, const uint8_t *vals)
{
    Codes t{};
    uint32_t code = 0;
    int k = 0;
    for (int len = 1; len <= 16; ++len) {
        for (int j = 0; j < bits[len - 1]; ++j) t.v[vals[k++]] = (code++ << 8) | (uint32_t)len;
        code <<= 1;
    }
    return t;
}
// [0]: AC luminance, [1]: AC chrominance, [2]: DC luminance in [0, 12) and DC chrominance in [16, 28)
constexpr Codes dc_codes()
{
    Codes t{};
    const Codes l = codes_of(DC_LUM_BITS, DC_VALS), c = codes_of(DC_CHR_BITS, DC_VALS);
    for (int k = 0; k < 12; ++k) { t.v[k] = l.v[k]; t.v[16 + k] = c.v[k]; }
    return t;
}
__constant__ Codes c_codes[3] = {codes_of(AC_LUM_BITS, AC_LUM_VALS), codes_of(AC_CHR_BITS, AC_CHR_VALS), dc_codes()};
// round(2^16 c(u) / 2 cos((2 x + 1) u pi / 16)), [u][x]; the absolute values of a row sum to 185360 at most
__constant__ int16_t c_dct[64] = {
    23170, 23170, 23170, 23170, 23170, 23170, 23170, 23170, 32138, 27246, 18205, 6393, -6393, -18205, -27246, -32138,
    30274, 12540, -12540, -30274, -30274, -12540, 12540, 30274, 27246, -6393, -32138, -18205, 18205, 32138, 6393,
    -27246, 23170, -23170, -23170, 23170, 23170, -23170, -23170, 23170, 18205, -32138, 6393, 27246, -27246, -6393,
    32138, -18205, 12540, -30274, 30274, -12540, -12540, 30274, -30274, 12540, 6393, -18205, 27246, -32138, 32138,
    -27246, 18205, -6393};
__constant__ uint8_t c_zigzag[64] = {0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,
                                     7, 14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31,
                                     39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

__device__ __forceinline__ uint32_t wave_inclusive(uint32_t v, int lane)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = (uint32_t)__shfl_up((int)v, d, 64);
        if (lane >= d) v += o;
    }
    return v;
}

// ---- colour, DCT, quantisation ------------------------------------------------------------------------------------------
// A WAVE takes one MCU at a time, lane 8 y + x its pixel (y, x); pixels beyond the frame repeat the last column / row.  After
// the first product lane 8 y + u holds row y's u-th sum, after the second lane 8 v + u the coefficient (v, u); lane k then
// fetches the k-th coefficient of the zigzag sequence, so that a block is stored as 128 contiguous bytes.
// The level-shifted sample v of lane 8 y + x becomes, in lane k, the k-th quantised coefficient of the zigzag sequence.
__device__ __forceinline__ int16_t dct_quantised(int v, const int (&cx)[8], const int (&cy)[8], uint32_t q, int lane, int x, int zz)
{
    int rows = 0;                                                  // |rows| <= 128 * 185360 < 2^25
#pragma unroll
    for (int k = 0; k < 8; ++k) rows += cx[k] * __shfl(v, (lane & ~7) + k, 64);
    long long full = 0;                                            // scaled by 2^32, below 2^43
#pragma unroll
    for (int k = 0; k < 8; ++k) full += (long long)cy[k] * __shfl(rows, 8 * k + x, 64);
    const int acc = (int)((full + (1ll << 19)) >> 20);             // 12 fraction bits: |acc| <= 1024 * 4096 + a little
    const uint32_t mag = ((uint32_t)(acc < 0 ? -acc : acc) + (q << 11)) / (q << 12);
    int val = acc < 0 ? -(int)mag : (int)mag;
    val = std::max(lane == 0 ? -1024 : -1023, std::min(1023, val));
    return (int16_t)__shfl(val, zz, 64);
}

__global__ __launch_bounds__(256) void k_mj_blocks(const uint8_t *__restrict__ dib, int n, int H, int W, int stride, size_t frame_bytes,
                                                   int bottom_up, Quant qt, int16_t *__restrict__ coef)
{
    const int lane = threadIdx.x & 63, y = lane >> 3, x = lane & 7;
    int cx[8], cy[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) { cx[k] = c_dct[8 * x + k]; cy[k] = c_dct[8 * y + k]; }
    const uint32_t q_of[2] = {qt.q[0][lane], qt.q[1][lane]};
    const int zz = c_zigzag[lane];
    const int W8 = (W + 7) >> 3, H8 = (H + 7) >> 3;
    const long long per_frame = (long long)H8 * W8, total = per_frame * n;
    for (long long m = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); m < total; m += (long long)gridDim.x * 4) {
        const long long f = m / per_frame;
        const int rem = (int)(m - f * per_frame), r = rem / W8, c = rem - r * W8;
        const int py = std::min(8 * r + y, H - 1), px = std::min(8 * c + x, W - 1);
        const uint8_t *p = dib + (size_t)f * frame_bytes + (size_t)(bottom_up ? H - 1 - py : py) * (size_t)stride + 3 * (size_t)px;
        const int B = p[0], G = p[1], R = p[2];
        int s[3];
        s[0] = (19595 * R + 38470 * G + 7471 * B + 32768) >> 16;
        s[1] = ((-11059 * R - 21709 * G + 32768 * B + 32767) >> 16) + 128;
        s[2] = ((32768 * R - 27439 * G - 5329 * B + 32767) >> 16) + 128;
        int16_t *o = coef + (size_t)m * 192;
#pragma unroll
        for (int comp = 0; comp < 3; ++comp)
            o[64 * comp + lane] = dct_quantised(std::min(std::max(s[comp], 0), 255) - 128, cx, cy, q_of[comp ? 1 : 0], lane, x, zz);
    }
}

// The subsampled frames: the MCU is 8 h x 8 v pixels, (h, v) = (2, 1) or (2, 2).  A WAVE takes one MCU at a time: its h v
// luminance blocks row by row, lane 8 y + x the pixel (y, x) of each, then Cb and Cr, whose sample (y, x) is libjpeg's
// average of the h v clamped samples it covers -- (a + b + bias) >> 1 with bias 0, 1, 0, 1, ... along the row, or
// (a + b + c + d + bias) >> 2 with bias 1, 2, 1, 2, ... -- taken BEFORE the level shift.  Pixels beyond the frame repeat the last
// column / row, so the padded frame is a whole number of MCUs.  The blocks of an MCU are stored in the order of the scan.
__global__ __launch_bounds__(256) void k_mj_blocks_sampled(const uint8_t *__restrict__ dib, int n, int H, int W, int stride,
                                                           size_t frame_bytes, int bottom_up, int v_luma, Quant qt,
                                                           int16_t *__restrict__ coef)
{
    const int lane = threadIdx.x & 63, y = lane >> 3, x = lane & 7;
    int cx[8], cy[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) { cx[k] = c_dct[8 * x + k]; cy[k] = c_dct[8 * y + k]; }
    const uint32_t q_of[2] = {qt.q[0][lane], qt.q[1][lane]};
    const int zz = c_zigzag[lane];
    const int hv = 2 * v_luma, Wm = (W + 15) >> 4, Hm = (H + 8 * v_luma - 1) / (8 * v_luma);
    const long long per_frame = (long long)Hm * Wm, total = per_frame * n;
    for (long long m = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); m < total; m += (long long)gridDim.x * 4) {
        const long long f = m / per_frame;
        const int rem = (int)(m - f * per_frame), r = rem / Wm, c = rem - r * Wm;
        const uint8_t *frame = dib + (size_t)f * frame_bytes;
        auto pixel = [&](int py, int px) {
            py = std::min(py, H - 1);
            px = std::min(px, W - 1);
            return frame + (size_t)(bottom_up ? H - 1 - py : py) * (size_t)stride + 3 * (size_t)px;
        };
        int16_t *o = coef + (size_t)m * (hv + 2) * 64;
        for (int k = 0; k < hv; ++k) {
            const uint8_t *p = pixel(8 * (v_luma * r + (k >> 1)) + y, 8 * (2 * c + (k & 1)) + x);
            const int B = p[0], G = p[1], R = p[2];
            const int s = (19595 * R + 38470 * G + 7471 * B + 32768) >> 16;
            o[64 * k + lane] = dct_quantised(std::min(std::max(s, 0), 255) - 128, cx, cy, q_of[0], lane, x, zz);
        }
        int cb = hv == 2 ? (x & 1) : 1 + (x & 1), cr = cb;                  // the bias
        for (int k = 0; k < hv; ++k) {
            const uint8_t *p = pixel(v_luma * (8 * r + y) + (k >> 1), 2 * (8 * c + x) + (k & 1));
            const int B = p[0], G = p[1], R = p[2];
            cb += std::min(std::max(((-11059 * R - 21709 * G + 32768 * B + 32767) >> 16) + 128, 0), 255);
            cr += std::min(std::max(((32768 * R - 27439 * G - 5329 * B + 32767) >> 16) + 128, 0), 255);
        }
        const int shift = hv == 2 ? 1 : 2;
        o[64 * hv + lane] = dct_quantised((cb >> shift) - 128, cx, cy, q_of[1], lane, x, zz);
        o[64 * hv + 64 + lane] = dct_quantised((cr >> shift) - 128, cx, cy, q_of[1], lane, x, zz);
    }
}

// ---- entropy coding -----------------------------------------------------------------------------------------------------
// The codes of the workgroup into LDS: the Annex K.3 tables, or, where `built` holds a set per frame, those of the frame
// blockIdx.y -- the grid's y is then the frame, and a workgroup touches no other frame's intervals (span_of).
__device__ __forceinline__ void load_codes(uint32_t *s_codes, const uint32_t *__restrict__ built)
{
    if (built)
        for (int k = threadIdx.x; k < CODE_WORDS; k += blockDim.x) s_codes[k] = built[(size_t)blockIdx.y * CODE_WORDS + k];
    else
        for (int k = threadIdx.x; k < CODE_WORDS; k += blockDim.x) s_codes[k] = c_codes[k >> 8].v[k & 255];
    __syncthreads();
}

// What a workgroup of the entropy kernels works on: all intervals (gridDim.y = 1), or those of the frame blockIdx.y.
__device__ __forceinline__ void span_of(long long intervals, long long &first, long long &end)
{
    const long long per = intervals / gridDim.y;
    first = per * blockIdx.y;
    end = first + per;
}

// The code of a value of size category `size` behind the Huffman code `entry` of its symbol: both in one piece.
__device__ __forceinline__ void coded(uint32_t entry, int v, int size, uint32_t &bits, int &len)
{
    const uint32_t low = (uint32_t)(v < 0 ? v - 1 : v) & ((1u << size) - 1u);       // v < 0: v + 2^size - 1
    bits = ((entry >> 8) << size) | low;
    len = (int)(entry & 255u) + size;
}

// One block's symbols, in order, handed to sink(slot, value, size): the DC difference against `pred`, then the AC
// coefficients with their runs of zeros, ZRL for every 16 zeros in front of a coefficient, EOB if the block ends in zeros
// (both with size 0).  slot: the symbol's place among the CODE_WORDS words of a frame's codes or histogram.
// `blk`: 64 int16 in zigzag order, 16-byte aligned; t: 0 luminance, 1 chrominance.
template <typename Sink>
__device__ __forceinline__ void walk_symbols(const int16_t *__restrict__ blk, int pred, int t, Sink &&sink)
{
    const int ac = 256 * t, dc = 512 + 16 * t;
    int run = -1;                              // (the DC's place counts as a zero below)
    for (int g = 0; g < 8; ++g) {
        uint4 v = *reinterpret_cast<const uint4 *>(blk + 8 * g);
        if (g == 0) {
            const int diff = (int)(int16_t)(v.x & 0xFFFFu) - pred;
            const int size = 32 - __clz(diff < 0 ? -diff : diff);
            sink(dc + size, diff, size);
            v.x &= 0xFFFF0000u;
        }
        if (!(v.x | v.y | v.z | v.w)) { run += 8; continue; }
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int c = (int)(int16_t)((w[j >> 1] >> (16 * (j & 1))) & 0xFFFFu);
            if (c == 0) { ++run; continue; }
            while (run > 15) { sink(ac + 0xF0, 0, 0); run -= 16; }
            const int size = 32 - __clz(c < 0 ? -c : c);
            sink(ac + ((run << 4) | size), c, size);
            run = 0;
        }
    }
    if (run > 0) sink(ac, 0, 0);
}

// The same as codes: sink(bits, len), len <= 27 (a code of at most 16 bits and a value of at most 11).
template <typename Sink>
__device__ __forceinline__ void walk_block(const int16_t *__restrict__ blk, int pred, int t, const uint32_t *s_codes, Sink &&sink)
{
    walk_symbols(blk, pred, t, [&](int slot, int v, int size) {
        uint32_t bits;
        int len;
        coded(s_codes[slot], v, size, bits, len);
        sink(bits, len);
    });
}

// The block b of an interval: where it is, whether it is a chrominance block (t), what its DC is predicted from.  An MCU
// holds hv luminance blocks, then Cb, then Cr (T.81 A.2.3); a luminance block predicts from the one coded before it, in
// this MCU or as the last of the MCU before, a chrominance block from its component's block of the MCU before.
__device__ __forceinline__ const int16_t *block_at(const int16_t *coef, long long interval, int nb, int hv, int b, int &t, int &pred)
{
    const int16_t *blk = coef + ((size_t)interval * nb + b) * 64;
    const int mcu = hv == 1 ? b / 3 : hv == 2 ? b >> 2 : b / 6, k = b - mcu * (hv + 2);
    t = k >= hv;
    const int back = t ? hv + 2 : k ? 1 : 3;             // (k = 0: behind Cr and Cb of the MCU before)
    pred = mcu || (k && !t) ? (int)blk[-64 * back] : 0;
    return blk;
}

// A WAVE takes one restart interval at a time, its lanes 64 blocks at a time.
__global__ __launch_bounds__(256) void k_mj_lengths(const int16_t *__restrict__ coef, long long intervals, int nb, int hv, int bw,
                                                    const uint32_t *__restrict__ built, uint32_t *__restrict__ bit_start,
                                                    uint32_t *__restrict__ interval_bits, uint32_t *__restrict__ bitbuf)
{
    __shared__ uint32_t s_codes[CODE_WORDS];
    load_codes(s_codes, built);
    const int lane = threadIdx.x & 63;
    long long first, end;
    span_of(intervals, first, end);
    for (long long i = first + (long long)blockIdx.x * 4 + (threadIdx.x >> 6); i < end; i += (long long)gridDim.x * 4) {
        uint32_t carry = 0;
        for (int base = 0; base < nb; base += 64) {
            const int b = base + lane;
            uint32_t mine = 0;
            if (b < nb) {
                int t, pred;
                const int16_t *blk = block_at(coef, i, nb, hv, b, t, pred);
                walk_block(blk, pred, t, s_codes, [&](uint32_t, int len) { mine += (uint32_t)len; });
            }
            const uint32_t incl = wave_inclusive(mine, lane);
            if (b < nb) bit_start[(size_t)i * nb + b] = carry + incl - mine;
            carry += (uint32_t)__shfl((int)incl, 63, 64);
        }
        if (lane == 0) interval_bits[i] = carry;
        uint32_t *words = bitbuf + (size_t)i * nb * bw;
        const uint32_t used = (carry + 31u) >> 5;                          // <= nb * bw: a block has <= 32 bw bits (BLOCK_WORDS)
        for (uint32_t w = lane; w < used; w += 64) words[w] = 0u;
    }
}

// The symbols of the frame blockIdx.y, a lane per block, counted in LDS and added to the frame's histogram (zeroed by the
// host's memset): integer sums, so the order does not matter.
__global__ __launch_bounds__(256) void k_mj_hist(const int16_t *__restrict__ coef, int frame_intervals, int nb, int hv,
                                                 uint32_t *__restrict__ hist)
{
    __shared__ uint32_t s_hist[CODE_WORDS];
    for (int k = threadIdx.x; k < CODE_WORDS; k += 256) s_hist[k] = 0u;
    __syncthreads();
    const long long i0 = (long long)blockIdx.y * frame_intervals;
    const int blocks = frame_intervals * nb;
    for (int gb = blockIdx.x * 256 + threadIdx.x; gb < blocks; gb += gridDim.x * 256) {
        const int r = gb / nb;
        int t, pred;
        const int16_t *blk = block_at(coef, i0 + r, nb, hv, gb - r * nb, t, pred);
        walk_symbols(blk, pred, t, [&](int slot, int, int) { atomicAdd(&s_hist[slot], 1u); });
    }
    __syncthreads();
    for (int k = threadIdx.x; k < CODE_WORDS; k += 256)
        if (s_hist[k]) atomicAdd(&hist[(size_t)blockIdx.y * CODE_WORDS + k], s_hist[k]);
}

// ONE WORKGROUP per (table, frame): blockIdx.x = 0 DC luminance, 1 AC luminance, 2 DC chrominance, 3 AC chrominance, the
// order of the DHT segments.  The code lengths are those of png_codes.h with a limit of 16 bits over an alphabet of 257:
// entry 0 is the pseudo-symbol of T.81 K.2 with the count 1, entry s + 1 the symbol s.  Being the first of the lightest, the
// pseudo-symbol is the LAST to be given a length and so has a longest one; it is then left out, which leaves the last code of
// that length, the one of all 1-bits, unused.  Codes are canonical (T.81 Annex C): by length, then by symbol.  What is
// independent per symbol, leaf or length is spread over the threads, as k_png_dcodes does (png.hip).
// Out: the frame's code words ((code << 8) | length), the DHT segment and its length.
__global__ __launch_bounds__(256) void k_mj_tables(const uint32_t *__restrict__ hist, uint32_t *__restrict__ built,
                                                   uint8_t *__restrict__ dht, uint32_t *__restrict__ dht_bytes)
{
    namespace pc = ysmr::pngc;
    constexpr int N = 257;
    __shared__ pc::Work w;
    __shared__ uint32_t s_counts[N], s_first[17], s_before[17];
    __shared__ uint8_t s_len[N];
    __shared__ int s_used;
    const int t = threadIdx.x, tb = blockIdx.x, f = blockIdx.y;
    const int ac = tb & 1, slot0 = ac ? 256 * (tb >> 1) : 512 + 16 * (tb >> 1), n_sym = ac ? 256 : 16;
    const uint32_t *h = hist + (size_t)f * CODE_WORDS + slot0;
    for (int s = t; s < N; s += 256) s_counts[s] = s == 0 ? 1u : s <= n_sym ? h[s - 1] : 0u;
    __syncthreads();
    if (t == 0) s_used = pc::used_of(s_counts, N);
    __syncthreads();
    const int m = s_used;                                      // >= 2: the pseudo-symbol, and a block has a DC and an AC symbol
    for (int s = t; s < N; s += 256) {
        s_len[s] = 0;
        if (s_counts[s]) w.order[pc::rank_of(s_counts, N, s)] = (uint16_t)s;
    }
    __syncthreads();
    for (int i = t; i < m; i += 256) pc::leaf_weight(s_counts, i, w);
    __syncthreads();
    if (t == 0) pc::huffman_links(m, w);
    __syncthreads();
    for (int i = t; i < m; i += 256) pc::leaf_depth(m, i, w);
    __syncthreads();
    if (t >= 1 && t <= 16) pc::count_depth(m, 16, t, w);
    __syncthreads();
    if (t == 0) pc::limit_lengths(m, 16, w);
    __syncthreads();
    for (int i = t; i < m; i += 256) pc::assign_length(m, 16, i, s_len, w);
    __syncthreads();
    if (t >= 1 && t <= 16) {                                   // BITS: the symbols (without the pseudo-symbol) of every length
        uint32_t c = 0;
#pragma nounroll
        for (int s = 1; s < N; ++s) c += s_len[s] == t;
        w.num[t] = c;
    }
    __syncthreads();
    if (t == 0) {
        uint32_t code = 0, before = 0;
#pragma nounroll
        for (int len = 1; len <= 16; ++len) {
            s_first[len] = code;
            s_before[len] = before;
            code = (code + w.num[len]) << 1;
            before += w.num[len];
        }
        s_before[0] = before;                                  // the number of symbols
    }
    __syncthreads();
    uint8_t *seg = dht + ((size_t)f * 4 + tb) * DHT_STRIDE;
    const uint32_t n_vals = s_before[0], body = 19 + n_vals;
    for (int s = t + 1; s <= n_sym; s += 256) {
        const int len = s_len[s];
        uint32_t entry = 0;
        if (len) {
            uint32_t earlier = 0;
#pragma nounroll
            for (int u = 1; u < s; ++u) earlier += s_len[u] == len;
            entry = ((s_first[len] + earlier) << 8) | (uint32_t)len;
            seg[21 + s_before[len] + earlier] = (uint8_t)(s - 1);
        }
        built[(size_t)f * CODE_WORDS + slot0 + s - 1] = entry;
    }
    if (t < 21)
        seg[t] = t == 0 ? 0xFFu : t == 1 ? 0xC4u : t == 2 ? (uint8_t)(body >> 8) : t == 3 ? (uint8_t)body
               : t == 4 ? (uint8_t)((ac << 4) | (tb >> 1)) : (uint8_t)w.num[t - 4];
    if (t == 0) dht_bytes[f * 4 + tb] = 21 + n_vals;
}

// A LANE takes one block.  The stream is big-endian bit by bit, the buffer is made of little-endian words: 32 finished bits
// are byte-swapped and OR-ed into their word.
__global__ __launch_bounds__(256) void k_mj_pack(const int16_t *__restrict__ coef, long long intervals, int nb, int hv, int bw,
                                                 const uint32_t *__restrict__ built, const uint32_t *__restrict__ bit_start,
                                                 const uint32_t *__restrict__ interval_bits, uint32_t *__restrict__ bitbuf)
{
    __shared__ uint32_t s_codes[CODE_WORDS];
    load_codes(s_codes, built);
    long long first, end;
    span_of(intervals, first, end);
    const long long total = end * nb;
    for (long long gb = first * nb + (long long)blockIdx.x * blockDim.x + threadIdx.x; gb < total; gb += (long long)gridDim.x * blockDim.x) {
        const long long i = gb / nb;
        const int b = (int)(gb - i * nb);
        int t, pred;
        const int16_t *blk = block_at(coef, i, nb, hv, b, t, pred);
        uint32_t *words = bitbuf + (size_t)i * nb * bw;
        const uint32_t start = bit_start[gb];
        uint32_t wi = start >> 5;
        int fill = (int)(start & 31u);
        uint64_t acc = 0;
        auto put = [&](uint32_t bits, int len) {
            acc |= (uint64_t)bits << (64 - fill - len);                   // fill < 32, len <= 27
            fill += len;
            if (fill >= 32) {
                atomicOr(&words[wi++], __builtin_bswap32((uint32_t)(acc >> 32)));
                acc <<= 32;
                fill -= 32;
            }
        };
        walk_block(blk, pred, t, s_codes, put);
        if (b == nb - 1) {                                                 // the interval ends here: 1-bits up to a byte
            const int pad = (int)(-interval_bits[i] & 7u);
            if (pad) put((1u << pad) - 1u, pad);
        }
        if (fill > 0) atomicOr(&words[wi], __builtin_bswap32((uint32_t)(acc >> 32)));
    }
}

__device__ __forceinline__ uint32_t count_ff(uint32_t v)
{
    return ((v & 0xFFu) == 0xFFu) + ((v & 0xFF00u) == 0xFF00u) + ((v & 0xFF0000u) == 0xFF0000u) + ((v >> 24) == 0xFFu);
}

// A WAVE takes one interval: bytes + 0xFF bytes (+ 2 for the RST marker behind every interval of a frame but the last).  The
// bytes of the last word beyond the interval's end are zero (k_mj_lengths zeroed whole words).
__global__ __launch_bounds__(256) void k_mj_count(const uint32_t *__restrict__ bitbuf, const uint32_t *__restrict__ interval_bits,
                                                  long long intervals, int nb, int bw, int H8, uint32_t *__restrict__ interval_size)
{
    const int lane = threadIdx.x & 63;
    for (long long i = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); i < intervals; i += (long long)gridDim.x * 4) {
        const uint32_t *words = bitbuf + (size_t)i * nb * bw;
        const uint32_t bytes = (interval_bits[i] + 7u) >> 3, used = (bytes + 3u) >> 2;
        uint32_t ff = 0;
        for (uint32_t w = lane; w < used; w += 64) ff += count_ff(words[w]);
        ff = (uint32_t)__shfl((int)wave_inclusive(ff, lane), 63, 64);
        if (lane == 0) interval_size[i] = bytes + ff + ((int)(i % H8) < H8 - 1 ? 2u : 0u);
    }
}

// SOI .. SOS header of frame f: with built tables (dht_bytes: the frame's four segment lengths) it varies per frame.
__device__ __forceinline__ uint32_t header_bytes(const uint32_t *__restrict__ dht_bytes, long long f)
{
    if (!dht_bytes) return HEADER_BYTES;
    const uint32_t *d = dht_bytes + 4 * f;
    return HEADER_FRONT + d[0] + d[1] + d[2] + d[3] + HEADER_BACK;
}

// ONE WORKGROUP.  A thread sums the intervals of a frame; wave 0 scans the chunk sizes 64 frames at a time; a thread then
// places its frame's intervals.
__global__ __launch_bounds__(256) void k_mj_layout(const uint32_t *__restrict__ interval_size, int n, int H8, size_t out_capacity,
                                                   const uint32_t *__restrict__ dht_bytes, uint32_t *__restrict__ payload,
                                                   long long *__restrict__ interval_at, long long *__restrict__ offsets,
                                                   int *__restrict__ status)
{
    for (int f = threadIdx.x; f < n; f += 256) {
        uint32_t sum = header_bytes(dht_bytes, f) + 2;
        for (int r = 0; r < H8; ++r) sum += interval_size[(size_t)f * H8 + r];
        payload[f] = sum;
    }
    __syncthreads();
    if (threadIdx.x < 64) {
        const int lane = threadIdx.x;
        long long carry = 0;
        for (int base = 0; base < n; base += 64) {
            const int f = base + lane;
            const long long mine = f < n ? 8ll + payload[f] + (payload[f] & 1u) : 0ll;
            long long incl = mine;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const long long o = __shfl_up(incl, d, 64);
                if (lane >= d) incl += o;
            }
            if (f < n) offsets[f] = carry + incl - mine;
            carry += __shfl(incl, 63, 64);
        }
        if (lane == 0) {
            offsets[n] = carry;
            *status = (unsigned long long)carry > (unsigned long long)out_capacity ? 1 : 0;
        }
    }
    __syncthreads();
    for (int f = threadIdx.x; f < n; f += 256) {
        long long at = offsets[f] + 8 + header_bytes(dht_bytes, f);
        for (int r = 0; r < H8; ++r) {
            interval_at[(size_t)f * H8 + r] = at;
            at += interval_size[(size_t)f * H8 + r];
        }
    }
}

// A WAVE takes one interval, a lane four of its packed bytes at a time: how many bytes they become (one more for every
// 0xFF), a prefix sum, the bytes.  Nothing at or beyond out_capacity is written.
__global__ __launch_bounds__(256) void k_mj_write(const uint32_t *__restrict__ bitbuf, const uint32_t *__restrict__ interval_bits,
                                                  const long long *__restrict__ interval_at, const long long *__restrict__ offsets,
                                                  const uint32_t *__restrict__ payload, long long intervals, int nb, int bw, int H8,
                                                  Header head, const uint8_t *__restrict__ dht, const uint32_t *__restrict__ dht_bytes,
                                                  uint8_t *__restrict__ out, size_t out_capacity)
{
    const int lane = threadIdx.x & 63;
    auto store = [&](long long at, uint32_t byte) {
        if ((unsigned long long)at < (unsigned long long)out_capacity) out[at] = (uint8_t)byte;
    };
    for (long long i = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); i < intervals; i += (long long)gridDim.x * 4) {
        const long long f = i / H8;
        const int r = (int)(i - f * H8);
        const uint32_t *words = bitbuf + (size_t)i * nb * bw;
        const uint32_t bytes = (interval_bits[i] + 7u) >> 3;
        const long long at0 = interval_at[i];
        uint32_t carry = 0;
        for (uint32_t base = 0; base < bytes; base += 256) {
            const uint32_t first = base + 4u * lane, mine = first < bytes ? std::min(4u, bytes - first) : 0u;
            const uint32_t v = mine ? words[first >> 2] : 0u;
            const uint32_t grown = mine + count_ff(v);
            const uint32_t incl = wave_inclusive(grown, lane);
            long long at = at0 + carry + (incl - grown);
#pragma unroll
            for (uint32_t k = 0; k < 4; ++k)
                if (k < mine) {
                    const uint32_t byte = (v >> (8 * k)) & 0xFFu;
                    store(at++, byte);
                    if (byte == 0xFFu) store(at++, 0u);
                }
            carry += (uint32_t)__shfl((int)incl, 63, 64);
        }
        const long long chunk = offsets[f];
        const uint32_t size = payload[f];
        if (lane == 0) {
            store(at0 + carry, 0xFFu);
            if (r < H8 - 1) store(at0 + carry + 1, 0xD0u + (uint32_t)(r & 7));
            else {
                store(at0 + carry + 1, 0xD9u);
                if (size & 1u) store(chunk + 8 + size, 0u);
            }
        }
        if (r == 0) {
            // `head` is the whole header with the Annex K.3 tables; the frame's own DHT segments take their place between
            // its front and its back
            const uint32_t *d = dht_bytes ? dht_bytes + 4 * f : nullptr;
            const int d0 = d ? (int)d[0] : 0, d1 = d ? d0 + (int)d[1] : 0, d2 = d ? d1 + (int)d[2] : 0;
            const int d3 = d ? d2 + (int)d[3] : HEADER_BYTES - HEADER_FRONT - HEADER_BACK;
            for (int k = lane; k < 8 + HEADER_FRONT + d3 + HEADER_BACK; k += 64) {
                const uint32_t tag = 0x63643030u;                           // '00dc'
                const int j = k - 8 - HEADER_FRONT;                         // (the place among the DHT segments)
                uint32_t byte;
                if (k < 8) byte = k < 4 ? (tag >> (8 * k)) & 0xFFu : (size >> (8 * (k - 4))) & 0xFFu;
                else if (!d || j < 0) byte = head.b[k - 8];
                else if (j >= d3) byte = head.b[HEADER_BYTES - HEADER_BACK + j - d3];
                else {
                    const int tb = (j >= d0) + (j >= d1) + (j >= d2);
                    byte = dht[((size_t)f * 4 + tb) * DHT_STRIDE + (j - (tb == 0 ? 0 : tb == 1 ? d0 : tb == 2 ? d1 : d2))];
                }
                store(chunk + k, byte);
            }
        }
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------------
// W8, H8: the frame in MCUs (8 h x 8 v pixels); hv = h v luminance blocks per MCU; nb: blocks per interval; bw: words of bit
// buffer per block.  hist .. dht_bytes exist only with built tables.
struct Plan {
    size_t coef, bit_start, interval_bits, interval_size, interval_at, payload, bitbuf, hist, built, dht, dht_bytes, total;
    long long intervals;
    int W8, H8, nb, h, v, hv, bw;
};

Plan plan_of(int n, int H, int W, int sampling, int huffman)
{
    Plan p;
    p.h = sampling == 1 ? 1 : 2; p.v = sampling == 3 ? 2 : 1; p.hv = p.h * p.v;
    p.W8 = (W + 8 * p.h - 1) / (8 * p.h); p.H8 = (H + 8 * p.v - 1) / (8 * p.v); p.nb = (p.hv + 2) * p.W8;
    p.bw = huffman ? BLOCK_WORDS_BUILT : BLOCK_WORDS;
    p.intervals = (long long)n * p.H8;
    const size_t blocks = (size_t)p.intervals * p.nb;
    size_t at = 0;
    auto take = [&](size_t bytes) { const size_t here = at; at += ysmr::align_up(bytes, 256); return here; };
    p.coef = take(blocks * 128);
    p.bit_start = take(blocks * 4);
    p.interval_bits = take((size_t)p.intervals * 4);
    p.interval_size = take((size_t)p.intervals * 4);
    p.interval_at = take((size_t)p.intervals * 8);
    p.payload = take((size_t)n * 4);
    p.bitbuf = take(blocks * p.bw * 4);
    p.hist = p.built = p.dht = p.dht_bytes = 0;
    if (huffman) {
        p.hist = take((size_t)n * CODE_WORDS * 4);
        p.built = take((size_t)n * CODE_WORDS * 4);
        p.dht = take((size_t)n * 4 * DHT_STRIDE);
        p.dht_bytes = take((size_t)n * 4 * 4);
    }
    p.total = at;
    return p;
}

void quant_tables(int quality, Quant &qt)
{
    const int s = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    for (int k = 0; k < 64; ++k) {
        qt.q[0][k] = (uint32_t)std::min(255, std::max(1, (K1_LUM[k] * s + 50) / 100));
        qt.q[1][k] = (uint32_t)std::min(255, std::max(1, (K1_CHR[k] * s + 50) / 100));
    }
}

int header_of(int H, int W, const Plan &plan, const Quant &qt, Header &h)
{
    uint8_t *p = h.b;
    auto put = [&](int v) { *p++ = (uint8_t)v; };
    auto marker = [&](int m, int body) { put(0xFF); put(m); put((body + 2) >> 8); put((body + 2) & 255); };
    put(0xFF); put(0xD8);
    marker(0xE0, 14);
    put('A'); put('V'); put('I'); put('1');
    for (int k = 0; k < 10; ++k) put(0);
    marker(0xDB, 130);
    for (int t = 0; t < 2; ++t) {
        put(t);
        for (int k = 0; k < 64; ++k) put((int)qt.q[t][ZIGZAG[k]]);
    }
    marker(0xC0, 15);
    put(8); put(H >> 8); put(H & 255); put(W >> 8); put(W & 255); put(3);
    for (int c = 0; c < 3; ++c) { put(c + 1); put(c ? 0x11 : (plan.h << 4) | plan.v); put(c ? 1 : 0); }
    const struct { int id, n; const uint8_t *bits, *vals; } tables[4] = {
        {0x00, 12, DC_LUM_BITS, DC_VALS}, {0x10, 162, AC_LUM_BITS, AC_LUM_VALS},
        {0x01, 12, DC_CHR_BITS, DC_VALS}, {0x11, 162, AC_CHR_BITS, AC_CHR_VALS}};
    for (const auto &t : tables) {
        marker(0xC4, 17 + t.n);
        put(t.id);
        for (int k = 0; k < 16; ++k) put(t.bits[k]);
        for (int k = 0; k < t.n; ++k) put(t.vals[k]);
    }
    const int dri = plan.W8;
    marker(0xDD, 2);
    put(dri >> 8); put(dri & 255);
    marker(0xDA, 10);
    put(3); put(1); put(0x00); put(2); put(0x11); put(3); put(0x11); put(0); put(63); put(0);
    return (int)(p - h.b);
}

unsigned grid_of(long long items, int per_block)
{
    return (unsigned)std::max<long long>(1, std::min<long long>((items + per_block - 1) / per_block, MAX_GRID));
}

bool geometry_ok(int n, int H, int W)
{
    // (SOF0 and DRI hold 16 bits each; the bit offsets of an interval 32)
    return n > 0 && H > 0 && W > 0 && H <= 65535 && W <= 65535;
}

bool mode_ok(int sampling, int huffman) { return sampling >= 1 && sampling <= 3 && (huffman == 0 || huffman == 1); }

}  // namespace

extern "C" size_t ysmr_mjpeg_encode_workspace_bytes(int n_frames, int height, int width, int sampling, int huffman)
{
    if (!geometry_ok(n_frames, height, width) || !mode_ok(sampling, huffman)) return 0;
    return plan_of(n_frames, height, width, sampling, huffman).total;
}

extern "C" size_t ysmr_mjpeg_workspace_bytes(int n_frames, int height, int width)
{
    return ysmr_mjpeg_encode_workspace_bytes(n_frames, height, width, 1, 0);
}

extern "C" int ysmr_mjpeg_encode_batch(void *stream, const uint8_t *dib_dev, int n_frames, int height, int width, int stride,
                                       size_t frame_bytes, int bottom_up, int quality, int sampling, int huffman,
                                       void *workspace_dev, size_t workspace_bytes, uint8_t *out_dev, size_t out_capacity,
                                       int64_t *offsets_dev, int32_t *status_dev)
{
    if (!geometry_ok(n_frames, height, width))
        return ysmr::fail(YSMR_ERR_ARG, "n_frames must be positive, height and width 1 .. 65535 (got %d, %d, %d)", n_frames, height, width);
    if (quality < 1 || quality > 100) return ysmr::fail(YSMR_ERR_ARG, "quality must be 1 .. 100, got %d", quality);
    if (!mode_ok(sampling, huffman))
        return ysmr::fail(YSMR_ERR_ARG, "sampling must be 1 (4:4:4), 2 (4:2:2) or 3 (4:2:0) and huffman 0 or 1, got %d and %d", sampling,
                          huffman);
    if (huffman && n_frames > 65535) return ysmr::fail(YSMR_ERR_ARG, "at most 65535 frames per call with huffman = 1, got %d", n_frames);
    if ((long long)stride < 3LL * width || (stride & 3) || frame_bytes < (size_t)stride * height)
        return ysmr::fail(YSMR_ERR_ARG, "stride %d (a multiple of 4) / frame_bytes %zu too small for %d x %d x 3", stride, frame_bytes,
                          width, height);
    if (!dib_dev || !workspace_dev || !out_dev || !offsets_dev || !status_dev)
        return ysmr::fail(YSMR_ERR_ARG, "dib_dev, workspace_dev, out_dev, offsets_dev and status_dev must not be NULL");
    const Plan p = plan_of(n_frames, height, width, sampling, huffman);
    if (workspace_bytes < p.total)
        return ysmr::fail(YSMR_ERR_ARG, "workspace of %zu bytes, %zu needed (ysmr_mjpeg_encode_workspace_bytes)", workspace_bytes, p.total);
    if (((uintptr_t)workspace_dev & 255) || ((uintptr_t)offsets_dev & 7) || ((uintptr_t)status_dev & 3))
        return ysmr::fail(YSMR_ERR_ARG, "workspace_dev must be 256-byte aligned, offsets_dev 8-byte, status_dev 4-byte");
    Quant qt;
    Header head = {};
    quant_tables(quality, qt);
    if (header_of(height, width, p, qt, head) != HEADER_BYTES) return ysmr::fail(YSMR_ERR_STATE, "JPEG header is not %d bytes", HEADER_BYTES);

    hipStream_t st = (hipStream_t)stream;
    uint8_t *ws = (uint8_t *)workspace_dev;
    int16_t *coef = (int16_t *)(ws + p.coef);
    uint32_t *bit_start = (uint32_t *)(ws + p.bit_start), *interval_bits = (uint32_t *)(ws + p.interval_bits);
    uint32_t *interval_size = (uint32_t *)(ws + p.interval_size), *payload = (uint32_t *)(ws + p.payload);
    uint32_t *bitbuf = (uint32_t *)(ws + p.bitbuf);
    long long *interval_at = (long long *)(ws + p.interval_at);
    // with built tables: the frame is the grid's y in the kernels that hold one frame's codes or histogram in LDS
    uint32_t *hist = huffman ? (uint32_t *)(ws + p.hist) : nullptr, *built = huffman ? (uint32_t *)(ws + p.built) : nullptr;
    uint32_t *dht_bytes = huffman ? (uint32_t *)(ws + p.dht_bytes) : nullptr;
    uint8_t *dht = huffman ? ws + p.dht : nullptr;
    const unsigned gy = huffman ? (unsigned)n_frames : 1u;
    const long long mcus = p.intervals * p.W8, per_y = huffman ? p.H8 : p.intervals;
    if (sampling == 1)
        hipLaunchKernelGGL(k_mj_blocks, dim3(grid_of(mcus, 4)), dim3(256), 0, st, dib_dev, n_frames, height, width, stride, frame_bytes,
                           bottom_up, qt, coef);
    else
        hipLaunchKernelGGL(k_mj_blocks_sampled, dim3(grid_of(mcus, 4)), dim3(256), 0, st, dib_dev, n_frames, height, width, stride,
                           frame_bytes, bottom_up, p.v, qt, coef);
    YSMR_LAUNCH_CHECK();
    if (huffman) {
        YSMR_HIP_CHECK(hipMemsetAsync(hist, 0, (size_t)n_frames * CODE_WORDS * 4, st));
        hipLaunchKernelGGL(k_mj_hist, dim3(grid_of((long long)p.H8 * p.nb, 256), gy), dim3(256), 0, st, coef, p.H8, p.nb, p.hv, hist);
        YSMR_LAUNCH_CHECK();
        hipLaunchKernelGGL(k_mj_tables, dim3(4, gy), dim3(256), 0, st, hist, built, dht, dht_bytes);
        YSMR_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(k_mj_lengths, dim3(grid_of(per_y, 4), gy), dim3(256), 0, st, coef, p.intervals, p.nb, p.hv, p.bw, built, bit_start,
                       interval_bits, bitbuf);
    YSMR_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_mj_pack, dim3(grid_of(per_y * p.nb, 256), gy), dim3(256), 0, st, coef, p.intervals, p.nb, p.hv, p.bw, built,
                       bit_start, interval_bits, bitbuf);
    YSMR_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_mj_count, dim3(grid_of(p.intervals, 4)), dim3(256), 0, st, bitbuf, interval_bits, p.intervals, p.nb, p.bw, p.H8,
                       interval_size);
    YSMR_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_mj_layout, dim3(1), dim3(256), 0, st, interval_size, n_frames, p.H8, out_capacity, dht_bytes, payload,
                       interval_at, (long long *)offsets_dev, (int *)status_dev);
    YSMR_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_mj_write, dim3(grid_of(p.intervals, 4)), dim3(256), 0, st, bitbuf, interval_bits, interval_at,
                       (const long long *)offsets_dev, payload, p.intervals, p.nb, p.bw, p.H8, head, dht, dht_bytes, out_dev, out_capacity);
    YSMR_LAUNCH_CHECK();
    return YSMR_OK;
}

extern "C" int ysmr_mjpeg_batch(void *stream, const uint8_t *dib_dev, int n_frames, int height, int width, int stride,
                                size_t frame_bytes, int bottom_up, int quality, void *workspace_dev, size_t workspace_bytes,
                                uint8_t *out_dev, size_t out_capacity, int64_t *offsets_dev, int32_t *status_dev)
{
    return ysmr_mjpeg_encode_batch(stream, dib_dev, n_frames, height, width, stride, frame_bytes, bottom_up, quality, 1, 0, workspace_dev,
                                   workspace_bytes, out_dev, out_capacity, offsets_dev, status_dev);
}


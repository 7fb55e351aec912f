// mjpeg_decode.hip -- frame ingest from a Motion-JPEG AVI: the '00dc' chunk bodies as they are in the file become frames in the
// layout ysmr_threshold_batch reads, without the host.  tests/jpeg_decode_model.py is the specification (and the kernels are
// tested against it byte for byte, status for status); ITS yardstick is what Pillow's libjpeg-turbo delivers on the host path.
// SUPPORTED: baseline sequential JPEG (SOF0, 8 bit, Huffman), ONE interleaved scan of all components; one component 1 x 1, or
// three (ids 1, 2, 3) with luminance 1 x 1, 2 x 1 or 2 x 2 and both chrominances 1 x 1.  Everything else, and every stream that
// contradicts itself, sets the frame's status and leaves its pixels to the caller (DeviceFrameFeed decodes them on the host).
// FIVE LAUNCHES and one memset on the caller's stream, nothing between them but the workspace:
//   k_mjd_headers  a lane per frame: the marker walk up to SOS -- DQT, SOF0, DHT (else Annex K.3), DRI, SOS --, geometry and
//                  sampling checked against the call's; the frame's tables go to the workspace (frames of a batch may differ)
//   k_mjd_markers  a workgroup per frame, 16 bytes per thread and step: the RSTn positions in file order (a scan places them)
//                  and the first other marker, which ends the entropy data; count and sequence of the RSTn are checked
//   k_mjd_entropy  a lane per restart interval (the lanes of a wave take neighbouring intervals of ONE frame, whose tables
//                  sit in LDS behind a 9-bit look-up); the bit reader is bounded by the interval's end, every coefficient
//                  index is checked before its store -> int16 coef[frame][block][64], natural order, zeroed by the memset
//   k_mjd_idct     eight threads per block: dequantise, columns, rows (through LDS), clamp -> sample planes (gray: the frame)
//   k_mjd_colour   a thread per pixel: fancy upsampling of the chrominance planes, 16-bit fixed-point colour -> B, G, R
// ysmr_mjpeg_decode_batch_sync is the same call for files WITHOUT restart markers (what cameras, ffmpeg, OpenCV and Pillow write): a
// frame with a restart interval takes k_mjd_entropy as above, one without takes k_mjd_destuff, k_mjd_sync and k_mjd_dc (below,
// "entropy decode of a frame WITHOUT restart markers"), which decode it with a lane per 64 bytes instead of one per frame.
// No kernel writes outside the workspace, status_dev and the frame's own H * W * channels bytes; every read of chunks_dev lies
// inside the frame's own [offsets[i], offsets[i + 1]).
#include "common.h"
#include "mjpeg_decode_plan.h"
#include <algorithm>

namespace {

constexpr int MAX_GRID = 2048;
constexpr int ENTROPY_GRID_X = 32;           // workgroups per frame at most; each takes 64 intervals at a time
constexpr int LUT_BITS = 9;

// ---- tables of the standard: Annex K.3, codes per length 1 .. 16, then the symbols in code order ------------------------------
struct StdTable { uint8_t bits[16]; uint8_t vals[256]; };
__constant__ StdTable c_std[4] = {
    // DC luminance, DC chrominance
    {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}},
    {{0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}},
    // AC luminance, AC chrominance
    {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7D},
     {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91,
      0xA1, 0x08, 0x23, 0x42, 0xB1, 0xC1, 0x15, 0x52, 0xD1, 0xF0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0A, 0x16, 0x17, 0x18, 0x19, 0x1A,
      0x25, 0x26, 0x27, 0x28, 0x29, 0x2A, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4A, 0x53,
      0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79,
      0x7A, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9A, 0xA2, 0xA3, 0xA4, 0xA5,
      0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4, 0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3, 0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9,
      0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA, 0xE1, 0xE2, 0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF1, 0xF2,
      0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9, 0xFA}},
    {{0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77},
     {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14,
      0x42, 0x91, 0xA1, 0xB1, 0xC1, 0x09, 0x23, 0x33, 0x52, 0xF0, 0x15, 0x62, 0x72, 0xD1, 0x0A, 0x16, 0x24, 0x34, 0xE1, 0x25, 0xF1, 0x17,
      0x18, 0x19, 0x1A, 0x26, 0x27, 0x28, 0x29, 0x2A, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4A,
      0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78,
      0x79, 0x7A, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9A, 0xA2, 0xA3,
      0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4, 0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3, 0xC4, 0xC5, 0xC6, 0xC7,
      0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA, 0xE2, 0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF2,
      0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9, 0xFA}}};
// natural index (8 * row + column) of the k-th coefficient of the zigzag sequence
__constant__ uint8_t c_zigzag[64] = {0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,
                                     7, 14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31,
                                     39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// the geometry of a call, what k_mjd_headers leaves per frame and the workspace's layout: mjpeg_decode_plan.h (host-only code)
using mjd::FrameInfo;
using mjd::Geo;
using mjd::geometry_of;
using mjd::HuffRaw;
using mjd::Plan;
using mjd::plan_of;

// the part of the geometry the serial kernels need (a kernel's arguments live in scalar registers, and these kernels have few to spare)
struct SmallGeo { int H, W, nc, lh, lv, mx, mcus, ycols, ccols, blocks_y, blocks_c, blocks; };

// ---- headers -----------------------------------------------------------------------------------------------------------------
// A LANE walks the markers of one frame; `at(p)` never reads outside the frame.  The checks come in the order of the model's, so
// that a stream with two faults gets the status of the first.
__global__ __launch_bounds__(64) void k_mjd_headers(const uint8_t *__restrict__ chunks, const long long *__restrict__ offsets, int n, SmallGeo g,
                                                    FrameInfo *__restrict__ info, uint16_t *__restrict__ quant, HuffRaw *__restrict__ huff,
                                                    int *__restrict__ status)
{
    const int f = blockIdx.x * 64 + threadIdx.x;
    if (f >= n) return;
    const long long off = offsets[f], len64 = offsets[f + 1] - off;
    const uint8_t *base = chunks + off;
    const int len = (int)std::min<long long>(std::max<long long>(len64, 0), 0x7FFFFFF0);
    auto at = [&](int p) -> uint32_t { return p < len ? base[p] : 0u; };
    uint16_t *q = quant + (size_t)f * 256;
    HuffRaw *hf = huff + (size_t)f * 8;
    FrameInfo fi = {};
    uint32_t ids = 0, quant_defined = 0, standard = 0;
    bool have_sof = false;
    int st = 0, pos = 2;
    if (len64 != len || len < 4 || at(0) != 0xFF || at(1) != 0xD8) st = YSMR_MJPEGD_CORRUPT;
    while (!st) {
        if (pos >= len || at(pos) != 0xFF) { st = YSMR_MJPEGD_CORRUPT; break; }
        while (pos < len && at(pos) == 0xFF) ++pos;
        if (pos >= len) { st = YSMR_MJPEGD_CORRUPT; break; }
        const uint32_t marker = at(pos++);
        if (marker == 0x01 || (marker >= 0xD0 && marker <= 0xD8)) continue;
        if (marker == 0xD9 || marker == 0x00 || pos + 2 > len) { st = YSMR_MJPEGD_CORRUPT; break; }
        const int length = (int)((at(pos) << 8) | at(pos + 1));
        if (length < 2 || pos + length > len) { st = YSMR_MJPEGD_CORRUPT; break; }
        const int body = pos + 2, blen = length - 2;
        if (marker == 0xDB) {
            #pragma nounroll
            for (int a = 0; a < blen && !st; a += 65) {
                const uint32_t pq_tq = at(body + a);
                if (pq_tq >> 4) st = YSMR_MJPEGD_UNSUPPORTED;
                else if ((pq_tq & 15) > 3 || a + 65 > blen) st = YSMR_MJPEGD_CORRUPT;
                else {
                    #pragma nounroll
                    for (int k = 0; k < 64; ++k) q[(pq_tq & 15) * 64 + c_zigzag[k]] = (uint16_t)at(body + a + 1 + k);
                    quant_defined |= 1u << (pq_tq & 15);
                }
            }
        } else if (marker == 0xC0) {
            if (have_sof) st = YSMR_MJPEGD_UNSUPPORTED;
            else if (blen < 6 || blen != 6 + 3 * (int)at(body + 5)) st = YSMR_MJPEGD_CORRUPT;
            else if (at(body) != 8 || (int)((at(body + 1) << 8) | at(body + 2)) != g.H || (int)((at(body + 3) << 8) | at(body + 4)) != g.W ||
                     (int)at(body + 5) != g.nc)
                st = YSMR_MJPEGD_UNSUPPORTED;
            else {
                have_sof = true;
                #pragma nounroll
                for (int c = 0; c < g.nc && !st; ++c) {
                    const uint32_t id = at(body + 6 + 3 * c), hv = at(body + 7 + 3 * c), tq = at(body + 8 + 3 * c);
                    const uint32_t want = c == 0 ? (uint32_t)((g.lh << 4) | g.lv) : 0x11u;
                    if (hv != want || (g.nc == 3 && id != (uint32_t)c + 1)) st = YSMR_MJPEGD_UNSUPPORTED;
                    else if (tq > 3) st = YSMR_MJPEGD_CORRUPT;
                    ids |= id << (8 * c);
                    fi.tq |= tq << (8 * c);
                }
            }
        } else if (marker == 0xC4) {
            #pragma nounroll
            for (int a = 0; a < blen && !st;) {
                const uint32_t tc = at(body + a) >> 4, th = at(body + a) & 15;
                if (tc > 1 || th > 3 || a + 17 > blen) { st = YSMR_MJPEGD_CORRUPT; break; }
                HuffRaw *t = hf + tc * 4 + th;
                int count = 0;
                uint32_t code = 0;
                bool fits = true;
                #pragma nounroll
                for (int l = 1; l <= 16; ++l) {
                    const uint32_t b = at(body + a + l);
                    t->bits[l - 1] = (uint8_t)b;
                    count += (int)b;
                    code += b;
                    if (b && code > (1u << l)) fits = false;
                    code <<= 1;
                }
                if (count > 256 || a + 17 + count > blen || !fits) { st = YSMR_MJPEGD_CORRUPT; break; }
                #pragma nounroll
                for (int k = 0; k < count; ++k) t->vals[k] = (uint8_t)at(body + a + 17 + k);
                fi.defined |= 1u << (tc * 4 + th);
                a += 17 + count;
            }
        } else if (marker == 0xDD) {
            if (length != 4) st = YSMR_MJPEGD_CORRUPT;
            else fi.ri = (int)((at(body) << 8) | at(body + 1));
        } else if (marker == 0xEE || (marker >= 0xC1 && marker <= 0xCF && marker != 0xC8)) {
            st = YSMR_MJPEGD_UNSUPPORTED;
        } else if (marker == 0xDA) {
            if (!have_sof || blen < 1 || blen != 4 + 2 * (int)at(body)) st = YSMR_MJPEGD_CORRUPT;
            else if ((int)at(body) != g.nc) st = YSMR_MJPEGD_UNSUPPORTED;
            #pragma nounroll
            for (int c = 0; c < g.nc && !st; ++c) {
                const uint32_t sel = at(body + 1 + 2 * c), td = at(body + 2 + 2 * c) >> 4, ta = at(body + 2 + 2 * c) & 15;
                if (sel != ((ids >> (8 * c)) & 255)) st = YSMR_MJPEGD_UNSUPPORTED;
                else if (td > 3 || ta > 3) st = YSMR_MJPEGD_CORRUPT;
                fi.td |= td << (8 * c);
                fi.ta |= ta << (8 * c);
            }
            if (!st && (at(body + 1 + 2 * g.nc) != 0 || at(body + 2 + 2 * g.nc) != 63 || at(body + 3 + 2 * g.nc) != 0)) st = YSMR_MJPEGD_UNSUPPORTED;
            #pragma nounroll
            for (int c = 0; c < g.nc && !st; ++c) {
                if (!((quant_defined >> ((fi.tq >> (8 * c)) & 255)) & 1)) { st = YSMR_MJPEGD_CORRUPT; break; }
                #pragma nounroll
                for (int cls = 0; cls < 2 && !st; ++cls) {
                    const uint32_t slot = ((cls ? fi.ta : fi.td) >> (8 * c)) & 255, bit = 1u << (cls * 4 + slot);
                    if ((fi.defined | standard) & bit) continue;
                    if (slot >= 2) st = YSMR_MJPEGD_CORRUPT;
                    else standard |= bit;
                }
            }
            fi.ent_start = pos + length;
            fi.ent_end = len;
            fi.nseg = fi.ri ? (g.mcus + fi.ri - 1) / fi.ri : 1;
            break;
        }
        pos += length;
    }
    // what Motion-JPEG frames leave out: the typical tables of Annex K.3 (slots 0 and 1 of either class)
    #pragma nounroll
    for (int t = 0; t < 8 && !st; ++t) {
        if (!((standard >> t) & 1)) continue;
        const StdTable &s = c_std[(t >> 2) * 2 + (t & 3)];
        int count = 0;
        #pragma nounroll
        for (int l = 0; l < 16; ++l) { hf[t].bits[l] = s.bits[l]; count += s.bits[l]; }
        #pragma nounroll
        for (int k = 0; k < count; ++k) hf[t].vals[k] = s.vals[k];
        fi.defined |= 1u << t;
    }
    info[f] = fi;
    status[f] = st;
}

// Eight bytes at p, the first in bits 0 .. 7; bytes at or behind `end` read as 0 and are not touched.
__device__ __forceinline__ uint64_t load8(const uint8_t *p, const uint8_t *end)
{
    uint64_t w = 0;
    if (p + 8 <= end)
        __builtin_memcpy(&w, p, 8);
    else
        for (int k = 0; k < 8 && p + k < end; ++k) w |= (uint64_t)p[k] << (8 * k);
    return w;
}

// ---- restart markers -----------------------------------------------------------------------------------------------------------
// A marker is 0xFF followed by anything but 0x00 and 0xFF (a 0xFF before a 0xFF is a fill byte).  RSTn are numbered in file order
// by a scan over the workgroup; the first marker of another kind ends the entropy data, and what follows it is not looked at.
__global__ __launch_bounds__(256) void k_mjd_markers(const uint8_t *__restrict__ chunks, const long long *__restrict__ offsets, int max_seg,
                                                     FrameInfo *__restrict__ info, int32_t *__restrict__ seg_start, int *__restrict__ status)
{
    __shared__ int s_term, s_count, s_bad, s_wave[4];
    const int f = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (status[f] != 0) return;
    const uint8_t *base = chunks + offsets[f];
    const int start = info[f].ent_start, len = info[f].ent_end, nseg = info[f].nseg;
    int32_t *seg = seg_start + (size_t)f * max_seg;
    if (tid == 0) { s_term = len; s_count = 0; s_bad = 0; }
    __syncthreads();
    for (long long step0 = start; step0 < len; step0 += 256 * 16) {
        const long long p0 = step0 + tid * 16;
        uint32_t marks = 0;
        if (p0 < len) {
            // bytes p0 .. p0 + 16 (the last one is the next thread's first); those behind the frame's end read as 0: no marker
            const uint64_t w0 = load8(base + p0, base + len), w1 = load8(base + p0 + 8, base + len);
            uint32_t b = (uint32_t)(w0 & 255);
            for (int j = 0; j < 16; ++j) {
                const uint32_t nb = j < 7 ? (uint32_t)(w0 >> (8 * j + 8)) & 255 : j < 15 ? (uint32_t)(w1 >> (8 * j - 56)) & 255
                                                                                         : (p0 + 16 < len ? base[p0 + 16] : 0u);
                if (b == 0xFF && nb != 0x00 && nb != 0xFF) {
                    if ((nb & 0xF8) == 0xD0) marks |= 1u << j;
                    else atomicMin(&s_term, (int)(p0 + j));
                }
                b = nb;
            }
        }
        __syncthreads();
        const int term = s_term;
        for (int j = 0; j < 16; ++j)
            if (((marks >> j) & 1) && p0 + j >= term) marks &= ~(1u << j);
        int incl = __popc(marks);
        const int mine = incl;
        for (int d = 1; d < 64; d <<= 1) {
            const int o = __shfl_up(incl, d, 64);
            if (lane >= d) incl += o;
        }
        if (lane == 63) s_wave[wave] = incl;
        __syncthreads();
        int k = s_count + incl - mine;
        for (int w = 0; w < wave; ++w) k += s_wave[w];
        for (int j = 0; j < 16; ++j) {
            if (!((marks >> j) & 1)) continue;
            // the k-th RST marker: RST(k mod 8), and interval k + 1 starts behind it
            if (base[p0 + j + 1] != (uint32_t)(0xD0 + (k & 7))) s_bad = 1;
            if (k + 1 < nseg && k + 1 < max_seg) seg[k + 1] = (int32_t)(p0 + j + 2);
            ++k;
        }
        __syncthreads();
        if (tid == 0) s_count += s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
        __syncthreads();
        if (term < len) break;
    }
    if (tid == 0) {
        seg[0] = start;
        info[f].ent_end = s_term;
        if (s_count != nseg - 1 || s_bad) atomicOr(&status[f], YSMR_MJPEGD_CORRUPT);
    }
}

// ---- entropy decode ------------------------------------------------------------------------------------------------------------
// The tables of ONE frame in LDS: per table the last code of every length (-1: none) and where its symbols start, the symbols,
// and a look-up by the next 9 bits -> (length << 8) | symbol, 0 for longer codes (those walk the lengths 10 .. 16).
struct Tables {
    uint16_t lut[8][1 << LUT_BITS];
    int32_t maxcode[8][17];
    int32_t valoff[8][17];
    uint8_t vals[8][256];
    uint8_t zigzag[64];
};

struct BitReader {
    const uint8_t *q, *end;   // the next byte; the interval's end
    uint64_t acc;             // the next bits, from bit 63 down
    int nbits, fake;          // bits in acc; bytes of zeros fed behind the interval's end (they are the last ones fed)

    // A load per byte.  Fetching eight bytes at a time, one fetch ahead, was built and measured on the same box: 18.7 against
    // 17.6 ms per batch of 248 frames with a restart interval per MCU row, 350 against 345 ms without restart markers
    // (profiles/mjpeg_decode_e2e.log) -- the neighbouring bytes are in the cache already, and the extra state costs more.
    __device__ __forceinline__ void start(const uint8_t *p, const uint8_t *e)
    {
        q = p; end = e;
        acc = 0; nbits = 0; fake = 0;
    }
    __device__ __forceinline__ int next_byte()          // -1 behind the end
    {
        if (q >= end) return -1;
        return (int)*q++;
    }
    __device__ __forceinline__ void fill()
    {
        while (nbits <= 56) {
            int b = next_byte();
            if (b == 0xFF) {                              // 0x00 behind it (after any number of fill bytes) is stuffing ...
                int c;
                do c = next_byte(); while (c == 0xFF);
                if (c != 0x00) { q = end; b = -1; }       // ... anything else a marker: the interval is over
            }
            if (b < 0) { b = 0; ++fake; }
            acc |= (uint64_t)b << (56 - nbits);
            nbits += 8;
        }
    }
    __device__ __forceinline__ uint32_t take(int k)   // 1 <= k <= 16, after fill()
    {
        const uint32_t v = (uint32_t)(acc >> (64 - k));
        acc <<= k;
        nbits -= k;
        return v;
    }
    __device__ __forceinline__ bool overran() const { return nbits < 8 * fake; }
};

// the next symbol of table t, or -1 if no code of the table matches
__device__ __forceinline__ int next_symbol(BitReader &r, const Tables &tb, int t)
{
    r.fill();
    const uint32_t e = tb.lut[t][r.acc >> (64 - LUT_BITS)];
    if (e) {
        r.take((int)(e >> 8));
        return (int)(e & 255);
    }
    for (int l = LUT_BITS + 1; l <= 16; ++l) {
        const int code = (int)(r.acc >> (64 - l));
        if (code <= tb.maxcode[t][l]) {
            r.take(l);
            return tb.vals[t][(tb.valoff[t][l] + code) & 255];
        }
    }
    return -1;
}

__device__ __forceinline__ int extend(uint32_t v, int size) { return v < (1u << (size - 1)) ? (int)v - (1 << size) + 1 : (int)v; }

// (every thread of a workgroup of `threads` calls it; the tables are complete behind it)
__device__ __forceinline__ void build_tables(Tables &tb, const FrameInfo &fi, const HuffRaw *__restrict__ hf, int tid, int threads)
{
    if (tid < 8) {
        int code = 0, k = 0;
        tb.maxcode[tid][0] = -1; tb.valoff[tid][0] = 0;
        for (int l = 1; l <= 16; ++l) {
            const int b = ((fi.defined >> tid) & 1) ? hf[tid].bits[l - 1] : 0;
            tb.valoff[tid][l] = k - code;
            tb.maxcode[tid][l] = b ? code + b - 1 : -1;
            code = (code + b) << 1;
            k += b;
        }
    }
    for (int i = tid; i < 8 * 256; i += threads) tb.vals[i >> 8][i & 255] = ((fi.defined >> (i >> 8)) & 1) ? hf[i >> 8].vals[i & 255] : 0;
    if (tid < 64) tb.zigzag[tid] = c_zigzag[tid];
    __syncthreads();
    for (int i = tid; i < 8 << LUT_BITS; i += threads) {
        const int t = i >> LUT_BITS, idx = i & ((1 << LUT_BITS) - 1);
        uint32_t e = 0;
        for (int l = 1; l <= LUT_BITS; ++l) {
            const int code = idx >> (LUT_BITS - l);
            if (code <= tb.maxcode[t][l]) { e = ((uint32_t)l << 8) | tb.vals[t][(tb.valoff[t][l] + code) & 255]; break; }
        }
        tb.lut[t][idx] = (uint16_t)e;
    }
    __syncthreads();
}

__global__ __launch_bounds__(64) void k_mjd_entropy(const uint8_t *__restrict__ chunks, const long long *__restrict__ offsets, SmallGeo g,
                                                    const FrameInfo *__restrict__ info, const HuffRaw *__restrict__ huff,
                                                    const int32_t *__restrict__ seg_start, int16_t *__restrict__ coef, int *__restrict__ status)
{
    __shared__ Tables tb;
    const int f = blockIdx.y, tid = threadIdx.x;
    if (status[f] != 0) return;
    const FrameInfo fi = info[f];
    if ((int)blockIdx.x * 64 >= fi.nseg) return;
    const HuffRaw *hf = huff + (size_t)f * 8;
    build_tables(tb, fi, hf, tid, 64);

    const uint8_t *base = chunks + offsets[f];
    const int32_t *seg = seg_start + (size_t)f * g.mcus;
    int16_t *fcoef = coef + (size_t)f * g.blocks * 64;
    const int per = fi.ri ? fi.ri : g.mcus;
    const int luma = g.lh * g.lv, per_mcu = g.nc == 1 ? 1 : luma + 2;       // blocks of an MCU: the luminance's, Cb, Cr
    bool corrupt = false;
    for (int s = blockIdx.x * 64 + tid; s < fi.nseg && !corrupt; s += gridDim.x * 64) {
        BitReader r;
        r.start(base + seg[s], base + (s + 1 < fi.nseg ? seg[s + 1] - 2 : fi.ent_end));
        int pred0 = 0, pred1 = 0, pred2 = 0;
        const int m0 = s * per, m1 = (int)std::min<long long>((long long)m0 + per, g.mcus);
        int mrow = m0 / g.mx, mcol = m0 - mrow * g.mx, k = 0;                // the MCU, and the block inside it
        // ONE loop over the interval's blocks and one over a block's symbols (the DC difference is symbol 0): every level of
        // divergent control flow costs a pair of scalar registers
        for (int left = (m1 - m0) * per_mcu; left > 0 && !corrupt; --left) {
            const int c = k < luma ? 0 : k - luma + 1;
            const int sy = g.lh == 2 ? k >> 1 : k, sx = g.lh == 2 ? k & 1 : 0;
            const int block = c == 0 ? (mrow * g.lv + sy) * g.ycols + mcol * g.lh + sx : g.blocks_y + (c - 1) * g.blocks_c + mrow * g.ccols + mcol;
            const int tdc = (int)((fi.td >> (8 * c)) & 3), tac = 4 + (int)((fi.ta >> (8 * c)) & 3);
            int16_t *out = fcoef + (size_t)block * 64;
            int i = 0;
            while (i < 64) {
                const int sym = next_symbol(r, tb, i == 0 ? tdc : tac);
                if (sym < 0 || (i == 0 && sym > 11)) { corrupt = true; break; }
                const int size = sym & 15, run = i == 0 ? 0 : sym >> 4;
                if (i > 0 && size == 0) {
                    if (run != 15) break;
                    i += 16;
                    continue;
                }
                i += run;
                if (i > 63) { corrupt = true; break; }                       // (the index is checked before the store)
                int v = size ? extend(r.take(size), size) : 0;
                if (i == 0) {
                    v += c == 0 ? pred0 : c == 1 ? pred1 : pred2;
                    if (c == 0) pred0 = v; else if (c == 1) pred1 = v; else pred2 = v;
                }
                out[tb.zigzag[i]] = (int16_t)v;
                ++i;
            }
            if (++k == per_mcu) {
                k = 0;
                if (++mcol == g.mx) { mcol = 0; ++mrow; }
                if (r.fake > 8) left = 0;                                    // (far behind the end already: overran() holds)
            }
        }
        if (r.overran()) corrupt = true;
    }
    if (corrupt) atomicOr(&status[f], YSMR_MJPEGD_CORRUPT);
}

// ---- entropy decode of a frame WITHOUT restart markers (ysmr_mjpeg_decode_batch_sync) ------------------------------------------
// Huffman-coded data has no marks a decoder could start from, but a decoder started at a wrong bit falls into step with the
// code after a few symbols.  So the frame's data is cut into subsequences of SYNC_SUB_BYTES, a lane each, and
//   k_mjd_destuff  takes the stuffing out first: the reader's rules -- 0x00 behind a 0xFF (after any number of fill 0xFF) is no
//                  data, a marker ends it -- applied once, by a compaction; behind it a position is a plain bit number and a
//                  decoder can start at any of them
//   k_mjd_sync     a workgroup per frame, SYNC_PASS subsequences per pass: every lane decodes the symbols that START in its
//                  subsequence from an assumed state (its first bit, a DC symbol of block 0), storing nothing, and hands its
//                  exit state to its successor, which decodes again from that -- until no lane's entry state changed; then the
//                  blocks are counted by a scan and every lane decodes once more, from its TRUE state, and stores.  DC values
//                  are stored as differences
//   k_mjd_dc       the prefix sums of those differences per component, over the blocks in scan order
// tests/jpeg_sync_model.py is the same in Python, with the rounds of every pass.

// STATE of a decoder between two symbols: the bit position in the destuffed data and (k | i << 8 | error << 16): block k of the
// MCU, zigzag index i inside it; `error`: it met a code no table holds, a DC category above 11 or an index past 63 on the way --
// for an assumed state an exit like any other, which flags nothing and which the successor does not take over.
constexpr int SYNC_ERROR = 1 << 16;

// 32 bits at any bit position of data[0, bytes): bytes behind the end read as zeros.  The window holds eight bytes and is loaded
// anew when the position has left its first 32 bits.  The data lies in the workspace with eight bytes to spare behind it
// (SyncPlan::data_pitch), so that is ONE load and a mask that clears what lies behind the end -- whatever the workspace held
// there is not used.
struct BitWindow {
    const uint8_t *data;
    int bytes;
    uint64_t w;
    int first;                        // bit number of the window's first bit; far away: nothing loaded
    __device__ __forceinline__ void start(const uint8_t *d, int n) { data = d; bytes = n; w = 0; first = -(1 << 30); }
    __device__ __forceinline__ uint32_t peek(int pos)                       // 0 <= pos < 8 * bytes
    {
        uint32_t off = (uint32_t)(pos - first);
        if (off > 32u) {
            const int at = pos >> 3, valid = bytes - at;                     // valid >= 1
            uint64_t raw;
            __builtin_memcpy(&raw, data + at, 8);
            if (valid < 8) raw &= ~0ull >> (64 - 8 * valid);
            first = pos & ~7;
            w = __builtin_bswap64(raw);
            off = (uint32_t)(pos & 7);
        }
        return (uint32_t)((w << off) >> 32);
    }
};

struct SyncFrame {                    // what the symbol loop needs of the frame and the call, in registers
    uint32_t td, ta;
    int luma, per_mcu;
};

// The symbols that start before bit `stop`, from state (pos, ki) on; `done` counts the blocks completed.  `store` (the same in
// every lane): `block0` is the frame's number of blocks completed before, the coefficients go to fcoef (DC as the difference),
// and decoding ends with the frame's last block; the return value then tells whether the frame is damaged.  ONE copy of this
// loop serves the rounds and the write pass: two of them cost more scalar registers than there are.
__device__ __forceinline__ bool sync_decode(BitWindow &r, const Tables &tb, const SyncFrame &sf, int &pos, int &ki, int stop, int &done,
                                            const SmallGeo &g, bool store, int block0, int total_bits, int16_t *__restrict__ fcoef)
{
    int k = ki & 255, i = (ki >> 8) & 255;
    bool error = (ki & SYNC_ERROR) != 0, ended = store && block0 >= g.blocks;
    int16_t *out = nullptr;
    done = 0;
    while (pos < stop && !error && !ended) {
        const int c = k < sf.luma ? 0 : k - sf.luma + 1;
        if (store && (i == 0 || !out)) {
            // where the block lies (a lane may enter in the middle of one): MCU (mrow, mcol) of the scan, block k inside it
            const int mcu = (block0 + done) / sf.per_mcu, mrow = mcu / g.mx, mcol = mcu - mrow * g.mx;
            const int sy = g.lh == 2 ? k >> 1 : k, sx = g.lh == 2 ? k & 1 : 0;
            const int block = c == 0 ? (mrow * g.lv + sy) * g.ycols + mcol * g.lh + sx : g.blocks_y + (c - 1) * g.blocks_c + mrow * g.ccols + mcol;
            if ((unsigned)block >= (unsigned)g.blocks) { error = true; break; }      // (the block index is checked before the store)
            out = fcoef + (size_t)block * 64;
        }
        const int t = i == 0 ? (int)((sf.td >> (8 * c)) & 3) : 4 + (int)((sf.ta >> (8 * c)) & 3);
        const uint32_t w = r.peek(pos);
        uint32_t e = tb.lut[t][w >> (32 - LUT_BITS)];
        if (!e) {
            #pragma nounroll
            for (int l = LUT_BITS + 1; l <= 16; ++l) {
                const int code = (int)(w >> (32 - l));
                if (code <= tb.maxcode[t][l]) { e = ((uint32_t)l << 8) | tb.vals[t][(tb.valoff[t][l] + code) & 255]; break; }
            }
        }
        const int len = (int)(e >> 8), sym = (int)(e & 255);
        if (!e || (i == 0 && sym > 11)) { error = true; break; }
        const int size = sym & 15, run = i == 0 ? 0 : sym >> 4;
        bool complete;
        if (i > 0 && size == 0) {                                            // end of block, or sixteen zeros
            pos += len;
            i += 16;
            complete = run != 15 || i > 63;
        } else {
            i += run;
            if (i > 63) { error = true; break; }                             // (the index is checked before the store)
            if (store) out[tb.zigzag[i]] = (int16_t)(size ? extend((w << len) >> (32 - size), size) : 0);
            pos += len + size;
            complete = ++i == 64;
        }
        if (complete) {
            i = 0;
            if (++k == sf.per_mcu) k = 0;
            ++done;
            if (store && block0 + done == g.blocks) ended = true;            // what follows the last block is not looked at
        }
    }
    ki = k | (i << 8) | (error ? SYNC_ERROR : 0);
    // damaged: a symbol of the frame's blocks that no table holds, or bits of them beyond the data's end
    return store && block0 < g.blocks && (error || (ended && pos > total_bits));
}

// A WORKGROUP compacts one frame's entropy data, 16 bytes per thread and step (the loop of k_mjd_markers).  Inside [ent_start,
// ent_end) of a frame that k_mjd_markers passed there is no marker: a 0xFF is followed by 0x00, by another 0xFF or by the end.
// Of a run of 0xFF the first is data and the others fill bytes, the 0x00 behind it is stuffing; a run the data ends with is
// the beginning of the marker that ended it.  The frames of this call that HAVE a restart interval are k_mjd_entropy's, and
// those that have none are taken from it here: no restart interval of theirs is left (nseg = 0).
__global__ __launch_bounds__(256) void k_mjd_destuff(const uint8_t *__restrict__ chunks, const long long *__restrict__ offsets, int max_chunk,
                                                     FrameInfo *__restrict__ info, uint8_t *__restrict__ data, size_t pitch,
                                                     int32_t *__restrict__ data_bytes, int *__restrict__ status)
{
    __shared__ int s_go, s_count, s_wave[4];
    const int f = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) {
        int st = status[f];
        if (st == 0 && offsets[f + 1] - offsets[f] > (long long)max_chunk) status[f] = st = YSMR_MJPEGD_CORRUPT;
        s_go = st == 0 && info[f].ri == 0;
        if (s_go) info[f].nseg = 0;
        s_count = 0;
    }
    __syncthreads();
    if (!s_go) return;
    const uint8_t *base = chunks + offsets[f];
    const int start = info[f].ent_start, len = info[f].ent_end;
    uint8_t *out = data + (size_t)f * pitch;
    for (long long step0 = start; step0 < len; step0 += 256 * 16) {
        const long long p0 = step0 + tid * 16;
        uint32_t keep = 0;
        uint64_t w0 = 0, w1 = 0;
        if (p0 < len) {
            w0 = load8(base + p0, base + len); w1 = load8(base + p0 + 8, base + len);
            uint32_t prev = p0 > start ? base[p0 - 1] : 0u;
            for (int j = 0; j < 16 && p0 + j < len; ++j) {
                const uint32_t b = (uint32_t)((j < 8 ? w0 >> (8 * j) : w1 >> (8 * j - 64)) & 255);
                if (!(prev == 0xFF && (b == 0x00 || b == 0xFF))) keep |= 1u << j;
                prev = b;
            }
        }
        int incl = __popc(keep);
        const int mine = incl;
        for (int d = 1; d < 64; d <<= 1) {
            const int o = __shfl_up(incl, d, 64);
            if (lane >= d) incl += o;
        }
        if (lane == 63) s_wave[wave] = incl;
        __syncthreads();
        int k = s_count + incl - mine;
        for (int v = 0; v < wave; ++v) k += s_wave[v];
        for (int j = 0; j < 16; ++j)
            if ((keep >> j) & 1) {
                if ((size_t)k < pitch) out[k] = (uint8_t)((j < 8 ? w0 >> (8 * j) : w1 >> (8 * j - 64)) & 255);
                ++k;
            }
        __syncthreads();
        if (tid == 0) s_count += s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
        __syncthreads();
    }
    if (tid == 0) data_bytes[f] = s_count - (len > start && base[len - 1] == 0xFF ? 1 : 0);
}

__global__ __launch_bounds__(mjd::SYNC_PASS) void k_mjd_sync(SmallGeo g0, const FrameInfo *__restrict__ info, const HuffRaw *__restrict__ huff,
                                                             const uint8_t *__restrict__ data, size_t pitch,
                                                             const int32_t *__restrict__ data_bytes, int16_t *__restrict__ coef,
                                                             int *__restrict__ status)
{
    constexpr int PASS = mjd::SYNC_PASS, SUB_BITS = 8 * mjd::SYNC_SUB_BYTES, WAVES = PASS / 64;
    __shared__ Tables tb;
    __shared__ int s_pos[PASS], s_ki[PASS], s_wave[WAVES];
    __shared__ SmallGeo s_geo;        // the geometry is read from here: once per block, and scalar registers are the scarce ones
    const int f = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    if (status[f] != 0) return;
    const FrameInfo fi = info[f];
    if (fi.ri != 0) return;
    if (tid == 0) s_geo = g0;
    build_tables(tb, fi, huff + (size_t)f * 8, tid, PASS);
    const SmallGeo &g = s_geo;

    // (what is the same in every lane is told to be: loops whose conditions are scalar cost no saved execution masks)
    const int bytes = __builtin_amdgcn_readfirstlane(data_bytes[f]), total_bits = 8 * bytes;
    const int blocks = __builtin_amdgcn_readfirstlane(g.blocks);
    const int nsub = (bytes + mjd::SYNC_SUB_BYTES - 1) / mjd::SYNC_SUB_BYTES;
    int16_t *fcoef = coef + (size_t)f * g.blocks * 64;
    SyncFrame sf;
    sf.td = fi.td; sf.ta = fi.ta;
    sf.luma = g.lh * g.lv; sf.per_mcu = g.nc == 1 ? 1 : sf.luma + 2;
    BitWindow r;
    r.start(data + (size_t)f * pitch, bytes);
    int true_pos = 0, true_ki = 0, blocks_done = 0;                         // the state behind the passes so far (the same in every lane)
    bool corrupt = false;
    for (int s0 = 0; s0 < nsub && blocks_done < blocks && !(true_ki & SYNC_ERROR); s0 += PASS) {
        const int s = s0 + tid;
        const bool active = s < nsub;
        const int stop = (int)std::min<long long>((long long)(s + 1) * SUB_BITS, total_bits);
        // lane 0 starts from the TRUE state, every other lane at its first bit, expecting the DC symbol of block 0
        const int first_bit = active ? s * SUB_BITS : 0;
        int in_pos = tid == 0 ? true_pos : first_bit, in_ki = tid == 0 ? true_ki : 0;
        int was_pos = -1, was_ki = -1, done = 0, before = 0, all = 0;
        // After round r the first r lanes hold true states and decode no more, so there are PASS rounds at most; the rounds
        // end when NO lane's entry state changed, and then every entry state is the true one: the blocks completed before
        // each lane are counted, and the loop's last turn is the write pass.
        for (bool store = false;;) {
            const bool go = active && (store || in_pos != was_pos || in_ki != was_ki);
            if (go) {
                int pos = in_pos, ki = in_ki, n;
                const bool damaged = sync_decode(r, tb, sf, pos, ki, stop, n, g, store, before, total_bits, fcoef);
                if (store) {
                    corrupt = corrupt || damaged;
                } else {
                    s_pos[tid] = pos; s_ki[tid] = ki; done = n;
                    was_pos = in_pos; was_ki = in_ki;
                }
            }
            if (store) break;
            if (__builtin_amdgcn_readfirstlane(__syncthreads_or(go))) {
                if (active && tid > 0) {
                    in_pos = s_pos[tid - 1]; in_ki = s_ki[tid - 1];
                    // a predecessor that met an error has nothing to hand on: this lane keeps to its assumed state (the error
                    // of one wrong guess must not silence every lane behind it until the true state arrives)
                    if (in_ki & SYNC_ERROR) { in_pos = first_bit; in_ki = 0; }
                }
                __syncthreads();
                continue;
            }
            // blocks completed before this lane's subsequence: an exclusive scan.  (The lanes are chosen by arithmetic, x >> 31 =
            // -1 for x < 0: comparisons that do not change from round to round are kept in scalar register pairs, ten of them)
            int incl = done;
            for (int d = 1; d < 64; d <<= 1) incl += __builtin_amdgcn_ds_bpermute((lane - d) << 2, incl) & ((d - 1 - lane) >> 31);
            if (lane == 63) s_wave[wave] = incl;
            __syncthreads();
            before = blocks_done + incl - done;
            #pragma nounroll
            for (int v = 0; v < WAVES; ++v) {
                if (v < wave) before += s_wave[v];                           // (`wave` is a scalar)
                all += s_wave[v];
            }
            all = __builtin_amdgcn_readfirstlane(all);
            store = true;
        }
        const int last = std::min(PASS, nsub - s0) - 1;
        true_pos = __builtin_amdgcn_readfirstlane(s_pos[last]); true_ki = __builtin_amdgcn_readfirstlane(s_ki[last]);
        blocks_done += all;
        // (a barrier in any case: s_pos, s_ki and s_wave are written again; behind a damaged pass nothing is worth decoding)
        if (__builtin_amdgcn_readfirstlane(__syncthreads_or(corrupt))) break;
    }
    // the data ended before the frame's last block (a decoder that read on would read the zeros behind it)
    if (blocks_done < blocks) corrupt = true;
    if (corrupt) atomicOr(&status[f], YSMR_MJPEGD_CORRUPT);
}

// DC: the prefix sums of the differences, per component over its blocks in SCAN order (the luminance blocks of an MCU follow
// each other in the scan, not in the plane), 32 bits wide and stored as the serial decoder's (int16_t) v -- truncation commutes
// with the sum.  A thread sums a run of consecutive blocks, the runs are scanned, the thread walks its run again.
__global__ __launch_bounds__(256) void k_mjd_dc(SmallGeo g, const FrameInfo *__restrict__ info, const int *__restrict__ status,
                                                int16_t *__restrict__ coef)
{
    __shared__ int s_wave[4];
    const int f = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (status[f] != 0 || info[f].ri != 0) return;
    int16_t *fcoef = coef + (size_t)f * g.blocks * 64;
    const int luma = g.lh * g.lv;
    for (int c = 0; c < g.nc; ++c) {
        const int count = c == 0 ? g.blocks_y : g.blocks_c, per = (count + 255) / 256;
        const int j0 = std::min(count, tid * per), j1 = std::min(count, j0 + per);
        auto block_of = [&](int j) {
            if (c > 0) return g.blocks_y + (c - 1) * g.blocks_c + j;
            const int mcu = j / luma, k = j - mcu * luma, mrow = mcu / g.mx, mcol = mcu - mrow * g.mx;
            const int sy = g.lh == 2 ? k >> 1 : k, sx = g.lh == 2 ? k & 1 : 0;
            return (mrow * g.lv + sy) * g.ycols + mcol * g.lh + sx;
        };
        uint32_t sum = 0;                                                    // (unsigned: the sums wrap by definition)
        for (int j = j0; j < j1; ++j) sum += (uint32_t)(int)fcoef[(size_t)block_of(j) * 64];
        uint32_t incl = sum;
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t o = (uint32_t)__shfl_up((int)incl, d, 64);
            if (lane >= d) incl += o;
        }
        if (lane == 63) s_wave[wave] = (int)incl;
        __syncthreads();
        uint32_t v = incl - sum;
        for (int u = 0; u < wave; ++u) v += (uint32_t)s_wave[u];
        for (int j = j0; j < j1; ++j) {
            int16_t *dc = fcoef + (size_t)block_of(j) * 64;
            v += (uint32_t)(int)*dc;
            *dc = (int16_t)v;
        }
        __syncthreads();
    }
}

// ---- dequantise + IDCT ---------------------------------------------------------------------------------------------------------
// One direction of the accurate integer IDCT: 13-bit constants, 32-bit sums, rounded and shifted.  Widths as in the model: the
// dequantised coefficient is the low 16 bits of the product, the first pass saturates to 16 bits, the sample to -128 .. 127.
__device__ __forceinline__ void idct_pass(const int (&d)[8], int (&o)[8], int shift)
{
    const uint32_t half = 1u << (shift - 1);
    // (unsigned arithmetic: the sums wrap at 32 bits by definition)
    const uint32_t i0 = d[0], i1 = d[1], i2 = d[2], i3 = d[3], i4 = d[4], i5 = d[5], i6 = d[6], i7 = d[7];
    uint32_t z1 = (i2 + i6) * 4433u;
    const uint32_t e2 = z1 - i6 * 15137u, e3 = z1 + i2 * 6270u;
    const uint32_t e0 = (i0 + i4) << 13, e1 = (i0 - i4) << 13;
    const uint32_t t10 = e0 + e3, t13 = e0 - e3, t11 = e1 + e2, t12 = e1 - e2;
    uint32_t t0 = i7, t1 = i5, t2 = i3, t3 = i1;
    z1 = t0 + t3;
    uint32_t z2 = t1 + t2, z3 = t0 + t2, z4 = t1 + t3;
    const uint32_t z5 = (z3 + z4) * 9633u;
    t0 *= 2446u; t1 *= 16819u; t2 *= 25172u; t3 *= 12299u;
    z1 *= (uint32_t)-7373; z2 *= (uint32_t)-20995;
    z3 = z3 * (uint32_t)-16069 + z5; z4 = z4 * (uint32_t)-3196 + z5;
    t0 += z1 + z3; t1 += z2 + z4; t2 += z2 + z3; t3 += z1 + z4;
    o[0] = (int)(t10 + t3 + half) >> shift; o[7] = (int)(t10 - t3 + half) >> shift;
    o[1] = (int)(t11 + t2 + half) >> shift; o[6] = (int)(t11 - t2 + half) >> shift;
    o[2] = (int)(t12 + t1 + half) >> shift; o[5] = (int)(t12 - t1 + half) >> shift;
    o[3] = (int)(t13 + t0 + half) >> shift; o[4] = (int)(t13 - t0 + half) >> shift;
}

constexpr int IDCT_ROW = 65;   // words of LDS per block (64 + 1: the eight blocks of a wave's half start on different banks)

// EIGHT THREADS take a block: thread j column j, then row j.  Colour: the samples go to the frame's planes in the workspace
// (whole blocks, 8 bytes per thread); one component: straight into the frame, the part of the block that lies inside it.
__global__ __launch_bounds__(256) void k_mjd_idct(const int16_t *__restrict__ coef, const uint16_t *__restrict__ quant,
                                                  const FrameInfo *__restrict__ info, const int *__restrict__ status, int n, Geo g,
                                                  uint8_t *__restrict__ planes, uint8_t *__restrict__ frames)
{
    __shared__ int ws[32 * IDCT_ROW];
    const int tid = threadIdx.x, slot = tid >> 3, j = tid & 7;
    const long long total = (long long)n * g.blocks;
    for (long long b0 = (long long)blockIdx.x * 32; b0 < total; b0 += (long long)gridDim.x * 32) {
        const long long blk = b0 + slot;
        const int f = (int)(blk / g.blocks), r = (int)(blk - (long long)f * g.blocks);
        const bool live = blk < total && status[f] == 0;
        int c = 0, rb = r;
        if (r >= g.blocks_y) { c = 1 + (r - g.blocks_y) / g.blocks_c; rb = r - g.blocks_y - (c - 1) * g.blocks_c; }
        if (live) {
            const uint16_t *q = quant + (size_t)f * 256 + ((info[f].tq >> (8 * c)) & 3) * 64;
            const int16_t *in = coef + (size_t)blk * 64;
            int d[8], o[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) d[k] = (int16_t)((int)in[8 * k + j] * (int)q[8 * k + j]);
            idct_pass(d, o, 11);
#pragma unroll
            for (int k = 0; k < 8; ++k) ws[slot * IDCT_ROW + 8 * k + j] = std::min(32767, std::max(-32768, o[k]));
        }
        __syncthreads();
        if (live) {
            int d[8], o[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) d[k] = ws[slot * IDCT_ROW + 8 * j + k];
            idct_pass(d, o, 18);
            uint32_t lo = 0, hi = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                lo |= (uint32_t)(std::min(127, std::max(-128, o[k])) + 128) << (8 * k);
                hi |= (uint32_t)(std::min(127, std::max(-128, o[k + 4])) + 128) << (8 * k);
            }
            const int cols = c == 0 ? g.ycols : g.ccols;
            const int by = rb / cols, bx = rb - by * cols;
            if (g.nc == 3) {
                uint8_t *plane = planes + (size_t)f * g.planes + (c == 0 ? 0 : g.plane_y + (size_t)(c - 1) * g.plane_c);
                const int pitch = c == 0 ? g.ypitch : g.cpitch;
                *(uint2 *)(plane + (size_t)(8 * by + j) * pitch + 8 * bx) = make_uint2(lo, hi);
            } else {
                const int y = 8 * by + j;
                if (y < g.H) {
                    uint8_t *row = frames + ((size_t)f * g.H + y) * g.W;
#pragma unroll
                    for (int k = 0; k < 8; ++k)
                        if (8 * bx + k < g.W) row[8 * bx + k] = (uint8_t)((k < 4 ? lo >> (8 * k) : hi >> (8 * (k - 4))) & 255);
                }
            }
        }
        __syncthreads();
    }
}

// ---- upsampling + colour -------------------------------------------------------------------------------------------------------
// The "fancy" triangle filters.  A chrominance plane holds whole blocks; the component is its first cw = ceil(W / 2) columns (and
// ch = ceil(H / 2) rows), and those numbers set the filters' ends: the first output sample and the last of 2 cw are one-sided
// (2 x 1: copies), the row above the first and below the last row of the component is that row itself.
__device__ __forceinline__ int chroma_at(const uint8_t *__restrict__ p, int pitch, int x, int y, int W, int H, int sampling)
{
    if (sampling == 1) return p[(size_t)y * pitch + x];
    const int cw = (W + 1) >> 1, j = x >> 1, odd = x & 1;
    const bool end = x == 0 || (x == 2 * cw - 1 && cw > 1);
    const int other = end ? j : odd ? j + 1 : j - 1;
    if (sampling == 2) {
        const uint8_t *row = p + (size_t)y * pitch;
        return end ? row[j] : (3 * row[j] + row[other] + (odd ? 2 : 1)) >> 2;
    }
    const int ch = (H + 1) >> 1, i = y >> 1;
    const int near = std::min(ch - 1, std::max(0, (y & 1) ? i + 1 : i - 1));
    const uint8_t *r0 = p + (size_t)i * pitch, *r1 = p + (size_t)near * pitch;
    const int s = 3 * r0[j] + r1[j], t = 3 * r0[other] + r1[other];
    return end ? (4 * s + (odd ? 7 : 8)) >> 4 : (3 * s + t + (odd ? 7 : 8)) >> 4;
}

__global__ __launch_bounds__(256) void k_mjd_colour(const uint8_t *__restrict__ planes, const int *__restrict__ status, int n, Geo g,
                                                    uint8_t *__restrict__ frames)
{
    const long long per = (long long)g.H * g.W, total = per * n;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int f = (int)(i / per);
        if (status[f] != 0) continue;
        const long long at = i - (long long)f * per;
        const int y = (int)(at / g.W), x = (int)(at - (long long)y * g.W);
        const uint8_t *py = planes + (size_t)f * g.planes, *pb = py + g.plane_y, *pr = pb + g.plane_c;
        const int Y = py[(size_t)y * g.ypitch + x];
        const int cb = chroma_at(pb, g.cpitch, x, y, g.W, g.H, g.sampling) - 128;
        const int cr = chroma_at(pr, g.cpitch, x, y, g.W, g.H, g.sampling) - 128;
        const int R = Y + ((91881 * cr + 32768) >> 16);
        const int G = Y + ((-22554 * cb - 46802 * cr + 32768) >> 16);
        const int B = Y + ((116130 * cb + 32768) >> 16);
        uint8_t *out = frames + (size_t)i * 3;
        out[0] = (uint8_t)std::min(255, std::max(0, B));
        out[1] = (uint8_t)std::min(255, std::max(0, G));
        out[2] = (uint8_t)std::min(255, std::max(0, R));
    }
}

unsigned grid_of(long long items, int per_block)
{
    return (unsigned)std::max<long long>(1, std::min<long long>((items + per_block - 1) / per_block, MAX_GRID));
}

}  // namespace

extern "C" size_t ysmr_mjpeg_decode_workspace_bytes(int n_frames, int height, int width, int channels, int sampling)
{
    Geo g;
    if (!geometry_of(n_frames, height, width, channels, sampling, g)) return 0;
    return plan_of(n_frames, g).total;
}

extern "C" int ysmr_mjpeg_decode_batch(void *stream, const uint8_t *chunks_dev, const int64_t *offsets_dev, int n_frames, int height,
                                       int width, int channels, int sampling, void *workspace_dev, size_t workspace_bytes,
                                       uint8_t *frames_dev, int32_t *status_dev)
{
    Geo g;
    if (!geometry_of(n_frames, height, width, channels, sampling, g))
        return ysmr::fail(YSMR_ERR_ARG, "n_frames must be positive, height and width 1 .. 65535, sampling 0 .. 3 with 1 channel for 0 and 3 "
                          "otherwise (got %d, %d, %d, sampling %d, %d channels)", n_frames, height, width, sampling, channels);
    if (!chunks_dev || !offsets_dev || !workspace_dev || !frames_dev || !status_dev)
        return ysmr::fail(YSMR_ERR_ARG, "chunks_dev, offsets_dev, workspace_dev, frames_dev and status_dev must not be NULL");
    const Plan p = plan_of(n_frames, g);
    if (workspace_bytes < p.total)
        return ysmr::fail(YSMR_ERR_ARG, "workspace of %zu bytes, %zu needed (ysmr_mjpeg_decode_workspace_bytes)", workspace_bytes, p.total);
    if (((uintptr_t)workspace_dev & 255) || ((uintptr_t)offsets_dev & 7) || ((uintptr_t)status_dev & 3))
        return ysmr::fail(YSMR_ERR_ARG, "workspace_dev must be 256-byte aligned, offsets_dev 8-byte, status_dev 4-byte");

    hipStream_t st = (hipStream_t)stream;
    uint8_t *ws = (uint8_t *)workspace_dev;
    FrameInfo *info = (FrameInfo *)(ws + p.info);
    uint16_t *quant = (uint16_t *)(ws + p.quant);
    HuffRaw *huff = (HuffRaw *)(ws + p.huff);
    int32_t *seg_start = (int32_t *)(ws + p.seg_start);
    int16_t *coef = (int16_t *)(ws + p.coef);
    uint8_t *planes = ws + p.planes;
    const long long *offsets = (const long long *)offsets_dev;
    const SmallGeo sg = {g.H, g.W, g.nc, g.lh, g.lv, g.mx, g.mcus, g.ycols, g.ccols, g.blocks_y, g.blocks_c, g.blocks};
    hipLaunchKernelGGL(k_mjd_headers, dim3((n_frames + 63) / 64), dim3(64), 0, st, chunks_dev, offsets, n_frames, sg, info, quant, huff,
                       (int *)status_dev);
    YSMR_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_mjd_markers, dim3(n_frames), dim3(256), 0, st, chunks_dev, offsets, g.mcus, info, seg_start, (int *)status_dev);
    YSMR_LAUNCH_CHECK();
    YSMR_HIP_CHECK(hipMemsetAsync(coef, 0, (size_t)n_frames * g.blocks * 64 * sizeof(int16_t), st));
    const unsigned ex = (unsigned)std::min(ENTROPY_GRID_X, (g.mcus + 63) / 64);
    hipLaunchKernelGGL(k_mjd_entropy, dim3(ex, n_frames), dim3(64), 0, st, chunks_dev, offsets, sg, info, huff, seg_start, coef,
                       (int *)status_dev);
    YSMR_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_mjd_idct, dim3(grid_of((long long)n_frames * g.blocks, 32)), dim3(256), 0, st, coef, quant, info,
                       (const int *)status_dev, n_frames, g, planes, frames_dev);
    YSMR_LAUNCH_CHECK();
    if (g.nc == 3) {
        hipLaunchKernelGGL(k_mjd_colour, dim3(grid_of((long long)n_frames * height * width, 256)), dim3(256), 0, st, planes,
                           (const int *)status_dev, n_frames, g, frames_dev);
        YSMR_LAUNCH_CHECK();
    }
    return YSMR_OK;
}

extern "C" void ysmr_mjpeg_decode_sync_geometry(int *subsequence_bytes, int *subsequences_per_pass)
{
    if (subsequence_bytes) *subsequence_bytes = mjd::SYNC_SUB_BYTES;
    if (subsequences_per_pass) *subsequences_per_pass = mjd::SYNC_PASS;
}

extern "C" size_t ysmr_mjpeg_decode_sync_workspace_bytes(int n_frames, int height, int width, int channels, int sampling, int max_chunk_bytes)
{
    Geo g;
    mjd::SyncPlan p;
    if (!mjd::sync_plan_of(n_frames, height, width, channels, sampling, max_chunk_bytes, g, p)) return 0;
    return p.total;
}

extern "C" int ysmr_mjpeg_decode_batch_sync(void *stream, const uint8_t *chunks_dev, const int64_t *offsets_dev, int n_frames, int height,
                                            int width, int channels, int sampling, int max_chunk_bytes, void *workspace_dev,
                                            size_t workspace_bytes, uint8_t *frames_dev, int32_t *status_dev)
{
    Geo g;
    mjd::SyncPlan sp;
    if (!mjd::sync_plan_of(n_frames, height, width, channels, sampling, max_chunk_bytes, g, sp))
        return ysmr::fail(YSMR_ERR_ARG, "n_frames must be positive, height and width 1 .. 65535, sampling 0 .. 3 with 1 channel for 0 and 3 "
                          "otherwise, max_chunk_bytes 1 .. %d (got %d, %d, %d, sampling %d, %d channels, max_chunk_bytes %d), and the "
                          "workspace's size must fit a size_t", mjd::SYNC_MAX_CHUNK, n_frames, height, width, sampling, channels, max_chunk_bytes);
    if (!chunks_dev || !offsets_dev || !workspace_dev || !frames_dev || !status_dev)
        return ysmr::fail(YSMR_ERR_ARG, "chunks_dev, offsets_dev, workspace_dev, frames_dev and status_dev must not be NULL");
    if (workspace_bytes < sp.total)
        return ysmr::fail(YSMR_ERR_ARG, "workspace of %zu bytes, %zu needed (ysmr_mjpeg_decode_sync_workspace_bytes)", workspace_bytes, sp.total);
    if (((uintptr_t)workspace_dev & 255) || ((uintptr_t)offsets_dev & 7) || ((uintptr_t)status_dev & 3))
        return ysmr::fail(YSMR_ERR_ARG, "workspace_dev must be 256-byte aligned, offsets_dev 8-byte, status_dev 4-byte");

    hipStream_t st = (hipStream_t)stream;
    const Plan &p = sp.base;
    uint8_t *ws = (uint8_t *)workspace_dev;
    FrameInfo *info = (FrameInfo *)(ws + p.info);
    uint16_t *quant = (uint16_t *)(ws + p.quant);
    HuffRaw *huff = (HuffRaw *)(ws + p.huff);
    int32_t *seg_start = (int32_t *)(ws + p.seg_start);
    int16_t *coef = (int16_t *)(ws + p.coef);
    uint8_t *planes = ws + p.planes, *data = ws + sp.data;
    int32_t *data_bytes = (int32_t *)(ws + sp.data_bytes);
    const long long *offsets = (const long long *)offsets_dev;
    const SmallGeo sg = {g.H, g.W, g.nc, g.lh, g.lv, g.mx, g.mcus, g.ycols, g.ccols, g.blocks_y, g.blocks_c, g.blocks};
    hipLaunchKernelGGL(k_mjd_headers, dim3((n_frames + 63) / 64), dim3(64), 0, st, chunks_dev, offsets, n_frames, sg, info, quant, huff,
                       (int *)status_dev);
    YSMR_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_mjd_markers, dim3(n_frames), dim3(256), 0, st, chunks_dev, offsets, g.mcus, info, seg_start, (int *)status_dev);
    YSMR_LAUNCH_CHECK();
    YSMR_HIP_CHECK(hipMemsetAsync(coef, 0, (size_t)n_frames * g.blocks * 64 * sizeof(int16_t), st));
    // the frames part here: those without a restart interval leave k_mjd_entropy none to decode (k_mjd_destuff) and are
    // k_mjd_sync's and k_mjd_dc's, which pass over the others
    hipLaunchKernelGGL(k_mjd_destuff, dim3(n_frames), dim3(256), 0, st, chunks_dev, offsets, max_chunk_bytes, info, data, sp.data_pitch,
                       data_bytes, (int *)status_dev);
    YSMR_LAUNCH_CHECK();
    const unsigned ex = (unsigned)std::min(ENTROPY_GRID_X, (g.mcus + 63) / 64);
    hipLaunchKernelGGL(k_mjd_entropy, dim3(ex, n_frames), dim3(64), 0, st, chunks_dev, offsets, sg, info, huff, seg_start, coef,
                       (int *)status_dev);
    YSMR_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_mjd_sync, dim3(n_frames), dim3(mjd::SYNC_PASS), 0, st, sg, info, huff, data, sp.data_pitch, data_bytes, coef,
                       (int *)status_dev);
    YSMR_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_mjd_dc, dim3(n_frames), dim3(256), 0, st, sg, info, (const int *)status_dev, coef);
    YSMR_LAUNCH_CHECK();
    hipLaunchKernelGGL(k_mjd_idct, dim3(grid_of((long long)n_frames * g.blocks, 32)), dim3(256), 0, st, coef, quant, info,
                       (const int *)status_dev, n_frames, g, planes, frames_dev);
    YSMR_LAUNCH_CHECK();
    if (g.nc == 3) {
        hipLaunchKernelGGL(k_mjd_colour, dim3(grid_of((long long)n_frames * height * width, 256)), dim3(256), 0, st, planes,
                           (const int *)status_dev, n_frames, g, frames_dev);
        YSMR_LAUNCH_CHECK();
    }
    return YSMR_OK;
}

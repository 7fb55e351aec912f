// k_threshold_mfma: a1-a3 (gray input) as "decide on the matrix pipe, refine exactly".
//
// What the reference computes per pixel (track_eval.py:182-208):
//   b   = GaussianBlur 3x3 of the gray frame (exact integers, REFLECT_101)
//   acc = 11x11 Gaussian (sigma 2) of b in float32, cv2's evaluation order (row pass = ascending FMA chain,
//         column pass = symmetric form), REPLICATE border
//   m   = round-half-even(acc);  thresh = (b - m > t_low), markers = (b - m > t_high)   [INV: <=]
// The two class bits only depend on where acc lies relative to b - t - 0.5.  This kernel evaluates
//   v = mean - b   with |v - (acc - b)| < EPS   (a bound worked out on the host: detect_plan.h, choose_scales / walk_bound)
// on the matrix pipe and decides every pixel whose v is farther than EPS from both levels; the others (a few dozen per frame)
// are listed and recomputed with cv2's exact float32 chain at the end of the workgroup, from the frame in global memory.
// Results are bit for bit those of k_threshold / k_threshold_strip (detect.hip), which remain the path for BGR input and odd
// geometries.
//
// Why the matrix pipe: the float32-chain kernel is bound by vector-instruction issue (~34 instructions per pixel), and
// so was a first version of this kernel that still did the 3x3 blur with SWAR integer arithmetic.  Here every multiply-add
// is an MFMA (5.2 per 16 x 16 tile since round 5; 8.8 in round 4, when every tap and the intermediate were f16 hi + lo pairs):
//   blur, row direction     v_mfma_i32_16x16x64_i8: the gray BYTES as they lie in LDS (XOR 0x80 makes them signed) times
//                           a banded (1, 2, 1) matrix; the accumulator starts at 0x6400 + 512, so a result IS the f16
//                           bit pattern of 1024 + sum -- two results pack into an f16 pair with one v_lshl_or
//   blur, column direction  v_mfma_f32_16x16x32_f16 over the previous and this 16-row block of those sums (kept in
//                           registers: the accumulator layout is the next product's B operand); exact integers;
//                           (sum + 8) >> 4 is folded into the taps and a round-toward-zero conversion at 1024 + x;
//                           the tile then holds b - 128: centred, so that the Gaussian's f16 taps meet |b - 128| <= 128
//   Gaussian, columns       the blurred tile lives in LDS as [column][row] f16, so the operand is a 16-byte read;
//                           ONE f16 per tap (the taps scaled by a host-chosen s near 1 at which all eleven lie close to f16
//                           values); the result ONE f16, rounded to nearest (v_cvt_pk_f16_f32)
//   Gaussian, rows          1 MFMA per 16x16 output tile over two neighbouring blocks, transposed (a lane ends up with four
//                           consecutive columns of one row: a dword of class bytes); the taps carry the classification's
//                           scale X, the accumulator starts at -X theta_1 - X (b - 128) (one more product: tile x scaled
//                           shifted identity), so the result is x = X (mean - b - theta_1)
//   classification          v_cvt_pk_bf8_f32 of x: the byte's sign bit IS the class bit and its exponent's top bit says
//                           |x| >= 2, i.e. decided; the second level only in tiles where the first fires somewhere
// which leaves about 45 vector instructions per 256 pixels (round 4: 62): the blur's XOR / pack / conversions, two conversions
// of the intermediate, the classification, addresses and control.
//
// Memory skeleton (scripts/ubench/skeleton.hip): a 1024-thread workgroup owns a band of rows of one frame over a
// column panel (the whole width up to 1232 columns) and walks down in steps of 16 rows: whole rows come in by
// LDS-DMA (global_load_lds_dwordx4, no registers), the class map leaves as 16-byte stores.  Per step:
//   stores class bytes of step s-1 (they waited in the wave's staging rows)
//   DMA    gray rows of step s+2                                       -> s_raw[s & 1]   (half of the waves: between two tiles)
//   filter output rows of step s-1 from the tile blocks of steps s-1 and s -> class bytes -> wave-private staging
//   barrier
//   blur   step s+1: s_raw[(s+1) & 1] -> tile block (s+1) & 1
//   barrier
// The tile (blurred pixels - 128 as f16, a ring of two 16-row blocks) lies in LDS as four planes, one per octet of its 32 rows:
// TM_PLANES below.
//
// Error bound: the comment at walk_bound() (detect_plan.h): 0.0423 gray levels for cv2's sigma-2 taps with any image,
// of which 0.031 is the f16 rounding of the intermediate (half an ulp at |v1| < 128); EPS = 1.875 / 39.375 = 0.0476.
// MEASURED: tests/test_gpu_detect.py (48 cases, every geometry class, noise and synthetic video, the bench's and the 4K launch
// shapes) byte for byte against the oracle; scripts/sim/thr_single_f16.py models the same arithmetic in numpy: worst
// |model - real| 0.037 on the bench clip, ~35 undecided pixels per 1.13-Mpx frame (4 at round 4's EPS = 1/256).
#include "common.h"
#include "thr_mfma.h"
#include <cstring>
#include <mutex>
#include <type_traits>

namespace {

typedef _Float16 half8_t __attribute__((ext_vector_type(8)));
typedef _Float16 half2_t __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

#ifndef TM_MEM_WAVE_N
#define TM_MEM_WAVE_N 0
#endif
// Round 5, an experiment switch (-DTM_MEM_WAVE_N=1; parity-tested, NOT the default: it measures the same 230 us per 256 frames
// as the default within 2 %, profiles/r05_ab_thr_memory_wave.log).  ONE wave of the sixteen, at priority 3 and with no tiles
// of its own, issues every global memory instruction of the walk -- a step's gray rows as 32 LDS-DMA requests addressed on the
// scalar unit, a step's class rows as 24 stores out of sixteen dense staging rows, the two chunks that straddle a row's ends
// dword by dword through a side buffer -- and the other fifteen issue none.  Built because with every wave issuing its share the
// 53 one-KB instructions of a step cost each wave 700 - 1 500 cycles of a 7 665-cycle step; what it showed is that those cycles were
// not the limit: with the memory wave off the critical path of both phases (stamps: it waits at both barriers) the fifteen
// others' filter and blur phases stretch to fill the step.
constexpr bool TM_MEM_WAVE = TM_MEM_WAVE_N != 0;
#ifndef TM_WAVES_N
#define TM_WAVES_N 16
#endif
constexpr int TM_WAVES = TM_WAVES_N, TM_THREADS = 64 * TM_WAVES;
constexpr int TM_ROWS = 16;                                  // rows per step (one MFMA tile row block)
using detect_plan::TM_MAX_PANEL;                             // columns per panel, a multiple of 16 (detect_plan.h)
constexpr int TM_MAX_TILES = TM_MAX_PANEL / 16;              // output tiles t: columns 16t .. 16t + 15 of the panel
constexpr int TM_MAX_BLOCKS = TM_MAX_TILES + 1;              // tile column blocks u: columns 16u - 8 .. 16u + 7
// blocks (and tiles) per wave: 5 -- with the memory wave, which has none: fifteen waves of five and one more for the three that share
// the memory wave's SIMD (waves 3, 7, 11: 18 blocks beside the memory wave, 20 on the other SIMDs)
constexpr int TM_PER_WAVE = (TM_MAX_BLOCKS + TM_WAVES - 1) / TM_WAVES + (TM_MEM_WAVE ? 1 : 0);
static_assert(!TM_MEM_WAVE || (TM_WAVES == 16 && 5 * 15 + 3 >= TM_MAX_BLOCKS), "the memory wave's split of the blocks");
constexpr int TM_POS = 16 * TM_MAX_BLOCKS;                   // tile positions: p = column - x0 + 8
#ifndef TM_COL_PITCH_N
#define TM_COL_PITCH_N 40
#endif
constexpr int TM_COL_PITCH = TM_COL_PITCH_N;                             // f16 per tile column: 32 rows + 8 (80 bytes: 16 columns hit 16 x 4 banks)
#ifndef TM_PLANES_N
#define TM_PLANES_N 1
#endif
// Round 5 (end): the tile as four PLANES, one per octet of its 32 rows -- plane o holds rows 8 o .. 8 o + 7 of EVERY column position,
// 16 bytes apiece, one position behind the other (a plane is 1248 x 16 = 19 968 bytes, a multiple of 256).  A lane's MFMA operand
// (8 consecutive rows of one column) is still one 16-byte read, and now the sixteen lanes the LDS serves together -- eight columns of
// one octet and eight of the next: MI355X_MICROARCH.md's ds_read_b128 groups -- fall on 64 different banks: 4 cycles per read
// where the 80-byte columns took 8 (SQ_LDS_BANK_CONFLICT was 45 % of the LDS-active cycles, scripts/sim/lds_banks.py), and the tile
// is 80 KB instead of 100.
constexpr bool TM_PLANES = TM_PLANES_N != 0;
constexpr int TM_POS_PITCH = TM_PLANES ? 8 : TM_COL_PITCH;               // f16 from a column position to the next
constexpr int TM_RAW_CHUNKS = TM_MAX_TILES + 4;              // 16-byte chunks per gray row: columns x0 - 24 ...
constexpr int TM_RAW_PITCH = 16 * TM_RAW_CHUNKS;
constexpr int TM_RAW_PIECES = (TM_ROWS * TM_RAW_CHUNKS + 63) / 64;       // 1 KiB DMA pieces per step
constexpr int TM_PIECES_PER_WAVE = (TM_RAW_PIECES + TM_WAVES - 1) / TM_WAVES;
constexpr int TM_OUT_PITCH = 16 * TM_PER_WAVE;               // bytes per row of a wave's class-byte staging
#ifndef TM_DMA_AFTER_BLOCK_N
#define TM_DMA_AFTER_BLOCK_N 2
#endif
constexpr int TM_DMA_AFTER_BLOCK = TM_DMA_AFTER_BLOCK_N;     // the second half of the waves request their rows behind this block of the filter (-1: at the start, like the first half)
#ifndef TM_STORE_ROWS_N
#define TM_STORE_ROWS_N 0
#endif
constexpr bool TM_STORE_ROWS = TM_STORE_ROWS_N != 0;          // whole rows leave behind the step's first barrier (20 store instructions per step instead of 32)
#ifndef TM_STORE_AT_START_N
#define TM_STORE_AT_START_N 1
#endif
constexpr bool TM_STORE_AT_START = TM_STORE_AT_START_N != 0;  // a step's class bytes leave at the start of the next step (0: behind its filter, round 4)
#ifndef TM_BLUR_GROUP_N
#define TM_BLUR_GROUP_N 1
#endif
constexpr int TM_BLUR_GROUP = TM_BLUR_GROUP_N;               // blocks of the blur a wave takes through its phases together (1: one chain per block)
#ifndef TM_PREFETCH_N
#define TM_PREFETCH_N 1
#endif
// the walk's LDS reads (the filter's column and centre operands, the blur's gray bytes) an iteration ahead of their use, outside the
// wave-uniform tests that fence every block: 232 -> 224 us per 256 frames (profiles/r05_ab_thr_prefetch.log)
constexpr bool TM_PREFETCH = TM_PREFETCH_N != 0;
#ifndef TM_LIST_CAP_N
#define TM_LIST_CAP_N 248
#endif
constexpr int TM_LIST_CAP = TM_LIST_CAP_N;                   // ambiguous pixels a workgroup can list

#ifdef YSMR_STAMPS
// phases of one workgroup's walk (stamps build): [wave][step][stamp]; scripts/thr_stamps.py
constexpr int TM_ST_STEPS = 20, TM_ST_N = 8;
__device__ unsigned long long g_tm_stamps[TM_WAVES][TM_ST_STEPS][TM_ST_N];
#define TMSTAMP(step, k) do { if (blockIdx.x == TM_ST_BLOCK && (step) < TM_ST_STEPS && lane == 0) g_tm_stamps[wave][step][k] = __builtin_amdgcn_s_memtime(); } while (0)
#ifndef TM_ST_BLOCK
#define TM_ST_BLOCK 100
#endif
#else
#define TMSTAMP(step, k) do {} while (0)
#endif

// The lane number, opaque to the optimiser: addresses built from it are worked out where they are used (one add in front
// of a phase, the blocks then differ by immediate offsets) instead of being hoisted out of the walk as dozens of
// loop-invariant registers -- which is what spilled (every reload of a spilled register waits vmcnt(0), i.e. for the class-map
// stores and the DMA in flight).
__device__ __forceinline__ int opaque_lane(int lane) { asm volatile("" : "+v"(lane)); return lane; }

struct ThrItem {
    int f, x0, x1, y0, y1;
};

__device__ __forceinline__ int reflect101(int i, int n) { if (i < 0) i = -i; if (i >= n) i = 2 * (n - 1) - i; return i; }
__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// x - float(h) for the low / high half of a packed f16 pair, in one instruction
__device__ __forceinline__ float sub_f16_lo(float x, uint32_t h)
{
    float r;
    asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel_hi:[1,0,0]" : "=v"(r) : "v"(h), "v"(x));
    return r;
}
__device__ __forceinline__ float sub_f16_hi(float x, uint32_t h)
{
    float r;
    asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(r) : "v"(h), "v"(x));
    return r;
}
// float(h) * a + b for the low / high half of a packed f16 pair
__device__ __forceinline__ float mad_f16_lo(uint32_t h, float a, float b)
{
    float r;
    asm("v_fma_mix_f32 %0, %1, %2, %3 op_sel_hi:[1,0,0]" : "=v"(r) : "v"(h), "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ float mad_f16_hi(uint32_t h, float a, float b)
{
    float r;
    asm("v_fma_mix_f32 %0, %1, %2, %3 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(r) : "v"(h), "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ uint32_t pkrtz(float a, float b)
{
    auto h = __builtin_amdgcn_cvt_pkrtz(a, b);
    return __builtin_bit_cast(uint32_t, h);
}
// two floats -> an f16 pair, round to nearest even (v_cvt_pk_f16_f32, new with gfx950)
__device__ __forceinline__ uint32_t pkrtn(float a, float b)
{
    typedef float f32x2 __attribute__((ext_vector_type(2)));
    const f32x2 v = {a, b};
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, half2_t));
}
__device__ __forceinline__ half8_t as_half8(uint32_t a, uint32_t b, uint32_t c, uint32_t d)
{
    u32x4 v = {a, b, c, d};
    return __builtin_bit_cast(half8_t, v);
}
__device__ __forceinline__ uint32_t f16_bits(float x) { _Float16 h = (_Float16)x; unsigned short b; __builtin_memcpy(&b, &h, 2); return b; }
__device__ __forceinline__ float f16_value(uint32_t bits) { unsigned short b = (unsigned short)bits; _Float16 h; __builtin_memcpy(&h, &b, 2); return (float)h; }

// the eleven taps from the six distinct weights
__device__ __forceinline__ float tap_weight(const ysmr_thr::Params &P, int tap) { return P.kw[tap <= 5 ? tap : 10 - tap]; }

// ---- exact path: cv2's float32 arithmetic for one pixel, sixteen lanes per pixel (lane dy computes one row) -------
// Kept SMALL on purpose: the code is cold when a workgroup first needs it, and every instruction-cache line it spans is a
// round trip that the whole workgroup waits for (a fully unrolled version cost 20 us per launch).  The 13 x 13 gray pixels
// around (y, x) -- rows and columns clamped to the image, which is where every reflected neighbour lies -- are staged in
// LDS by one load per lane and row; the blur and the row filter then index that window.
// Every lane of a 16-lane group passes the same (y, x) and a 256-byte scratch of its group; returns the class byte in all.
__device__ __forceinline__ uint32_t exact_class(const uint8_t *frame, const ysmr_thr::Params &P, int y, int x, int lane, uint8_t *win)
{
    const int H = P.H, W = P.W, dy = lane & 15, base = lane & ~15;
    // window[a][b] = gray[clamp(y - 6 + a)][clamp(x - 6 + b)], a, b = 0..12 (pitch 16)
    if (dy < 13) {
        const uint8_t *row = frame + (size_t)clampi(y - 6 + dy, 0, H - 1) * W;
        uint8_t v[13];
#pragma unroll
        for (int b = 0; b < 13; ++b) v[b] = row[clampi(x - 6 + b, 0, W - 1)];
#pragma unroll
        for (int b = 0; b < 13; ++b) win[16 * dy + b] = v[b];
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    // lane dy: the Gaussian's row y - 5 + dy (REPLICATE: clamped), blurred pixels at columns clamp(x - 5 + i)
    const int yy = clampi(y - 5 + min(dy, 10), 0, H - 1);
    const int ra = reflect101(yy - 1, H) - (y - 6), rb = yy - (y - 6), rc = reflect101(yy + 1, H) - (y - 6);
    float acc = 0.0f;
    uint32_t centre = 0;
#pragma unroll 1
    for (int i = 0; i < 11; ++i) {
        const int xx = clampi(x - 5 + i, 0, W - 1);
        const int ca = reflect101(xx - 1, W) - (x - 6), cb = xx - (x - 6), cc = reflect101(xx + 1, W) - (x - 6);
        const uint32_t s = win[16 * ra + ca] + 2u * win[16 * ra + cb] + win[16 * ra + cc] +
                           2u * (win[16 * rb + ca] + 2u * win[16 * rb + cb] + win[16 * rb + cc]) +
                           win[16 * rc + ca] + 2u * win[16 * rc + cb] + win[16 * rc + cc];
        const uint32_t b = (s + 8u) >> 4;
        if (i == 5) centre = b;
        acc = __builtin_fmaf((float)b, tap_weight(P, i), acc);
    }
    // column filter, symmetric form, in every lane (the eleven row values by cross-lane reads)
    float m = __builtin_fmaf(__shfl(acc, base + 5, 64), P.kw[5], 0.0f);
#pragma unroll 1
    for (int j = 1; j <= 5; ++j) m = __builtin_fmaf(__shfl(acc, base + 5 + j, 64) + __shfl(acc, base + 5 - j, 64), P.kw[5 - j], m);
    const uint32_t s = (uint32_t)__shfl((int)centre, base + 5, 64);
    const int mi = clampi((int)__builtin_rintf(m), 0, 255);
    const int d = (int)s - mi;
    const int lo = P.inv ? (d <= P.t_low) : (d > P.t_low);
    const int hi = P.use_high ? (P.inv ? (d <= P.t_high) : (d > P.t_high)) : lo;
    return (uint32_t)(lo | (hi << 1));
}

// The same arithmetic for ONE pixel per WAVE, laid out for latency (the list of a workgroup holds a handful of pixels and
// the whole unit waits for them): the 13 x 13 gray window in one round of loads (three bytes per lane), the 11 x 11
// blurred pixels two per lane, the eleven row chains on eleven lanes, the column pass from their registers.  About 2 us
// for the first pixel against 6-7 us for exact_class's rolled loops (profiles/r04_thr_refine.log).
// scratch: 208 + 528 bytes of the wave's own.
__device__ __forceinline__ uint32_t exact_class_wave(const uint8_t *frame, const ysmr_thr::Params &P, int y, int x, int lane, uint8_t *scratch)
{
    const int H = P.H, W = P.W;
    uint8_t *win = scratch;                                        // [13][16]: gray[clamp(y - 6 + a)][clamp(x - 6 + b)]
    float *bl = reinterpret_cast<float *>(scratch + 208);          // [11][12]: blurred pixels of the Gaussian's window
    uint8_t g[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int e = min(lane + 64 * k, 168), a = e / 13, b = e - 13 * a;
        g[k] = frame[(size_t)clampi(y - 6 + a, 0, H - 1) * W + clampi(x - 6 + b, 0, W - 1)];
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int e = min(lane + 64 * k, 168), a = e / 13, b = e - 13 * a;
        win[16 * a + b] = g[k];
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int e = min(lane + 64 * k, 120), dy = e / 11, i = e - 11 * dy;
        // the Gaussian's row y - 5 + dy and column x - 5 + i (REPLICATE: clamped); the blur around them reflects
        const int yy = clampi(y - 5 + dy, 0, H - 1), xx = clampi(x - 5 + i, 0, W - 1);
        const int ra = reflect101(yy - 1, H) - (y - 6), rb = yy - (y - 6), rc = reflect101(yy + 1, H) - (y - 6);
        const int ca = reflect101(xx - 1, W) - (x - 6), cb = xx - (x - 6), cc = reflect101(xx + 1, W) - (x - 6);
        const uint32_t sum = win[16 * ra + ca] + 2u * win[16 * ra + cb] + win[16 * ra + cc] +
                             2u * (win[16 * rb + ca] + 2u * win[16 * rb + cb] + win[16 * rb + cc]) +
                             win[16 * rc + ca] + 2u * win[16 * rc + cb] + win[16 * rc + cc];
        bl[12 * dy + i] = (float)((sum + 8u) >> 4);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    // row pass: lane dy < 11 runs cv2's ascending chain over its row; column pass: the symmetric form, in every lane
    const float *row = bl + 12 * min(lane, 10);
    float v[11];
#pragma unroll
    for (int i = 0; i < 11; ++i) v[i] = row[i];
    const float centre = bl[12 * 5 + 5];
    float acc = 0.0f;
#pragma unroll
    for (int i = 0; i < 11; ++i) acc = __builtin_fmaf(v[i], tap_weight(P, i), acc);
    auto at = [&](int l) { return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, acc), l)); };
    float m = __builtin_fmaf(at(5), P.kw[5], 0.0f);
#pragma unroll
    for (int j = 1; j <= 5; ++j) m = __builtin_fmaf(at(5 + j) + at(5 - j), P.kw[5 - j], m);
    const int mi = clampi((int)__builtin_rintf(m), 0, 255);
    const int d = (int)centre - mi;
    const int lo = P.inv ? (d <= P.t_low) : (d > P.t_low);
    const int hi = P.use_high ? (P.inv ? (d <= P.t_high) : (d > P.t_high)) : lo;
    return (uint32_t)(lo | (hi << 1));
}

struct Lds {
    // blurred pixels: [column position][row of a 2 x 16-row ring] at TM_COL_PITCH, or four planes [row octet][column position][8 rows]
    _Float16 tile[TM_PLANES ? 4 * TM_POS * 8 : TM_POS * TM_COL_PITCH];
    __device__ __forceinline__ _Float16 *at(int pos, int row)       // row: a multiple of 4 here (operands are 8 rows, the blur writes 4)
    {
        return TM_PLANES ? &tile[(row >> 3) * (TM_POS * 8) + pos * 8 + (row & 7)] : &tile[pos * TM_COL_PITCH + row];
    }
    uint8_t raw[2][TM_ROWS * TM_RAW_PITCH];              // gray rows of a step: row r, columns x0 - 24 ... at r * 16 * (chunks per row)
    // a wave's class bytes of a step; with the memory wave: the step's sixteen dense rows of 16 ntiles bytes (read as one array)
    uint32_t out[TM_WAVES][TM_MEM_WAVE ? TM_ROWS * 16 * TM_MAX_TILES / 4 / TM_WAVES : TM_ROWS * TM_OUT_PITCH / 4];
    uint8_t side[TM_MEM_WAVE ? 2 : 1][512];              // the memory wave: the two 16-row x 16-byte chunks that straddle a row's ends, as they come from memory
    uint32_t list[TM_LIST_CAP];                          // ambiguous pixels: y << 16 | x ...
    uint16_t list_f[TM_LIST_CAP];                        // ... and their frame (the list is worked off once per workgroup)
    uint32_t n_list;
};
static_assert(sizeof(Lds) <= 160 * 1024, "LDS of one CU");
static_assert(!TM_MEM_WAVE || (TM_ROWS * 16 * TM_MAX_TILES / 4) % TM_WAVES == 0, "the dense staging rows as TM_WAVES equal parts");
static_assert(sizeof(Lds::out) >= 256 * (TM_THREADS / 16), "the exact path's windows live in the class-byte staging");
static_assert(sizeof(Lds::out) >= 768 * TM_WAVES, "and so does the wave-per-pixel form's scratch");

// f16 bit pattern of w / 16 for w = 0..4 (the blur's column taps carry the division by 16)
__device__ __forceinline__ uint32_t small_f16(int w) { return w == 0 ? 0u : w == 1 ? 0x2C00u : w == 2 ? 0x3000u : w == 3 ? 0x3200u : 0x3400u; }

template <int EPS_MODE>
__global__ __launch_bounds__(TM_THREADS) __attribute__((amdgpu_waves_per_eu(4, 4))) void k_threshold_mfma(const uint8_t *__restrict__ frames, uint8_t *__restrict__ cls,
                                                               ysmr_thr::Params P)
{
    extern __shared__ __align__(16) uint8_t lds_bytes[];
    Lds &L = *reinterpret_cast<Lds *>(lds_bytes);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int H = P.H, W = P.W;
    const int l16 = lane & 15, q = lane >> 4;

    // ---- constant MFMA operands of this lane (all maps: lane (x = l16, q) holds k = (8 or 16) q + j) -------------------
    // blur rows, B [k][n] (i8, K = 64): k is gray column 16u - 24 + k, n is tile position 16u + n = column 16u - 8 + n.
    uint32_t thi[4];
    // blur columns, A [m][k] (f16, K = 32): halves j = 0..3 / 4..7 of the other operand hold rows 4q + (j & 3) of one 16-row
    // block of row sums each; variant v: the NEWER block sits in half v.  Window row w = 4q + (j & 3) (+ 16 for the newer
    // block); output row m is centred on window row 15 + m.
    uint32_t tv[4];                   // (variant 1 is variant 0 with its register pairs exchanged: built where it is used)
    // Gaussian columns, B [k][n]: k = window row (0..15 the older tile block, 16..31 the newer), output row n is window
    // row n + 8: tap k - n - 3.  ONE f16 per tap (round 5): the taps are scaled by P.col_scale, chosen on the host so that the
    // eleven scaled weights lie close to f16 values (the bound: detect_plan.h).
    uint32_t tbh[4];
    // Gaussian rows, B [k][n]: the A operand is two column blocks' accumulators kept in place, halves j = 0..3 / 4..7 =
    // positions 4q + (j & 3) of one block each; variant v: the RIGHT block (u = t + 1) sits in half v.  Position i of block u
    // is column 16u - 8 + i, output n is column 16t + n: tap = column_in - n + 5.  These taps carry the classification's scale
    // (and undo the column pass's).
    uint32_t thh[4];                  // (variant 0; variant 1 likewise)
    // The row pass runs TRANSPOSED (taps as the A operand, the column-filtered values as B): its result then has a lane
    // hold four consecutive COLUMNS of one row (columns 4q + r of row l16) -- one dword of class bytes.  Its accumulator
    // starts at lo_add - x_mul (b - 128) in that same layout: one more product, blurred tile (A: column l16, window rows k) times
    // B [k][n] = -x_mul if window row k is output row n (k = n + 8), on top of lo_add.
    uint32_t bid[4];
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) {
        uint32_t b1 = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int d = 16 * q + 4 * jj + e - 16 - l16;        // gray column minus output column
            b1 |= (uint32_t)(d == 0 ? 2 : (d == 1 || d == -1) ? 1 : 0) << (8 * e);
        }
        thi[jj] = b1;
        uint32_t v0 = 0, bh = 0, hh = 0, bd = 0;
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int j = 2 * jj + e, k = 8 * q + j;
            const int w0 = 4 * q + (j & 3) + ((j >> 2) == 0 ? 16 : 0);
            const int d0 = w0 - 15 - l16;
            v0 |= small_f16(d0 == 0 ? 2 : (d0 == 1 || d0 == -1) ? 1 : 0) << (16 * e);
            bd |= (k == l16 + 8 ? f16_bits(P.neg_x_mul) : 0u) << (16 * e);
            int taps[2] = {k - l16 - 3, -8 + 4 * q + (j & 3) + ((j >> 2) == 0 ? 16 : 0) - l16 + 5};
            uint32_t hb[2];
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const bool ok = taps[c] >= 0 && taps[c] <= 10;
                const float w = ok ? tap_weight(P, clampi(taps[c], 0, 10)) * (c == 0 ? P.col_scale : P.row_scale) : 0.0f;
                hb[c] = f16_bits(w);
            }
            bh |= hb[0] << (16 * e);
            hh |= hb[1] << (16 * e);
        }
        tv[jj] = v0; bid[jj] = bd;
        tbh[jj] = bh;
        thh[jj] = hh;
    }
    const i32x4 THI = {(int)thi[0], (int)thi[1], (int)thi[2], (int)thi[3]};
    // accumulator presets (kept in registers: an MFMA whose preset stays live writes its result elsewhere, no copies).
    // Row sums: 0x6400 + 512 + sum over (gray - 128) = the f16 BIT PATTERN of 1024 + row sum (0 .. 1020).
    // Column sums: the taps are (1, 2, 1) / 16, so the product is 256 + S / 16 exactly; + 768.5 and a round-toward-zero
    // conversion at 1024 + x, where f16 counts in ones, leaves 1024 + ((S + 8) >> 4).
    i32x4 K_ROW = {0x6600, 0x6600, 0x6600, 0x6600};
    f32x4 K_COL = {768.5f, 768.5f, 768.5f, 768.5f};
    f32x4 K_LO = {P.k_first, P.k_first, P.k_first, P.k_first};
    asm volatile("" : "+v"(K_ROW), "+v"(K_COL), "+v"(K_LO));   // (opaque: not rematerialised as four moves per use)
    const half8_t BID = as_half8(bid[0], bid[1], bid[2], bid[3]);
    const half8_t TBh = as_half8(tbh[0], tbh[1], tbh[2], tbh[3]);

    // every tile entry and gray byte must be a finite number from the first read on (they meet zero taps)
    for (int i = tid; i < (int)((sizeof(L.tile) + sizeof(L.raw)) / 4); i += TM_THREADS) reinterpret_cast<uint32_t *>(lds_bytes)[i] = 0u;
    if (tid == 0) L.n_list = 0;
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");

    // Work: the rows of every (frame, panel) column, laid end to end and cut into one equal range per workgroup -- whatever
    // the number of workgroups (256; 255 when the batch link holds a compute unit: with one item per workgroup and one unit
    // short, the last item started when the others ended and the kernel took twice its time).  A range that crosses the
    // end of a column is two items (each re-filters its own 16 halo rows).  With a grid that is a multiple of 8 every XCD
    // works through whole frames (f = 8 k + xcd), so a range's halo rows come out of the XCD's own L2.
    const int groups = P.by_xcd ? 8 : 1;
    const long long cols = (long long)(P.batch / groups) * P.panels, rows_all = cols * H;
    const long long nb = gridDim.x / groups, bi = P.by_xcd ? (blockIdx.x >> 3) : blockIdx.x;
    // Equal COST, not equal rows: starting an item (two blocks of rows fetched and blurred before the first output row)
    // costs what P.start_rows rows of the walk cost, and a range that holds the top of a column starts two items.  The cut
    // is even in a space where every column is that much longer (its top repeated); a position there maps back to a row.
    // (The host passes 0 when the workgroups divide the columns evenly: every range then starts exactly one item.)
    (void)rows_all;
    const long long vh = H + P.start_rows, v_all = cols * vh;
    auto real_row = [&](long long v) { const long long c = v / vh, r = v - c * vh; return c * H + (r > P.start_rows ? r - P.start_rows : 0); };
    long long g0 = real_row(v_all * bi / nb);
    const long long g1 = bi + 1 == nb ? cols * H : real_row(v_all * (bi + 1) / nb);
    const int f_add = P.by_xcd ? (int)(blockIdx.x & 7u) : 0;

    uint32_t n_kept = 0;                                   // listed pixels of the items done so far
    while (g0 < g1) {
        ThrItem it;
        {
            const long long col = g0 / H;
            it.f = (int)(col / P.panels) * groups + f_add;
            const int panel = (int)(col % P.panels);
            it.x0 = panel * P.panel_w; it.x1 = min(it.x0 + P.panel_w, W);
            it.y0 = (int)(g0 % H);
            it.y1 = (int)min((long long)H, it.y0 + (g1 - g0));
            g0 += it.y1 - it.y0;
        }
        const uint8_t *frame = frames + (size_t)it.f * H * W;
        uint8_t *dst = cls + (size_t)it.f * H * W;
        const int PW = it.x1 - it.x0;                       // a multiple of 4
        int ntiles = (PW + 15) >> 4;                        // output tiles; column blocks u = 0 .. ntiles (not const: TM_FRESH below)
        const int nch = ntiles + 4;                         // gray chunks per row
        const int nblk = (it.y1 - it.y0 + TM_ROWS - 1) / TM_ROWS;
        const bool edge_l = it.x0 == 0, edge_r = it.x1 == W;
        // this wave's blocks u0 .. u0 + cnt - 1 and tiles t = u0 .. u0 + cnt - 1
        int u0 = TM_MEM_WAVE ? 5 * wave + (wave > 3) + (wave > 7) + (wave > 11) : wave * TM_PER_WAVE;
        int cnt = TM_MEM_WAVE ? (wave == TM_WAVES - 1 ? 0 : 5 + ((wave & 3) == 3)) : TM_PER_WAVE;
        // blurred block j holds rows yb(j) .. + 15; it is made of gray blocks j - 1 and j (rows yb(j) + 1 ...)
        auto yb = [&](int j) { return it.y0 - 8 + TM_ROWS * j; };

        // ---- gray rows: whole 16-byte chunks by LDS-DMA; chunks that straddle the row's ends through registers ------------
        const int npieces = (TM_ROWS * nch + 63) >> 6;
        const uint32_t nch_recip = 65536u / (uint32_t)nch + 1u;          // chunk index / nch for indices < 2048
        // Chunks that straddle an end of the image row go through registers (lanes 0..15 of the last wave: the chunk that
        // holds columns -8 .. 7; lanes 16..31: the chunk that holds column W), and they carry the blur's REFLECT_101
        // neighbours: column -1 := column 1, column W := column W - 2 -- the banded matrix of the row pass is the same everywhere.
        const int part_c = lane < 16 ? 1 : (W - (it.x0 - 24)) >> 4;
        const int part_col = it.x0 - 24 + 16 * part_c;
        const bool part_lane = lane < 32 && part_c < nch && (lane < 16 ? edge_l : edge_r);
        auto part_load = [&](int j, u32x4 &v, uint32_t &last4) __attribute__((always_inline)) {
            const uint8_t *row = frame + (size_t)clampi(yb(j) + 1 + (lane & 15), 0, H - 1) * W;
#pragma unroll
            for (int i = 0; i < 4; ++i) v[i] = *reinterpret_cast<const uint32_t *>(row + clampi(part_col + 4 * i, 0, W - 4));
            last4 = *reinterpret_cast<const uint32_t *>(row + W - 4);
        };
        auto part_write = [&](int j, u32x4 v, uint32_t last4) __attribute__((always_inline)) {
            if (lane < 16) {
                v[1] = (v[1] & 0x00FFFFFFu) | ((v[2] << 16) & 0xFF000000u);           // column -1 := column 1
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (part_col + 4 * i == W) v[i] = (v[i] & 0xFFFFFF00u) | ((last4 >> 16) & 0xFFu);   // column W := column W - 2
            }
            *reinterpret_cast<u32x4 *>(&L.raw[j & 1][(lane & 15) * 16 * nch + 16 * part_c]) = v;   // (rows lie 16 nch bytes apart: the DMA's chunk order)
        };
        // What a lane fetches does not change along the walk: chunk (r, c) of every 16-row block -- worked out once per item.
        uint32_t rq_off[TM_PIECES_PER_WAVE];               // r W + column, for blocks that lie inside the image
        bool rq_on[TM_PIECES_PER_WAVE];
        int rq_n = 0;                                       // DMA instructions per request: the step waits with a COUNTED vmcnt
        auto rq_chunk = [&](int k, int &r, int &col) __attribute__((always_inline)) {
            const uint32_t ci = (uint32_t)(wave + TM_WAVES * k) * 64u + (uint32_t)lane;
            r = (int)((ci * nch_recip) >> 16);
            col = it.x0 - 24 + 16 * ((int)ci - r * nch);
        };
#pragma unroll
        for (int k = 0; k < TM_PIECES_PER_WAVE; ++k) {
            int r, col;
            rq_chunk(k, r, col);
            rq_off[k] = (uint32_t)r * (uint32_t)W + (uint32_t)max(col, 0);
            rq_on[k] = wave + TM_WAVES * k < npieces && r < TM_ROWS && col >= 0 && col + 16 <= W;
            rq_n += __builtin_amdgcn_ballot_w64(rq_on[k]) != 0ull ? 1 : 0;          // (no lane: the instruction is branched over)
        }
        rq_n = __builtin_amdgcn_readfirstlane(rq_n);
        auto request_raw = [&](int j) __attribute__((always_inline)) -> int {
#ifdef TM_DBG_NOLOAD
            return 0;
#endif
            const int r0 = yb(j) + 1;
            const bool inside = r0 >= 0 && r0 + TM_ROWS <= H;                  // (wave-uniform)
#pragma unroll
            for (int k = 0; k < TM_PIECES_PER_WAVE; ++k) {
                const int piece = wave + TM_WAVES * k;
                if (piece < npieces) {   // wave-uniform
                    const uint32_t lds = (uint32_t)(uintptr_t)&L.raw[j & 1][piece * 1024];
                    uint32_t off = rq_off[k] + (uint32_t)(r0 * W);
                    if (!inside) {       // rows above / below the image repeat its first / last row
                        int r, col;
                        rq_chunk(k, r, col);
                        off = (uint32_t)clampi(r0 + r, 0, H - 1) * (uint32_t)W + (uint32_t)max(col, 0);
                    }
                    if (rq_on[k])
#ifdef TM_NT_LOADS
                        asm volatile("s_mov_b32 m0, %0\n\tglobal_load_lds_dwordx4 %1, %2 nt" ::"s"(__builtin_amdgcn_readfirstlane(lds)), "v"(off), "s"(frame) : "memory");
#else
                        asm volatile("s_mov_b32 m0, %0\n\tglobal_load_lds_dwordx4 %1, %2" ::"s"(__builtin_amdgcn_readfirstlane(lds)), "v"(off), "s"(frame) : "memory");
#endif
                }
            }
            if (wave == TM_WAVES - 1) {   // the lightest wave waits for these sixteen-plus-sixteen chunks at once
                if (part_lane) {
                    u32x4 v;
                    uint32_t last4;
                    part_load(j, v, last4);
                    part_write(j, v, last4);
                }
            }
            return rq_n;
        };

        // The memory wave's form: block j row by row, addressed on the SCALAR unit -- a row's chunks 64 g .. 64 g + 63 are one
        // instruction whose lanes read 16 lane bytes behind a scalar base (the clamped row, the panel's first gray column) under an
        // execution mask that leaves out the chunks beyond the image's ends; two scalar additions, m0 and the request per piece,
        // no vector arithmetic.  (The first build walked 64-chunk pieces across the rows with per-lane arithmetic, ~30
        // instructions and three branches per piece: 250 cycles apiece, 5 300 per step -- profiles/r05_thr_stamps_memory_wave.log.)
        const int c_lo = it.x0 >= 24 ? 0 : (24 - it.x0 + 15) >> 4;                          // first chunk that lies inside the row
        const int c_hi = min(nch - 1, (W - 16 - (it.x0 - 24)) >> 4);                       // last one
        auto lane_mask = [](int lo, int hi) -> uint64_t {                                   // lanes lo .. hi of 0 .. 63 (scalar)
            lo = lo < 0 ? 0 : lo; hi = hi > 63 ? 63 : hi;
            if (lo > hi) return 0ull;
            const uint64_t upto = hi >= 63 ? ~0ull : ((1ull << (hi + 1)) - 1ull);
            return upto & ~((1ull << lo) - 1ull);
        };
        auto dma_piece = [&](uint64_t mask, uint32_t m0v, const uint8_t *sbase, uint32_t lane16) __attribute__((always_inline)) {
            uint64_t saved;
            asm volatile("s_mov_b64 %0, exec\n\ts_mov_b64 exec, %1\n\ts_mov_b32 m0, %2\n\tglobal_load_lds_dwordx4 %3, %4\n\ts_mov_b64 exec, %0"
                         : "=&s"(saved) : "s"(mask), "s"(__builtin_amdgcn_readfirstlane(m0v)), "v"(lane16), "s"(sbase) : "memory");
        };
        // sixteen consecutive rows inside the image: the request, the next row's LDS address (m0 += the row pitch), the next row's
        // offset (a lane's += W) -- three instructions per piece under one execution mask
        auto dma_rows16 = [&](uint64_t mask, uint32_t m0v, const uint8_t *sbase, uint32_t voff) __attribute__((always_inline)) {
            uint64_t saved;
            asm volatile("s_mov_b64 %0, exec\n\ts_mov_b64 exec, %2\n\ts_mov_b32 m0, %3\n\t"
                         ".rept 16\n\tglobal_load_lds_dwordx4 %1, %4\n\ts_add_u32 m0, m0, %6\n\tv_add_u32 %1, %5, %1\n\t.endr\n\t"
                         "s_mov_b64 exec, %0"
                         : "=&s"(saved), "+v"(voff) : "s"(mask), "s"(m0v), "s"(sbase), "s"(W), "s"(16 * nch) : "memory", "scc");
        };
        const int part_cr = (W - (it.x0 - 24)) >> 4;        // the chunk that holds column W (edge_r)
        const bool side_l = edge_l && 1 < nch, side_r = edge_r && part_cr < nch;
        auto request_all = [&](int j) __attribute__((always_inline)) -> int {
#ifdef TM_DBG_NOLOAD
            return 0;
#endif
            const int r0 = yb(j) + 1;
            const bool inside = r0 >= 0 && r0 + TM_ROWS <= H;                  // (wave-uniform)
            const uint32_t lds0 = (uint32_t)(uintptr_t)&L.raw[j & 1][0];
            const uint64_t dma_mask0 = lane_mask(c_lo, c_hi), dma_mask1 = lane_mask(c_lo - 64, c_hi - 64);
            const int lo = opaque_lane(lane);
            const uint32_t lane16 = 16u * (uint32_t)lo;
            int n = 0;
            if (inside) {
                const uint8_t *sbase = frame + (ptrdiff_t)r0 * W + (it.x0 - 24);
                if (dma_mask0 != 0ull) { dma_rows16(dma_mask0, lds0, sbase, lane16); n += TM_ROWS; }
                if (dma_mask1 != 0ull) { dma_rows16(dma_mask1, lds0 + 1024u, sbase + 1024, lane16); n += TM_ROWS; }
            } else {
#pragma unroll 1
                for (int r = 0; r < TM_ROWS; ++r) {
                    const uint8_t *sbase = frame + (ptrdiff_t)clampi(r0 + r, 0, H - 1) * W + (it.x0 - 24);     // rows above / below the image repeat its first / last row
                    if (dma_mask0 != 0ull) { dma_piece(dma_mask0, lds0 + (uint32_t)(r * 16 * nch), sbase, lane16); ++n; }
                    if (dma_mask1 != 0ull) { dma_piece(dma_mask1, lds0 + (uint32_t)(r * 16 * nch) + 1024u, sbase + 1024, lane16); ++n; }
                }
            }
            // the chunks that straddle the row's ends: dword by dword (clamped into the row) into the side buffer, lane = 4 row + dword
            if (side_l || side_r) {   // wave-uniform
                const uint32_t rowoff = (uint32_t)clampi(r0 + (lo >> 2), 0, H - 1) * (uint32_t)W;
                if (side_l) {
                    const uint32_t off = rowoff + (uint32_t)clampi(it.x0 - 8 + 4 * (lo & 3), 0, W - 4);
                    asm volatile("s_mov_b32 m0, %0\n\tglobal_load_lds_dword %1, %2" ::"s"((uint32_t)(uintptr_t)&L.side[j & 1][0]), "v"(off), "s"(frame) : "memory");
                    ++n;
                }
                if (side_r) {
                    const uint32_t off = rowoff + (uint32_t)clampi(it.x0 - 24 + 16 * part_cr + 4 * (lo & 3), 0, W - 4);
                    asm volatile("s_mov_b32 m0, %0\n\tglobal_load_lds_dword %1, %2" ::"s"((uint32_t)(uintptr_t)&L.side[j & 1][256]), "v"(off), "s"(frame) : "memory");
                    ++n;
                }
            }
            return n;
        };
        // ... and, once they have landed: the blur's REFLECT_101 neighbours patched in (as part_write), into the rows' chunks
        auto side_patch = [&](int j) __attribute__((always_inline)) {
            if (part_lane) {
                const u32x4 v = *reinterpret_cast<const u32x4 *>(&L.side[j & 1][(lane < 16 ? 0 : 256) + 16 * (lane & 15)]);
                uint32_t last4 = 0;
#pragma unroll
                for (int i = 0; i < 4; ++i) last4 = part_col + 4 * i == W ? v[i] : last4;      // (the dword asked for at column W was clamped to W - 4)
                part_write(j, v, last4);
            }
        };
        auto wait_all_but_n = [&](int n) __attribute__((always_inline)) {    // n: wave-uniform, at most 32 (two pieces per row)
            switch (n) {
#define TM_W(i) case i: asm volatile("s_waitcnt vmcnt(" #i ")" ::: "memory"); break;
                TM_W(1) TM_W(2) TM_W(3) TM_W(4) TM_W(5) TM_W(6) TM_W(7) TM_W(8) TM_W(9) TM_W(10) TM_W(11) TM_W(12) TM_W(13) TM_W(14) TM_W(15) TM_W(16)
                TM_W(17) TM_W(18) TM_W(19) TM_W(20) TM_W(21) TM_W(22) TM_W(23) TM_W(24) TM_W(25) TM_W(26) TM_W(27) TM_W(28) TM_W(29) TM_W(30) TM_W(31) TM_W(32)
#undef TM_W
                default: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
            }
        };
        static_assert(TM_RAW_CHUNKS <= 128, "two pieces per gray row");

        // ---- blur: gray block j -> row sums (kept for two steps) -> tile block j ------------------------------------------
        uint32_t hst[TM_PER_WAVE][4];
#pragma unroll
        for (int bi = 0; bi < TM_PER_WAVE; ++bi)
#pragma unroll
            for (int k = 0; k < 4; ++k) hst[bi][k] = 0x64006400u;
        const bool blur_left = edge_l && u0 == 0;
        const bool blur_right = edge_r && ((PW + 7) >> 4) >= u0 && ((PW + 7) >> 4) < u0 + cnt && ((PW + 7) >> 4) <= ntiles;
        auto blur_step = [&](int j, auto par_tag, auto sums_tag) __attribute__((always_inline)) {
#ifdef TM_DBG_NOBLUR
            return;
#endif
            constexpr int PAR = decltype(par_tag)::value;    // j & 1: the half the new sums go to
            constexpr bool SUMS_ONLY = decltype(sums_tag)::value;
            const uint8_t *raw = L.raw[j & 1];
            // column taps: the interior constant, or (blocks that touch the image's first / last row) built here: a row outside
            // the image repeats the nearest inside, and that row's neighbours reflect
            uint32_t tvv[4] = {tv[2 * PAR], tv[2 * PAR + 1], tv[2 - 2 * PAR], tv[3 - 2 * PAR]};
            if (!SUMS_ONLY && (yb(j) < 1 || yb(j) + TM_ROWS > H - 1)) {   // wave-uniform
                const int lc = opaque_lane(lane), l16 = lc & 15, q = lc >> 4;          // (cold: nothing of it hoisted out of the walk)
                const int yc = clampi(yb(j) + l16, 0, H - 1);
                const int ra = reflect101(yc - 1, H), rc = reflect101(yc + 1, H);
#pragma unroll
                for (int jj = 0; jj < 4; ++jj) {
                    uint32_t v = 0;
#pragma unroll
                    for (int e = 0; e < 2; ++e) {
                        const int jx = 2 * jj + e;
                        const int rho = yb(j) + 1 - TM_ROWS + 4 * q + (jx & 3) + ((jx >> 2) == PAR ? 16 : 0);   // gray row of the slot
                        v |= small_f16((rho == ra) + 2 * (rho == yc) + (rho == rc)) << (16 * e);
                    }
                    tvv[jj] = v;
                }
            }
            const half8_t TV = as_half8(tvv[0], tvv[1], tvv[2], tvv[3]);
            const int lo = opaque_lane(lane), l16o = lo & 15, qo = lo >> 4;
            const uint8_t *rawp = raw + l16o * 16 * nch + 16 * u0 + 16 * qo;
            uint2 *cellp = reinterpret_cast<uint2 *>(L.at(16 * u0 + l16o, 16 * PAR + 4 * qo));
            if constexpr (TM_BLUR_GROUP > 1) {
                // Blocks in groups of TM_BLUR_GROUP, phase by phase in straight-line code: the LDS reads, the row products, the column
                // products, the conversions of the group's blocks back to back, then their (guarded) writes.  One block at a time is
                // a chain of LDS latency, two MFMA latencies and three waits that the compiler cannot overlap with the next block's
                // (each sits behind its own wave-uniform test): a wave's five blocks took 2 100 - 2 800 cycles where their
                // instructions issue in ~450, and four such waves do not fill a SIMD (profiles/r05_thr_stamps_*.log).  Blocks beyond
                // the panel (the last wave's) are computed like the others -- their reads stay inside LDS, nobody uses the result --
                // only their tile writes are held back.
                const half2_t bias = {(_Float16)1152.0f, (_Float16)1152.0f};
#pragma unroll
                for (int g0 = 0; g0 < TM_PER_WAVE; g0 += TM_BLUR_GROUP) {
                    constexpr int G = TM_BLUR_GROUP;
                    u32x4 a[G];
                    i32x4 ch[G];
                    f32x4 y[G];
                    uint32_t b01[G], b23[G];
#pragma unroll
                    for (int b = 0; b < G; ++b)
                        if (g0 + b < TM_PER_WAVE) a[b] = *reinterpret_cast<const u32x4 *>(rawp + 16 * (g0 + b));
#pragma unroll
                    for (int b = 0; b < G; ++b)
                        if (g0 + b < TM_PER_WAVE) {
                            a[b] ^= 0x80808080u;
                            ch[b] = __builtin_amdgcn_mfma_i32_16x16x64_i8(__builtin_bit_cast(i32x4, a[b]), THI, K_ROW, 0, 0, 0);
                        }
#pragma unroll
                    for (int b = 0; b < G; ++b)
                        if (g0 + b < TM_PER_WAVE) {
                            const int bi = g0 + b;
                            hst[bi][2 * PAR] = ((uint32_t)ch[b][1] << 16) | (uint32_t)ch[b][0];
                            hst[bi][2 * PAR + 1] = ((uint32_t)ch[b][3] << 16) | (uint32_t)ch[b][2];
                            if (!SUMS_ONLY)
                                y[b] = __builtin_amdgcn_mfma_f32_16x16x32_f16(TV, as_half8(hst[bi][0], hst[bi][1], hst[bi][2], hst[bi][3]), K_COL, 0, 0, 0);
                        }
                    if (!SUMS_ONLY) {
#pragma unroll
                        for (int b = 0; b < G; ++b)
                            if (g0 + b < TM_PER_WAVE) {
                                b01[b] = __builtin_bit_cast(uint32_t, __builtin_bit_cast(half2_t, pkrtz(y[b][0], y[b][1])) - bias);
                                b23[b] = __builtin_bit_cast(uint32_t, __builtin_bit_cast(half2_t, pkrtz(y[b][2], y[b][3])) - bias);
                            }
                        __builtin_amdgcn_sched_barrier(0);       // (the writes and their tests behind the arithmetic of the whole group)
#pragma unroll
                        for (int b = 0; b < G; ++b)
                            if (g0 + b < TM_PER_WAVE) {
                                const int bi = g0 + b, u = u0 + bi;
                                uint2 *cell = cellp + bi * (16 * TM_POS_PITCH / 4);
                                if (u <= ntiles && (!edge_r || 16 * u <= PW + 7)) *cell = make_uint2(b01[b], b23[b]);
                                if (edge_l && u == 0) {                          // wave-uniform
                                    if (l16o == 8)
#pragma unroll
                                        for (int e = 1; e <= 8; ++e) cell[-e * (TM_POS_PITCH / 4)] = make_uint2(b01[b], b23[b]);
                                }
                                if (edge_r && u == (PW + 7) >> 4) {              // wave-uniform: the block of column W - 1
                                    if (l16o == ((PW + 7) & 15))
                                        for (int e = 1; PW + 7 + e < 16 * ntiles + 16; ++e) cell[e * (TM_POS_PITCH / 4)] = make_uint2(b01[b], b23[b]);
                                }
                            }
                    }
                    __builtin_amdgcn_sched_barrier(0);           // (one group's registers at a time)
                }
                return;
            }
            u32x4 a_pre = {};
            if (TM_PREFETCH) a_pre = *reinterpret_cast<const u32x4 *>(rawp);
#pragma unroll
            for (int bi = 0; bi < TM_PER_WAVE; ++bi) {
                const int u = u0 + bi;
                const u32x4 a_now = a_pre;
                if (TM_PREFETCH && bi + 1 < TM_PER_WAVE) a_pre = *reinterpret_cast<const u32x4 *>(rawp + 16 * (bi + 1));   // (the next block's gray bytes, whether it exists or not)
                if (u <= ntiles && bi < cnt) {   // wave-uniform
                    u32x4 a = TM_PREFETCH ? a_now : *reinterpret_cast<const u32x4 *>(rawp + 16 * bi);
                    a ^= 0x80808080u;
                    const i32x4 ch = __builtin_amdgcn_mfma_i32_16x16x64_i8(__builtin_bit_cast(i32x4, a), THI, K_ROW, 0, 0, 0);
                    hst[bi][2 * PAR] = ((uint32_t)ch[1] << 16) | (uint32_t)ch[0];
                    hst[bi][2 * PAR + 1] = ((uint32_t)ch[3] << 16) | (uint32_t)ch[2];
                    if (!SUMS_ONLY) {
                        const f32x4 y = __builtin_amdgcn_mfma_f32_16x16x32_f16(TV, as_half8(hst[bi][0], hst[bi][1], hst[bi][2], hst[bi][3]), K_COL, 0, 0, 0);
                        // y = 1024.5 + S / 16, exactly; the tile holds b - 128 (exact integers -128 .. 127: what the Gaussian's f16
                        // taps multiply is centred, so their rounding errors meet |b - 128| <= 128, not b <= 255)
                        const half2_t bias = {(_Float16)1152.0f, (_Float16)1152.0f};
                        const uint32_t b01 = __builtin_bit_cast(uint32_t, __builtin_bit_cast(half2_t, pkrtz(y[0], y[1])) - bias);
                        const uint32_t b23 = __builtin_bit_cast(uint32_t, __builtin_bit_cast(half2_t, pkrtz(y[2], y[3])) - bias);
                        uint2 *cell = cellp + bi * (16 * TM_POS_PITCH / 4);
                        // (positions beyond column W - 1 in the block of that column are rewritten by the lane that holds it, below:
                        // a wave's LDS accesses complete in order; a block wholly beyond it -- wave-uniform -- stays away)
                        if (!edge_r || 16 * u <= PW + 7) *cell = make_uint2(b01, b23);
                    }
                }
                if (bi & 1) __builtin_amdgcn_sched_barrier(0);   // (two blocks in flight are enough; all five cost registers)
            }
            // the Gaussian's REPLICATE border: columns < 0 repeat column 0 (position 8), columns >= W column W - 1.  Behind the
            // blocks, for the one or two waves of a panel that hold an image edge (round 4 tested every block of every wave for
            // both edges: two v_readlane, a v_cmp and a dozen scalar instructions per block): the lane that holds the edge column
            // reads back what it has just written (a wave's LDS accesses complete in order) and copies it outward.
            if (!SUMS_ONLY && blur_left) {                               // wave-uniform
                if (l16o == 8) {
                    const uint2 v = *cellp;
#pragma unroll
                    for (int e = 1; e <= 8; ++e) cellp[-e * (TM_POS_PITCH / 4)] = v;
                }
            }
            if (!SUMS_ONLY && blur_right) {                              // wave-uniform: the block of column W - 1 is this wave's
                if (l16o == ((PW + 7) & 15)) {
                    uint2 *cell = cellp + (((PW + 7) >> 4) - u0) * (16 * TM_POS_PITCH / 4);
                    const uint2 v = *cell;
                    for (int e = 1; PW + 7 + e < 16 * ntiles + 16; ++e) cell[e * (TM_POS_PITCH / 4)] = v;
                }
            }
        };

        // ---- filter: output rows of step s - 1 = window rows 8 .. 23 (window rows 0..15: tile block s - 1, 16..31: block s) ---
        auto filter_step = [&](int s, bool late_dma, int &mine) __attribute__((always_inline)) {
#ifdef TM_DBG_NOFILTER
            if (late_dma) mine = request_raw(s + 2);
            return;
#endif
            const int oy = it.y0 + TM_ROWS * (s - 1);            // first output row
            const int lo = opaque_lane(lane), l16o = lo & 15, qo = lo >> 4;
            // this lane's dword of a tile's staging rows (a block per wave; with the memory wave: dense rows of the whole panel)
            uint8_t *wout = TM_MEM_WAVE ? reinterpret_cast<uint8_t *>(L.out) + l16o * (16 * ntiles) + 16 * u0 + 4 * qo
                                        : reinterpret_cast<uint8_t *>(L.out[wave]) + l16o * TM_OUT_PITCH + 4 * qo;
            // window rows 8q .. 8q + 7 of this lane's column (A operand of the column pass), from the wave's first block on
            const _Float16 *colp = L.at(16 * u0 + l16o, (qo >> 1 ? (s & 1) : ((s - 1) & 1)) * 16 + 8 * (qo & 1));
            uint32_t xh[4] = {0, 0, 0, 0};
            const half8_t THh[2] = {as_half8(thh[0], thh[1], thh[2], thh[3]), as_half8(thh[2], thh[3], thh[0], thh[1])};
            // TM_PREFETCH: the two LDS reads of an iteration -- the next block's column, the next tile's centre pixels -- are issued an
            // iteration ahead, whatever the tests below say (a block beyond the panel reads LDS bytes nobody uses)
            half8_t A_pre = {}, Ab_pre = {};
            if (TM_PREFETCH) A_pre = *reinterpret_cast<const half8_t *>(colp);
#pragma unroll
            for (int bi = 0; bi <= TM_PER_WAVE; ++bi) {
                const int u = u0 + bi;                            // column block: positions 16u .. 16u + 15
                const int hsel = bi & 1;
                const half8_t A_now = A_pre, Ab_now = Ab_pre;
                if (TM_PREFETCH && bi < TM_PER_WAVE) {
                    A_pre = *reinterpret_cast<const half8_t *>(colp + 16 * (bi + 1) * TM_POS_PITCH);
                    Ab_pre = *reinterpret_cast<const half8_t *>(colp + (16 * bi + 8) * TM_POS_PITCH);
                }
                if ((bi == 0 ? u < ntiles : u - 1 < ntiles) && bi <= cnt && cnt > 0) {      // some tile of this wave uses the block (wave-uniform)
                    const half8_t A = TM_PREFETCH ? A_now : *reinterpret_cast<const half8_t *>(colp + 16 * bi * TM_POS_PITCH);
                    f32x4 cv = {0.f, 0.f, 0.f, 0.f};
#ifndef TM_DBG_NOMFMA
                    cv = __builtin_amdgcn_mfma_f32_16x16x32_f16(A, TBh, cv, 0, 0, 0);
#else
                    cv[0] = (float)A[0]; cv[1] = (float)A[2]; cv[2] = (float)A[5]; cv[3] = (float)A[7];
#endif
                    // cv[r]: output row l16, position 4q + r of the block; ONE f16 each, rounded to nearest (v_cvt_pk_f16_f32)
                    xh[2 * hsel] = pkrtn(cv[0], cv[1]);
                    xh[2 * hsel + 1] = pkrtn(cv[2], cv[3]);
                }
                if (bi >= 1) {
                    const int t = u - 1, ti = bi - 1;
                    if (t < ntiles && ti < cnt) {   // wave-uniform
                        // x = X (mean - b - theta_1): the taps carry X, the accumulator starts at -X theta_1 - X (b - 128)
                        // (the centre pixels: columns 16t + l16 = positions 16t + 8 + l16, this lane's window rows)
                        const half8_t Ab = TM_PREFETCH ? Ab_now : *reinterpret_cast<const half8_t *>(colp + (16 * ti + 8) * TM_POS_PITCH);
                        const half8_t XH = as_half8(xh[0], xh[1], xh[2], xh[3]);
#ifndef TM_DBG_NOMFMA
                        // (the preset ahead of the block's column pass, two independent MFMAs in flight: 232 against 226 us, dropped)
                        f32x4 c2 = __builtin_amdgcn_mfma_f32_16x16x32_f16(Ab, BID, K_LO, 0, 0, 0);
                        c2 = __builtin_amdgcn_mfma_f32_16x16x32_f16(THh[hsel], XH, c2, 0, 0, 0);
#else
                        f32x4 c2 = K_LO;
                        c2[0] += (float)XH[0] + (float)Ab[0]; c2[1] += (float)XH[2]; c2[2] += (float)XH[4]; c2[3] += (float)XH[6];
#endif
                        // c2[r] = x at output COLUMN 16t + 4q + r, row l16: x = X (v - theta_1) for the FIRST level, the one whose clear bit
                        // implies the other's (launch()); negative <=> the level's class bit is set.  v_cvt_pk_bf8_f32 packs two x into two
                        // bytes sign | 5 exponent bits | 2 mantissa bits: bit 7 IS the class bit, and bit 6 -- the exponent's top bit --
                        // is set exactly when |x| rounds to 2 or more, i.e. when v is EPS = 1.875 / |X| or more away from the level
                        // (decided).  Two instructions per four pixels (round 4: eight v_cvt_pk_u8_f32 and four adds for the two levels).
                        uint32_t f1 = (uint32_t)__builtin_amdgcn_cvt_pk_bf8_f32(c2[0], c2[1], 0, false);
                        f1 = (uint32_t)__builtin_amdgcn_cvt_pk_bf8_f32(c2[2], c2[3], (int)f1, true);
                        // Most tiles hold background only: every pixel of every lane decided and clear at the first level, hence at
                        // the second -- class 0, nothing to list -- and the second level is not evaluated at all (wave-uniform)
                        uint32_t cb = 0u;
                        const bool calm = (f1 & 0xC0C0C0C0u) == 0x40404040u;
                        if (EPS_MODE == 2 || __builtin_amdgcn_ballot_w64(!calm) != 0ull) {
                            uint32_t f2 = (uint32_t)__builtin_amdgcn_cvt_pk_bf8_f32(c2[0] + P.d2, c2[1] + P.d2, 0, false);
                            f2 = (uint32_t)__builtin_amdgcn_cvt_pk_bf8_f32(c2[2] + P.d2, c2[3] + P.d2, (int)f2, true);
                            cb = ((f1 >> P.sh1) & P.k1) | ((f2 >> P.sh2) & P.k2);
                            // (the levels are dozens of x-units apart: at most one of a pixel's two bytes is undecided)
                            uint32_t amb = ~(f1 & f2) & 0x40404040u;
                            if (EPS_MODE == 2) amb = 0x40404040u;          // diagnostic build: every pixel takes the exact path
                            if (__builtin_expect(__builtin_amdgcn_ballot_w64(amb != 0u) != 0ull, 0)) {
                                const int lc = opaque_lane(lane), l16 = lc & 15, q = lc >> 4;      // (cold)
                                const int y = oy + l16;
                                if (amb != 0u && y < it.y1) {
#pragma unroll
                                    for (int r = 0; r < 4; ++r) {
                                        const int x = it.x0 + 16 * t + 4 * q + r;
                                        if (((amb >> (8 * r)) & 0xFFu) && x < it.x1) {
                                            const uint32_t slot = atomicAdd(&L.n_list, 1u);
                                            if (slot < (uint32_t)TM_LIST_CAP) { L.list[slot] = ((uint32_t)y << 16) | (uint32_t)x; L.list_f[slot] = (uint16_t)it.f; }
                                        }
                                    }
                                }
                            }
                        }
                        // 1 row x 4 columns per lane: one dword of the wave's staging rows
                        *reinterpret_cast<uint32_t *>(wout + 16 * ti) = cb;
                    }
                }
                // The second half of the waves (two per SIMD) ask for the gray rows of step s + 2 HERE, in the middle of their tiles,
                // the first half at the step's start: sixteen waves' LDS-DMA instructions at one point of the step queue for ~600
                // cycles each while every SIMD waits for its first wave to get through (profiles/r04_thr_stamps.log)
                if (bi == TM_DMA_AFTER_BLOCK && late_dma) mine = request_raw(s + 2);     // (wave-uniform)
                if (bi & 1) __builtin_amdgcn_sched_barrier(0);
            }
        };
        // the wave's 16 rows x 80 bytes leave as 16-byte pieces: piece = (row, 16 columns)
        // (which 16-byte piece of its 16 rows x 80 bytes a lane stores does not change along the walk either)
        // TM_STORE_ROWS (round 5, an experiment switch): the step's sixteen WHOLE rows leave behind the step's first barrier,
        // where every wave's staging bytes are visible to every wave: 16 x 77 sixteen-byte pieces in row order = 20 store
        // instructions per step for the workgroup instead of the 32 that sixteen waves' private 16 x 80-byte blocks take
        // (two each, the second a quarter full), each writing 1 KB of ONE row.
        constexpr int ST_ITERS = TM_STORE_ROWS ? (TM_ROWS * TM_MAX_TILES + 64 * TM_WAVES - 1) / (64 * TM_WAVES) : (TM_ROWS * TM_PER_WAVE + 63) / 64;
        int st_lds[ST_ITERS], st_g[ST_ITERS];
        bool st_full[ST_ITERS], st_part[ST_ITERS];
        auto st_piece = [&](int k, int &r, int &x) __attribute__((always_inline)) {
            if (TM_STORE_ROWS) {
                const int pc = lane + 64 * (wave + TM_WAVES * k);        // piece = (row, 16-byte chunk of the panel's row)
                r = pc / ntiles;
                x = it.x0 + 16 * (pc - r * ntiles);
            } else {
                const int pc = lane + 64 * k;
                r = pc / TM_PER_WAVE;
                x = it.x0 + 16 * u0 + 16 * (pc - r * TM_PER_WAVE);
            }
        };
#pragma unroll
        for (int k = 0; k < ST_ITERS; ++k) {
            int r, x;
            st_piece(k, r, x);
            if (TM_STORE_ROWS) {
                const int chunk = (x - it.x0) >> 4;                      // whose staging block: wave chunk / 5, tile chunk % 5
                st_lds[k] = (chunk / TM_PER_WAVE) * (TM_ROWS * TM_OUT_PITCH) + r * TM_OUT_PITCH + 16 * (chunk % TM_PER_WAVE);
            } else st_lds[k] = r * TM_OUT_PITCH + (x - it.x0 - 16 * u0);
            st_g[k] = r * W + x;
            st_full[k] = r < TM_ROWS && it.x1 - x >= 16;
            st_part[k] = r < TM_ROWS && it.x1 - x > 0 && it.x1 - x < 16;      // (4, 8 or 12 bytes left in the row)
        }
        auto store_step = [&](int s) __attribute__((always_inline)) {
#ifdef TM_DBG_NOFILTER
            return;
#endif
            const int oy = it.y0 + TM_ROWS * (s - 1);
            const uint8_t *wout = reinterpret_cast<const uint8_t *>(TM_STORE_ROWS ? L.out[0] : L.out[wave]);
            const int rows = min(TM_ROWS, it.y1 - oy);                         // (below 16 in an item's last step only)
            uint8_t *base = dst + (size_t)oy * W;                              // (wave-uniform)
#pragma unroll
            for (int k = 0; k < ST_ITERS; ++k) {
                bool full = st_full[k], part = st_part[k];
                if (rows < TM_ROWS) {    // wave-uniform
                    int r, x;
                    st_piece(k, r, x);
                    full = full && r < rows; part = part && r < rows;
                }
#ifdef TM_DBG_NOSTORE
                full = full && lane == 77; part = false;
#endif
                if (full) {
                    const u32x4 v = *reinterpret_cast<const u32x4 *>(wout + st_lds[k]);
#ifdef TM_NT_STORES
                    __builtin_nontemporal_store(v, reinterpret_cast<u32x4 *>(base + st_g[k]));
#else
                    __builtin_memcpy(base + st_g[k], &v, 16);
#endif
                }
                if (__builtin_amdgcn_ballot_w64(part) != 0ull) {
                    if (part) {
                        int r, x;
                        st_piece(k, r, x);
                        const int nb = it.x1 - x;
                        const u32x4 v = *reinterpret_cast<const u32x4 *>(wout + st_lds[k]);
                        uint32_t *g4 = reinterpret_cast<uint32_t *>(base + st_g[k]);
                        g4[0] = v[0];
                        if (nb >= 8) g4[1] = v[1];
                        if (nb >= 12) g4[2] = v[2];
                    }
                }
            }
        };
        // The memory wave's form.  In this mode the class bytes of a step are staged as sixteen DENSE rows of 16 ntiles bytes (not a block
        // per wave), and leave row by row behind scalar bases: chunks 0 .. 63 of a row as one 1-KB instruction, the rows' tails
        // (chunks 64 .. and the 4-, 8- or 12-byte end of a row whose length is no multiple of 16) several rows per instruction.
        const int stage_pitch = 16 * ntiles;
        const int n_full = PW >> 4, rem = PW & 15;                         // whole 16-byte chunks of a row; bytes behind them
        const int head = min(64, n_full);
        const int tail_c0 = n_full > 64 ? 64 : n_full, tail_n = (n_full > 64 ? n_full - 64 : 0) + (rem ? 1 : 0);    // at most 14 chunks
        static_assert(TM_MAX_TILES - 64 + 1 <= 16, "a row's tail");
        auto store_rows = [&](int s) __attribute__((always_inline)) {
#if defined(TM_DBG_NOFILTER) || defined(TM_DBG_NOSTORE)
            return;
#endif
            const int oy = it.y0 + TM_ROWS * (s - 1);
            const int rows = min(TM_ROWS, it.y1 - oy);                         // (below 16 in an item's last step only)
            uint8_t *base = dst + (size_t)oy * W + it.x0;                      // (wave-uniform)
            const uint8_t *stage = reinterpret_cast<const uint8_t *>(L.out);
            const uint32_t l16b = 16u * (uint32_t)opaque_lane(lane);
            // heads.  A full step of a panel of 64 chunks or more: eight rows at a time in straight-line code -- eight LDS reads (a
            // lane's address += the staging pitch), then the eight stores as their data arrives (a lane's offset += W); 16 bytes
            // per lane behind a scalar base.  (The compiler's version of the loop below gave every store a basic block of its own,
            // two v_readlane for a spilled row base and a 64-bit address add: 130 cycles per store at priority 3.)
            if (head == 64 && rows == TM_ROWS) {   // wave-uniform
                uint32_t la = (uint32_t)(uintptr_t)stage + l16b, go = l16b;
#pragma unroll
                for (int r0 = 0; r0 < TM_ROWS; r0 += 8) {
                    u32x4 t0, t1, t2, t3, t4, t5, t6, t7;
                    asm volatile("ds_read_b128 %0, %8\n\tv_add_u32 %8, %10, %8\n\tds_read_b128 %1, %8\n\tv_add_u32 %8, %10, %8\n\t"
                                 "ds_read_b128 %2, %8\n\tv_add_u32 %8, %10, %8\n\tds_read_b128 %3, %8\n\tv_add_u32 %8, %10, %8\n\t"
                                 "ds_read_b128 %4, %8\n\tv_add_u32 %8, %10, %8\n\tds_read_b128 %5, %8\n\tv_add_u32 %8, %10, %8\n\t"
                                 "ds_read_b128 %6, %8\n\tv_add_u32 %8, %10, %8\n\tds_read_b128 %7, %8\n\tv_add_u32 %8, %10, %8\n\t"
                                 "s_waitcnt lgkmcnt(7)\n\tglobal_store_dwordx4 %9, %0, %11\n\tv_add_u32 %9, %12, %9\n\t"
                                 "s_waitcnt lgkmcnt(6)\n\tglobal_store_dwordx4 %9, %1, %11\n\tv_add_u32 %9, %12, %9\n\t"
                                 "s_waitcnt lgkmcnt(5)\n\tglobal_store_dwordx4 %9, %2, %11\n\tv_add_u32 %9, %12, %9\n\t"
                                 "s_waitcnt lgkmcnt(4)\n\tglobal_store_dwordx4 %9, %3, %11\n\tv_add_u32 %9, %12, %9\n\t"
                                 "s_waitcnt lgkmcnt(3)\n\tglobal_store_dwordx4 %9, %4, %11\n\tv_add_u32 %9, %12, %9\n\t"
                                 "s_waitcnt lgkmcnt(2)\n\tglobal_store_dwordx4 %9, %5, %11\n\tv_add_u32 %9, %12, %9\n\t"
                                 "s_waitcnt lgkmcnt(1)\n\tglobal_store_dwordx4 %9, %6, %11\n\tv_add_u32 %9, %12, %9\n\t"
                                 "s_waitcnt lgkmcnt(0)\n\tglobal_store_dwordx4 %9, %7, %11\n\tv_add_u32 %9, %12, %9"
                                 : "=&v"(t0), "=&v"(t1), "=&v"(t2), "=&v"(t3), "=&v"(t4), "=&v"(t5), "=&v"(t6), "=&v"(t7), "+v"(la), "+v"(go)
                                 : "s"(stage_pitch), "s"(base), "s"(W)
                                 : "memory");
                }
            } else {
#pragma unroll 1
                for (int r0 = 0; r0 < TM_ROWS; r0 += 4) {
                    u32x4 v[4];
                    if (lane < head) {
#pragma unroll
                        for (int e = 0; e < 4; ++e) v[e] = *reinterpret_cast<const u32x4 *>(stage + (r0 + e) * stage_pitch + l16b);
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            if (r0 + e < rows) __builtin_memcpy(base + (size_t)(r0 + e) * W + l16b, &v[e], 16);       // (wave-uniform test)
                    }
                }
            }
            // tails: at most four instructions' worth of rows (64 / tail_n >= 4 rows each), their reads first
            if (tail_n) {   // wave-uniform
                // rows per tail instruction: 64 / tail_n, by table (tail_n <= 16)
                const int tail_rows = tail_n <= 4 ? TM_ROWS : (int)((0x4444556789AC0000ull >> (4 * (tail_n - 1))) & 15ull);
                const uint32_t tail_recip = (uint32_t)(65536.0f / (float)tail_n) + 2u;       // lane / tail_n for lanes < 64
                const int tr = (int)(((uint32_t)lane * tail_recip) >> 16), ti = lane - tr * tail_n;
                const bool t_on = tr < tail_rows;
                const bool t_part = rem != 0 && ti == tail_n - 1;
                const uint32_t t_lds = (uint32_t)(tr * stage_pitch + 16 * (tail_c0 + ti)), t_g = (uint32_t)(tr * W + 16 * (tail_c0 + ti));
                u32x4 v[4];
                if (t_on) {
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        if (k * tail_rows < rows) v[k] = *reinterpret_cast<const u32x4 *>(stage + k * tail_rows * stage_pitch + t_lds);   // (wave-uniform test; the last lanes' rows may lie beyond the step's: not stored)
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const int g0 = k * tail_rows;
                        if (g0 < rows && g0 + tr < rows) {
                            uint8_t *g = base + (size_t)g0 * W + t_g;
                            if (!t_part) __builtin_memcpy(g, &v[k], 16);
                            else {
                                uint32_t *g4 = reinterpret_cast<uint32_t *>(g);
                                g4[0] = v[k][0];
                                if (rem >= 8) g4[1] = v[k][1];
                                if (rem >= 12) g4[2] = v[k][2];
                            }
                        }
                    }
                }
            }
        };
        auto blur_any = [&](int j) __attribute__((always_inline)) {
            if (j & 1) blur_step(j, std::integral_constant<int, 1>{}, std::false_type{});
            else blur_step(j, std::integral_constant<int, 0>{}, std::false_type{});
        };

        // ---- the walk ------------------------------------------------------------------------------------------------
        // vmcnt retires DMA and stores together, in issue order.  A step needs the gray rows requested ONE step ago, so it
        // waits until only the DMA instructions it has just issued itself are outstanding -- the class-map stores go out after
        // that wait and are never waited for inside the walk (round 3 waited vmcnt(0) at every step's second barrier: the
        // stores' round trip to HBM, twice per 16 rows).
        auto wait_all_but = [&](int n) __attribute__((always_inline)) {      // n: wave-uniform
            static_assert(TM_PIECES_PER_WAVE <= 3, "counted wait");
            if (n <= 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            else if (n == 1) asm volatile("s_waitcnt vmcnt(1)" ::: "memory");
            else if (n == 2) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
            else asm volatile("s_waitcnt vmcnt(3)" ::: "memory");
        };
#if !defined(TM_PRIO_FLAT) && !defined(TM_PRIO4) && !defined(TM_PRIO4R)
        // The second-dispatched half of the waves (two per SIMD) issues ahead of the first: with equal priorities the four waves
        // of a SIMD reach every memory instruction and every barrier of a step together; with two of them preferred the pairs
        // drift half a phase apart and one pair's stalls meet the other pair's arithmetic (241 -> 228 us per 256 frames;
        // four levels or the older half preferred: 232 / 245, profiles/r05_ab_thr_priority.log)
        if (wave >= TM_WAVES / 2) __builtin_amdgcn_s_setprio(1);
#elif defined(TM_PRIO4)
        if ((wave >> 2) == 1) __builtin_amdgcn_s_setprio(1); else if ((wave >> 2) == 2) __builtin_amdgcn_s_setprio(2); else if ((wave >> 2) == 3) __builtin_amdgcn_s_setprio(3);
#elif defined(TM_PRIO4R)
        if ((wave >> 2) == 2) __builtin_amdgcn_s_setprio(1); else if ((wave >> 2) == 1) __builtin_amdgcn_s_setprio(2); else if ((wave >> 2) == 0) __builtin_amdgcn_s_setprio(3);
#endif
        request_raw(-1);
        request_raw(0);
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
        blur_step(-1, std::integral_constant<int, 1>{}, std::true_type{});                                       // row sums of the sixteen gray rows above the first block
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
        if (nblk >= 1) request_raw(1);
        blur_any(0);
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
        if constexpr (TM_MEM_WAVE) {
            const bool is_mem = wave == TM_WAVES - 1;
            // The memory wave issues AHEAD of the others: at equal priority each of its instructions waits its turn behind three
            // waves' MFMAs -- 260 - 1 000 cycles per memory instruction beside busy waves, 20 - 40 at priority 3
            // (scripts/ubench/vmem_issue.hip, profiles/r05_vmem_issue.log)
#ifndef TM_MEM_PRIO_FLAT
            if (is_mem) __builtin_amdgcn_s_setprio(3);
#endif
            for (int s = 0; s <= nblk; ++s) {
                int n_dma = 0, unused = 0;
#ifndef TM_NO_FRESH
                // The per-block tests (is this block / tile inside the panel, is it this wave's) are scalar comparisons of these three.
                // Left to itself the compiler works all of them out once per item and keeps each as a 64-bit mask: dozens of scalar
                // register pairs, spilled to vector-register lanes and fetched with two v_readlane per test inside the walk.  Opaque here,
                // they are compared where they are used (two scalar instructions, no storage).
                asm volatile("" : "+s"(ntiles), "+s"(cnt), "+s"(u0));
#endif
                TMSTAMP(s, 0);
                if (is_mem && s + 2 <= nblk) n_dma = request_all(s + 2);       // (into the buffer the blur of step s has finished with)
                TMSTAMP(s, 1);
                if (s >= 1 && cnt > 0) filter_step(s, false, unused);
                TMSTAMP(s, 2);
                // the rows of step s + 1 have landed, and every older store has retired (vmcnt counts in issue order)
                if (is_mem) {
                    wait_all_but_n(n_dma);
                    if (s >= 1 && s + 1 <= nblk) side_patch(s + 1);
                }
                TMSTAMP(s, 3);
                TMSTAMP(s, 4);
                asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
                // (every wave's class bytes of the step are in LDS: the rows leave, and stay in flight through the next filter)
                if (is_mem && s >= 1) store_rows(s);
                TMSTAMP(s, 5);
                if (s + 1 <= nblk && cnt > 0) blur_any(s + 1);           // overwrites the tile block of step s - 1
                TMSTAMP(s, 6);
                asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
                TMSTAMP(s, 7);
            }
        } else {
        for (int s = 0; s <= nblk; ++s) {
                int mine = 0;
                TMSTAMP(s, 0);
    #ifdef YSMR_STAMPS
                // (the shader clock under this kernel's own load: s_memrealtime counts at a constant 100 MHz)
                if (blockIdx.x == TM_ST_BLOCK && lane == 0 && wave == 0 && (s == 3 || s == 13)) {
                    unsigned long long rt;
                    asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(rt) :: "memory");
                    g_tm_stamps[1][s == 3 ? 18 : 19][0] = rt;
                    g_tm_stamps[1][s == 3 ? 18 : 19][1] = __builtin_amdgcn_s_memtime();
                }
    #endif
                // The class bytes of step s - 1 leave at the START of step s (they wait in the wave's staging rows, which only this
                // step's tiles overwrite): a wave that stalls on its store instructions here stalls while the other waves of its SIMD
                // have tiles to filter; behind the filter (round 4) the stall of the LAST wave to finish was the phase's last 540 - 880
                // cycles, with every other wave already at the barrier (profiles/r05_thr_stamps_*.log).
                if (!TM_STORE_ROWS && TM_STORE_AT_START && s >= 2) store_step(s - 1);
                // (into the buffer the blur of step s has finished with; half of the waves ask later, inside filter_step)
                const bool late_dma = TM_DMA_AFTER_BLOCK >= 0 && s >= 1 && s + 2 <= nblk && wave >= TM_WAVES / 2;
                if (s + 2 <= nblk && !late_dma) mine = request_raw(s + 2);
                TMSTAMP(s, 1);
                if (s >= 1) filter_step(s, late_dma, mine);
                TMSTAMP(s, 2);
                wait_all_but(__builtin_amdgcn_readfirstlane(mine));  // the rows of step s + 1 have landed (and every older store)
                TMSTAMP(s, 3);
                if (!TM_STORE_ROWS && !TM_STORE_AT_START && s >= 1) store_step(s);
                TMSTAMP(s, 4);
                asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
                if (TM_STORE_ROWS && s >= 1) store_step(s);        // (every wave's class bytes of the step are in LDS: whole rows leave)
                TMSTAMP(s, 5);
                if (s + 1 <= nblk) blur_any(s + 1);           // overwrites the tile block of step s - 1
                TMSTAMP(s, 6);
                asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
                TMSTAMP(s, 7);
            }
            if (!TM_STORE_ROWS && TM_STORE_AT_START && nblk >= 1) store_step(nblk);
    
        }

        // ---- an item whose ambiguous pixels outgrew the list (a frame made to sit on the levels): all of it again, exactly ----
        const uint32_t n_now = L.n_list;
        if (__builtin_expect(n_now > (uint32_t)TM_LIST_CAP, 0)) {
            asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");          // (the item's own stores lie under these bytes)
            const int npx = PW * (it.y1 - it.y0);
            for (int p0 = 0; p0 < npx; p0 += TM_THREADS / 16) {
                const int p = min(p0 + (tid >> 4), npx - 1);
                const int y = it.y0 + p / PW, x = it.x0 + p % PW;
                const uint32_t c = exact_class(frame, P, y, x, lane, reinterpret_cast<uint8_t *>(L.out) + 256 * (tid >> 4));
                if (p0 + (tid >> 4) < npx && l16 == 0) dst[(size_t)y * W + x] = (uint8_t)c;
            }
            asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
            if (tid == 0) L.n_list = n_kept;                  // (what the earlier items of this workgroup listed stays)
            asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
        } else n_kept = n_now;
    }

    // ---- ambiguous pixels of all of this workgroup's items: cv2's own arithmetic, sixteen lanes per pixel -----------------
    // (once per workgroup: the code is cold, its first pixel costs microseconds of instruction fetch)
#ifdef TM_DBG_NOREFINE
    n_kept = 0;
#endif
    if (__builtin_expect(n_kept != 0u, 0)) {
        asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");              // the walk's stores lie under these bytes
        for (uint32_t e0 = 0; e0 < n_kept; e0 += TM_WAVES) {          // a pixel per wave
            const uint32_t e = e0 + (uint32_t)wave;
            const uint32_t ent = L.list[min(e, n_kept - 1)];
            const size_t fo = (size_t)L.list_f[min(e, n_kept - 1)] * H * W;
            const int y = (int)(ent >> 16), x = (int)(ent & 0xFFFFu);
            const uint32_t c = exact_class_wave(frames + fo, P, y, x, lane, reinterpret_cast<uint8_t *>(L.out) + 768 * wave);
            if (e < n_kept && lane == 0) cls[fo + (size_t)y * W + x] = (uint8_t)c;
        }
    }
}

}  // namespace

#ifdef YSMR_STAMPS
extern "C" int ysmr_debug_read_thr_stamps(unsigned long long *out) { return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_tm_stamps), sizeof(g_tm_stamps)); }
#endif

namespace ysmr_thr {

size_t lds_bytes() { return sizeof(Lds); }

int launch(hipStream_t st, const uint8_t *frames, uint8_t *cls, int batch, int H, int W, int inv, int t_low, int t_high,
           int use_high, const float *gauss11, const detect_plan::MfmaShape &shape, int variant, hipEvent_t ev_start, hipEvent_t ev_stop)
{
    // (a -DTM_MAX_PANEL_N build of this file alone: the plan was made for wider panels than this kernel's LDS holds)
    if (shape.panel_w > TM_MAX_PANEL)
        return ysmr::fail(YSMR_ERR_ARG, "panels of %d columns, the matrix-pipe threshold kernel was built for %d", shape.panel_w, TM_MAX_PANEL);
    // the scale search (detect_plan.h: choose_scales) once per set of taps
    static std::mutex mu;
    static float key[6] = {0, 0, 0, 0, 0, 0};
    static detect_plan::Scales cached{0.0, 0.0, 0.0};
    detect_plan::Scales sc;
    {
        std::lock_guard<std::mutex> lk(mu);
        if (!(cached.S > 0.0 && !std::memcmp(key, gauss11, sizeof(key)))) {
            cached = detect_plan::choose_scales(gauss11);
            std::memcpy(key, gauss11, sizeof(key));
        }
        sc = cached;
    }
    if (!(sc.S > 0.0)) return ysmr::fail(YSMR_ERR_ARG, "the matrix-pipe threshold kernel found no admissible scale for these taps");
    const detect_plan::LevelConsts c = detect_plan::level_consts(sc, inv, t_low, t_high, use_high, variant);
    Params P{};
    P.H = H; P.W = W; P.batch = batch;
    P.panels = shape.panels; P.panel_w = shape.panel_w; P.by_xcd = shape.by_xcd; P.start_rows = shape.start_rows;
    P.inv = inv; P.use_high = use_high; P.t_low = t_low; P.t_high = use_high ? t_high : t_low;
    for (int i = 0; i < 6; ++i) P.kw[i] = gauss11[i];
    P.col_scale = c.col_scale; P.row_scale = c.row_scale;
    P.neg_x_mul = c.neg_x_mul; P.k_first = c.k_first; P.d2 = c.d2;
    P.sh1 = c.sh1; P.k1 = c.k1; P.sh2 = c.sh2; P.k2 = c.k2;
    auto kern = variant == 2 ? k_threshold_mfma<2> : k_threshold_mfma<0>;
    YSMR_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(Lds)));
    ysmr::launch(kern, dim3(shape.grid), dim3(TM_THREADS), sizeof(Lds), st, ev_start, ev_stop, frames, cls, P);
    YSMR_LAUNCH_CHECK();
    return YSMR_OK;
}

}  // namespace ysmr_thr

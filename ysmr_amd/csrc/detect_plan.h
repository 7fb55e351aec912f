// detect_plan.h -- the host-only part of detection (detect.hip, thr_mfma.hip, meangray.hip): the constants host and kernels
// share, the geometry every entry point accepts, the layout of the workspace, which threshold kernel serves a launch and with
// what shape and grid, the scales that make the matrix-pipe kernel exact, and the grids of the labelling chain and of the
// mean-gray branch.  Plain C++17 with no HIP in it: tests/detect_plan_check.cc compiles it alone, under the host sanitizers.
// The knobs' values (YSMR_TUNING, the environment) are read in detect.hip and passed in; a constant that only a kernel reads
// stays beside that kernel.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "hd.h"
#include "ysmr_hip.h"      // the cv_flavour bits

namespace detect_plan {

// ---- constants -------------------------------------------------------------------------------------------------------
constexpr int CU_COUNT = 256;                // compute units: one workgroup of the matrix-pipe kernel each
constexpr int TW = 64, TH = 32;              // k_threshold: output tile per 256-thread block
constexpr int STRIP_HALO_LANES = 3;
constexpr int STRIP_MAX_OUT_LANES = 64 - 2 * STRIP_HALO_LANES;   // 58 lanes = 232 columns
// k_threshold_strip, k_level_strip: 3 blocks per CU (105 / 111 VGPRs, allocated as 112): a wave slot and 176 VGPRs per
// SIMD stay free for the link kernel's waves
constexpr int STRIP_RESIDENT = 768;
#ifndef TM_MAX_PANEL_N
#define TM_MAX_PANEL_N 1232
#endif
#ifndef TM_START_ROWS_N
#define TM_START_ROWS_N 48
#endif
constexpr int TM_START_ROWS = TM_START_ROWS_N;               // what an item's start costs, in rows of the walk (swept: profiles/r04_thr_start_rows.log)
constexpr int TM_MAX_PANEL = TM_MAX_PANEL_N;                 // columns per panel, a multiple of 16 (1232: 77 tiles of 16)

constexpr int NR_STRIDE = 32;                // ints between per-frame counters
constexpr int SHARED_COUNTERS = 8;           // words behind them: n_holed, arena_used, k_residue's barrier, max_roots, four spare
constexpr int HOLED_CAP = 4096;
constexpr int WIN_CORE = 32;
#ifndef WIN_GROUP_N
#define WIN_GROUP_N 8
#endif
constexpr int WIN_GROUP = WIN_GROUP_N;       // cores per work item, side by side (4, or 8: round 5)
constexpr int CLEAR_BLOCKS = 512;
// k_windows' resident grid: 4 blocks per CU.  The kernel's own time hardly depends on it (1536 .. 2560 blocks: 62 .. 66 us), but
// every block holds 10 KB of LDS, and with 8 per CU only one of k_frame's 59 KB blocks fits next to them
// (scripts/sweep_e2e_blocks.sh: end to end 83.7 k frames/s with 2048 blocks here and 1536 in k_geometry, 85.7 k
// with 1024 and 512).
#ifndef WINDOW_BLOCKS_N
#define WINDOW_BLOCKS_N 1024
#endif
constexpr int WINDOW_BLOCKS = WINDOW_BLOCKS_N;
#ifndef WINDOW_BLOCKS_FREE_N
#define WINDOW_BLOCKS_FREE_N 8192
#endif
constexpr int WINDOW_BLOCKS_FREE = WINDOW_BLOCKS_FREE_N;   // k_windows' grid where no per-frame link kernel runs beside it
constexpr int RANK_THREADS = 1024;
constexpr int RESIDUE_BLOCKS = 128;
#ifndef RESF_MIN_BATCH_N
#define RESF_MIN_BATCH_N 8
#endif
constexpr int RESF_MIN_BATCH = RESF_MIN_BATCH_N;
constexpr int NEST_BLOCKS = 128;
constexpr int GEO_BLOCKS = 512;

constexpr int MG_BLOCKS = 1024;
constexpr int LEVEL_SEG = 32;                // output rows per thread item of k_level_threshold
constexpr int LSTRIP_OUT_LANES = 62;

// Tuning knobs: resident grid sizes of the detection kernels and the strip kernel's segment height; values <= 0 keep the
// defaults (detect.hip: knobs()).
struct Knobs {
    int seg_h, thr_blocks, collect_blocks, sparse_blocks, clear_blocks, geo_blocks;
};

// ---- the geometry every entry point accepts (common.hip: check_geometry has the messages) -----------------------------
enum class Bad { none, positive, channels, too_large };
inline Bad check_geometry(int batch, int H, int W, int channels, int max_det)
{
    if (batch <= 0 || H <= 0 || W <= 0 || max_det <= 0) return Bad::positive;
    if (channels != 1 && channels != 3) return Bad::channels;
    if (H > 16384 || W > 16384 || (size_t)batch * H * W > (1ull << 32) - 64) return Bad::too_large;
    return Bad::none;
}

// ---- k_windows' work items: WIN_GROUP cores side by side -------------------------------------------------------------
struct WinItems { int groups_x, rows_y; long long per_frame, items; };
YSMR_HD_FORCE WinItems win_items(int batch, int H, int W)
{
    constexpr int SPAN = WIN_GROUP * WIN_CORE;   // 256
    const int groups_x = (W + SPAN - 1) / SPAN, rows_y = (H + WIN_CORE - 1) / WIN_CORE;
    const long long per_frame = (long long)groups_x * rows_y;
    return WinItems{groups_x, rows_y, per_frame, per_frame * batch};
}

// ---- the workspace: ONE device allocation, carved in steps of 256 bytes -----------------------------------------------
// Byte offsets of the regions, in the order they lie.  The counter block is batch * NR_STRIDE per-frame counters and
// SHARED_COUNTERS words behind them, given as int32 indices from `counters`; k_clear zeroes all `n_counters` in one go.
struct Layout {
    size_t hdr;          // WsHeader, 256 bytes: persists across calls (ysmr_detect_workspace_init zeroes it)
    size_t counters, prev_n, pixels, holed, roots, order, bbox, euler4, nested, bbox_tmp, euler_tmp, det_tmp;
    size_t arena;        // scratch shared by k_geometry (hulls wider than the LDS fast path) and its nesting workgroups
                         // (windows larger than LDS): room for 16 full-width hulls per frame, and at least one full-frame window
    size_t oldbits;      // k_windows' words for the next call's clearing: per work item 32 rows x WIN_GROUP words
    size_t total;
    size_t n_holed, arena_used, barrier, max_roots;
    int n_counters;
    uint32_t pixel_cap, arena_floats;
    size_t oldbits_words;
};

inline Layout layout(int batch, int H, int W, int max_det)
{
    Layout l{};
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t o = off; off = (off + bytes + 255) / 256 * 256; return o; };
    const size_t bm = (size_t)batch * max_det;
    l.hdr = take(256);
    l.n_holed = (size_t)batch * NR_STRIDE;
    l.arena_used = l.n_holed + 1;
    l.barrier = l.n_holed + 2;
    l.max_roots = l.n_holed + 3;
    l.n_counters = (int)(l.n_holed + SHARED_COUNTERS);
    l.counters = take(sizeof(int32_t) * (l.n_holed + SHARED_COUNTERS));
    l.prev_n = take(sizeof(int32_t) * (size_t)batch);
    l.pixel_cap = (uint32_t)(((size_t)batch * H * W + 7) / 8);
    l.pixels = take(sizeof(uint32_t) * l.pixel_cap);
    l.holed = take(2 * sizeof(int32_t) * HOLED_CAP);
    l.roots = take(sizeof(int32_t) * bm);
    l.order = take(sizeof(int32_t) * bm);
    l.bbox = take(sizeof(int32_t) * bm * 4);
    l.euler4 = take(sizeof(int32_t) * bm);
    l.nested = take(sizeof(int32_t) * bm);
    l.bbox_tmp = take(sizeof(int32_t) * bm * 4);
    l.euler_tmp = take(sizeof(int32_t) * bm);
    l.det_tmp = take(sizeof(float) * bm * 5);
    size_t arena_floats = (size_t)batch * std::max<size_t>(16 * 5 * (2 * (size_t)W + 3), ((size_t)(H + 2) * (W + 2) + 3) / 4);
    if (arena_floats > 0x7FFFFFFFull) arena_floats = 0x7FFFFFFFull;
    l.arena_floats = (uint32_t)arena_floats;
    l.arena = take(sizeof(float) * arena_floats);
    l.oldbits_words = (size_t)win_items(batch, H, W).items * WIN_CORE * WIN_GROUP;
    l.oldbits = take(sizeof(uint32_t) * l.oldbits_words);
    l.total = off;
    return l;
}

// ---- which threshold kernel, with what shape and grid ------------------------------------------------------------------
// workgroups of the matrix-pipe kernel under the caller's hints (ysmr_threshold_workgroups)
inline int threshold_workgroups(int cv_flavour)
{
    return (cv_flavour & YSMR_BESIDE_BATCH_LINK) ? 248 : ((cv_flavour & YSMR_BESIDE_SPLIT_LINK) ? 160 : CU_COUNT);
}

// geometry / arguments the matrix-pipe kernel serves (everything else stays on k_threshold_strip / k_threshold)
inline bool mfma_supported(int H, int W, int channels, int t_low, int t_high, int use_high)
{
    const int gap = use_high ? (t_high > t_low ? t_high - t_low : t_low - t_high) : 1;
    return channels == 1 && (W & 3) == 0 && W >= 64 && W <= 16384 && H >= 18 && H <= 16383 && gap >= 1 &&
           t_low > -1000 && t_low < 1000 && t_high > -1000 && t_high < 1000;
}

// a wave owns a vertical strip of `out_lanes` dwords of columns and `seg_h` rows of it: k_threshold_strip (StripParams
// without its levels and gray coefficients), k_level_strip (LevelStrip; never by_xcd)
struct StripShape {
    int out_lanes, strips_x, seg_h, segs_y;
    int by_xcd;            // frames are dealt to the 8 XCDs (needs batch % 8 == 0 and a grid that is a multiple of 8)
    unsigned blocks;
};
struct MfmaShape {
    int panels, panel_w;   // column panels of at most TM_MAX_PANEL columns (a multiple of 16 wide, the last one may be narrower)
    int by_xcd;
    int start_rows;        // the cost of starting an item, in rows of the walk (0: the workgroups divide the columns evenly)
    unsigned grid;
};
enum class Kernel { refused, mfma, strip, tile };
struct ThresholdPlan {
    Kernel kernel;
    int mfma_variant;      // thr_mfma.h: 0 = shipped, 1 = half the scale, 2 = every pixel through the exact path
    MfmaShape mfma;
    StripShape strip;
    unsigned tile_grid[3];
};

inline MfmaShape mfma_shape(int batch, int H, int W, int blocks_wanted, size_t mfma_lds)
{
    MfmaShape m{};
    m.panels = (W + TM_MAX_PANEL - 1) / TM_MAX_PANEL;
    m.panel_w = ((W + m.panels - 1) / m.panels + 15) & ~15;
    m.panels = (W + m.panel_w - 1) / m.panel_w;
    // every CU full; a build whose workgroups are small enough for several per compute unit (TM_WAVES_N = 8 with narrow panels: an
    // experiment of round 5) takes the caller's figure as compute units
    const int per_cu = (int)((160 * 1024) / mfma_lds);
    const int blocks = blocks_wanted * per_cu;
    // (no workgroup with fewer than 32 rows: an item re-filters 16 halo rows)
    const long long grid = std::max<long long>(1, std::min<long long>((long long)batch * m.panels * H / 32, blocks));
    m.by_xcd = (batch % 8 == 0 && grid % 8 == 0) ? 1 : 0;
    const long long groups = m.by_xcd ? 8 : 1, cols = (long long)(batch / groups) * m.panels, nb = grid / groups;
    m.start_rows = nb % cols == 0 ? 0 : TM_START_ROWS;
    m.grid = (unsigned)grid;
    return m;
}

inline StripShape strip_shape(int batch, int H, int W, const Knobs &kn)
{
    StripShape s{};
    const int quads = (W + 3) / 4;
    s.strips_x = (quads + STRIP_MAX_OUT_LANES - 1) / STRIP_MAX_OUT_LANES;
    s.out_lanes = (quads + s.strips_x - 1) / s.strips_x;
    const int resident = kn.thr_blocks > 0 ? kn.thr_blocks : STRIP_RESIDENT;
    // rows per work item: every item re-reads and re-filters 10 halo rows, so items are as tall as they can
    // be while there is still one for every resident wave (1228x922, 64 frames: 384 strip columns x 8
    // segments of 116 rows = 3072 items = 768 blocks x 4 waves; it was 45 rows, 2.6 items per wave); never
    // shorter than 32 rows
    const long long columns = (long long)batch * s.strips_x;
    const long long segs = std::max<long long>(1, (long long)resident * 4 / columns);
    s.seg_h = kn.seg_h > 0 ? kn.seg_h : (int)std::max<long long>(32, (H + segs - 1) / segs);
    s.segs_y = (H + s.seg_h - 1) / s.seg_h;
    const long long waves = columns * s.segs_y;
    long long blocks = std::min<long long>((waves + 3) / 4, resident);
    s.by_xcd = (batch % 8 == 0 && blocks % 8 == 0) ? 1 : 0;
    if (s.by_xcd && blocks / 8 * 4 > (long long)(batch / 8) * s.strips_x * s.segs_y)    // (no more waves than an XCD has items)
        blocks = (((long long)(batch / 8) * s.strips_x * s.segs_y + 3) / 4) * 8;
    s.blocks = (unsigned)blocks;
    return s;
}

// variant (ysmr_threshold_batch_variant): 0 = the shipped choice of kernel -- strip / tile beside the one-launch link
// (YSMR_BESIDE_LINK); 1 = strip / tile kernels only (bit-exact float32 chain for every pixel); 2, 3 = the matrix-pipe kernel's
// diagnostic builds, refused where it does not serve the geometry.  mfma_lds: the matrix-pipe kernel's LDS (thr_mfma.hip: Lds)
inline ThresholdPlan threshold_plan(int batch, int H, int W, int channels, int t_low, int t_high, int use_high, int cv_flavour,
                                    int variant, const Knobs &kn, size_t mfma_lds)
{
    ThresholdPlan p{};
    if (variant == 0 && (cv_flavour & YSMR_BESIDE_LINK)) variant = 1;
    if (variant != 1 && mfma_supported(H, W, channels, t_low, t_high, use_high)) {
        p.kernel = Kernel::mfma;
        p.mfma_variant = variant >= 2 ? variant - 1 : 0;
        p.mfma = mfma_shape(batch, H, W, kn.thr_blocks > 0 ? kn.thr_blocks : threshold_workgroups(cv_flavour), mfma_lds);
        return p;
    }
    if (variant >= 2) return p;      // Kernel::refused
    const int t_gap = use_high ? (t_high > t_low ? t_high - t_low : t_low - t_high) : 0;
    if ((W & 3) == 0 && W >= 16 && H >= 2 && t_low > -100000 && t_low < 100000 && t_high > -100000 && t_high < 100000 && t_gap <= 127) {
        p.kernel = Kernel::strip;
        p.strip = strip_shape(batch, H, W, kn);
    } else {
        p.kernel = Kernel::tile;
        p.tile_grid[0] = (unsigned)((W + TW - 1) / TW); p.tile_grid[1] = (unsigned)((H + TH - 1) / TH); p.tile_grid[2] = (unsigned)batch;
    }
    return p;
}

// ---- cv2.getGaussianKernel(11, 0): sigma 2, float32 ------------------------------------------------------------------
inline void gauss11(float *k)
{
    const double sigma = 0.3 * ((11 - 1) * 0.5 - 1.0) + 0.8;
    const double scale2x = -0.5 / (sigma * sigma);
    double t[11], sum = 0.0;
    for (int i = 0; i < 11; ++i) {
        double x = i - 5.0;
        t[i] = std::exp(scale2x * x * x);
        sum += t[i];
    }
    sum = 1.0 / sum;
    for (int i = 0; i < 11; ++i) k[i] = (float)(t[i] * sum);
}

// ---- the scales of the matrix-pipe kernel's arithmetic and its error bound ---------------------------------------------
// The walk evaluates  x = X (mean - b - theta_1), X = +-S,  with ONE f16 per tap and ONE f16 for the column-filtered value:
//   tile          b - 128, exact integers in [-128, 127]
//   column pass   v1 = sum_j f16(s w_j) (b_j - 128)            float32 accumulation of exact products
//   intermediate  h = f16(v1), round to nearest                 |h - v1| <= 2^-5 while |v1| < 128
//   row pass      x = sum_i f16(X / s  w_i) h_i + [-X theta_1 - X (b - 128)]
// against the real number  X (sum_ij w_i w_j b_ij - b - theta_1).  In gray levels (divide by S):
//   column taps   |sum_j (f16(s w_j) / s - w_j) (b_j - 128)|            <= 128 dc,   dc = sum_j |f16(s w_j) / s - w_j|
//   intermediate  (1 / s) sum_i w_i |h_i - v1_i|                        <= 2^-5 / s  (needs s 128 (1 + dc) sum w < 128)
//   row taps      |sum_i (f16(S / s w_i) / S - w_i / s) h_i|, |h_i| <= 128   <= 128 dr / s,   dr = sum_i |f16(S / s w_i) s / S - w_i|
//   accumulation  one float32 rounding per product, all lined up: 32 x 2^-18 (column pass, partial sums below 128) plus
//                 64 half-ulps at S x 384 (the two products of the row pass), over S
//   cv2 itself    its float32 chain is within 22 x 2^-24 x 255 of the real mean; its taps sum to 1 within 1e-8
// s and S are free: s is searched so that the eleven scaled weights lie close to f16 values (dc = 3.1e-5 at s = 0.9945 for
// cv2's sigma-2 kernel, against 2.1e-4 at s = 1), S -- an f16 value itself, it is a tap of the accumulator's preset --
// likewise, the largest whose 1.875 / S (where the bf8 conversion of x sets its exponent's top bit) covers 1.1 x the bound:
// S = 39.375, bound 0.0423, EPS = 1.875 / S = 0.0476 gray levels
// (scripts/sim/thr_single_f16.py is the same arithmetic in numpy, with the counts of undecided pixels it leaves).
struct Scales { double s, S, bound; };

inline double host_f16(double x)      // round to nearest even at 11 significant bits (normal range only: checked by walk_bound)
{
    if (x == 0.0) return 0.0;
    int e;
    const double m = std::frexp(x, &e);
    return std::ldexp(std::nearbyint(std::ldexp(m, 11)), e - 11);
}

inline double taps_error(const double *w11, double scale)
{
    double d = 0.0;
    for (int i = 0; i < 11; ++i) d += std::fabs(host_f16(w11[i] * scale) / scale - w11[i]);
    return d;
}

inline double walk_bound(const double *w11, double s, double S)
{
    double sum = 0.0;
    for (int i = 0; i < 11; ++i) sum += w11[i];
    const double dc = taps_error(w11, s), dr = taps_error(w11, S / s);
    if (!(s * 128.0 * (1.0 + dc) * sum < 128.0 * (1.0 - 1e-6))) return 1e30;        // the intermediate must stay below 128
    if (S / s * w11[5] > 60000.0 || s * w11[0] < 6.2e-5 || S / s * w11[0] < 6.2e-5) return 1e30;   // taps in f16's normal range
    const double acc = 32.0 * std::ldexp(1.0, -18) + 64.0 * std::ldexp(1.0, (int)std::floor(std::log2(S * 384.0)) - 24) / S;
    const double cv2 = 22.0 * std::ldexp(1.0, -24) * 255.0 + std::fabs(sum - 1.0) * 255.0;
    return 128.0 * dc + std::ldexp(1.0, -5) / s + 128.0 * dr / s + acc + cv2;
}

// gauss6: the Gaussian's distinct weights k[0..5] (k[i] == k[10 - i]).  S == 0: no admissible scale for these taps
inline Scales choose_scales(const float *gauss6)
{
    double w[11];
    for (int i = 0; i < 11; ++i) w[i] = (double)gauss6[i <= 5 ? i : 10 - i];
    Scales best{0.0, 0.0, 0.0};
    double best_score = 1e30;
    for (int k = 0; k < 2000; ++k) {
        const double s = 0.9 + 5e-5 * k;
        if (walk_bound(w, s, 1024.0) > 1e29) continue;
        const double score = 128.0 * taps_error(w, s) + std::ldexp(1.0, -5) / s;
        if (score < best_score) { best_score = score; best.s = s; }
    }
    if (best.s > 0.0)
        for (int k = 64 * 16; k >= 4 * 16; --k) {    // multiples of 1/16 below 64: f16 values, and so are their halves (the diagnostic variant)
            const double S = k / 16.0, E = walk_bound(w, best.s, S);
            if (1.1 * E <= 1.875 / S) { best.S = S; best.bound = E; break; }
        }
    return best;
}

// What the kernel takes of the scales and the levels (thr_mfma.h: Params has the fields' meaning).
// v = mean - b.  BINARY: bit = (b - m > t) <=> v < theta = -t - 0.5;  INV: bit = (b - m <= t) <=> v > theta (ties: exact path).
// x = X (v - theta) with X = +S (BINARY) / -S (INV) is negative exactly where the bit is set, and |x| >= 1.875 -- where its
// bf8 conversion has the exponent's top bit set -- exactly when v is 1.875 / S or more away from theta: S is the largest scale
// whose 1.875 / S still covers the error bound of the walk's arithmetic with a tenth to spare (choose_scales: S = 39.375,
// EPS = 0.0476 gray levels for cv2's sigma-2 taps; variant 1, diagnostic: half that scale, twice the list).
// The FIRST level is the one whose clear, decided bit implies the other's: the larger theta for BINARY, the smaller for INV;
// a tile in which it fires nowhere is class 0 throughout and never evaluates the second.  One level: the second = the first.
struct LevelConsts {
    float neg_x_mul, k_first, d2, col_scale, row_scale;
    uint32_t sh1, k1, sh2, k2;
};
inline LevelConsts level_consts(const Scales &sc, int inv, int t_low, int t_high, int use_high, int mfma_variant)
{
    const double S = mfma_variant == 1 ? sc.S / 2 : sc.S, X = inv ? -S : S;
    const double th_lo = -(double)t_low - 0.5, th_hi = use_high ? -(double)t_high - 0.5 : th_lo;
    const bool lo_first = inv ? th_lo <= th_hi : th_lo >= th_hi;
    const double th1 = lo_first ? th_lo : th_hi, th2 = lo_first ? th_hi : th_lo;
    LevelConsts c{};
    c.col_scale = (float)sc.s;
    c.row_scale = (float)(X / sc.s);
    c.neg_x_mul = (float)-X;
    c.k_first = (float)(-X * th1);
    c.d2 = (float)(X * (th1 - th2));
    c.sh1 = lo_first ? 7 : 6; c.k1 = lo_first ? 0x01010101u : 0x02020202u;
    c.sh2 = lo_first ? 6 : 7; c.k2 = lo_first ? 0x02020202u : 0x01010101u;
    return c;
}

// ---- the labelling chain's grids (ysmr_components_batch) ---------------------------------------------------------------
struct ChainPlan {
    unsigned clear, windows, rank_x, rank_y, geometry;      // k_geometry's: its own blocks and the NEST_BLOCKS in front of them
    bool residue_frames;                                    // k_residue_frames, a workgroup per frame; else k_residue
    unsigned residue;
};
// fused_max_det: tracker_plan.h's FUSED_MAX_DET, the largest table the one-launch link (k_frame) takes
inline ChainPlan chain_plan(int batch, int H, int W, int max_det, int cv_flavour, const Knobs &kn, int fused_max_det)
{
    ChainPlan c{};
    // (the LDS reserve matters to k_frame, the one-launch link, which tables of more than FUSED_MAX_DET detections do not use
    // and which the caller announces with YSMR_BESIDE_LINK)
    const bool small_tables = max_det <= fused_max_det && (cv_flavour & YSMR_BESIDE_LINK);
    // k_windows' grid.  Beside the per-frame link kernels (one-launch or split) it stays a RESIDENT grid that leaves them their LDS
    // and wave slots.  Beside the batch link -- one workgroup that has long been seated -- or with no link at all, a wave per work item
    // and the dispatcher hands the workgroups out as units become free: the work items differ (a core with twenty islands, a core
    // with none), and 2048 resident workgroups with 4.4 items per wave ended as late as the unluckiest of them (round 5, last hours:
    // 293 -> 267-270 us of labelling chain per 256 frames with 7168-8192 workgroups, scripts/sweep_window_blocks.sh; the link's
    // time does not change)
    const bool per_frame_link = (cv_flavour & (YSMR_BESIDE_LINK | YSMR_BESIDE_SPLIT_LINK)) != 0;
    const unsigned window_blocks = kn.collect_blocks > 0 ? (unsigned)kn.collect_blocks
                                   : (unsigned)(small_tables ? WINDOW_BLOCKS : (per_frame_link ? 2 * WINDOW_BLOCKS : WINDOW_BLOCKS_FREE));
    long long wblocks = std::min<long long>((win_items(batch, H, W).items + 3) / 4, window_blocks);
    if (wblocks >= 8) wblocks &= ~7ll;   // (a multiple of 8: the kernel deals its items to the XCDs)
    c.windows = (unsigned)wblocks;
    c.clear = kn.clear_blocks > 0 ? (unsigned)kn.clear_blocks : (unsigned)CLEAR_BLOCKS;
    c.residue_frames = batch >= RESF_MIN_BATCH;
    c.residue = c.residue_frames ? (unsigned)batch : (unsigned)RESIDUE_BLOCKS;
    c.rank_x = (unsigned)batch;
    c.rank_y = (unsigned)std::min((max_det + RANK_THREADS / 4 - 1) / (RANK_THREADS / 4), 32);
    c.geometry = (kn.geo_blocks > 0 ? (unsigned)kn.geo_blocks : (unsigned)(small_tables ? GEO_BLOCKS : 3 * GEO_BLOCKS)) + NEST_BLOCKS;
    return c;
}

// ---- the mean-gray branch (ysmr_mean_threshold_batch) --------------------------------------------------------------------
struct MeanPlan {
    int parts;             // k_gray_sums: parts per frame
    unsigned sum_blocks;
    bool strip;            // k_level_strip (W % 4 == 0, W >= 8, dword-aligned buffers); else k_level_threshold
    StripShape level;      // k_level_strip's
    int groups_x, segs_y;  // k_level_threshold's: a thread takes 4 columns x LEVEL_SEG rows
    unsigned thr_blocks;
};
inline MeanPlan mean_plan(int batch, int H, int W, bool dword_aligned)
{
    MeanPlan m{};
    const uint32_t HW = (uint32_t)H * (uint32_t)W;
    // k_gray_sums: enough parts per frame to fill the resident grid, each at least 4096 pixels
    int parts = (MG_BLOCKS + batch - 1) / batch;
    const int max_parts = (int)((HW + 4095u) / 4096u);
    m.parts = parts < 1 ? 1 : (parts > max_parts ? max_parts : parts);
    m.sum_blocks = (unsigned)std::min<long long>((long long)batch * m.parts, MG_BLOCKS);
    m.strip = (W & 3) == 0 && W >= 8 && dword_aligned;
    if (m.strip) {
        StripShape &s = m.level;
        const int quads = W / 4;
        s.strips_x = (quads + LSTRIP_OUT_LANES - 1) / LSTRIP_OUT_LANES;
        s.out_lanes = (quads + s.strips_x - 1) / s.strips_x;
        // rows per item: the tallest segment <= 64 rows for which the items fill the resident waves a whole
        // number of times (a last, nearly empty round costs as much as a full one)
        const long long columns = (long long)batch * s.strips_x;
        s.seg_h = 32;
        for (int k = 1; k <= 16; ++k) {
            const long long segs = (long long)k * STRIP_RESIDENT * 4 / columns;
            if (segs < 1) continue;
            const int h = (int)((H + segs - 1) / segs);
            if (h <= 64) { s.seg_h = h < 8 ? 8 : h; break; }
        }
        s.segs_y = (H + s.seg_h - 1) / s.seg_h;
        s.blocks = (unsigned)std::min<long long>((columns * s.segs_y + 3) / 4, STRIP_RESIDENT);
    } else {
        m.groups_x = (W + 3) / 4; m.segs_y = (H + LEVEL_SEG - 1) / LEVEL_SEG;
        m.thr_blocks = (unsigned)std::min<long long>(((long long)m.groups_x * m.segs_y * batch + 255) / 256, MG_BLOCKS);
    }
    return m;
}

}  // namespace detect_plan

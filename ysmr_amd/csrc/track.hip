// track.hip -- a7-a19 of the YSMR hot path on gfx950: CentroidTracker.update (ysmr/tracker.py:93-230)
// with the Gaussian-sum FIR filter (ysmr/gsff.py:204-347) and row emission
// (ysmr/track_eval.py:313-316), device-resident across frames.
//
// Per frame ONE launch, no host round trip (k_frame, the fused path): every workgroup recomputes the
// frame's bookkeeping in LDS (claim resolution, ageing / deregistration, stable compaction of the
// id-ordered table, registration in CPython set order), then each WAVE handles one track: GSFF
// correct + predict, the frame's output row, and the nearest detection of the NEXT frame -- the fused
// row-min / arg-min of the N x M float64 distance matrix, which is never stored (tracker.py:151-163
// only ever reads D.min(1), D.argmin(1)).  k_rowmin does that last step stand-alone for the first
// frame of a batch.  Configurations beyond the LDS budget of k_frame (max_det > FUSED_MAX_DET, very
// large capacity) run the same device functions as two launches: k_link (one workgroup) + k_track
// (one wave per track).
//
// Which of the five link paths a handle takes -- k_frame | k_link + k_track | k_link + k_track_lanes |
// k_batch | k_batch3 (batch_link.h) -- is decided in tracker_plan.h, host-only and tested without a
// device: qualifies() says what a configuration can run, link_of(caps, dims, link_mode) which one
// links.  Here the device may only clear a capability (a refused LDS size); every reader asks
// ysmr_tracker::link() / frame_link().  The state block's carving and every size are there too.
//
// Claim rule (tracker.py:158-189): proposals are visited in ascending (row minimum, row); a
// proposal is accepted iff its column is still free.  Each row occurs once, so the winner of a
// column is simply the proposer with the smallest (distance, row) -- resolved with two atomicMin
// rounds instead of a sort and a sequential loop.
//
// All arithmetic is float64 like the reference; -ffp-contract=off keeps mul/add unfused.
#include "common.h"
#include "set_order.h"
#include "tracker_plan.h"
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

struct DetGrid {
    const int *start;     // [GRID_CELLS + 1] first item of each cell (cells row-major: cy * GRID_N + cx)
    const int *items;     // [max_det] detection columns, cell by cell (any order inside a cell)
    const float *hdr;     // x0, y0, cell size, 1 / cell size
    const float2 *xy;     // [max_det] the centres of `items`, in the same order: a cell's candidates arrive with one round
                          // of loads instead of column numbers first and the detections they name after them
};

namespace plan = tracker_plan;

struct ysmr_tracker {
    TrackerDev d;      // view of parity 0
    TrackerDev d1;     // view of parity 1 (k_frame: small per-frame arrays are double-buffered)
    int par = 0;       // parity of the current state
    // tracker_plan.h: what the arguments of ysmr_tracker_create come to, and which link paths the handle can take (the
    // device may have cleared one: a refused LDS size).  link() says which one it takes
    plan::Config cfg;
    plan::Caps caps;
    int dims = 2;                  // ysmr_tracker_dimensions: 2 (x, y) or 3 (x, y, luminosity)
    int link_mode = 0;             // ysmr_tracker_link_mode
    bool in_batch = false;         // the state rests in the seat-major arrays of `bd` (else: the per-slot layout)
    bool linked = false;           // a frame has been linked since creation / the last reset: the dimension is fixed
    void *block = nullptr;         // the single device allocation
    size_t block_bytes = 0;
    std::vector<double> gains_host;
    void *grid_block = nullptr;    // two-launch paths: DetGrid arrays for grid_frames frames; batch link: k_bgrid's blocks
    int grid_frames = 0;           //   (allocated by ysmr_tracker_create: no allocation on the call path)
    BatchDev bd;                   // batch link (batch_link.h), and the filter state of k_track_lanes: seat-major by slot from the start
    const BlGains *bgains_dev = nullptr;     // cfg.bgains in device memory (behind the grid blocks): k_batch reads it frame by frame
    // ysmr_tracker_prepare: which batch each of the two caller-named grid blocks was binned for (block 2 is run's own)
    struct Prepared { const void *det = nullptr; const void *count = nullptr; const void *third = nullptr; int batch = 0; } prepared[2];
    int lanes_head = 0;            // k_track_lanes: the ring's head (every live track appends one measurement per frame)
    double *pos3 = nullptr;        // [capacity] third coordinate of the track in a slot
    // the batch link of a 3-D handle (batch_link.h: k_bgrid3 + k_batch3), on request only (link mode 2): its grid blocks -- a
    // larger stride than the 2-D ones, for the third coordinate's two planes -- and the seat-major third coordinate are
    // allocated when the mode is first selected on a 3-D handle, so a 2-D handle's footprint is what it was
    void *grid3_block = nullptr;   // [3][BL_MAX_BATCH][grid3_stride] bytes, then seat3 f64 [seat_cap]
    unsigned grid3_stride = 0;
    double *seat3 = nullptr;
    plan::Link link() const { return plan::link_of(caps, dims, link_mode); }      // how a `run` call is linked
    plan::Link frame_link() const { return plan::link_of(caps, dims, 1); }        // ... and a single frame (update; link mode 1)
    DetGrid grid(int f) const
    {
        char *b = (char *)grid_block;
        const size_t per = grid_bytes_per_frame(d.max_det);
        const size_t o_items = sizeof(int) * (GRID_CELLS + 64), o_hdr = o_items + sizeof(int) * (size_t)d.max_det;
        return DetGrid{(const int *)(b + per * f), (const int *)(b + per * f + o_items), (const float *)(b + per * f + o_hdr),
                       (const float2 *)(b + per * f + o_hdr + 64)};
    }
    const TrackerDev &cur() const { return par ? d1 : d; }
    const TrackerDev &nxt() const { return par ? d : d1; }
};


#ifdef YSMR_STAMPS
__device__ unsigned long long g_stamps[32];
#define GSTAMP(k) do { if (blockIdx.x == 1 && threadIdx.x == 0) { unsigned long long t_; asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_) :: "memory"); g_stamps[k] = t_; } } while (0)
__device__ unsigned long long g_block_stamps[2 * 2048 * 8];
#ifndef YSMR_BS_A
#define YSMR_BS_A 62   // frames (mod 64) whose per-block stamps are kept: slot 0 / slot 1
#define YSMR_BS_B 63
#endif
#define BSTAMP(k) do { const int fs_ = frame; if (threadIdx.x == 0 && (fs_ == YSMR_BS_A || fs_ == YSMR_BS_B)) { const int sl_ = fs_ == YSMR_BS_B; unsigned long long t_; asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_) :: "memory"); g_block_stamps[(sl_ * 2048 + blockIdx.x) * 8 + (k)] = t_; asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_) :: "memory"); g_block_stamps[(sl_ * 2048 + blockIdx.x) * 8 + 4 + (k)] = t_; } } while (0)
extern "C" int ysmr_debug_read_block_stamps(unsigned long long *out, int n) { return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_block_stamps), sizeof(unsigned long long) * n); }
__device__ unsigned long long g_ring[4096 * 2];
__device__ unsigned int g_ring_n;
#define RING(tag) do { unsigned long long t_; asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_) :: "memory"); unsigned int i_ = atomicAdd(&g_ring_n, 1u) & 4095u; g_ring[2 * i_] = (unsigned long long)(tag); g_ring[2 * i_ + 1] = t_; } while (0)
extern "C" int ysmr_debug_read_ring(unsigned long long *out, unsigned int *n) { hipError_t e = hipMemcpyFromSymbol(out, HIP_SYMBOL(g_ring), sizeof(unsigned long long) * 8192); if (e == hipSuccess) e = hipMemcpyFromSymbol(n, HIP_SYMBOL(g_ring_n), 4); return (int)e; }
extern "C" int ysmr_debug_read_stamps(unsigned long long *out) { return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_stamps), sizeof(unsigned long long) * 32); }
#define LRING(k) do { if (threadIdx.x == 0) RING(((10ull + (k)) << 40) | (unsigned)frame); } while (0)   // k_link phases
// when every wave of a frame's k_track finished (plain stores, one slot per wave; the host takes the maximum)
__device__ unsigned long long g_wave_end[64 * 8192];
#define TRACK_END() do { if ((threadIdx.x & 63) == 0 && i < 8192) { unsigned long long t_; asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_) :: "memory"); g_wave_end[(frame & 63) * 8192 + i] = t_; } } while (0)
extern "C" int ysmr_debug_read_wave_end(unsigned long long *out) { return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_wave_end), sizeof(unsigned long long) * 64 * 8192); }
#else
#define GSTAMP(k) do {} while (0)
#define BSTAMP(k) do {} while (0)
#define RING(tag) do {} while (0)
#define LRING(k) do {} while (0)
#define TRACK_END() do {} while (0)
#endif

namespace {

constexpr int ERR_TRACK_CAPACITY = 1;  // more live tracks than `capacity`
constexpr int ERR_ROWS_CAPACITY = 2;   // row buffer full
constexpr int ERR_DET_CLAMPED = 4;     // detection count exceeded max_det

__device__ __forceinline__ int det_count(int m_host, const int32_t *m_dev, int max_det, int *err)
{
    int m = m_host >= 0 ? m_host : *m_dev;
    if (m > max_det) { m = max_det; if (err) atomicOr(err, ERR_DET_CLAMPED); }
    return m < 0 ? 0 : m;
}

// ------------------------------------------------------------------------------------------
// Nearest detection of one track, computed by one wave (64 lanes stride over the detections).
// scipy cdist('euclidean') on 2-D points is sqrt(dx*dx + dy*dy) in float64; argmin
// takes the lowest column among equal distances.  sqrt is monotone, so the row minimum is
// sqrt(min s) -- but two different s can round to the same sqrt, and then the lower column wins.
// Pass 1 finds min s; pass 2 takes the lowest column whose s is within 2^-48 (relative) of it.
// Only if one of those differs from min s at all (practically never) a third pass compares the
// float64 square roots themselves; that pass sits behind a wave-uniform branch.
// ------------------------------------------------------------------------------------------
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ double dpp_min(double v)
{
    long long b = __double_as_longlong(v);
    // lanes outside ROW_MASK / without a source read +inf (old = +inf bits, bound_ctrl off keeps old)
    int lo = __builtin_amdgcn_update_dpp(0, (int)(b & 0xFFFFFFFFll), CTRL, ROW_MASK, 0xF, false);
    int hi = __builtin_amdgcn_update_dpp(0x7FF00000, (int)(b >> 32), CTRL, ROW_MASK, 0xF, false);
    const double o = __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
    return __builtin_fmin(o, v);      // (one v_min_f64; squared distances are never NaN)
}
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ int dpp_min(int v)
{
    const int o = __builtin_amdgcn_update_dpp(0x7FFFFFFF, v, CTRL, ROW_MASK, 0xF, false);
    return min(o, v);
}
template <typename T>
__device__ __forceinline__ T wave_min_lane63(T v)
{
    v = dpp_min<0x111, 0xF>(v);   // row_shr:1
    v = dpp_min<0x112, 0xF>(v);   // row_shr:2
    v = dpp_min<0x114, 0xF>(v);   // row_shr:4
    v = dpp_min<0x118, 0xF>(v);   // row_shr:8  -> lane 15 of each row holds the row minimum
    v = dpp_min<0x142, 0xA>(v);   // row_bcast:15 into rows 1 and 3
    v = dpp_min<0x143, 0xC>(v);   // row_bcast:31 into rows 2 and 3 -> lane 63 holds the minimum
    return v;
}
__device__ __forceinline__ double wave_min(double v)
{
    long long b = __double_as_longlong(wave_min_lane63(v));
    int lo = __builtin_amdgcn_readlane((int)(b & 0xFFFFFFFFll), 63);
    int hi = __builtin_amdgcn_readlane((int)(b >> 32), 63);
    return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}
__device__ __forceinline__ int wave_min(int v) { return __builtin_amdgcn_readlane(wave_min_lane63(v), 63); }

constexpr int ROWMIN_U = 8;   // detections per lane per chunk (all loads of a chunk in flight together)

// The third tracking coordinate of a 3-D handle (ysmr_tracker_dimensions: the mean luminosity under a detection's box,
// tracker.py:111, 151).  The per-frame kernels are instantiated twice: D3 = false is the code they were before the third
// coordinate existed (the argument is empty and nothing reads it), D3 = true adds one float64 per track and per detection to
// the distances and to the stored position -- nothing else of the link changes.  There is no filter bank on a 3-D handle.
template <bool D3> struct Third3 {};
template <> struct Third3<true> {
    double *pos3;           // [capacity] by slot, beside TrackerDev::pos
    const double *det3;     // [m] of the frame being linked
    const double *next3;    // [m_next] of the frame whose row minima the launch prepares (NULL without one)
};

template <typename DetT>
struct DetChunk { DetT qx[ROWMIN_U], qy[ROWMIN_U]; };   // raw: converting here would wait for the loads here

template <typename DetT>
__device__ __forceinline__ void load_chunk(DetChunk<DetT> &c, const DetT *__restrict__ det, int m, int j0, int lane)
{
#pragma unroll
    for (int u = 0; u < ROWMIN_U; ++u) {
        int j = min(j0 + u * 64 + lane, m - 1);
        c.qx[u] = det[(size_t)j * 5 + 0];
        c.qy[u] = det[(size_t)j * 5 + 1];
    }
}

// `first` holds detections [0, 64*ROWMIN_U) already loaded by the caller (issued before the GSFF so
// that their latency hides behind it).  With m <= 64*ROWMIN_U every pass runs out of registers.
template <typename DetT, bool D3 = false>
__device__ __forceinline__ void rowmin_wave(const TrackerDev &t, int row, double px, double py,
                                            const DetT *__restrict__ det, int m, int lane, DetChunk<DetT> &first,
                                            double pl = 0.0, const double *__restrict__ det3 = nullptr)
{
    // (3-D: cdist sums dx*dx + dy*dy + dl*dl in that order; the third coordinate is fetched where it is used -- a masked
    // tail entry reads the last real one and is moved out of the way by its x as before)
    auto third = [&](double s, int j) {
        if constexpr (D3) {
            const double dl = pl - det3[min(j, m - 1)];
            s = s + dl * dl;
        }
        return s;
    };
    constexpr int CHUNK = 64 * ROWMIN_U;
    const bool multi = m > CHUNK;
    const double inf = __longlong_as_double(0x7FF0000000000000ll);
    double lane_min = inf;
    // entries past m (stale rows of the frame slice / the clamped tail of the last chunk) are moved out of the way ONCE,
    // in their 32-bit x: 1e30 squared is finite, larger than any real squared distance and never "near" the minimum --
    // no select on the 64-bit distance in either pass
    auto mask_tail = [&](int j0) {
#pragma unroll
        for (int u = 0; u < ROWMIN_U; ++u)
            first.qx[u] = (j0 + u * 64 + lane < m) ? first.qx[u] : (DetT)1e30f;
    };
    for (int j0 = 0; j0 < m; j0 += CHUNK) {
        if (j0 > 0) load_chunk(first, det, m, j0, lane);
        mask_tail(j0);
#pragma unroll
        for (int u = 0; u < ROWMIN_U; ++u) {
            const double dx = px - (double)first.qx[u];
            const double dy = py - (double)first.qy[u];
            double s = dx * dx;
            s = s + dy * dy;
            s = third(s, j0 + u * 64 + lane);
            lane_min = __builtin_fmin(s, lane_min);
        }
    }
    const double s_min = wave_min(lane_min);
    const double near_limit = s_min + s_min * 0x1p-48;
    int cand = 0x7FFFFFFF;
    bool inexact = false;
    for (int j0 = 0; j0 < m; j0 += CHUNK) {
        if (multi) { load_chunk(first, det, m, j0, lane); mask_tail(j0); }
#pragma unroll
        for (int u = 0; u < ROWMIN_U; ++u) {
            const int j = j0 + u * 64 + lane;
            const double dx = px - (double)first.qx[u];
            const double dy = py - (double)first.qy[u];
            double s = dx * dx;
            s = s + dy * dy;
            s = third(s, j);
            const bool near = s <= near_limit;
            cand = near ? min(cand, j) : cand;
            inexact = inexact || (near && s != s_min);
        }
    }
    const double d_min = sqrt(s_min);
    if (__any(inexact)) {   // some s differs from min s by a few ulps: compare the rounded roots
        cand = 0x7FFFFFFF;
        for (int j = lane; j < m; j += 64) {
            const double dx = px - (double)det[(size_t)j * 5 + 0];
            const double dy = py - (double)det[(size_t)j * 5 + 1];
            double s = dx * dx;
            s = s + dy * dy;
            s = third(s, j);
            if (s <= near_limit && sqrt(s) == d_min) cand = min(cand, j);
        }
    }
    const int best = wave_min(cand);
    if (lane == 0) {
        t.row_min[row] = d_min;
        t.row_arg[row] = best;
    }
}

// One block per frame: bounding box of the detection centres, 128 x 128 cells over it (one cell of margin), a
// counting sort of the detection columns by cell.  Runs once per batch, off the frame-to-frame chain.
template <typename DetT>
__global__ __launch_bounds__(1024) void k_grid_build(const DetT *__restrict__ det_all, const int32_t *__restrict__ det_count,
                                                     int max_det, char *grid_block, size_t per_frame)
{
    __shared__ int s_cnt[GRID_CELLS];          // counts, then cursors
    __shared__ float s_red[4][16];
    __shared__ int s_wave_sum[16];
    const int f = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const DetT *det = det_all + (size_t)f * max_det * 5;
    int m = det_count[f];
    m = m < 0 ? 0 : (m > max_det ? max_det : m);
    int *start = (int *)(grid_block + per_frame * f);
    int *items = start + GRID_CELLS + 64;
    float *hdr = (float *)(items + max_det);
    float2 *xy = (float2 *)(hdr + 16);
    for (int c = tid; c < GRID_CELLS; c += 1024) s_cnt[c] = 0;
    float lo_x = 3.0e38f, lo_y = 3.0e38f, hi_x = -3.0e38f, hi_y = -3.0e38f;
    for (int j = tid; j < m; j += 1024) {
        const float x = (float)det[(size_t)j * 5], y = (float)det[(size_t)j * 5 + 1];
        lo_x = fminf(lo_x, x); hi_x = fmaxf(hi_x, x); lo_y = fminf(lo_y, y); hi_y = fmaxf(hi_y, y);
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        lo_x = fminf(lo_x, __shfl_xor(lo_x, d)); hi_x = fmaxf(hi_x, __shfl_xor(hi_x, d));
        lo_y = fminf(lo_y, __shfl_xor(lo_y, d)); hi_y = fmaxf(hi_y, __shfl_xor(hi_y, d));
    }
    if (lane == 0) { s_red[0][w] = lo_x; s_red[1][w] = hi_x; s_red[2][w] = lo_y; s_red[3][w] = hi_y; }
    __syncthreads();
    lo_x = s_red[0][0]; hi_x = s_red[1][0]; lo_y = s_red[2][0]; hi_y = s_red[3][0];
    for (int k = 1; k < 16; ++k) {
        lo_x = fminf(lo_x, s_red[0][k]); hi_x = fmaxf(hi_x, s_red[1][k]);
        lo_y = fminf(lo_y, s_red[2][k]); hi_y = fmaxf(hi_y, s_red[3][k]);
    }
    float extent = fmaxf(fmaxf(hi_x - lo_x, hi_y - lo_y), 1.0f);
    const float cell = extent / (float)(GRID_N - 2), inv = 1.0f / cell;
    const float x0 = lo_x - cell, y0 = lo_y - cell;
    if (tid == 0) { hdr[0] = x0; hdr[1] = y0; hdr[2] = cell; hdr[3] = inv; }
    auto cell_of = [&](int j) {
        int cx = (int)floorf(((float)det[(size_t)j * 5] - x0) * inv), cy = (int)floorf(((float)det[(size_t)j * 5 + 1] - y0) * inv);
        cx = cx < 0 ? 0 : (cx > GRID_N - 1 ? GRID_N - 1 : cx);
        cy = cy < 0 ? 0 : (cy > GRID_N - 1 ? GRID_N - 1 : cy);
        return cy * GRID_N + cx;
    };
    for (int j = tid; j < m; j += 1024) atomicAdd(&s_cnt[cell_of(j)], 1);
    __syncthreads();
    // exclusive scan of the 16384 counts: 16 consecutive cells per thread, wave scan of the thread sums, wave sums
    int local[16], sum = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) { local[k] = sum; sum += s_cnt[tid * 16 + k]; }
    int incl = sum;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const int o = __shfl_up(incl, d); if (lane >= d) incl += o; }
    if (lane == 63) s_wave_sum[w] = incl;
    __syncthreads();
    int before = incl - sum;
    for (int k = 0; k < w; ++k) before += s_wave_sum[k];
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const int at = before + local[k];
        start[tid * 16 + k] = at;
        s_cnt[tid * 16 + k] = at;
    }
    if (tid == 1023) start[GRID_CELLS] = before + sum;
    __syncthreads();
    for (int j = tid; j < m; j += 1024) {
        const int at = atomicAdd(&s_cnt[cell_of(j)], 1);
        items[at] = j;
        xy[at] = make_float2((float)det[(size_t)j * 5], (float)det[(size_t)j * 5 + 1]);
    }
}

// Row minimum through the grid: rings of cells around the track until no unseen detection can be as near as the
// best one found (the block of cells' boundary is farther, with a margin far above rounding), then the same tie
// rule as rowmin_wave on the detections of that block -- lowest column among the equal rounded distances.
// Returns false when four rings were not enough (a track far from every detection): the caller falls back to
// all pairs.
struct GridHdr { float x0, y0, cell, inv; };
__device__ __forceinline__ GridHdr grid_hdr(const DetGrid &g)   // (fetched by the caller ahead of everything the search waits for)
{
    return g.start ? GridHdr{g.hdr[0], g.hdr[1], g.hdr[2], g.hdr[3]} : GridHdr{0.f, 0.f, 1.f, 1.f};
}
template <typename DetT>
__device__ __forceinline__ bool rowmin_grid(const TrackerDev &t, int row, double px, double py, const DetT *__restrict__ det,
                                            const DetGrid &g, int lane, const GridHdr &gh)
{
    const double x0 = (double)gh.x0, y0 = (double)gh.y0, cell = (double)gh.cell, inv = (double)gh.inv;
    int cx = (int)floor((px - x0) * inv), cy = (int)floor((py - y0) * inv);
    cx = cx < 0 ? 0 : (cx > GRID_N - 1 ? GRID_N - 1 : cx);
    cy = cy < 0 ? 0 : (cy > GRID_N - 1 ? GRID_N - 1 : cy);
    const double inf = __longlong_as_double(0x7FF0000000000000ll);
    for (int k = 0; k <= 3; ++k) {
        const int side = 2 * k + 1;
        const int ix = cx - k + lane % side, iy = cy - k + lane / side;
        const bool have = lane < side * side && ix >= 0 && ix < GRID_N && iy >= 0 && iy < GRID_N;
        int a = 0, b = 0;
        if (have) { a = g.start[iy * GRID_N + ix]; b = g.start[iy * GRID_N + ix + 1]; }
        double lane_min = inf;
        for (int q = a; q < b; ++q) {
            const float2 c = g.xy[q];
            const double dx = px - (double)c.x;
            const double dy = py - (double)c.y;
            double s = dx * dx;
            s = s + dy * dy;
            lane_min = __builtin_fmin(s, lane_min);
        }
        const double s_min = wave_min(lane_min);
        // distance from the track to the outside of the block [cx-k, cx+k] x [cy-k, cy+k]; a side of the block on
        // the edge of the grid has nothing beyond it (every detection lies inside the grid)
        double bound = inf;
        if (cx - k > 0) bound = fmin(bound, px - (x0 + (cx - k) * cell));
        if (cx + k < GRID_N - 1) bound = fmin(bound, (x0 + (cx + k + 1) * cell) - px);
        if (cy - k > 0) bound = fmin(bound, py - (y0 + (cy - k) * cell));
        if (cy + k < GRID_N - 1) bound = fmin(bound, (y0 + (cy + k + 1) * cell) - py);
        bound -= 1e-3 * cell;       // (cells were assigned in float arithmetic)
        const bool done = bound == inf || (s_min < inf && bound > 0.0 && bound * bound > s_min * (1.0 + 1e-9));
        if (!done) continue;
        if (!(s_min < inf)) return false;   // no detection at all in a block that covers the grid: m == 0 is the caller's
        const double near_limit = s_min + s_min * 0x1p-48;
        const double d_min = sqrt(s_min);
        int cand = 0x7FFFFFFF;
        bool inexact = false;
        for (int q = a; q < b; ++q) {
            const int j = g.items[q];
            const float2 c = g.xy[q];
            const double dx = px - (double)c.x;
            const double dy = py - (double)c.y;
            double s = dx * dx;
            s = s + dy * dy;
            const bool near = s <= near_limit;
            cand = near ? min(cand, j) : cand;
            inexact = inexact || (near && s != s_min);
        }
        if (__any(inexact)) {   // some s differs from min s by a few ulps: compare the rounded roots
            cand = 0x7FFFFFFF;
            for (int q = a; q < b; ++q) {
                const int j = g.items[q];
                const float2 c = g.xy[q];
                const double dx = px - (double)c.x;
                const double dy = py - (double)c.y;
                double s = dx * dx;
                s = s + dy * dy;
                if (s <= near_limit && sqrt(s) == d_min) cand = min(cand, j);
            }
        }
        const int best = wave_min(cand);
        if (lane == 0) {
            t.row_min[row] = d_min;
            t.row_arg[row] = best;
        }
        return true;
    }
    return false;
}

// Stand-alone row-min pass (first frame of a batch / single-frame updates); inside a batch the
// row-min of frame f+1 rides on k_track of frame f.
template <typename DetT, bool D3 = false>
__global__ __launch_bounds__(256) void k_rowmin(TrackerDev t, const DetT *__restrict__ det, int m_host,
                                                const int32_t *m_dev, int set_row_base, const long long *row_count_ext,
                                                DetGrid grid, Third3<D3> th)
{
    // (fused path, start of ysmr_tracker_run / _update: row_base of the current state := the caller's
    // running row count; folded in here to save a launch per batch)
    if (set_row_base && blockIdx.x == 0 && threadIdx.x == 0) t.row_base[0] = row_count_ext ? *row_count_ext : 0;
    const int n = *t.n_tracks;
    const int m = det_count(m_host, m_dev, t.max_det, nullptr);
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n || m == 0) return;
    const int slot = t.order[row];
    const int lane = threadIdx.x & 63;
    if (lane == 0 && !t.gone_by_row) t.row_gone[row] = t.gone[slot];
    const GridHdr gh = grid_hdr(grid);
    if (grid.start && rowmin_grid(t, row, t.pos[slot], t.pos[t.capacity + slot], det, grid, lane, gh)) return;
    DetChunk<DetT> first;
    load_chunk(first, det, m, 0, lane);
    if constexpr (D3) rowmin_wave<DetT, true>(t, row, t.pos[slot], t.pos[t.capacity + slot], det, m, lane, first, th.pos3[slot], th.det3);
    else rowmin_wave(t, row, t.pos[slot], t.pos[t.capacity + slot], det, m, lane, first);
}

// ------------------------------------------------------------------------------------------
// GSFF (gsff.py), one WAVE per track.  The track's history ring (hist_cap entries of (x, y),
// contiguous in HBM) is spread over the lanes -- value k = 2*entry + component lives in lane
// k % 64 -- so a FIR estimate sum_k G[k] * y[k] is one multiply per lane plus a butterfly
// reduction instead of a 2N-long chain of dependent float64 adds, and the whole state arrives with
// one coalesced load.
// ------------------------------------------------------------------------------------------
constexpr int TRACK_VALS = 2;  // values per lane: supports hist_cap <= 64 entries

struct TrackRegs {
    double v[TRACK_VALS];   // history values held by this lane
};

template <int CTRL, int ROW_MASK>
__device__ __forceinline__ double dpp_add(double v)
{
    long long b = __double_as_longlong(v);
    int lo = __builtin_amdgcn_update_dpp(0, (int)(b & 0xFFFFFFFFll), CTRL, ROW_MASK, 0xF, false);
    int hi = __builtin_amdgcn_update_dpp(0, (int)(b >> 32), CTRL, ROW_MASK, 0xF, false);
    // lanes outside ROW_MASK / without a source get +0.0 (old = 0, bound_ctrl off writes old)
    return v + __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}

// sum over the 64 lanes, returned to every lane; a fixed (deterministic) association order
__device__ __forceinline__ double wave_total(double v)
{
    v = dpp_add<0x111, 0xF>(v);   // row_shr:1
    v = dpp_add<0x112, 0xF>(v);   // row_shr:2
    v = dpp_add<0x114, 0xF>(v);   // row_shr:4
    v = dpp_add<0x118, 0xF>(v);   // row_shr:8  -> lane 15 of each row holds the row sum
    v = dpp_add<0x142, 0xA>(v);   // row_bcast:15 into rows 1 and 3
    v = dpp_add<0x143, 0xC>(v);   // row_bcast:31 into rows 2 and 3 -> lane 63 holds the total
    long long b = __double_as_longlong(v);
    int lo = __builtin_amdgcn_readlane((int)(b & 0xFFFFFFFFll), 63);
    int hi = __builtin_amdgcn_readlane((int)(b >> 32), 63);
    return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}

// History layout inside the wave: lane l, register q holds coordinate (l >> 5) of history entry
// (l & 31) + 32 q -- x in lanes 0..31, y in lanes 32..63 -- so that for a decoupled gain (x-hat
// from x only, y-hat from y only: every constant-velocity LSF gain) one 5-step half-wave reduction
// yields both sums.  In memory the history stays [entry][coordinate].
// Entry e is the measurement of e frames ago (NEWEST FIRST, shifted by one lane every frame and written back whole: one
// 512-byte store, as a ring's single new entry was one store instruction too).  The gain that multiplies a lane's entry
// is then a property of the lane: it is fetched with the very first loads of the kernel (FirGains), where a ring needed
// its head -- part of the state -- before it could even address the gain table (1150 of the filter bank's 6000 cycles
// were that gather and its index arithmetic).
__device__ __forceinline__ int hist_entry(int lane, int q) { return (lane & 31) + 32 * q; }
__device__ __forceinline__ int hist_comp(int lane) { return lane >> 5; }

__device__ __forceinline__ double wave_shr1_f64(double v)   // the value of lane - 1
{
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_update_dpp(0, (int)(b & 0xFFFFFFFFll), 0x138 /* wave_shr:1 */, 0xF, 0xF, false);
    const int hi = __builtin_amdgcn_update_dpp(0, (int)(b >> 32), 0x138, 0xF, 0xF, false);
    return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}
__device__ __forceinline__ double lane_value(double v, int src_lane)
{
    long long b = __double_as_longlong(v);
    int lo = __builtin_amdgcn_readlane((int)(b & 0xFFFFFFFFll), src_lane);
    int hi = __builtin_amdgcn_readlane((int)(b >> 32), src_lane);
    return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}
// lanes 0..31 and lanes 32..63 summed separately: lane 31 and lane 63 hold the two totals
__device__ __forceinline__ double half_wave_totals(double v)
{
    v = dpp_add<0x111, 0xF>(v);   // row_shr:1
    v = dpp_add<0x112, 0xF>(v);   // row_shr:2
    v = dpp_add<0x114, 0xF>(v);   // row_shr:4
    v = dpp_add<0x118, 0xF>(v);   // row_shr:8  -> lane 15 of each row holds the row sum
    v = dpp_add<0x142, 0xA>(v);   // row_bcast:15 into rows 1 and 3
    return v;
}

// This lane's gains: for each filter the coefficient of history entry (lane & 31) in the x-hat row (lanes 0..31) or the
// y-hat row (lanes 32..63) of a DECOUPLED gain; 0 where the entry lies beyond the filter's horizon.  Depends on nothing
// but the lane, so it is requested before the track's state is known.  (Entries 32.. -- horizons beyond 32 frames --
// and coupled gains fetch theirs where they are used.)
template <int NF>
struct FirGains { double g[NF]; };
template <int NF>
__device__ __forceinline__ void fir_gains_fetch(const TrackerDev &t, const double *gains, int lane, FirGains<NF> &G)
{
    const int comp = hist_comp(lane), e = hist_entry(lane, 0);
#pragma unroll
    for (int f = 0; f < NF; ++f) {
        const int N = t.n_i[f < t.n_f ? f : 0];
        const bool in = f < t.n_f && e < t.hist_cap && e < N && t.gains_decoupled;
        const double g = gains[in ? t.gain_off[f] + comp * (2 * N + 1) + 2 * (N - 1 - e) : 0];
        G.g[f] = in ? g : 0.0;
    }
}

// FIR estimates of ALL active filters at once (rows 0 and 1 of gain f times the last n_f[f]
// measurements: lsff_calc, gsff.py:156-177).  Branch-free over the filter bank so that the
// independent reductions interleave; filters >= mode are computed on masked zeros and discarded.
template <int NF>
__device__ __forceinline__ void fir_wave_all(const TrackerDev &t, const double *gains, const TrackRegs &h, int lane,
                                             int mode, const FirGains<NF> &G, double *x0, double *x1)
{
    const int L = t.hist_cap;
    const int comp = hist_comp(lane);
    GSTAMP(8);
    if (t.gains_decoupled) {
        double p[NF];
#pragma unroll
        for (int f = 0; f < NF; ++f) p[f] = (f < mode) ? G.g[f] * h.v[0] : 0.0;      // (G.g is 0 beyond the horizon)
        if (L > 32) {                      // (uniform) horizons beyond 32 frames: the second register of the history
            const int e = hist_entry(lane, 1);
#pragma unroll
            for (int f = 0; f < NF; ++f) {
                const int N = t.n_i[f < t.n_f ? f : 0];
                const bool in = (f < mode) && (e < L) && (e < N);
                const double g = gains[in ? t.gain_off[f] + comp * (2 * N + 1) + 2 * (N - 1 - e) : 0];
                p[f] = in ? p[f] + g * h.v[1] : p[f];
            }
        }
        GSTAMP(9);
#pragma unroll
        for (int f = 0; f < NF; ++f) p[f] = half_wave_totals(p[f]);
#pragma unroll
        for (int f = 0; f < NF; ++f) {
            const double sx = lane_value(p[f], 31), sy = lane_value(p[f], 63);
            if (f < mode) { x0[f] = sx; x1[f] = sy; }
        }
        GSTAMP(10);
        return;
    }
    double p0[NF], p1[NF];
#pragma unroll
    for (int f = 0; f < NF; ++f) { p0[f] = 0.0; p1[f] = 0.0; }
#pragma unroll
    for (int q = 0; q < TRACK_VALS; ++q) {
        const int e = hist_entry(lane, q);          // = age: 0 is the newest measurement
        double ga[NF], gb[NF];
        bool in[NF];
#pragma unroll
        for (int f = 0; f < NF; ++f) {
            const int N = t.n_i[f < t.n_f ? f : 0];
            in[f] = (f < mode) && (e < L) && (e < N);
            const int col = in[f] ? 2 * (N - 1 - e) + comp : 0;
            ga[f] = gains[t.gain_off[f < t.n_f ? f : 0] + col];
            gb[f] = gains[t.gain_off[f < t.n_f ? f : 0] + 2 * N + col];
        }
#pragma unroll
        for (int f = 0; f < NF; ++f) {
            p0[f] = in[f] ? p0[f] + ga[f] * h.v[q] : p0[f];
            p1[f] = in[f] ? p1[f] + gb[f] * h.v[q] : p1[f];
        }
    }
    // wave sums by DPP (no LDS round trips): row_shr 1,2,4,8 leave each 16-lane row's sum in its
    // last lane, row_bcast15 / row_bcast31 carry it across rows, lane 63 ends with the total
#pragma unroll
    for (int f = 0; f < NF; ++f) {
        const double sx = wave_total(p0[f]), sy = wave_total(p1[f]);
        if (f < mode) { x0[f] = sx; x1[f] = sy; }
    }
}

// GSFF correct + predict of one track by one wave (gsff.py:204-347).  z = measurement; returns the
// filtered position (o) and the prediction (p), and leaves the prediction in t.pos[slot].
// fresh_track: the slot was just (re)assigned -- ignore whatever filter state it still holds.
// filter state of one track, spread over the wave (history) or replicated (the rest)
template <int NF>
struct GsffState {
    TrackRegs h;
    double w[NF], xh0[NF], xh1[NF];
    int len, mode;
    double raw;          // this lane's field of the slot's record, as fetched (decoded by gsff_decode)
    // where the slot's state lives, worked out when it is fetched and kept for the write-back (re-reading the three base
    // pointers and the record stride from the kernel's arguments there cost four scalar loads, each with its own wait)
    double *hist_p, *rec_p, *pos_p;
    int rec_lanes;       // rec_stride
};
template <int NF>
__device__ __forceinline__ void gsff_point(const TrackerDev &t, int slot, GsffState<NF> &s)
{
    s.hist_p = t.hist + (size_t)slot * 2 * t.hist_cap;
    s.rec_p = t.rec + (size_t)slot * t.rec_stride;
    s.pos_p = t.pos + slot;
    s.rec_lanes = t.rec_stride;
}
// Issue every load of a track's filter state; no load depends on another, so one round trip.
template <int NF>
__device__ __forceinline__ void gsff_fetch(const TrackerDev &t, int slot, int lane, GsffState<NF> &s)
{
    const int L = t.hist_cap;
    gsff_point(t, slot, s);
    const double *hist = s.hist_p;
    s.raw = lane < s.rec_lanes ? s.rec_p[lane] : 0.0;
#pragma unroll
    for (int q = 0; q < TRACK_VALS; ++q) {
        const int e = hist_entry(lane, q);
        s.h.v[q] = (e < L) ? hist[2 * e + hist_comp(lane)] : 0.0;
    }
}
// the fields of the fetched record, broadcast to the wave (v_readlane: the wait for the load lands here)
template <int NF>
__device__ __forceinline__ void gsff_decode(const TrackerDev &t, GsffState<NF> &s)
{
    const int nf = t.n_f;
    const long long b = __double_as_longlong(s.raw);
    const int lo = (int)(b & 0xFFFFFFFFll), hi = (int)(b >> 32);
    auto field = [&](int k) {
        return __longlong_as_double(((long long)__builtin_amdgcn_readlane(hi, k) << 32) | (unsigned int)__builtin_amdgcn_readlane(lo, k));
    };
    s.len = __builtin_amdgcn_readlane(lo, 0);
    s.mode = __builtin_amdgcn_readlane(lo, 1);
#pragma unroll
    for (int f = 0; f < NF; ++f) {
        const bool on = f < nf;   // entries >= mode hold stale values that nothing reads
        s.w[f] = on ? field(2 + f) : 0.0;
        s.xh0[f] = on ? field(2 + nf + f) : 0.0;
        s.xh1[f] = on ? field(2 + 2 * nf + f) : 0.0;
    }
}
template <int NF>
__device__ __forceinline__ void gsff_blank(GsffState<NF> &s)
{
    s.len = s.mode = 0;
    s.raw = 0.0;         // (decodes to an empty bank)
#pragma unroll
    for (int q = 0; q < TRACK_VALS; ++q) s.h.v[q] = 0.0;
#pragma unroll
    for (int f = 0; f < NF; ++f) s.w[f] = s.xh0[f] = s.xh1[f] = 0.0;
}
template <int NF>
__device__ __forceinline__ void gsff_wave(const TrackerDev &t, const double *gains, int slot, int lane, double z0,
                                          double z1, bool fresh_track, GsffState<NF> &st, const FirGains<NF> &G,
                                          double &o0, double &o1, double &p0, double &p1)
{
    const int cap = t.capacity, nf = t.n_f, L = t.hist_cap;
    GSTAMP(0);
    double *hist = st.hist_p;
    gsff_decode(t, st);
    int len = st.len, mode = st.mode;
    TrackRegs &h = st.h;
    double (&w)[NF] = st.w;
    double (&xh0)[NF] = st.xh0;
    double (&xh1)[NF] = st.xh1;
    GSTAMP(1);
    // ---- correct (gsff.py:251-347)
    bool fresh = (len == 0) || fresh_track;
    if (fresh_track) { len = 0; mode = 0; }
    if (fresh) {   // history starts as n_i[0] copies of the first measurement
#pragma unroll
        for (int q = 0; q < TRACK_VALS; ++q)
            if (hist_entry(lane, q) < t.n_i[0]) h.v[q] = hist_comp(lane) ? z1 : z0;
        len = t.n_i[0];
    }
    bool grew = false;
    if (mode < nf) {
        while (len >= t.n_i[mode]) {
            ++mode;
            grew = true;
            if (mode >= nf) break;
        }
    }
    if (grew) {
        const double w0 = 1.0 / (double)mode;
        fir_wave_all<NF>(t, gains, h, lane, mode, G, xh0, xh1);
#pragma unroll
        for (int f = 0; f < NF; ++f)
            if (f < mode) w[f] = w0;
    }
    GSTAMP(2);
    // append the measurement and start the predict-step FIR (gsff.py:204-249) right away: it reads
    // only the history, so its reductions overlap the likelihood arithmetic below
    // (every entry one frame older: one lane up; the measurement becomes entry 0 of each half)
    if (L > 32) {                          // (uniform) the second register takes over what leaves the first
        const double cx = lane_value(h.v[0], 31), cy = lane_value(h.v[0], 63);
        h.v[1] = wave_shr1_f64(h.v[1]);
        h.v[1] = (lane & 31) == 0 ? (hist_comp(lane) ? cy : cx) : h.v[1];
    }
    h.v[0] = wave_shr1_f64(h.v[0]);
    h.v[0] = (lane & 31) == 0 ? (hist_comp(lane) ? z1 : z0) : h.v[0];
    if (len < L) ++len;
    double nx0[NF], nx1[NF];
#pragma unroll
    for (int f = 0; f < NF; ++f) { nx0[f] = 0.0; nx1[f] = 0.0; }
    fir_wave_all<NF>(t, gains, h, lane, mode, G, nx0, nx1);
    GSTAMP(3);
    // likelihoods (gsff.py:179-202): lane f evaluates filter f's exp(), the results are broadcast
    // (the float64 exp is ~150 instructions; doing the n_f of them one after the other on every
    // lane was a third of this function)
    double lik[NF];
    double total = 0.0;
    {
        double xa = 0.0, xb = 0.0;
#pragma unroll
        for (int f = 0; f < NF; ++f) { xa = (lane == f) ? xh0[f] : xa; xb = (lane == f) ? xh1[f] : xb; }
        double d0 = z0 - xa, d1 = z1 - xb;
        double q = d0 * d0;
        q = q + d1 * d1;
        double l = exp(-0.5 * q);
        if (l < t.lik_min) l = t.lik_min;
#pragma unroll
        for (int f = 0; f < NF; ++f) {
            lik[f] = lane_value(l, f);
            total = (f < mode) ? total + lik[f] * w[f] : total;
        }
    }
    // new weights; output = np.sum(x_hat * w, axis=1) = a0 + ((a1 + a2) + ...)
    double f0 = 0.0, f1 = 0.0, r0 = 0.0, r1 = 0.0;
    {   // new weights w_i = lik_i * w_i / total: one division per lane instead of n_f per lane
        double lw = 1.0;
#pragma unroll
        for (int f = 0; f < NF; ++f) lw = (lane == f) ? lik[f] * w[f] : lw;
        const double wn = lw / total;
#pragma unroll
        for (int f = 0; f < NF; ++f) {
            const double v = lane_value(wn, f);
            w[f] = (f < mode) ? v : w[f];
        }
    }
#pragma unroll
    for (int f = 0; f < NF; ++f)
        if (f < mode) {
            double a = xh0[f] * w[f], b = xh1[f] * w[f];
            if (f == 0) { f0 = a; f1 = b; }
            else if (f == 1) { r0 = a; r1 = b; }
            else { r0 = r0 + a; r1 = r1 + b; }
        }
    o0 = mode > 1 ? f0 + r0 : f0;
    o1 = mode > 1 ? f1 + r1 : f1;
    GSTAMP(4);
    // ---- predict: the new estimates, weighted
    f0 = f1 = r0 = r1 = 0.0;
#pragma unroll
    for (int f = 0; f < NF; ++f)
        if (f < mode) {
            xh0[f] = nx0[f]; xh1[f] = nx1[f];
            double a = xh0[f] * w[f], b = xh1[f] * w[f];
            if (f == 0) { f0 = a; f1 = b; }
            else if (f == 1) { r0 = a; r1 = b; }
            else { r0 = r0 + a; r1 = r1 + b; }
        }
    p0 = mode > 1 ? f0 + r0 : f0;
    p1 = mode > 1 ? f1 + r1 : f1;
    GSTAMP(5);
    // ---- write back
#pragma unroll
    for (int q = 0; q < TRACK_VALS; ++q) {
        const int e = hist_entry(lane, q);
        if (e < L && (q == 0 || L > 32)) hist[2 * e + hist_comp(lane)] = h.v[q];     // the whole history, shifted
    }
    if (lane == 0) {
        st.pos_p[0] = p0;
        st.pos_p[cap] = p1;
    }
    {   // the record, one store: every lane picks its field
        double val = __longlong_as_double(lane == 0 ? (long long)(unsigned int)len : (long long)(unsigned int)mode);
#pragma unroll
        for (int f = 0; f < NF; ++f)
            if (f < nf) {
                val = lane == 2 + f ? w[f] : val;
                val = lane == 2 + nf + f ? xh0[f] : val;
                val = lane == 2 + 2 * nf + f ? xh1[f] : val;
            }
        if (lane < st.rec_lanes) st.rec_p[lane] = val;
    }
    GSTAMP(6);
}

template <typename DetT, int NF, bool D3 = false>
__global__ __launch_bounds__(256) void k_track(TrackerDev t, int frame, ysmr_row *rows, long long rows_capacity,
                                               const DetT *__restrict__ det, const DetT *__restrict__ next_det,
                                               const int32_t *next_m_dev, DetGrid next_grid, Third3<D3> th)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) RING((4ull << 40) | (unsigned)frame);   // k_track entry
    BSTAMP(0);
    // one round trip: the table size, this wave's slot (row i of a table of `capacity` rows: valid memory whatever n is)
    // and the next frame's grid header are requested together
    // (one straight-line block, the counters first -- see k_frame: a branch in here costs a scalar load of the arguments
    // behind it and a wait of its own)
    const int cap = t.capacity;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int n_live = *t.n_tracks, claims_by_row = t.n_tracks[4];
    const int slot_spec = t.order[min(i, cap - 1)];
    const int claim_spec = t.claim_row[min(i, cap - 1)];
    const float *hdr = next_grid.start ? next_grid.hdr : reinterpret_cast<const float *>(t.n_tracks);   // (always readable)
    const GridHdr gh{hdr[0], hdr[1], hdr[2], hdr[3]};
    FirGains<NF> G;
    fir_gains_fetch(t, t.gains, threadIdx.x & 63, G);
    if (i >= n_live) return;
    const int lane = threadIdx.x & 63;
    // the next frame's detections do not depend on this frame's state: fetch them first
    const int m_next = next_det ? det_count(-1, next_m_dev, t.max_det, nullptr) : 0;
    DetChunk<DetT> first;
    if (m_next > 0 && !next_grid.start) load_chunk(first, next_det, m_next, 0, lane);
    const int slot = __builtin_amdgcn_readfirstlane(slot_spec);
    if (blockIdx.x == 0 && threadIdx.x == 0) RING((5ull << 40) | (unsigned)frame);   // slot known
    BSTAMP(1);
    // the measurement: the detection k_link let this track claim (tracker.py:186-196 -- position and box are
    // stored here, by the track's own wave), or the position it already has
    GsffState<NF> st;
    if (t.use_gsff) gsff_fetch(t, slot, lane, st);
    const int c = __builtin_amdgcn_readfirstlane(claims_by_row ? claim_spec : t.claim_slot[slot]);
    double z0, z1;
    [[maybe_unused]] double z2 = 0.0;      // (3-D handles)
    float bw, bh, ba;
    if (c >= 0) {
        const DetT *d = det + (size_t)c * 5;
        z0 = (double)d[0]; z1 = (double)d[1];
        bw = (float)d[2]; bh = (float)d[3]; ba = (float)d[4];
        if constexpr (D3) z2 = th.det3[c];
        if (lane == 0) {
            t.pos[slot] = z0; t.pos[cap + slot] = z1;
            t.info[slot] = bw; t.info[cap + slot] = bh; t.info[2 * cap + slot] = ba;
            if constexpr (D3) th.pos3[slot] = z2;
        }
    } else {
        z0 = t.pos[slot]; z1 = t.pos[cap + slot];
        bw = t.info[slot]; bh = t.info[cap + slot]; ba = t.info[2 * cap + slot];
        if constexpr (D3) z2 = th.pos3[slot];
    }
    double o0 = z0, o1 = z1, p0 = z0, p1 = z1;
    if (t.use_gsff) gsff_wave(t, t.gains, slot, lane, z0, z1, false, st, G, o0, o1, p0, p1);
    if (blockIdx.x == 0 && threadIdx.x == 0) RING((6ull << 40) | (unsigned)frame);   // filter bank done
    BSTAMP(2);
    if (lane == 0) {
        const long long base = t.row_base[0];
        const int gone = t.gone[slot];
        t.row_gone[i] = gone;
        if (rows && base + i < rows_capacity) {
            ysmr_row r;
            r.frame = frame;
            r.track_id = t.id[slot];
            r.x = o0; r.y = o1;
            r.w = bw; r.h = bh; r.angle = ba;
            r.disappeared = gone;
            rows[base + i] = r;
        }
    }
    // ---- nearest detection of the NEXT frame for this track (tracker.py:151-163)
    if (m_next > 0) {
        if (next_grid.start) {
            if (rowmin_grid(t, i, p0, p1, next_det, next_grid, lane, gh)) {
                if (blockIdx.x == 0 && threadIdx.x == 0) RING((7ull << 40) | (unsigned)frame);   // next row minimum known
                BSTAMP(3);
                TRACK_END();
                return;
            }
            load_chunk(first, next_det, m_next, 0, lane);
        }
        if constexpr (D3) rowmin_wave<DetT, true>(t, i, p0, p1, next_det, m_next, lane, first, z2, th.next3);
        else rowmin_wave(t, i, p0, p1, next_det, m_next, lane, first);
    }
}

// ------------------------------------------------------------------------------------------
// CPython set model: iteration order of set(range(m)).difference(used_cols) (tracker.py:193,216).
// set_order.h has its rules and the serial form, which runs here on one thread over tables in HBM;
// the number of unused columns per frame is small (k_frame does everything else of the model with
// the whole block).
// ------------------------------------------------------------------------------------------
__device__ int cpython_unused_order(const TrackerDev &t, int m, int n_used, int n_unused, int *out)
{
    return set_unused_order(t.unused, m, n_used, n_unused, out, t.set_table, t.set_table + t.table_cap, t.table_cap);
}

// ------------------------------------------------------------------------------------------
// k_link: one workgroup
// ------------------------------------------------------------------------------------------
#ifndef YSMR_LINK_THREADS
#define YSMR_LINK_THREADS 1024
#endif
constexpr int LINK_THREADS = YSMR_LINK_THREADS;
constexpr int LINK_ROWS = 8192 / LINK_THREADS;       // rows per thread k_link keeps in registers for tables of more than 1024 rows

// LDS_ONLY: the two barriers wait for LDS traffic only (s_waitcnt lgkmcnt(0); s_barrier) -- __syncthreads also waits
// for every global load and store the wave has in flight, a round trip to HBM each time; only for callers that order
// nothing in global memory through these barriers.
template <bool LDS_ONLY>
__device__ __forceinline__ void block_sync()
{
    if constexpr (LDS_ONLY) asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    else __syncthreads();
}

template <bool LDS_ONLY = false>
__device__ int block_exclusive_scan(int v, int *s_scan, int *total)
{
    // exclusive rank of a 0/1 flag among the block's 1024 flags: a ballot per wave, the sixteen wave
    // counts through LDS, two barriers (the Hillis-Steele scan this replaces needed twenty-one)
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const unsigned long long bal = __ballot(v != 0);
    if (lane == 0) s_scan[w] = __popcll(bal);
    block_sync<LDS_ONLY>();
    int before = 0, all = 0;
#pragma unroll
    for (int k = 0; k < LINK_THREADS / 64; ++k) {
        const int c = s_scan[k];
        before += k < w ? c : 0;
        all += c;
    }
    *total = all;
    block_sync<LDS_ONLY>();      // (s_scan is reused by the caller's next chunk)
    return before + __popcll(bal & ((1ull << lane) - 1ull));
}

// Up to 64 insertions at once, with the result of doing them one after the other in lane order.  A slot holds
// (sequence number << 16 | key); every lane walks its key's probe sequence and takes a slot with an atomic minimum, so
// a slot ends up with the EARLIEST key that ever asked for it; a lane whose entry was displaced by an earlier key (or
// that found an earlier key there) moves on along its sequence.  The fixed point -- every key in the first slot of its
// sequence that no earlier key holds -- is exactly what sequential insertion produces (an earlier key's place never
// depends on a later one), and it is reached in as many rounds as the longest displacement chain instead of one LDS
// round trip per probe per key (36 keys, with the re-insertions of two resizes: 14 us one key at a time).
// Entries of earlier batches carry smaller sequence numbers and never move.  seq + 63 < 65535, key < 65536.
constexpr uint32_t SET_EMPTY32 = 0xFFFFFFFFu;
__device__ __forceinline__ void set_insert_batch(uint32_t *table, unsigned mask, bool active, unsigned key, unsigned seq)
{
    const uint32_t mine = (seq << 16) | key;
    unsigned long long perturb = (unsigned long long)key;
    unsigned i = key & mask;
    int j = 0;                       // offset inside the linear run that starts at i
    unsigned at = 0;
    bool need = active;              // has to propose its next candidate
    const SetProbeStep advance{i, mask, j, perturb};
    while (true) {
        if (need) {
            at = i + (unsigned)j;
            const uint32_t old = atomicMin(&table[at], mine);
            if (old > mine) need = false;      // ours for now (a displaced later entry's lane notices below)
            else advance();                    // an earlier key holds it
        }
        if (active && !need && table[at] != mine) { need = true; advance(); }   // displaced by an earlier key
        if (__ballot(need) == 0ull) return;
    }
}

// The model for k_link, in the LDS its claim tables no longer need (all LINK_THREADS threads call it): one table of
// 32-bit slots (set_insert_batch), a list for the resizes and the staged list of unclaimed columns.  Wave 0 inserts, 64
// keys at a time; clearing the table, collecting it in slot order at a resize and the final walk are done by the whole
// block.  (One thread over tables in HBM, cpython_unused_order, spent 575 us on 300 unregistered columns: 700 dependent
// insertions and a 2048-slot walk.)  Returns the number of keys, or -1 when the table would outgrow `cap_table` slots
// (the caller falls back to cpython_unused_order).
__device__ int cpython_order_block(const int *unused, int n_unused, int m, int n_used, int *out, uint32_t *table,
                                   int cap_table, uint32_t *list, unsigned short *stage, int *s_scan, int *s_state)
{
    const int tid = threadIdx.x, lane = tid & 63;
    if (set_order_is_ascending(m, n_used)) {
        for (int k = tid; k < n_unused; k += LINK_THREADS) out[k] = unused[k];
        return n_unused;
    }
    for (int k = tid; k < n_unused; k += LINK_THREADS) stage[k] = (unsigned short)unused[k];
    if (tid < 8) table[tid] = SET_EMPTY32;
    __syncthreads();
    unsigned mask = 7, seq = 0;
    int k = 0, fill = 0;
    // occupied slots of the table in slot order: keys -> dst (LDS list or the global result)
    auto collect = [&](auto *dst) {
        int base = 0;
        for (unsigned i0 = 0; i0 <= mask; i0 += LINK_THREADS) {
            const unsigned i = i0 + tid;
            const uint32_t e = i <= mask ? table[i] : SET_EMPTY32;
            int total;
            const int ex = block_exclusive_scan<true>(e != SET_EMPTY32 ? 1 : 0, s_scan, &total);
            if (e != SET_EMPTY32) dst[base + ex] = e & 0xFFFFu;
            base += total;
        }
        return base;
    };
    while (true) {
        // wave 0: keys go in until the table wants to grow (setobject.c: fill*5 >= mask*3 after an add)
        const int thresh = set_growth_fill(mask);
        const int upto = min(n_unused, k + (thresh - fill));
        if (tid < 64) {
            for (int k0 = k; k0 < upto; k0 += 64) {
                const int b = min(64, upto - k0);
                set_insert_batch(table, mask, lane < b, lane < b ? (unsigned)stage[k0 + lane] : 0u, seq + (unsigned)(k0 - k) + lane);
            }
        }
        seq += (unsigned)(upto - k); fill += upto - k; k = upto;
        __syncthreads();
        if (fill < thresh) break;
        const unsigned newsize = set_grown_size(fill);
        if ((int)newsize > cap_table) return -1;                      // (uniform)
        const int cnt = collect(list);
        __syncthreads();
        for (unsigned i = tid; i < newsize; i += LINK_THREADS) table[i] = SET_EMPTY32;
        mask = newsize - 1;
        __syncthreads();
        if (tid < 64) {
            for (int j0 = 0; j0 < cnt; j0 += 64) {
                const int b = min(64, cnt - j0);
                set_insert_batch(table, mask, lane < b, lane < b ? list[j0 + lane] : 0u, seq + (unsigned)j0 + lane);
            }
        }
        seq += (unsigned)cnt;
        __syncthreads();
    }
    return collect(out);
}

// LDS_TABLES: the per-column winner tables fit in LDS (12 B per detection column <= 140 KiB, e.g. 96 KiB at 8192; the
// per-row claims are in HBM): the claim rounds cost LDS atomics.  Otherwise the tables live in HBM (three rounds of
// device-scope atomics, ~6 us more at 5000 rows) and capacity / max_det are only bounded by 65536.
template <typename DetT, bool LDS_TABLES, bool D3 = false>
__global__ __launch_bounds__(LINK_THREADS) void k_link(TrackerDev t, const DetT *__restrict__ det, int m_host,
                                                       const int32_t *m_dev, int frame, ysmr_row *rows,
                                                       long long rows_capacity, long long *row_count,
                                                       int32_t *n_rows_out, int32_t *claim_out, int32_t *n_before_out,
                                                       int32_t *new_cols_out, int32_t *n_new_out, Third3<D3> th)
{
    extern __shared__ unsigned long long s_dyn[];
    unsigned long long *s_col_key = LDS_TABLES ? s_dyn : t.link_key;                                        // [max_det]
    int *s_col_row = LDS_TABLES ? reinterpret_cast<int *>(s_dyn + t.max_det) : t.link_row;                  // [max_det]
    // (a row's claim is written and read back by one thread only: it lives in HBM, and the workgroup asks a compute unit
    // for 12 bytes of LDS per column, not 16 -- 96 KB at 8192, which fits beside four of k_windows' workgroups)
    int *s_claim = t.link_claim;                                                                            // [capacity]
    // (in HBM, a value another wave has just changed with an atomic is read past this CU's L1)
    auto key_of = [&](int c) {
        if constexpr (LDS_TABLES) return s_col_key[c];
        else return __hip_atomic_load(&s_col_key[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    };
    auto row_of = [&](int c) {
        if constexpr (LDS_TABLES) return s_col_row[c];
        else return __hip_atomic_load(&s_col_row[c], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    };
    __shared__ int s_scan[LINK_THREADS];
    __shared__ int s_n_used, s_n_new, s_any_dead, s_set_state[2];
    __shared__ __attribute__((aligned(16))) int s_keep[LINK_ROWS][LINK_THREADS / 64];
    const int tid = threadIdx.x;
    const int cap = t.capacity;
    if (tid == 0) RING((9ull << 40) | (unsigned)frame);    // entry (before the first load)
    const int n = *t.n_tracks, nfree0 = *t.n_free;
    int nfree_now = nfree0;        // (the register-resident path keeps the height of the free stack here)
    const int m = det_count(m_host, m_dev, t.max_det, t.err);
    LRING(0);
    if (tid == 0) { s_n_used = 0; s_n_new = 0; s_any_dead = 0; }
    for (int c = tid; c < m; c += LINK_THREADS) {
        if constexpr (LDS_TABLES) { s_col_key[c] = ~0ull; s_col_row[c] = 0x7FFFFFFF; }
        else {
            __hip_atomic_store(&s_col_key[c], ~0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(&s_col_row[c], 0x7FFFFFFF, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    // (with the tables in LDS the barriers of the claim rounds order LDS traffic only: the rows' loads and the stores of
    // the decisions stay in flight across them)
    block_sync<LDS_TABLES>();
    LRING(1);
    // rows of a large table held per thread (see the `big` branch below)
    const bool big = n > LINK_THREADS && n <= LINK_ROWS * LINK_THREADS && m > 0;
    int pa[LINK_ROWS], po[LINK_ROWS], pg[LINK_ROWS], pd[LINK_ROWS];
    unsigned long long pk[LINK_ROWS];
#pragma unroll
    for (int k = 0; k < LINK_ROWS; ++k) { pa[k] = 0; po[k] = 0; pg[k] = 0; pd[k] = 0; pk[k] = ~0ull; }

    // ---- claims: the winner of a column is the proposer with the smallest (distance, row)
    if (n > 0 && m > 0 && n <= LINK_THREADS) {
        // common case, one row per thread: everything a claim will need is fetched up front so the
        // LDS rounds below overlap the loads instead of waiting behind them
        const int r = tid;
        int c = 0, slot = 0;
        unsigned long long key = ~0ull;
        if (r < n) {
            c = t.row_arg[r];
            key = (unsigned long long)__double_as_longlong(t.row_min[r]);
            slot = t.order[r];
            atomicMin(&s_col_key[c], key);
        }
        __syncthreads();
        if (r < n && key == key_of(c)) atomicMin(&s_col_row[c], r);
        __syncthreads();
        bool won = false;
        if (r < n) {
            const bool mine = (row_of(c) == r);
            s_claim[r] = mine ? c : -1;
            t.claim_slot[slot] = mine ? c : -1;
            if (mine) t.gone[slot] = 0;
            won = mine;
        }
        const int used = __popcll(__ballot(won));          // one LDS atomic per wave, not per thread
        if ((tid & 63) == 0 && used) atomicAdd(&s_n_used, used);
    } else if (big) {
        // large tables (the 4K configuration: ~5000 rows): thread tid owns rows tid + LINK_THREADS * k.  Everything
        // the LDS rounds, the ageing and the compaction below need is requested up front and kept in
        // registers, so that a pass costs one round of loads or atomics instead of a global round trip per row chunk
        // (requesting the rows before n is known, 8192 instead of ~5000, was slower: one unit's load path is the limit)
#pragma unroll
        for (int k = 0; k < LINK_ROWS; ++k) {
            const int r = tid + k * LINK_THREADS;
            if (r < n) {
                pa[k] = t.row_arg[r];
                pk[k] = (unsigned long long)__double_as_longlong(t.row_min[r]);
                po[k] = t.order[r];
                pg[k] = t.row_gone[r];
            }
        }
#ifdef YSMR_STAMPS
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        LRING(7);          // the rows' loads have landed
#endif
#pragma unroll
        for (int k = 0; k < LINK_ROWS; ++k)
            if (tid + k * LINK_THREADS < n) atomicMin(&s_col_key[pa[k]], pk[k]);
        block_sync<LDS_TABLES>();
        LRING(8);
#pragma unroll
        for (int k = 0; k < LINK_ROWS; ++k) {
            const int r = tid + k * LINK_THREADS;
            if (r < n && pk[k] == key_of(pa[k])) atomicMin(&s_col_row[pa[k]], r);
        }
        block_sync<LDS_TABLES>();
        LRING(9);
        int used = 0;
#pragma unroll
        for (int k = 0; k < LINK_ROWS; ++k) {
            const int r = tid + k * LINK_THREADS;
            const bool mine = r < n && row_of(pa[k]) == r;
            used += __popcll(__ballot(mine));
            if (r >= n) continue;
            if (claim_out) s_claim[r] = mine ? pa[k] : -1;
            if (mine) {
                t.gone[po[k]] = 0;
                pg[k] = -1;          // claimed (ageing below skips it; claim_row below)
            }
        }
        if ((tid & 63) == 0 && used) atomicAdd(&s_n_used, used);   // one LDS atomic per wave (1024 on one address: 3 us)
    } else if (n > 0 && m > 0) {
        for (int r = tid; r < n; r += LINK_THREADS)
            atomicMin(&s_col_key[t.row_arg[r]], (unsigned long long)__double_as_longlong(t.row_min[r]));
        __syncthreads();
        for (int r = tid; r < n; r += LINK_THREADS) {
            int c = t.row_arg[r];
            if ((unsigned long long)__double_as_longlong(t.row_min[r]) == key_of(c)) atomicMin(&s_col_row[c], r);
        }
        __syncthreads();
        int used = 0;
        for (int r = tid; r < n; r += LINK_THREADS) {
            int c = t.row_arg[r];
            int mine = (row_of(c) == r) ? c : -1;
            const int slot = t.order[r];
            s_claim[r] = mine;
            t.claim_slot[slot] = mine;
            if (mine >= 0) {
                t.gone[slot] = 0;
                ++used;
            }
        }
        if (used) atomicAdd(&s_n_used, used);
    } else {
        for (int r = tid; r < n; r += LINK_THREADS) { s_claim[r] = -1; t.claim_slot[t.order[r]] = -1; }
    }
    block_sync<LDS_TABLES>();      // (s_n_used; what the paths above stored in global memory is read back by no other thread)

    LRING(2);
    // ---- ageing (tracker.py:95-107, 198-211): only when there are no detections or N >= M
    const bool age = (m == 0) || (n > 0 && n >= m);
    if (age && big) {
#pragma unroll
        for (int k = 0; k < LINK_ROWS; ++k) {
            const int r = tid + k * LINK_THREADS;
            if (r >= n) continue;
            int d = 0;
            if (pg[k] >= 0) {            // not claimed this frame
                const int slot = po[k], g = pg[k] + 1;
                t.gone[slot] = g;
                t.info[slot] = 0.f; t.info[cap + slot] = 0.f; t.info[2 * cap + slot] = 0.f;
                if ((double)g > t.max_gone) { d = 1; s_any_dead = 1; }
            }
            pd[k] = d;
        }
    } else if (age) {
        for (int r = tid; r < n; r += LINK_THREADS) {
            int d = 0;
            if (s_claim[r] < 0) {
                int slot = t.order[r];
                int g = t.gone[slot] + 1;
                t.gone[slot] = g;
                t.info[slot] = 0.f; t.info[cap + slot] = 0.f; t.info[2 * cap + slot] = 0.f;
                if ((double)g > t.max_gone) { d = 1; s_any_dead = 1; }
            }
            t.dead[r] = d;
        }
    }
    block_sync<true>();            // (s_any_dead; a row's `dead` flag is read back by the thread that wrote it)

    LRING(3);
    // ---- stable compaction of the ordered track table
    int n_live = n;
    if (s_any_dead && big) {
        // one pass: every wave counts its survivors chunk by chunk (a ballot each), ONE barrier, every thread adds up the
        // counts in front of its rows (the chunk-by-chunk scan took two barriers per 1024 rows).  In place: every row's
        // slot has been in registers since the start
        // The slots of the dead go on the free stack in row order, ranked the same way (a returning global atomic per
        // dead row was a round trip to HBM inside this phase).  Nothing written here is read again in this launch: ageing
        // happens when n >= m, registration -- the reader of the free stack -- when n < m.
        const int lane = tid & 63, w = tid >> 6;
        const unsigned long long below = (1ull << lane) - 1ull;
        unsigned long long bal[LINK_ROWS], dbal[LINK_ROWS];
#pragma unroll
        for (int k = 0; k < LINK_ROWS; ++k) {
            const int r = tid + k * LINK_THREADS;
            bal[k] = __ballot(r < n && !pd[k]);
            dbal[k] = __ballot(r < n && pd[k]);
            if (lane == 0) s_keep[k][w] = __popcll(bal[k]) | (__popcll(dbal[k]) << 16);
        }
        block_sync<true>();
        int base = 0, dbase = 0;
#pragma unroll
        for (int k = 0; k < LINK_ROWS; ++k) {
            const int r = tid + k * LINK_THREADS;
            int before = 0, all = 0;
            static_assert((LINK_THREADS / 64) % 4 == 0, "16-byte reads of the waves' counts");
#pragma unroll
            for (int q4 = 0; q4 < LINK_THREADS / 64 / 4; ++q4) {
                const int4 c = reinterpret_cast<const int4 *>(s_keep[k])[q4];
                const int cs[4] = {c.x, c.y, c.z, c.w};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    before += 4 * q4 + e < w ? cs[e] : 0;
                    all += cs[e];
                }
            }
            if (r < n) {
                if (!pd[k]) {
                    const int at = base + (before & 0xFFFF) + __popcll(bal[k] & below);
                    t.order[at] = po[k];
                    t.claim_row[at] = pg[k] == -1 ? pa[k] : -1;
                } else t.free_slots[nfree0 + dbase + (before >> 16) + __popcll(dbal[k] & below)] = po[k];
            }
            base += all & 0xFFFF;
            dbase += all >> 16;
        }
        n_live = base;
        nfree_now = nfree0 + dbase;
        if (tid == 0) *t.n_free = nfree_now;
    } else if (big) {              // nobody died: the rows stay where they are
#pragma unroll
        for (int k = 0; k < LINK_ROWS; ++k) {
            const int r = tid + k * LINK_THREADS;
            if (r < n) t.claim_row[r] = pg[k] == -1 ? pa[k] : -1;
        }
    } else if (s_any_dead) {
        int base = 0;
        for (int r0 = 0; r0 < n; r0 += LINK_THREADS) {
            int r = r0 + tid;
            int keep = (r < n && !t.dead[r]) ? 1 : 0;
            const int slot_r = r < n ? t.order[r] : 0;   // read before the scan's barriers: the writes below go to rows
            int total;                                   // at or before this chunk's, all of them read by then
            int ex = block_exclusive_scan(keep, s_scan, &total);
            if (keep) t.order[base + ex] = slot_r;
            if (r < n && !keep) {
                int k = atomicAdd(t.n_free, 1);
                t.free_slots[k] = slot_r;
            }
            base += total;
        }
        n_live = base;
        __threadfence_block();
        __syncthreads();
    }

    LRING(4);
    // ---- registration (tracker.py:135-137, 212-217)
    if (m > 0 && (n == 0 || n < m)) {
        if (n == 0) {
            for (int c = tid; c < m; c += LINK_THREADS) t.new_cols[c] = c;
            if (tid == 0) s_n_new = m;
        } else {
            // unused columns in ascending order (parallel), then CPython's set order (one thread)
            int base = 0;
            for (int c0 = 0; c0 < m; c0 += LINK_THREADS) {
                int c = c0 + tid;
                int un = (c < m && row_of(c) == 0x7FFFFFFF) ? 1 : 0;
                int total;
                int ex = block_exclusive_scan(un, s_scan, &total);
                if (un) t.unused[base + ex] = c;
                base += total;
            }
            __threadfence_block();
            __syncthreads();
            int cnt = -1;
            if constexpr (LDS_TABLES) {
                // (the claim tables are dead from here on: of the 8 B per column of the key table, 4 hold the set model's
                // table of max_det slots and 2 the staged list; the 4 B per column of the row table hold its resize list)
                uint32_t *tab = reinterpret_cast<uint32_t *>(s_dyn);
                unsigned short *stage = reinterpret_cast<unsigned short *>(tab + t.max_det);
                uint32_t *list = reinterpret_cast<uint32_t *>(s_dyn + t.max_det);
                if (t.max_det < 65535)
                    cnt = cpython_order_block(t.unused, base, m, s_n_used, t.new_cols, tab, t.max_det, list, stage, s_scan,
                                              s_set_state);
            }
            if (cnt >= 0) {
                if (tid == 0) s_n_new = cnt;
            } else if (tid == 0) {
                cnt = cpython_unused_order(t, m, s_n_used, base, t.new_cols);
                if (cnt < 0) { atomicOr(t.err, ERR_TRACK_CAPACITY); cnt = 0; }
                s_n_new = cnt;
            }
        }
        __threadfence_block();
        __syncthreads();
        int n_new = s_n_new;
        if (n_live + n_new > cap) {
            if (tid == 0) atomicOr(t.err, ERR_TRACK_CAPACITY);
            n_new = cap - n_live;
        }
        const int nfree = big ? nfree_now : *t.n_free;     // (the other paths push the dead with global atomics)
        const int id0 = *t.next_id;
        for (int j = tid; j < n_new; j += LINK_THREADS) {
            int c = t.new_cols[j];
            int slot = t.free_slots[nfree - 1 - j];
            t.order[n_live + j] = slot;
            t.id[slot] = id0 + j;
            t.pos[slot] = (double)det[(size_t)c * 5 + 0];
            t.pos[cap + slot] = (double)det[(size_t)c * 5 + 1];
            if constexpr (D3) th.pos3[slot] = th.det3[c];
            t.info[slot] = (float)det[(size_t)c * 5 + 2];
            t.info[cap + slot] = (float)det[(size_t)c * 5 + 3];
            t.info[2 * cap + slot] = (float)det[(size_t)c * 5 + 4];
            t.gone[slot] = 0;
            t.claim_slot[slot] = -1;                        // (k_track reads the position stored here)
            t.claim_row[n_live + j] = -1;
            t.rec[(size_t)slot * t.rec_stride + 0] = 0.0;   // history length, head
            t.rec[(size_t)slot * t.rec_stride + 1] = 0.0;   // mode
            if (new_cols_out) new_cols_out[j] = c;
        }
        __syncthreads();
        if (tid == 0) {
            *t.n_free = nfree - n_new;
            *t.next_id = id0 + s_n_new;  // ids are consumed even for registrations dropped on overflow
            s_n_new = n_new;
        }
        __syncthreads();
        n_live += n_new;
    }

    LRING(5);
    // ---- bookkeeping for k_track
    if (claim_out)
        for (int r = tid; r < n; r += LINK_THREADS) claim_out[r] = s_claim[r];
    if (tid == 0) {
        long long base = row_count ? *row_count : 0;
        *t.n_tracks = n_live;
        t.n_tracks[4] = big ? 1 : 0;      // claim_row is valid for this frame
        t.row_base[0] = base;
        if (rows && base + n_live > rows_capacity) atomicOr(t.err, ERR_ROWS_CAPACITY);
        if (row_count) *row_count = base + n_live;
        if (n_rows_out) *n_rows_out = n_live;
        if (n_before_out) *n_before_out = n;
        if (n_new_out) *n_new_out = s_n_new;
    }
    LRING(6);
}

// ------------------------------------------------------------------------------------------
// k_frame: the whole CentroidTracker.update of one frame in ONE launch (fused path).
//
// Every block redundantly resolves the frame's bookkeeping in LDS from the same inputs -- claims,
// ageing, which tracks die, the compacted id-ordered table, which detections become new tracks and
// in which (CPython set) order -- so no inter-block synchronisation is needed; then each WAVE
// processes one track of the NEW table: applies its claim, runs the GSFF, writes its row, and
// computes its nearest detection of the next frame.  Small per-frame arrays that one block would
// write while another still reads them (order, gone, row_min/row_arg, the counters) are
// double-buffered by frame parity: `a` is the state before this frame, `b` the state after it.
// ------------------------------------------------------------------------------------------

// LDS of k_frame.  Kept small on purpose (59 KB at capacity = max_det = 2048): a block that wants
// most of a CU's 160 KB cannot be placed while kernels of another stream hold LDS there, and the
// link waited tens of microseconds per frame for that.  Per-row inputs (slot, gone, row_arg,
// row_min) stay in the registers of the thread that owns the row instead.
struct FrameLds {
    double *gains;                 // [gain_total] LDS copy of the gain rows
    unsigned long long *col_key;   // [max_det] smallest proposing distance per column ...
    int *unused, *newcols;         //   ... reused after the claims: unused columns, registration order
    int *col_row;                  // [max_det] winning row per column
    int *cg;                       // [capacity] (claimed column + 1) | new `gone` << 16, per old row
    int *inv;                      // [capacity] new row -> old row
    int *scan;                     // [16]
    short *table;                  // 4 * FRAME_TABLE bytes: the set model's table of 32-bit slots
};


// Exclusive rank of this thread's flag among the block's flags (thread order) and their count:
// a ballot per wave, four wave counts through LDS, ONE barrier.  Consecutive calls must alternate
// between two 4-int buffers (a wave may still be reading the previous call's counts).
__device__ __forceinline__ int block_flag_rank(bool f, int *s_cnt, int *total)
{
    const unsigned long long bal = __ballot(f);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) s_cnt[w] = __popcll(bal);
    __syncthreads();
    const int c0 = s_cnt[0], c1 = s_cnt[1], c2 = s_cnt[2], c3 = s_cnt[3];
    *total = c0 + c1 + c2 + c3;
    const int before = (w > 0 ? c0 : 0) + (w > 1 ? c1 : 0) + (w > 2 ? c2 : 0);
    return before + __popcll(bal & ((1ull << lane) - 1ull));
}

// CPython order of the ascending list `unused` (see cpython_unused_order), 16-bit tables in LDS.
// All FRAME_THREADS threads call it; the model itself runs on wave 0 alone, without a block barrier inside.  One table
// of 32-bit slots (set_insert_batch) and a list: the keys of a stage go in 64 at a time; at a resize the wave writes the
// occupied slots in slot order to `list` (ballot prefix), clears the table at its new size and re-inserts the list, 64
// at a time; the final walk writes the iteration order the same way.  LDS operations of one wave execute in order, so
// nothing but program order is needed between these steps.
// Returns the number of keys, or -1 if the model would need a table larger than FRAME_TABLE.
template <int THREADS, int TABLE>
__device__ int cpython_order_lds(const int *unused, int n_unused, int m, int n_used, int *out, uint32_t *table,
                                 uint32_t *list, int *s_state)
{
    // (the thread index as a value of this call: called in a frame loop, the comparisons with it are otherwise hoisted
    // out of the loop and held in scalar registers for the whole launch)
    int tid = threadIdx.x;
    asm volatile("" : "+v"(tid));
    if (set_order_is_ascending(m, n_used)) {
        for (int k = tid; k < n_unused; k += THREADS) out[k] = unused[k];
        __syncthreads();
        return n_unused;
    }
    if (tid < 64) {
        const int lane = tid;
        unsigned mask = 7, seq = 0;
        int k = 0, fill = 0, result = 0;
        if (lane < 8) table[lane] = SET_EMPTY32;
        while (true) {
            // keys go in until the table wants to grow (setobject.c: fill*5 >= mask*3 after an add)
            const int thresh = set_growth_fill(mask);
            while (k < n_unused && fill < thresh) {
                const int b = min(64, min(n_unused - k, thresh - fill));
                set_insert_batch(table, mask, lane < b, lane < b ? (unsigned)unused[k + lane] : 0u, seq + lane);
                k += b; fill += b; seq += b;
            }
            if (fill < thresh) break;
            const unsigned newsize = set_grown_size(fill);
            if ((int)newsize > TABLE) { result = -1; break; }
            int cnt = 0;
            for (unsigned i0 = 0; i0 <= mask; i0 += 64) {   // the old table in slot order -> list
                const uint32_t e = i0 + lane <= mask ? table[i0 + lane] : SET_EMPTY32;
                const unsigned long long bal = __ballot(e != SET_EMPTY32);
                if (e != SET_EMPTY32) list[cnt + __popcll(bal & ((1ull << lane) - 1ull))] = e & 0xFFFFu;
                cnt += __popcll(bal);
            }
            for (unsigned i = lane; i < newsize; i += 64) table[i] = SET_EMPTY32;
            mask = newsize - 1;
            for (int j0 = 0; j0 < cnt; j0 += 64) {
                const int b = min(64, cnt - j0);
                set_insert_batch(table, mask, lane < b, lane < b ? list[j0 + lane] : 0u, seq + lane);
                seq += b;
            }
        }
        if (result == 0) {
            for (unsigned i0 = 0; i0 <= mask; i0 += 64) {
                const uint32_t e = i0 + lane <= mask ? table[i0 + lane] : SET_EMPTY32;
                const unsigned long long bal = __ballot(e != SET_EMPTY32);
                if (e != SET_EMPTY32) out[result + __popcll(bal & ((1ull << lane) - 1ull))] = (int)(e & 0xFFFFu);
                result += __popcll(bal);
            }
        }
        if (lane == 0) s_state[0] = result;
    }
    __syncthreads();
    const int r = s_state[0];
    __syncthreads();          // (s_state may be written again by the caller's next use)
    return r;
}

#ifdef YSMR_STAMPS
#ifndef YSMR_ST_FRAME
#define YSMR_ST_FRAME 40
#endif
#define STAMP(k) do { if (blockIdx.x == 1 && threadIdx.x == 0 && (YSMR_ST_FRAME < 64 ? (frame & 63) == YSMR_ST_FRAME : frame == YSMR_ST_FRAME)) { unsigned long long t_; asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_) :: "memory"); ((unsigned long long *)(rows + rows_capacity - 4))[k] = t_; } } while (0)
#else
#define STAMP(k) do {} while (0)
#endif

template <typename DetT, int NF, bool D3 = false>
__global__ __launch_bounds__(FRAME_THREADS) void k_frame(TrackerDev a, TrackerDev b, const DetT *__restrict__ det,
                                                         int m_host, const int32_t *m_dev, int frame, ysmr_row *rows,
                                                         long long rows_capacity, long long *row_count_ext,
                                                         int32_t *n_rows_out, int32_t *claim_out, int32_t *n_before_out,
                                                         int32_t *new_cols_out, int32_t *n_new_out,
                                                         const DetT *__restrict__ next_det, const int32_t *next_m_dev,
                                                         Third3<D3> th)
{
    extern __shared__ unsigned long long s_raw[];
    __shared__ int s_n_used, s_n_dead, s_set_state[2];
    // the link is a chain of short latency-bound kernels sharing SIMDs with throughput kernels of the
    // detection stream: let its waves win the issue arbitration
    __builtin_amdgcn_s_setprio(3);
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int cap = a.capacity, md = a.max_det;
    STAMP(0); BSTAMP(0);
#ifdef YSMR_STAMPS
    if (blockIdx.x == 0 && threadIdx.x == 0) RING((2ull << 40) | (unsigned)frame);
#endif
    // ---- round trip 1: everything that can be addressed without knowing n or m is requested
    // together with the counters (entries past n / m are stale and never used).  ONE straight-line block, the
    // counters first: every branch in here made the compiler fetch the kernel arguments it needs behind it in a
    // separate scalar load with its own wait, and the counters -- which the first decision waits for -- were requested
    // at the end of that chain of waits (4 k cycles from entry to the exit test).  (Passing what this block is addressed
    // with as eight leading pointer arguments, so that one 64-byte scalar load precedes the requests, was 6 % SLOWER end
    // to end, with or without kernel-argument preload.)
    // All counters in the same round trip: the two detection counts are read through pointers that
    // are always valid (a dummy when the count comes from the host / there is no next frame), so
    // that no load hides behind a branch and a wait
    const int32_t *m_ptr = m_host < 0 ? m_dev : a.n_tracks;
    const int32_t *mn_ptr = next_det ? next_m_dev : a.n_tracks;
    const int n_raw = *a.n_tracks, nfree_raw = *a.n_free, id0_raw = *a.next_id;
    const int m_raw = *m_ptr, mn_raw = *mn_ptr;
    const long long row_base = *a.row_base;     // (the previous frame's launch left it, or the call's k_rowmin)
    constexpr int SPEC_ROWS = 3;       // table rows tid + 256k, k < 3, are fetched before n is known
    const int i = blockIdx.x * 4 + wave;
    int so[SPEC_ROWS], sg[SPEC_ROWS], sa[SPEC_ROWS];
    unsigned long long sk[SPEC_ROWS];
#pragma unroll
    for (int k = 0; k < SPEC_ROWS; ++k) {
        const int r = min(tid + k * FRAME_THREADS, cap - 1);
        so[k] = a.order[r];
        sg[k] = a.gone[r];          // fused path: `gone` is indexed by table row, not by slot
        sa[k] = a.row_arg[r];
        sk[k] = (unsigned long long)__double_as_longlong(a.row_min[r]);
    }
    // Speculation for phase B: unless a track ahead of row i is deregistered this frame, row i of
    // the new table is row i of the old one, keeps its slot and can only claim row_arg[i].
    int slot_s = a.order[min(i, cap - 1)], c_s = a.row_arg[min(i, cap - 1)];
    FirGains<NF> G;                    // (this lane's filter gains, straight from the table: no copy of it in LDS;
    fir_gains_fetch(a, a.gains, lane, G);   //  without the filter bank the table has one readable entry and every gain is 0)
    // the next frame's detections do not depend on this frame's state either (rows past m_next
    // of the [max_det][5] frame slice are stale; rowmin_wave masks them; without a next frame this frame's are read)
    DetChunk<DetT> first;
    load_chunk(first, next_det ? next_det : det, md, 0, lane);
    const int n = __builtin_amdgcn_readfirstlane(n_raw);
    const int nfree = __builtin_amdgcn_readfirstlane(nfree_raw), id0 = __builtin_amdgcn_readfirstlane(id0_raw);
    int m = __builtin_amdgcn_readfirstlane(m_host < 0 ? m_raw : m_host);
    if (m > md) { m = md; if (blockIdx.x == 0) atomicOr(a.err, ERR_DET_CLAMPED); }
    m = max(m, 0);
    const int m_next = next_det ? max(min(__builtin_amdgcn_readfirstlane(mn_raw), md), 0) : 0;
    if ((long long)blockIdx.x * 4 >= (long long)n + m && blockIdx.x != 0) return;   // cannot own a live track
    STAMP(1);

    FrameLds L;
    L.gains = reinterpret_cast<double *>(s_raw);
    L.col_key = s_raw + a.gain_total;
    L.unused = reinterpret_cast<int *>(L.col_key);
    L.newcols = L.unused + md;
    L.col_row = reinterpret_cast<int *>(L.col_key + md);
    L.cg = L.col_row + md;
    L.inv = L.cg + cap;
    L.scan = L.inv + cap;
    L.table = reinterpret_cast<short *>(L.scan + 16);

    // ---- phase A (redundant in every block): the frame's bookkeeping
    if (tid == 0) { s_n_used = 0; s_n_dead = 0; }
    for (int c = tid; c < m; c += FRAME_THREADS) { L.col_key[c] = ~0ull; L.col_row[c] = 0x7FFFFFFF; }
    slot_s = __builtin_amdgcn_readfirstlane(i < n ? slot_s : -1);
    c_s = __builtin_amdgcn_readfirstlane((i < n && m > 0) ? c_s : -1);
    GsffState<NF> S;
    double zs0 = 0.0, zs1 = 0.0;
    [[maybe_unused]] double zs2 = 0.0, d3 = 0.0;   // (3-D handles: the track's and the claimed detection's third coordinate)
    int id_s = 0;
    float in_s[3] = {0.f, 0.f, 0.f};
    DetT dd[5] = {0, 0, 0, 0, 0};
    if (slot_s >= 0) {
        if (a.use_gsff) gsff_fetch(a, slot_s, lane, S);
        zs0 = a.pos[slot_s]; zs1 = a.pos[cap + slot_s];
        if constexpr (D3) zs2 = th.pos3[slot_s];
        id_s = a.id[slot_s];
#pragma unroll
        for (int k = 0; k < 3; ++k) in_s[k] = a.info[k * cap + slot_s];
        if (c_s >= 0) {
#pragma unroll
            for (int k = 0; k < 5; ++k) dd[k] = det[(size_t)c_s * 5 + k];
            if constexpr (D3) d3 = th.det3[c_s];
        }
    }
    // row r = tid + 256 k of the old table: from the registers above for k < SPEC_ROWS (the passes over them are
    // unrolled: picking so[k] with a run-time k was eight selects per row and pass on a wave that pays for every
    // instruction), from HBM beyond
    auto row_from_hbm = [&](int r, int &o_, int &g_, int &a_, unsigned long long &key_) {
        if (r < n) {
            o_ = a.order[r]; g_ = a.gone[r]; a_ = a.row_arg[r];
            key_ = (unsigned long long)__double_as_longlong(a.row_min[r]);
        }
    };
    __syncthreads();
    STAMP(2);
    if (n > 0 && m > 0) {   // winner of a column = proposer with the smallest (distance, row)
#pragma unroll
        for (int k = 0; k < SPEC_ROWS; ++k) {
            const int r = k * FRAME_THREADS + tid;
            if (r < n) atomicMin(&L.col_key[sa[k]], sk[k]);
        }
        for (int r0 = SPEC_ROWS * FRAME_THREADS; r0 < n; r0 += FRAME_THREADS) {
            const int r = r0 + tid;
            int o_ = 0, g_ = 0, a_ = 0; unsigned long long key_ = 0;
            row_from_hbm(r, o_, g_, a_, key_);
            if (r < n) atomicMin(&L.col_key[a_], key_);
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < SPEC_ROWS; ++k) {
            const int r = k * FRAME_THREADS + tid;
            if (r < n && sk[k] == L.col_key[sa[k]]) atomicMin(&L.col_row[sa[k]], r);
        }
        for (int r0 = SPEC_ROWS * FRAME_THREADS; r0 < n; r0 += FRAME_THREADS) {
            const int r = r0 + tid;
            int o_ = 0, g_ = 0, a_ = 0; unsigned long long key_ = 0;
            row_from_hbm(r, o_, g_, a_, key_);
            if (r < n && key_ == L.col_key[a_]) atomicMin(&L.col_row[a_], r);
        }
        __syncthreads();
    }
    STAMP(3);
    const bool age = (m == 0) || (n > 0 && n >= m);   // tracker.py:95-107, 198-211
    // claims, ageing and the stable compaction of the id-ordered table in one sweep: a row's fate is
    // known to the thread that ranks it, so nothing goes through LDS in between
    int used = 0;   // claims made by this wave's rows (wave-uniform)
    int n_keep = 0;
    auto sweep_chunk = [&](int chunk, int r, int o_, int g, int c) {
        bool mine = false, keep = false;
        if (r < n) {
            mine = (m > 0) && (L.col_row[c] == r);
            if (mine) g = 0;
            else if (age) ++g;
            keep = mine || !age || !((double)g > a.max_gone);
            L.cg[r] = (mine ? c + 1 : 0) | (g << 16);
        }
        used += __popcll(__ballot(mine));
        int total;
        const int ex = block_flag_rank(keep, L.scan + (chunk & 1) * 4, &total);
        if (keep) L.inv[n_keep + ex] = r;
        if (r < n && !keep && blockIdx.x == 0) {
            const int k = atomicAdd(&s_n_dead, 1);
            a.free_slots[nfree + k] = o_;   // entries above n_free are read by nobody this frame
        }
        n_keep += total;
    };
#pragma unroll
    for (int k = 0; k < SPEC_ROWS; ++k)
        if (k * FRAME_THREADS < n) sweep_chunk(k, k * FRAME_THREADS + tid, so[k], sg[k], sa[k]);     // (uniform)
    for (int r0 = SPEC_ROWS * FRAME_THREADS; r0 < n; r0 += FRAME_THREADS) {
        const int r = r0 + tid;
        int o_ = 0, g = 0, c = 0; unsigned long long key_ = 0;
        row_from_hbm(r, o_, g, c, key_);
        sweep_chunk(r0 / FRAME_THREADS, r, o_, g, c);
    }
    if (lane == 0 && used) atomicAdd(&s_n_used, used);   // one LDS atomic per wave, not per thread
    __syncthreads();
    STAMP(10);
    STAMP(11);
    int n_new = 0;
    if (m > 0 && (n == 0 || n < m)) {   // registration (tracker.py:135-137, 212-217)
        // (col_key is dead from here on: its space holds `unused` and `newcols`)
        if (n == 0) {
            for (int c = tid; c < m; c += FRAME_THREADS) L.newcols[c] = c;
            n_new = m;
        } else {
            int base = 0;
            for (int c0 = 0; c0 < m; c0 += FRAME_THREADS) {
                const int c = c0 + tid;
                const bool un = (c < m && L.col_row[c] == 0x7FFFFFFF);
                int total;
                const int ex = block_flag_rank(un, L.scan + 8 + ((c0 / FRAME_THREADS) & 1) * 4, &total);
                if (un) L.unused[base + ex] = c;
                base += total;
            }
            __syncthreads();
            STAMP(12);
            {
                // (col_row is dead once the unclaimed columns are listed: it holds the model's list)
                int cnt = cpython_order_lds<FRAME_THREADS, FRAME_TABLE>(L.unused, base, m, s_n_used, L.newcols, reinterpret_cast<uint32_t *>(L.table),
                                            reinterpret_cast<uint32_t *>(L.col_row), s_set_state);
                if (cnt < 0) { if (blockIdx.x == 0 && tid == 0) atomicOr(a.err, ERR_TRACK_CAPACITY); cnt = 0; }
                n_new = cnt;
            }
            __syncthreads();
            STAMP(13);
        }
        __syncthreads();
    }
    const int n_new_all = n_new;
    if (n_keep + n_new > cap) {
        if (blockIdx.x == 0 && tid == 0) atomicOr(a.err, ERR_TRACK_CAPACITY);
        n_new = cap - n_keep;
    }
    const int n_live = n_keep + n_new;

    STAMP(4); BSTAMP(1);
    // ---- phase B: one wave per track of the new table
    if (i < n_live) {
        int slot, gone, c;
        bool fresh_track = false;
        if (i < n_keep) {
            const int r = __builtin_amdgcn_readfirstlane(L.inv[i]);
            const int cg = __builtin_amdgcn_readfirstlane(L.cg[r]);
            gone = cg >> 16;
            c = (cg & 0xFFFF) - 1;
            slot = slot_s;
            if (r != i || slot_s < 0) {   // a deregistration ahead of this row moved it: fetch for real
                slot = __builtin_amdgcn_readfirstlane(a.order[r]);
                if (a.use_gsff) gsff_fetch(a, slot, lane, S);
                zs0 = a.pos[slot]; zs1 = a.pos[cap + slot];
                if constexpr (D3) zs2 = th.pos3[slot];
                id_s = a.id[slot];
#pragma unroll
                for (int k = 0; k < 3; ++k) in_s[k] = a.info[k * cap + slot];
                if (c >= 0) {
#pragma unroll
                    for (int k = 0; k < 5; ++k) dd[k] = det[(size_t)c * 5 + k];
                    if constexpr (D3) d3 = th.det3[c];
                }
            }
            if (c < 0) {
                if (age && lane < 3) a.info[lane * cap + slot] = 0.f;
            }
        } else {
            const int j = i - n_keep;
            c = __builtin_amdgcn_readfirstlane(L.newcols[j]);
            slot = __builtin_amdgcn_readfirstlane(a.free_slots[nfree - 1 - j]);
            gone = 0;
            fresh_track = true;
            id_s = id0 + j;
#pragma unroll
            for (int k = 0; k < 5; ++k) dd[k] = det[(size_t)c * 5 + k];
            if constexpr (D3) d3 = th.det3[c];
            gsff_blank(S);    // nothing of the slot's previous owner is read
            gsff_point(a, slot, S);
            if (lane == 0) a.id[slot] = id_s;
        }
        double z0 = zs0, z1 = zs1;
        if (c >= 0) {
            z0 = (double)dd[0];
            z1 = (double)dd[1];
            const DetT v = lane == 0 ? dd[2] : lane == 1 ? dd[3] : dd[4];
            if (lane < 3) a.info[lane * cap + slot] = (float)v;
        }
        double o0 = z0, o1 = z1, p0 = z0, p1 = z1;
        STAMP(5);
        if (a.use_gsff) gsff_wave(a, a.gains, slot, lane, z0, z1, fresh_track, S, G, o0, o1, p0, p1);
        else if (lane == 0) {
            a.pos[slot] = z0; a.pos[cap + slot] = z1;
            if constexpr (D3) th.pos3[slot] = c >= 0 ? d3 : zs2;
        }
        STAMP(6);
        if (lane == 0) {
            b.order[i] = slot;
            b.gone[i] = gone;
            if (rows && row_base + i < rows_capacity) {
                ysmr_row rr;
                rr.frame = frame;
                rr.track_id = id_s;
                rr.x = o0; rr.y = o1;
                if (c >= 0) {
                    rr.w = (float)dd[2]; rr.h = (float)dd[3]; rr.angle = (float)dd[4];
                } else if (age) {
                    rr.w = rr.h = rr.angle = 0.f;
                } else {
                    rr.w = in_s[0]; rr.h = in_s[1]; rr.angle = in_s[2];
                }
                rr.disappeared = gone;
                rows[row_base + i] = rr;
            }
        }
        STAMP(7);
        if constexpr (D3) {
            if (m_next > 0) rowmin_wave<DetT, true>(b, i, p0, p1, next_det, m_next, lane, first, c >= 0 ? d3 : zs2, th.next3);
        } else {
            if (m_next > 0) rowmin_wave(b, i, p0, p1, next_det, m_next, lane, first);
        }
        STAMP(8);
    }
    BSTAMP(2);
#ifdef YSMR_STAMPS
    if (blockIdx.x == 0 && threadIdx.x == 0) RING((3ull << 40) | (unsigned)frame);
#endif
    // ---- block 0 publishes the counters of the new state
    if (blockIdx.x == 0) {
        if (claim_out)
            for (int r = tid; r < n; r += FRAME_THREADS) claim_out[r] = (L.cg[r] & 0xFFFF) - 1;
        if (new_cols_out)
            for (int j = tid; j < n_new; j += FRAME_THREADS) new_cols_out[j] = L.newcols[j];
        __syncthreads();
        if (tid == 0) {
            *b.n_tracks = n_live;
            *b.next_id = id0 + n_new_all;   // ids are consumed even for registrations dropped on overflow
            *b.n_free = nfree - n_new + s_n_dead;
            b.row_base[0] = row_base + n_live;
            if (rows && row_base + n_live > rows_capacity) atomicOr(a.err, ERR_ROWS_CAPACITY);
            if (row_count_ext) *row_count_ext = row_base + n_live;
            if (n_rows_out) *n_rows_out = n_live;
            if (n_before_out) *n_before_out = n;
            if (n_new_out) *n_new_out = n_new;
        }
    }
}

#include "batch_link.h"

__global__ void k_tracker_reset(TrackerDev t)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < t.capacity) t.free_slots[i] = t.capacity - 1 - i;  // slot 0 is handed out first
    if (i == 0) { *t.n_tracks = 0; *t.next_id = 0; *t.err = 0; *t.n_free = t.capacity; }
}

// what tracker_plan.h found wrong with the arguments, as the library reports it
int plan_fail(const plan::Status &s)
{
    switch (s.what) {
    case plan::Bad::size: return ysmr::fail(YSMR_ERR_ARG, "capacity/max_det out of range: need 1 .. %d, got %d/%d", TRACKER_MAX_SIZE, s.a, s.b);
    case plan::Bad::filters: return ysmr::fail(YSMR_ERR_ARG, "number of LSFFs must be in 1..%d, got %d", s.a, s.b);
    case plan::Bad::fps: return ysmr::fail(YSMR_ERR_ARG, "fps must be positive");
    case plan::Bad::horizons:
        return ysmr::fail(YSMR_ERR_ARG, "filter horizons must be >= 1 and strictly increasing (n_min=%d n_max=%g n_f=%d)", s.a, s.x, s.b);
    case plan::Bad::horizon_max: return ysmr::fail(YSMR_ERR_ARG, "maximum horizon size %d exceeds the supported 63", s.a);
    case plan::Bad::none: break;
    }
    return YSMR_OK;
}

// One frame through the per-frame kernels.  `det` is [m][5] float (double with `f64`); the count is `m`, or *m_dev when m < 0.
struct FrameArgs {
    const void *det = nullptr;
    bool f64 = false;
    int m = -1;
    const int32_t *m_dev = nullptr;
    int frame = 0;
    ysmr_row *rows = nullptr;
    long long rows_capacity = 0;
    long long *row_count = nullptr;      // the caller's running row count (NULL: a call of its own, rows from 0)
    int32_t *n_rows = nullptr, *claim = nullptr, *n_before = nullptr, *new_cols = nullptr, *n_new = nullptr;
    const void *next_det = nullptr;      // the frame whose row minima this launch leaves behind (NULL: none)
    const int32_t *next_m_dev = nullptr;
    DetGrid grid{}, next_grid{};         // split path, 2-D: the grids over `det` and `next_det`
    const double *third = nullptr, *next_third = nullptr;    // 3-D handle: the third coordinate of `det` and `next_det`
    bool rowmin_done = false;            // the previous frame's launch left this frame's row minima (false: the first frame of
                                         // a call, or of a split-path chunk -- k_rowmin goes first)
};

template <typename DetT, bool D3>
int launch_frame_t(ysmr_tracker *t, hipStream_t st, const FrameArgs &a)
{
    const DetT *det = (const DetT *)a.det, *next_det = (const DetT *)a.next_det;
    const dim3 wgrid((t->d.capacity + 3) / 4);
    Third3<D3> th{};
    if constexpr (D3) th = {t->pos3, a.third, next_det ? a.next_third : nullptr};
    // the filter bank is unrolled at compile time: 3 covers tracking.ini's default (and 1, 2), 8 the rest (a 3-D handle has none)
    const bool wide = !D3 && t->d.n_f > 3;
    t->linked = true;
    const plan::Link path = t->frame_link();
    if (path == plan::Link::frame) {
        const TrackerDev &c = t->cur(), &n = t->nxt();
        // (a call's first frame: k_rowmin also sets the first output row -- *a.row_count in a run, 0 when it is NULL, an update)
        if (!a.rowmin_done)
            hipLaunchKernelGGL((k_rowmin<DetT, D3>), wgrid, dim3(256), 0, st, c, det, a.m, a.m_dev, 1, a.row_count, DetGrid{}, th);
        auto frame = k_frame<DetT, 3, D3>;
        if constexpr (!D3) if (wide) frame = k_frame<DetT, YSMR_MAX_FILTERS>;
        hipLaunchKernelGGL(frame, wgrid, dim3(FRAME_THREADS), t->caps.frame_lds, st, c, n, det, a.m, a.m_dev, a.frame, a.rows,
                           a.rows_capacity, a.row_count, a.n_rows, a.claim, a.n_before, a.new_cols, a.n_new, next_det, a.next_m_dev, th);
        t->par ^= 1;
    } else {
        const TrackerDev &d = t->d;
        if (!a.rowmin_done)
            hipLaunchKernelGGL((k_rowmin<DetT, D3>), wgrid, dim3(256), 0, st, d, det, a.m, a.m_dev, 0, nullptr, a.grid, th);
        const size_t link_lds = t->caps.link_lds_bytes;
#ifdef YSMR_TUNING
        static const bool hbm_tables = getenv("YSMR_LINK_TABLES") && !strcmp(getenv("YSMR_LINK_TABLES"), "hbm");
#else
        const bool hbm_tables = false;
#endif
        const bool lds_tables = t->caps.link_lds && (D3 || !hbm_tables);     // (the tuning hook is 2-D only)
        auto link = k_link<DetT, true, D3>;
        if (!lds_tables) link = k_link<DetT, false, D3>;
        hipLaunchKernelGGL(link, dim3(1), dim3(LINK_THREADS), lds_tables ? link_lds : 0, st, d, det, a.m, a.m_dev, a.frame, a.rows,
                           a.rows_capacity, a.row_count, a.n_rows, a.claim, a.n_before, a.new_cols, a.n_new, th);
        if (path == plan::Link::lanes) {
            hipLaunchKernelGGL(k_track_lanes<DetT>, dim3((d.capacity + TL_THREADS - 1) / TL_THREADS), dim3(TL_THREADS), 0, st, d, t->bd,
                               t->bgains_dev, t->lanes_head, a.frame, a.rows, a.rows_capacity, det, next_det, a.next_m_dev, a.next_grid);
            t->lanes_head = (t->lanes_head + 1) & (BL_HB - 1);
        } else {
            auto track = k_track<DetT, 3, D3>;
            if constexpr (!D3) if (wide) track = k_track<DetT, YSMR_MAX_FILTERS>;
            hipLaunchKernelGGL(track, wgrid, dim3(256), 0, st, d, a.frame, a.rows, a.rows_capacity, det, next_det, a.next_m_dev,
                               a.next_grid, th);
        }
    }
    YSMR_LAUNCH_CHECK();
    return YSMR_OK;
}

int launch_frame(ysmr_tracker *t, hipStream_t st, const FrameArgs &a)
{
    if (t->dims == 3) return a.f64 ? launch_frame_t<double, true>(t, st, a) : launch_frame_t<float, true>(t, st, a);
    return a.f64 ? launch_frame_t<double, false>(t, st, a) : launch_frame_t<float, false>(t, st, a);
}

__global__ void k_peek(TrackerDev t, int32_t *ids, double *xy, int32_t *gone, int32_t *n_out)
{
    const int n = *t.n_tracks;
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0 && n_out) *n_out = n;
    if (i >= n) return;
    int slot = t.order[i];
    if (ids) ids[i] = t.id[slot];
    if (xy) { xy[2 * i] = t.pos[slot]; xy[2 * i + 1] = t.pos[t.capacity + slot]; }
    if (gone) gone[i] = t.gone[t.gone_by_row ? i : slot];
}

// the third coordinate of every track in id order (ysmr_tracker_peek3, behind k_peek)
__global__ void k_peek_third(TrackerDev t, const double *pos3, double *third)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < *t.n_tracks) third[i] = pos3[t.order[i]];
}

}  // namespace

int ysmr::fused_max_det() { return FUSED_MAX_DET; }      // for detection's grids beside the one-launch link (detect_plan.h: chain_plan)

// One wave that waits `ticks` x 10 ns (the 100 MHz realtime counter), in front of every launch of the batch link.  In the pipeline the
// event behind a link launch releases two things at the same instant: the NEXT link launch (same stream) and the detection of the
// batch whose buffers that launch was reading -- the threshold kernel's 248 workgroups, one per free compute unit, 31 per XCD.  A link
// workgroup that takes its seat while those 248 are being placed, on an XCD where the previous launch's unit is not free yet, leaves
// that XCD one unit short: one threshold workgroup then waits for another to finish its frame, and the launch takes 372-379 us instead
// of 203 -- none in most runs, every eighth launch in some (profiles/r05_thr_launch_outliers.log: always at a link boundary; with a
// 3 us wait here EVERY launch, with 6 us one run in eight, with 10 us none).  The wait lets the 248 sit down first; the link's
// workgroup then finds its XCD's spare unit.  12 us per launch of up to 256 frames (0.8 % of the link's time at the bench's size).
#ifndef BL_PAUSE_TICKS_N
#define BL_PAUSE_TICKS_N 1200
#endif
constexpr int BL_PAUSE_TICKS = BL_PAUSE_TICKS_N;
__global__ __launch_bounds__(64) void k_pause(int ticks)
{
    unsigned long long t0, t;
    asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t0)::"memory");
    do {
        __builtin_amdgcn_s_sleep(8);
        asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
    } while (t - t0 < (unsigned long long)ticks);
}

extern "C" {

int ysmr_gsff_gains(double fps, int n_min, double n_max, int n_f, int32_t *n_i_out, double *gains_out)
{
    int n_i[YSMR_MAX_FILTERS];
    if (plan::Status s = plan::horizons(fps, n_min, n_max, n_f, n_i)) return plan_fail(s);
    if (!n_i_out) return ysmr::fail(YSMR_ERR_ARG, "n_i_out must not be NULL");
    size_t off = 0;
    for (int i = 0; i < n_f; ++i) {
        n_i_out[i] = n_i[i];
        if (gains_out) plan::closed_form_gain(n_i[i], gains_out + off);
        off += 4 * (size_t)n_i[i];
    }
    return YSMR_OK;
}

// What only the build and the device can say about a handle's capabilities: each may clear one, none sets one.
static void clear_refused(plan::Caps &q)
{
#ifdef YSMR_TUNING
    // YSMR_LINK_MODE (tuning builds only): "split" forces the two-launch path, "waves" keeps k_track (a wave per track) in it
    // for A/B runs, and anything but "batch" keeps the link per frame
    if (const char *mode_env = getenv("YSMR_LINK_MODE")) {
        if (!strcmp(mode_env, "split")) q.frame = false;
        if (strcmp(mode_env, "batch")) q.batch = false;
        if (!strcmp(mode_env, "waves")) q.lanes = false;
    }
#endif
    if (q.frame) {
        const void *variants[4] = {(const void *)k_frame<float, 3>, (const void *)k_frame<double, 3>,
                                   (const void *)k_frame<float, YSMR_MAX_FILTERS>, (const void *)k_frame<double, YSMR_MAX_FILTERS>};
        for (const void *fn : variants)
            if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)q.frame_lds) != hipSuccess) q.frame = false;
    }
    if (q.frame && q.batch &&
        hipFuncSetAttribute((const void *)k_batch, hipFuncAttributeMaxDynamicSharedMemorySize, (int)q.batch_lds) != hipSuccess)
        q.batch = false;
}

static int destroy_failed(ysmr_tracker *t, int rc)      // (rc: ysmr::fail's, its message already written)
{
    if (t->block) (void)hipFree(t->block);
    if (t->grid_block) (void)hipFree(t->grid_block);
    delete t;
    return rc;
}

// check, plan (tracker_plan.h), allocate, bind, upload
int ysmr_tracker_create(double max_disappeared, double fps, int n_min, double n_max, int n_f, int use_gsff,
                        int capacity, int max_det, const double *gains_host, ysmr_tracker **out)
{
    if (!out) return ysmr::fail(YSMR_ERR_ARG, "out must not be NULL");
    *out = nullptr;
    ysmr_tracker *t = new ysmr_tracker();
    const plan::Config &c = t->cfg;
    if (plan::Status s = plan::configure(max_disappeared, fps, n_min, n_max, n_f, use_gsff, capacity, max_det, gains_host, t->cfg,
                                         t->gains_host))
        return destroy_failed(t, plan_fail(s));
    plan::Caps &q = t->caps = plan::qualifies(c);
    t->block_bytes = plan::carve_state(nullptr, c, t->d, t->d1, t->bd, t->pos3);
    hipError_t e = hipMalloc(&t->block, t->block_bytes);
    if (e != hipSuccess) {
        t->block = nullptr;
        return destroy_failed(t, ysmr::fail(YSMR_ERR_HIP, "hipMalloc(%zu) failed: %s", t->block_bytes, hipGetErrorString(e)));
    }
    clear_refused(q);
    plan::carve_state(t->block, c, t->d, t->d1, t->bd, t->pos3);
    t->d.gone_by_row = t->d1.gone_by_row = q.frame ? 1 : 0;
    // the per-frame grids of a batch: sized here, once, for BL_MAX_BATCH frames (longer batches are cut to that); behind them the
    // affine gains of the lane kernels.  (A handle is created 2-D, in link mode 0.)
    const plan::Link own = t->link();
    const bool lane_bank = own == plan::Link::batch || own == plan::Link::lanes;
    const plan::GridBlocks g = plan::grid_blocks(q, max_det);
    if (g.blocks) {
        const size_t bytes = g.per_frame * BL_MAX_BATCH * g.blocks;
        e = hipMalloc(&t->grid_block, bytes + 256);
        if (e != hipSuccess) t->grid_block = nullptr;
        if (e == hipSuccess && lane_bank) {
            t->bgains_dev = reinterpret_cast<const BlGains *>((char *)t->grid_block + bytes);
            e = hipMemcpy((void *)t->bgains_dev, &c.bgains, sizeof(BlGains), hipMemcpyHostToDevice);
        }
        if (e != hipSuccess) return destroy_failed(t, ysmr::fail(YSMR_ERR_HIP, "hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(e)));
        t->grid_frames = BL_MAX_BATCH;
        t->bd.grid = (char *)t->grid_block;
        t->bd.grid_stride = (unsigned)g.per_frame;
    }
    e = hipMemset(t->block, 0, t->block_bytes);
    if (e == hipSuccess && own == plan::Link::lanes)      // no slot's filter state belongs to a track yet
        e = hipMemset(t->bd.i32, 0xFF, sizeof(int) * (size_t)t->bd.seat_cap);
    if (e == hipSuccess && c.gain_total)
        e = hipMemcpy((void *)t->d.gains, t->gains_host.data(), sizeof(double) * c.gain_total, hipMemcpyHostToDevice);
    if (e != hipSuccess) return destroy_failed(t, ysmr::fail(YSMR_ERR_HIP, "tracker state initialisation failed: %s", hipGetErrorString(e)));
    *out = t;
    return ysmr_tracker_reset(t, nullptr);
}

// The 3-D batch link of a handle, set up the first time link mode 2 meets three dimensions, for a handle that qualifies
// (caps.batch3: capacity 768 with max_det 2048, the pipeline's shape, does).  One that does not, or whose LDS the device
// refuses, keeps the per-frame link, silently, as 2-D handles do; after a failed allocation the next call tries again.
static int setup_batch3(ysmr_tracker *t)
{
    if (!(t->caps.frame && t->caps.batch3) || t->grid3_block) return YSMR_OK;
    const int max_det = t->d.max_det;
    if (hipFuncSetAttribute((const void *)k_batch3, hipFuncAttributeMaxDynamicSharedMemorySize, (int)t->caps.batch3_lds) != hipSuccess) {
        (void)hipGetLastError();
        t->caps.batch3 = false;
        return YSMR_OK;
    }
    const size_t per = bl3_grid_stride(max_det), grids = per * BL_MAX_BATCH * 3;
    hipError_t e = hipMalloc(&t->grid3_block, grids + sizeof(double) * (size_t)t->bd.seat_cap);
    if (e != hipSuccess) {
        t->grid3_block = nullptr;
        (void)hipGetLastError();
        return ysmr::fail(YSMR_ERR_HIP, "hipMalloc(%zu) failed: %s", grids, hipGetErrorString(e));
    }
    t->grid3_stride = (unsigned)per;
    t->seat3 = reinterpret_cast<double *>((char *)t->grid3_block + grids);
    return YSMR_OK;
}

int ysmr_tracker_dimensions(ysmr_tracker *t, int dimensions)
{
    if (!t) return ysmr::fail(YSMR_ERR_ARG, "tracker handle is NULL");
    if (dimensions != 2 && dimensions != 3) return ysmr::fail(YSMR_ERR_ARG, "a tracker links in 2 or 3 dimensions, got %d", dimensions);
    if (dimensions == 3 && t->d.use_gsff)
        return ysmr::fail(YSMR_ERR_ARG, "3 dimensions need a handle created with use_gsff = 0 (the reference's filter bank takes "
                                        "(x, y) only: its CentroidTracker raises on a third coordinate, ysmr/tracker.py:68-69, 222)");
    if (t->linked)
        return ysmr::fail(YSMR_ERR_STATE, "the dimension of a tracker is fixed with its first frame (ysmr_tracker_reset frees it)");
    if (dimensions == 3 && t->caps.frame) {
        const void *variants[2] = {(const void *)k_frame<float, 3, true>, (const void *)k_frame<double, 3, true>};
        for (const void *fn : variants)
            YSMR_HIP_CHECK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)t->caps.frame_lds));
    }
    if (dimensions == 3 && t->link_mode == 2)      // (in front of every change to the handle: a failure leaves it as it was)
        if (int rc = setup_batch3(t)) return rc;
    t->dims = dimensions;
    t->in_batch = plan::is_batch(t->link());      // (the table is empty: the same in both layouts)
    t->prepared[0] = t->prepared[1] = ysmr_tracker::Prepared();
    return YSMR_OK;
}

int ysmr_tracker_reset(ysmr_tracker *t, void *stream)
{
    if (!t) return ysmr::fail(YSMR_ERR_ARG, "tracker handle is NULL");
    int n = t->d.capacity > t->d.max_det ? t->d.capacity : t->d.max_det;
    t->par = 0;
    t->prepared[0] = t->prepared[1] = ysmr_tracker::Prepared();
    if (t->frame_link() == plan::Link::lanes) {      // (ids start over: a slot's old filter state must not pass for the new track 0's)
        YSMR_HIP_CHECK(hipMemsetAsync(t->bd.i32, 0xFF, sizeof(int) * (size_t)t->bd.seat_cap, (hipStream_t)stream));
        t->lanes_head = 0;
    }
    t->in_batch = plan::is_batch(t->link());      // (an empty table is the same in both layouts)
    t->linked = false;
    hipLaunchKernelGGL(k_tracker_reset, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, t->d);
    YSMR_LAUNCH_CHECK();
    return YSMR_OK;
}

int ysmr_tracker_destroy(ysmr_tracker *t)
{
    if (!t) return YSMR_OK;
    hipError_t e = hipFree(t->block);
    if (t->grid_block) (void)hipFree(t->grid_block);
    if (t->grid3_block) (void)hipFree(t->grid3_block);
    delete t;
    if (e != hipSuccess) return ysmr::fail(YSMR_ERR_HIP, "hipFree failed: %s", hipGetErrorString(e));
    return YSMR_OK;
}

// where the state rests: the seat-major arrays of the batch link, or the per-slot layout of the per-frame kernels
static int state_to_std(ysmr_tracker *t, hipStream_t st)
{
    // a binned block is matched by the addresses of its detections alone: once a frame is linked by the per-frame kernels
    // (this function is in front of every such call) the caller may refill that buffer without preparing it again, and a
    // later batch run must not take the old binning for the new contents
    t->prepared[0] = t->prepared[1] = ysmr_tracker::Prepared();
    if (!t->in_batch) return YSMR_OK;
    hipLaunchKernelGGL(k_to_std, dim3((std::max(t->d.capacity, t->bd.seat_cap) + 255) / 256), dim3(256), 0, st, t->d, t->bd,
                       t->dims == 3 ? t->pos3 : nullptr, t->dims == 3 ? t->seat3 : nullptr);
    YSMR_LAUNCH_CHECK();
    t->in_batch = false;
    t->par = 0;
    return YSMR_OK;
}
static int state_to_batch(ysmr_tracker *t, hipStream_t st)
{
    if (t->in_batch) return YSMR_OK;
    hipLaunchKernelGGL(k_to_batch, dim3((t->bd.seat_cap + 255) / 256), dim3(256), 0, st, t->cur(), t->bd,
                       t->dims == 3 ? t->pos3 : nullptr, t->dims == 3 ? t->seat3 : nullptr);
    YSMR_LAUNCH_CHECK();
    if (t->par) {      // the counters live in the parity-0 words from here on
        YSMR_HIP_CHECK(hipMemcpyAsync(t->d.n_tracks, t->d1.n_tracks, sizeof(int) * 2, hipMemcpyDeviceToDevice, st));
    }
    t->in_batch = true;
    t->par = 0;
    return YSMR_OK;
}

int ysmr_tracker_link_mode(ysmr_tracker *t, int mode)
{
    if (!t) return ysmr::fail(YSMR_ERR_ARG, "tracker handle is NULL");
    if (mode < 0 || mode > 2)
        return ysmr::fail(YSMR_ERR_ARG, "link mode must be 0 (the library's choice), 1 (per-frame launches) or 2 (as 0, and the batch "
                                        "launch for a 3-D handle as well)");
    if (t->link_mode != mode) t->prepared[0] = t->prepared[1] = ysmr_tracker::Prepared();
    if (mode == 2 && t->dims == 3)
        if (int rc = setup_batch3(t)) return rc;
    t->link_mode = mode;       // (the state changes its layout at the next call that needs the other one)
    return YSMR_OK;
}

#ifdef YSMR_STAMPS
int ysmr_debug_read_bstamps(unsigned long long *out) { return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_bstamps), sizeof(unsigned long long) * BL_WAVES * 16); }
int ysmr_debug_read_bcounts(unsigned long long *out) { return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_bcounts), sizeof(unsigned long long) * BL_WAVES * BL_COUNTS); }
int ysmr_debug_read_bwaves(unsigned long long *out) { return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_bwaves), sizeof(unsigned long long) * (BL_WAVES + 1)); }
int ysmr_debug_read_bseats(unsigned long long *out) { return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_bseats), sizeof(unsigned long long) * 2); }
int ysmr_debug_read_brefresh(unsigned long long *out) { return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_brefresh), sizeof(unsigned long long) * BL_WAVES * 4); }
int ysmr_debug_read_bsteady(unsigned long long *out) { return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_bsteady), sizeof(unsigned long long) * BL_WAVES * 16); }
#endif

int ysmr_tracker_batched(ysmr_tracker *t) { return t && plan::is_batch(t->link()) ? 1 : 0; }

// Test hooks for the ring (tests/test_gpu_batch_bookkeeping.py; not part of the ABI the host code binds).  _poison: every
// entry of positions 0 .. BL_HB - 1 becomes a NaN bit pattern (all ones) -- refused once the handle has registered a track: whatever a
// filter bank then sums that its own frames did not store shows in the rows.  For handles that STAY in the batch layout:
// k_to_std copies whole ring columns into the per-frame history, whose FIR (fir_wave_all) multiplies the entries beyond a
// young track's history by gains of zero -- zeros in a fresh handle, NaN x 0 in a poisoned one; the first update() behind a
// poisoned batch launch ended in an illegal memory access on the device (how the NaN position becomes an address out of
// bounds in the per-frame kernels was not traced, and the parent was not run that way).  _zero_line: the non-zero 64-bit words of
// position BL_HB, the line of zeros (read-only).  Both wait for the device before and after.
int ysmr_debug_ring_poison(ysmr_tracker *t)
{
    if (!t) return ysmr::fail(YSMR_ERR_ARG, "tracker handle is NULL");
    hipError_t e = hipDeviceSynchronize();
    int seen[2] = {0, 0};      // (live tracks, next id: a handle that has registered a track keeps its ring)
    if (e == hipSuccess) e = hipMemcpy(seen, t->cur().n_tracks, sizeof(seen), hipMemcpyDeviceToHost);
    if (e == hipSuccess && (seen[0] != 0 || seen[1] != 0))
        return ysmr::fail(YSMR_ERR_ARG, "ysmr_debug_ring_poison is for a handle that has held no track yet");
    if (e == hipSuccess) e = hipMemset(t->bd.ring, 0xFF, sizeof(double2) * BL_HB * (size_t)t->bd.seat_cap);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    return e == hipSuccess ? YSMR_OK : ysmr::fail(YSMR_ERR_HIP, "ring poison failed: %s", hipGetErrorString(e));
}
// Test hooks for the seats (tests/test_gpu_seat_compaction.py; not part of the ABI either).  The last k_batch launch's
// frames that gave up track waves and the tracks they moved; the highest wave that held a track when it ended, + 1.  Three
// words behind the ring's head, which the launch writes.  Both wait for the device first.
static int seat_words(ysmr_tracker *t, int (&w)[3])
{
    if (!t) return ysmr::fail(YSMR_ERR_ARG, "tracker handle is NULL");
    hipError_t e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(w, t->bd.head + 1, sizeof(w), hipMemcpyDeviceToHost);
    return e == hipSuccess ? YSMR_OK : ysmr::fail(YSMR_ERR_HIP, "seat words read failed: %s", hipGetErrorString(e));
}
int ysmr_debug_seat_events(ysmr_tracker *t, int *events_out, int *moved_out)
{
    int w[3];
    if (!events_out || !moved_out) return ysmr::fail(YSMR_ERR_ARG, "events_out and moved_out must be set");
    if (int rc = seat_words(t, w)) return rc;
    *events_out = w[0]; *moved_out = w[1];
    return YSMR_OK;
}
int ysmr_debug_track_waves(ysmr_tracker *t, int *out)
{
    int w[3];
    if (!out) return ysmr::fail(YSMR_ERR_ARG, "out must be set");
    if (int rc = seat_words(t, w)) return rc;
    *out = w[2];
    return YSMR_OK;
}
int ysmr_debug_ring_zero_line(ysmr_tracker *t, long long *nonzero)
{
    if (!t || !nonzero) return ysmr::fail(YSMR_ERR_ARG, "tracker handle and nonzero must be set");
    std::vector<unsigned long long> line(2 * (size_t)t->bd.seat_cap);
    hipError_t e = hipDeviceSynchronize();
    if (e == hipSuccess)
        e = hipMemcpy(line.data(), t->bd.ring + (size_t)BL_HB * t->bd.seat_cap, sizeof(double2) * (size_t)t->bd.seat_cap, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return ysmr::fail(YSMR_ERR_HIP, "ring read failed: %s", hipGetErrorString(e));
    *nonzero = 0;
    for (unsigned long long w : line) *nonzero += w != 0;
    return YSMR_OK;
}

// Test hook for the grid blocks (tests/test_gpu_cell_lists_split.py): the block k_bgrid left for frame `frame` of the batch
// last prepared into `slot` (ysmr_tracker_prepare), the first `bytes` of it (at most the handle's bytes per frame: header,
// cell starts, centres, columns, lists, overflow area -- batch_link.h).  Waits for the device first.
int ysmr_debug_read_grid_block(ysmr_tracker *t, int slot, int frame, void *out, size_t bytes)
{
    if (!t || !out) return ysmr::fail(YSMR_ERR_ARG, "tracker handle and out must be set");
    if (t->link() != plan::Link::batch) return ysmr::fail(YSMR_ERR_STATE, "the handle has no batch link: no grid blocks");
    if (slot < 0 || slot > 1 || t->prepared[slot].batch <= 0 || frame < 0 || frame >= t->prepared[slot].batch || bytes > t->bd.grid_stride)
        return ysmr::fail(YSMR_ERR_ARG, "slot 0 or 1 with a prepared batch, a frame of that batch, at most %u bytes", t->bd.grid_stride);
    hipError_t e = hipDeviceSynchronize();
    if (e == hipSuccess)
        e = hipMemcpy(out, t->bd.grid + ((size_t)slot * BL_MAX_BATCH + (size_t)frame) * t->bd.grid_stride, bytes, hipMemcpyDeviceToHost);
    return e == hipSuccess ? YSMR_OK : ysmr::fail(YSMR_ERR_HIP, "grid block read failed: %s", hipGetErrorString(e));
}

// The handle's batch-link arrays with grid block `block` of its dimension: 0, 1 are ysmr_tracker_prepare's callers', 2 is run's own.
static BatchDev batch_dev(const ysmr_tracker *t, int block)
{
    BatchDev bd = t->bd;
    if (t->dims == 3) { bd.grid = (char *)t->grid3_block; bd.grid_stride = t->grid3_stride; }
    bd.grid += (size_t)block * BL_MAX_BATCH * bd.grid_stride;
    return bd;
}

// `batch` frames of detections binned frame by frame into a grid block (`third` is NULL for a 2-D handle)
static void bin_batch(const ysmr_tracker *t, hipStream_t st, const float *det, const double *third, const int32_t *count, int batch,
                      const BatchDev &bd)
{
    if (t->dims == 3)
        hipLaunchKernelGGL(k_bgrid3, dim3(batch), dim3(BG_THREADS), 4 * (size_t)bl3_lds_dwords_max(t->d.max_det), st, det, third, count,
                           t->d.max_det, bd.grid, bd.grid_stride);
    else
        hipLaunchKernelGGL(k_bgrid, dim3(batch), dim3(BG_THREADS), bd.grid_stride, st, det, count, t->d.max_det, bd.grid, bd.grid_stride);
}

static int tracker_prepare(ysmr_tracker *t, hipStream_t st, const float *det_dev, const double *third_dev, const int32_t *det_count_dev,
                           int batch, int slot)
{
    if (!plan::is_batch(t->link()) || batch > BL_MAX_BATCH) return YSMR_OK;       // (nothing to prepare: the run call does it all)
    bin_batch(t, st, det_dev, third_dev, det_count_dev, batch, batch_dev(t, slot));
    YSMR_LAUNCH_CHECK();
    t->prepared[slot] = ysmr_tracker::Prepared{det_dev, det_count_dev, third_dev, batch};
    return YSMR_OK;
}

int ysmr_tracker_prepare(ysmr_tracker *t, void *stream, const float *det_dev, const int32_t *det_count_dev, int batch, int slot)
{
    if (!t) return ysmr::fail(YSMR_ERR_ARG, "tracker handle is NULL");
    if (!det_dev || !det_count_dev || batch <= 0 || slot < 0 || slot > 1)
        return ysmr::fail(YSMR_ERR_ARG, "det_dev, det_count_dev must be set, batch > 0, slot 0 or 1");
    // (a 3-D handle: a no-op, as it has always been -- its binning takes the third coordinate, ysmr_tracker_prepare3)
    if (t->dims != 2) return YSMR_OK;
    return tracker_prepare(t, (hipStream_t)stream, det_dev, nullptr, det_count_dev, batch, slot);
}

int ysmr_tracker_prepare3(ysmr_tracker *t, void *stream, const float *det_dev, const double *third_dev, const int32_t *det_count_dev,
                          int batch, int slot)
{
    if (!t) return ysmr::fail(YSMR_ERR_ARG, "tracker handle is NULL");
    if (!det_dev || !third_dev || !det_count_dev || batch <= 0 || slot < 0 || slot > 1)
        return ysmr::fail(YSMR_ERR_ARG, "det_dev, third_dev, det_count_dev must be set, batch > 0, slot 0 or 1");
    if (t->dims != 3) return ysmr::fail(YSMR_ERR_STATE, "ysmr_tracker_prepare3 needs a 3-D handle (ysmr_tracker_dimensions)");
    return tracker_prepare(t, (hipStream_t)stream, det_dev, third_dev, det_count_dev, batch, slot);
}

// one frame at a time: the per-frame kernels, rows from 0 (`third` is NULL for a 2-D handle)
static int tracker_update(ysmr_tracker *t, hipStream_t st, const void *det_dev, int det_is_f64, const double *third_dev, int m,
                          const int32_t *m_dev, int32_t frame_index, ysmr_row *rows_dev, int32_t *n_rows_dev, int32_t *claim_col_dev,
                          int32_t *n_before_dev, int32_t *new_cols_dev, int32_t *n_new_dev)
{
    if (int rc = state_to_std(t, st)) return rc;
    FrameArgs a;
    a.det = det_dev; a.f64 = det_is_f64 != 0; a.third = third_dev;
    a.m = m; a.m_dev = m_dev; a.frame = frame_index;
    a.rows = rows_dev; a.rows_capacity = t->d.capacity;
    a.n_rows = n_rows_dev; a.claim = claim_col_dev; a.n_before = n_before_dev; a.new_cols = new_cols_dev; a.n_new = n_new_dev;
    return launch_frame(t, st, a);
}

int ysmr_tracker_update(ysmr_tracker *t, void *stream, const void *det_dev, int det_is_f64, int m,
                        const int32_t *m_dev, int32_t frame_index, ysmr_row *rows_dev, int32_t *n_rows_dev,
                        int32_t *claim_col_dev, int32_t *n_before_dev, int32_t *new_cols_dev, int32_t *n_new_dev)
{
    if (!t) return ysmr::fail(YSMR_ERR_ARG, "tracker handle is NULL");
    if (m < 0 && !m_dev) return ysmr::fail(YSMR_ERR_ARG, "m < 0 requires m_dev");
    if (m > t->d.max_det) return ysmr::fail(YSMR_ERR_CAPACITY, "m = %d exceeds max_det = %d", m, t->d.max_det);
    if (!det_dev && m != 0) return ysmr::fail(YSMR_ERR_ARG, "det_dev is NULL");
    if (t->dims != 2) return ysmr::fail(YSMR_ERR_STATE, "a 3-D handle is updated with ysmr_tracker_update3");
    return tracker_update(t, (hipStream_t)stream, det_dev, det_is_f64, nullptr, m, m_dev, frame_index, rows_dev, n_rows_dev,
                          claim_col_dev, n_before_dev, new_cols_dev, n_new_dev);
}

int ysmr_tracker_update3(ysmr_tracker *t, void *stream, const void *det_dev, int det_is_f64, const double *third_dev, int m,
                         const int32_t *m_dev, int32_t frame_index, ysmr_row *rows_dev, int32_t *n_rows_dev,
                         int32_t *claim_col_dev, int32_t *n_before_dev, int32_t *new_cols_dev, int32_t *n_new_dev)
{
    if (!t) return ysmr::fail(YSMR_ERR_ARG, "tracker handle is NULL");
    if (m < 0 && !m_dev) return ysmr::fail(YSMR_ERR_ARG, "m < 0 requires m_dev");
    if (m > t->d.max_det) return ysmr::fail(YSMR_ERR_CAPACITY, "m = %d exceeds max_det = %d", m, t->d.max_det);
    if ((!det_dev || !third_dev) && m != 0) return ysmr::fail(YSMR_ERR_ARG, "det_dev / third_dev is NULL");
    if (t->dims != 3) return ysmr::fail(YSMR_ERR_STATE, "ysmr_tracker_update3 needs a 3-D handle (ysmr_tracker_dimensions)");
    return tracker_update(t, (hipStream_t)stream, det_dev, det_is_f64, third_dev, m, m_dev, frame_index, rows_dev, n_rows_dev,
                          claim_col_dev, n_before_dev, new_cols_dev, n_new_dev);
}

// a batch of frames on one row buffer and the caller's running row count (`third_dev` is NULL for a 2-D handle)
static int tracker_run(ysmr_tracker *t, hipStream_t st, const float *det_dev, const double *third_dev, const int32_t *det_count_dev,
                       int batch, int32_t first_frame_index, ysmr_row *rows_dev, long long rows_capacity, long long *row_count_dev)
{
    const bool d3 = t->dims == 3;
    const size_t md = (size_t)t->d.max_det;
    t->linked = true;
    if (plan::is_batch(t->link())) {
        // one launch links the batch, cut to the BL_MAX_BATCH frames a grid block holds (3-D: link mode 2 on a handle k_batch3 serves)
        if (int rc = state_to_batch(t, st)) return rc;
        for (int f0 = 0; f0 < batch; f0 += BL_MAX_BATCH) {
            const int nb = std::min(batch - f0, BL_MAX_BATCH);
            const float *det = det_dev + (size_t)f0 * md * 5;
            const double *third = d3 ? third_dev + (size_t)f0 * md : nullptr;
            // the batch's detections binned frame by frame: by ysmr_tracker_prepare ahead of this call, or here
            int block = 2;
            for (int s = 0; s < 2; ++s) {
                const ysmr_tracker::Prepared &p = t->prepared[s];
                if (f0 == 0 && batch <= BL_MAX_BATCH && p.det == (const void *)det_dev && p.third == (const void *)third_dev &&
                    p.count == (const void *)det_count_dev && p.batch == batch) {
                    block = s;
                    t->prepared[s] = ysmr_tracker::Prepared();       // (good for one call)
                }
            }
            const BatchDev bd = batch_dev(t, block);
            if (block == 2) bin_batch(t, st, det, third, det_count_dev + f0, nb, bd);
            if (BL_PAUSE_TICKS > 0) hipLaunchKernelGGL(k_pause, dim3(1), dim3(64), 0, st, BL_PAUSE_TICKS);
            if (d3) {
                BlKernArgs3 ka;
                ka.t = t->d; ka.bd = bd; ka.det_all = det; ka.third_all = third; ka.det_count = det_count_dev + f0; ka.batch = nb;
                ka.frame0 = first_frame_index + f0; ka.rows = rows_dev; ka.rows_capacity = rows_capacity;
                ka.row_count = row_count_dev; ka.seat3 = t->seat3;
                hipLaunchKernelGGL(k_batch3, dim3(1), dim3(BL_THREADS), t->caps.batch3_lds, st, ka);
            } else {
                BlKernArgs ka;
                ka.t = t->d; ka.bd = bd; ka.det_all = det; ka.det_count = det_count_dev + f0; ka.batch = nb;
                ka.frame0 = first_frame_index + f0; ka.rows = rows_dev; ka.rows_capacity = rows_capacity;
                ka.row_count = row_count_dev; ka.gains = t->bgains_dev;
                for (int k = 0; k < 4; ++k) ka.hz[k] = (k == 0 || k < t->d.n_f) && k < BL_NF ? t->d.n_i[k] : 0x7FFFFFFF;
                hipLaunchKernelGGL(k_batch, dim3(1), dim3(BL_THREADS), t->caps.batch_lds, st, ka);
            }
            YSMR_LAUNCH_CHECK();
        }
        return YSMR_OK;
    }
    if (int rc = state_to_std(t, st)) return rc;
    // One launch per frame (or two); a frame's launch leaves the next frame's row minima.  Large 2-D tables (the split path)
    // look for them in a uniform grid over each frame's detections, built a grid block of frames at a time: the look-ahead
    // stays inside such a chunk, whose first frame gets its own k_rowmin.
    const bool grids = plan::uses_det_grids(t->link(), t->dims);
    const int chunk = grids ? t->grid_frames : batch;
    for (int f0 = 0; f0 < batch; f0 += chunk) {
        const int nb = std::min(batch - f0, chunk);
        if (grids) {
            hipLaunchKernelGGL(k_grid_build<float>, dim3(nb), dim3(1024), 0, st, det_dev + (size_t)f0 * md * 5, det_count_dev + f0,
                               t->d.max_det, (char *)t->grid_block, grid_bytes_per_frame(t->d.max_det));
            YSMR_LAUNCH_CHECK();
        }
        for (int f = 0; f < nb; ++f) {
            const size_t g = (size_t)f0 + f;
            FrameArgs a;
            a.det = det_dev + g * md * 5; a.m_dev = det_count_dev + g; a.frame = first_frame_index + (int)g;
            a.rows = rows_dev; a.rows_capacity = rows_capacity; a.row_count = row_count_dev;
            a.rowmin_done = f > 0;
            if (d3) a.third = third_dev + g * md;
            if (grids) a.grid = t->grid(f);
            if (f + 1 < nb) {
                a.next_det = det_dev + (g + 1) * md * 5; a.next_m_dev = det_count_dev + g + 1;
                if (d3) a.next_third = third_dev + (g + 1) * md;
                if (grids) a.next_grid = t->grid(f + 1);
            }
            if (int rc = launch_frame(t, st, a)) return rc;
        }
    }
    return YSMR_OK;
}

int ysmr_tracker_run(ysmr_tracker *t, void *stream, const float *det_dev, const int32_t *det_count_dev, int batch,
                     int32_t first_frame_index, ysmr_row *rows_dev, int64_t rows_capacity, int64_t *row_count_dev)
{
    if (!t) return ysmr::fail(YSMR_ERR_ARG, "tracker handle is NULL");
    if (!det_dev || !det_count_dev || !rows_dev || !row_count_dev || batch <= 0)
        return ysmr::fail(YSMR_ERR_ARG, "det_dev, det_count_dev, rows_dev, row_count_dev must be set and batch > 0");
    if (t->dims != 2) return ysmr::fail(YSMR_ERR_STATE, "a 3-D handle is run with ysmr_tracker_run3");
    return tracker_run(t, (hipStream_t)stream, det_dev, nullptr, det_count_dev, batch, first_frame_index, rows_dev,
                       (long long)rows_capacity, (long long *)row_count_dev);
}

int ysmr_tracker_run3(ysmr_tracker *t, void *stream, const float *det_dev, const double *third_dev, const int32_t *det_count_dev,
                      int batch, int32_t first_frame_index, ysmr_row *rows_dev, int64_t rows_capacity, int64_t *row_count_dev)
{
    if (!t) return ysmr::fail(YSMR_ERR_ARG, "tracker handle is NULL");
    if (!det_dev || !third_dev || !det_count_dev || !rows_dev || !row_count_dev || batch <= 0)
        return ysmr::fail(YSMR_ERR_ARG, "det_dev, third_dev, det_count_dev, rows_dev, row_count_dev must be set and batch > 0");
    if (t->dims != 3) return ysmr::fail(YSMR_ERR_STATE, "ysmr_tracker_run3 needs a 3-D handle (ysmr_tracker_dimensions)");
    return tracker_run(t, (hipStream_t)stream, det_dev, third_dev, det_count_dev, batch, first_frame_index, rows_dev,
                       (long long)rows_capacity, (long long *)row_count_dev);
}

int ysmr_tracker_fused(ysmr_tracker *t) { return t && t->link() == plan::Link::frame ? 1 : 0; }

int ysmr_tracker_peek(ysmr_tracker *t, void *stream, int32_t *ids_dev, double *xy_dev, int32_t *disappeared_dev,
                      int32_t *n_dev)
{
    if (!t) return ysmr::fail(YSMR_ERR_ARG, "tracker handle is NULL");
    if (t->in_batch)
        hipLaunchKernelGGL(k_peek_batch, dim3((t->bd.seat_cap + 255) / 256), dim3(256), 0, (hipStream_t)stream, t->d, t->bd,
                           ids_dev, xy_dev, disappeared_dev, n_dev);
    else
        hipLaunchKernelGGL(k_peek, dim3((t->d.capacity + 255) / 256), dim3(256), 0, (hipStream_t)stream, t->cur(), ids_dev,
                           xy_dev, disappeared_dev, n_dev);
    YSMR_LAUNCH_CHECK();
    return YSMR_OK;
}

int ysmr_tracker_peek3(ysmr_tracker *t, void *stream, int32_t *ids_dev, double *xy_dev, double *third_dev,
                       int32_t *disappeared_dev, int32_t *n_dev)
{
    if (!t) return ysmr::fail(YSMR_ERR_ARG, "tracker handle is NULL");
    if (t->dims != 3) return ysmr::fail(YSMR_ERR_STATE, "ysmr_tracker_peek3 needs a 3-D handle (ysmr_tracker_dimensions)");
    if (int rc = ysmr_tracker_peek(t, stream, ids_dev, xy_dev, disappeared_dev, n_dev)) return rc;
    if (third_dev) {      // (from whichever layout holds the state)
        if (t->in_batch)
            hipLaunchKernelGGL(k_peek_third_batch, dim3((t->bd.seat_cap + 255) / 256), dim3(256), 0, (hipStream_t)stream, t->d, t->bd,
                               t->seat3, third_dev);
        else
            hipLaunchKernelGGL(k_peek_third, dim3((t->d.capacity + 255) / 256), dim3(256), 0, (hipStream_t)stream, t->cur(), t->pos3,
                               third_dev);
        YSMR_LAUNCH_CHECK();
    }
    return YSMR_OK;
}

int ysmr_tracker_info(ysmr_tracker *t, void *stream, int32_t *n_tracks, int32_t *next_id, int32_t *error_bits)
{
    if (!t) return ysmr::fail(YSMR_ERR_ARG, "tracker handle is NULL");
    int host[4], err = 0;
    YSMR_HIP_CHECK(hipMemcpyAsync(host, t->cur().n_tracks, sizeof(int) * 4, hipMemcpyDeviceToHost, (hipStream_t)stream));
    YSMR_HIP_CHECK(hipMemcpyAsync(&err, t->d.err, sizeof(int), hipMemcpyDeviceToHost, (hipStream_t)stream));
    YSMR_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));
    if (n_tracks) *n_tracks = host[0];
    if (next_id) *next_id = host[1];
    if (error_bits) *error_bits = err;
    return YSMR_OK;
}

}  // extern "C"

// batch_link.h -- the link of a whole BATCH of frames in one launch (included by track.hip, inside its namespace).
//
// CentroidTracker.update (ysmr/tracker.py:93-230) + GaussianSumFIR.correct / predict (ysmr/gsff.py:204-347) + row
// emission (ysmr/track_eval.py:313-316) for `batch` consecutive frames: ONE workgroup of BL_THREADS = 768 threads on ONE
// compute unit, a track per LANE, everything a frame needs of a track -- the filter bank's window sums, weights and
// estimates, prediction, box, id, counters: 55 registers -- in the lane from the first frame of the batch to the last.
//
//   detections   k_bgrid (one workgroup per frame, the whole batch at once, before this kernel) bins every frame's
//                detections into a uniform grid of cells (counting sort) and leaves header | cell starts (u16) |
//                centres in cell order | their column numbers (u16) | candidates per cell as one contiguous block per frame; this kernel
//                brings the block of frame f+2 into LDS by LDS-DMA while it works on frames f and f+1.
//   row minimum  tracker.py:151-163 reads only D.min(1) and D.argmin(1): a lane reads the candidate list k_bgrid left for
//                its prediction's cell (every detection that can be nearest to a point of the cell, <= 8), in float, and
//                evaluates the winner once in float64 (bl_search; a cell with more candidates is served by the lists of
//                its four quadrants); outside the grid, in a cell with a quadrant that still holds more, or
//                in frames of more than 600 detections (no lists) it looks at the 3 x 3 cells around the prediction
//                (bl_search_block); what float cannot decide -- a candidate a hair from the best, a nearer detection
//                possibly outside the block -- the wave settles exactly over all detections (bl_search_wave:
//                rowmin_wave's tie rule, lowest column among equal ROUNDED distances).
//   claims       the winner of a detection column is the proposer with the smallest (distance, id).  Table rows ascend
//                with the ids, so ONE LDS atomicMin on (squared distance without its ten lowest bits, table row) settles a
//                column; a frame in which two proposals of a column come closer than that key resolves -- an exact tie,
//                mostly -- repeats the claims exactly: full distance, rounded roots, id (k_batch: "claims").
//   lifecycle    ageing / deregistration per lane; a lane that loses its track is simply free; new tracks take free
//                lanes, in CPython set order of the unclaimed columns (cpython_order_lds).  Table ROWS (the order of the
//                reference's OrderedDict = ascending id = the order of a frame's rows) are kept as a per-lane rank:
//                a death lowers the rank of every younger track by one, a birth appends.
//   filter bank  The gain of a constant-velocity least-squares filter is AFFINE in the age a of a measurement:
//                g_N[a] = alpha_N - beta_N a (closed_form_gain), so x-hat_N = alpha_N S0_N - beta_N S1_N with the window
//                sums S0_N = sum_{a<N} h[a], S1_N = sum_{a<N} a h[a].  A new measurement z turns them into
//                S1' = S1 + S0 - N h[N-1], S0' = S0 + z - h[N-1]: six sums per coordinate in registers, updated with four
//                operations each, and of the 31 measurements of history a frame touches FOUR: the one it appends and the
//                three that leave the windows.  The history therefore lives in HBM, a ring of 32 frames x 768 seats
//                (every live track appends exactly one measurement per frame, so one head serves all seats and a ring
//                position is one coalesced line per wave); the leaving entries are requested before the claims and used
//                after them.  The sums are recomputed from the ring, exactly, in every frame whose NUMBER is a multiple of
//                BL_REFRESH = 64 (not at the start of a launch: the rows must not depend on how the frames were batched),
//                so rounding drift is bounded by 64 updates: ~1e-11 px, the size of a from-scratch sum's own rounding.
//   rows         one 40-byte ysmr_row per live lane at rows[base + rank] (k_batch: rowp[rank]), fire and forget.
//
// One workgroup barrier per frame, behind the atomic round of the claims: the ranks, the row and the counts of a frame --
// all that needs every wave to be past the frame's ageing -- are settled behind the NEXT frame's barrier, and a wave goes
// from its filter bank straight into the next frame's search (k_batch, above the frame loop).  Why not the history in registers (the first build of this kernel: 158 registers per
// track): 512 tracks fill a compute unit's register file, BASELINE configs[2] holds up to 535; and a frame then costs the
// 186 float64 operations of re-summing and shifting 62 values per track, on ONE unit's float64 pipe (7.4 us per frame).
//
// Between launches the small state rests in HBM seat by seat (a seat keeps its track for the track's whole life; free
// seats are flagged), next to the ring.  k_to_std / k_to_batch convert to and from the per-slot layout of k_frame /
// k_link + k_track (ysmr_tracker_update, tables beyond this kernel's 768 seats).
#pragma once

// (BL_* constants, struct BatchDev, BlShared, and the layout and size of a frame's block and of the LDS: tracker_plan.h)
#include "tracker_plan.h"

constexpr unsigned BL_FLAG = 0xFFFFu, BL_SPLIT = 0xFFFEu;      // first u16 of a cell's slot (positions are <= 600)

// One workgroup per frame: bounding box of the centres, G x G cells over it with one cell of margin, counting sort.  The
// detections are read ONCE (up to BG_PER per thread, kept in registers through the three passes), the block is assembled
// in LDS and leaves with 16-byte stores: one round of loads and one of stores instead of the five dependent round trips of
// the first version (35 us per batch beside the next batch's detection kernels).
constexpr int BG_THREADS = 256, BG_PER = 10;      // 2560 >= FUSED_MAX_DET, the detections a one-launch link serves
constexpr int BG_CAND = 32;                       // candidates of a cell before the pruning (more: the cell is flagged)
static_assert(BG_THREADS == 4 * 64 && BL_OVF <= 64, "k_bgrid's second pass: quadrant w of overflow entry `lane` on wave w");
static_assert(BG_THREADS * BG_PER >= FUSED_MAX_DET, "k_bgrid keeps a frame's detections in registers, BG_PER per thread");

// The candidate list of cell c (G <= 32).  R = the cell's rectangle grown by e on every side: a prediction that bl_search
// places in cell c lies in R (below).  Every point p of R has a detection within U = min over d of maxdist(d, R) -- found by
// a walk over rings of cells around c, which stops once no farther ring can hold a detection nearer than that -- so only
// detections with mindist(d, R) <= U + 1 px can matter: those are gathered (ascending, row-runs of cells), then pruned.
// d is left out when another candidate d' is nearer at EVERY point of R by the margin below,
//     s_d(p) > (1 + 3e-5) s_d'(p) + 0.6 px^2        (s: squared distance),
// which is tested at the four corners only: s_d - (1 + eps) s_d' = -eps |p|^2 + (linear in p) is concave, so its minimum
// over a rectangle lies at a corner.  Such a d is not the float64 argmin of any p in R, and it lies outside bl_search's float
// tie band (s <= best + 0.2 + 5e-6 best, on float distances each off by at most 0.1 + 3e-6 s for coordinates below 4096)
// around it: s_d,f >= (1 - 3e-6) s_d - 0.1 > s_d',f (1 + 5e-6) + 0.2 needs eps > 1.2e-5 and 0.4 px^2 -- the rest covers the
// float arithmetic here (corners to ~1e-3 px: below 2e-3 + 1.3e-6 s per distance).  The same bound, in distances, sets the
// gathering's 1 px.  The pruned set is never empty (in float too, "nearer at a corner by the margin" cannot go round in a
// circle), and at most a few detections per cell survive: uniform frames of 500 detections keep <= BL_LIST in 99.7 % of cells.
// e: a prediction's cell is floor((fx - x0) * inv) in float, fx = (float)px: off by |fx - px| <= 2.4e-4 px, plus 2.4e-4 px
// for fx - x0 and ~1e-5 cells for the product -- e = 4e-3 px + 2e-4 cells covers that and the corners' own rounding here.
// A QUADRANT of a cell (split lists, below): bl_search decides it from the same float product, frac = u - floor(u) >= 0.5
// with u = (fx - x0) * inv.  The subtraction is exact (u and floor(u) are less than one apart), so the decision is
// u >= cx + 0.5 for the float u, and u is off from the prediction's true place by what sets e above: |fx - px| <= 2.4e-4 px,
// 2.4e-4 px for fx - x0, ~1e-5 cells for the product.  The midline itself, x0 + (cx + 0.5) * cell, is rounded here like a
// cell's side (cx + 0.5 is exact).  The same e = 4e-3 px + 2e-4 cells therefore covers a quadrant's rectangle, on its
// inner sides as on its outer ones -- which are the cell's own, bit for bit (cx + 0.5 + 0.5 = cx + 1).
// The walk for U and the gathering stay centred on the quadrant's CELL: U only has to be an upper bound (any detection's
// maxdist is one), and the gathering's rho carries two cells of slack where the rectangle needs none beyond its cell.
__device__ __forceinline__ void bl_rect_list(int cx, int cy, float ax, float bx, float ay, float by, float e, int G, int m, float cell,
                                             float inv, const unsigned short *start16, const float2 *xy, unsigned short *list8,
                                             unsigned short *cand)
{
    // U^2: rings 0, 1, 2, ... (a detection of ring r + 1 is at least (r + 1) cells from the rectangle's far side -- of a
    // CELL's rectangle.  From a quadrant's far side it is only (r + 0.5) cells, so for a quadrant the walk may stop a ring
    // before the true minimum: U stays an upper bound, T comes out a little larger, a few more candidates are gathered and
    // pruned again.  Kept so that a quadrant's list is the cell's procedure verbatim.)
    float u2 = 3.0e38f;
    int ju = 0;                 // the detection that sets U: tried first as the nearer one in the pruning
    auto far2 = [&](int a, int b) {
        for (int j = a; j < b; ++j) {
            const float2 d = xy[j];
            const float dx = fmaxf(fabsf(d.x - ax), fabsf(d.x - bx)), dy = fmaxf(fabsf(d.y - ay), fabsf(d.y - by));
            const float v = dx * dx + dy * dy;
            ju = v < u2 ? j : ju;
            u2 = fminf(u2, v);
        }
    };
    for (int r = 0; r < G; ++r) {
        const int xl = max(cx - r, 0), xh = min(cx + r, G - 1);
        for (int y = max(cy - r, 0); y <= min(cy + r, G - 1); ++y) {
            if (y == cy - r || y == cy + r) far2(start16[y * G + xl], start16[y * G + xh + 1]);
            else {
                if (cx - r >= 0) far2(start16[y * G + cx - r], start16[y * G + cx - r + 1]);
                if (cx + r < G) far2(start16[y * G + cx + r], start16[y * G + cx + r + 1]);
            }
        }
        const float reach = (float)(r + 1) * cell;
        if (u2 <= reach * reach) break;
    }
    // the candidates: mindist(d, R) <= T, from the cells whose float assignment can hold such a detection
    const float T = sqrtf(u2) * 1.0001f + 1.0f, T2 = T * T;
    const int rho = min((int)((T + e) * inv) + 2, G);
    int n = 0;
    for (int y = max(cy - rho, 0); y <= min(cy + rho, G - 1); ++y) {
        const int a = start16[y * G + max(cx - rho, 0)], b = start16[y * G + min(cx + rho, G - 1) + 1];
        for (int j = a; j < b; ++j) {
            const float2 d = xy[j];
            const float dx = fmaxf(fmaxf(ax - d.x, d.x - bx), 0.f), dy = fmaxf(fmaxf(ay - d.y, d.y - by), 0.f);
            if (dx * dx + dy * dy <= T2) {
                if (n < BG_CAND) cand[n * BG_THREADS] = (unsigned short)j;
                ++n;
            }
        }
    }
    // the pruning: d_i stays unless some d_k is nearer by the margin at all four corners (any detection will do as d_k;
    // the one that sets U removes most candidates at once, the others are tried after it)
    int kept = 0;
    const float2 du = xy[ju];
    const float ua = ax - du.x, ub = bx - du.x, va = ay - du.y, vb = by - du.y;
    const float eps = 1.00003f, beta = 0.6f;
    const float u0 = (ua * ua + va * va) * eps + beta, u1 = (ub * ub + va * va) * eps + beta;
    const float u2c = (ua * ua + vb * vb) * eps + beta, u3 = (ub * ub + vb * vb) * eps + beta;
    if (n <= BG_CAND)
        for (int i = 0; i < n; ++i) {
            const int ji = cand[i * BG_THREADS];
            const float2 di = xy[ji];
            const float xa = ax - di.x, xb = bx - di.x, ya = ay - di.y, yb = by - di.y;
            const float s0 = xa * xa + ya * ya, s1 = xb * xb + ya * ya, s2 = xa * xa + yb * yb, s3 = xb * xb + yb * yb;
            bool beaten = ji != ju && s0 > u0 && s1 > u1 && s2 > u2c && s3 > u3;
            // (four rivals per pass, their reads in flight together: a rival costs two dependent LDS reads, and a crowded
            // rectangle tries ~150 of them -- one after the other that was the slowest thread's tail, and the second pass
            // of the split lists would have added a tail of its own; `beaten` is an OR over the rivals, so the order is free)
            for (int k = 0; k < n && !beaten; k += 4) {
                float2 dk[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) dk[u] = xy[cand[min(k + u, n - 1) * BG_THREADS]];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const float ka = ax - dk[u].x, kb = bx - dk[u].x, la = ay - dk[u].y, lb = by - dk[u].y;
                    beaten = beaten || (k + u < n && k + u != i && s0 > (ka * ka + la * la) * eps + beta && s1 > (kb * kb + la * la) * eps + beta &&
                                        s2 > (ka * ka + lb * lb) * eps + beta && s3 > (kb * kb + lb * lb) * eps + beta);
                }
            }
            if (!beaten) {
                if (kept < BL_LIST) list8[kept] = (unsigned short)ji;
                ++kept;
            }
        }
    if (n > BG_CAND || kept > BL_LIST) list8[0] = (unsigned short)BL_FLAG;
    else
        for (int k = kept; k < BL_LIST; ++k) list8[k] = (unsigned short)m;
}
__device__ __forceinline__ void bl_cell_list(int c, int G, int m, float x0, float y0, float cell, float inv, const unsigned short *start16,
                                             const float2 *xy, unsigned short *list16, unsigned short *cand)
{
    const int cx = c % G, cy = c / G;
    const float e = 4e-3f + 2e-4f * cell;
    const float ax = x0 + (float)cx * cell - e, bx = x0 + (float)(cx + 1) * cell + e;
    const float ay = y0 + (float)cy * cell - e, by = y0 + (float)(cy + 1) * cell + e;
    bl_rect_list(cx, cy, ax, bx, ay, by, e, G, m, cell, inv, start16, xy, list16 + c * BL_LIST, cand);
}
// quadrant q = (x half) + 2 * (y half) of cell c, into list8
__device__ __forceinline__ void bl_quad_list(int c, int q, int G, int m, float x0, float y0, float cell, float inv, const unsigned short *start16,
                                             const float2 *xy, unsigned short *list8, unsigned short *cand)
{
    const int cx = c % G, cy = c / G;
    const float e = 4e-3f + 2e-4f * cell;
    const float hx = (float)cx + 0.5f * (float)(q & 1), hy = (float)cy + 0.5f * (float)(q >> 1);
    const float ax = x0 + hx * cell - e, bx = x0 + (hx + 0.5f) * cell + e;
    const float ay = y0 + hy * cell - e, by = y0 + (hy + 0.5f) * cell + e;
    bl_rect_list(cx, cy, ax, bx, ay, by, e, G, m, cell, inv, start16, xy, list8, cand);
}

// The binning of one frame by one workgroup, for the planar link (D3 = false: k_bgrid) and the 3-D link (D3 = true: k_bgrid3):
// the load of the detections, the bounding box, the cells, the counting sort, the scan, the padding, the scatter and the
// copy-out are one text for both.  The 3-D instance adds the third coordinate -- z[], `wide` / s_wide and header word 7, the
// z32 plane in the LDS part and the z64 plane in HBM (above k_bgrid3) -- and builds no candidate lists; the planar instance
// builds them (first pass, split lists, overflow area).  A __shared__ array that an instance does not touch takes no LDS in it.
template <bool D3>
__device__ __forceinline__ void bl_bin_frame(const float *__restrict__ det_all, const double *__restrict__ third_all,
                                             const int32_t *__restrict__ det_count, int max_det, char *grid, unsigned grid_stride)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t s_out[];      // the block as it will lie in HBM (3-D: its LDS part)
    __shared__ int s_cnt[64 * 64];
    __shared__ float s_red[4][4];
    __shared__ int s_wave_sum[4];
    const int f = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    __shared__ unsigned short s_cand[BG_CAND][BG_THREADS];      // a cell's candidates, per thread
    __shared__ unsigned short s_crowded[BL_OVF];                // the cells that get an overflow entry, ascending
    __shared__ int s_crowded_n;                                 // how many of them (at most BL_OVF)
    __shared__ int s_any_crowded;                               // flag: the first pass flagged a cell
    __shared__ int s_wide;                                      // 3-D: some |third| of the frame is not below 4096
    const float *det = det_all + (size_t)f * max_det * 5;
    int m = det_count[f];
    m = m < 0 ? 0 : (m > max_det ? max_det : m);
    const int G = bl_grid_n(m), cells = G * G;
    unsigned short *start16 = reinterpret_cast<unsigned short *>(s_out + 16);
    float2 *xy = reinterpret_cast<float2 *>(s_out + 16 + bl_start_dwords(G));
    unsigned short *items = reinterpret_cast<unsigned short *>(s_out + 16 + bl_start_dwords(G) + 2 * bl_mp(m));
    unsigned short *list16 = reinterpret_cast<unsigned short *>(s_out + bl_list_off(m));      // (planar)
    // (3-D: the f32 plane stands where the planar block has its lists; the f64 plane does not pass through this kernel's LDS)
    float *z32 = reinterpret_cast<float *>(s_out + bl_list_off(m));
    double *z64 = nullptr;
    if constexpr (D3) z64 = reinterpret_cast<double *>(grid + (size_t)grid_stride * f + 4 * (size_t)bl3_lds_dwords_max(max_det));
    float x[BG_PER], y[BG_PER];
    double z[BG_PER];
    bool wide = false;
#pragma unroll
    for (int k = 0; k < BG_PER; ++k) {
        const int j = tid + k * BG_THREADS;
        x[k] = j < m ? det[(size_t)j * 5] : 0.f;
        y[k] = j < m ? det[(size_t)j * 5 + 1] : 0.f;
        if constexpr (D3) {      // (a slot at or beyond the frame's count is never read)
            z[k] = j < m ? (third_all + (size_t)f * max_det)[j] : 0.0;
            wide = wide || !(fabs(z[k]) < 4096.0);
        }
    }
    for (int c = tid; c < cells; c += BG_THREADS) s_cnt[c] = 0;
    if constexpr (D3) { if (tid == 0) s_wide = 0; }
    float lo_x = 3.0e38f, lo_y = 3.0e38f, hi_x = -3.0e38f, hi_y = -3.0e38f;
#pragma unroll
    for (int k = 0; k < BG_PER; ++k)
        if (tid + k * BG_THREADS < m) { lo_x = fminf(lo_x, x[k]); hi_x = fmaxf(hi_x, x[k]); lo_y = fminf(lo_y, y[k]); hi_y = fmaxf(hi_y, y[k]); }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        lo_x = fminf(lo_x, __shfl_xor(lo_x, d)); hi_x = fmaxf(hi_x, __shfl_xor(hi_x, d));
        lo_y = fminf(lo_y, __shfl_xor(lo_y, d)); hi_y = fmaxf(hi_y, __shfl_xor(hi_y, d));
    }
    if (lane == 0) { s_red[0][w] = lo_x; s_red[1][w] = hi_x; s_red[2][w] = lo_y; s_red[3][w] = hi_y; }
    __syncthreads();
    if constexpr (D3) { if (wide) s_wide = 1; }
    lo_x = s_red[0][0]; hi_x = s_red[1][0]; lo_y = s_red[2][0]; hi_y = s_red[3][0];
    for (int k = 1; k < 4; ++k) {
        lo_x = fminf(lo_x, s_red[0][k]); hi_x = fmaxf(hi_x, s_red[1][k]);
        lo_y = fminf(lo_y, s_red[2][k]); hi_y = fmaxf(hi_y, s_red[3][k]);
    }
    if (m == 0) { lo_x = lo_y = 0.f; hi_x = hi_y = 1.f; }
    const float extent = fmaxf(fmaxf(hi_x - lo_x, hi_y - lo_y), 1.0f);
    const float cell = extent / (float)(G - 2), inv = 1.0f / cell;
    const float x0 = lo_x - cell, y0 = lo_y - cell;
    if (tid < 16) s_out[tid] = 0;
    __syncthreads();
    if (tid == 0) {
        float *h = reinterpret_cast<float *>(s_out);
        h[0] = x0; h[1] = y0; h[2] = cell; h[3] = inv;
        s_out[4] = (uint32_t)G; s_out[5] = (uint32_t)m; s_out[6] = !D3 && bl_has_lists(m) ? BL_LIST : 0;
        if constexpr (D3) s_out[7] = (uint32_t)s_wide;
    }
    int cell_of[BG_PER];
#pragma unroll
    for (int k = 0; k < BG_PER; ++k) {
        int cx = (int)floorf((x[k] - x0) * inv), cy = (int)floorf((y[k] - y0) * inv);
        cx = cx < 0 ? 0 : (cx > G - 1 ? G - 1 : cx);
        cy = cy < 0 ? 0 : (cy > G - 1 ? G - 1 : cy);
        cell_of[k] = cy * G + cx;
        if (tid + k * BG_THREADS < m) atomicAdd(&s_cnt[cell_of[k]], 1);
    }
    __syncthreads();
    // exclusive scan of the counts: K consecutive cells per thread (K = 1, 4, 9 or 16), wave scan, wave sums
    const int K = cells / BG_THREADS;
    int local[16], sum = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k)
        if (k < K) { local[k] = sum; sum += s_cnt[tid * K + k]; }
    int incl = sum;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const int o = __shfl_up(incl, d); if (lane >= d) incl += o; }
    if (lane == 63) s_wave_sum[w] = incl;
    __syncthreads();
    int before = incl - sum;
    for (int k = 0; k < w; ++k) before += s_wave_sum[k];
#pragma unroll
    for (int k = 0; k < 16; ++k)
        if (k < K) {
            const int at = before + local[k];
            s_cnt[tid * K + k] = at;
            start16[tid * K + k] = (unsigned short)at;
        }
    if (tid == BG_THREADS - 1) { start16[cells] = (unsigned short)m; start16[cells + 1] = 0; }
    // (the padding of the lists reads as far away, should a lane ever look at it)
    for (int j = m + tid; j < bl_mp(m); j += BG_THREADS) {
        xy[j] = make_float2(1.0e30f, 1.0e30f); items[j] = 0;
        if constexpr (D3) { z32[j] = 0.f; z64[j] = 0.0; }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < BG_PER; ++k) {
        const int j = tid + k * BG_THREADS;
        if (j < m) {
            const int at = atomicAdd(&s_cnt[cell_of[k]], 1);
            items[at] = (unsigned short)j;
            xy[at] = make_float2(x[k], y[k]);
            if constexpr (D3) { z32[at] = (float)z[k]; z64[at] = z[k]; }      // (rounded into the LDS part, as given into the tail)
        }
    }
    if (!D3 && bl_has_lists(m)) {      // (the overflow area starts as zeros; "no crowded cell yet")
        for (int i = tid; i < BL_OVF * 4 * BL_LIST / 2; i += BG_THREADS) s_out[bl_ovf_off(m) + i] = 0;
        if (tid == 0) s_any_crowded = 0;
    }
    __syncthreads();
    if constexpr (!D3) {      // the candidate lists: first pass, split lists, overflow area
        unsigned short *ovf16 = reinterpret_cast<unsigned short *>(s_out + bl_ovf_off(m));      // (frames with lists only)
        if (bl_has_lists(m) && m > 0) {
            for (int c = tid; c < cells; c += BG_THREADS) {
                bl_cell_list(c, G, m, x0, y0, cell, inv, start16, xy, list16, &s_cand[0][tid]);
                if (list16[c * BL_LIST] == BL_FLAG) s_any_crowded = 1;     // (the second pass runs)
            }
            __syncthreads();
        }
        if (bl_has_lists(m) && m > 0 && s_any_crowded) {         // (uniform: read behind the barrier)
            // Split lists.  The crowded cells (flagged above) are compacted in cell order -- K consecutive cells per thread, the
            // scan of the counts again -- and the first BL_OVF of them get an overflow entry each; the (entry, quadrant) items
            // then go out over the workgroup, one per thread: the thread that owned a crowded cell was the slowest of the first
            // pass already, and four more lists in a row behind it would be the kernel's tail.
            int mine = 0;
#pragma unroll
            for (int k = 0; k < 16; ++k)
                if (k < K) mine += list16[(tid * K + k) * BL_LIST] == BL_FLAG;
            int inc2 = mine;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) { const int o = __shfl_up(inc2, d); if (lane >= d) inc2 += o; }
            if (lane == 63) s_wave_sum[w] = inc2;      // (its readers of the first scan are barriers back)
            __syncthreads();
            int at = inc2 - mine;
            for (int k = 0; k < w; ++k) at += s_wave_sum[k];
            if (mine)
                for (int k = 0; k < K; ++k)
                    if (list16[(tid * K + k) * BL_LIST] == BL_FLAG) {
                        if (at < BL_OVF) s_crowded[at] = (unsigned short)(tid * K + k);
                        ++at;
                    }
            if (tid == BG_THREADS - 1) s_crowded_n = min(at, BL_OVF);
            __syncthreads();
            const int entries = s_crowded_n;
            // (quadrant w of entry `lane` on wave w: a wave's lanes run their lists in lockstep, every lane through every other
            // lane's loops, so the items are spread over the four waves rather than packed into the first)
            if (lane < entries)
                bl_quad_list(s_crowded[lane], w, G, m, x0, y0, cell, inv, start16, xy, ovf16 + (4 * lane + w) * BL_LIST, &s_cand[0][tid]);
            __syncthreads();
            if (tid < entries) {
                bool fits = true;
                for (int q = 0; q < 4; ++q) fits = fits && ovf16[(4 * tid + q) * BL_LIST] != BL_FLAG;
                // (the slot's first dword: the marker and the entry; a cell with a quadrant that still overflows keeps its flag)
                if (fits) reinterpret_cast<uint32_t *>(list16)[s_crowded[tid] * (BL_LIST / 2)] = BL_SPLIT | ((uint32_t)tid << 16);
            }
            __syncthreads();
        }
    }
    uint4 *out = reinterpret_cast<uint4 *>(grid + (size_t)grid_stride * f);
    const uint4 *img = reinterpret_cast<const uint4 *>(s_out);
    for (int i = tid; i < (D3 ? bl3_lds_dwords(m) : bl_grid_dwords(m)) / 4; i += BG_THREADS) out[i] = img[i];
}

__global__ __launch_bounds__(BG_THREADS) void k_bgrid(const float *__restrict__ det_all, const int32_t *__restrict__ det_count,
                                                      int max_det, char *grid, unsigned grid_stride)
{
    bl_bin_frame<false>(det_all, nullptr, det_count, max_det, grid, grid_stride);
}

// ---- a track in registers -------------------------------------------------------------------------------------------
struct BlSeat {
    double s0x[BL_NF], s1x[BL_NF], s0y[BL_NF], s1y[BL_NF];   // window sums of the three horizons (x, y)
    double w[BL_NF], xa[BL_NF], xb[BL_NF];                   // filter weights, x-hat rows 0 / 1
    double px, py;                                           // CentroidTracker.objects[id]: the prediction (tracker.py:225)
    float info[3];
    int id, gone, len, mode, rank;
    bool alive;
};
// rest format, seat-major: f64 [BL_SF64][seat_cap] = w, xa, xb, px, py, the twelve window sums; f32 [3][seat_cap];
// i32 [6][seat_cap] = id, gone, history length, mode, rank, alive; ring double2 [BL_HB + 1][seat_cap] (the last line: zeros, never stored to)

__device__ __forceinline__ void bl_seat_blank(BlSeat &S)
{
#pragma unroll
    for (int f = 0; f < BL_NF; ++f) { S.s0x[f] = S.s1x[f] = S.s0y[f] = S.s1y[f] = 0.0; S.w[f] = S.xa[f] = S.xb[f] = 0.0; }
    S.px = S.py = 0.0;
    S.info[0] = S.info[1] = S.info[2] = 0.f;
    S.id = S.gone = S.len = S.mode = S.rank = 0;
    S.alive = false;
}

__device__ __forceinline__ void bl_seat_load(BlSeat &S, const BatchDev &bd, int at)
{
    const size_t sc = (size_t)bd.seat_cap;
    const double *p = bd.f64 + at;
#pragma unroll
    for (int f = 0; f < BL_NF; ++f) { S.w[f] = p[sc * f]; S.xa[f] = p[sc * (BL_NF + f)]; S.xb[f] = p[sc * (2 * BL_NF + f)]; }
    S.px = p[sc * (3 * BL_NF)];
    S.py = p[sc * (3 * BL_NF + 1)];
#pragma unroll
    for (int f = 0; f < BL_NF; ++f) {
        const double *q = p + sc * (3 * BL_NF + 2 + 4 * f);
        S.s0x[f] = q[0]; S.s1x[f] = q[sc]; S.s0y[f] = q[2 * sc]; S.s1y[f] = q[3 * sc];
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) S.info[k] = bd.f32[sc * k + at];
    S.id = bd.i32[at]; S.gone = bd.i32[sc + at]; S.len = bd.i32[2 * sc + at]; S.mode = bd.i32[3 * sc + at];
    S.rank = bd.i32[4 * sc + at];
}

__device__ __forceinline__ void bl_seat_store(const BlSeat &S, const BatchDev &bd, int at)
{
    const size_t sc = (size_t)bd.seat_cap;
    double *p = bd.f64 + at;
#pragma unroll
    for (int f = 0; f < BL_NF; ++f) { p[sc * f] = S.w[f]; p[sc * (BL_NF + f)] = S.xa[f]; p[sc * (2 * BL_NF + f)] = S.xb[f]; }
    p[sc * (3 * BL_NF)] = S.px;
    p[sc * (3 * BL_NF + 1)] = S.py;
#pragma unroll
    for (int f = 0; f < BL_NF; ++f) {
        double *q = p + sc * (3 * BL_NF + 2 + 4 * f);
        q[0] = S.s0x[f]; q[sc] = S.s1x[f]; q[2 * sc] = S.s0y[f]; q[3 * sc] = S.s1y[f];
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) bd.f32[sc * k + at] = S.info[k];
    bd.i32[at] = S.id; bd.i32[sc + at] = S.gone; bd.i32[2 * sc + at] = S.len; bd.i32[3 * sc + at] = S.mode;
    bd.i32[4 * sc + at] = S.rank;
}

// A ring entry as this compute unit's L2 holds it: the ring is written and read back by the same launch, frames apart;
// sc1 loads pass the unit's L1 (it is not refreshed by stores, the unit's own included, in any way the ISA promises).
__device__ __forceinline__ double2 bl_ring_load(const BatchDev &bd, int pos, int seat)
{
    const double *p = reinterpret_cast<const double *>(bd.ring + (size_t)pos * bd.seat_cap + seat);
    double2 v;
    v.x = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    v.y = __hip_atomic_load(p + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return v;
}
// (the same by its byte offset in the ring, 32 bits: a uniform base and a lane's offset, one address computation)
__device__ __forceinline__ double2 bl_ring_load_bytes(const BatchDev &bd, unsigned at)
{
    const double *p = reinterpret_cast<const double *>(reinterpret_cast<const char *>(bd.ring) + at);
    double2 v;
    v.x = __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    v.y = __hip_atomic_load(p + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return v;
}
// (a whole entry with ONE instruction, for the seats' ring copy: 16 bytes are more than an atomic load takes, so the load
// and its wait are written out -- sc1, as the compiler writes an agent-scope load; the compiler's own books know nothing
// of it and need not: it is complete where the statement ends)
typedef uint32_t bl_u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ bl_u32x4 bl_ring_load16(const double2 *p)
{
    bl_u32x4 v;
    asm volatile("global_load_dwordx4 %0, %1, off sc1\n\ts_waitcnt vmcnt(0)" : "=&v"(v) : "v"(p) : "memory");
    return v;
}
// (BL_RING_GROUP whole entries, requested together and all of them there where the
// statement ends: the refresh of the window sums, whose entries do not depend on each other -- one round trip past L1 for
// the group instead of one per entry.  The wait stands in the statement of the loads and the outputs are early-clobber, as
// above: the compiler takes an asm output for written where the statement ends, and must not hand a destination register
// to a later load's address.  The caller has nothing else in flight (vmcnt(0) would wait for it too).  Three, not four:
// tests/test_kernel_listing.py allows k_batch 46 vector-memory loads, and it had 44 with one entry per statement.)
constexpr int BL_RING_GROUP = 3;
__device__ __forceinline__ void bl_ring_load16_group(const double2 *const (&at)[BL_RING_GROUP], bl_u32x4 (&v)[BL_RING_GROUP])
{
    static_assert(BL_RING_GROUP == 3, "one load per entry is written out below");
    asm volatile("global_load_dwordx4 %0, %3, off sc1\n\t"
                 "global_load_dwordx4 %1, %4, off sc1\n\t"
                 "global_load_dwordx4 %2, %5, off sc1\n\t"
                 "s_waitcnt vmcnt(0)"
                 : "=&v"(v[0]), "=&v"(v[1]), "=&v"(v[2]) : "v"(at[0]), "v"(at[1]), "v"(at[2]) : "memory");
}
// (a whole entry with ONE instruction and NO wait of its own: the measurements that leave the windows in k_batch's steady
// frame, requested in front of barrier A and taken behind the frame's one bl_wait_vmem() in front of the filter bank, by
// bl_ring_taken16.  Between the two the compiler believes the destination registers written: were it to read, copy or
// spill them there, it would move what the load has not delivered yet -- early-clobber, as above, keeps them off the
// statement's own address, and THE GUARD for the stretch up to the wait is scripts/k_batch_census.py:
// pending_load_hazards, which follows every written-out `global_load_dwordx4 ... sc1` of the listing along every path
// to its vmcnt(0) wait, as it follows the written-out scalar loads.  The address is the seat's own entry of line 0 --
// what the frame's ring store is addressed from, a register pair the lane holds anyway -- plus the line's bytes: with the
// ring's base taken alone the compiler fetched it from the argument segment right in front of the first load.)
__device__ __forceinline__ void bl_ring_issue16(const BatchDev &bd, int seat, unsigned line_at, bl_u32x4 &v)
{
    const char *p = reinterpret_cast<const char *>(bd.ring + seat) + line_at;
    asm volatile("global_load_dwordx4 %0, %1, off sc1" : "=&v"(v) : "v"(p) : "memory");
}
// (behind the wait: the entries are handed on as that wait left them, and nothing that reads them is scheduled above it)
__device__ __forceinline__ void bl_ring_taken16(bl_u32x4 (&v)[BL_NF])
{
    static_assert(BL_NF == 3, "one operand per entry is written out below");
    asm volatile("" : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]));
}
// A ring entry as bl_gsff takes it: the two doubles, or the four registers a 16-byte load left (k_batch: the entry stays
// in them up to the operations that use it, and the seeding of a new track writes its copies into the same four -- as
// separate doubles the two sources met in six register moves per frame).
__device__ __forceinline__ double2 bl_entry(const double2 &e) { return e; }
__device__ __forceinline__ double2 bl_entry(const bl_u32x4 &v)
{
    return make_double2(__hiloint2double((int)v.y, (int)v.x), __hiloint2double((int)v.w, (int)v.z));
}
__device__ __forceinline__ void bl_entry_set(double2 &e, double x, double y) { e = make_double2(x, y); }
__device__ __forceinline__ void bl_entry_set(bl_u32x4 &v, double x, double y)
{
    v.x = (uint32_t)__double2loint(x); v.y = (uint32_t)__double2hiint(x);
    v.z = (uint32_t)__double2loint(y); v.w = (uint32_t)__double2hiint(y);
}
__device__ __forceinline__ void bl_ring_store(const BatchDev &bd, int pos, int seat, double x, double y)
{
    bd.ring[(size_t)pos * bd.seat_cap + seat] = make_double2(x, y);
}

// The window sums of a track from its history, exactly: the measurement of age a (0 = newest) is at ring position
// head - 1 - a; a filter's window holds the newest min(N, len) of them.  Done for every track at the frames whose index
// is a multiple of BL_REFRESH (a schedule in FRAME numbers: the rows of a video must not depend on how its frames were cut
// into batches), and by k_to_batch.
// (WHOLE: k_batch, where every live track does this in the same frame, on the frame's critical path -- whole entries,
// BL_RING_GROUP of them per round trip, and no further than the handle's largest horizon)
template <bool WHOLE = false>
__device__ __forceinline__ void bl_sums_from_ring(BlSeat &S, const BatchDev &bd, int seat, int head, int n0, int n1, int n2)
{
    const int lim[BL_NF] = {min(n0, S.len), min(n1, S.len), min(n2, S.len)};
    double s0x = 0.0, s1x = 0.0, s0y = 0.0, s1y = 0.0;
    if constexpr (WHOLE) {
        // BL_RING_GROUP entries per round trip, summed in the order of their ages with the operations of the loop below, as
        // far as the handle's largest horizon: behind it no filter records anything.  The bound is the handle's, not the lane's: the loop is the
        // wave's.  A lane asks for entries beyond its own history, and the last group for ages at and beyond the bound --
        // every position lies in the ring, whatever it holds -- and records nothing of them.
        // (the bound and the count are said to be uniform, readfirstlane: the compiler took both through vector registers
        // -- the count is converted to float64 below -- and made the loop an exec region of its own, scalar pairs that the
        // steady frame then spilled; the conversion gets a copy of the count)
        const int end = __builtin_amdgcn_readfirstlane(min(max(n0, max(n1, n2)), BL_HB - 1));
        // (a window longer than the ring holds is never recorded, as below: the last group's ages may reach it)
        const int rec[BL_NF] = {lim[0] > end ? -1 : lim[0], lim[1] > end ? -1 : lim[1], lim[2] > end ? -1 : lim[2]};
        for (int a0 = 0; a0 < end; a0 = __builtin_amdgcn_readfirstlane(a0 + BL_RING_GROUP)) {
            int a0v = a0;
            asm volatile("" : "+v"(a0v));
            const double2 *at[BL_RING_GROUP];
            bl_u32x4 w[BL_RING_GROUP];
#pragma unroll
            for (int k = 0; k < BL_RING_GROUP; ++k)
                at[k] = bd.ring + (size_t)((head - 1 - a0 - k) & (BL_HB - 1)) * bd.seat_cap + seat;
            bl_ring_load16_group(at, w);
#pragma unroll
            for (int k = 0; k < BL_RING_GROUP; ++k) {
                const int a = a0 + k;
                const double ex = __hiloint2double((int)w[k].y, (int)w[k].x), ey = __hiloint2double((int)w[k].w, (int)w[k].z);
                if (a < S.len) {      // (at and beyond the bound as well: nothing records those sums)
                    s0x = s0x + ex;
                    s0y = s0y + ey;
                    s1x = __builtin_fma((double)(a0v + k), ex, s1x);
                    s1y = __builtin_fma((double)(a0v + k), ey, s1y);
                }
#pragma unroll
                for (int f = 0; f < BL_NF; ++f)
                    if (a + 1 == rec[f]) { S.s0x[f] = s0x; S.s1x[f] = s1x; S.s0y[f] = s0y; S.s1y[f] = s1y; }
            }
        }
        return;
    }
    for (int a = 0; a < BL_HB - 1; ++a) {
        const double2 e = bl_ring_load(bd, (head - 1 - a) & (BL_HB - 1), seat);
        if (a < S.len) {
            s0x = s0x + e.x;
            s0y = s0y + e.y;
            s1x = __builtin_fma((double)a, e.x, s1x);
            s1y = __builtin_fma((double)a, e.y, s1y);
        }
#pragma unroll
        for (int f = 0; f < BL_NF; ++f)
            if (a + 1 == lim[f]) { S.s0x[f] = s0x; S.s1x[f] = s1x; S.s0y[f] = s0y; S.s1y[f] = s1y; }
    }
}

// exp(x) of BL_NF arguments x <= 0 at once, with the device library's own arithmetic for float64 (x log2(e) rounded to
// an integer n, the reduction r = x - n ln 2 with ln 2 in two constants, its degree-11 polynomial in Horner form, ldexp by
// n) -- every operation, operand and constant as in the listing of exp(), so every result bit -- but for two things.
// The three chains of dependent operations advance in step, not one after the other.  And the library's two range tests
// are left out (x > 1024: +inf; x < -1075: 0): the caller replaces everything below lik_min by lik_min, and that is where
// ldexp's own underflow ends as well (0 or a denormal).  Holds for -1e40 < x <= 0, squared distances no frame has: beyond
// it the rounding of n makes r large, far beyond that the polynomial overflows.
__device__ __forceinline__ void bl_exp_nonpos(const double (&x)[BL_NF], double (&e)[BL_NF])
{
    auto c = [](unsigned long long bits) { return __longlong_as_double((long long)bits); };
    const double coef[9] = {c(0x3ec71dee623fde64ull), c(0x3efa01997c89e6b0ull), c(0x3f2a01a014761f6eull), c(0x3f56c16c1852b7b0ull),
                            c(0x3f81111111122322ull), c(0x3fa55555555502a1ull), c(0x3fc5555555555511ull), c(0x3fe000000000000bull), 1.0};
    double n[BL_NF], r[BL_NF], p[BL_NF];
#pragma unroll
    for (int f = 0; f < BL_NF; ++f) n[f] = __builtin_rint(x[f] * c(0x3ff71547652b82feull));
#pragma unroll
    for (int f = 0; f < BL_NF; ++f) r[f] = __builtin_fma(c(0xbfe62e42fefa39efull), n[f], x[f]);
#pragma unroll
    for (int f = 0; f < BL_NF; ++f) r[f] = __builtin_fma(c(0xbc7abc9e3b39803full), n[f], r[f]);
#pragma unroll
    for (int f = 0; f < BL_NF; ++f) p[f] = __builtin_fma(c(0x3e5ade156a5dcb37ull), r[f], c(0x3e928af3fca7ab0cull));
#pragma unroll
    for (int k = 0; k < 9; ++k)
#pragma unroll
        for (int f = 0; f < BL_NF; ++f) p[f] = __builtin_fma(r[f], p[f], coef[k]);
#pragma unroll
    for (int f = 0; f < BL_NF; ++f) p[f] = __builtin_fma(r[f], p[f], 1.0);
#pragma unroll
    for (int f = 0; f < BL_NF; ++f) e[f] = __builtin_ldexp(p[f], (int)n[f]);
}

// The history length at which a lane's filter bank next leaves the steady path (k_batch): 0 for a track without history
// (the seeding), n_i[mode] while a filter is still to be switched on, INT_MAX once all are.  One compare of the length
// against it guards everything a track does in three frames of its life.  It is not part of the rest format: n_i ascends
// strictly (ysmr_tracker_create), so the mode is the number of horizons below it, and the threshold is derived from the
// stored mode when a seat is loaded (bl_grow_at) and turned back into it in the rare block and at the store (bl_mode_of).
__device__ __forceinline__ int bl_grow_at(int len, int mode, int nf, const int (&n_i)[BL_NF])
{
    if (len == 0) return 0;
    return mode == 0 && 0 < nf ? n_i[0] : (mode == 1 && 1 < nf ? n_i[1] : (mode == 2 && 2 < nf ? n_i[2] : 0x7FFFFFFF));
}
__device__ __forceinline__ int bl_mode_of(int grow_at, int nf, const int (&n_i)[BL_NF])
{
    return (int)(0 < nf && n_i[0] < grow_at) + (int)(1 < nf && n_i[1] < grow_at) + (int)(2 < nf && n_i[2] < grow_at);
}

// GaussianSumFIR.correct + predict of one track by its lane (gsff.py:204-347; the statement order of gsff_wave).
// leave[f]: the measurement of age N_f - 1 (requested by the caller before the claims); head: the ring position this
// frame's measurement takes.
// (struct BlGains { alpha[filter][x / y row], beta[..][..] }: track.hip, the host handle holds one)
// Gains: BlGains behind a plain pointer (k_track_lanes), or in the constant address space (k_batch: the gains then come
// with scalar loads and enter the multiplications as scalar operands)
// GATED (k_batch): the caller requested leave[f] only where the window of filter f is full and left 0.0 elsewhere, a new
// track comes with S.len = 0, and grow_at (above) stands in for S.mode, which is not read and not written.  The steady
// path then has no select on `full` / `fresh` and no mode cascade: those sit behind `len >= grow_at`.  Not GATED
// (k_track_lanes, whose ring loads leave in the same round as the seat that would gate them): leave[] is whatever the
// ring held, fresh says that the seat's state is not this track's, grow_at is unused.
// tr: the tracker's arguments again, for what only the rare block and the tail need (horizons, hist_cap, lik_min) -- k_batch
// passes the argument segment itself, so that they come with scalar loads where they are used.
// Entry: double2, or the registers of a 16-byte load (bl_entry, above: k_batch).
template <bool GATED, typename Args, typename Gains, typename Entry>
__device__ __forceinline__ void bl_gsff(BlSeat &S, const TrackerDev &t, const Args &tr, const BatchDev &bd, const Gains &g, int seat, int head,
                                        Entry (&leave)[BL_NF], double z0, double z1, bool fresh, int &grow_at, double &o0, double &o1)
{
    const int nf = t.n_f, L = tr.hist_cap;
    const double lik_min = tr.lik_min;
    int len = GATED ? S.len : (fresh ? 0 : S.len), mode = GATED ? 0 : (fresh ? 0 : S.mode);
    if (!GATED || len >= grow_at) {
        const int n_i[BL_NF] = {tr.n_i[0], nf > 1 ? tr.n_i[1] : 0x7FFFFFFF, nf > 2 ? tr.n_i[2] : 0x7FFFFFFF};
        if (GATED) mode = bl_mode_of(grow_at, nf, n_i);
        if (len == 0) {      // history starts as n_i[0] copies of the first measurement (gsff.py:281)
            const int n0 = n_i[0];
#pragma unroll
            for (int f = 0; f < BL_NF; ++f) { S.w[f] = 0.0; S.xa[f] = 0.0; S.xb[f] = 0.0; }
            const double c1 = (double)(n0 * (n0 - 1) / 2);
#pragma unroll
            for (int f = 0; f < BL_NF; ++f) {
                S.s0x[f] = (double)n0 * z0; S.s1x[f] = c1 * z0;
                S.s0y[f] = (double)n0 * z1; S.s1y[f] = c1 * z1;
            }
            for (int a = 0; a < n0; ++a) bl_ring_store(bd, (head - 1 - a) & (BL_HB - 1), seat, z0, z1);
            len = n0;
            if (GATED) {     // what leaves a window that these copies fill is a copy; nothing leaves the others (the caller
                             // requested nothing for a lane that held no track then: leave[] is unset on entry)
#pragma unroll
                for (int f = 0; f < BL_NF; ++f) {
                    const bool copy = len >= n_i[f];
                    bl_entry_set(leave[f], copy ? z0 : 0.0, copy ? z1 : 0.0);
                }
            }
        }
        bool grew = false;   // gsff.py:283-289: while len(history) >= n_i[mode]: mode += 1
        if (mode == 0 && 0 < nf && len >= n_i[0]) { mode = 1; grew = true; }
        if (mode == 1 && 1 < nf && len >= n_i[1]) { mode = 2; grew = true; }
        if (mode == 2 && 2 < nf && len >= n_i[2]) { mode = 3; grew = true; }
        // Filters that are not switched on yet carry weight 0 (and finite estimates): every sum below may then run over all
        // three without a select -- adding a zero term is exact, so a0 + (a1 + a2) is the reference's a0, or a0 + a1
        if (grew) {          // the estimates of every active filter from the history as it stands, uniform weights
            const double w0 = mode == 1 ? 1.0 : (mode == 2 ? 0.5 : 1.0 / 3.0);
#pragma unroll
            for (int f = 0; f < BL_NF; ++f)
                if (f < mode) {
                    S.xa[f] = __builtin_fma(-g.beta[f][0], S.s1x[f], g.alpha[f][0] * S.s0x[f]);
                    S.xb[f] = __builtin_fma(-g.beta[f][1], S.s1y[f], g.alpha[f][1] * S.s0y[f]);
                    S.w[f] = w0;
                }
        }
        if (GATED) grow_at = mode == 0 ? n_i[0] : (mode == 1 ? n_i[1] : (mode == 2 ? n_i[2] : 0x7FFFFFFF));
    }
    // append the measurement: every entry one frame older, the entry of age N - 1 leaves a full window
#pragma unroll
    for (int f = 0; f < BL_NF; ++f) {
        const double2 lv = bl_entry(leave[f]);
        double lx = lv.x, ly = lv.y;
        if (!GATED) {
            const bool full = f < nf && len >= t.n_i[f];
            // (a track born in this frame: its history is copies of z, written above -- after `leave` was requested)
            lx = full ? (fresh ? z0 : lx) : 0.0; ly = full ? (fresh ? z1 : ly) : 0.0;
        }
        // (GATED, a window that is not full: fma(nn, 0.0, s) = s and (s0 + z) - 0.0 = s0 + z, the bits of the line above)
        const double nn = -(double)(f < nf ? t.n_i[f] : 0);
        S.s1x[f] = __builtin_fma(nn, lx, S.s1x[f] + S.s0x[f]);
        S.s1y[f] = __builtin_fma(nn, ly, S.s1y[f] + S.s0y[f]);
        S.s0x[f] = (S.s0x[f] + z0) - lx;
        S.s0y[f] = (S.s0y[f] + z1) - ly;
    }
    bl_ring_store(bd, head, seat, z0, z1);
    if (len < L) ++len;
    // likelihoods of the measurement under last frame's estimates (gsff.py:179-202)
    double lik[BL_NF], total = 0.0;
    double ex[BL_NF];
#pragma unroll
    for (int f = 0; f < BL_NF; ++f) {
        const double d0 = z0 - S.xa[f], d1 = z1 - S.xb[f];
        double q = d0 * d0;
        q = q + d1 * d1;
        ex[f] = -0.5 * q;
    }
    bl_exp_nonpos(ex, lik);
    // (max, not compare and select: the same value for every l that is not a NaN, and bl_exp_nonpos's domain -- finite
    // squared distances -- has none)
#pragma unroll
    for (int f = 0; f < BL_NF; ++f) {
        const double l = __builtin_fmax(lik[f], lik_min);
        lik[f] = l;
        total = f == 0 ? l * S.w[f] : total + l * S.w[f];      // (0.0 + a product of non-negative factors is that product)
    }
    // w_i <- lik_i w_i / total (gsff.py:333-336) as lik_i w_i * (1 / total): one division for the three weights; a weight
    // may differ from the quotient in its last bit (the per-frame kernels divide three times)
    const double r_total = 1.0 / total;
#pragma unroll
    for (int f = 0; f < BL_NF; ++f) S.w[f] = (lik[f] * S.w[f]) * r_total;
    // output = np.sum(x_hat * w, axis=1) = a0 + (a1 + a2)
    o0 = S.xa[0] * S.w[0] + (S.xa[1] * S.w[1] + S.xa[2] * S.w[2]);
    o1 = S.xb[0] * S.w[0] + (S.xb[1] * S.w[1] + S.xb[2] * S.w[2]);
    // predict: the new estimates (behind the outputs, which need the old ones: straight into their registers), weighted
#pragma unroll
    for (int f = 0; f < BL_NF; ++f) {
        S.xa[f] = __builtin_fma(-g.beta[f][0], S.s1x[f], g.alpha[f][0] * S.s0x[f]);
        S.xb[f] = __builtin_fma(-g.beta[f][1], S.s1y[f], g.alpha[f][1] * S.s0y[f]);
    }
    S.px = S.xa[0] * S.w[0] + (S.xa[1] * S.w[1] + S.xa[2] * S.w[2]);
    S.py = S.xb[0] * S.w[0] + (S.xb[1] * S.w[1] + S.xb[2] * S.w[2]);
    S.len = len;
    if (!GATED) S.mode = mode;
}

// Nearest detection of a prediction among the frame's detections in LDS: D.min(1) / D.argmin(1) of tracker.py:151-163.
//
// Fast path, per lane, straight-line and in FLOAT: the 3 x 3 cells around the prediction are three runs of the cell-ordered
// list (one per row of cells); their six bounds come with one round of LDS reads, the first five candidates of each run
// with a second.  A candidate's float squared distance and its slot become ONE 32-bit key (a non-negative float orders
// like its bits; the slot number replaces the four lowest mantissa bits), and the two smallest keys are kept with a
// minimum and a median-of-three per candidate -- no second pass, no index bookkeeping.  A run with more than five
// candidates is finished in a loop on the same two registers.  Float decides only what float can decide: the result
// stands when the second smallest key lies outside the float error band of the smallest (then the smallest is the
// float64 argmin among the block's candidates, and no tie rule is needed) and nothing outside the block can be as near
// (the block's boundary is farther than the best distance, with a margin far above rounding; cells were assigned in
// float arithmetic too).  Its float64 squared distance is then evaluated once, for the claim key.  Everything else -- a
// lost track far from every detection, two candidates a hair apart, an exact tie -- is left to bl_search_wave.
// Error band: |fx - px| <= 2^-24 * 4096 = 2.4e-4 for coordinates below 4096, the candidates are float already, so a float
// squared distance of a candidate within ~100 px is off by less than 2 * 200 * 2.4e-4 + 3 * 2^-24 * s < 0.1 + 2e-7 s, and the
// key drops 2^-19 s more.
struct BlNear { double s; float zx, zy; int col; bool done; };
// The kernel's dynamic LDS, at namespace scope and addressed by OFFSET everywhere: a pointer that went through an array
// or a struct of pointers comes back generic, and the compiler then reads LDS with flat_load -- twice the latency and a
// 64-bit address per access (97 of them in the first build of this kernel).
extern __shared__ __attribute__((aligned(16))) unsigned long long bl_lds[];
__device__ __forceinline__ uint32_t *bl_u32(int dword_off) { return reinterpret_cast<uint32_t *>(bl_lds) + dword_off; }
// (entry i of a 3-D block's f32 plane, z32 its dword offset)
__device__ __forceinline__ float bl_z32_at(int z32, int i) { return reinterpret_cast<const float *>(bl_u32(z32))[i]; }
struct BlGridView {
    int start, xy, items, lists, G;      // dword offsets into bl_lds (lists: -1, none); cells per side
    float x0, y0, cell, inv;
    __device__ __forceinline__ int start_at(int i) const { return reinterpret_cast<const unsigned short *>(bl_u32(start))[i]; }
    __device__ __forceinline__ int item_at(int i) const { return reinterpret_cast<const unsigned short *>(bl_u32(items))[i]; }
    __device__ __forceinline__ float2 xy_at(int i) const { return reinterpret_cast<const float2 *>(bl_u32(xy))[i]; }
};
// (the block's header x0, y0, cell, 1 / cell: its first four words)
__device__ __forceinline__ float4 bl_grid_header(int buf)
{
    const float2 *h = reinterpret_cast<const float2 *>(bl_u32(buf));
    const float2 a = h[0], b = h[1];
    return make_float4(a.x, a.y, b.x, b.y);
}
__device__ __forceinline__ BlGridView bl_grid_view(int buf, int m, const float4 &hdr)     // buf: dword offset of the frame's block
{
    BlGridView g;
    g.G = bl_grid_n(m);
    g.start = buf + 16;
    g.xy = buf + 16 + bl_start_dwords(g.G);
    g.items = buf + 16 + bl_start_dwords(g.G) + 2 * bl_mp(m);
    g.lists = bl_has_lists(m) ? buf + bl_list_off(m) : -1;
    g.x0 = hdr.x; g.y0 = hdr.y; g.cell = hdr.z; g.inv = hdr.w;
    return g;
}
__device__ __forceinline__ BlGridView bl_grid_view(int buf, int m) { return bl_grid_view(buf, m, bl_grid_header(buf)); }
// The winner's centre and its column: both addresses come from the winner's position, so both reads are issued in front of
// ONE wait (left to itself the compiler issued the column's read behind the centre's wait: a second LDS round trip in
// front of the claim).
__device__ __forceinline__ void bl_winner(const BlGridView &g, int q, float2 &c, int &col)
{
    c = g.xy_at(q);
    col = g.item_at(q);
    asm volatile("" : "+v"(c.x), "+v"(c.y), "+v"(col));
}
__device__ __forceinline__ double bl_dist2(double px, double py, float2 c)
{
    const double dx = px - (double)c.x;
    const double dy = py - (double)c.y;
    double s = dx * dx;
    s = s + dy * dy;
    return s;
}
__device__ __forceinline__ float bl_dist2f(float fx, float fy, float2 c)
{
    const float dx = fx - c.x, dy = fy - c.y;
    return __builtin_fmaf(dy, dy, dx * dx);
}
// The 3-D link's (k_batch3, below) result and distances: a third coordinate beside the planar ones.
struct BlNear3 { double s, z; float zx, zy; int col; bool done; };
__device__ __forceinline__ double bl_dist3(double px, double py, double pz, float2 c, double cz)
{
    // cdist's order (luminosity_model.cdist; rowmin_wave<.., true>): dx * dx + dy * dy + dz * dz, summed left to right
    const double dx = px - (double)c.x;
    const double dy = py - (double)c.y;
    const double dz = pz - cz;
    double s = dx * dx;
    s = s + dy * dy;
    s = s + dz * dz;
    return s;
}
__device__ __forceinline__ float bl_dist3f(float fx, float fy, float fz, float2 c, float cz)
{
    const float dx = fx - c.x, dy = fy - c.y, dz = fz - cz;
    return __builtin_fmaf(dz, dz, __builtin_fmaf(dy, dy, dx * dx));
}
// Float error band of a 3-D squared distance, for |px|, |py|, |pz| and every |third| below 4096 (k_bgrid3 flags a frame
// with a larger one, the caller tests pz).  (float)px, (float)py and (float)pz are off by at most 2^-24 * 4096 = 2.4e-4; the
// centres are float already, but the candidate's third coordinate was ROUNDED to float as well: dz is off by 4.9e-4, dx
// and dy by 2.4e-4.  Unlike a planar distance inside a 3 x 3 block, dz has no bound but 8192, so the error is taken relative
// to the distance: |s_f - s| <= 2 (|dx| + |dy|) 2.4e-4 + 2 |dz| 4.9e-4 + 4 * 2^-24 s <= 9.8e-4 * sqrt(3 s) + 2.4e-7 s, and with
// a sqrt(s) <= t + a^2 s / (4 t) at t = 0.05: <= 0.05 + 1.5e-5 s; the key drops 2^-19 s more: e(s) <= 0.05 + 1.7e-5 s.
// A detection that is truly as near as the float winner (float distance b) has a float distance of at most
// b + 2 e(s_winner) <= b + 0.1002 + 3.5e-5 b: the band below is that with a margin (twice in the constant, 1.4 x in the slope).
__device__ __forceinline__ float bl3_band(float best) { return best + (0.2f + 5e-5f * best); }
// What the searches below, one text for both dimensions, take per dimension: the result, the float key's distance, its
// band, the exact distance (pz / fz / cz: unused in the plane)
template <bool D3> using BlNearOf = std::conditional_t<D3, BlNear3, BlNear>;
template <bool D3> __device__ __forceinline__ float bl_distf(float fx, float fy, float fz, float2 c, float cz)
{
    if constexpr (D3) return bl_dist3f(fx, fy, fz, c, cz);
    else return bl_dist2f(fx, fy, c);
}
template <bool D3> __device__ __forceinline__ double bl_dist(double px, double py, double pz, float2 c, double cz)
{
    if constexpr (D3) return bl_dist3(px, py, pz, c, cz);
    else return bl_dist2(px, py, c);
}
template <bool D3> __device__ __forceinline__ float bl_band(float best)
{
    if constexpr (D3) return bl3_band(best);
    else return best + (0.2f + 5e-6f * best);
}
__device__ __forceinline__ uint32_t bl_med3(uint32_t a, uint32_t b, uint32_t c)
{
    uint32_t r;                                          // (the compiler spells the median out as three min / max)
    asm("v_med3_u32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}
// One body for the planar link (D3 = false) and the 3-D link (D3 = true), which adds the third coordinate: fz, the f32
// plane's cz[] beside the centres (z32: the plane's dword offset in LDS), float keys of dx^2 + dy^2 + dz^2 and their band
// (bl3_band), and the winner's exact third coordinate from the f64 plane in HBM (z64).  "Nothing outside the block is as
// near" stays a test in the PLANE in both: a detection's 3-D distance is never below its planar distance, so one that lies
// beyond the block's boundary in the plane is farther than the boundary in space.  The planar branch is spelt as k_batch was
// compiled with it (its expressions, bl_winner, the sched_barrier): k_batch's register allocation moves at a touch.
template <bool D3>
__device__ __forceinline__ BlNearOf<D3> bl_block_search(const BlGridView &g, int z32, const double *__restrict__ z64, double px, double py,
                                                        double pz, int m)
{
    constexpr int R = 3, C = 5;
    const int G = g.G;
    const float fx = (float)px, fy = (float)py;
    [[maybe_unused]] const float fz = (float)pz;
    int cx = (int)floorf((fx - g.x0) * g.inv), cy = (int)floorf((fy - g.y0) * g.inv);
    const bool in_grid = cx >= 0 && cx < G && cy >= 0 && cy < G;
    cx = cx < 0 ? 0 : (cx > G - 1 ? G - 1 : cx);
    cy = cy < 0 ? 0 : (cy > G - 1 ? G - 1 : cy);
    const int xl = max(cx - 1, 0), xh = min(cx + 1, G - 1), yl = max(cy - 1, 0), yh = min(cy + 1, G - 1);
    int a[R], b[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int iy = min(yl + r, G - 1);
        a[r] = g.start_at(iy * G + xl);
        b[r] = g.start_at(iy * G + xh + 1);
        if (yl + r > yh) b[r] = a[r];                   // (a block cut by the edge of the grid has fewer rows)
    }
    // every candidate's read is issued before the first is used (left to itself the compiler, short of registers, waits
    // for each read before it issues the next: fifteen LDS round trips in a row); a slot beyond the end of its run reads
    // whatever follows in LDS and is masked afterwards (3-D: inside the block's LDS part -- a run starts at or below m, and
    // entry m + 4 lies in the padding or in the next plane)
    float2 c[R * C];
    float cz[R * C] = {};
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const float2 *run = reinterpret_cast<const float2 *>(bl_u32(g.xy)) + a[r];
#pragma unroll
        for (int j = 0; j < C; ++j) {
            c[C * r + j] = run[j];
            if constexpr (D3) cz[C * r + j] = bl_z32_at(z32, a[r] + j);
        }
    }
    __builtin_amdgcn_sched_barrier(0);
    uint32_t lo = 0xFFFFFFFFu, hi = 0xFFFFFFFFu;        // the two smallest keys
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int j = 0; j < C; ++j) {
            const float d2 = bl_distf<D3>(fx, fy, fz, c[C * r + j], cz[C * r + j]);
            uint32_t key = (__float_as_uint(d2) & 0xFFFFFFF0u) | (uint32_t)(C * r + j);
            key = a[r] + j < b[r] ? key : 0xFFFFFFFFu;
            hi = bl_med3(lo, hi, key);
            lo = min(lo, key);
        }
    int q_extra = 0;
    bool more = false;
#pragma unroll
    for (int r = 0; r < R; ++r) more = more || (b[r] - a[r] > C);
    if (more) {                                        // the runs' sixth and later candidates: slot 15, position kept aside
#pragma unroll
        for (int r = 0; r < R; ++r)
            for (int qq = a[r] + C; qq < b[r]; ++qq) {
                const uint32_t key = (__float_as_uint(bl_distf<D3>(fx, fy, fz, g.xy_at(qq), D3 ? bl_z32_at(z32, qq) : 0.f)) & 0xFFFFFFF0u) | 15u;
                q_extra = key < lo ? qq : q_extra;
                hi = bl_med3(lo, hi, key);
                lo = min(lo, key);
            }
    }
    const float best = __uint_as_float(lo & 0xFFFFFFF0u), second = __uint_as_float(hi & 0xFFFFFFF0u);
    const float band = bl_band<D3>(best);              // (twice the error bound: both distances are off)
    const int slot = (int)(lo & 15u);
    const int run = slot >= 2 * C ? 2 : (slot >= C ? 1 : 0);
    const int bq = slot == 15 ? q_extra : (run == 2 ? a[2] : (run == 1 ? a[1] : a[0])) + slot - C * run;
    // Nothing outside the block is as near: a prediction inside the grid lies in its own cell, a whole cell away from the
    // block's boundary -- one comparison for nearly every lane; the others measure the distance to the outside of the
    // block (a side on the edge of the grid has nothing beyond it)
    const bool found = lo != 0xFFFFFFFFu;
    double wz = 0.0;
    if constexpr (D3) wz = z64[found ? bq : 0];         // (the winner's exact third coordinate: requested at once)
    const float reach = 0.998f * g.cell;
    bool inside = in_grid && band < reach * reach;
    if (!inside) {
        const float big = 3.0e38f;
        float bound = big;
        if (xl > 0) bound = fminf(bound, fx - (g.x0 + (float)xl * g.cell));
        if (xh < G - 1) bound = fminf(bound, (g.x0 + (float)(xh + 1) * g.cell) - fx);
        if (yl > 0) bound = fminf(bound, fy - (g.y0 + (float)yl * g.cell));
        if (yh < G - 1) bound = fminf(bound, (g.y0 + (float)(yh + 1) * g.cell) - fy);
        bound -= 1e-3f * g.cell;
        inside = bound >= big * 0.5f || (bound > 0.f && bound * bound > band);
    }
    float2 cw;
    BlNearOf<D3> r;
    if constexpr (D3) { cw = g.xy_at(found ? bq : 0); r.col = g.item_at(found ? bq : 0); r.z = wz; }
    else bl_winner(g, found ? bq : 0, cw, r.col);
    r.s = bl_dist<D3>(px, py, pz, cw, wz);
    r.zx = cw.x; r.zy = cw.y;
    r.done = found && inside && !(second <= band);     // (hi = 0xFFFFFFFF reads as a NaN: no second candidate)
    return r;
}
__device__ __forceinline__ BlNear bl_search_block(const BlGridView &g, double px, double py, int m)
{
    return bl_block_search<false>(g, 0, nullptr, px, py, 0.0, m);
}

// The same from the candidate list of the prediction's cell (frames with G <= 32, predictions inside the grid): one LDS
// round for the list, one for the centres, eight keys as above -- the slot is the list position -- and no bounds, masks or
// outside test: the list holds the float64 argmin of every point of the cell and every detection within the float band of
// it (k_bgrid: bl_cell_list), so what it leaves open is what the 3 x 3 block would (the band), and that goes to the wave.
// A cell whose list came out too long is served the same way from the list of the prediction's QUADRANT (bl_quad_list).
// A lane outside the grid or in a cell still flagged takes bl_search_block; the wave runs it only when some lane needs it.
__device__ __forceinline__ BlNear bl_search(const BlGridView &g, double px, double py, int m)
{
    const int G = g.G;
    const float fx = (float)px, fy = (float)py;
    const float ux = (fx - g.x0) * g.inv, uy = (fy - g.y0) * g.inv;
    const float wx = floorf(ux), wy = floorf(uy);
    const int cx = (int)wx, cy = (int)wy;
    bool listed = g.lists >= 0 && cx >= 0 && cx < G && cy >= 0 && cy < G;
    uint4 l = make_uint4(0u, 0u, 0u, 0u);
    if (listed) l = reinterpret_cast<const uint4 *>(bl_u32(g.lists))[cy * G + cx];
    // a split cell (k_bgrid: its own list came out too long): the list of the prediction's quadrant, from the overflow
    // area behind the lists -- one more dependent read for these lanes, then the same eight candidates as everyone
    if (listed && (l.x & 0xFFFFu) == BL_SPLIT) {
        const int q = (int)(ux - wx >= 0.5f) + 2 * (int)(uy - wy >= 0.5f);
        l = reinterpret_cast<const uint4 *>(bl_u32(g.lists))[G * G + (int)(l.x >> 16) * 4 + q];
    }
    listed = listed && (l.x & 0xFFFFu) != BL_FLAG;
    BlNear r;
    if (listed) {
        const uint32_t w[4] = {l.x, l.y, l.z, l.w};
        float2 c[BL_LIST];
#pragma unroll
        for (int k = 0; k < BL_LIST; ++k) c[k] = g.xy_at((w[k >> 1] >> (16 * (k & 1))) & 0xFFFFu);
        __builtin_amdgcn_sched_barrier(0);
        uint32_t lo = 0xFFFFFFFFu, hi = 0xFFFFFFFFu;
#pragma unroll
        for (int k = 0; k < BL_LIST; ++k) {
            const uint32_t key = (__float_as_uint(bl_dist2f(fx, fy, c[k])) & 0xFFFFFFF0u) | (uint32_t)k;
            hi = bl_med3(lo, hi, key);
            lo = min(lo, key);
        }
        const float best = __uint_as_float(lo & 0xFFFFFFF0u), second = __uint_as_float(hi & 0xFFFFFFF0u);
        const float band = best + (0.2f + 5e-6f * best);
        const uint32_t slot = lo & 15u;
        const uint32_t wd = (slot & 4u) ? ((slot & 2u) ? l.w : l.z) : ((slot & 2u) ? l.y : l.x);
        const int bq = (int)((wd >> (16u * (slot & 1u))) & 0xFFFFu);
        float2 cw;
        bl_winner(g, bq, cw, r.col);
        r.s = bl_dist2(px, py, cw);
        r.zx = cw.x; r.zy = cw.y;
        r.done = !(second <= band);      // (a padding slot is 1e30 away: its distance is +inf, never within the band)
    } else {
        r = bl_search_block(g, px, py, m);
    }
    return r;
}

// The same for ONE track by the whole wave over EVERY detection of the frame, 512 at a time (eight per lane, their reads
// in flight together).  First in float, like bl_search: when exactly one detection lies within the float error band of
// the smallest float distance it is the argmin, and its float64 distance is evaluated once (a lost track far from
// everything: most calls end here).  Otherwise exactly, rowmin_wave's three passes: the smallest squared distance; the
// lowest column within 2^-48 of it; the rounded roots themselves only if some s differs from the smallest at all.
// px, py, the result: wave-uniform.
// One body for both dimensions, as bl_block_search, its planar branch spelt as k_batch was compiled with it.  The 3-D
// instance adds pz and `narrow` (wave-uniform too): its float pre-pass runs only where the 3-D band holds (`narrow`) and reads
// the f32 plane in LDS; its exact passes read the f64 plane in HBM, coalesced, in cell order like the centres.
template <bool D3>
__device__ __forceinline__ BlNearOf<D3> bl_wave_search(const BlGridView &g, int z32, const double *__restrict__ z64, double px, double py,
                                                       double pz, int m, int lane, bool narrow)
{
    const double inf = __longlong_as_double(0x7FF0000000000000ll);
    BlNearOf<D3> r;
    r.done = true;
    if (m <= 512 && (!D3 || narrow)) {
        const float fx = (float)px, fy = (float)py;
        [[maybe_unused]] const float fz = (float)pz;
        float sf[8];
        int lo = 0x7F800000;                              // (a non-negative float orders like its bits, as an int too)
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int j = u * 64 + lane;
            sf[u] = j < m ? bl_distf<D3>(fx, fy, fz, g.xy_at(min(j, m - 1)), D3 ? bl_z32_at(z32, min(j, m - 1)) : 0.f) : 3.0e38f;
            lo = min(lo, (int)__float_as_uint(sf[u]));
        }
        const float best = __uint_as_float((uint32_t)wave_min(lo));
        const float band = bl_band<D3>(best);
        int n_near = 0, jn = 0;
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const unsigned long long b = __ballot(sf[u] <= band);
            n_near += (int)__popcll(b);
            if (b) jn = u * 64 + __builtin_ctzll(b);
        }
        if (n_near == 1) {
            const float2 c = g.xy_at(jn);
            double wz = 0.0;
            if constexpr (D3) r.z = wz = z64[jn];
            r.s = bl_dist<D3>(px, py, pz, c, wz); r.zx = c.x; r.zy = c.y; r.col = g.item_at(jn);
            return r;
        }
    }
    double lane_min = inf;
    for (int j0 = 0; j0 < m; j0 += 512) {
        float2 c[8];
        double cz[8] = {};
#pragma unroll
        for (int u = 0; u < 8; ++u) { const int j = min(j0 + u * 64 + lane, m - 1); c[u] = g.xy_at(j); if constexpr (D3) cz[u] = z64[j]; }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const double s = bl_dist<D3>(px, py, pz, c[u], cz[u]);
            lane_min = (j0 + u * 64 + lane < m) ? __builtin_fmin(lane_min, s) : lane_min;
        }
    }
    const double s_min = wave_min(lane_min);
    const double near_limit = s_min + s_min * 0x1p-48;
    int cand = 0x7FFFFFFF;
    bool inexact = false;
    for (int j0 = 0; j0 < m; j0 += 512) {
        float2 c[8];
        double cz[8] = {};
        int it[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) { const int j = min(j0 + u * 64 + lane, m - 1); c[u] = g.xy_at(j); it[u] = g.item_at(j); if constexpr (D3) cz[u] = z64[j]; }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int j = j0 + u * 64 + lane;
            const double s = bl_dist<D3>(px, py, pz, c[u], cz[u]);
            const bool near = j < m && s <= near_limit;
            cand = near ? min(cand, (it[u] << 15) | j) : cand;          // (column, then position: both below 32768)
            inexact = inexact || (near && s != s_min);
        }
    }
    if (__any(inexact)) {
        const double d_min = sqrt(s_min);
        cand = 0x7FFFFFFF;
        for (int j = lane; j < m; j += 64) {
            const double s = bl_dist<D3>(px, py, pz, g.xy_at(j), D3 ? z64[j] : 0.0);
            if (s <= near_limit && sqrt(s) == d_min) cand = min(cand, (g.item_at(j) << 15) | j);
        }
    }
    const int win = wave_min(cand);
    const float2 c = g.xy_at(win & 0x7FFF);
    if constexpr (D3) r.z = z64[win & 0x7FFF];
    r.s = s_min; r.zx = c.x; r.zy = c.y; r.col = win >> 15;
    return r;
}
__device__ __forceinline__ BlNear bl_search_wave(const BlGridView &g, double px, double py, int m, int lane)
{
    return bl_wave_search<false>(g, 0, nullptr, px, py, 0.0, m, lane, true);
}

// ---- the kernel ----------------------------------------------------------------------------------------------------
constexpr int BL_COUNTS = 9;
constexpr int BL_SEAT_SLACK_WAVES = 0;      // a track wave is given up when the live tracks fit in this many fewer than hold one, + 1
constexpr int BL_MOVE_WORDS = 7 * BL_NF + 4 + 4;      // a track on the move, 64-bit words: the filter state, px, py, o0, o1; eight 32-bit fields
#ifdef YSMR_STAMPS
__device__ unsigned long long g_bstamps[BL_WAVES][16];
#ifndef YSMR_BL_FRAME
#define YSMR_BL_FRAME 40
#endif
// (stamp 8 stands directly behind the frame's wait for vector memory, in front of the filter bank: 6 -> 8 is the exposed
// wait, 8 -> 7 the filter bank.  g_bsteady: the same stamps of launch frame YSMR_BL_STEADY, so that a build whose stamped
// frame is the refresh frame has a steady frame's phases of the same launch beside it.)
__device__ unsigned long long g_bsteady[BL_WAVES][16];
#ifndef YSMR_BL_STEADY
#define YSMR_BL_STEADY 40
#endif
#define BLSTAMP(k) BLSTAMP_IN(f, k)
// (stamp 8: the frame number through an empty asm statement, so that its test is not the test of stamp 6 -- the compiler
// merged the two and took the wait between them into both halves of ONE branch, `lane 0 of a stamped frame` and the rest;
// every wave still waited, but scripts/k_batch_census.py's walk saw a way round the wait in either half)
#define BLSTAMP_OWN_TEST(k) do { int f_ = f; asm volatile("" : "+s"(f_)); BLSTAMP_IN(f_, k); } while (0)
#define BLSTAMP_IN(f, k) do { if ((f == YSMR_BL_FRAME || f == YSMR_BL_STEADY) && lane == 0) { unsigned long long t_; asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_) :: "memory"); if (f == YSMR_BL_FRAME) g_bstamps[wave][k] = t_; if (f == YSMR_BL_STEADY) g_bsteady[wave][k] = t_; } } while (0)
// per wave, over the launch's frames, how often a rarely taken path ran: 0 wave-frames with a lane on the 3 x 3 block search,
// 1 such lanes, 2 wave-frames with a lane seeding a new track's filter bank, 3 with a lane whose filter bank grew (not new),
// 4 frames with registration, 5 wave-frames refreshing the window sums from the ring, 6 frames with deaths, 7 deaths,
// 8 frames on the exact claim path
__device__ unsigned long long g_bcounts[BL_WAVES][BL_COUNTS];
// (the seats' two counts and the histogram in arrays of their own: tests/test_gpu_batch_claims.py reads g_bcounts as it is)
__device__ unsigned long long g_bseats[2];                 // the launch's frames that gave up track waves, tracks moved in them
__device__ unsigned long long g_bwaves[BL_WAVES + 1];      // the launch's frames by the track waves they ran on (0 .. BL_WAVES)
#define BLCOUNT(k, cond) do { const unsigned long long b_ = __ballot(cond); if (lane == 0 && b_) g_bcounts[wave][k] += 1; } while (0)
// (the refresh of the window sums, an array of its own as well: per wave 0, 1 the block's first and last instruction in the
// stamped frame, taken around the block by every wave of a refresh frame -- a wave without a live track passes it at once;
// 2, 3 the head and the end of launch frame YSMR_BL_STEADY, a steady frame of the same launch to set the refresh frame
// against)
__device__ unsigned long long g_brefresh[BL_WAVES][4];
#ifndef YSMR_BL_STEADY
#define YSMR_BL_STEADY 40
#endif
#define BLSTAMP_AT(cond, k) do { if ((cond) && lane == 0) { unsigned long long t_; asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_) :: "memory"); g_brefresh[wave][k] = t_; } } while (0)
#else
#define BLSTAMP(k) do {} while (0)
#define BLSTAMP_OWN_TEST(k) do {} while (0)
#define BLSTAMP_AT(cond, k) do {} while (0)
#endif

// The kernel's arguments as ONE structure: the kernel argument segment then IS this structure, and an argument that one
// phase of a frame needs (the row buffer, the detections' boxes, the error word, the state arrays at the end) is read
// from it where it is needed -- one scalar load out of the scalar cache -- instead of sitting in scalar registers for the
// whole launch: with everything passed and kept the usual way this kernel had 113 of them spilled into vector lanes.
struct BlKernArgs {
    TrackerDev t;
    BatchDev bd;
    const float *det_all;
    const int32_t *det_count;
    int batch, frame0;
    ysmr_row *rows;
    long long rows_capacity;
    long long *row_count;
    const BlGains *gains;
    // horizons, the kernel's one source of them: the history length from which a filter's window is full, which is also the
    // ring offset of its leaver -- n_i[0], and n_i[k] of every further filter the handle has; of one it does not have,
    // INT_MAX (never full: one compare per filter gates its load, with no test of n_f)
    alignas(16) int hz[4];
};
typedef const __attribute__((address_space(4))) BlKernArgs *BlKernArgsPtr;
typedef const __attribute__((address_space(4))) BlGains *BlGainsPtr;     // (written once when the handle is made, before any launch)
__device__ __forceinline__ BlKernArgsPtr bl_kernargs()
{
    BlKernArgsPtr p = (BlKernArgsPtr)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(p));          // (opaque: a load through it is not merged with the preloaded arguments)
    return p;
}

// s_waitcnt vmcnt(0) through the builtin: the compiler's own wait insertion then knows that every vector memory access of
// the wave is complete here.  Inline assembly is opaque to it: behind one, the claimed box's load still counted as
// outstanding, and the compiler waited for vmcnt(0) again after the row store -- a store's round trip in every frame.
__device__ __forceinline__ void bl_wait_vmem() { __builtin_amdgcn_s_waitcnt(0x0F70); }     // vmcnt 0, expcnt 7, lgkmcnt 15

// Kernel arguments a phase ahead.  A load through bl_kernargs() is issued where the compiler needs its result and waited
// for a few instructions later: a scalar-cache round trip on the wave's serial chain, in every frame.  These issue the
// s_load where the phase's inputs are known and wait for it where they are used, a barrier's worth of instructions
// later.  The compiler's own wait insertion does not see a load in inline assembly, so the wait is written out, and the
// values are used only as that wait hands them on.  Between the two the compiler believes the registers valid: were it to
// copy, spill or reuse them there, a stale pointer would be used, or the load would land on something else -- and nothing
// at compile time says so.  THE GUARD is scripts/k_batch_census.py: pending_load_hazards, which follows every s_load of
// the kernel's listing along every path to its lgkmcnt(0) wait; tests/test_kernel_round_trips.py runs it on the built
// library and on every variant build it finds, scripts/build_stamps.sh on the stamps build.  Hence also: every wait is
// reached by every wave on every path from its load (none under a test of `alive`).  (An access the compiler does not know of only makes its own
// lgkmcnt(N) waits stricter: LDS returns in order, so "at most N open" still covers every older LDS access.)
struct BlSearchArgs { const float *det_all; int hz[BL_NF]; };
// The rows a buffer of `capacity` still takes behind `base`, in 32 bits.  A launch writes fewer than 2^20 rows (BL_MAX_BATCH
// frames of at most BL_THREADS), so the clamps are never reached by counting down: above INT_MAX everything fits, and a
// buffer that is already overrun (base > capacity: the count goes on past the capacity) takes nothing -- -1, not 0: an
// empty frame fits a full buffer, and does not fit an overrun one (base + 0 > capacity).
__device__ __forceinline__ int bl_room(long long capacity, long long base)
{
    const long long left = capacity - base;
    return left > 0x7FFFFFFFll ? 0x7FFFFFFF : (left < 0 ? -1 : (int)left);
}
// the pointer to the gains: requested behind the row, taken in front of the filter bank (behind the frame's vmcnt(0))
__device__ __forceinline__ unsigned long long bl_gains_issue(BlKernArgsPtr kp)
{
    unsigned long long g;
    asm volatile("s_load_dwordx2 %0, %1, %2" : "=&s"(g) : "s"(kp), "i"(__builtin_offsetof(BlKernArgs, gains)) : "memory");
    return g;
}
__device__ __forceinline__ BlGainsPtr bl_gains_wait(unsigned long long g)
{
    asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(g) :: "memory");
    return (BlGainsPtr)g;
}
// det_all and the horizons: what the loads behind the search need (the claimed box, the ring entries that leave the
// windows).  Requested behind the search, a dozen instructions in front of the claim's atomic; the compiler waits for
// lgkmcnt(0) in front of that atomic, so that is where they are waited for (the written-out wait behind it finds them in).
static_assert(BL_NF <= 4, "one s_load_dwordx4: the horizons");
__device__ __forceinline__ void bl_search_args_issue(BlKernArgsPtr kp, unsigned long long &det_all, bl_u32x4 &hz)
{
    asm volatile("s_load_dwordx2 %0, %2, %3\n\ts_load_dwordx4 %1, %2, %4" : "=&s"(det_all), "=&s"(hz)
                 : "s"(kp), "i"(__builtin_offsetof(BlKernArgs, det_all)), "i"(__builtin_offsetof(BlKernArgs, hz)) : "memory");
}
__device__ __forceinline__ BlSearchArgs bl_search_args_wait(unsigned long long det_all, bl_u32x4 hz)
{
    asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(det_all), "+s"(hz) :: "memory");
    BlSearchArgs a;
    a.det_all = (const float *)(const __attribute__((address_space(1))) float *)det_all;
#pragma unroll
    for (int k = 0; k < BL_NF; ++k) a.hz[k] = (int)hz[k];
    return a;
}

__global__ __launch_bounds__(BL_THREADS) void k_batch(BlKernArgs ka)
{
    const TrackerDev &t = ka.t;
    const BatchDev &bd = ka.bd;
    const int32_t *__restrict__ det_count = ka.det_count;
    const int batch = ka.batch, frame0 = ka.frame0;
    long long *row_count = ka.row_count;
    __shared__ BlShared sh;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const unsigned long long below = (1ull << lane) - 1ull;
    const int md = t.max_det, mdp = bl_md_padded(md);
    const int bufw = bl_grid_dwords_max(md);
    // LDS by offset (bl_lds): THREE tables of the smallest proposing key per column (u64; frame f uses table f % 3, see the
    // frame loop), one table of the winning id per column (u32: the exact claim path's second round and the registration's
    // list, which never overlap -- the registration starts with a barrier), per frame parity the frame's detections
    // (k_bgrid's block); the CPython set model's table
    auto key_at = [&](int k) { return bl_lds + k * mdp; };
    auto cid_at = [&]() { return bl_u32(6 * mdp); };
    auto buf_off = [&](int p) { return 7 * mdp + p * bufw; };
    const int tab_off = 7 * mdp + 2 * bufw;
    const int seats = min(t.capacity, BL_THREADS);
    const int nf = t.n_f;
    const int gone_max = (int)floor(t.max_gone);        // tracker.py:104, 208: disappeared > maxDisappeared, a float
    // (max_disappeared < 32000 for a one-launch handle, so the conversion is exact)
    const int hn[BL_NF] = {ka.hz[0], ka.hz[1], ka.hz[2]};      // (the horizons, BlKernArgs::hz: here for the first frame's mode threshold)

    // ---- start of the batch: counters, this lane's track, the first frame's detections
    int n = *t.n_tracks, next_id = *t.next_id, head = *bd.head & (BL_HB - 1);
    // The rows of the launch: `rowp`, where the next frame's row of rank 0 goes, and `room`, the rows the buffer still
    // takes, in 32 bits (bl_room) -- a frame's capacity decision is then ONE scalar compare, and a row's address one
    // multiply-add on a scalar base.  The row count goes back to HBM as what it was plus what `room` lost (sh.rows_then).
    ysmr_row *rowp = ka.rows + *row_count;
    int room = bl_room(ka.rows_capacity, *row_count);
    if (tid == 0) sh.rows_then = *row_count + room;
    for (int f = tid; f < batch; f += BL_THREADS) {
        int m = det_count[f];
        if (m > md) { m = md; atomicOr(t.err, ERR_DET_CLAMPED); }
        sh.cnt[f] = m < 0 ? 0 : m;
    }
    if (tid < 2) { sh.used[tid] = 0; sh.n_dead[tid] = 0; sh.tie[tid] = -1; }
    // (column 0 of every key table holds a key or all ones from the first frame on, also in frames without detections,
    // whose tables nobody clears: a lane that proposes nothing reads it and compares it with a key no table holds)
    if (tid < 3) key_at(tid)[0] = ~0ull;
    if (tid == 0) sh.top = 0;
    // (the launch's seat events, tracks moved and track waves at its end, behind the ring's head: ysmr_debug_seat_events)
    if (tid == 0) { bd.head[1] = 0; bd.head[2] = 0; bd.head[3] = 0; }
    BlSeat S;
    bl_seat_blank(S);
    if (n > 0 && tid < seats && bd.i32[5 * (size_t)bd.seat_cap + tid]) {     // (an empty table: whatever the flags say)
        bl_seat_load(S, bd, tid);
        S.alive = true;
    }
    // (S.mode is carried as the threshold it implies, bl_grow_at: the frame loop neither reads nor writes it)
    int grow_at = bl_grow_at(S.len, S.mode, nf, hn);
    __syncthreads();
    {   // (the ballot outside the branch: under `lane == 0 &&` only lane 0 would vote)
        const unsigned long long ba = __ballot(S.alive);
        if (lane == 0 && ba) atomicMax(&sh.top, 64 * (wave + 1));
    }
    __syncthreads();
    // The chores of a frame -- the LDS-DMA of the detections two frames ahead, clearing their key table -- go to the waves
    // that hold no track, when there are any: with 9 of 12 waves in use, three of them share one SIMD and set the frame's
    // pace, and the idle waves sit on the other SIMDs.  (Seats are handed out lowest first, so the waves in use are the
    // first ones.)
    int helpers_from = (sh.top + 63) >> 6;               // first wave without a track; BL_WAVES: none
    auto chore_first = [&]() { return helpers_from < BL_WAVES ? tid - 64 * helpers_from : tid; };
    auto chore_stride = [&]() { return helpers_from < BL_WAVES ? 64 * (BL_WAVES - helpers_from) : BL_THREADS; };
    auto dma = [&](int f, int m_f) {        // frame f's block (m_f detections) -> s_buf[f & 1], whole 1-KiB pieces, a wave-instruction each
        const int pieces = bl_grid_dwords(m_f) >> 8;
        const char *src = bd.grid + (size_t)bd.grid_stride * f;
        const int w0 = helpers_from < BL_WAVES ? helpers_from : 0, nw = BL_WAVES - w0;
        for (int c = wave - w0; c >= 0 && c < pieces; c += nw) {
            const uint32_t lds = (uint32_t)(uintptr_t)(bl_u32(buf_off(f & 1) + c * 256));
            const uint32_t off = (uint32_t)c * 1024u + (uint32_t)lane * 16u;
            asm volatile("s_mov_b32 m0, %0\n\tglobal_load_lds_dwordx4 %1, %2" ::"s"(__builtin_amdgcn_readfirstlane(lds)), "v"(off), "s"(src) : "memory");
        }
    };
    // the first two frames' detections and key tables
#pragma nounroll
    for (int k = 0; k < 2 && k < batch; ++k) dma(k, sh.cnt[k]);
    for (int c = tid; c < sh.cnt[0]; c += BL_THREADS) key_at(0)[c] = ~0ull;
    if (batch > 1)
        for (int c = tid; c < sh.cnt[1]; c += BL_THREADS) key_at(1)[c] = ~0ull;
    bl_wait_vmem();
    __syncthreads();

    // ---- the frame loop: ONE workgroup barrier per frame, barrier A behind the claims' atomic round.
    // Between A(f) and A(f + 1) a wave runs, in this order: the ranks and the row of frame f - 1 (settle), the counts; the
    // key read of frame f, ageing / deregistration, registration (rare, with barriers of its own), the filter bank; then
    // the search of frame f + 1 and its claim.  Nothing frame f + 1's search needs waits for the other waves: the lane's
    // own prediction, and the grid block of f + 1, which landed before A(f).  What does need "every wave is past frame
    // f's ageing" -- n_dead / dead_id of frame f, hence the ranks, the row and the counts -- is read behind A(f + 1).
    // What the end-of-frame barrier of earlier versions ordered, and what orders it now (A(f) = barrier A of frame f):
    //   key tables   three.  Table (f + 2) % 3 is cleared for frame f + 2 between A(f) and A(f + 1); its last readers (the
    //                key read, the exact path and the registration's scan of frame f - 1) finished before they arrived at
    //                A(f), which the clearing wave has passed; frame f + 2's atomics come behind A(f + 1).  Behind A(f)
    //                that table is dead, so it is frame f's registration's scratch first; the clearing follows the
    //                registration's last barrier in program order.
    //   cid          one table: the exact path's last read of it and the registration's first write are a barrier apart.
    //   grid blocks  two.  Block f + 2 is requested behind A(f) into the buffer of frame f, last read (search, wave
    //                search) in front of A(f); the requesting waves wait vmcnt(0) in front of A(f + 1), the search of
    //                f + 2 starts behind it.
    //   sh.tie       holds a frame number per parity, compared with the frame's own: no reset, which would race with
    //                the next frame's setters in the same interval.
    //   sh.n_dead    a running count per parity, never reset: written (atomicAdd) between A(f) and A(f + 1), read behind
    //                A(f + 1), written again behind A(f + 2), which every reader has passed.  Every wave keeps the value
    //                a parity's count had when the frame started (d_cur, d_prev: read behind a barrier, so uniform) and
    //                subtracts it.  dead_id likewise: rewritten behind A(f + 2).
    //   sh.used      as before: parity par ^ 1 is reset behind A(f); it was last read by frame f - 1's registration, in
    //                front of A(f), and is next added to behind A(f + 1).
    //   seat block   (rare: a track wave is given up, at the head of frame f, four barriers of its own; every wave takes it
    //                or none.)  Its opening barrier stands behind every wave's frame f - 1: the key table of frame f - 1
    //                and the table of winning ids are dead, and every lane's ring store of frame f - 1 has landed (each
    //                wave waits for its vector memory in front of it -- a helper's grid pieces with it).  The state and
    //                the seat lists are written in front of the second barrier and read behind it; the waves' `alive`
    //                votes in front of the third, sh.top and the ring copy behind it; the closing barrier stands behind
    //                every thread's wait for its copies, and sh.top is read behind it.  helpers_from only falls here, so a
    //                wave that requested grid pieces as a helper is still one where it waits for them.  The table is
    //                cleared for frame f + 2 behind A(f), behind the registration, whose scratch it is next; its column 0
    //                is not touched.  n_dead / dead_id of frame f - 1 are not touched either: the moved tracks' stale ranks
    //                are settled behind A(f), in their new lanes.
    // The claim key carries S.rank as it stood BEFORE frame f - 1's deaths were taken off (they are, behind A(f)).  It is
    // still a valid tie-breaker: for two live tracks a < b (by id) the stale ranks are the true ranks plus the number of
    // frame f - 1's dead with a smaller id, which is no smaller for b than for a -- so stale ranks stay unique among the
    // live tracks, ascend with the id, and stay below the seat count (10 bits).  A birth's rank n + fr is exact: a frame
    // that registers ages nobody (`age` is false when n < m), n has had every earlier frame's deaths taken off behind
    // A(f), and its births are added where they happen.
    int kc = 0;                      // the frame's key table: f % 3
    int d_cur = 0, d_prev = 0;       // sh.n_dead[par], sh.n_dead[par ^ 1] as they stood before frame f, frame f - 1
    double o0 = 0.0, o1 = 0.0;       // the filter bank's outputs: a frame's row leaves behind the next frame's barrier A
    // ranks, row and counts of frame `fr`, whose deaths were counted in sh.n_dead[slot] from `start` on; behind the barrier
    // that follows the frame's ageing.  Returns the running count.
    auto settle = [&](int slot, int start, int fr, bool row) {
        const int total = __builtin_amdgcn_readfirstlane(sh.n_dead[slot]);      // (uniform: one lane move serves the count and the return)
        const int n_dead = total - start;
#ifdef YSMR_STAMPS
        if (lane == 0 && n_dead) { g_bcounts[wave][6] += 1; g_bcounts[wave][7] += n_dead; }
#endif
        if (n_dead && S.alive)
            for (int k = 0; k < n_dead; ++k) S.rank -= sh.dead_id[slot][k] < S.id;
        n -= n_dead;
        if (row) {
            // Every live lane has rank < n, so a frame whose n rows fit decides nothing per lane; the frame that does not
            // fit is the one that raises ERR_ROWS_CAPACITY, and only it compares ranks (rank < room: base + rank < capacity).
            bool fits = S.alive;
            if (n > room) {
                fits = S.alive && S.rank < room;
                if (tid == 0) atomicOr(bl_kernargs()->t.err, ERR_ROWS_CAPACITY);
            }
            if (fits) {      // track_eval.py:313-316
                // (the box and `gone` first: their four registers are put together for the store, the position's are not --
                // the same 40 bytes as one struct assignment, which can come back if a later compiler's allocation keeps
                // tests/test_kernel_bookkeeping.py's limit on ranks + row without this order)
                ysmr_row *rp = rowp + S.rank;
                rp->w = S.info[0]; rp->h = S.info[1]; rp->angle = S.info[2];
                rp->disappeared = S.gone;
                rp->frame = frame0 + fr;
                rp->track_id = S.id;
                rp->x = o0; rp->y = o1;
            }
            rowp += n; room -= n;
        }
        return total;
    };
    // The frame's constants a frame ahead: the count and the grid header of frame f + 1 are fixed before the launch and in
    // LDS before A(f) (the block of f + 1 landed in front of it), so they are read behind A(f), where every wave has just
    // waited anyway, and the head of the next search starts from registers.  The count of frame f + 2 is read there for
    // the LDS-DMA and the key clearing, and moves up a frame with each pass: ONE read of sh.cnt per frame.
    int mv_cur = sh.cnt[0], mv_next = sh.cnt[batch > 1 ? 1 : 0];      // (uniform, kept in vector registers: scalar ones are short)
    float4 hdr_cur = bl_grid_header(buf_off(0));
    for (int f = 0; f < batch; ++f) {
        const int par = f & 1;
        const int kn = kc == 2 ? 0 : kc + 1, ks = 3 - kc - kn;      // the tables of frame f + 1, and of f + 2 = f - 1 (the third of 0, 1, 2)
        const int m = __builtin_amdgcn_readfirstlane(mv_cur);
        BLSTAMP(0);
        BLSTAMP_AT(f == YSMR_BL_STEADY, 2);
#ifdef YSMR_STAMPS
        if (f == 0 && lane == 0)
            for (int k = 0; k < BL_COUNTS; ++k) g_bcounts[wave][k] = 0;
        if (f == 0 && tid == 0) {      // (in front of the seat block, which counts into them)
            g_bseats[0] = g_bseats[1] = 0;
            for (int k = 0; k <= BL_WAVES; ++k) g_bwaves[k] = 0;
        }
        BLCOUNT(5, ((frame0 + f) & (BL_REFRESH - 1)) == 0 && S.alive && t.use_gsff);
#endif
        // ---- a track wave is given up (rare): the live tracks fit in fewer waves than hold one.  `n` is stale by the
        // deaths of the frame before (they come off behind barrier A), which only makes the test conservative.
        if (((n + 63) >> 6) + BL_SEAT_SLACK_WAVES < helpers_from) {
            // (the thread, its wave and lane as values of this frame, as in the registration)
            // (and the table's number: held from here it would take a scalar register through the search of every frame)
            int tl = tid, wv = wave, ln = lane, mp = mdp, kd = kc;
            asm volatile("" : "+v"(tl), "+s"(wv), "+v"(ln), "+s"(mp), "+s"(kd));
            kd = 3 - kd - (kd == 2 ? 0 : kd + 1);
            const int keep = (n + 63) >> 6;                  // the waves that stay track waves
            // The live lanes at and above wave `keep` move into the free lanes below it, highest wave first, mover k into
            // the k-th free lane.  The state passes through the key table of frame f - 1 (dead behind the opening barrier,
            // cleared for frame f + 2 behind barrier A; column 0 stays as it is, see the prologue), the seat numbers through
            // the table of winning ids.  What the table does not hold stays seated and moves in the next frame.
            // (what the block keeps across its barriers, in vector registers: scalar ones are short)
            int room_for = (mp - 1) / BL_MOVE_WORDS;
            unsigned long long *box = bl_lds + kd * mp + 1;
            uint32_t *seat_of = bl_u32(6 * mp);
            int role = S.alive ? (tl >= 64 * keep ? 1 : 0) : (tl < min(64 * keep, seats) ? 2 : 0);      // 1: mover, 2: target
            int mr, tr;
            {
                const unsigned long long b_mv = __ballot(role == 1), b_tg = __ballot(role == 2);
                if (ln == 0) { sh.wave_cnt[0][wv] = (int)__popcll(b_mv); sh.wave_cnt[1][wv] = (int)__popcll(b_tg); }
                mr = (int)__popcll(b_mv & below); tr = (int)__popcll(b_tg & below);
            }
            asm volatile("" : "+v"(role), "+v"(room_for), "+v"(mr), "+v"(tr));
            // (this lane's ring store of the frame before has landed: another thread copies it below)
            bl_wait_vmem();
            __syncthreads();
            int movers = 0;
#pragma unroll
            for (int k = 0; k < BL_WAVES; ++k) {
                const int v = sh.wave_cnt[0][k];
                mr += k > wv ? v : 0; movers += v;
                tr += k < wv ? sh.wave_cnt[1][k] : 0;
            }
            int n_mov = min(movers, room_for);
            asm volatile("" : "+v"(n_mov));
            if (role == 1 && mr >= n_mov) role = 0;      // (does not fit the table: stays seated)
            if (role == 2 && tr >= n_mov) role = 0;
            asm volatile("" : "+v"(role));
            if (role == 1) {
                unsigned long long *p = box + mr;
                int j = 0;
                auto put = [&](double v) { p[room_for * j++] = (unsigned long long)__double_as_longlong(v); };
                auto put2 = [&](uint32_t lo, uint32_t hi) { p[room_for * j++] = (unsigned long long)lo | ((unsigned long long)hi << 32); };
#pragma unroll
                for (int k = 0; k < BL_NF; ++k) {
                    put(S.s0x[k]); put(S.s1x[k]); put(S.s0y[k]); put(S.s1y[k]); put(S.w[k]); put(S.xa[k]); put(S.xb[k]);
                }
                put(S.px); put(S.py); put(o0); put(o1);
                put2(__float_as_uint(S.info[0]), __float_as_uint(S.info[1]));
                put2(__float_as_uint(S.info[2]), (uint32_t)S.id);
                put2((uint32_t)S.gone, (uint32_t)S.len);
                put2((uint32_t)S.rank, (uint32_t)grow_at);
                seat_of[mr] = (uint32_t)tl;
            }
            if (role == 2) seat_of[room_for + tr] = (uint32_t)tl;
            __syncthreads();
            if (role == 1) {
                bl_seat_blank(S);
                grow_at = 0; o0 = o1 = 0.0;
            }
            if (role == 2) {
                const unsigned long long *p = box + tr;
                int j = 0;
                auto get = [&]() { return __longlong_as_double((long long)p[room_for * j++]); };
                auto get2 = [&](uint32_t &lo, uint32_t &hi) { const unsigned long long v = p[room_for * j++]; lo = (uint32_t)v; hi = (uint32_t)(v >> 32); };
#pragma unroll
                for (int k = 0; k < BL_NF; ++k) {
                    S.s0x[k] = get(); S.s1x[k] = get(); S.s0y[k] = get(); S.s1y[k] = get(); S.w[k] = get(); S.xa[k] = get(); S.xb[k] = get();
                }
                S.px = get(); S.py = get(); o0 = get(); o1 = get();
                uint32_t a, b;
                get2(a, b); S.info[0] = __uint_as_float(a); S.info[1] = __uint_as_float(b);
                get2(a, b); S.info[2] = __uint_as_float(a); S.id = (int)b;
                get2(a, b); S.gone = (int)a; S.len = (int)b;
                get2(a, b); S.rank = (int)a; grow_at = (int)b;
                S.alive = true;
            }
            {
                const unsigned long long b_live = __ballot(S.alive);
                if (ln == 0) sh.wave_cnt[0][wv] = b_live != 0ull;
            }
            __syncthreads();
            if (tl == 0) {      // one past the highest seat in use, set, not raised: between two barriers
                int top = 0;
#pragma unroll
                for (int k = 0; k < BL_WAVES; ++k) top = sh.wave_cnt[0][k] ? 64 * (k + 1) : top;
                sh.top = top;
                int *seen = bl_kernargs()->bd.head;      // (ysmr_debug_seat_events: events and tracks moved of this launch)
                atomicAdd(seen + 1, 1); atomicAdd(seen + 2, n_mov);
#ifdef YSMR_STAMPS
                g_bseats[0] += 1; g_bseats[1] += n_mov;
#endif
            }
            // The ring goes with the seat: the 32 entries of every mover (not the line of zeros), one entry of one mover per
            // thread and pass, past this unit's L1 as every ring load.  The copies have landed before the closing barrier.
            {
                double2 *ring = bl_kernargs()->bd.ring;
                const size_t sc = (size_t)bl_kernargs()->bd.seat_cap;
                for (int i = tl; i < n_mov * BL_HB; i += BL_THREADS) {
                    const int k = i / BL_HB, e = i & (BL_HB - 1);
                    *reinterpret_cast<bl_u32x4 *>(ring + e * sc + seat_of[room_for + k]) = bl_ring_load16(ring + e * sc + seat_of[k]);
                }
            }
            bl_wait_vmem();
            __syncthreads();
            helpers_from = (sh.top + 63) >> 6;
        }
#ifdef YSMR_STAMPS
        if (tid == 0) atomicAdd(&g_bwaves[helpers_from], 1ull);      // (no return value: nothing in the frame waits for a load)
#endif
        BLSTAMP_AT(f == YSMR_BL_FRAME && ((frame0 + f) & (BL_REFRESH - 1)) == 0, 0);
        if (((frame0 + f) & (BL_REFRESH - 1)) == 0 && S.alive && t.use_gsff) {     // (uniform but for `alive`: see bl_sums_from_ring)
            // (the lane's own ring stores of the frame before are complete, and nothing of the ring is left outstanding
            // in the compiler's books: it would otherwise wait for vmcnt(0) -- the row stores -- in the search of every frame)
            bl_wait_vmem();
            // (the horizons from the argument segment, here where they are needed once in BL_REFRESH frames; a filter the
            // handle does not have: 0)
            const BlKernArgsPtr kh = bl_kernargs();
            const int h1 = kh->hz[1], h2 = kh->hz[2];
            bl_sums_from_ring<true>(S, bd, tid, head, kh->hz[0], h1 == 0x7FFFFFFF ? 0 : h1, h2 == 0x7FFFFFFF ? 0 : h2);
            bl_wait_vmem();
        }
        BLSTAMP_AT(f == YSMR_BL_FRAME && ((frame0 + f) & (BL_REFRESH - 1)) == 0, 1);
        // ---- each track proposes its nearest detection (tracker.py:151-163)
        const bool propose = S.alive && m > 0;
        const BlGridView gv = bl_grid_view(buf_off(par), m, hdr_cur);
        BlNear nr{0.0, 0.f, 0.f, 0, true};
        // (a lane that proposes nothing: a key no column can hold -- a squared distance has no sign bit, an empty column is
        // all ones -- so that `the column's winner is my key` needs no `and I proposed`)
        unsigned long long key = 1ull << 63;
        if (propose) nr = bl_search(gv, S.px, S.py, m);
#ifdef YSMR_STAMPS
        {   // (bl_search's test for the candidate list, repeated)
            bool block = false;
            if (propose) {
                const int cx = (int)floorf(((float)S.px - gv.x0) * gv.inv), cy = (int)floorf(((float)S.py - gv.y0) * gv.inv);
                block = gv.lists < 0 || cx < 0 || cx >= gv.G || cy < 0 || cy >= gv.G ||
                        (reinterpret_cast<const uint4 *>(bl_u32(gv.lists))[cy * gv.G + cx].x & 0xFFFFu) == 0xFFFFu;
            }
            BLCOUNT(0, block);
            const unsigned long long bb = __ballot(block);
            if (lane == 0) g_bcounts[wave][1] += __popcll(bb);
        }
#endif
        BLSTAMP(11);
        {   // the lanes bl_search did not settle (a second candidate within its float band, or a block that does not settle
            // the lane), one after the other, by the whole wave
            unsigned long long todo = __ballot(propose && !nr.done);
#ifdef YSMR_STAMPS
            if (f == YSMR_BL_FRAME && lane == 0) g_bstamps[wave][12] = __popcll(todo);
            // (the shader clock over frames 8 .. 56: s_memrealtime counts at a constant 100 MHz; column 15 of rows 0 .. 3)
            if (wave == 0 && lane == 0 && (f == 8 || f == 56)) {
                unsigned long long rt_;
                asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(rt_) :: "memory");
                g_bstamps[f == 8 ? 0 : 1][15] = rt_;
                g_bstamps[f == 8 ? 2 : 3][15] = __builtin_amdgcn_s_memtime();
            }
            if (lane == 0) { if (f == 0) { g_bstamps[wave][13] = 0; g_bstamps[wave][14] = 0; } g_bstamps[wave][13] += __popcll(todo); g_bstamps[wave][14] += todo ? 1 : 0; }
#endif
            while (todo) {
                const int l = __builtin_ctzll(todo);
                todo &= todo - 1ull;
                const BlNear w = bl_search_wave(gv, lane_value(S.px, l), lane_value(S.py, l), m, lane);
                if (lane == l) nr = w;
                // (nothing of the wave search is left in flight where the steady path goes on: the compiler would wait for
                // it at the first register it shares with the claim, which may be right behind the scalar loads below)
                __builtin_amdgcn_s_waitcnt(0xC07F);      // lgkmcnt 0 (vmcnt 63, expcnt 7)
            }
        }
        unsigned long long sa_det;       // (det_all and the horizons: requested here, used behind the claim's atomic)
        bl_u32x4 sa_hz;
        bl_search_args_issue(bl_kernargs(), sa_det, sa_hz);
        // ---- claims (tracker.py:151-189): a column goes to the proposer with the smallest (distance, id)
        // ONE key per proposal: the bits of the squared distance s without their ten lowest (a non-negative double orders
        // like its bits), and in their place the lane's table row -- below 768, unique among the live tracks, ascending
        // with the id (the order the reference breaks ties in, tracker.py:158), as the settling of the frame before last
        // or a registration left it (stale by the last frame's deaths: see above the loop).  The smallest key of a column
        // is its winner unless two proposals are so close that the dropped bits could matter: their s agree in the 54 bits kept, or differ by one step there (a pair a few ulps
        // apart can straddle a truncation boundary).  Only then can two different s round to the same root, or the smaller
        // s belong to the higher row.  Every other key lies at least two steps above the minimum: its s is larger by more
        // than 2^-43 of it, its root differs, and it loses under the exact rule too.
        // Such a pair is noticed from what the atomic returns.  Let M be the column's final minimum and X another key
        // within one step of M.  Whichever of the two did its atomic later got back a value between M (the column never
        // goes below its final minimum) and the earlier one's key (already in place): a value within the band of both, so
        // that lane raises the frame's flag.  Keys farther above M need no flag.
        if (propose) {
            key = ((unsigned long long)__double_as_longlong(nr.s) & ~0x3FFull) | (unsigned long long)S.rank;
            // (the key's half of the band test in front of the atomic: behind it, on the wave's serial chain, the test is a
            // shift, an add and a compare.  The same arithmetic modulo 2^64 as (before >> 10) - (key >> 10) + 1; written
            // this way for tests/test_kernel_bookkeeping.py's limit on the claims -- it can go back to the one expression
            // if a later compiler's allocation makes room)
            unsigned long long band = 1ull - (key >> 10);
            asm volatile("" : "+v"(band));
            const unsigned long long before = atomicMin(&key_at(kc)[nr.col], key);
            if ((before >> 10) + band <= 2ull) sh.tie[par] = f;     // (an empty column: 2^54 - 1, far from every s)
        }
        // the measurements that leave the filters' windows with this frame (used behind the claims): requested where the
        // window is full, 0.0 elsewhere -- bl_gsff then uses them as they are (a track born in this frame has none: its
        // seeding supplies them).  An entry a lane reads here it wrote itself, frames ago as a rule; in the frame before
        // only when the track was born in it, and that frame waited for its ring stores (below, behind the filter bank).
        // The box of the proposed detection, requested before the claim is settled (a proposer that loses its column has
        // asked for nothing it uses; behind the claim's atomic, in front of which det_all and the horizons have arrived) and taken in front of the filter bank: behind barrier A the load would be the
        // youngest in flight where the filter bank waits for the leaving measurements, and the wait for those -- counted
        // in order -- would wait for it as well, a round trip to HBM a few dozen instructions old.
        const BlSearchArgs sa = bl_search_args_wait(sa_det, sa_hz);
        // (every lane asks: a lane that proposed nothing has column 0, whose five floats lie inside frame f's block of
        // det_all whatever the frame holds, and uses nothing of it -- `mine` implies `propose`.  No exec region, no zeros.)
        float bx[3];
        {
            // (frame and column in 32 bits -- batch x max_det detections are far below 2^32 -- then bytes in 64)
            const float *d = sa.det_all + (size_t)((unsigned)f * (unsigned)md + (unsigned)nr.col) * 5;
            bx[0] = d[2]; bx[1] = d[3]; bx[2] = d[4];
        }
        // ONE exec region for the three filters: where a window is not full (a filter the handle lacks: hz = INT_MAX) the
        // lane reads the ring's line of zeros, position BL_HB, which nothing ever stores to -- a select of the position,
        // not of the value: an entry that was never written may hold anything, and bl_gsff<true> needs exactly 0.0, 0.0.
        // (whole entries, one 16-byte load each, outside the compiler's books: bl_ring_issue16; taken behind the frame's
        // wait for vector memory, in front of the filter bank)
        bl_u32x4 leaving[BL_NF];
        if (S.alive && t.use_gsff) {
            const unsigned line = (unsigned)bd.seat_cap * (unsigned)sizeof(double2);
#pragma unroll
            for (int k = 0; k < BL_NF; ++k) {
                const unsigned pos = S.len >= sa.hz[k] ? (unsigned)((head - sa.hz[k]) & (BL_HB - 1)) : (unsigned)BL_HB;
                bl_ring_issue16(bd, tid, __umul24(pos, line), leaving[k]);      // (33 lines of 768 seats: 24 bits hold a line)
            }
        }
        BLSTAMP(1);
        // (the waves that requested a grid block behind the barrier before: it has landed.  Track waves beside helper
        // waves requested none and wait for no vector memory access here: their row and ring stores go on in flight)
        if (helpers_from >= BL_WAVES || wave >= helpers_from) bl_wait_vmem();
        block_sync<true>();
        BLSTAMP(2);
        // ---- behind barrier A: every wave is past frame f - 1's ageing and registration, and past frame f's search
        if (tid == BL_THREADS - 1) sh.used[par ^ 1] = 0;
        // (frame f + 2's count; frame f + 1's header -- past the batch's end nobody uses either, and the read stays inside
        // the kernel's own LDS)
        const int c_ahead = sh.cnt[f + 2 < batch ? f + 2 : f];
        const float4 hdr_next = bl_grid_header(buf_off(par ^ 1));
        // (in the same LDS round: every lane reads a key -- column 0 where it proposed nothing -- and the flag rides along)
        const unsigned long long k_won = key_at(kc)[nr.col];
        const int exact = sh.tie[par] == f;
        if (f + 2 < batch) dma(f + 2, __builtin_amdgcn_readfirstlane(c_ahead));
        const int d_total = settle(par ^ 1, d_prev, f - 1, f > 0);
        const unsigned long long gains_pending = bl_gains_issue(bl_kernargs());
        BLSTAMP(3);
        unsigned long long won = k_won;      // (`mine` is ONE compare behind the rare block: a vote on it is that compare's mask)
        if (exact) {
            // The exact rule, for every column of the frame (uniform: the flag was set before barrier A and stands until
            // frame f + 2 sets it again, behind A(f + 1)): the smallest s in full, then the proposers at the column's
            // smallest DISTANCE contend by id.  sqrt is monotone, so that is the smallest s -- and an s a few ulps above it that rounds to the same
            // root: only those take the square roots.  A wave that comes here late may have read a key above that the
            // clearing had already replaced; its `mine` is set again below.
#ifdef YSMR_STAMPS
            if (wave == 0 && lane == 0) g_bcounts[0][8] += 1;
#endif
            for (int c = tid; c < m; c += BL_THREADS) { key_at(kc)[c] = ~0ull; cid_at()[c] = 0xFFFFFFFFu; }
            block_sync<true>();
            if (propose) {
                key = (unsigned long long)__double_as_longlong(nr.s);
                atomicMin(&key_at(kc)[nr.col], key);
            }
            block_sync<true>();
            if (propose) {
                const unsigned long long kmin = key_at(kc)[nr.col];
                bool tie = key == kmin;
                if (!tie) {
                    const double smin = __longlong_as_double((long long)kmin);
                    if (nr.s <= smin + smin * 0x1p-48) tie = sqrt(nr.s) == sqrt(smin);
                }
                if (tie) atomicMin(&cid_at()[nr.col], (uint32_t)S.id);
            }
            block_sync<true>();
            won = propose && cid_at()[nr.col] == (uint32_t)S.id ? key : ~key;
        }
        const bool mine = won == key;
        const unsigned long long bm = __ballot(mine);      // (here, beside the compare: its mask IS the vote)
        BLSTAMP(4);
        // ---- ageing and deregistration (tracker.py:95-107, 198-211)
        // (tracker.py ages when there are no detections, or when n > 0 and n >= m, and registers when m > 0 and n == 0 or
        // n < m.  Counts are never negative, so the two are `n >= m` and `n < m`: one scalar compare, each the other's
        // complement.)
        const bool births = n < m, age = !births;
        double z0 = S.px, z1 = S.py;
        bool fresh = false, died = false;
        if (mine) {
            z0 = (double)nr.zx; z1 = (double)nr.zy;
            S.gone = 0;      // (the claimed box: in front of the filter bank)
        } else if (S.alive && age) {
            ++S.gone;
            S.info[0] = S.info[1] = S.info[2] = 0.f;
            if (S.gone > gone_max) { S.alive = false; died = true; }
        }
        {
            const unsigned long long bx = __ballot(died);
            if (lane == 0 && bm) atomicAdd(&sh.used[par], (int)__popcll(bm));
            if (bx) {      // the ids of the deregistered tracks: every younger track moves up one table row (settle)
                int at = 0;
                if (lane == 0) at = atomicAdd(&sh.n_dead[par], (int)__popcll(bx));
                at = __builtin_amdgcn_readfirstlane(at) - d_cur;
                if (died) sh.dead_id[par][at + __popcll(bx & below)] = S.id;
            }
        }
        BLSTAMP(5);
        // ---- registration (tracker.py:135-137, 212-217): unclaimed columns become tracks, in CPython set order
        // (`births`, above: uniform; nobody was aged in such a frame)
#ifdef YSMR_STAMPS
        BLCOUNT(4, births);
#endif
        if (births) {
            // (the thread, its wave and lane as values of this frame: the compiler hoisted the comparisons with them out of
            // the frame loop, a pair of scalar registers each, held for the whole launch and spilled into vector lanes)
            int tl = tid, wv = wave, ln = lane, mp = mdp;
            asm volatile("" : "+v"(tl), "+s"(wv), "+v"(ln), "+s"(mp));
            // scratch: the key table of frame f - 1, dead behind A(f) and cleared for frame f + 2 below
            int *unused = reinterpret_cast<int *>(key_at(ks)), *newcols = unused + mp;
            uint32_t *list = cid_at();
            __syncthreads();
            int n_new = 0, n_new_all = 0;
            if (n == 0) {
                for (int c = tl; c < m; c += BL_THREADS) newcols[c] = c;
                n_new_all = m;
            } else {
                // the unclaimed columns in ascending order: K consecutive columns per thread, ranked by a wave scan
                const int K = (m + BL_THREADS - 1) / BL_THREADS;
                const int c0 = tl * K, c1 = min(c0 + K, m);
                int cnt = 0;
                for (int c = c0; c < c1; ++c) cnt += key_at(kc)[c] == ~0ull;      // (a column with a proposer has a winner)
                int incl = cnt;
#pragma unroll
                for (int d = 1; d < 64; d <<= 1) { const int o = __shfl_up(incl, d); if (ln >= d) incl += o; }
                if (ln == 63) sh.wave_cnt[0][wv] = incl;
                __syncthreads();
                int at = incl - cnt, total = 0;
#pragma unroll
                for (int k = 0; k < BL_WAVES; ++k) { const int v = sh.wave_cnt[0][k]; at += k < wv ? v : 0; total += v; }
                for (int c = c0; c < c1; ++c)
                    if (key_at(kc)[c] == ~0ull) unused[at++] = c;
                __syncthreads();
                int cnt_set = cpython_order_lds<BL_THREADS, BL_TABLE>(unused, total, m, sh.used[par], newcols, bl_u32(tab_off), list, sh.set_state);
                if (cnt_set < 0) { if (tl == 0) atomicOr(bl_kernargs()->t.err, ERR_TRACK_CAPACITY); cnt_set = 0; }
                n_new_all = cnt_set;
            }
            n_new = n_new_all;
            if (n + n_new > seats) {
                if (tl == 0) atomicOr(bl_kernargs()->t.err, ERR_TRACK_CAPACITY);
                n_new = seats - n;
            }
            // free lanes take the new tracks, in lane order
            const bool free_lane = !S.alive && tl < seats;
            const unsigned long long bf = __ballot(free_lane);
            if (ln == 0) sh.wave_cnt[1][wv] = (int)__popcll(bf);
            __syncthreads();
            int fr = (int)__popcll(bf & below);
#pragma unroll
            for (int k = 0; k < BL_WAVES; ++k) fr += k < wv ? sh.wave_cnt[1][k] : 0;
            if (free_lane && fr < n_new) {
                const int c = newcols[fr];
                const float *d = bl_kernargs()->det_all + ((size_t)f * md + c) * 5;
                z0 = (double)d[0]; z1 = (double)d[1];
                S.info[0] = d[2]; S.info[1] = d[3]; S.info[2] = d[4];
                S.id = next_id + fr; S.rank = n + fr; S.gone = 0;
                S.len = 0; grow_at = 0;      // (no history: the filter bank seeds it)
                S.alive = true; fresh = true;
                atomicMax(&sh.top, tl + 1);
            }
            // (the counts take the births where they happen: nothing between here and the settling reads them, and the
            // deaths -- none in this frame -- come off behind the next barrier A)
            n += n_new;
            next_id += n_new_all;
            // (a wave that stops being a helper here has requested its pieces of a grid block: they land before it
            // forgets; __syncthreads: the lists lived in the table that is cleared next, and sh.top is complete)
            bl_wait_vmem();
            __syncthreads();
            helpers_from = (sh.top + 63) >> 6;
        }
        // The keys of frame f + 2 are cleared here, by the waves that would otherwise wait at barrier A: see above the loop
        // (behind the registration, whose scratch this table was)
        if (f + 2 < batch)
            for (int c = chore_first(); c >= 0 && c < c_ahead; c += chore_stride()) key_at(ks)[c] = ~0ull;
        // ---- the filter bank (tracker.py:219-227)
        BLSTAMP(6);
        // The one wait for vector memory of a track wave's frame: the leaving measurements and the box, requested in front
        // of barrier A, and with them (the count is in order) the row stores of the frame before, a hundred instructions
        // old.  For every lane, with or without a track: the compiler then knows that no load is in flight at the head of
        // the loop, and does not guard the search's registers with waits that would catch the ring store.
        bl_wait_vmem();
        BLSTAMP_OWN_TEST(8);
        bl_ring_taken16(leaving);
        // (the gains' pointer, requested behind the row: taken here by EVERY wave, with or without a live track -- a load
        // left in flight would land in registers the compiler has meanwhile given to something else)
        const BlGainsPtr gq = bl_gains_wait(gains_pending);
        if (mine) { S.info[0] = bx[0]; S.info[1] = bx[1]; S.info[2] = bx[2]; }
        o0 = z0; o1 = z1;
#ifdef YSMR_STAMPS
        const int mode_before = grow_at;      // (the threshold moves when the mode does)
        BLCOUNT(2, S.alive && t.use_gsff && fresh);
#endif
        if (S.alive) {
            if (t.use_gsff) {
                // (the twelve gain constants are read in every frame: as kernel arguments they sat in 24 scalar registers for
                // the whole launch, and this kernel spilled 113 of them into vector lanes -- a tenth of a frame's vector
                // instructions were v_readlane / v_writelane.  Through a pointer in the CONSTANT address space they come out
                // of the scalar cache, s_load_dwordx16 + s_load_dwordx8 and one wait; a plain pointer that went through the
                // asm below came back generic, and the listing had six flat_load_dwordx4 per wave and frame with two
                // vmcnt(0) lgkmcnt(0) waits in the middle of the float64 chain: tests/test_kernel_listing.py)
                // (hist_cap, lik_min and the rare block's horizons likewise: read from the argument segment here, beside the
                // gains, they hold no scalar register across the frame)
                bl_gsff<true>(S, t, bl_kernargs()->t, bd, *gq, tid, head, leaving, z0, z1, fresh, grow_at, o0, o1);
            }
            else { S.px = z0; S.py = z1; }
        }
#ifdef YSMR_STAMPS
        BLCOUNT(3, S.alive && t.use_gsff && !fresh && grow_at != mode_before);
#endif
        // (a frame that registered: the seeding's ring stores are complete before the next frame reads the entries that
        // leave the new tracks' windows -- the only ring entries a lane reads in the frame after it wrote them)
        if (births) bl_wait_vmem();
        // (the search below is the next frame's: nothing of it is scheduled into the filter bank, nor the reverse --
        // scripts/k_batch_census.py ends the filter bank's phase at its last float64 instruction / the ring store)
        __builtin_amdgcn_sched_barrier(0);
        BLSTAMP(7);
        BLSTAMP_AT(f == YSMR_BL_STEADY, 3);
        d_prev = d_cur; d_cur = d_total;
        kc = kn;
        head = (head + 1) & (BL_HB - 1);
        mv_cur = mv_next; mv_next = c_ahead; hdr_cur = hdr_next;
    }
    // ---- the last frame's ranks, row and counts, behind a barrier that every wave's ageing of it has reached
    block_sync<true>();
    settle((batch - 1) & 1, d_prev, batch - 1, true);
    // ---- end of the batch: the small state goes back to HBM, seat by seat
    {
        const BlKernArgsPtr ke = bl_kernargs();
        BatchDev be;                       // (field by field: the structure lies in the constant address space)
        be.ring = ke->bd.ring; be.f64 = ke->bd.f64; be.f32 = ke->bd.f32; be.i32 = ke->bd.i32; be.head = ke->bd.head;
        be.grid = ke->bd.grid; be.grid_stride = ke->bd.grid_stride; be.seat_cap = ke->bd.seat_cap;
        if (tid < seats) {
            be.i32[5 * (size_t)be.seat_cap + tid] = S.alive ? 1 : 0;
            S.mode = bl_mode_of(grow_at, ke->t.n_f, {ke->hz[0], ke->hz[1], ke->hz[2]});
            if (S.alive) bl_seat_store(S, be, tid);
        }
        if (tid == 0) { *ke->t.n_tracks = n; *ke->t.next_id = next_id; *ke->row_count = sh.rows_then - room; *be.head = head; }
        {   // (the highest wave that ends the launch with a track, + 1: ysmr_debug_track_waves)
            const unsigned long long b_live = __ballot(S.alive);
            if (lane == 0 && b_live) atomicMax(be.head + 3, wave + 1);
        }
    }
}

// ---- the split link's second kernel with a track per LANE (round 5) ------------------------------------------------
// Tables beyond k_batch's 768 seats (4K: ~5 000 tracks) link with two launches per frame: k_link DECIDES (one workgroup), then
// every track applies its claim, runs its filter bank, writes its row and finds its nearest detection of the next frame.  That
// second kernel was k_track, a WAVE per track: 5 000 waves every frame, whose tail waits for wave slots that the detection
// kernels of the next batch hold (12 us alone, 19 beside them: profiles/r04_timeline_4k.txt).  k_track_lanes does the same per
// LANE with the batch link's arithmetic: the filter bank as window sums over an HBM ring (bl_gsff: four operations per filter
// and coordinate, four ring entries per frame), the state seat-major by SLOT (a track keeps its slot for life), the row
// minimum from the 3 x 3 cells of the next frame's grid around the prediction in exact float64, then from the 5 x 5 for the
// lanes that leaves open -- 20 workgroups of 256 lanes instead of 1 250 of four waves.  What neither settles (a prediction
// farther from every detection than the block reaches, or more candidates than slots) goes to the wave, one lane at a time,
// through k_track's own rowmin_grid / rowmin_wave.
// Measured (profiles/r05_link_4k_lanes.log): as fast as k_track, not faster -- 21 us per launch beside detection,
// 14.7 with no lane falling through.  The kernel is a chain of dependent rounds of loads at 1.5-2 us each (data k_link wrote on
// another XCD, HBM busy with the next batch's detection), six of them; arithmetic and gathers are ~2 us.  Hence the order of
// the loads below: whatever hangs on the row or on the slot alone is requested in the first round that can, and before stores.
// A handle that can (three filters of <= 31 frames, affine gains) keeps its filter state in this layout from the start:
// ysmr_tracker_update, ysmr_tracker_run and the peeks need no conversion; rec / hist of the per-slot layout stay unused.
// bd.i32 row 0 holds the id the slot's filter state belongs to (-1: none): a slot whose track id differs is a new track.

// nearest detection of (px, py) among the (2 REACH + 1)^2 cells around it, exactly (rowmin_grid's rules: smallest squared
// distance; the lowest column among the equal ROUNDED distances); false: the block does not settle it (nothing in it, something
// outside it could be nearer, or it holds more than SLOTS candidates).  Two rounds of loads -- the bounds of the block's row-runs,
// then every candidate's centre and column at once into registers, the runs laid end to end over the slots: a loop that fetched
// a candidate per iteration was a chain of round trips (the first build of k_track_lanes: 26-36 us per launch).
template <int REACH, int SLOTS>
__device__ __forceinline__ bool bl_rowmin_lane(const DetGrid &g, const GridHdr &gh, double px, double py, int m, double &d_min, int &arg)
{
    constexpr int ROWS = 2 * REACH + 1;
    const double x0 = (double)gh.x0, y0 = (double)gh.y0, cell = (double)gh.cell, inv = (double)gh.inv;
    int cx = (int)floor((px - x0) * inv), cy = (int)floor((py - y0) * inv);
    cx = cx < 0 ? 0 : (cx > GRID_N - 1 ? GRID_N - 1 : cx);
    cy = cy < 0 ? 0 : (cy > GRID_N - 1 ? GRID_N - 1 : cy);
    const int xl = max(cx - REACH, 0), xh = min(cx + REACH, GRID_N - 1), yl = max(cy - REACH, 0), yh = min(cy + REACH, GRID_N - 1);
    const double inf = __longlong_as_double(0x7FF0000000000000ll);
    int a[ROWS], e[ROWS + 1];        // first entry of each row's run; the runs laid end to end: run r takes slots e[r] .. e[r + 1] - 1
    e[0] = 0;
#pragma unroll
    for (int r = 0; r < ROWS; ++r) {
        const int iy = min(yl + r, GRID_N - 1);
        a[r] = g.start[iy * GRID_N + xl];
        const int b = g.start[iy * GRID_N + xh + 1];
        e[r + 1] = e[r] + (yl + r > yh ? 0 : b - a[r]);
    }
    const int n_all = e[ROWS];
    float2 c[SLOTS];
    int col[SLOTS];
#pragma unroll
    for (int k = 0; k < SLOTS; ++k) {
        int q = a[0] + k;
#pragma unroll
        for (int r = 1; r < ROWS; ++r) q = k >= e[r] ? a[r] + (k - e[r]) : q;
        q = min(q, m - 1);                              // (a slot behind the runs reads some entry and is masked below)
        c[k] = g.xy[q];
        col[k] = g.items[q];
    }
    double sq[SLOTS], s_min = inf;
#pragma unroll
    for (int k = 0; k < SLOTS; ++k) {
        const double dx = px - (double)c[k].x;
        const double dy = py - (double)c[k].y;
        double v = dx * dx;
        v = v + dy * dy;
        sq[k] = k < n_all ? v : inf;
        s_min = __builtin_fmin(sq[k], s_min);
    }
    const bool fits = n_all <= SLOTS;
    // distance from the prediction to the outside of the block; a side on the edge of the grid has nothing beyond it
    double bound = inf;
    if (cx - REACH > 0) bound = fmin(bound, px - (x0 + (cx - REACH) * cell));
    if (cx + REACH < GRID_N - 1) bound = fmin(bound, (x0 + (cx + REACH + 1) * cell) - px);
    if (cy - REACH > 0) bound = fmin(bound, py - (y0 + (cy - REACH) * cell));
    if (cy + REACH < GRID_N - 1) bound = fmin(bound, (y0 + (cy + REACH + 1) * cell) - py);
    bound -= 1e-3 * cell;       // (cells were assigned in float arithmetic)
    if (!fits || !(s_min < inf)) return false;
    if (!(bound == inf || (bound > 0.0 && bound * bound > s_min * (1.0 + 1e-9)))) return false;
    const double near_limit = s_min + s_min * 0x1p-48;
    d_min = sqrt(s_min);
    int cand = 0x7FFFFFFF;
    bool inexact = false;
#pragma unroll
    for (int k = 0; k < SLOTS; ++k) {
        const bool near = sq[k] <= near_limit;
        cand = near ? min(cand, col[k]) : cand;
        inexact = inexact || (near && sq[k] != s_min);
    }
    if (inexact) {              // some s differs from min s by a few ulps: compare the rounded roots
        cand = 0x7FFFFFFF;
#pragma unroll
        for (int k = 0; k < SLOTS; ++k)
            if (sq[k] <= near_limit && sqrt(sq[k]) == d_min) cand = min(cand, col[k]);
    }
    arg = cand;
    return true;
}

constexpr int TL_THREADS = 256;
template <typename DetT>
__global__ __launch_bounds__(TL_THREADS) void k_track_lanes(TrackerDev t, BatchDev bd, const BlGains *gains, int head, int frame,
                                                            ysmr_row *rows, long long rows_capacity, const DetT *__restrict__ det,
                                                            const DetT *__restrict__ next_det, const int32_t *next_m_dev,
                                                            DetGrid next_grid)
{
    const int cap = t.capacity, nf = t.n_f;
    const int tid = threadIdx.x, lane = tid & 63;
    const int i = blockIdx.x * TL_THREADS + tid;                       // table row
    const int n_live = *t.n_tracks, claims_by_row = t.n_tracks[4];
    const int m_next = next_det ? det_count(-1, next_m_dev, t.max_det, nullptr) : 0;
    const GridHdr gh = grid_hdr(next_grid);
    // (the row's slot and claim are requested beside the counts that say whether the row is live, not after them: every round of
    // dependent loads is 1-2 us here, the data having been written by k_link on another XCD a moment ago)
    const int i_safe = min(i, cap - 1);
    const int slot = t.order[i_safe];
    const int c_row = t.claim_row[i_safe];
    const bool live = i < n_live;
    double p0 = 0.0, p1 = 0.0;
    bool to_wave = false;
    if (live) {
        const int c = claims_by_row ? c_row : t.claim_slot[slot];
        // (everything the row needs that hangs on the slot alone, requested now: a load issued after the seat's stores would wait for them)
        const int id = t.id[slot], gone = t.gone[slot];
        const long long base = t.row_base[0];
        // the measurement: the detection k_link let this track claim (position and box stored here), or the position it has
        double z0, z1;
        float bw, bh, ba;
        if (c >= 0) {
            const DetT *d = det + (size_t)c * 5;
            z0 = (double)d[0]; z1 = (double)d[1];
            bw = (float)d[2]; bh = (float)d[3]; ba = (float)d[4];
            t.info[slot] = bw; t.info[cap + slot] = bh; t.info[2 * cap + slot] = ba;
        } else {
            z0 = t.pos[slot]; z1 = t.pos[cap + slot];
            bw = t.info[slot]; bh = t.info[cap + slot]; ba = t.info[2 * cap + slot];
        }
        double o0 = z0, o1 = z1;
        p0 = z0; p1 = z1;
        if (t.use_gsff) {
            // (the seat and the ring entries are requested whatever the slot holds -- in the same round of loads as the id that says
            // whether they are this track's; a new track's are blanked afterwards)
            BlSeat S;
            bl_seat_load(S, bd, slot);
            const int hn[BL_NF] = {t.n_i[0], nf > 1 ? t.n_i[1] : 1, nf > 2 ? t.n_i[2] : 1};
            double2 leave[BL_NF];
#pragma unroll
            for (int k = 0; k < BL_NF; ++k) leave[k] = k < nf ? bl_ring_load(bd, (head - hn[k]) & (BL_HB - 1), slot) : make_double2(0.0, 0.0);
            const bool fresh = S.id != id;
            if (fresh) bl_seat_blank(S);
            else if ((frame & (BL_REFRESH - 1)) == 0)          // (on the frame NUMBER, as k_batch: rows must not depend on the batching)
                bl_sums_from_ring(S, bd, slot, head, t.n_i[0], nf > 1 ? t.n_i[1] : 0, nf > 2 ? t.n_i[2] : 0);
            { int unused = 0; bl_gsff<false>(S, t, t, bd, *gains, slot, head, leave, z0, z1, fresh, unused, o0, o1); }
            p0 = S.px; p1 = S.py;
            S.id = id;
            bl_seat_store(S, bd, slot);
        }
        t.pos[slot] = p0; t.pos[cap + slot] = p1;      // CentroidTracker.objects[id]: the prediction (tracker.py:225), or the raw centroid
        {
            t.row_gone[i] = gone;
            if (rows && base + i < rows_capacity) {
                ysmr_row r;
                r.frame = frame;
                r.track_id = id;
                r.x = o0; r.y = o1;
                r.w = bw; r.h = bh; r.angle = ba;
                r.disappeared = gone;
                rows[base + i] = r;
            }
        }
        to_wave = m_next > 0;
    }
    // nearest detection of the NEXT frame (tracker.py:151-163): the 3 x 3 cells around the prediction; for the lanes they do not
    // settle (lost tracks, mostly: nothing near the prediction) the 5 x 5; the whole wave for what is left
    if (next_grid.start) {
        double d_min = 0.0;
        int arg = 0;
        if (to_wave && bl_rowmin_lane<1, 16>(next_grid, gh, p0, p1, m_next, d_min, arg)) { t.row_min[i] = d_min; t.row_arg[i] = arg; to_wave = false; }
#ifndef TL_ONE_PASS
        if (__ballot(to_wave) != 0ull) {
            if (to_wave && bl_rowmin_lane<2, 32>(next_grid, gh, p0, p1, m_next, d_min, arg)) { t.row_min[i] = d_min; t.row_arg[i] = arg; to_wave = false; }
        }
#endif
    }
    // the lanes whose 3 x 3 cells did not settle it, one after the other, by the whole wave (k_track's own search)
    unsigned long long todo = __ballot(to_wave);
#ifdef TL_NOFALLBACK
    todo = 0ull;       // (tuning build: what the lanes alone cost; results are wrong)
#endif
    while (todo) {
        const int l = __builtin_ctzll(todo);
        todo &= todo - 1ull;
        const int row_l = blockIdx.x * TL_THREADS + (tid & ~63) + l;
        const double qx = lane_value(p0, l), qy = lane_value(p1, l);
        if (next_grid.start && rowmin_grid(t, row_l, qx, qy, next_det, next_grid, lane, gh)) continue;
        DetChunk<DetT> first;
        load_chunk(first, next_det, m_next, 0, lane);
        rowmin_wave(t, row_l, qx, qy, next_det, m_next, lane, first);
    }
}

// ---- conversions between the seat-major rest format and the per-slot layout of k_frame / k_link + k_track ----------
// (a: the CURRENT parity view of the per-slot state; table row r takes seat r)
// pos3 / seat3: a 3-D handle's third coordinate by slot, and seat-major f64 [seat_cap] (NULL on a 2-D handle)
__global__ void k_to_batch(TrackerDev a, BatchDev bd, const double *pos3, double *seat3)
{
    const int n = *a.n_tracks, cap = a.capacity, L = a.hist_cap, nf = a.n_f;
    const int head = *bd.head & (BL_HB - 1);
    const size_t sc = (size_t)bd.seat_cap;
    for (int r = blockIdx.x * blockDim.x + threadIdx.x; r < bd.seat_cap; r += gridDim.x * blockDim.x) {
        bd.i32[5 * sc + r] = r < n ? 1 : 0;
        if (r >= n) continue;
        const int slot = a.order[r];
        const double *hist = a.hist + (size_t)slot * 2 * L;
        for (int e = 0; e < L && e < BL_HB - 1; ++e)           // entry e: the measurement of e frames ago
            bd.ring[(size_t)((head - 1 - e) & (BL_HB - 1)) * sc + r] = make_double2(hist[2 * e], hist[2 * e + 1]);
        double *p = bd.f64 + r;
        const double *rec = a.rec + (size_t)slot * a.rec_stride;
        const int mode_r = (int)(__double_as_longlong(rec[1]) & 0xFFFFFFFFll);
        for (int f = 0; f < BL_NF; ++f) {      // (a filter that is not switched on: weight 0, as k_batch keeps it)
            const bool on = f < nf && f < mode_r;
            p[sc * f] = on ? rec[2 + f] : 0.0;
            p[sc * (BL_NF + f)] = on ? rec[2 + nf + f] : 0.0;
            p[sc * (2 * BL_NF + f)] = on ? rec[2 + 2 * nf + f] : 0.0;
        }
        p[sc * (3 * BL_NF)] = a.pos[slot];
        p[sc * (3 * BL_NF + 1)] = a.pos[cap + slot];
        if (seat3) seat3[r] = pos3[slot];
        {   // the window sums, exactly as bl_sums_from_ring forms them
            const int len = (int)(__double_as_longlong(rec[0]) & 0xFFFFFFFFll);
            double s0x = 0.0, s1x = 0.0, s0y = 0.0, s1y = 0.0;
            for (int e = 0; e < BL_HB - 1; ++e) {
                if (e < len && e < L) {
                    s0x = s0x + hist[2 * e];
                    s0y = s0y + hist[2 * e + 1];
                    s1x = __builtin_fma((double)e, hist[2 * e], s1x);
                    s1y = __builtin_fma((double)e, hist[2 * e + 1], s1y);
                }
                for (int f = 0; f < BL_NF; ++f)
                    if (f < nf && e + 1 == min(a.n_i[f], len)) {
                        double *q = p + sc * (3 * BL_NF + 2 + 4 * f);
                        q[0] = s0x; q[sc] = s1x; q[2 * sc] = s0y; q[3 * sc] = s1y;
                    }
            }
        }
        for (int k = 0; k < 3; ++k) bd.f32[sc * k + r] = a.info[k * cap + slot];
        bd.i32[r] = a.id[slot];
        bd.i32[sc + r] = a.gone[a.gone_by_row ? r : slot];
        bd.i32[2 * sc + r] = (int)(__double_as_longlong(rec[0]) & 0xFFFFFFFFll);
        bd.i32[3 * sc + r] = (int)(__double_as_longlong(rec[1]) & 0xFFFFFFFFll);
        bd.i32[4 * sc + r] = r;
    }
}

// (d: the parity-0 view; the track in seat s goes to table row rank[s], which takes slot rank[s]; the free stack hands
// out slot n next)
__global__ void k_to_std(TrackerDev d, BatchDev bd, double *pos3, const double *seat3)
{
    const int n = *d.n_tracks, cap = d.capacity, L = d.hist_cap, nf = d.n_f;
    const int head = *bd.head & (BL_HB - 1);
    const size_t sc = (size_t)bd.seat_cap;
    const int span = cap > bd.seat_cap ? cap : bd.seat_cap;
    for (int s = blockIdx.x * blockDim.x + threadIdx.x; s < span; s += gridDim.x * blockDim.x) {
        if (s < cap - n) d.free_slots[s] = cap - 1 - s;
        if (s == 0) *d.n_free = cap - n;
        if (s >= bd.seat_cap || n == 0 || !bd.i32[5 * sc + s]) continue;
        const int r = bd.i32[4 * sc + s];
        const double *p = bd.f64 + s;
        double *hist = d.hist + (size_t)r * 2 * L;
        for (int e = 0; e < L && e < BL_HB - 1; ++e) {
            const double2 v = bd.ring[(size_t)((head - 1 - e) & (BL_HB - 1)) * sc + s];
            hist[2 * e] = v.x; hist[2 * e + 1] = v.y;
        }
        double *rec = d.rec + (size_t)r * d.rec_stride;
        rec[0] = __longlong_as_double((long long)(unsigned int)bd.i32[2 * sc + s]);
        rec[1] = __longlong_as_double((long long)(unsigned int)bd.i32[3 * sc + s]);
        for (int f = 0; f < nf && f < BL_NF; ++f) {
            rec[2 + f] = p[sc * f];
            rec[2 + nf + f] = p[sc * (BL_NF + f)];
            rec[2 + 2 * nf + f] = p[sc * (2 * BL_NF + f)];
        }
        d.pos[r] = p[sc * (3 * BL_NF)];
        d.pos[cap + r] = p[sc * (3 * BL_NF + 1)];
        if (seat3) pos3[r] = seat3[s];
        for (int k = 0; k < 3; ++k) d.info[k * cap + r] = bd.f32[sc * k + s];
        d.id[r] = bd.i32[s];
        d.order[r] = r;
        d.gone[r] = bd.i32[sc + s];       // (row r = slot r: right for either indexing)
        d.row_gone[r] = bd.i32[sc + s];
    }
}

__global__ void k_peek_batch(TrackerDev t, BatchDev bd, int32_t *ids, double *xy, int32_t *gone, int32_t *n_out)
{
    const size_t sc = (size_t)bd.seat_cap;
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    const int n = *t.n_tracks;
    if (s == 0 && n_out) *n_out = n;
    if (s >= bd.seat_cap || n == 0 || !bd.i32[5 * sc + s]) return;
    const int i = bd.i32[4 * sc + s];
    if (ids) ids[i] = bd.i32[s];
    if (xy) { xy[2 * i] = bd.f64[sc * (3 * BL_NF) + s]; xy[2 * i + 1] = bd.f64[sc * (3 * BL_NF + 1) + s]; }
    if (gone) gone[i] = bd.i32[sc + s];
}

// the third coordinate of every track in id order from the seat-major rest format (ysmr_tracker_peek3, behind k_peek_batch)
__global__ void k_peek_third_batch(TrackerDev t, BatchDev bd, const double *seat3, double *third)
{
    const size_t sc = (size_t)bd.seat_cap;
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= bd.seat_cap || *t.n_tracks == 0 || !bd.i32[5 * sc + s]) return;
    third[bd.i32[4 * sc + s]] = seat3[s];
}

// ==== the batch link of a 3-D handle (ysmr_tracker_dimensions(t, 3), ysmr_tracker_link_mode(t, 2)) ====================
// CentroidTracker.update on (x, y, luminosity) points without a filter bank (the reference raises with one): k_batch without
// the ring, the gains and bl_gsff, and with a third coordinate in the prediction, in the distances and in the stored
// position.  One workgroup, a track per lane, a batch per launch; the frame loop, its one barrier, the claim keys, the
// registration and the rows are k_batch's (the comments above its loop hold here word for word).  Rows carry x and y only.
//
// A frame's block, written by k_bgrid3 (cells in the plane, exactly as k_bgrid bins them):
//   [0, 16)            header as above; [6] = 0 (no candidate lists); [7] = 1 when some |third| of the frame is not below
//                      4096 (or not a number): the float stage's error band does not hold, every lane searches exactly
//   [16, ..)           start (u16), centres (x, y) f32 in cell order, column numbers (u16): as above
//   [.., + MP)         the third coordinate in cell order, ROUNDED to f32 (padding: 0): the float stage's plane
//   -- up to here, rounded up to whole KiB, the block is brought into LDS; at the same offset in every block of a handle
//      (bl3_lds_dwords_max(max_det) dwords from its start) follows, in HBM only:
//   [.., + 2 MP)       the third coordinate in cell order as the f64 the caller gave
// No candidate lists: bl_cell_list drops a detection that is farther IN THE PLANE at every point of the cell, and in three
// dimensions such a detection can still be the nearest.  The search is the 3 x 3 block's, in every frame: the 3-D instances
// of the planar link's bl_block_search and bl_wave_search (BlNear3, bl_dist3 / bl_dist3f and bl3_band stand beside them).
// Why the f64 plane stays in HBM: the two LDS buffers, the three key tables, the id table and the set model take 140 KB at
// max_det = 2048; an f64 plane in both buffers would add 33 KB, the f32 plane adds 16 (157 KB with the static part, of 160).
// A lane's float-stage winner costs one 8-byte load from the tail before its claim key is built; the exact wave search
// reads the tail coalesced, in cell order like the centres.

// One workgroup per frame: bl_bin_frame's 3-D instance.  The cells lie in the plane and the counting sort is the planar
// link's, so a frame's centres come out in the order k_bgrid gives them; a detection's third coordinate follows its centre
// into its cell, rounded to f32 in the LDS part and as given in the tail (which this kernel stores straight to HBM: its
// block image in LDS is the LDS part alone, and the copy-out ends there).
__global__ __launch_bounds__(BG_THREADS) void k_bgrid3(const float *__restrict__ det_all, const double *__restrict__ third_all,
                                                       const int32_t *__restrict__ det_count, int max_det, char *grid, unsigned grid_stride)
{
    bl_bin_frame<true>(det_all, third_all, det_count, max_det, grid, grid_stride);
}

// ---- a 3-D track in registers: the point the reference keeps in objects[id], the box, id, counters -------------------
struct Bl3Seat {
    double px, py, pz;
    float info[3];
    int id, gone, rank;
    bool alive;
};
// rest format: px, py, the box, id, gone, rank and the seat flag where k_batch keeps them in BatchDev (k_peek_batch reads both),
// history length and mode 0, pz in seat3 f64 [seat_cap]

struct BlKernArgs3 {
    TrackerDev t;
    BatchDev bd;                  // grid / grid_stride: the 3-D blocks
    const float *det_all;
    const double *third_all;      // [batch][max_det]: read at a frame's columns below its count only
    const int32_t *det_count;
    int batch, frame0;
    ysmr_row *rows;
    long long rows_capacity;
    long long *row_count;
    double *seat3;                // [seat_cap] the third coordinate at rest
};
typedef const __attribute__((address_space(4))) BlKernArgs3 *BlKernArgs3Ptr;
__device__ __forceinline__ BlKernArgs3Ptr bl_kernargs3()
{
    BlKernArgs3Ptr p = (BlKernArgs3Ptr)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(p));
    return p;
}

__global__ __launch_bounds__(BL_THREADS) void k_batch3(BlKernArgs3 ka)
{
    const TrackerDev &t = ka.t;
    const BatchDev &bd = ka.bd;
    const int32_t *__restrict__ det_count = ka.det_count;
    const int batch = ka.batch;
    long long *row_count = ka.row_count;
    __shared__ BlShared sh;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const unsigned long long below = (1ull << lane) - 1ull;
    int md = t.max_det, mdp = bl_md_padded(md);
    int bufw = bl3_lds_dwords_max(md);
    // LDS by offset, laid out as k_batch's: three key tables, the id table, two grid blocks (their LDS part), the set model
    auto key_at = [&](int k) { return bl_lds + k * mdp; };
    auto cid_at = [&]() { return bl_u32(6 * mdp); };
    auto buf_off = [&](int p) { return 7 * mdp + p * bufw; };
    auto tab_off = [&]() { return 7 * mdp + 2 * bufw; };
    const int seats = min(t.capacity, BL_THREADS);
    const int gone_max = (int)floor(t.max_gone);

    // ---- start of the batch
    int n = *t.n_tracks, next_id = *t.next_id;
    long long base = *row_count;
    for (int f = tid; f < batch; f += BL_THREADS) {
        int m = det_count[f];
        if (m > md) { m = md; atomicOr(t.err, ERR_DET_CLAMPED); }
        sh.cnt[f] = m < 0 ? 0 : m;
    }
    if (tid < 2) { sh.used[tid] = 0; sh.n_dead[tid] = 0; sh.tie[tid] = -1; }
    if (tid == 0) sh.top = 0;
    Bl3Seat S;
    S.px = S.py = S.pz = 0.0;
    S.info[0] = S.info[1] = S.info[2] = 0.f;
    S.id = S.gone = S.rank = 0;
    S.alive = false;
    {
        const size_t sc = (size_t)bd.seat_cap;
        if (n > 0 && tid < seats && bd.i32[5 * sc + tid]) {
            S.px = bd.f64[sc * (3 * BL_NF) + tid]; S.py = bd.f64[sc * (3 * BL_NF + 1) + tid]; S.pz = ka.seat3[tid];
#pragma unroll
            for (int k = 0; k < 3; ++k) S.info[k] = bd.f32[sc * k + tid];
            S.id = bd.i32[tid]; S.gone = bd.i32[sc + tid]; S.rank = bd.i32[4 * sc + tid];
            S.alive = true;
        }
    }
    __syncthreads();
    {
        const unsigned long long ba = __ballot(S.alive);
        if (lane == 0 && ba) atomicMax(&sh.top, 64 * (wave + 1));
    }
    __syncthreads();
    int helpers_from = (sh.top + 63) >> 6;
    auto chore_first = [&]() { return helpers_from < BL_WAVES ? tid - 64 * helpers_from : tid; };
    auto chore_stride = [&]() { return helpers_from < BL_WAVES ? 64 * (BL_WAVES - helpers_from) : BL_THREADS; };
    auto dma = [&](int f) {        // the LDS part of frame f's block -> buffer f & 1, whole 1-KiB pieces
        const int pieces = bl3_lds_dwords(sh.cnt[f]) >> 8;
        const BlKernArgs3Ptr kd = bl_kernargs3();
        const char *src = kd->bd.grid + (size_t)kd->bd.grid_stride * f;
        const int w0 = helpers_from < BL_WAVES ? helpers_from : 0, nw = BL_WAVES - w0;
        for (int c = wave - w0; c >= 0 && c < pieces; c += nw) {
            const uint32_t lds = (uint32_t)(uintptr_t)(bl_u32(buf_off(f & 1) + c * 256));
            const uint32_t off = (uint32_t)c * 1024u + (uint32_t)lane * 16u;
            asm volatile("s_mov_b32 m0, %0\n\tglobal_load_lds_dwordx4 %1, %2" ::"s"(__builtin_amdgcn_readfirstlane(lds)), "v"(off), "s"(src) : "memory");
        }
    };
#pragma nounroll
    for (int k = 0; k < 2 && k < batch; ++k) dma(k);
    for (int c = tid; c < sh.cnt[0]; c += BL_THREADS) key_at(0)[c] = ~0ull;
    if (batch > 1)
        for (int c = tid; c < sh.cnt[1]; c += BL_THREADS) key_at(1)[c] = ~0ull;
    bl_wait_vmem();
    __syncthreads();

    // ---- the frame loop: k_batch's, one barrier A per frame (what orders what: above k_batch's loop)
    int kc = 0;
    int d_cur = 0, d_prev = 0;
    double o0 = 0.0, o1 = 0.0;
    auto settle = [&](int slot, int start, int fr, bool row) {
        const int total = sh.n_dead[slot];
        const int n_dead = total - start;
        if (n_dead && S.alive)
            for (int k = 0; k < n_dead; ++k) S.rank -= sh.dead_id[slot][k] < S.id;
        n -= n_dead;
        if (row) {
            const BlKernArgs3Ptr kr = bl_kernargs3();
            ysmr_row *rows = kr->rows;
            const long long rows_capacity = kr->rows_capacity;
            if (S.alive && base + S.rank < rows_capacity) {
                ysmr_row rr;
                rr.frame = kr->frame0 + fr;
                rr.track_id = S.id;
                rr.x = o0; rr.y = o1;
                rr.w = S.info[0]; rr.h = S.info[1]; rr.angle = S.info[2];
                rr.disappeared = S.gone;
                rows[base + S.rank] = rr;
            }
            if (tid == 0 && base + n > rows_capacity) atomicOr(kr->t.err, ERR_ROWS_CAPACITY);
            base += n;
        }
        return total;
    };
    for (int f = 0; f < batch; ++f) {
        const int par = f & 1;
        const int kn = kc == 2 ? 0 : kc + 1, ks = kc == 0 ? 2 : kc - 1;
        const int m = sh.cnt[f];
        // (the sizes every LDS offset derives from, as values of this frame: left to itself the compiler works out each
        // table's and buffer's address once in front of the loop, holds a scalar register for every one of them through the
        // launch and spills a dozen into vector lanes; worked out again where they are used they cost a scalar add or two)
        asm volatile("" : "+s"(md), "+s"(mdp), "+s"(bufw));
        // ---- each track proposes its nearest detection in (x, y, third)
        const bool propose = S.alive && m > 0;
        const BlGridView gv = bl_grid_view(buf_off(par), m);
        const int z32 = buf_off(par) + bl_list_off(m);
        const bool wide = bl_u32(buf_off(par))[7] != 0u;          // some |third| of the frame >= 4096: no float stage
        // (the blocks' address and stride: read from the argument segment here, they hold no scalar register across the frame)
        const double *z64 = reinterpret_cast<const double *>(bl_kernargs3()->bd.grid + (size_t)bl_kernargs3()->bd.grid_stride * f + 4 * (size_t)bufw);
        const bool narrow = !wide && __builtin_fabs(S.pz) < 4096.0;
        BlNear3 nr{0.0, 0.0, 0.f, 0.f, 0, true};
        unsigned long long key = 0;
        if (propose) {
            if (narrow) nr = bl_block_search<true>(gv, z32, z64, S.px, S.py, S.pz, m);
            else nr.done = false;
        }
        {
            unsigned long long todo = __ballot(propose && !nr.done);
#ifdef YSMR_STAMPS
            if (lane == 0) { if (f == 0) { g_bstamps[wave][13] = 0; g_bstamps[wave][14] = 0; } g_bstamps[wave][13] += __popcll(todo); g_bstamps[wave][14] += todo ? 1 : 0; }
#endif
            while (todo) {
                const int l = __builtin_ctzll(todo);
                todo &= todo - 1ull;
                const bool nw = __builtin_amdgcn_readlane((int)narrow, l) != 0;
                const BlNear3 w = bl_wave_search<true>(gv, z32, z64, lane_value(S.px, l), lane_value(S.py, l), lane_value(S.pz, l), m, lane, nw);
                if (lane == l) nr = w;
            }
        }
        float bx[3] = {0.f, 0.f, 0.f};
        if (propose) {
            const float *d = bl_kernargs3()->det_all + ((size_t)f * md + nr.col) * 5;
            bx[0] = d[2]; bx[1] = d[3]; bx[2] = d[4];
        }
        // ---- claims: k_batch's key (the squared distance without its ten lowest bits | table row) and flag
        if (propose) {
            key = ((unsigned long long)__double_as_longlong(nr.s) & ~0x3FFull) | (unsigned long long)S.rank;
            const unsigned long long before = atomicMin(&key_at(kc)[nr.col], key);
            if ((before >> 10) - (key >> 10) + 1ull <= 2ull) sh.tie[par] = f;
        }
        if (helpers_from >= BL_WAVES || wave >= helpers_from) bl_wait_vmem();
        block_sync<true>();
        // ---- behind barrier A
        if (tid == BL_THREADS - 1) sh.used[par ^ 1] = 0;
        if (f + 2 < batch) dma(f + 2);
        const unsigned long long k_won = key_at(kc)[nr.col];
        const int exact = sh.tie[par] == f;
        const int d_total = settle(par ^ 1, d_prev, f - 1, f > 0);
        bool mine = propose && k_won == key;
        if (exact) {
            for (int c = tid; c < m; c += BL_THREADS) { key_at(kc)[c] = ~0ull; cid_at()[c] = 0xFFFFFFFFu; }
            block_sync<true>();
            if (propose) {
                key = (unsigned long long)__double_as_longlong(nr.s);
                atomicMin(&key_at(kc)[nr.col], key);
            }
            block_sync<true>();
            if (propose) {
                const unsigned long long kmin = key_at(kc)[nr.col];
                bool tie = key == kmin;
                if (!tie) {
                    const double smin = __longlong_as_double((long long)kmin);
                    if (nr.s <= smin + smin * 0x1p-48) tie = sqrt(nr.s) == sqrt(smin);
                }
                if (tie) atomicMin(&cid_at()[nr.col], (uint32_t)S.id);
            }
            block_sync<true>();
            mine = propose && cid_at()[nr.col] == (uint32_t)S.id;
        }
        // ---- ageing and deregistration
        const bool age = (m == 0) || (n > 0 && n >= m);
        double z0 = S.px, z1 = S.py, z2 = S.pz;
        bool died = false;
        if (mine) {
            z0 = (double)nr.zx; z1 = (double)nr.zy; z2 = nr.z;
            S.gone = 0;
        } else if (S.alive && age) {
            ++S.gone;
            S.info[0] = S.info[1] = S.info[2] = 0.f;
            if (S.gone > gone_max) { S.alive = false; died = true; }
        }
        {
            const unsigned long long bm = __ballot(mine), bxd = __ballot(died);
            if (lane == 0 && bm) atomicAdd(&sh.used[par], (int)__popcll(bm));
            if (bxd) {
                int at = 0;
                if (lane == 0) at = atomicAdd(&sh.n_dead[par], (int)__popcll(bxd));
                at = __builtin_amdgcn_readfirstlane(at) - d_cur;
                if (died) sh.dead_id[par][at + __popcll(bxd & below)] = S.id;
            }
        }
        // ---- registration: unclaimed columns become tracks, in CPython set order
        const bool births = m > 0 && (n == 0 || n < m);
        if (births) {
            int tl = tid, wv = wave, ln = lane, mp = mdp;
            asm volatile("" : "+v"(tl), "+s"(wv), "+v"(ln));
            int *unused = reinterpret_cast<int *>(key_at(ks)), *newcols = unused + mp;
            uint32_t *list = cid_at();
            __syncthreads();
            int n_new = 0, n_new_all = 0;
            if (n == 0) {
                for (int c = tl; c < m; c += BL_THREADS) newcols[c] = c;
                n_new_all = m;
            } else {
                const int K = (m + BL_THREADS - 1) / BL_THREADS;
                const int c0 = tl * K, c1 = min(c0 + K, m);
                int cnt = 0;
                for (int c = c0; c < c1; ++c) cnt += key_at(kc)[c] == ~0ull;
                int incl = cnt;
#pragma unroll
                for (int d = 1; d < 64; d <<= 1) { const int o = __shfl_up(incl, d); if (ln >= d) incl += o; }
                if (ln == 63) sh.wave_cnt[0][wv] = incl;
                __syncthreads();
                int at = incl - cnt, total = 0;
#pragma unroll
                for (int k = 0; k < BL_WAVES; ++k) { const int v = sh.wave_cnt[0][k]; at += k < wv ? v : 0; total += v; }
                for (int c = c0; c < c1; ++c)
                    if (key_at(kc)[c] == ~0ull) unused[at++] = c;
                __syncthreads();
                int cnt_set = cpython_order_lds<BL_THREADS, BL_TABLE>(unused, total, m, sh.used[par], newcols, bl_u32(tab_off()), list, sh.set_state);
                if (cnt_set < 0) { if (tl == 0) atomicOr(bl_kernargs3()->t.err, ERR_TRACK_CAPACITY); cnt_set = 0; }
                n_new_all = cnt_set;
            }
            n_new = n_new_all;
            const int seats = min(bl_kernargs3()->t.capacity, BL_THREADS);
            if (n + n_new > seats) {
                if (tl == 0) atomicOr(bl_kernargs3()->t.err, ERR_TRACK_CAPACITY);
                n_new = seats - n;
            }
            const bool free_lane = !S.alive && tl < seats;
            const unsigned long long bf = __ballot(free_lane);
            if (ln == 0) sh.wave_cnt[1][wv] = (int)__popcll(bf);
            __syncthreads();
            int fr = (int)__popcll(bf & below);
#pragma unroll
            for (int k = 0; k < BL_WAVES; ++k) fr += k < wv ? sh.wave_cnt[1][k] : 0;
            if (free_lane && fr < n_new) {
                const int c = newcols[fr];
                const BlKernArgs3Ptr kb = bl_kernargs3();
                const float *d = kb->det_all + ((size_t)f * md + c) * 5;
                z0 = (double)d[0]; z1 = (double)d[1];
                z2 = kb->third_all[(size_t)f * md + c];        // (c < m: a slot at or beyond the count is never read)
                S.info[0] = d[2]; S.info[1] = d[3]; S.info[2] = d[4];
                S.id = next_id + fr; S.rank = n + fr; S.gone = 0;
                S.alive = true;
                atomicMax(&sh.top, tl + 1);
            }
            n += n_new;
            next_id += n_new_all;
            bl_wait_vmem();
            __syncthreads();
            helpers_from = (sh.top + 63) >> 6;
        }
        {
            const int m_ahead = f + 2 < batch ? sh.cnt[f + 2] : 0;
            for (int c = chore_first(); c >= 0 && c < m_ahead; c += chore_stride()) key_at(ks)[c] = ~0ull;
        }
        // ---- the point the track keeps (tracker.py:181, 228-230: the claimed detection, or where it was)
        bl_wait_vmem();
        if (mine) { S.info[0] = bx[0]; S.info[1] = bx[1]; S.info[2] = bx[2]; }
        o0 = z0; o1 = z1;
        if (S.alive) { S.px = z0; S.py = z1; S.pz = z2; }
        d_prev = d_cur; d_cur = d_total;
        kc = kn;
    }
    block_sync<true>();
    settle((batch - 1) & 1, d_prev, batch - 1, true);
    // ---- end of the batch: the state goes back to HBM, seat by seat
    {
        const BlKernArgs3Ptr ke = bl_kernargs3();
        const size_t sc = (size_t)ke->bd.seat_cap;
        double *f64 = ke->bd.f64;
        float *f32 = ke->bd.f32;
        int *i32 = ke->bd.i32;
        if (tid < min(ke->t.capacity, BL_THREADS)) {      // (from the argument segment: no lane mask kept since the first frame)
            i32[5 * sc + tid] = S.alive ? 1 : 0;
            if (S.alive) {
                f64[sc * (3 * BL_NF) + tid] = S.px; f64[sc * (3 * BL_NF + 1) + tid] = S.py; ke->seat3[tid] = S.pz;
#pragma unroll
                for (int k = 0; k < 3; ++k) f32[sc * k + tid] = S.info[k];
                i32[tid] = S.id; i32[sc + tid] = S.gone; i32[2 * sc + tid] = 0; i32[3 * sc + tid] = 0; i32[4 * sc + tid] = S.rank;
            }
        }
        if (tid == 0) { *ke->t.n_tracks = n; *ke->t.next_id = next_id; *ke->row_count = base; }
    }
}

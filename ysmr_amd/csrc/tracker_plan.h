// tracker_plan.h -- the host-only part of the tracker (track.hip, batch_link.h): the constants its kernels are built with, the
// layout and size of a frame's grid block and of the kernels' LDS, the configuration derived from ysmr_tracker_create's
// arguments, the carving of the state block, and which of the five link paths a handle runs.  Plain C++17 with no HIP in it:
// tests/tracker_plan_check.cc compiles it alone, under the host sanitizers.  What only the device can answer -- a refused
// LDS size, a failed allocation -- stays in track.hip and only clears a capability (Caps) there.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "hd.h"

#ifndef __HIPCC__
struct alignas(16) double2 { double x, y; };     // HIP's vector type where there is no HIP: BatchDev names it
#endif

#define YSMR_MAX_FILTERS 8

struct TrackerDev {
    // what the link kernels' first round of loads is addressed with, together at the head of the structure: one scalar
    // load of the kernel's arguments fetches them all
    int *n_tracks, *next_id, *err, *n_free;
    int *order, *gone;
    int *row_arg;                 // [cap]
    double *row_min;              // [cap]
    long long *row_base;          // first output row of the current frame (k_link -> k_gsff)
    int capacity, max_det, n_f, use_gsff, hist_cap, table_cap, gain_total, gone_by_row;
    int gains_decoupled;             // x-hat reads only x columns, y-hat only y columns (every closed-form gain)
    double max_gone, lik_min;
    int n_i[YSMR_MAX_FILTERS];
    int gain_off[YSMR_MAX_FILTERS];  // filter i: row0 at gains[gain_off[i]], row1 at +2*n_i[i]
    const double *gains;
    // persistent state
    int *free_slots;
    int *id;
    double *pos;      // [2][cap]
    float *info;      // [3][cap]
    double *hist;     // [cap][hist_cap][2]  (one contiguous ring per track slot)
    // the filter bank's scalars of a slot as ONE record of rec_stride doubles: [0] history length | head << 32,
    // [1] mode, [2 + f] weight, [2 + n_f + f] / [2 + 2 n_f + f] x-hat of filter f (the likelihoods are recomputed in
    // every step and not kept).  A wave fetches and stores it with one instruction, lane = field: 15 VGPRs fewer than
    // separately addressed scalars in k_frame and 10 in k_track (more of its 5000 waves resident at 4K: +2.5 %)
    double *rec;      // [cap][rec_stride]
    int rec_stride;
    // per-frame scratch
    int *unused;                  // [max_det] unclaimed detection columns, ascending
    int *row_gone;                // [cap] split path: `gone` of the track in a row, written with the row minimum (k_link then
                                  // has everything a row's claim and ageing need from ONE round of loads by row)
    int *dead;                    // [cap]
    int *new_cols;                // [max_det]
    int *set_table;               // [2][table_cap] CPython set model
    // split path (tables too large for LDS): k_link's per-column winners and per-row claims
    unsigned long long *link_key; // [max_det]
    int *link_row;                // [max_det]
    int *link_claim;              // [capacity]
    // split path: the detection column the track in a slot claimed in the current frame (-1: none).  k_link only decides;
    // the winner's detection is fetched, and position / box are stored, by the track's own wave in k_track (5000 waves
    // instead of one workgroup's two rounds of dependent gathers: 5 us of k_link's 12.6 at 4K)
    int *claim_slot;              // [capacity]
    // ... and by ROW of the table k_track sees (after compaction and registration), valid when n_tracks[4] != 0 (k_link's
    // register-resident path, the 4K configuration): the wave then knows its detection one round of loads earlier -- with
    // its slot instead of after it
    int *claim_row;               // [capacity]
};

// ---- the batch link (batch_link.h): one workgroup links a whole batch of frames per launch, a track per lane
#ifndef YSMR_BL_THREADS
#define YSMR_BL_THREADS 768
#endif
constexpr int BL_THREADS = YSMR_BL_THREADS;      // seats: one track per lane
constexpr int BL_WAVES = BL_THREADS / 64;
constexpr int BL_HB = 32;             // ring of measurements per seat (hist_cap <= 32; a power of two)
constexpr int BL_NF = 3;              // filters (n_f <= 3)
#ifndef YSMR_BL_MAX_BATCH
#define YSMR_BL_MAX_BATCH 256
#endif
constexpr int BL_MAX_BATCH = YSMR_BL_MAX_BATCH;      // frames per launch (the grid block is sized for it; longer batches are cut).
                                                    // 256 since the end of round 4: a launch's fixed costs (state in and out, the gap to the next
                                                    // launch) and the detection kernels' per-item costs are paid per BATCH (bench.py: 161.5 k frames/s
                                                    // at 64 frames per batch, 163.5 k at 128, 165 k at 256)
constexpr int BL_TABLE = 4096;        // CPython set model table, 32-bit slots (as FRAME_TABLE)
constexpr int BL_SF64 = 3 * BL_NF + 2 + 4 * BL_NF;   // w, xa, xb, px, py, the window sums
constexpr int BL_REFRESH = 64;        // frames between two exact recomputations of the window sums (a power of two)

struct BatchDev {
    double2 *ring;      // [BL_HB + 1][seat_cap]  the measurements of the last BL_HB frames, seat by seat; position BL_HB is
                        // a line of zeros, cleared when the handle is made and never stored to (k_batch: what leaves a window
                        // that is not full)
    double *f64;        // [BL_SF64][seat_cap]
    float *f32;         // [3][seat_cap]      box of the last claimed detection (0 while lost)
    int *i32;           // [6][seat_cap]      id, gone, history length, mode, table row, seat taken
    int *head;          // ring position of the next frame's measurements
    char *grid;         // [BL_MAX_BATCH][grid_stride] bytes, written by k_bgrid
    unsigned grid_stride;   // bytes per frame (a multiple of 1024)
    int seat_cap;
};

struct BlGains { double alpha[BL_NF][2], beta[BL_NF][2]; };    // [filter][x / y row]; batch_link.h: bl_fir
// Uniform grid over one frame's detections (split path): the nearest detection of a track is looked for in the
// cells around it instead of among all of them (25 M distances per frame at 5000 x 5000).
constexpr int GRID_N = 128;                         // cells per side
constexpr int GRID_CELLS = GRID_N * GRID_N;
// bytes of a frame's DetGrid arrays (track.hip): cell starts, detection columns, header, centres
YSMR_HD inline size_t grid_bytes_per_frame(int max_det)
{
    return (sizeof(int) * (GRID_CELLS + 64) + sizeof(int) * (size_t)max_det + 64 + 2 * sizeof(float) * (size_t)max_det + 255) / 256 * 256;
}

constexpr int FRAME_THREADS = 256;
constexpr int FRAME_TABLE = 4096;   // CPython set model table (entries) in LDS: up to FUSED_MAX_DET + 1 unused columns
// LDS of k_frame (track.hip: FrameLds)
YSMR_HD inline size_t frame_lds_bytes(int cap, int max_det, int gain_total)
{
    return 8 * ((size_t)gain_total + max_det) + 4 * ((size_t)max_det + 2 * (size_t)cap + 16) + 2 * 2 * FRAME_TABLE + 64;
}

// ---- the limits of the link paths, each named once ----------------------------------------------------------------
constexpr int TRACKER_MAX_SIZE = 65536;             // capacity and max_det: 32-bit indices, a sane state block
constexpr int FUSED_MAX_DET = 2456;                 // k_frame / k_batch: what the LDS set model holds of unregistered columns
constexpr size_t FRAME_LDS_LIMIT = 150 * 1024;      // k_frame's LDS
constexpr double FUSED_MAX_GONE = 32000.0;          // k_frame packs a `gone` counter into 15 bits: max_disappeared below this
constexpr size_t LINK_LDS_LIMIT = 140 * 1024;       // k_link's per-column winner tables (12 B per detection column) in LDS
constexpr size_t BL_LDS_LIMIT = 160 * 1024;         // a compute unit's LDS: k_batch, k_batch3

// ---- a frame's detections as the batch link wants them: one block of dwords per frame ------------------------------
//   [0, 16)            header: x0, y0, cell, 1 / cell (f32), cells per side G, m, candidates per cell (0: no lists) (i32)
//   [16, 16 + SW)      start[G * G + 1] as u16: first item of each cell (row-major), the last entry = m
//   [.., + 2 * MP)     centres (x, y) f32 of the detections in cell order;  MP = m + 1 rounded up to 8 (entry m and the
//                      rest: 1e30, far from everything -- the sentinel the candidate lists are padded with)
//   [.., + MP / 2)     their column numbers as u16
//   [.., + 4 G G)      G <= 32 only: per cell BL_LIST u16 positions in the cell-ordered centres -- every detection that can
//                      be nearest to, or within the float tie band of the nearest to, a point of the cell (k_bgrid),
//                      ascending, padded with m; 0xFFFF first: more than BL_LIST, the cell's lanes search the 3 x 3 block;
//                      BL_SPLIT first: the cell's four quadrants have lists of their own, in overflow entry <second u16>
//                      (of a slot that starts with 0xFFFF or BL_SPLIT the rest is unspecified: what the first pass left)
//   [.., + 16 BL_OVF)  G <= 32 only, the overflow area: BL_OVF entries of 4 x BL_LIST u16 -- the lists of the quadrants
//                      (x half + 2 * y half) of a cell whose own list came out too long, built like a cell's list on the
//                      quadrant's rectangle.  Entries go to the crowded cells in cell order; a cell beyond the BL_OVF-th,
//                      or one with a quadrant that still overflows, keeps 0xFFFF.  Unused entries are zero.
// (cells per side so that a cell holds ~0.45 detections: the three cells of a row of the 3 x 3 block around a prediction
// then hold more than five candidates once in 200 rows, and the block reaches one cell -- ~1.7 mean nearest-neighbour
// distances -- beyond the prediction's own cell)
constexpr int BL_LIST = 8;        // candidates per cell: one ds_read_b128 per lane
constexpr int BL_OVF = 8;         // overflow entries per frame (512 bytes; DESIGN.md section 4, round 16, has the distribution:
                                  // the bench clip's frames hold 0 .. 5 crowded cells, and a frame of ~530 detections still
                                  // takes 24 LDS-DMA pieces with them)
YSMR_HD inline int bl_grid_n(int m) { return m <= 128 ? 16 : (m <= 600 ? 32 : (m <= 1300 ? 48 : 64)); }
// (the lists of 48 x 48 cells would take 36 KB per block: two of them beside the tables of max_det = 2048 do not fit a
// compute unit's 160 KB; those frames keep the 3 x 3 search)
YSMR_HD inline bool bl_has_lists(int m) { return bl_grid_n(m) <= 32; }
YSMR_HD inline int bl_start_dwords(int G) { return ((G * G + 2) / 2 + 3) / 4 * 4; }
YSMR_HD inline int bl_pad8(int m) { return (m + 7) / 8 * 8; }
YSMR_HD inline int bl_mp(int m) { return bl_pad8(m + 1); }
YSMR_HD inline int bl_list_off(int m)      // dword offset of the lists in the block (a multiple of 4)
{
    return 16 + bl_start_dwords(bl_grid_n(m)) + 2 * bl_mp(m) + bl_mp(m) / 2;
}
YSMR_HD inline int bl_ovf_off(int m)       // dword offset of the overflow area (frames with lists)
{
    return bl_list_off(m) + bl_grid_n(m) * bl_grid_n(m) * BL_LIST / 2;
}
YSMR_HD inline int bl_grid_dwords(int m)   // rounded up to whole 1-KiB pieces (one LDS-DMA wave-instruction)
{
    const int raw = bl_has_lists(m) ? bl_ovf_off(m) + BL_OVF * 4 * BL_LIST / 2 : bl_list_off(m);
    return (raw + 255) / 256 * 256;
}
YSMR_HD inline int bl_grid_dwords_max(int max_det)
{
    int most = bl_grid_dwords(max_det);
    const int steps[4] = {128, 600, 1300, max_det};      // (the size is monotone in m between two changes of the grid)
    for (int k = 0; k < 4; ++k)
        if (steps[k] <= max_det && bl_grid_dwords(steps[k]) > most) most = bl_grid_dwords(steps[k]);
    return most;
}

struct BlShared {      // static part of k_batch's and k_batch3's LDS
    int cnt[BL_MAX_BATCH];           // detections per frame (clamped)
    int used[2];                     // per frame parity: claims made
    int n_dead[2];                   // per frame parity: tracks deregistered, as a RUNNING count over the launch (k_batch)
    int tie[2];                      // per frame parity: the last frame in which some column's proposals were too close
                                     // for the short key (a frame NUMBER: never reset)
    int dead_id[2][BL_THREADS];      // ids of the tracks deregistered in the frame
    int wave_cnt[2][BL_WAVES];       // registration: per-wave counts of the two ranked lists
    int set_state[2];
    int top;                         // one past the highest seat ever taken
    long long rows_then;             // k_batch: the row count at the start of the launch plus the room it found (thread 0's,
                                     // for the end of the launch; in the padding of the 16-byte rounding: bl_lds_total is what it was)
};

YSMR_HD inline int bl_md_padded(int max_det) { return (max_det + 3) / 4 * 4; }
// dynamic part: three key tables (u64 per column), one table of winning ids (u32), two grid blocks, the set model's table
YSMR_HD inline size_t bl_lds_bytes(int max_det)
{
    return 2 * 4 * (size_t)bl_grid_dwords_max(max_det) + (3 * 8 + 4) * (size_t)bl_md_padded(max_det) + 4 * BL_TABLE + 64;
}
// all of it: what one workgroup of k_batch takes of a compute unit's 160 KiB (the static part is BlShared and nothing else)
YSMR_HD inline size_t bl_lds_total(int max_det) { return bl_lds_bytes(max_det) + (sizeof(BlShared) + 15) / 16 * 16; }

// the 3-D batch link's block (batch_link.h, above k_bgrid3, has its layout): the part brought into LDS, per frame and at most
YSMR_HD inline int bl3_lds_dwords(int m) { return (bl_list_off(m) + bl_mp(m) + 255) / 256 * 256; }
// (without candidate lists the size only grows with m -- bl_grid_n and bl_mp do -- so the largest block is max_det's)
YSMR_HD inline int bl3_lds_dwords_max(int max_det) { return bl3_lds_dwords(max_det); }
YSMR_HD inline size_t bl3_grid_stride(int max_det)      // bytes per frame: the LDS part and the f64 tail, whole KiB
{
    return 4 * (size_t)bl3_lds_dwords_max(max_det) + (8 * (size_t)bl_mp(max_det) + 1023) / 1024 * 1024;
}
YSMR_HD inline size_t bl3_lds_bytes(int max_det)
{
    return 2 * 4 * (size_t)bl3_lds_dwords_max(max_det) + (3 * 8 + 4) * (size_t)bl_md_padded(max_det) + 4 * BL_TABLE + 64;
}
YSMR_HD inline size_t bl3_lds_total(int max_det) { return bl3_lds_bytes(max_det) + (sizeof(BlShared) + 15) / 16 * 16; }

namespace tracker_plan {

// ---- what can be wrong with ysmr_tracker_create's arguments: a status and the arguments of its message (track.hip: plan_fail)
enum class Bad { none, size, filters, fps, horizons, horizon_max };
struct Status {
    Bad what = Bad::none;
    int a = 0, b = 0, c = 0;
    double x = 0.0;
    explicit operator bool() const { return what != Bad::none; }
};

// generate_n_i (gsff.py:87-109); CentroidTracker passes n_max = fps when it is None (tracker.py:58-59)
inline Status horizons(double fps, int n_min, double n_max, int n_f, int *n_i)
{
    if (n_f < 1 || n_f > YSMR_MAX_FILTERS) return Status{Bad::filters, YSMR_MAX_FILTERS, n_f};
    if (!(fps > 0)) return Status{Bad::fps};
    double top = n_max > 0 ? n_max : fps;
    double p = (top - n_min) / n_f;
    for (int i = 1; i <= n_f; ++i) n_i[i - 1] = (int)(n_min + p * i);
    for (int i = 0; i < n_f; ++i)
        if (n_i[i] < 1 || (i && n_i[i] <= n_i[i - 1])) return Status{Bad::horizons, n_min, n_f, 0, top};
    return Status{};
}

inline void closed_form_gain(int N, double *g)
{
    // rows 0/1 of (L^T L)^-1 L^T for the constant-velocity model: the one-step-ahead
    // least-squares line fit, c_j = 1/N + t_j * ((N+1)/2) / sum(t^2), t_j = j - (N-1)/2
    double st2 = 0.0;
    for (int j = 0; j < N; ++j) { double tj = j - (N - 1) / 2.0; st2 += tj * tj; }
    std::memset(g, 0, sizeof(double) * 4 * N);
    for (int j = 0; j < N; ++j) {
        double tj = j - (N - 1) / 2.0;
        double c = 1.0 / N + (st2 > 0 ? tj * ((N + 1) / 2.0) / st2 : 0.0);
        g[2 * j] = c;              // row 0, x columns
        g[2 * N + 2 * j + 1] = c;  // row 1, y columns
    }
}

// ---- the configuration of a handle, derived from ysmr_tracker_create's arguments --------------------------------------
struct Config {
    int capacity, max_det, use_gsff;
    double max_gone;
    int n_f, n_i[YSMR_MAX_FILTERS], gain_off[YSMR_MAX_FILTERS], gain_total;
    int hist_cap, table_cap, rec_stride;
    int gains_decoupled;       // row 0 vanishes on the y columns, row 1 on the x columns
    bool gains_affine;         // ... and every row is affine in a measurement's age: `bgains` states it (batch_link.h: bl_fir)
    BlGains bgains;
};

// `gains`: the caller's, laid out as ysmr_gsff_gains writes them, or NULL for the closed form; `gains_out` gets the handle's
inline Status configure(double max_disappeared, double fps, int n_min, double n_max, int n_f, int use_gsff, int capacity,
                        int max_det, const double *gains, Config &c, std::vector<double> &gains_out)
{
    // (the tables of the two-launch path live in HBM; the bound only keeps 32-bit indices and the state block sane)
    if (capacity <= 0 || max_det <= 0 || capacity > TRACKER_MAX_SIZE || max_det > TRACKER_MAX_SIZE)
        return Status{Bad::size, capacity, max_det};
    c = Config{};
    c.capacity = capacity;
    c.max_det = max_det;
    c.use_gsff = use_gsff ? 1 : 0;
    c.max_gone = max_disappeared;
    c.n_f = use_gsff ? n_f : 1;
    size_t gain_doubles = 0;
    gains_out.clear();
    if (use_gsff) {
        if (Status s = horizons(fps, n_min, n_max, n_f, c.n_i)) return s;
        for (int i = 0; i < n_f; ++i) { c.gain_off[i] = (int)gain_doubles; gain_doubles += 4 * (size_t)c.n_i[i]; }
        gains_out.resize(gain_doubles);
        if (gains) std::memcpy(gains_out.data(), gains, sizeof(double) * gain_doubles);
        else for (int i = 0; i < n_f; ++i) closed_form_gain(c.n_i[i], gains_out.data() + c.gain_off[i]);
        c.gains_decoupled = 1;   // row 0 must vanish on the y columns, row 1 on the x columns
        for (int i = 0; i < n_f && c.gains_decoupled; ++i) {
            const double *g = gains_out.data() + c.gain_off[i];
            for (int j = 0; j < c.n_i[i]; ++j)
                if (g[2 * j + 1] != 0.0 || g[2 * c.n_i[i] + 2 * j] != 0.0) { c.gains_decoupled = 0; break; }
        }
        c.hist_cap = c.n_i[n_f - 1] + 1;
        if (c.hist_cap > 64) return Status{Bad::horizon_max, c.n_i[n_f - 1]};
    } else {
        c.n_i[0] = 1;
        c.hist_cap = 1;
    }
    unsigned tc = 8;
    while (tc <= (unsigned)max_det * 4u) tc <<= 1;
    c.table_cap = (int)tc;
    c.gain_total = (int)gain_doubles;
    c.rec_stride = (2 + 3 * c.n_f + 7) / 8 * 8;
    // the gains as the batch kernel takes them: affine in the age of a measurement (batch_link.h: bl_fir); its bank holds BL_NF filters
    c.gains_affine = c.n_f <= BL_NF;
    if (use_gsff && c.gains_affine) {
        for (int f = 0; f < c.n_f; ++f) {
            const int N = c.n_i[f];
            const double *g = gains_out.data() + c.gain_off[f];
            for (int r = 0; r < 2; ++r) {
                auto gain = [&](int a) { return r ? g[2 * N + 2 * (N - 1 - a) + 1] : g[2 * (N - 1 - a)]; };   // age a, row r
                const double alpha = gain(0), beta = N > 1 ? gain(0) - gain(1) : 0.0;
                for (int a = 0; a < N; ++a)
                    if (std::fabs(gain(a) - (alpha - beta * a)) > 1e-14 * std::fabs(alpha)) c.gains_affine = false;
                c.bgains.alpha[f][r] = alpha;
                c.bgains.beta[f][r] = beta;
            }
        }
    }
    return Status{};
}

// ---- the state block: ONE device allocation, carved in steps of 256 bytes -------------------------------------------
// Run on a null base the function gives the size alone (every pointer null), as ysmr::table::Arena does for the table stages.
struct Arena {
    char *base;
    size_t at = 0;
    template <class T> T *take(size_t count)
    {
        T *p = base ? reinterpret_cast<T *>(base + at) : nullptr;
        at = (at + count * sizeof(T) + 255) / 256 * 256;
        return p;
    }
};

// The views of both frame parities (k_frame double-buffers the small per-frame arrays: `d1` shares everything else with
// `d0`), the batch link's seat-major rest format and a 3-D handle's third coordinate.  Returns the bytes.
inline size_t carve_state(void *base, const Config &c, TrackerDev &d0, TrackerDev &d1, BatchDev &bd, double *&pos3)
{
    Arena a{static_cast<char *>(base)};
    const size_t cap = c.capacity, md = c.max_det;
    std::memset(&d0, 0, sizeof(d0));
    d0.capacity = c.capacity; d0.max_det = c.max_det; d0.n_f = c.n_f; d0.use_gsff = c.use_gsff;
    d0.hist_cap = c.hist_cap; d0.table_cap = c.table_cap; d0.gain_total = c.gain_total; d0.rec_stride = c.rec_stride;
    d0.gains_decoupled = c.gains_decoupled;
    d0.max_gone = c.max_gone;
    d0.lik_min = 1e-20;  // tracker.py:67
    std::memcpy(d0.n_i, c.n_i, sizeof(d0.n_i));
    std::memcpy(d0.gain_off, c.gain_off, sizeof(d0.gain_off));
    // sixteen words of scalars per parity: live tracks, next id, error bits (parity 0's only: sticky), free slots; [8] the
    // first output row; parity 0's [12 .. 15]: the ring's head and the three words behind it (k_batch)
    auto word = [](int *s, int k) { return s ? s + k : nullptr; };
    auto scalars = [&](TrackerDev &q) {
        int *s = a.take<int>(16);
        q.n_tracks = s; q.next_id = word(s, 1); q.n_free = word(s, 3);
        q.row_base = reinterpret_cast<long long *>(word(s, 8));
        return s;
    };
    int *scal = scalars(d0);
    d0.err = word(scal, 2);
    bd.head = word(scal, 12);
    d0.order = a.take<int>(cap); d0.free_slots = a.take<int>(cap);
    d0.id = a.take<int>(cap); d0.gone = a.take<int>(cap);
    d0.pos = a.take<double>(2 * cap); d0.info = a.take<float>(3 * cap);
    pos3 = a.take<double>(cap);      // (a 3-D handle's third coordinate: ysmr_tracker_dimensions)
    d0.hist = a.take<double>(2 * cap * c.hist_cap);
    d0.rec = a.take<double>((size_t)c.rec_stride * cap);
    d0.gains = a.take<double>(c.gain_total ? c.gain_total : 1);
    d0.unused = a.take<int>(md);
    d0.row_min = a.take<double>(cap); d0.row_arg = a.take<int>(cap); d0.row_gone = a.take<int>(cap);
    d0.dead = a.take<int>(cap);
    d0.new_cols = a.take<int>(md); d0.set_table = a.take<int>(2 * (size_t)c.table_cap);
    d0.link_key = a.take<unsigned long long>(md); d0.link_row = a.take<int>(md);
    d0.link_claim = a.take<int>(cap); d0.claim_slot = a.take<int>(cap); d0.claim_row = a.take<int>(cap);
    // parity-1 copies of the arrays k_frame double-buffers
    d1 = d0;
    scalars(d1);
    d1.order = a.take<int>(cap); d1.gone = a.take<int>(cap);
    d1.row_min = a.take<double>(cap); d1.row_arg = a.take<int>(cap);
    // the batch link's rest format (seat-major)
    const size_t seat_cap = c.capacity > BL_THREADS ? cap : (size_t)BL_THREADS;     // (k_batch: 768 seats; k_track_lanes: a seat per slot)
    // (BL_HB positions and the line of zeros behind them: cleared with the block; every store indexes 0 .. BL_HB - 1)
    bd.ring = a.take<double2>((BL_HB + 1) * seat_cap);
    bd.f64 = a.take<double>(BL_SF64 * seat_cap); bd.f32 = a.take<float>(3 * seat_cap);
    bd.i32 = a.take<int>(6 * seat_cap);
    bd.seat_cap = (int)seat_cap;
    bd.grid = nullptr; bd.grid_stride = 0;
    return a.at;
}

// ---- the link path --------------------------------------------------------------------------------------------------
// The five ways a `run` call is linked.  link_of below is the only place that says which one a handle takes.
enum class Link {
    frame,      // one launch per frame: k_frame
    waves,      // two launches per frame, a wave per track: k_link + k_track
    lanes,      // two launches per frame, a track per lane: k_link + k_track_lanes
    batch,      // one launch per batch: k_batch
    batch3,     // the same in three dimensions: k_batch3
};

// What a configuration qualifies for, and the LDS each kernel would take.
struct Caps {
    bool frame;       // k_frame's LDS fits, the LDS set model holds max_det columns, `gone` fits its 15 bits
    bool lanes;       // the filter bank is one the lane kernels run: up to BL_NF filters of at most BL_HB - 1 frames, gains
                      // that are decoupled and affine in a measurement's age (k_track_lanes: 2-D tables beyond k_frame)
    bool batch;       // ... and k_frame's conditions, at most BL_THREADS tracks, k_batch's LDS within a compute unit's
    bool batch3;      // 3-D: k_frame's conditions, no filter bank, at most BL_THREADS tracks, k_batch3's LDS within a unit's
    bool link_lds;    // k_link keeps its per-column winner tables in LDS (else in HBM)
    size_t frame_lds, batch_lds, batch3_lds, link_lds_bytes;     // dynamic LDS of k_frame, k_batch, k_batch3, k_link (tables in LDS)
};

inline Caps qualifies(const Config &c)
{
    Caps q{};
    q.frame_lds = frame_lds_bytes(c.capacity, c.max_det, c.gain_total);
    q.batch_lds = bl_lds_bytes(c.max_det);
    q.batch3_lds = bl3_lds_bytes(c.max_det);
    q.link_lds_bytes = 12 * (size_t)c.max_det;
    q.frame = q.frame_lds <= FRAME_LDS_LIMIT && c.max_det <= FUSED_MAX_DET && c.max_gone < FUSED_MAX_GONE;
    q.lanes = c.n_f <= BL_NF && c.hist_cap <= BL_HB && (!c.use_gsff || (c.gains_decoupled && c.gains_affine));
    q.batch = q.frame && q.lanes && c.capacity <= BL_THREADS && bl_lds_total(c.max_det) <= BL_LDS_LIMIT;
    q.batch3 = q.frame && !c.use_gsff && c.capacity <= BL_THREADS && bl3_lds_total(c.max_det) <= BL_LDS_LIMIT;
    q.link_lds = q.link_lds_bytes <= LINK_LDS_LIMIT;
    return q;
}

// link_mode (ysmr_tracker_link_mode): 0 = the library's choice, 1 = one (or two) launches per frame, 2 = as 0, and a 3-D
// handle that can also links a batch with one launch.  A 3-D handle has no grid search and no lane kernel; the batch
// paths need what k_frame needs (a capability the device clears takes them along).
inline Link link_of(const Caps &q, int dims, int link_mode)
{
    if (dims == 3) {
        if (q.frame && q.batch3 && link_mode == 2) return Link::batch3;
        return q.frame ? Link::frame : Link::waves;
    }
    if (q.frame && q.batch && link_mode != 1) return Link::batch;
    if (q.frame) return Link::frame;
    return q.lanes ? Link::lanes : Link::waves;
}
inline bool is_batch(Link l) { return l == Link::batch || l == Link::batch3; }
// the two-launch paths of a 2-D handle look for a track's nearest detection in a uniform grid (track.hip: DetGrid)
inline bool uses_det_grids(Link l, int dims) { return dims == 2 && (l == Link::waves || l == Link::lanes); }

// The grid blocks a handle is created with, for BL_MAX_BATCH frames each: three of k_bgrid's for the batch link (two for
// ysmr_tracker_prepare's callers, one for ysmr_tracker_run itself), one of DetGrid arrays for the two-launch paths, none
// for a handle that links with k_frame alone.
struct GridBlocks { size_t per_frame; int blocks; };
inline GridBlocks grid_blocks(const Caps &q, int max_det)
{
    const Link l = link_of(q, 2, 0);
    if (l == Link::batch) return GridBlocks{(size_t)bl_grid_dwords_max(max_det) * 4, 3};
    if (l == Link::frame) return GridBlocks{0, 0};
    return GridBlocks{grid_bytes_per_frame(max_det), 1};
}

}  // namespace tracker_plan

// Stand-alone check of the tracker's host-only part (ysmr_amd/csrc/tracker_plan.h), built as plain C++ -- with the host's
// address and undefined-behaviour sanitizers by tests/test_tracker_plan_sanitized.py.  Three parts:
//   cases   every line of the standard input is a case of tests/tracker_plan_cases.py (line_of); per case one line
//           "case NAME path=.. caps=.. frame_lds=.. batch_lds=.. batch3_lds=.. link_lds=.. block=..", or "case NAME error=..".
//   walk    a grid of capacity x max_det x filter banks: the state block's carving on a reserved (never touched) address
//           range -- every offset a multiple of 256, the arrays ascending and apart, the total equal to the parts summed
//           in 128 bits and to the run on a null base, both parities sharing exactly the arrays they share.  "walk ok N".
//   grid    for every m in 0 .. 2560 "grid M bl_grid_n bl_list_off bl_ovf_off bl_grid_dwords" (tests/test_cell_list_model.py).
// Returns 0, or says what failed and returns 1.
#include "tracker_plan.h"

#include <sys/mman.h>

#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

namespace plan = tracker_plan;
typedef unsigned __int128 u128;

static const char *name_of(plan::Link l)
{
    switch (l) {
    case plan::Link::frame: return "frame";
    case plan::Link::waves: return "waves";
    case plan::Link::lanes: return "lanes";
    case plan::Link::batch: return "batch";
    case plan::Link::batch3: return "batch3";
    }
    return "?";
}
static const char *name_of(plan::Bad b)
{
    switch (b) {
    case plan::Bad::none: return "none";
    case plan::Bad::size: return "size";
    case plan::Bad::filters: return "filters";
    case plan::Bad::fps: return "fps";
    case plan::Bad::horizons: return "horizons";
    case plan::Bad::horizon_max: return "horizon_max";
    }
    return "?";
}

// the caller's gains of a case: tests/tracker_plan_cases.py, perturb_gains
static std::vector<double> case_gains(const std::string &kind, double fps, int n_min, double n_max, int n_f)
{
    std::vector<double> g;
    int n_i[YSMR_MAX_FILTERS];
    if (kind == "closed" || plan::horizons(fps, n_min, n_max, n_f, n_i)) return g;
    size_t total = 0;
    for (int i = 0; i < n_f; ++i) total += 4 * (size_t)n_i[i];
    g.resize(total);
    size_t off = 0;
    for (int i = 0; i < n_f; ++i) { plan::closed_form_gain(n_i[i], g.data() + off); off += 4 * (size_t)n_i[i]; }
    if (kind == "cross") g[1] = 0.01;
    if (kind == "bent") g[0] += 0.01;
    if (kind == "faint") g[1] = 1e-300;
    return g;
}

static int run_cases()
{
    char name[128], kind[32];
    double gone, fps, n_max;
    int n_min, n_f, use_gsff, capacity, max_det, dims, mode;
    while (std::scanf("%127s %lf %lf %d %lf %d %d %d %d %31s %d %d", name, &gone, &fps, &n_min, &n_max, &n_f, &use_gsff, &capacity,
                      &max_det, kind, &dims, &mode) == 12) {
        const std::vector<double> caller = case_gains(kind, fps, n_min, n_max, n_f);
        plan::Config c;
        std::vector<double> gains;
        const plan::Status s = plan::configure(gone, fps, n_min, n_max, n_f, use_gsff, capacity, max_det,
                                               caller.empty() ? nullptr : caller.data(), c, gains);
        if (s) {
            std::printf("case %s error=%s\n", name, name_of(s.what));
            continue;
        }
        const plan::Caps q = plan::qualifies(c);
        TrackerDev d0, d1;
        BatchDev bd;
        double *pos3;
        const size_t block = plan::carve_state(nullptr, c, d0, d1, bd, pos3);
        std::string caps;
        for (auto [on, word] : {std::pair<bool, const char *>{q.frame, "frame"}, {q.lanes, "lanes"}, {q.batch, "batch"},
                                {q.batch3, "batch3"}, {q.link_lds, "link_lds"}})
            if (on) caps += std::string(caps.empty() ? "" : ",") + word;
        std::printf("case %s path=%s caps=%s frame_lds=%zu batch_lds=%zu batch3_lds=%zu link_lds=%zu block=%zu\n", name,
                    name_of(plan::link_of(q, dims, mode)), caps.c_str(), q.frame_lds, bl_lds_total(max_det), bl3_lds_total(max_det),
                    q.link_lds_bytes, block);
    }
    return 0;
}

struct Part { const char *name; const void *p; u128 bytes; };

static int walk_one(const plan::Config &c)
{
    TrackerDev n0, n1, d0, d1;
    BatchDev nb, bd;
    double *npos3, *pos3;
    const size_t total = plan::carve_state(nullptr, c, n0, n1, nb, npos3);
    if (n0.order || n1.order || nb.ring || npos3 || n0.n_tracks || n0.next_id || n0.err || n1.row_base || nb.head) {
        std::printf("null base: a pointer is not null (capacity %d max_det %d)\n", c.capacity, c.max_det);
        return 1;
    }
    void *base = mmap(nullptr, total, PROT_NONE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_NORESERVE, -1, 0);     // addresses only
    if (base == MAP_FAILED) { std::printf("mmap(%zu) failed\n", total); return 1; }
    int bad = 0;
    auto fail = [&](const char *what, const char *which) {
        std::printf("%s: %s (capacity %d max_det %d n_f %d hist_cap %d)\n", what, which, c.capacity, c.max_det, c.n_f, c.hist_cap);
        bad = 1;
    };
    if (plan::carve_state(base, c, d0, d1, bd, pos3) != total) fail("total", "differs from the null-base run");
    const u128 cap = (u128)c.capacity, md = (u128)c.max_det, seats = cap > (u128)BL_THREADS ? cap : (u128)BL_THREADS;
    if ((u128)bd.seat_cap != seats) fail("seat_cap", "wrong");
    const Part parts[] = {
        {"scalars", d0.n_tracks, 64}, {"order", d0.order, 4 * cap}, {"free_slots", d0.free_slots, 4 * cap}, {"id", d0.id, 4 * cap},
        {"gone", d0.gone, 4 * cap}, {"pos", d0.pos, 16 * cap}, {"info", d0.info, 12 * cap}, {"pos3", pos3, 8 * cap},
        {"hist", d0.hist, 16 * cap * (u128)c.hist_cap}, {"rec", d0.rec, 8 * (u128)c.rec_stride * cap},
        {"gains", d0.gains, 8 * (u128)(c.gain_total ? c.gain_total : 1)}, {"unused", d0.unused, 4 * md}, {"row_min", d0.row_min, 8 * cap},
        {"row_arg", d0.row_arg, 4 * cap}, {"row_gone", d0.row_gone, 4 * cap}, {"dead", d0.dead, 4 * cap}, {"new_cols", d0.new_cols, 4 * md},
        {"set_table", d0.set_table, 8 * (u128)c.table_cap}, {"link_key", d0.link_key, 8 * md}, {"link_row", d0.link_row, 4 * md},
        {"link_claim", d0.link_claim, 4 * cap}, {"claim_slot", d0.claim_slot, 4 * cap}, {"claim_row", d0.claim_row, 4 * cap},
        {"scalars 1", d1.n_tracks, 64}, {"order 1", d1.order, 4 * cap}, {"gone 1", d1.gone, 4 * cap}, {"row_min 1", d1.row_min, 8 * cap},
        {"row_arg 1", d1.row_arg, 4 * cap}, {"ring", bd.ring, 16 * (u128)(BL_HB + 1) * seats}, {"f64", bd.f64, 8 * (u128)BL_SF64 * seats},
        {"f32", bd.f32, 12 * seats}, {"i32", bd.i32, 24 * seats},
    };
    u128 at = 0;
    for (const Part &p : parts) {
        const u128 off = (u128)((const char *)p.p - (const char *)base);
        if (off % 256) fail("offset not a multiple of 256", p.name);
        if (off != at) fail("not where the arrays before it end", p.name);      // ascending, apart, nothing between
        at = off + (p.bytes + 255) / 256 * 256;
    }
    if (at != (u128)total) fail("total", "is not the sum of the parts");
    // the scalar words of a parity, and what the batch link keeps behind parity 0's
    for (const TrackerDev *q : {&d0, &d1})
        if (q->next_id != q->n_tracks + 1 || q->n_free != q->n_tracks + 3 || (const void *)q->row_base != (const void *)(q->n_tracks + 8))
            fail("scalars", "words are not where they were");
    if (d0.err != d0.n_tracks + 2 || d1.err != d0.err || bd.head != d0.n_tracks + 12) fail("scalars", "err / head");
    // parity 1 shares everything but the double-buffered arrays
    TrackerDev same = d1;
    same.n_tracks = d0.n_tracks; same.next_id = d0.next_id; same.n_free = d0.n_free; same.row_base = d0.row_base;
    same.order = d0.order; same.gone = d0.gone; same.row_min = d0.row_min; same.row_arg = d0.row_arg;
    if (std::memcmp(&same, &d0, sizeof(TrackerDev)) != 0) fail("parity 1", "differs from parity 0 beyond the double-buffered arrays");
    if (d1.n_tracks == d0.n_tracks || d1.order == d0.order || d1.gone == d0.gone || d1.row_min == d0.row_min || d1.row_arg == d0.row_arg)
        fail("parity 1", "shares a double-buffered array");
    if (d0.capacity != c.capacity || d0.max_det != c.max_det || d0.n_f != c.n_f || d0.hist_cap != c.hist_cap ||
        d0.table_cap != c.table_cap || d0.gain_total != c.gain_total || d0.rec_stride != c.rec_stride || d0.lik_min != 1e-20)
        fail("TrackerDev", "configuration not copied");
    munmap(base, total);
    return bad;
}

static int walk()
{
    const int sizes[] = {1, 2, 63, 64, 65, 255, 256, 257, 767, 768, 769, 1000, 2456, 2457, 4096, 8192, 65535, 65536};
    long n = 0;
    for (int capacity : sizes)
        for (int max_det : sizes)
            for (int n_f = 0; n_f <= YSMR_MAX_FILTERS; ++n_f)          // 0: no filter bank
                for (double n_max : {8.0, 30.0, 63.0}) {
                    plan::Config c;
                    std::vector<double> gains;
                    if (plan::configure(30.0, 30.0, 0, n_max, n_f ? n_f : 3, n_f != 0, capacity, max_det, nullptr, c, gains)) continue;
                    if (walk_one(c)) return 1;
                    ++n;
                }
    std::printf("walk ok %ld\n", n);
    return 0;
}

int main()
{
    if (run_cases() || walk()) return 1;
    for (int m = 0; m <= 2560; ++m) std::printf("grid %d %d %d %d %d\n", m, bl_grid_n(m), bl_list_off(m), bl_ovf_off(m), bl_grid_dwords(m));
    return 0;
}

// Stand-alone check of detection's host-only part (ysmr_amd/csrc/detect_plan.h), built as plain C++ -- with the host's
// address and undefined-behaviour sanitizers by tests/test_detect_plan_sanitized.py.  Two parts:
//   cases   every line of the standard input is a case of tests/detect_plan_cases.py (line_of): its kind (ws, thr, chain,
//           mean, levels), its name and its arguments; per case one line "case NAME key=value ...", or "case NAME error=..".
//   walk    a grid of small shapes: the workspace's layout (regions 256-aligned, ascending and apart, the counter block's
//           words inside it, a total that never shrinks when an argument grows, k_windows' item count as its kernel takes it),
//           the strip kernels' shapes (lanes, strips and segments that cover the frame; the kernel's item loop replayed: every
//           (frame, strip, segment) exactly once), the matrix-pipe kernel's (panels; its range cut replayed: every row of every
//           (frame, panel) column exactly once), the scales for cv2's taps.  "walk ok N".
// Returns 0, or says what failed and returns 1.
#include "detect_plan.h"

#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

namespace plan = detect_plan;
typedef unsigned __int128 u128;

static unsigned bits(float f) { unsigned u; std::memcpy(&u, &f, 4); return u; }

static void print_strip(const plan::StripShape &s)
{
    std::printf(" kernel=strip strips_x=%d out_lanes=%d seg_h=%d segs_y=%d blocks=%u", s.strips_x, s.out_lanes, s.seg_h, s.segs_y, s.blocks);
}

// the regions in the order they lie, with their sizes worked out here
struct Part { const char *name; size_t off; u128 bytes; };
static std::vector<Part> parts_of(const plan::Layout &l, int batch, int H, int W, int max_det)
{
    const u128 b = (u128)batch, bm = b * (u128)max_det, px = b * (u128)H * (u128)W;
    const u128 hull = 16 * 5 * (2 * (u128)W + 3), window = ((u128)(H + 2) * (u128)(W + 2) + 3) / 4;
    u128 arena = b * (hull > window ? hull : window);
    if (arena > 0x7FFFFFFFull) arena = 0x7FFFFFFFull;
    const u128 items = b * (u128)((H + 31) / 32) * (u128)((W + 32 * plan::WIN_GROUP - 1) / (32 * plan::WIN_GROUP));
    return {{"hdr", l.hdr, 256}, {"counters", l.counters, 4 * (b * plan::NR_STRIDE + 8)}, {"prev_n", l.prev_n, 4 * b},
            {"pixels", l.pixels, 4 * ((px + 7) / 8)}, {"holed", l.holed, 8 * (u128)plan::HOLED_CAP}, {"roots", l.roots, 4 * bm},
            {"order", l.order, 4 * bm}, {"bbox", l.bbox, 16 * bm}, {"euler4", l.euler4, 4 * bm}, {"nested", l.nested, 4 * bm},
            {"bbox_tmp", l.bbox_tmp, 16 * bm}, {"euler_tmp", l.euler_tmp, 4 * bm}, {"det_tmp", l.det_tmp, 20 * bm},
            {"arena", l.arena, 4 * arena}, {"oldbits", l.oldbits, 4 * items * 32 * plan::WIN_GROUP}};
}

static int run_cases()
{
    char kind[16], name[128];
    while (std::scanf("%15s %127s", kind, name) == 2) {
        std::printf("case %s", name);
        const std::string k = kind;
        if (k == "ws") {
            int batch, H, W, channels, max_det;
            if (std::scanf("%d %d %d %d %d", &batch, &H, &W, &channels, &max_det) != 5) return 1;
            const plan::Bad bad = plan::check_geometry(batch, H, W, channels, max_det);
            if (bad != plan::Bad::none) {
                std::printf(" error=%s\n", bad == plan::Bad::positive ? "positive" : bad == plan::Bad::channels ? "channels" : "too_large");
                continue;
            }
            const plan::Layout l = plan::layout(batch, H, W, max_det);
            std::string offs;
            for (const Part &p : parts_of(l, batch, H, W, max_det)) offs += (offs.empty() ? "" : ",") + std::to_string(p.off);
            std::printf(" total=%zu offsets=%s counters=%zu,%zu,%zu,%zu,%d pixel_cap=%u arena_floats=%u win_items=%lld", l.total, offs.c_str(),
                        l.n_holed, l.arena_used, l.barrier, l.max_roots, l.n_counters, l.pixel_cap, l.arena_floats, plan::win_items(batch, H, W).items);
        } else if (k == "thr") {
            int batch, H, W, channels, t_low, t_high, use_high, flavour, variant;
            long lds;
            plan::Knobs kn{};
            if (std::scanf("%d %d %d %d %d %d %d %d %d %d %d %ld", &batch, &H, &W, &channels, &t_low, &t_high, &use_high, &flavour, &variant,
                           &kn.thr_blocks, &kn.seg_h, &lds) != 12) return 1;
            const plan::ThresholdPlan p = plan::threshold_plan(batch, H, W, channels, t_low, t_high, use_high, flavour, variant, kn, (size_t)lds);
            std::printf(" workgroups=%d", plan::threshold_workgroups(flavour));
            switch (p.kernel) {
            case plan::Kernel::refused: std::printf(" kernel=refused"); break;
            case plan::Kernel::mfma:
                std::printf(" kernel=mfma variant=%d panels=%d panel_w=%d grid=%u by_xcd=%d start_rows=%d", p.mfma_variant, p.mfma.panels, p.mfma.panel_w,
                            p.mfma.grid, p.mfma.by_xcd, p.mfma.start_rows);
                break;
            case plan::Kernel::strip: print_strip(p.strip); std::printf(" by_xcd=%d", p.strip.by_xcd); break;
            case plan::Kernel::tile: std::printf(" kernel=tile grid=%ux%ux%u", p.tile_grid[0], p.tile_grid[1], p.tile_grid[2]); break;
            }
        } else if (k == "chain") {
            int batch, H, W, max_det, flavour;
            plan::Knobs kn{};
            if (std::scanf("%d %d %d %d %d %d %d %d", &batch, &H, &W, &max_det, &flavour, &kn.collect_blocks, &kn.clear_blocks, &kn.geo_blocks) != 8) return 1;
            const plan::ChainPlan c = plan::chain_plan(batch, H, W, max_det, flavour, kn, 2456);
            std::printf(" clear=%u windows=%u residue=%s:%u rank=%ux%u geometry=%u", c.clear, c.windows, c.residue_frames ? "frames" : "grid", c.residue,
                        c.rank_x, c.rank_y, c.geometry);
        } else if (k == "mean") {
            int batch, H, W, aligned;
            if (std::scanf("%d %d %d %d", &batch, &H, &W, &aligned) != 4) return 1;
            const plan::MeanPlan m = plan::mean_plan(batch, H, W, aligned != 0);
            std::printf(" parts=%d sum_blocks=%u", m.parts, m.sum_blocks);
            if (m.strip) print_strip(m.level);
            else std::printf(" kernel=thread groups_x=%d segs_y=%d blocks=%u", m.groups_x, m.segs_y, m.thr_blocks);
        } else if (k == "levels") {
            int inv, t_low, t_high, use_high, variant;
            if (std::scanf("%d %d %d %d %d", &inv, &t_low, &t_high, &use_high, &variant) != 5) return 1;
            float g[11];
            plan::gauss11(g);
            const plan::Scales sc = plan::choose_scales(g);
            const plan::LevelConsts c = plan::level_consts(sc, inv, t_low, t_high, use_high, variant);
            std::printf(" s=%.17g S=%.17g bound=%.17g col_scale=%08x row_scale=%08x neg_x_mul=%08x k_first=%08x d2=%08x sh=%d,%x,%d,%x", sc.s, sc.S,
                        sc.bound, bits(c.col_scale), bits(c.row_scale), bits(c.neg_x_mul), bits(c.k_first), bits(c.d2), c.sh1, c.k1, c.sh2, c.k2);
        } else {
            return 1;
        }
        std::printf("\n");
    }
    return 0;
}

static int bad(const char *what, const char *which, int batch, int H, int W, int extra = 0)
{
    std::printf("%s: %s (batch %d H %d W %d, %d)\n", what, which, batch, H, W, extra);
    return 1;
}

static int walk_layout(int batch, int H, int W, int max_det)
{
    const plan::Layout l = plan::layout(batch, H, W, max_det);
    u128 at = 0;
    for (const Part &p : parts_of(l, batch, H, W, max_det)) {
        if (p.off % 256) return bad("offset not a multiple of 256", p.name, batch, H, W, max_det);
        if ((u128)p.off != at) return bad("not where the regions before it end", p.name, batch, H, W, max_det);     // ascending, apart
        at = p.off + (p.bytes + 255) / 256 * 256;
    }
    if (at != (u128)l.total) return bad("total", "is not where the last region ends", batch, H, W, max_det);
    // the counter block: the per-frame counters, the shared words behind them, all inside the region and what k_clear zeroes
    const size_t frames_end = (size_t)batch * plan::NR_STRIDE;
    const size_t words[4] = {l.n_holed, l.arena_used, l.barrier, l.max_roots};
    for (int i = 0; i < 4; ++i) {
        if (words[i] < frames_end || words[i] >= (size_t)l.n_counters) return bad("counters", "a shared word outside its range", batch, H, W, i);
        for (int j = 0; j < i; ++j)
            if (words[i] == words[j]) return bad("counters", "two words share a place", batch, H, W, i);
    }
    if (l.n_holed != frames_end || l.arena_used != frames_end + 1 || l.barrier != frames_end + 2 || l.max_roots != frames_end + 3)
        return bad("counters", "words are not where they were", batch, H, W);
    if (l.counters + 4 * (size_t)l.n_counters > l.prev_n) return bad("counters", "what k_clear zeroes runs into the next region", batch, H, W);
    // k_windows' items as the kernel counts them
    const plan::WinItems wi = plan::win_items(batch, H, W);
    if (wi.per_frame != (long long)wi.groups_x * wi.rows_y || wi.items != wi.per_frame * batch || l.oldbits_words != (size_t)wi.items * 32 * plan::WIN_GROUP ||
        wi.groups_x * plan::WIN_GROUP * plan::WIN_CORE < W || wi.rows_y * plan::WIN_CORE < H)
        return bad("win_items", "does not cover the frame", batch, H, W);
    // monotone
    if (plan::layout(batch + 1, H, W, max_det).total < l.total || plan::layout(batch, H + 1, W, max_det).total < l.total ||
        plan::layout(batch, H, W + 1, max_det).total < l.total || plan::layout(batch, H, W, max_det + 1).total < l.total)
        return bad("total", "shrinks when an argument grows", batch, H, W, max_det);
    return 0;
}

// lanes, strips and segments; `visit(frame, strip, segment)` for every item of every wave, as the kernel's loop deals them
template <class Deal>
static int walk_strip(const char *who, const plan::StripShape &s, int lane_limit, int batch, int H, int W, Deal deal)
{
    if (s.out_lanes < 1 || s.out_lanes > lane_limit) return bad(who, "out_lanes beyond the lane limit", batch, H, W);
    if (s.strips_x * s.out_lanes * 4 < W || (s.strips_x - 1) * s.out_lanes * 4 >= W) return bad(who, "strips do not cover W, or one is empty", batch, H, W);
    if (s.seg_h < 1 || (long long)s.segs_y * s.seg_h < H || (long long)(s.segs_y - 1) * s.seg_h >= H) return bad(who, "segments do not cover H, or one is empty", batch, H, W);
    if (s.by_xcd && (batch % 8 != 0 || s.blocks % 8 != 0)) return bad(who, "by_xcd without a batch and a grid that are multiples of 8", batch, H, W);
    if (s.blocks < 1) return bad(who, "no block", batch, H, W);
    const int per_frame = s.strips_x * s.segs_y;
    std::vector<int> seen((size_t)batch * per_frame, 0);
    for (unsigned block = 0; block < s.blocks; ++block)
        for (int wave = 0; wave < 4; ++wave)
            deal(block, wave, per_frame, [&](int f, int sx, int sy) {
                if (f >= 0 && f < batch && sx >= 0 && sx < s.strips_x && sy >= 0 && sy < s.segs_y) ++seen[((size_t)f * s.segs_y + sy) * s.strips_x + sx];
                else seen[0] += 2;
            });
    for (int n : seen)
        if (n != 1) return bad(who, "an item is not visited exactly once", batch, H, W);
    return 0;
}

static int walk_threshold(int batch, int H, int W)
{
    const plan::Knobs none{};
    // k_threshold_strip (variant 1: the strip / tile kernels only)
    const plan::ThresholdPlan p = plan::threshold_plan(batch, H, W, 1, 5, 9, 1, 0, 1, none, 143828);
    const bool strip_geometry = (W & 3) == 0 && W >= 16 && H >= 2;
    if ((p.kernel == plan::Kernel::strip) != strip_geometry || (p.kernel == plan::Kernel::tile) == strip_geometry)
        return bad("threshold_plan", "strip | tile", batch, H, W);
    if (p.kernel == plan::Kernel::strip) {
        const plan::StripShape &s = p.strip;
        // detect.hip: k_threshold_strip's loop
        auto deal = [&](unsigned block, int wave_in_block, int per_frame, auto visit) {
            long long first, step, count;
            int f_mul, f_add;
            if (s.by_xcd) {
                first = (long long)(block >> 3) * 4 + wave_in_block; step = (long long)(s.blocks >> 3) * 4;
                count = (long long)(batch >> 3) * per_frame; f_mul = 8; f_add = (int)(block & 7u);
            } else {
                first = (long long)block * 4 + wave_in_block; step = (long long)s.blocks * 4;
                count = (long long)batch * per_frame; f_mul = 1; f_add = 0;
            }
            for (long long wave = first; wave < count; wave += step) {
                const int f = (int)(wave / per_frame) * f_mul + f_add;
                const int rem = (int)(wave % per_frame);
                visit(f, rem % s.strips_x, rem / s.strips_x);
            }
        };
        if (walk_strip("strip", s, plan::STRIP_MAX_OUT_LANES, batch, H, W, deal)) return 1;
    } else if (p.tile_grid[0] * plan::TW < (unsigned)W || p.tile_grid[1] * plan::TH < (unsigned)H || p.tile_grid[2] != (unsigned)batch) {
        return bad("tile", "the grid does not cover the frames", batch, H, W);
    }
    // k_level_strip
    const plan::MeanPlan m = plan::mean_plan(batch, H, W, true);
    if (m.strip != ((W & 3) == 0 && W >= 8) || plan::mean_plan(batch, H, W, false).strip) return bad("mean_plan", "strip | thread", batch, H, W);
    if (m.parts < 1 || m.sum_blocks < 1 || m.sum_blocks > (unsigned)plan::MG_BLOCKS) return bad("mean_plan", "k_gray_sums' parts or grid", batch, H, W);
    if (m.strip) {
        const plan::StripShape &s = m.level;
        // meangray.hip: k_level_strip's loop
        auto deal = [&](unsigned block, int wave_in_block, int per_frame, auto visit) {
            const long long n_items = (long long)batch * per_frame;
            for (long long item = (long long)block * 4 + wave_in_block; item < n_items; item += (long long)s.blocks * 4) {
                const int f = (int)(item / per_frame);
                const int rem = (int)(item - (long long)f * per_frame);
                visit(f, rem % s.strips_x, rem / s.strips_x);
            }
        };
        if (s.by_xcd) return bad("level strip", "by_xcd", batch, H, W);
        if (walk_strip("level strip", s, plan::LSTRIP_OUT_LANES, batch, H, W, deal)) return 1;
    } else if (m.groups_x * 4 < W || m.segs_y * plan::LEVEL_SEG < H || m.thr_blocks < 1) {
        return bad("mean_plan", "k_level_threshold's items do not cover the frame", batch, H, W);
    }
    // k_threshold_mfma
    for (int wanted : {256, 248, 7}) {
        plan::Knobs kn{};
        kn.thr_blocks = wanted;
        const plan::ThresholdPlan q = plan::threshold_plan(batch, H, W, 1, 5, 9, 1, 0, 0, kn, 143828);
        if ((q.kernel == plan::Kernel::mfma) != (strip_geometry && W >= 64 && H >= 18)) return bad("threshold_plan", "matrix-pipe | strip", batch, H, W);
        if (q.kernel != plan::Kernel::mfma) continue;
        const plan::MfmaShape &m = q.mfma;
        if (m.panel_w % 16 || m.panel_w > plan::TM_MAX_PANEL || m.panels * m.panel_w < W || (m.panels - 1) * m.panel_w >= W)
            return bad("mfma", "panels", batch, H, W, wanted);
        if (m.grid < 1 || m.grid > (unsigned)wanted || (m.by_xcd && (batch % 8 != 0 || m.grid % 8 != 0))) return bad("mfma", "grid", batch, H, W, wanted);
        // thr_mfma.hip: the range cut of k_threshold_mfma
        std::vector<int> seen((size_t)batch * m.panels * H, 0);
        for (unsigned block = 0; block < m.grid; ++block) {
            const int groups = m.by_xcd ? 8 : 1;
            const long long cols = (long long)(batch / groups) * m.panels;
            const long long nb = m.grid / groups, bi = m.by_xcd ? (block >> 3) : block;
            const long long vh = H + m.start_rows, v_all = cols * vh;
            auto real_row = [&](long long v) { const long long c = v / vh, r = v - c * vh; return c * H + (r > m.start_rows ? r - m.start_rows : 0); };
            long long g0 = real_row(v_all * bi / nb);
            const long long g1 = bi + 1 == nb ? cols * H : real_row(v_all * (bi + 1) / nb);
            const int f_add = m.by_xcd ? (int)(block & 7u) : 0;
            while (g0 < g1) {
                const long long col = g0 / H;
                const int f = (int)(col / m.panels) * groups + f_add, panel = (int)(col % m.panels);
                const int y0 = (int)(g0 % H), y1 = (int)std::min((long long)H, y0 + (g1 - g0));
                if (f < 0 || f >= batch || panel * m.panel_w >= W) return bad("mfma", "an item outside the batch", batch, H, W, wanted);
                for (int y = y0; y < y1; ++y) ++seen[((size_t)f * m.panels + panel) * H + y];
                g0 += y1 - y0;
            }
        }
        for (int n : seen)
            if (n != 1) return bad("mfma", "a row is not covered exactly once", batch, H, W, wanted);
    }
    return 0;
}

static int walk()
{
    const int batches[] = {1, 2, 3, 7, 8, 9, 16, 24}, heights[] = {1, 2, 17, 18, 19, 31, 32, 33, 64, 100, 231},
              widths[] = {1, 4, 8, 12, 16, 60, 64, 68, 232, 236, 1228, 1232, 1236, 2468};
    long n = 0;
    for (int batch : batches)
        for (int H : heights)
            for (int W : widths) {
                for (int max_det : {1, 63, 64, 2048})
                    if (walk_layout(batch, H, W, max_det)) return 1;
                if (walk_threshold(batch, H, W)) return 1;
                ++n;
            }
    // the scales for cv2's taps
    float g[11];
    plan::gauss11(g);
    const plan::Scales sc = plan::choose_scales(g);
    if (sc.S != 39.375 || !(1.1 * sc.bound <= 1.875 / sc.S) || !(sc.bound > 0.0)) {
        std::printf("scales: S %.6f bound %.6f\n", sc.S, sc.bound);
        return 1;
    }
    std::printf("walk ok %ld\n", n);
    return 0;
}

int main() { return run_cases() || walk(); }

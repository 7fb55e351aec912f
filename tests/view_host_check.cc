// view_host_check.cc -- the detection view's pixel rule (csrc/view_rule.h: the body of ysmr_view_batch_host, which is also the
// code that decides a pixel in csrc/view.hip's kernels) in a stand-alone host program, built as plain C++ with the address
// and undefined-behaviour sanitizers by tests/test_view_host_sanitized.py.  Every buffer is allocated at its exact size, so a
// byte read or written outside is reported.  Input (stdin), one case after another:
//   case <name> <n> <H> <W> <channels> <max_det> <n_rows> <first> <stride> <frame_bytes> <bottom_up> <row_begin> <row_end> <seed>
//   <n> det counts, then <n * max_det> detections of five floats (hex floats are accepted), then <n_rows> rows
//   "<frame> <track_id> <x> <y> <disappeared>"
// Frames are bytes of a 32-bit LCG from <seed>, below 200.  Output per case: "case <name> <status> <fnv1a-64 of the output>
// <blue pixels> <green pixels>", the output buffer having been filled with 0xA5 first.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "view_rule.h"

int main()
{
    char name[128];
    int n, H, W, channels, max_det, n_rows, first, stride, bottom_up;
    long long frame_bytes, row_begin, row_end;
    unsigned seed;
    while (scanf(" case %127s %d %d %d %d %d %d %d %d %lld %d %lld %lld %u", name, &n, &H, &W, &channels, &max_det, &n_rows, &first,
                 &stride, &frame_bytes, &bottom_up, &row_begin, &row_end, &seed) == 14) {
        std::vector<int32_t> count((size_t)n);
        std::vector<float> det((size_t)n * max_det * 5);
        for (auto &c : count)
            if (scanf("%" SCNd32, &c) != 1) return 2;
        for (auto &v : det)
            if (scanf("%f", &v) != 1) return 2;
        // (exactly n_rows rows, on the heap: no slack behind the last one)
        ysmr_row *rows = n_rows ? (ysmr_row *)malloc(sizeof(ysmr_row) * (size_t)n_rows) : nullptr;
        for (int i = 0; i < n_rows; ++i) {
            long long id;
            ysmr_row r;
            memset(&r, 0, sizeof r);
            if (scanf("%" SCNd32 " %lld %lf %lf %" SCNd32, &r.frame, &id, &r.x, &r.y, &r.disappeared) != 5) return 2;
            r.track_id = (int32_t)(uint32_t)id;
            rows[i] = r;
        }
        std::vector<uint8_t> frames((size_t)n * H * W * channels);
        uint32_t state = seed;
        for (auto &b : frames) { state = state * 1664525u + 1013904223u; b = (uint8_t)((state >> 24) % 200u); }
        std::vector<uint8_t> out((size_t)n * (size_t)frame_bytes, 0xA5);
        const char *why = ysmr::view::batch_host(frames.data(), n, H, W, channels, det.data(), count.data(), max_det, rows, row_begin,
                                                 row_end, first, out.data(), stride, (size_t)frame_bytes, bottom_up);
        uint64_t h = 1469598103934665603ull;
        long long blue = 0, green = 0;
        for (uint8_t b : out) { h ^= b; h *= 1099511628211ull; }
        if (!why)
            for (int f = 0; f < n; ++f)
                for (int y = 0; y < H; ++y)
                    for (int x = 0; x < W; ++x) {
                        const uint8_t *p = out.data() + (size_t)f * frame_bytes + (size_t)y * stride + 3 * (size_t)x;
                        blue += p[0] == 255 && p[1] == 0 && p[2] == 0;
                        green += p[0] == 0 && p[1] == 255 && p[2] == 0;
                    }
        printf("case %s %s %016" PRIx64 " %lld %lld\n", name, why ? "refused" : "ok", h, blue, green);
        free(rows);
    }
    return 0;
}

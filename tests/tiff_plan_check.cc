// Stand-alone check of the host-only plan code of ysmr_tiff_decode_batch (ysmr_amd/csrc/tiff_decode_plan.h), meant to be built with
// the host's address and undefined-behaviour sanitizers (tests/test_tiff_plan_sanitized.py builds and runs it).  It walks a grid
// of frame counts, shapes, strip heights and body sizes, the refused limits among them, and compares what the plan accepts and
// every size it gives with the same rules worked out in 128 bits: a product that wrapped somewhere would differ.  Prints
// "ok <cases>" and returns 0, or says what failed.
#include "tiff_decode_plan.h"

#include <climits>
#include <cstdio>
#include <vector>

typedef __int128 i128;

int main()
{
    const std::vector<int> frames = {INT_MIN, -1, 0, 1, 2, 65, 1920, 1 << 20, INT_MAX};
    const std::vector<int> sides = {INT_MIN, -1, 0, 1, 7, 96, 922, 1228, 46340, 46341, 65536, INT_MAX};
    const std::vector<int> strip_rows = {INT_MIN, -1, 0, 1, 6, 7, 922, INT_MAX};
    const std::vector<long long> bodies = {LLONG_MIN, -1, 0, 1, 1133416, INT_MAX, (long long)INT_MAX + 1, LLONG_MAX};
    const int compressions[] = {0, 1, 5, 8, 32773};
    long cases = 0, accepted = 0;
    for (int n : frames)
        for (int h : sides)
            for (int w : sides)
                for (int channels : {0, 1, 2, 3, 4})
                    for (int compression : compressions)
                        for (int predictor : {1, 2, 3})
                            for (int photometric : {-1, 0, 1, 2, 3})
                                for (int rows : strip_rows)
                                    for (long long body : bodies) {
                                        ++cases;
                                        tfd::Plan p = {};
                                        const bool ok = tfd::plan_of(n, h, w, channels, compression, predictor, photometric, rows, body, p);
                                        bool valid = n > 0 && h > 0 && w > 0 && (channels == 1 || channels == 3) &&
                                                     (compression == 1 || compression == 5 || compression == 32773) &&
                                                     (predictor == 1 || predictor == 2) && photometric >= 0 && photometric <= 2 &&
                                                     (photometric == 2) == (channels == 3) && rows >= 1 && rows <= h && body >= 0 &&
                                                     body <= INT_MAX;
                                        i128 per_frame = 0, strips = 0, frame_bytes = 0;
                                        if (valid) {
                                            frame_bytes = (i128)h * w * channels;
                                            per_frame = ((i128)h + rows - 1) / rows;
                                            strips = per_frame * n;
                                            valid = frame_bytes <= INT_MAX && strips <= INT_MAX;
                                        }
                                        if (ok != valid) {
                                            std::printf("%s: n %d, %d x %d x %d, compression %d, predictor %d, photometric %d, rows %d, body %lld\n",
                                                        ok ? "accepted" : "refused", n, h, w, channels, compression, predictor, photometric, rows, body);
                                            return 1;
                                        }
                                        if (!ok) continue;
                                        ++accepted;
                                        const i128 want = (strips * 4 + 255) / 256 * 256;
                                        if ((i128)p.total != want || p.total == 0 || p.n_strips != (long long)strips ||
                                            p.strips_per_frame != (int)per_frame || p.frame_bytes != (long long)frame_bytes ||
                                            p.row_bytes != (long long)w * channels || p.strip_status + (size_t)strips * 4 > p.total) {
                                            std::printf("n %d, %d x %d x %d, rows %d: total %zu, %lld strips\n", n, h, w, channels, rows, p.total, p.n_strips);
                                            return 1;
                                        }
                                        // the strips the call would derive from the count tile the frame again
                                        const int back = tfd::rows_per_strip_of(p.n_strips, n, h);
                                        if (back <= 0 || ((i128)h + back - 1) / back != per_frame) {
                                            std::printf("n %d, %d rows in strips of %d: %d strips give strips of %d\n", n, h, rows, p.strips_per_frame, back);
                                            return 1;
                                        }
                                    }
    // counts that tile no frame
    const long long counts[] = {LLONG_MIN, -1, 0, 1, 2, 3, 6, 7, 9, 10, 11, 922, 923, INT_MAX, LLONG_MAX};
    for (long long s : counts)
        for (int n : frames)
            for (int h : sides) {
                ++cases;
                const int rows = tfd::rows_per_strip_of(s, n, h);
                const bool valid = n > 0 && h > 0 && s > 0 && s % n == 0 && s / n <= h &&
                                   ((i128)h + (((i128)h + s / n - 1) / (s / n)) - 1) / (((i128)h + s / n - 1) / (s / n)) == s / n;
                if ((rows > 0) != valid || (valid && (rows > h || ((i128)h + rows - 1) / rows != s / n))) {
                    std::printf("%lld strips, %d frames of %d rows: strips of %d rows\n", s, n, h, rows);
                    return 1;
                }
            }
    if (accepted == 0) { std::printf("no case was accepted\n"); return 1; }
    std::printf("ok %ld cases, %ld accepted\n", cases, accepted);
    return 0;
}

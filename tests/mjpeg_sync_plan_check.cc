// Stand-alone check of the host-only plan code of ysmr_mjpeg_decode_batch_sync (ysmr_amd/csrc/mjpeg_decode_plan.h), meant to be
// built with the host's address and undefined-behaviour sanitizers (tests/test_mjpeg_sync_plan_sanitized.py builds and runs it).
// It walks a grid of shapes and chunk sizes, the limits among them, and compares every workspace size with the same sum worked
// out in 128 bits: a size_t that wrapped somewhere would differ from it.  Prints "ok <cases>" and returns 0, or says what failed.
#include "mjpeg_decode_plan.h"

#include <climits>
#include <cstdio>
#include <vector>

typedef unsigned __int128 u128;

static u128 up(u128 v) { return (v + 255) / 256 * 256; }

// the workspace of a call, part by part, without size_t
static u128 expected(int n, const mjd::Geo &g, int max_chunk)
{
    const u128 N = (u128)n;
    return up(N * sizeof(mjd::FrameInfo)) + up(N * 4 * 64 * 2) + up(N * 8 * sizeof(mjd::HuffRaw)) + up(N * (u128)g.mcus * 4) +
           up(N * (u128)g.blocks * 128) + up(N * (u128)g.planes) + up(N * up((u128)max_chunk + 8)) + up(N * 4);
}

int main()
{
    const std::vector<int> frames = {INT_MIN, -1, 0, 1, 2, 65, 248, 65535, 1 << 20, INT_MAX};
    const std::vector<int> sides = {INT_MIN, 0, 1, 7, 8, 9, 922, 1228, 65535, 65536, INT_MAX};
    const std::vector<int> chunks = {INT_MIN, -1, 0, 1, 255, 256, 257, 136992, mjd::SYNC_MAX_CHUNK, mjd::SYNC_MAX_CHUNK + 1, INT_MAX};
    long cases = 0, accepted = 0;
    for (int n : frames)
        for (int h : sides)
            for (int w : sides)
                for (int sampling = -1; sampling <= 4; ++sampling)
                    for (int channels : {1, 3})
                        for (int chunk : chunks) {
                            ++cases;
                            mjd::Geo g = {};
                            mjd::SyncPlan p = {};
                            const bool ok = mjd::sync_plan_of(n, h, w, channels, sampling, chunk, g, p);
                            const bool valid = n > 0 && h > 0 && w > 0 && h <= 65535 && w <= 65535 && sampling >= 0 && sampling <= 3 &&
                                               channels == (sampling == 0 ? 1 : 3) && chunk > 0 && chunk <= mjd::SYNC_MAX_CHUNK;
                            if (ok && !valid) {
                                std::printf("accepted: n %d, %d x %d, sampling %d, channels %d, chunk %d\n", n, h, w, sampling, channels, chunk);
                                return 1;
                            }
                            if (!valid) continue;
                            const u128 want = expected(n, g, chunk);
                            const bool fits = want <= (u128)SIZE_MAX;
                            if (ok != fits || (ok && (u128)p.total != want) || (ok && p.total % 256) ||
                                (ok && (p.data < p.base.total || p.data_bytes < p.data + (size_t)n * p.data_pitch || p.data_pitch < (size_t)chunk + 8))) {
                                std::printf("n %d, %d x %d, sampling %d, chunk %d: %s, total %zu, expected %.0Lf (%s a size_t)\n", n, h, w, sampling,
                                            chunk, ok ? "accepted" : "refused", ok ? p.total : (size_t)0, (long double)want, fits ? "fits" : "beyond");
                                return 1;
                            }
                            accepted += ok;
                        }
    if (accepted == 0) { std::printf("no case was accepted\n"); return 1; }
    std::printf("ok %ld cases, %ld accepted\n", cases, accepted);
    return 0;
}

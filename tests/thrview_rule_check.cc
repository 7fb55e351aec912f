// thrview_rule_check.cc -- the threshold view's pixel rule (csrc/thrview_rule.h: the body of ysmr_thrview_batch_host, which is
// also the code that decides a pixel in csrc/thrview.hip's kernel) in a stand-alone host program, built as plain C++ with the
// address and undefined-behaviour sanitizers by tests/test_thrview_sanitized.py.  Every input is a heap block of exactly its
// size, so a byte read outside is reported; the output has 64 guard bytes on either side, which the program checks itself,
// as it checks the row padding and the gaps between frames.  No input: the shapes of tests/thrview_model.py, every mode, 1
// and 3 channels, both row orders, the tight stride and a wider one with a gap between frames.  Frames, class maps and masks
// are bytes of a 32-bit LCG (frames: the byte; cls: its low three bits; mask: 255 where its bit 3 is set).  Output per case:
// "case <n> <H> <W> <channels> <mode> <bottom_up> <stride> <frame_bytes> <fnv1a-64 of the output>", then "ok <cases>".
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "thrview_rule.h"

static uint32_t state;
static uint8_t next_byte()
{
    state = state * 1664525u + 1013904223u;
    return (uint8_t)(state >> 24);
}

int main()
{
    static const int shapes[][3] = {{1, 1, 1}, {3, 3, 5}, {2, 5, 16}, {2, 4, 63}, {1, 7, 67}, {2, 3, 1040}};
    const size_t GUARD = 64;
    int cases = 0;
    for (const auto &shape : shapes)
        for (int channels = 1; channels <= 3; channels += 2)
            for (int mode = 0; mode <= 2; ++mode)
                for (int bottom_up = 0; bottom_up <= 1; ++bottom_up)
                    for (int wide = 0; wide <= 1; ++wide) {
                        const int n = shape[0], H = shape[1], W = shape[2];
                        const size_t pixels = (size_t)n * H * W;
                        const int stride = ((3 * W + 3) & ~3) + 8 * wide;
                        const size_t frame_bytes = (size_t)stride * H + 12 * wide;
                        state = (uint32_t)(W * 1000 + H * 10 + channels);
                        uint8_t *frames = (uint8_t *)malloc(pixels * channels), *cls = (uint8_t *)malloc(pixels), *mask = (uint8_t *)malloc(pixels);
                        uint8_t *block = (uint8_t *)malloc(GUARD + n * frame_bytes + GUARD);
                        if (!frames || !cls || !mask || !block) return 2;
                        for (size_t i = 0; i < pixels * channels; ++i) frames[i] = next_byte();
                        for (size_t i = 0; i < pixels; ++i) cls[i] = next_byte() & 7;
                        for (size_t i = 0; i < pixels; ++i) mask[i] = (next_byte() & 8) ? 255 : 0;
                        memset(block, 0x5A, GUARD);
                        memset(block + GUARD, 0xA5, n * frame_bytes);
                        memset(block + GUARD + n * frame_bytes, 0x5A, GUARD);
                        uint8_t *out = block + GUARD;
                        // (pointers a mode does not read are NULL here: the loop must not touch them)
                        const char *why = ysmr::thrview::batch_host(mode == 2 ? frames : nullptr, cls, mode == 1 ? nullptr : mask, n, H, W, channels, mode,
                                                                    out, stride, frame_bytes, bottom_up);
                        if (why) { printf("refused: %s\n", why); return 3; }
                        for (size_t i = 0; i < GUARD; ++i)
                            if (block[i] != 0x5A || block[GUARD + n * frame_bytes + i] != 0x5A) { printf("guard byte %zu written\n", i); return 4; }
                        for (int f = 0; f < n; ++f) {
                            const uint8_t *frame = out + (size_t)f * frame_bytes;
                            for (int y = 0; y < H; ++y)
                                for (int k = 3 * W; k < stride; ++k)
                                    if (frame[(size_t)y * stride + k] != 0) { printf("padding of row %d not zero\n", y); return 5; }
                            for (size_t k = (size_t)stride * H; k < frame_bytes; ++k)
                                if (frame[k] != 0xA5) { printf("gap behind frame %d written\n", f); return 6; }
                            // ... and every pixel against the rule's one-pixel form
                            for (int y = 0; y < H; ++y)
                                for (int x = 0; x < W; ++x) {
                                    const size_t at = ((size_t)f * H + y) * W + x;
                                    uint8_t want[3];
                                    const uint8_t *src = frames + at * channels;
                                    ysmr::thrview::pixel(mode, cls[at], mask[at], src[0], src[channels == 3 ? 1 : 0], src[channels == 3 ? 2 : 0], want);
                                    const uint8_t *got = frame + (size_t)(bottom_up ? H - 1 - y : y) * stride + 3 * (size_t)x;
                                    if (memcmp(got, want, 3)) { printf("pixel (%d, %d, %d) differs from the one-pixel rule\n", f, y, x); return 7; }
                                }
                        }
                        uint64_t h = 1469598103934665603ull;
                        for (size_t i = 0; i < n * frame_bytes; ++i) { h ^= out[i]; h *= 1099511628211ull; }
                        printf("case %d %d %d %d %d %d %d %zu %016" PRIx64 "\n", n, H, W, channels, mode, bottom_up, stride, frame_bytes, h);
                        free(frames); free(cls); free(mask); free(block);
                        ++cases;
                    }
    // what the entries refuse is refused before anything is written
    uint8_t in[16] = {0}, out[64];
    memset(out, 0xA5, sizeof out);
    using ysmr::thrview::batch_host;
    const bool refused = batch_host(in, nullptr, in, 1, 1, 1, 1, 0, out, 4, 4, 0) && batch_host(in, in, nullptr, 1, 1, 1, 1, 0, out, 4, 4, 0) &&
                         batch_host(nullptr, in, in, 1, 1, 1, 1, 2, out, 4, 4, 0) && batch_host(in, in, in, 1, 1, 1, 2, 0, out, 4, 4, 0) &&
                         batch_host(in, in, in, 1, 1, 1, 1, 3, out, 4, 4, 0) && batch_host(in, in, in, 1, 1, 2, 1, 0, out, 4, 4, 0) &&
                         batch_host(in, in, in, 1, 1, 1, 1, 0, nullptr, 4, 4, 0) && batch_host(in, in, in, 1, 2, 1, 1, 0, out, 4, 4, 0);
    for (uint8_t b : out)
        if (b != 0xA5 || !refused) { printf("a refused call wrote, or a bad call was not refused\n"); return 8; }
    printf("ok %d\n", cases);
    return 0;
}

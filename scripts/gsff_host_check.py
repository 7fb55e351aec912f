#!/usr/bin/env python3
"""bl_gsff<GATED = true> (k_batch) against bl_gsff<GATED = false> (k_track_lanes: the form both kernels shared before
round 11) on the CPU, bit for bit.

The filter bank's source is plain C++ but for its qualifiers: this cuts BlSeat, bl_exp_nonpos, bl_grow_at, bl_mode_of and
bl_gsff out of ysmr_amd/csrc/batch_link.h, puts them in front of a driver with a ring of its own, builds that with the host
compiler (-ffp-contract=off, as the device build) and runs random tracks through both variants the way their kernels
call them: leave[] requested for every filter / only where the window is full, `fresh` / S.len = 0 for a track born in
the frame, the lane's leftovers of an earlier track, handles of one, two and three filters, and -- at random frames -- the
end of a launch, where k_batch turns its threshold into the stored mode and back.  Every output, every field of the seat
and the ring must agree in every frame.

    python scripts/gsff_host_check.py [trials]        exit status 0: identical
"""
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "ysmr_amd", "csrc", "batch_link.h")

PRELUDE = r'''
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <cmath>
#include <random>
#include <vector>
#define __device__
#define __forceinline__ inline
struct double2 { double x, y; };
static inline double2 make_double2(double x, double y) { return {x, y}; }
static inline double __longlong_as_double(long long v) { double d; memcpy(&d, &v, 8); return d; }
constexpr int BL_NF = 3, BL_HB = 32;
struct TrackerDev { int n_f, hist_cap; int n_i[8]; double lik_min; };
struct BatchDev { double2 *ring; int seat_cap; };
struct BlGains { double alpha[BL_NF][2], beta[BL_NF][2]; };
static inline void bl_ring_store(const BatchDev &bd, int pos, int seat, double x, double y) { bd.ring[(size_t)pos * bd.seat_cap + seat] = make_double2(x, y); }
static inline double2 bl_ring_load(const BatchDev &bd, int pos, int seat) { return bd.ring[(size_t)pos * bd.seat_cap + seat]; }
// (a ring entry as bl_gsff takes it: here the two doubles; k_batch hands it the four registers of a 16-byte load)
static inline double2 bl_entry(const double2 &e) { return e; }
static inline void bl_entry_set(double2 &e, double x, double y) { e = make_double2(x, y); }
'''

DRIVER = r'''
int main(int argc, char **argv)
{
    const int trials = argc > 1 ? atoi(argv[1]) : 2000;
    std::mt19937_64 rng(7);
    std::uniform_real_distribution<double> U(0, 1);
    long long frames_done = 0, rare = 0;
    for (int trial = 0; trial < trials; ++trial) {
        const int nf = 1 + trial % 3;
        TrackerDev t{};
        t.n_f = nf; t.lik_min = 1e-20;
        for (int i = 1; i <= nf; ++i) t.n_i[i - 1] = (int)(30.0 / nf * i);             // ysmr_tracker_create, n_min = 0, n_max = 30
        if (trial % 7 == 3) { t.n_i[0] = 1 + (int)(rng() % 3); for (int i = 1; i < nf; ++i) t.n_i[i] = t.n_i[i - 1] + 1 + (int)(rng() % 12); }
        t.hist_cap = t.n_i[nf - 1] + 1;
        BlGains g{};
        for (int f = 0; f < nf; ++f) {      // closed_form_gain's shape: alpha, beta of a horizon of N frames (any finite values will do)
            const double N = t.n_i[f];
            g.alpha[f][0] = 2.0 * (2.0 * N - 1.0) / (N * (N + 1.0)); g.beta[f][0] = 6.0 / (N * (N + 1.0));
            g.alpha[f][1] = g.alpha[f][0] * 1.001; g.beta[f][1] = g.beta[f][0] * 0.999;
        }
        std::vector<double2> ring_a(BL_HB), ring_b(BL_HB);
        for (auto &e : ring_a) e = make_double2(U(rng) * 1e3, U(rng) * 1e3);           // an earlier track's entries
        ring_b = ring_a;
        BatchDev ba{ring_a.data(), 1}, bb{ring_b.data(), 1};
        BlSeat A{}, B{};
        A.len = B.len = (int)(rng() % 40); A.mode = B.mode = (int)(rng() % 4);         // a free lane's leftovers
        A.s0x[1] = B.s0x[1] = 3.5; A.w[2] = B.w[2] = 0.25;
        int head = (int)(rng() % BL_HB), grow_at = 12345, unused = 0;
        bool alive = false;
        double x = U(rng) * 1000, y = U(rng) * 900, vx = U(rng) - 0.5, vy = U(rng) - 0.5;
        const int n_frames = 80 + (int)(rng() % 60);
        for (int f = 0; f < n_frames; ++f) {
            bool fresh = false;
            const int hn[BL_NF] = {t.n_i[0], nf > 1 ? t.n_i[1] : 0x7FFFFFFF, nf > 2 ? t.n_i[2] : 0x7FFFFFFF};
            double2 la[BL_NF], lb[BL_NF];            // requested before the claims: every filter's / the full windows'
            for (int k = 0; k < BL_NF; ++k) la[k] = lb[k] = make_double2(0.0, 0.0);
            if (alive)
                for (int k = 0; k < BL_NF; ++k) {
                    if (k < nf) la[k] = bl_ring_load(ba, (head - t.n_i[k]) & (BL_HB - 1), 0);
                    if (B.len >= hn[k]) lb[k] = bl_ring_load(bb, (head - hn[k]) & (BL_HB - 1), 0);
                }
            if (!alive && U(rng) < 0.3) { alive = true; fresh = true; B.len = 0; grow_at = 0; }       // k_batch's registration
            if (alive) {
                x += vx + (U(rng) - 0.5) * 0.3; y += vy + (U(rng) - 0.5) * 0.3;
                double z0 = (double)(float)x, z1 = (double)(float)y;
                if (U(rng) < 0.02) z0 += 400.0;          // a jump: the likelihoods fall below lik_min
                double a0, a1, b0, b1;
                bl_gsff<false>(A, t, t, ba, g, 0, head, la, z0, z1, fresh, unused, a0, a1);
                const int before = grow_at;
                bl_gsff<true>(B, t, t, bb, g, 0, head, lb, z0, z1, fresh, grow_at, b0, b1);
                rare += before != grow_at;
                ++frames_done;
                B.mode = bl_mode_of(grow_at, nf, hn);
                const bool same = !memcmp(&a0, &b0, 8) && !memcmp(&a1, &b1, 8) && A.len == B.len && A.mode == B.mode
                    && !memcmp(A.s0x, B.s0x, sizeof A.s0x) && !memcmp(A.s1x, B.s1x, sizeof A.s1x) && !memcmp(A.s0y, B.s0y, sizeof A.s0y)
                    && !memcmp(A.s1y, B.s1y, sizeof A.s1y) && !memcmp(A.w, B.w, sizeof A.w) && !memcmp(A.xa, B.xa, sizeof A.xa)
                    && !memcmp(A.xb, B.xb, sizeof A.xb) && !memcmp(&A.px, &B.px, 8) && !memcmp(&A.py, &B.py, 8)
                    && !memcmp(ring_a.data(), ring_b.data(), sizeof(double2) * BL_HB);
                if (!same) { printf("MISMATCH: trial %d frame %d, %d filters, length %d / %d, mode %d / %d\n", trial, f, nf, A.len, B.len, A.mode, B.mode); return 1; }
                if (U(rng) < 0.15) grow_at = bl_grow_at(B.len, B.mode, nf, hn);      // a launch ends here: the seat is stored and loaded
                if (U(rng) < 0.02) alive = false;                                    // the track dies; the lane keeps what it held
            }
            head = (head + 1) & (BL_HB - 1);
        }
    }
    printf("ok: %lld track-frames bit-identical, %lld of them with a moved threshold\n", frames_done, rare);
    return 0;
}
'''


def cut(text, start, end):
    a = text.index(start)
    return text[a:text.index(end, a)]


def source():
    h = open(HEADER).read()
    return (PRELUDE + cut(h, "struct BlSeat {", "// rest format") + cut(h, "__device__ __forceinline__ void bl_exp_nonpos", "// The history length at which")
            + cut(h, "__device__ __forceinline__ int bl_grow_at", "// Nearest detection of a prediction") + DRIVER)


def compiler():
    return shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")


def run(trials=2000):
    """(exit status, output); None where there is no host compiler."""
    cxx = compiler()
    if not cxx:
        return None
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "gsff_host.cpp"), os.path.join(tmp, "gsff_host")
        with open(src, "w") as fh:
            fh.write(source())
        subprocess.run([cxx, "-O1", "-std=c++17", "-ffp-contract=off", "-Wno-attributes", "-o", exe, src], check=True)
        p = subprocess.run([exe, str(trials)], capture_output=True, text=True)
        return p.returncode, p.stdout.strip()


if __name__ == "__main__":
    r = run(int(sys.argv[1]) if len(sys.argv) > 1 else 2000)
    if r is None:
        raise SystemExit("no host C++ compiler")
    print(r[1])
    sys.exit(r[0])

// marks_rule_check.cc -- csrc/marks_rule.h alone, built with the host compiler (tests/test_marks_model_cpu.py): the row rule of
// the annotated video's marks on rows given as text, for a comparison with annotate.build_marks.
//   marks_rule_check <n_frames> <subtype or -1> <by_track 0|1>  <  rows
// A row per input line: x and y as the 16 hex digits of their float64 bits, t, id, moving, turn_points, phenotype (hex bits).
// A line per row comes out: kept (0|1), key (hex), x, y, track_id, style; then "bits <key bits> distinct <0|1>".
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "marks_rule.h"

static double of_bits(uint64_t u)
{
    double d;
    memcpy(&d, &u, 8);
    return d;
}

int main(int argc, char **argv)
{
    if (argc != 4) return 2;
    const int n_frames = atoi(argv[1]), subtype = atoi(argv[2]), by_track = atoi(argv[3]);
    std::vector<uint32_t> ids;
    uint64_t xb, yb, pb;
    long long t;
    unsigned long id;
    int moving, turn;
    while (scanf("%" SCNx64 " %" SCNx64 " %lld %lu %d %d %" SCNx64, &xb, &yb, &t, &id, &moving, &turn, &pb) == 7) {
        const double x = of_bits(xb), y = of_bits(yb);
        const bool keep = ysmr::marks::kept(x, y, (int64_t)t, n_frames, subtype >= 0, of_bits(pb), subtype);
        const ysmr_mark m = ysmr::marks::mark_of_row(x, y, (uint32_t)id, (int8_t)moving, (int8_t)turn);
        const uint64_t key = keep ? ysmr::marks::sort_key((int64_t)t, (uint32_t)id, by_track != 0) : ysmr::marks::KEY_DROPPED;
        printf("%d %016" PRIx64 " %d %d %u %u\n", keep ? 1 : 0, key, (int)m.x, (int)m.y, (unsigned)m.track_id, (unsigned)m.style);
        ids.push_back((uint32_t)id);
    }
    printf("bits %d distinct %d\n", ysmr::marks::key_bits(n_frames),
           ids.empty() ? 1 : (int)ysmr::marks::first_ids_distinct(ids.data(), (long long)ids.size()));
    return 0;
}

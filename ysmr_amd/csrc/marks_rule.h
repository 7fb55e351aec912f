// marks_rule.h -- which rows of the evaluated table become marks of the annotated video and what a row's mark is, in the one
// form that the kernels of marks.hip and a stand-alone host program both compile (plain C++ as well as HIP): what
// annotate.build_marks does to a row (ysmr/track_eval.py:1419-1447).
//
// ROW RULE.  A row is kept if POSITION_X and POSITION_Y are finite, 0 <= POSITION_T < n_frames and, where a subtype is
// selected, motility_phenotype == its code (a NaN phenotype equals none).  Its mark: x, y truncated toward zero (int(), as
// upstream) and moved to the ends of int32 where they lie beyond them; the 32 bits of the id; style 1 where moving == 0, else
// 2 where turn_points == 1, else 0.  Its sort key puts frames in order and, inside a frame, the table's order: the frame above
// the id (table order: by track) or above zeros (file order); the sort is stable, so the row number settles the rest.
#pragma once
#include <cstdint>
#include "hd.h"
#include "ysmr_hip.h"

namespace ysmr {
namespace marks {

constexpr uint64_t KEY_DROPPED = ~0ull;        // behind every kept row's key: a kept frame is below 2^31 - 1

YSMR_HD_FORCE bool finite_bits(double v)
{
    union { double d; uint64_t u; } b;
    b.d = v;
    return ((b.u >> 52) & 0x7FFu) != 0x7FFu;
}

YSMR_HD_FORCE bool kept(double x, double y, int64_t t, int n_frames, bool by_subtype, double phenotype, int subtype)
{
    return finite_bits(x) && finite_bits(y) && t >= 0 && t < (int64_t)n_frames && (!by_subtype || phenotype == (double)subtype);
}

YSMR_HD_FORCE int32_t coordinate(double v)
{
    const double lo = -2147483648.0, hi = 2147483647.0;
    return (int32_t)(v < lo ? lo : v > hi ? hi : v);             // (a conversion truncates toward zero, as int())
}

YSMR_HD_FORCE uint32_t style(int8_t moving, int8_t turn_points) { return moving == 0 ? 1u : turn_points == 1 ? 2u : 0u; }

YSMR_HD_FORCE uint64_t sort_key(int64_t t, uint32_t track_id, bool by_track) { return ((uint64_t)t << 32) | (by_track ? track_id : 0u); }

// bits of the key a sort has to look at: the id's 32 and as many (a multiple of 8) as hold n_frames ITSELF, so that
// KEY_DROPPED's ones in those bits lie above every kept frame
YSMR_HD_FORCE int key_bits(int n_frames)
{
    int bits = 8;
    while (bits < 32 && ((uint32_t)n_frames >> bits)) bits += 8;
    return 32 + bits;
}

// upstream's rough check (helper_file.py:892-905): rows 0 .. 5, or all rows of a shorter table, hold pairwise distinct ids
YSMR_HD_FORCE bool first_ids_distinct(const uint32_t *track_id, long long n_rows)
{
    const int n = n_rows < 6 ? (int)n_rows : 6;
    bool distinct = true;
    for (int a = 1; a < n; ++a)
        for (int b = 0; b < a; ++b) distinct = distinct && track_id[a] != track_id[b];
    return distinct;
}

YSMR_HD_FORCE ysmr_mark mark_of_row(double x, double y, uint32_t track_id, int8_t moving, int8_t turn_points)
{
    ysmr_mark m;
    m.x = coordinate(x);
    m.y = coordinate(y);
    m.track_id = track_id;
    m.style = style(moving, turn_points);
    return m;
}

}  // namespace marks
}  // namespace ysmr

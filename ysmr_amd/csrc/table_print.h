// table_print.h -- what the printers of a table of typed columns share (table_csv.hip: csv lines; xlsx.hip: worksheet rows).
// A printer owns its row rule and its row kernel's loop over the cells; everything behind a staged row is here, once: the
// float64 cell with its wide side slot, the row kernel's tail (prefix sum over the rows' lengths, the piece's length, the
// compacted piece) and the launches of the wide-cell pre-pass and of the packing kernel.  The kernels and host functions
// declared here are defined in table_csv.hip.  Only .hip files include this; the host-only arithmetic is table_csv_plan.h.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "common.h"
#include "prim.h"
#include "fmt.h"
#include "table_csv_plan.h"

namespace tablep {

struct Columns {
    const void *data[MAX_COLUMNS];
    int32_t type[MAX_COLUMNS];
    int32_t n;
};

// the types of the columns into types[], or why the call is refused (the error is set)
int check_columns(int n_columns, const ysmr_table_column *columns, long long n_rows, int32_t *types);

// the same for the size functions, which refuse with 0 and no message: false for a column count outside 1 .. 16 or no columns
bool types_of(int n_columns, const ysmr_table_column *columns, int32_t *types);

// wide_incl [n_rows]: wide cells per row, then their inclusive sums; wide_temp: scan_words(n_rows) words; slots / slot_len:
// 24 bytes and a length per wide cell, in (row, column) order; *wide_cells_dev: their number.  n_rows > 0, a float64 column
// among the n_columns.  Asynchronous on st.
void launch_wide_cells(hipStream_t st, int n_columns, const void *const *data, const int32_t *types, long long n_rows,
                       uint32_t *wide_incl, uint32_t *wide_temp, char *slots, uint8_t *slot_len, uint32_t *wide_cells_dev);

// out[0, head) is written already.  Piece g (piece_len[g] bytes at pieces + g * piece_stride, 16-byte aligned with 16 bytes of
// slack behind the text; piece_incl: the lengths' inclusive sums) goes behind the head and the pieces before it, the
// suffix_bytes at suffix_dev behind the last piece, and *length_dev becomes the length of it all.  Nothing is written at or
// behind out + capacity.  n_pieces = 0 and suffix_bytes = 0 are served.  Asynchronous on st.
void launch_pack(hipStream_t st, const char *pieces, size_t piece_stride, const uint32_t *piece_len, const uint32_t *piece_incl,
                 unsigned n_pieces, size_t head, const char *suffix_dev, uint32_t suffix_bytes, char *out, size_t capacity,
                 unsigned long long *length_dev);

// The float64 cell of a staged row: a wide value is copied from its side slot -- wide_at, the row's next one, moves on --, any
// other is printed in place with the lane's digits.  Returns the end.
__device__ __forceinline__ char *put_f64_cell(char *q, double v, const char *__restrict__ slots, const uint8_t *__restrict__ slot_len,
                                              uint32_t &wide_at, ysmr_fmt::Digits &digits)
{
    if (!ysmr_fmt::is_wide_cell(v)) return ysmr_fmt::put_f64_steady(q, v, digits);
    const char *slot = slots + (size_t)wide_at * WIDE_SLOT;
    const int l = slot_len[wide_at];
    for (int b = 0; b < l; ++b) q[b] = slot[b];
    ++wide_at;
    return q + l;
}

// The tail of a row kernel of R lanes, a row each: lane `lane` has staged len bytes at s_text + lane * row_stride (0: no row).
// s_off [R + 1] and, for more than one wave, s_wave [R / 64] are the caller's LDS.  Where every row goes in the piece, the
// piece's length to piece_len[blockIdx.x], and the workgroup's text to pieces + blockIdx.x * piece_stride compacted.
template <int R>
__device__ __forceinline__ void store_piece(uint32_t len, const char *s_text, int row_stride, uint32_t *s_off, uint32_t *s_wave,
                                            char *__restrict__ pieces, size_t piece_stride, uint32_t *__restrict__ piece_len)
{
    static_assert(R >= 64 && (R & (R - 1)) == 0, "whole waves, and the search below halves R");
    const int lane = threadIdx.x;
    uint32_t incl = ysmr::prim::wave_inclusive_sum(len);
    if constexpr (R > 64) {
        if ((lane & 63) == 63) s_wave[lane >> 6] = incl;
        __syncthreads();
        for (int w = 0; w < (lane >> 6); ++w) incl += s_wave[w];
    }
    if (lane == 0) s_off[0] = 0u;
    s_off[lane + 1] = incl;
    __syncthreads();
    const uint32_t total = s_off[R];
    if (lane == 0) piece_len[blockIdx.x] = total;
    // the piece leaves compacted: lane after lane sixteen consecutive bytes of it, gathered from the rows they lie in
    uint4 *const out = (uint4 *)(pieces + (size_t)blockIdx.x * piece_stride);
    for (uint32_t chunk = (uint32_t)lane; chunk * 16u < total; chunk += (uint32_t)R) {
        const uint32_t first = chunk * 16u;
        int r = 0;
#pragma unroll
        for (int step = R / 2; step; step >>= 1)                 // the last row that begins at or before `first`
            if (s_off[r + step] <= first) r += step;
        uint32_t pos = first - s_off[r], row_len = s_off[r + 1] - s_off[r];
        const char *src = s_text + (size_t)r * row_stride;
        uint32_t word[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            uint32_t w = 0;
#pragma unroll
            for (int b = 0; b < 4; ++b) {
                if (first + 4u * k + b < total) {
                    w |= (uint32_t)(uint8_t)src[pos] << (8 * b);
                    if (++pos == row_len && r + 1 < R) { ++r; src += row_stride; pos = 0; row_len = s_off[r + 1] - s_off[r]; }
                }
            }
            word[k] = w;
        }
        out[chunk] = make_uint4(word[0], word[1], word[2], word[3]);
    }
}

}  // namespace tablep

// The figures' PNG files, finished on the device: the lettering (ysmr_plot_stamp) and the zlib stream of the scanlines
// (ysmr_png_deflate).  gfx950, wave64.
//
// The stream is ONE deflate block in the fixed Huffman code (RFC 1951, 3.2.6) over the scanline bytes: H rows of
// S = 1 + 3 W bytes, a filter byte 0 in front of every row.  A row is cut into pieces of PNG_PIECE bytes and a piece is parsed
// on its own: no match crosses a piece's end, a match's source may lie anywhere before it.  Two distances are searched, 3
// (the pixel before) and S (the byte above, while S <= 32768); the parse is greedy ("The figures").
//
//   k_png_maps    a thread per scanline byte, a block per piece: one bit per byte and distance (byte == byte - distance),
//                 a wave's ballot is one 64-bit word of the map; and the piece's share of Adler-32
//   k_png_count   a lane per piece walks the two maps with ctz and counts the bits of its codes; exclusive prefix
//                 inside the block, the block's total
//   k_png_finish  one block: prefix over the block totals, Adler-32 in a fixed order, the two header bytes, the
//                 checksum behind the last code, the stream's length
//   k_png_emit    the walk again, the codes written from the piece's bit offset
//
// The output is zeroed first; the end-of-block code is seven zero bits and is never written.  Words a piece shares with
// its neighbours (its first, its last) are OR-ed in atomically, the words between are its own and plainly stored.
#include <hip/hip_runtime.h>

#include "common.h"
#include "prim.h"

namespace {

constexpr int PNG_PIECE = 1024;                 // bytes; a multiple of 64 * 4: a block of k_png_maps makes whole map words
constexpr int PNG_MAX_SIDE = 16384;
constexpr int PNG_MAX_MATCH = 258;
constexpr uint32_t ADLER = 65521u;
constexpr int STAMP_MAX_RECORDS = 4096;
constexpr int STAMP_BLOCKS = 32;                // per record, striding over its bitmap

struct Geometry {
    int W, H, S;            // S: bytes of a scanline
    int row_words;          // 64-bit map words of a row
    int row_pieces;
    long long pieces;
    long long blocks;       // of k_png_count / k_png_emit: 256 pieces each
    // the code of distance S: 5 bits (as the value, most significant bit first in the stream), extra bits
    int use_row, dist_code, dist_extra_bits, dist_extra;
};

Geometry geometry(int W, int H)
{
    Geometry g{};
    g.W = W, g.H = H, g.S = 1 + 3 * W;
    g.row_words = (g.S + 63) / 64;
    g.row_pieces = (g.S + PNG_PIECE - 1) / PNG_PIECE;
    g.pieces = (long long)H * g.row_pieces;
    g.blocks = (g.pieces + 255) / 256;
    g.use_row = g.S <= 32768;
    const int dd = g.S - 1;                                 // >= 3
    if (dd < 4) {
        g.dist_code = dd;
    } else {
        int k = 31 - __builtin_clz((unsigned)dd);
        g.dist_code = 2 * k + ((dd >> (k - 1)) & 1);
        g.dist_extra_bits = k - 1;
        g.dist_extra = dd & ((1 << (k - 1)) - 1);
    }
    return g;
}

// workspace: the two maps, the pieces' Adler shares and bit offsets, the block totals
struct Layout { size_t m3, ms, part, off, tot, bytes; };
Layout layout(const Geometry &g)
{
    Layout l{};
    const size_t map = ysmr::align_up((size_t)g.H * g.row_words * 8, 256);
    l.m3 = 0;
    l.ms = map;
    l.part = 2 * map;
    l.off = l.part + ysmr::align_up((size_t)g.pieces * 8, 256);
    l.tot = l.off + ysmr::align_up((size_t)g.pieces * 4, 256);
    l.bytes = l.tot + ysmr::align_up((size_t)g.blocks * 8, 256);
    return l;
}

size_t stream_bound(const Geometry &g)
{
    const size_t bits = 3 + 9 * (size_t)g.H * g.S + 7;      // every code spends at most 9 bits on a byte
    return ysmr::align_up((bits + 7) / 8 + 6, 4) + 4;         // + a word: the packer stores whole words
}

// ---- the maps and Adler-32 ---------------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void k_png_maps(const uint8_t *__restrict__ rgb, int W, int H, int use_row, int row_words,
                                                  unsigned long long *__restrict__ m3, unsigned long long *__restrict__ ms,
                                                  uint2 *__restrict__ part)
{
    __shared__ uint32_t s_a[4], s_b[4];
    const int S = 1 + 3 * W, r = blockIdx.y, k = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint8_t *row = rgb + (size_t)r * 3 * W;            // scanline byte c > 0 is row[c - 1]
    const uint8_t *above = row - (size_t)3 * W;              // read only where r > 0
    const unsigned long long n = (unsigned long long)H * S;
    uint32_t a = 0, b = 0;
#pragma unroll
    for (int it = 0; it < PNG_PIECE / 256; ++it) {
        const int c = k * PNG_PIECE + it * 256 + (int)threadIdx.x;
        bool e3 = false, es = false;
        if (c < S) {
            const uint32_t v = c ? row[c - 1] : 0u;
            if (c >= 3)
                e3 = (c > 3 ? row[c - 4] : 0u) == v;
            else if (r > 0)
                e3 = above[S - 4 + c] == v;                  // scanline byte S - 3 + c >= 1 of the row above
            if (use_row && r > 0) es = (c ? above[c - 1] : 0u) == v;
            const unsigned long long pos = (unsigned long long)r * S + c;
            a += v;
            b += (uint32_t)((n - pos) % ADLER) * v;          // < 2^24 each, four of them
        }
        const unsigned long long w3 = __ballot(e3), ws = __ballot(es);
        const int word = k * (PNG_PIECE / 64) + it * 4 + wave;
        if (lane == 0 && word < row_words) {
            m3[(size_t)r * row_words + word] = w3;
            ms[(size_t)r * row_words + word] = ws;
        }
    }
    b %= ADLER;
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        a += (uint32_t)__shfl_down((int)a, d, 64);
        b += (uint32_t)__shfl_down((int)b, d, 64);
    }
    if (lane == 0) s_a[wave] = a, s_b[wave] = b;
    __syncthreads();
    if (threadIdx.x == 0)
        part[(size_t)r * gridDim.x + k] = make_uint2((s_a[0] + s_a[1] + s_a[2] + s_a[3]) % ADLER, (s_b[0] + s_b[1] + s_b[2] + s_b[3]) % ADLER);
}

// ---- the parse -------------------------------------------------------------------------------------------------------

// the 1-bits of `m` from bit i on, at most `cap` (cap <= the piece's bytes left: the words read are the piece's)
__device__ __forceinline__ int run_of(const unsigned long long *__restrict__ m, int i, int cap)
{
    int w = i >> 6;
    const int b = i & 63;
    unsigned long long t = ~m[w] >> b;
    if (t) return min((int)__builtin_ctzll(t), cap);
    int n = 64 - b;
    while (n < cap) {
        t = ~m[++w];
        if (t) {
            n += (int)__builtin_ctzll(t);
            break;
        }
        n += 64;
    }
    return min(n, cap);
}

// sink.literal(i), sink.match(length, row): row = 0 is distance 3, row = 1 distance S
template <typename Sink>
__device__ __forceinline__ void parse_piece(const unsigned long long *__restrict__ m3, const unsigned long long *__restrict__ ms, int len,
                                            int use_row, Sink &sink)
{
    int i = 0;
    while (i < len) {
        const int cap = min(PNG_MAX_MATCH, len - i);
        const int l3 = run_of(m3, i, cap);
        const int ls = use_row ? run_of(ms, i, cap) : 0;
        if (l3 >= ls && l3 >= 3) {
            sink.match(l3, 0);
            i += l3;
        } else if (ls >= 4) {
            sink.match(ls, 1);
            i += ls;
        } else if (l3 >= 3) {
            sink.match(l3, 0);
            i += l3;
        } else {
            sink.literal(i);
            ++i;
        }
    }
}

// length 3..258 -> its symbol 257..285 and extra bits
__device__ __forceinline__ void length_symbol(int length, int &sym, int &extra_bits, int &extra)
{
    const int l = length - 3;
    if (length == PNG_MAX_MATCH) {
        sym = 285, extra_bits = 0, extra = 0;
    } else if (l < 8) {
        sym = 257 + l, extra_bits = 0, extra = 0;
    } else {
        extra_bits = 29 - __builtin_clz((unsigned)l);         // floor(log2 l) - 2
        sym = 261 + 4 * extra_bits + ((l >> extra_bits) & 3);
        extra = l & ((1 << extra_bits) - 1);
    }
}

struct Piece {
    const unsigned long long *m3, *ms;
    const uint8_t *row;     // of the canvas
    int c0, len;            // first scanline byte, bytes
};

__device__ __forceinline__ Piece piece_at(long long p, const uint8_t *__restrict__ rgb, int W, int row_words, int row_pieces,
                                          const unsigned long long *__restrict__ m3, const unsigned long long *__restrict__ ms)
{
    const int S = 1 + 3 * W;
    const long long r = p / row_pieces;
    const int k = (int)(p - r * row_pieces);
    Piece q;
    q.m3 = m3 + (size_t)r * row_words + k * (PNG_PIECE / 64);
    q.ms = ms + (size_t)r * row_words + k * (PNG_PIECE / 64);
    q.row = rgb + (size_t)r * 3 * W;
    q.c0 = k * PNG_PIECE;
    q.len = min(PNG_PIECE, S - q.c0);
    return q;
}

struct CountSink {
    const Piece &q;
    int dist_bits;          // 5 + the extra bits of distance S
    uint32_t bits;
    __device__ __forceinline__ void literal(int i)
    {
        const int c = q.c0 + i;
        bits += (c ? q.row[c - 1] : 0u) < 144u ? 8u : 9u;
    }
    __device__ __forceinline__ void match(int length, int row)
    {
        int sym, eb, e;
        length_symbol(length, sym, eb, e);
        bits += (sym < 280 ? 7u : 8u) + (uint32_t)eb + (row ? (uint32_t)dist_bits : 5u);
    }
};

__global__ __launch_bounds__(256) void k_png_count(const uint8_t *__restrict__ rgb, int W, int row_words, int row_pieces, long long pieces,
                                                   int use_row, int dist_extra_bits, const unsigned long long *__restrict__ m3,
                                                   const unsigned long long *__restrict__ ms, uint32_t *__restrict__ piece_off,
                                                   unsigned long long *__restrict__ block_tot)
{
    __shared__ uint32_t s_wave[4];
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    uint32_t mine = 0;
    if (p < pieces) {
        const Piece q = piece_at(p, rgb, W, row_words, row_pieces, m3, ms);
        CountSink sink{q, 5 + dist_extra_bits, 0u};
        parse_piece(q.m3, q.ms, q.len, use_row, sink);
        mine = sink.bits;                                    // <= 9 * PNG_PIECE
    }
    const uint32_t incl = ysmr::prim::wave_inclusive_sum(mine);
    if ((threadIdx.x & 63) == 63) s_wave[threadIdx.x >> 6] = incl;
    __syncthreads();
    uint32_t before = incl - mine;
    for (int w = 0; w < (int)(threadIdx.x >> 6); ++w) before += s_wave[w];
    if (p < pieces) piece_off[p] = before;
    if (threadIdx.x == 255) block_tot[blockIdx.x] = (unsigned long long)before + mine;
}

__device__ __forceinline__ void or_byte(uint32_t *out, unsigned long long at, uint32_t v) { atomicOr(&out[at >> 2], v << (8 * (at & 3))); }

// One block.  block_tot becomes its exclusive prefix; the header, the checksum and the length are written.
__global__ __launch_bounds__(256) void k_png_finish(unsigned long long *__restrict__ block_tot, long long blocks, const uint2 *__restrict__ part,
                                                    long long pieces, unsigned long long n_bytes, uint32_t *__restrict__ out,
                                                    unsigned long long *__restrict__ out_len)
{
    __shared__ unsigned long long s_sum[256], s_a[256], s_b[256];
    const int t = threadIdx.x;
    const long long per = (blocks + 255) / 256, lo = min((long long)t * per, blocks), hi = min(lo + per, blocks);
    unsigned long long sum = 0, a = 0, b = 0;
    for (long long i = lo; i < hi; ++i) sum += block_tot[i];
    for (long long i = t; i < pieces; i += 256) {            // < 2^20 pieces, each share < 2^16
        const uint2 v = part[i];
        a += v.x, b += v.y;
    }
    s_sum[t] = sum, s_a[t] = a, s_b[t] = b;
    __syncthreads();
    unsigned long long before = 0;
    for (int k = 0; k < t; ++k) before += s_sum[k];
    for (long long i = lo; i < hi; ++i) {
        const unsigned long long v = block_tot[i];
        block_tot[i] = before;
        before += v;
    }
    if (t == 255) {                                          // `before` is the total now
        a = 1, b = n_bytes % ADLER;                          // Adler-32 starts at a = 1: it is counted once per byte in b
        for (int k = 0; k < 256; ++k) a += s_a[k], b += s_b[k];
        a %= ADLER, b %= ADLER;
        const unsigned long long end_bit = 16 + 3 + before + 7;      // two header bytes, the block's header, the codes, end of block
        const unsigned long long tail = (end_bit + 7) >> 3;
        atomicOr(&out[0], 0x78u | 0x01u << 8 | 3u << 16);    // BFINAL = 1, BTYPE = 01: bits 1, 1, 0
        or_byte(out, tail, (uint32_t)(b >> 8));
        or_byte(out, tail + 1, (uint32_t)(b & 255));
        or_byte(out, tail + 2, (uint32_t)(a >> 8));
        or_byte(out, tail + 3, (uint32_t)(a & 255));
        *out_len = tail + 4;
    }
}

struct EmitSink {
    const Piece &q;
    uint32_t *out;
    unsigned long long word;    // of the next store
    int fill;                   // bits waiting in acc, < 32 between calls
    bool shared;                // the next word stored may hold a neighbour's bits
    unsigned long long acc;
    uint32_t dist_code_rev;     // distance S: the 5 code bits reversed, the extra bits above them
    int dist_bits;
    __device__ __forceinline__ void put(uint32_t bits, int len)     // len <= 31; the stream fills bytes from bit 0
    {
        acc |= (unsigned long long)bits << fill;
        fill += len;
        if (fill >= 32) {
            if (shared) atomicOr(&out[word], (uint32_t)acc);
            else out[word] = (uint32_t)acc;
            shared = false;
            ++word;
            acc >>= 32;
            fill -= 32;
        }
    }
    __device__ __forceinline__ void code(uint32_t value, int len) { put(__brev(value) >> (32 - len), len); }   // Huffman: top bit first
    __device__ __forceinline__ void literal(int i)
    {
        const int c = q.c0 + i;
        const uint32_t v = c ? q.row[c - 1] : 0u;
        if (v < 144u) code(0x30u + v, 8);
        else code(0x190u + v - 144u, 9);
    }
    __device__ __forceinline__ void match(int length, int row)
    {
        int sym, eb, e;
        length_symbol(length, sym, eb, e);
        const int len = sym < 280 ? 7 : 8;
        const uint32_t c = __brev(sym < 280 ? (uint32_t)(sym - 256) : 0xC0u + (uint32_t)(sym - 280)) >> (32 - len);
        put(c | (uint32_t)e << len, len + eb);               // <= 13 bits
        if (row) put(dist_code_rev, dist_bits);              // <= 18 bits
        else put(__brev(2u) >> 27, 5);                       // distance 3 is code 2
    }
    __device__ __forceinline__ void flush()
    {
        if (fill > 0) atomicOr(&out[word], (uint32_t)acc);
    }
};

__global__ __launch_bounds__(256) void k_png_emit(const uint8_t *__restrict__ rgb, int W, int row_words, int row_pieces, long long pieces,
                                                  int use_row, int dist_code, int dist_extra_bits, int dist_extra,
                                                  const unsigned long long *__restrict__ m3, const unsigned long long *__restrict__ ms,
                                                  const uint32_t *__restrict__ piece_off, const unsigned long long *__restrict__ block_pre,
                                                  uint32_t *__restrict__ out)
{
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    if (p >= pieces) return;
    const Piece q = piece_at(p, rgb, W, row_words, row_pieces, m3, ms);
    const unsigned long long start = 16 + 3 + block_pre[blockIdx.x] + piece_off[p];
    EmitSink sink{q, out, start >> 5, (int)(start & 31), true, 0ull,
                  (__brev((uint32_t)dist_code) >> 27) | (uint32_t)dist_extra << 5, 5 + dist_extra_bits};
    parse_piece(q.m3, q.ms, q.len, use_row, sink);
    sink.flush();
}

// ---- the lettering ---------------------------------------------------------------------------------------------------

__device__ __forceinline__ bool stamp_valid(const ysmr_stamp &s, unsigned long long n_bits)
{
    return s.w > 0 && s.h > 0 && (unsigned long long)s.bit_offset + (unsigned long long)s.w * (unsigned long long)s.h <= n_bits;
}
__device__ __forceinline__ bool stamp_bit(const uint8_t *__restrict__ bits, unsigned long long at) { return (bits[at >> 3] >> (at & 7)) & 1; }

// blockIdx.y: the record.  A set bit's pixel is stored unless a later record has a set bit there: the last record wins.
__global__ __launch_bounds__(256) void k_png_stamp(uint8_t *__restrict__ rgb, int W, int H, const ysmr_stamp *__restrict__ records, int n,
                                                   const uint8_t *__restrict__ bits, unsigned long long n_bits)
{
    const int j = blockIdx.y;
    const ysmr_stamp s = records[j];
    if (!stamp_valid(s, n_bits)) return;
    const unsigned long long pixels = (unsigned long long)s.w * (unsigned long long)s.h;
    for (unsigned long long at = (unsigned long long)blockIdx.x * 256 + threadIdx.x; at < pixels; at += (unsigned long long)gridDim.x * 256) {
        if (!stamp_bit(bits, s.bit_offset + at)) continue;
        const long long x = (long long)s.x + (long long)(at % (unsigned)s.w), y = (long long)s.y + (long long)(at / (unsigned)s.w);
        if (x < 0 || y < 0 || x >= W || y >= H) continue;
        bool hidden = false;
        for (int m = j + 1; m < n && !hidden; ++m) {
            const ysmr_stamp o = records[m];
            const long long dx = x - o.x, dy = y - o.y;
            hidden = stamp_valid(o, n_bits) && dx >= 0 && dy >= 0 && dx < o.w && dy < o.h &&
                     stamp_bit(bits, o.bit_offset + (unsigned long long)dy * (unsigned long long)o.w + (unsigned long long)dx);
        }
        if (hidden) continue;
        uint8_t *px = rgb + ((size_t)y * W + (size_t)x) * 3;
        px[0] = (uint8_t)(s.colour & 255u), px[1] = (uint8_t)((s.colour >> 8) & 255u), px[2] = (uint8_t)((s.colour >> 16) & 255u);
    }
}

int check_canvas(int width, int height)
{
    if (width < 1 || height < 1 || width > PNG_MAX_SIDE || height > PNG_MAX_SIDE)
        return ysmr::fail(YSMR_ERR_ARG, "the canvas must be within 1..%d pixels each way, got %d x %d", PNG_MAX_SIDE, width, height);
    return YSMR_OK;
}

}  // namespace

extern "C" {

size_t ysmr_png_workspace_bytes(int width, int height)
{
    if (width < 1 || height < 1 || width > PNG_MAX_SIDE || height > PNG_MAX_SIDE) return 0;
    return layout(geometry(width, height)).bytes;
}

size_t ysmr_png_stream_bytes_max(int width, int height)
{
    if (width < 1 || height < 1 || width > PNG_MAX_SIDE || height > PNG_MAX_SIDE) return 0;
    return stream_bound(geometry(width, height));
}

int ysmr_png_deflate(void *stream, const uint8_t *rgb_dev, int width, int height, void *workspace_dev, size_t workspace_bytes,
                     uint8_t *out_dev, size_t out_bytes, unsigned long long *out_len_dev)
{
    if (int rc = check_canvas(width, height)) return rc;
    const Geometry g = geometry(width, height);
    const Layout l = layout(g);
    const size_t bound = stream_bound(g);
    if (!rgb_dev || !workspace_dev || !out_dev || !out_len_dev)
        return ysmr::fail(YSMR_ERR_ARG, "rgb_dev, workspace_dev, out_dev and out_len_dev must not be NULL");
    if (workspace_bytes < l.bytes) return ysmr::fail(YSMR_ERR_ARG, "the workspace holds %zu bytes, %zu are needed", workspace_bytes, l.bytes);
    if (out_bytes < bound) return ysmr::fail(YSMR_ERR_ARG, "the output holds %zu bytes, ysmr_png_stream_bytes_max is %zu", out_bytes, bound);
    if (((uintptr_t)workspace_dev & 7) || ((uintptr_t)out_dev & 3) || ((uintptr_t)out_len_dev & 7))
        return ysmr::fail(YSMR_ERR_ARG, "workspace_dev and out_len_dev must be 8-byte aligned, out_dev 4-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    char *ws = (char *)workspace_dev;
    unsigned long long *m3 = (unsigned long long *)(ws + l.m3), *ms = (unsigned long long *)(ws + l.ms), *tot = (unsigned long long *)(ws + l.tot);
    uint2 *part = (uint2 *)(ws + l.part);
    uint32_t *off = (uint32_t *)(ws + l.off), *out = (uint32_t *)out_dev;
    YSMR_HIP_CHECK(hipMemsetAsync(out_dev, 0, bound, st));
    hipLaunchKernelGGL(k_png_maps, dim3((unsigned)g.row_pieces, (unsigned)g.H), dim3(256), 0, st, rgb_dev, g.W, g.H, g.use_row, g.row_words, m3, ms, part);
    hipLaunchKernelGGL(k_png_count, dim3((unsigned)g.blocks), dim3(256), 0, st, rgb_dev, g.W, g.row_words, g.row_pieces, g.pieces, g.use_row,
                       g.dist_extra_bits, m3, ms, off, tot);
    hipLaunchKernelGGL(k_png_finish, dim3(1), dim3(256), 0, st, tot, g.blocks, part, g.pieces, (unsigned long long)g.H * g.S, out, out_len_dev);
    hipLaunchKernelGGL(k_png_emit, dim3((unsigned)g.blocks), dim3(256), 0, st, rgb_dev, g.W, g.row_words, g.row_pieces, g.pieces, g.use_row,
                       g.dist_code, g.dist_extra_bits, g.dist_extra, m3, ms, off, tot, out);
    YSMR_LAUNCH_CHECK();
    return YSMR_OK;
}

int ysmr_plot_stamp(void *stream, uint8_t *rgb_dev, int width, int height, const ysmr_stamp *records_dev, int n_records,
                    const uint8_t *bits_dev, size_t bits_bytes)
{
    if (width < 1 || height < 1 || width > 32768 || height > 32768)
        return ysmr::fail(YSMR_ERR_ARG, "the canvas must be within 1..32768 pixels each way, got %d x %d", width, height);
    if (n_records < 0 || n_records > STAMP_MAX_RECORDS) return ysmr::fail(YSMR_ERR_ARG, "n_records must be in 0..%d, got %d", STAMP_MAX_RECORDS, n_records);
    if (bits_bytes > ((size_t)1 << 28)) return ysmr::fail(YSMR_ERR_ARG, "bits_bytes must be at most 2^28, got %zu", bits_bytes);
    if (n_records == 0) return YSMR_OK;
    if (!rgb_dev || !records_dev || !bits_dev) return ysmr::fail(YSMR_ERR_ARG, "rgb_dev, records_dev and bits_dev must not be NULL");
    hipLaunchKernelGGL(k_png_stamp, dim3(STAMP_BLOCKS, (unsigned)n_records), dim3(256), 0, (hipStream_t)stream, rgb_dev, width, height, records_dev,
                       n_records, bits_dev, (unsigned long long)bits_bytes * 8);
    YSMR_LAUNCH_CHECK();
    return YSMR_OK;
}

}  // extern "C"

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
//
// ysmr_png_deflate_dynamic, further down, is a second stream beside this one: one block in a dynamic Huffman code, four
// distances.  It shares run_of, length_symbol and the packer's scheme and changes nothing ysmr_png_deflate launches.
#include <hip/hip_runtime.h>

#include "common.h"
#include "png_codes.h"
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

// ---- the dynamic stream (ysmr_png_deflate_dynamic) ----------------------------------------------------------------------
//
// One block of BTYPE = 10 over the same scanline bytes and the same pieces.  Four distances are searched, 3, S, S - 3 and
// S + 3 (the pixel before, above, above-right, above-left), each only while it is at most 32768 and the source lies inside the
// stream; at a byte the longest match wins (at least 3 bytes at distance 3, 4 at the others), ties go in the order 3, S, S - 3,
// S + 3.  With the distances 3 and S alone this is parse_piece's rule.  The codes come from the whole parse's histogram
// (png_codes.h), so the pieces are walked three times, each walk reading the four maps and the literals only:
//
//   k_png_dmaps    k_png_maps with four maps; a source byte may lie one or two rows up
//   k_png_dhist    a lane per piece counts its symbols into the block's LDS histogram, the block adds it to the global one
//                  (integer atomics: the sums do not depend on the order)
//   k_png_dcodes   one block: code lengths, canonical codes, the block's header (png_codes.h)
//   k_png_dsize    k_png_count with the real code lengths
//   k_png_dfinish  k_png_finish; it places the header and the end-of-block code as well
//   k_png_demit    k_png_emit with the code tables in LDS

struct Dist4 {
    int mask;                       // bit k: distance k is searched (bit 0 always)
    int sym[4], extra_bits[4], extra[4];
};

Dist4 distances(const Geometry &g)
{
    Dist4 d{};
    const int dist[4] = {3, g.S, g.S - 3, g.S + 3};
    for (int k = 0; k < 4; ++k) {
        if (dist[k] > 32768) continue;                        // not searched: symbol 0, so that a table look-up stays in range
        d.mask |= 1 << k;
        const int dd = dist[k] - 1;
        if (dd < 4) {
            d.sym[k] = dd;
        } else {
            const int b = 31 - __builtin_clz((unsigned)dd);
            d.sym[k] = 2 * b + ((dd >> (b - 1)) & 1);
            d.extra_bits[k] = b - 1;
            d.extra[k] = dd & ((1 << (b - 1)) - 1);
        }
    }
    return d;
}

constexpr int DYN_CODES_WORDS = ysmr::pngc::N_BOTH + 1 + ysmr::pngc::HEADER_WORDS;     // the tables, the header's bits, the header

// workspace: the four maps, the pieces' Adler shares and bit offsets, the block totals, the histogram, k_png_dcodes' results
struct DynLayout { size_t maps, map_words, part, off, tot, hist, codes, bytes; };
DynLayout dyn_layout(const Geometry &g)
{
    DynLayout l{};
    const size_t map = ysmr::align_up((size_t)g.H * g.row_words * 8, 256);
    l.maps = 0;
    l.map_words = map / 8;
    l.part = 4 * map;
    l.off = l.part + ysmr::align_up((size_t)g.pieces * 8, 256);
    l.tot = l.off + ysmr::align_up((size_t)g.pieces * 4, 256);
    l.hist = l.tot + ysmr::align_up((size_t)g.blocks * 8, 256);
    l.codes = l.hist + ysmr::align_up((size_t)ysmr::pngc::N_BOTH * 4, 256);
    l.bytes = l.codes + ysmr::align_up((size_t)DYN_CODES_WORDS * 4, 256);
    return l;
}

size_t dyn_stream_bound(const Geometry &g)
{
    // a literal is at most 15 bits; a match of n >= 3 bytes at most 15 + 5 + 15 + 13 = 48, and where n < 11 the length has
    // no extra bits (n = 3: distance 3 has none either, 30 bits): never more than 15 bits a byte
    const size_t bits = (size_t)ysmr::pngc::HEADER_BITS_MAX + 15 * (size_t)g.H * g.S + 15;
    return ysmr::align_up((bits + 7) / 8 + 6, 4) + 4;
}

// scanline byte (r, c + dc) of the row dr above, wrapped into the row before or after: does it exist and equal v?  |dc| <= 3 < S
__device__ __forceinline__ bool same_as(const uint8_t *__restrict__ rgb, int W, int S, int r, int c, int dr, int dc, uint32_t v)
{
    int rr = r - dr, cc = c + dc;
    if (cc < 0) cc += S, --rr;
    else if (cc >= S) cc -= S, ++rr;
    if (rr < 0) return false;                                // the source lies before the stream
    return (cc ? rgb[(size_t)rr * 3 * W + cc - 1] : 0u) == v;
}

__global__ __launch_bounds__(256) void k_png_dmaps(const uint8_t *__restrict__ rgb, int W, int H, int mask, int row_words, size_t map_words,
                                                   unsigned long long *__restrict__ maps, uint2 *__restrict__ part)
{
    __shared__ uint32_t s_a[4], s_b[4];
    const int S = 1 + 3 * W, r = blockIdx.y, k = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint8_t *row = rgb + (size_t)r * 3 * W;            // scanline byte c > 0 is row[c - 1]
    const unsigned long long n = (unsigned long long)H * S;
    uint32_t a = 0, b = 0;
#pragma unroll
    for (int it = 0; it < PNG_PIECE / 256; ++it) {
        const int c = k * PNG_PIECE + it * 256 + (int)threadIdx.x;
        bool e0 = false, e1 = false, e2 = false, e3 = false;
        if (c < S) {
            const uint32_t v = c ? row[c - 1] : 0u;
            e0 = same_as(rgb, W, S, r, c, 0, -3, v);
            e1 = (mask & 2) && same_as(rgb, W, S, r, c, 1, 0, v);
            e2 = (mask & 4) && same_as(rgb, W, S, r, c, 1, 3, v);
            e3 = (mask & 8) && same_as(rgb, W, S, r, c, 1, -3, v);
            const unsigned long long pos = (unsigned long long)r * S + c;
            a += v;
            b += (uint32_t)((n - pos) % ADLER) * v;          // < 2^24 each, four of them
        }
        const unsigned long long w0 = __ballot(e0), w1 = __ballot(e1), w2 = __ballot(e2), w3 = __ballot(e3);
        const int word = k * (PNG_PIECE / 64) + it * 4 + wave;
        if (lane == 0 && word < row_words) {
            unsigned long long *m = maps + (size_t)r * row_words + word;
            m[0] = w0, m[map_words] = w1, m[2 * map_words] = w2, m[3 * map_words] = w3;
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

struct DynPiece {
    const unsigned long long *m;    // the piece's first word of map 0; map k is map_words * k further
    const uint8_t *row;
    int c0, len;
};

__device__ __forceinline__ DynPiece dyn_piece_at(long long p, const uint8_t *__restrict__ rgb, int W, int row_words, int row_pieces,
                                                 const unsigned long long *__restrict__ maps)
{
    const int S = 1 + 3 * W;
    const long long r = p / row_pieces;
    const int k = (int)(p - r * row_pieces);
    DynPiece q;
    q.m = maps + (size_t)r * row_words + k * (PNG_PIECE / 64);
    q.row = rgb + (size_t)r * 3 * W;
    q.c0 = k * PNG_PIECE;
    q.len = min(PNG_PIECE, S - q.c0);
    return q;
}

// sink.literal(i), sink.match(length, k): k = 0..3 is distance 3, S, S - 3, S + 3
template <typename Sink>
__device__ __forceinline__ void dyn_parse_piece(const unsigned long long *__restrict__ m, size_t map_words, int len, int mask, Sink &sink)
{
    int i = 0;
    while (i < len) {
        const int cap = min(PNG_MAX_MATCH, len - i);
        int best = 0, which = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (!((mask >> k) & 1)) continue;
            const int l = run_of(m + k * map_words, i, cap);
            if (l >= (k ? 4 : 3) && l > best) best = l, which = k;
        }
        if (best) {
            sink.match(best, which);
            i += best;
        } else {
            sink.literal(i);
            ++i;
        }
    }
}

struct HistSink {
    const DynPiece &q;
    uint32_t *hist;                 // LDS
    const int *dist_sym;            // LDS
    __device__ __forceinline__ void literal(int i)
    {
        const int c = q.c0 + i;
        atomicAdd(&hist[c ? q.row[c - 1] : 0u], 1u);
    }
    __device__ __forceinline__ void match(int length, int k)
    {
        int sym, eb, e;
        length_symbol(length, sym, eb, e);
        atomicAdd(&hist[sym], 1u);
        atomicAdd(&hist[ysmr::pngc::N_LITLEN + dist_sym[k]], 1u);
    }
};

__global__ __launch_bounds__(256) void k_png_dhist(const uint8_t *__restrict__ rgb, int W, int row_words, int row_pieces, long long pieces,
                                                   Dist4 d, size_t map_words, const unsigned long long *__restrict__ maps,
                                                   uint32_t *__restrict__ hist)
{
    __shared__ uint32_t s_hist[ysmr::pngc::N_BOTH];
    __shared__ int s_sym[4];
    for (int s = threadIdx.x; s < ysmr::pngc::N_BOTH; s += 256) s_hist[s] = 0;
    if (threadIdx.x == 0) s_sym[0] = d.sym[0], s_sym[1] = d.sym[1], s_sym[2] = d.sym[2], s_sym[3] = d.sym[3];
    __syncthreads();
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    if (p < pieces) {
        const DynPiece q = dyn_piece_at(p, rgb, W, row_words, row_pieces, maps);
        HistSink sink{q, s_hist, s_sym};
        dyn_parse_piece(q.m, map_words, q.len, d.mask, sink);
    }
    __syncthreads();
    for (int s = threadIdx.x; s < ysmr::pngc::N_BOTH; s += 256)
        if (s_hist[s]) atomicAdd(&hist[s], s_hist[s]);
}

// One block.  codes: [0, 316) the tables (reversed code | length << 16), [316] the header's bits, then the header's words.
__global__ __launch_bounds__(256) void k_png_dcodes(const uint32_t *__restrict__ hist, uint32_t *__restrict__ codes)
{
    namespace pc = ysmr::pngc;
    __shared__ pc::Codes c;
    __shared__ int s_used;
    for (int s = threadIdx.x; s < pc::N_BOTH; s += 256) c.counts[s] = hist[s];
    __syncthreads();
    if (threadIdx.x == 0) {
        c.counts[pc::END_OF_BLOCK] += 1;
        pc::force_two(c.counts + pc::N_LITLEN, pc::N_DIST);
        s_used = pc::used_of(c.counts, pc::N_LITLEN);
    }
    __syncthreads();
    const int t = threadIdx.x, m = s_used;                   // m >= 2: a canvas has a literal, and the end of block
    pc::Work &w = c.work;
    // the literal/length alphabet with what is independent per symbol, leaf or length spread over the threads
    // (png_codes.h); on one thread this kernel took 0.43 ms, most of it LDS round trips one after the other
    for (int s = t; s < pc::N_LITLEN; s += 256) {
        c.lengths[s] = 0;
        if (c.counts[s]) w.order[pc::rank_of(c.counts, pc::N_LITLEN, s)] = (uint16_t)s;
    }
    __syncthreads();
    if (m < 2) {
        if (t == 0) pc::lengths_from_order(c.counts, pc::N_LITLEN, m, 15, c.lengths, w);
        __syncthreads();
    } else {
        for (int i = t; i < m; i += 256) pc::leaf_weight(c.counts, i, w);
        __syncthreads();
        if (t == 0) pc::huffman_links(m, w);
        __syncthreads();
        for (int i = t; i < m; i += 256) pc::leaf_depth(m, i, w);
        __syncthreads();
        if (t >= 1 && t <= 15) pc::count_depth(m, 15, t, w);
        __syncthreads();
        if (t == 0) pc::limit_lengths(m, 15, w);
        __syncthreads();
        for (int i = t; i < m; i += 256) pc::assign_length(m, 15, i, c.lengths, w);
        __syncthreads();
    }
    if (t >= 1 && t <= 15) pc::count_code_length(c.lengths, pc::N_LITLEN, t, w);
    __syncthreads();
    if (t == 0) pc::first_codes(w);
    __syncthreads();
    for (int s = t; s < pc::N_LITLEN; s += 256) c.table[s] = pc::canonical_symbol(c.lengths, s, w);
    __syncthreads();
    // the two small alphabets and the header: serial
    if (t == 0) {
        pc::code_lengths(c.counts + pc::N_LITLEN, pc::N_DIST, 15, c.lengths + pc::N_LITLEN, w);
        pc::canonical(c.lengths + pc::N_LITLEN, pc::N_DIST, c.table + pc::N_LITLEN, w);
    }
    __syncthreads();
    if (t == 0) pc::header_tokens(c);
    __syncthreads();
    if (t == 0) pc::header_codes(c);
    __syncthreads();
    if (t == 0) pc::header_bits(c);
    __syncthreads();
    for (int s = threadIdx.x; s < pc::N_BOTH; s += 256) codes[s] = c.table[s];
    for (int s = threadIdx.x; s < pc::HEADER_WORDS; s += 256) codes[pc::N_BOTH + 1 + s] = c.header[s];
    if (threadIdx.x == 0) codes[pc::N_BOTH] = c.header_bits;
}

struct DynCountSink {
    const DynPiece &q;
    const uint8_t *len_of;          // LDS: the 316 code lengths
    const int *dist_bits;           // LDS: a distance's code length + extra bits
    uint32_t bits;
    __device__ __forceinline__ void literal(int i)
    {
        const int c = q.c0 + i;
        bits += len_of[c ? q.row[c - 1] : 0u];
    }
    __device__ __forceinline__ void match(int length, int k)
    {
        int sym, eb, e;
        length_symbol(length, sym, eb, e);
        bits += (uint32_t)len_of[sym] + (uint32_t)eb + (uint32_t)dist_bits[k];
    }
};

__global__ __launch_bounds__(256) void k_png_dsize(const uint8_t *__restrict__ rgb, int W, int row_words, int row_pieces, long long pieces,
                                                   Dist4 d, size_t map_words, const unsigned long long *__restrict__ maps,
                                                   const uint32_t *__restrict__ codes, uint32_t *__restrict__ piece_off,
                                                   unsigned long long *__restrict__ block_tot)
{
    __shared__ uint8_t s_len[ysmr::pngc::N_BOTH];
    __shared__ int s_dist[4];
    __shared__ uint32_t s_wave[4];
    for (int s = threadIdx.x; s < ysmr::pngc::N_BOTH; s += 256) s_len[s] = (uint8_t)(codes[s] >> 16);
    __syncthreads();
    if (threadIdx.x == 0) {
        s_dist[0] = s_len[ysmr::pngc::N_LITLEN + d.sym[0]] + d.extra_bits[0];
        s_dist[1] = s_len[ysmr::pngc::N_LITLEN + d.sym[1]] + d.extra_bits[1];
        s_dist[2] = s_len[ysmr::pngc::N_LITLEN + d.sym[2]] + d.extra_bits[2];
        s_dist[3] = s_len[ysmr::pngc::N_LITLEN + d.sym[3]] + d.extra_bits[3];
    }
    __syncthreads();
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    uint32_t mine = 0;
    if (p < pieces) {
        const DynPiece q = dyn_piece_at(p, rgb, W, row_words, row_pieces, maps);
        DynCountSink sink{q, s_len, s_dist, 0u};
        dyn_parse_piece(q.m, map_words, q.len, d.mask, sink);
        mine = sink.bits;                                    // <= 15 * PNG_PIECE
    }
    const uint32_t incl = ysmr::prim::wave_inclusive_sum(mine);
    if ((threadIdx.x & 63) == 63) s_wave[threadIdx.x >> 6] = incl;
    __syncthreads();
    uint32_t before = incl - mine;
    for (int w = 0; w < (int)(threadIdx.x >> 6); ++w) before += s_wave[w];
    if (p < pieces) piece_off[p] = before;
    if (threadIdx.x == 255) block_tot[blockIdx.x] = (unsigned long long)before + mine;
}

// One block, as k_png_finish; the header's words go behind the two zlib bytes, the end-of-block code behind the last piece.
__global__ __launch_bounds__(256) void k_png_dfinish(unsigned long long *__restrict__ block_tot, long long blocks, const uint2 *__restrict__ part,
                                                     long long pieces, unsigned long long n_bytes, const uint32_t *__restrict__ codes,
                                                     uint32_t *__restrict__ out, unsigned long long *__restrict__ out_len)
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
    if (t < ysmr::pngc::HEADER_WORDS) {                      // header bit j is stream bit 16 + j
        const uint32_t w = codes[ysmr::pngc::N_BOTH + 1 + t];
        if (w << 16) atomicOr(&out[t], w << 16);
        if (w >> 16) atomicOr(&out[t + 1], w >> 16);
    }
    if (t == 255) {                                          // `before` is the total now
        a = 1, b = n_bytes % ADLER;
        for (int k = 0; k < 256; ++k) a += s_a[k], b += s_b[k];
        a %= ADLER, b %= ADLER;
        const uint32_t eob = codes[ysmr::pngc::END_OF_BLOCK];
        const unsigned long long eob_at = 16 + codes[ysmr::pngc::N_BOTH] + before;
        const unsigned long long v = (unsigned long long)(eob & 0xFFFFu) << (eob_at & 31);
        atomicOr(&out[eob_at >> 5], (uint32_t)v);
        if (v >> 32) atomicOr(&out[(eob_at >> 5) + 1], (uint32_t)(v >> 32));
        const unsigned long long tail = (eob_at + (eob >> 16) + 7) >> 3;
        atomicOr(&out[0], 0x78u | 0x01u << 8);
        or_byte(out, tail, (uint32_t)(b >> 8));
        or_byte(out, tail + 1, (uint32_t)(b & 255));
        or_byte(out, tail + 2, (uint32_t)(a >> 8));
        or_byte(out, tail + 3, (uint32_t)(a & 255));
        *out_len = tail + 4;
    }
}

struct DynEmitSink {
    const DynPiece &q;
    uint32_t *out;
    const uint32_t *table;          // LDS: reversed code | length << 16
    const uint2 *dist;              // LDS: a distance's reversed code with its extra bits above, the number of bits
    unsigned long long word;        // of the next store
    int fill;                       // bits waiting in acc, < 32 between calls
    bool shared;                    // the next word stored may hold a neighbour's bits
    unsigned long long acc;
    __device__ __forceinline__ void put(uint32_t bits, int len)     // len <= 31
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
    __device__ __forceinline__ void literal(int i)
    {
        const int c = q.c0 + i;
        const uint32_t e = table[c ? q.row[c - 1] : 0u];
        put(e & 0xFFFFu, (int)(e >> 16));
    }
    __device__ __forceinline__ void match(int length, int k)
    {
        int sym, eb, ex;
        length_symbol(length, sym, eb, ex);
        const uint32_t e = table[sym];
        const int len = (int)(e >> 16);
        put((e & 0xFFFFu) | (uint32_t)ex << len, len + eb);  // <= 15 + 5 bits
        const uint2 dd = dist[k];
        put(dd.x, (int)dd.y);                                // <= 15 + 13 bits
    }
    __device__ __forceinline__ void flush()
    {
        if (fill > 0) atomicOr(&out[word], (uint32_t)acc);
    }
};

__global__ __launch_bounds__(256) void k_png_demit(const uint8_t *__restrict__ rgb, int W, int row_words, int row_pieces, long long pieces,
                                                   Dist4 d, size_t map_words, const unsigned long long *__restrict__ maps,
                                                   const uint32_t *__restrict__ codes, const uint32_t *__restrict__ piece_off,
                                                   const unsigned long long *__restrict__ block_pre, uint32_t *__restrict__ out)
{
    __shared__ uint32_t s_table[ysmr::pngc::N_BOTH];
    __shared__ uint2 s_dist[4];
    for (int s = threadIdx.x; s < ysmr::pngc::N_BOTH; s += 256) s_table[s] = codes[s];
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t e;
        e = s_table[ysmr::pngc::N_LITLEN + d.sym[0]], s_dist[0] = make_uint2((e & 0xFFFFu) | (uint32_t)d.extra[0] << (e >> 16), (e >> 16) + d.extra_bits[0]);
        e = s_table[ysmr::pngc::N_LITLEN + d.sym[1]], s_dist[1] = make_uint2((e & 0xFFFFu) | (uint32_t)d.extra[1] << (e >> 16), (e >> 16) + d.extra_bits[1]);
        e = s_table[ysmr::pngc::N_LITLEN + d.sym[2]], s_dist[2] = make_uint2((e & 0xFFFFu) | (uint32_t)d.extra[2] << (e >> 16), (e >> 16) + d.extra_bits[2]);
        e = s_table[ysmr::pngc::N_LITLEN + d.sym[3]], s_dist[3] = make_uint2((e & 0xFFFFu) | (uint32_t)d.extra[3] << (e >> 16), (e >> 16) + d.extra_bits[3]);
    }
    __syncthreads();
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    if (p >= pieces) return;
    const DynPiece q = dyn_piece_at(p, rgb, W, row_words, row_pieces, maps);
    const unsigned long long start = 16 + codes[ysmr::pngc::N_BOTH] + block_pre[blockIdx.x] + piece_off[p];
    DynEmitSink sink{q, out, s_table, s_dist, start >> 5, (int)(start & 31), true, 0ull};
    dyn_parse_piece(q.m, map_words, q.len, d.mask, sink);
    sink.flush();
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

size_t ysmr_png_dynamic_workspace_bytes(int width, int height)
{
    if (width < 1 || height < 1 || width > PNG_MAX_SIDE || height > PNG_MAX_SIDE) return 0;
    return dyn_layout(geometry(width, height)).bytes;
}

size_t ysmr_png_dynamic_stream_bytes_max(int width, int height)
{
    if (width < 1 || height < 1 || width > PNG_MAX_SIDE || height > PNG_MAX_SIDE) return 0;
    return dyn_stream_bound(geometry(width, height));
}

int ysmr_png_deflate_dynamic(void *stream, const uint8_t *rgb_dev, int width, int height, void *workspace_dev, size_t workspace_bytes,
                             uint8_t *out_dev, size_t out_bytes, unsigned long long *out_len_dev)
{
    if (int rc = check_canvas(width, height)) return rc;
    const Geometry g = geometry(width, height);
    const DynLayout l = dyn_layout(g);
    const Dist4 d = distances(g);
    const size_t bound = dyn_stream_bound(g);
    if (!rgb_dev || !workspace_dev || !out_dev || !out_len_dev)
        return ysmr::fail(YSMR_ERR_ARG, "rgb_dev, workspace_dev, out_dev and out_len_dev must not be NULL");
    if (workspace_bytes < l.bytes) return ysmr::fail(YSMR_ERR_ARG, "the workspace holds %zu bytes, %zu are needed", workspace_bytes, l.bytes);
    if (out_bytes < bound) return ysmr::fail(YSMR_ERR_ARG, "the output holds %zu bytes, ysmr_png_dynamic_stream_bytes_max is %zu", out_bytes, bound);
    if (((uintptr_t)workspace_dev & 7) || ((uintptr_t)out_dev & 3) || ((uintptr_t)out_len_dev & 7))
        return ysmr::fail(YSMR_ERR_ARG, "workspace_dev and out_len_dev must be 8-byte aligned, out_dev 4-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    char *ws = (char *)workspace_dev;
    unsigned long long *maps = (unsigned long long *)(ws + l.maps), *tot = (unsigned long long *)(ws + l.tot);
    uint2 *part = (uint2 *)(ws + l.part);
    uint32_t *off = (uint32_t *)(ws + l.off), *hist = (uint32_t *)(ws + l.hist), *codes = (uint32_t *)(ws + l.codes), *out = (uint32_t *)out_dev;
    YSMR_HIP_CHECK(hipMemsetAsync(out_dev, 0, bound, st));   // the whole bound: every word of the stream is OR-ed or stored into zeros
    YSMR_HIP_CHECK(hipMemsetAsync(hist, 0, (size_t)ysmr::pngc::N_BOTH * 4, st));
    const dim3 per_piece((unsigned)g.blocks), block(256);
    hipLaunchKernelGGL(k_png_dmaps, dim3((unsigned)g.row_pieces, (unsigned)g.H), block, 0, st, rgb_dev, g.W, g.H, d.mask, g.row_words, l.map_words, maps, part);
    hipLaunchKernelGGL(k_png_dhist, per_piece, block, 0, st, rgb_dev, g.W, g.row_words, g.row_pieces, g.pieces, d, l.map_words, maps, hist);
    hipLaunchKernelGGL(k_png_dcodes, dim3(1), block, 0, st, hist, codes);
    hipLaunchKernelGGL(k_png_dsize, per_piece, block, 0, st, rgb_dev, g.W, g.row_words, g.row_pieces, g.pieces, d, l.map_words, maps, codes, off, tot);
    hipLaunchKernelGGL(k_png_dfinish, dim3(1), block, 0, st, tot, g.blocks, part, g.pieces, (unsigned long long)g.H * g.S, codes, out, out_len_dev);
    hipLaunchKernelGGL(k_png_demit, per_piece, block, 0, st, rgb_dev, g.W, g.row_words, g.row_pieces, g.pieces, d, l.map_words, maps, codes, off, tot, out);
    YSMR_LAUNCH_CHECK();
    return YSMR_OK;
}

int ysmr_png_code_lengths(const uint32_t *counts, int n_symbols, int max_bits, uint8_t *lengths_out)
{
    if (!counts || !lengths_out) return ysmr::fail(YSMR_ERR_ARG, "counts and lengths_out must not be NULL");
    if (n_symbols < 1 || n_symbols > ysmr::pngc::MAX_SYMBOLS) return ysmr::fail(YSMR_ERR_ARG, "n_symbols must be in 1..288, got %d", n_symbols);
    if (max_bits < 1 || max_bits > 15) return ysmr::fail(YSMR_ERR_ARG, "max_bits must be in 1..15, got %d", max_bits);
    ysmr::pngc::Work work;
    if (!ysmr::pngc::code_lengths(counts, n_symbols, max_bits, lengths_out, work))
        return ysmr::fail(YSMR_ERR_ARG, "%d used symbols cannot have codes of at most %d bits", ysmr::pngc::used_of(counts, n_symbols), max_bits);
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

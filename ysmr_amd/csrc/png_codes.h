// The Huffman codes of ysmr_png_deflate_dynamic (png.hip), written once for the host and the device: the length-limited code
// lengths of a histogram, the canonical codes (RFC 1951, 3.2.2) and the block's header (3.2.7).  A plain C++ compiler takes
// this header as it is (YSMR_HD, hd.h); the kernel k_png_dcodes and the host export ysmr_png_code_lengths call the same text.
//
// Code lengths, for a histogram counts[0..n) and a limit max_bits (tests/png_dynamic_model.py restates every step):
//   1. the used symbols (count > 0) in ascending order of (count, symbol): rank_of, a symbol's place, is independent of the
//      others' -- a kernel computes the ranks a thread per symbol;
//   2. none used: all lengths 0; one used: its length is 1;
//   3. Huffman's tree by the two-queue method: the sorted leaves are one queue, the internal nodes in the order they were made
//      the other (their weights never fall); the lighter head is taken, the LEAF on a tie; 64-bit weights;
//   4. a leaf deeper than max_bits counts as one of depth max_bits; while the Kraft sum, in units of 2^-max_bits, exceeds
//      2^max_bits: one code of length max_bits is taken away, the longest length i < max_bits that has a code gives one up, and
//      two codes of length i + 1 are added -- the sum falls by exactly one unit, so there are fewer rounds than symbols;
//   5. the lengths are handed out from the shortest on, to the symbols in DESCENDING order of (count, symbol).
// Where no leaf is deeper than max_bits, step 4 does nothing and step 5 gives Huffman's multiset of lengths to the symbols in
// order of weight: the total cost is the optimum.  Every loop is bounded by the alphabet's size or by max_bits.
//
// Nothing here keeps an array in a local variable: all of them live in the caller's Work / Codes, which a kernel puts in LDS.
// No loop is unrolled: this is serial work of a few hundred steps on one thread, and unrolled it cost k_png_dcodes ten
// thousand instructions and spilled scalar registers.
#pragma once
#include <stdint.h>

#include "hd.h"

namespace ysmr {
namespace pngc {

constexpr int MAX_SYMBOLS = 288;
constexpr int N_LITLEN = 286, N_DIST = 30, N_CLEN = 19, N_BOTH = N_LITLEN + N_DIST;
constexpr int END_OF_BLOCK = 256;
constexpr int HEADER_BITS_MAX = 3 + 5 + 5 + 4 + 3 * N_CLEN + N_BOTH * (7 + 7);      // 4498
constexpr int HEADER_WORDS = (HEADER_BITS_MAX + 31) / 32 + 1;                         // 142

struct Work {
    unsigned long long weight[2 * MAX_SYMBOLS];     // the leaves in order, then the internal nodes as they are made
    uint16_t link[2 * MAX_SYMBOLS];                 // a node's parent
    uint16_t order[MAX_SYMBOLS];                    // the used symbols, ascending by (count, symbol)
    uint16_t depth[MAX_SYMBOLS];                    // of the leaves
    uint32_t num[17];                               // codes per length (1 .. 16: mjpeg.hip limits its codes to 16 bits)
    uint32_t next[17];                              // the codes of at most that length; canonical: a length's first code
};

YSMR_HD_FORCE int used_of(const uint32_t *counts, int n)
{
    int m = 0;
#pragma nounroll
    for (int s = 0; s < n; ++s) m += counts[s] != 0;
    return m;
}

// the place of the used symbol s among the used symbols
YSMR_HD_FORCE int rank_of(const uint32_t *counts, int n, int s)
{
    const uint32_t c = counts[s];
    int r = 0;
#pragma nounroll
    for (int t = 0; t < n; ++t) {
        const uint32_t ct = counts[t];
        r += ct != 0 && (ct < c || (ct == c && t < s));
    }
    return r;
}

// Steps 3 to 5 in pieces: what is independent per leaf or per length is a function of that leaf or length -- a kernel
// gives each to a thread, with a barrier between the pieces --, and only Huffman's merging and the repair are serial.
// lengths_from_order below runs the pieces one after the other.

YSMR_HD_FORCE void leaf_weight(const uint32_t *counts, int i, Work &w) { w.weight[i] = counts[w.order[i]]; }

// serial: the tree over the m >= 2 sorted leaves; w.link becomes every node's parent, the root is node 2 m - 2
YSMR_HD_FORCE void huffman_links(int m, Work &w)
{
    int leaf = 0, node = m;
#pragma nounroll
    for (int made = m; made < 2 * m - 1; ++made) {
        unsigned long long sum = 0;
#pragma nounroll
        for (int k = 0; k < 2; ++k) {
            const bool take_leaf = leaf < m && (node >= made || w.weight[leaf] <= w.weight[node]);
            const int at = take_leaf ? leaf++ : node++;
            sum += w.weight[at];
            w.link[at] = (uint16_t)made;
        }
        w.weight[made] = sum;
    }
}

// leaf i's depth: the parents up to the root (a parent's index is larger, so at most 2 m steps)
YSMR_HD_FORCE void leaf_depth(int m, int i, Work &w)
{
    int k = i, d = 0;
#pragma nounroll
    for (int step = 0; step < 2 * m && k != 2 * m - 2; ++step) {
        k = w.link[k];
        ++d;
    }
    w.depth[i] = (uint16_t)d;
}

// the leaves whose depth, counted as max_bits where it is deeper, is `len`
YSMR_HD_FORCE void count_depth(int m, int max_bits, int len, Work &w)
{
    uint32_t c = 0;
#pragma nounroll
    for (int i = 0; i < m; ++i) c += (w.depth[i] < max_bits ? w.depth[i] : max_bits) == len;
    w.num[len] = c;
}

// serial: step 4's repair of w.num[1 .. max_bits]; then w.next[len] = the codes of at most len bits
YSMR_HD_FORCE void limit_lengths(int m, int max_bits, Work &w)
{
    uint32_t total = 0;
#pragma nounroll
    for (int i = 1; i <= max_bits; ++i) total += w.num[i] << (max_bits - i);
#pragma nounroll
    for (int round = 0; round < m && total > (1u << max_bits); ++round) {
        int from = 0;
#pragma nounroll
        for (int i = max_bits - 1; i >= 1 && !from; --i)
            if (w.num[i]) from = i;
        if (!from || !w.num[max_bits]) break;                 // cannot happen while m <= 2^max_bits; keeps the loop bounded regardless
        w.num[max_bits] -= 1;
        w.num[from] -= 1;
        w.num[from + 1] += 2;
        total -= 1;
    }
    uint32_t upto = 0;
    w.next[0] = 0;
#pragma nounroll
    for (int len = 1; len <= max_bits; ++len) w.next[len] = upto += w.num[len];
}

// step 5 for leaf i: the p-th symbol from the heavy end, p = m - 1 - i, has the shortest length whose w.next exceeds p
YSMR_HD_FORCE void assign_length(int m, int max_bits, int i, uint8_t *lengths, Work &w)
{
    const uint32_t p = (uint32_t)(m - 1 - i);
    int len = 1;
#pragma nounroll
    for (; len < max_bits && w.next[len] <= p; ++len) {}
    lengths[w.order[i]] = (uint8_t)len;
}

// steps 2 to 5; w.order holds the m used symbols.  False (and all lengths 0) if m symbols cannot have codes of max_bits bits.
YSMR_HD_FORCE bool lengths_from_order(const uint32_t *counts, int n, int m, int max_bits, uint8_t *lengths, Work &w)
{
#pragma nounroll
    for (int s = 0; s < n; ++s) lengths[s] = 0;
    if (m == 0) return true;
    if (m == 1) {
        lengths[w.order[0]] = 1;
        return true;
    }
    if (m > (1 << max_bits)) return false;
#pragma nounroll
    for (int i = 0; i < m; ++i) leaf_weight(counts, i, w);
    huffman_links(m, w);
#pragma nounroll
    for (int i = 0; i < m; ++i) leaf_depth(m, i, w);
#pragma nounroll
    for (int len = 1; len <= max_bits; ++len) count_depth(m, max_bits, len, w);
    limit_lengths(m, max_bits, w);
#pragma nounroll
    for (int i = 0; i < m; ++i) assign_length(m, max_bits, i, lengths, w);
    return true;
}

// all five steps on one thread
YSMR_HD_FORCE bool code_lengths(const uint32_t *counts, int n, int max_bits, uint8_t *lengths, Work &w)
{
    int m = 0;
#pragma nounroll
    for (int s = 0; s < n; ++s)
        if (counts[s]) {
            w.order[rank_of(counts, n, s)] = (uint16_t)s;
            ++m;
        }
    return lengths_from_order(counts, n, m, max_bits, lengths, w);
}

// As zlib does, the distance alphabet always has two codes: while fewer than two symbols are used, the lowest unused one
// gets the count 1.
YSMR_HD_FORCE void force_two(uint32_t *counts, int n)
{
    int m = used_of(counts, n);
#pragma nounroll
    for (int s = 0; s < n && m < 2; ++s)
        if (!counts[s]) {
            counts[s] = 1;
            ++m;
        }
}

YSMR_HD_FORCE uint32_t reverse_bits(uint32_t code, int len)
{
#ifdef __HIP_DEVICE_COMPILE__
    return __brev(code) >> (32 - len);                       // len >= 1
#else
    uint32_t r = 0;
    for (int k = 0; k < len; ++k) r |= ((code >> k) & 1u) << (len - 1 - k);
    return r;
#endif
}

// The canonical codes (RFC 1951, 3.2.2), in pieces as above: the symbols of a length, per length; the first code of every
// length, serial; a symbol's code, per symbol.
YSMR_HD_FORCE void count_code_length(const uint8_t *lengths, int n, int len, Work &w)
{
    uint32_t c = 0;
#pragma nounroll
    for (int s = 0; s < n; ++s) c += lengths[s] == len;
    w.num[len] = c;
}

YSMR_HD_FORCE void first_codes(Work &w)
{
    uint32_t code = 0;
    w.num[0] = 0;
    w.next[0] = 0;
#pragma nounroll
    for (int len = 1; len <= 15; ++len) {
        code = (code + w.num[len - 1]) << 1;
        w.next[len] = code;
    }
}

// the code of symbol s, bit-reversed for a packer that fills bytes from bit 0, | its length << 16; 0 for an unused symbol
YSMR_HD_FORCE uint32_t canonical_symbol(const uint8_t *lengths, int s, const Work &w)
{
    const int len = lengths[s];
    if (!len) return 0u;
    uint32_t earlier = 0;
#pragma nounroll
    for (int t = 0; t < s; ++t) earlier += lengths[t] == len;
    return reverse_bits(w.next[len] + earlier, len) | (uint32_t)len << 16;
}

YSMR_HD_FORCE void canonical(const uint8_t *lengths, int n, uint32_t *table, Work &w)
{
#pragma nounroll
    for (int len = 1; len <= 15; ++len) count_code_length(lengths, n, len, w);
    first_codes(w);
#pragma nounroll
    for (int s = 0; s < n; ++s) table[s] = canonical_symbol(lengths, s, w);
}

// Everything the block needs, built from the two histograms.
struct Codes {
    uint32_t counts[N_BOTH];        // in: literal/length symbols (the end of block NOT yet counted), then distances
    uint8_t lengths[N_BOTH];
    uint32_t table[N_BOTH];         // canonical()
    uint16_t token[N_BOTH];         // the header's run-length symbols: symbol | extra bits' value << 5
    uint32_t cl_counts[N_CLEN];
    uint8_t cl_lengths[N_CLEN];
    uint32_t cl_table[N_CLEN];
    uint32_t header[HEADER_WORDS];  // BFINAL, BTYPE, HLIT, HDIST, HCLEN, the code-length code, the two length sequences
    uint32_t header_bits;
    int n_lit, n_dist, n_token;     // HLIT + 257, HDIST + 1, the run-length symbols
    Work work;
};

YSMR_HD_FORCE void put_bits(uint32_t *words, uint32_t &at, uint32_t value, int len)      // len <= 16
{
    const uint32_t sh = at & 31;
    words[at >> 5] |= value << sh;
    if (sh + (uint32_t)len > 32) words[(at >> 5) + 1] |= value >> (32 - sh);
    at += (uint32_t)len;
}

YSMR_HD_FORCE int cl_order(int k)     // RFC 1951, 3.2.7: 16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15
{
    if (k < 3) return 16 + k;
    if (k == 3) return 0;
    const int j = k - 4;
    return (j & 1) ? 8 - (j + 1) / 2 : 8 + j / 2;
}

// The header.  c.lengths is complete.  The two length sequences, HLIT + 257 and HDIST + 1 long, are run-length coded as ONE
// sequence, run by run of equal values: a run of r zeros is 18 (up to 138 zeros) while r >= 11, then 17 if r >= 3, then
// single zeros; a run of r lengths v > 0 is v once, then 16 (up to 6 repeats) while r >= 3 remain, then single v's.
// (Three steps, so that a kernel can put barriers between them: each stays small enough to need no spilled register.)
YSMR_HD_FORCE void header_tokens(Codes &c)
{
    int n_lit = N_LITLEN, n_dist = N_DIST;
#pragma nounroll
    while (n_lit > 257 && !c.lengths[n_lit - 1]) --n_lit;
#pragma nounroll
    while (n_dist > 1 && !c.lengths[N_LITLEN + n_dist - 1]) --n_dist;
    const int total = n_lit + n_dist;
    int n_tok = 0;
#pragma nounroll
    for (int k = 0; k < N_CLEN; ++k) c.cl_counts[k] = 0;
    int i = 0;
#pragma nounroll
    while (i < total) {                                       // every round consumes at least one entry
        const int v = c.lengths[i < n_lit ? i : N_LITLEN + i - n_lit];
        int r = 1;
#pragma nounroll
        while (i + r < total && c.lengths[i + r < n_lit ? i + r : N_LITLEN + i + r - n_lit] == v) ++r;
        i += r;
        if (v == 0) {
#pragma nounroll
            while (r >= 11) {
                const int k = r < 138 ? r : 138;
                c.token[n_tok++] = (uint16_t)(18 | (k - 11) << 5);
                r -= k;
            }
            if (r >= 3) {
                c.token[n_tok++] = (uint16_t)(17 | (r - 3) << 5);
                r = 0;
            }
        } else {
            c.token[n_tok++] = (uint16_t)v;
            --r;
#pragma nounroll
            while (r >= 3) {
                const int k = r < 6 ? r : 6;
                c.token[n_tok++] = (uint16_t)(16 | (k - 3) << 5);
                r -= k;
            }
        }
#pragma nounroll
        for (; r > 0; --r) c.token[n_tok++] = (uint16_t)v;
    }
#pragma nounroll
    for (int k = 0; k < n_tok; ++k) c.cl_counts[c.token[k] & 31] += 1;
    c.n_lit = n_lit, c.n_dist = n_dist, c.n_token = n_tok;
}

YSMR_HD_FORCE void header_codes(Codes &c)
{
    code_lengths(c.cl_counts, N_CLEN, 7, c.cl_lengths, c.work);
    canonical(c.cl_lengths, N_CLEN, c.cl_table, c.work);
}

YSMR_HD_FORCE void header_bits(Codes &c)
{
    const int n_lit = c.n_lit, n_dist = c.n_dist, n_tok = c.n_token;
    int n_cl = N_CLEN;
#pragma nounroll
    while (n_cl > 4 && !c.cl_lengths[cl_order(n_cl - 1)]) --n_cl;
#pragma nounroll
    for (int k = 0; k < HEADER_WORDS; ++k) c.header[k] = 0;
    uint32_t at = 0;
    put_bits(c.header, at, 1u | 2u << 1, 3);                  // BFINAL = 1, BTYPE = 10 with its low bit first
    put_bits(c.header, at, (uint32_t)(n_lit - 257), 5);
    put_bits(c.header, at, (uint32_t)(n_dist - 1), 5);
    put_bits(c.header, at, (uint32_t)(n_cl - 4), 4);
#pragma nounroll
    for (int k = 0; k < n_cl; ++k) put_bits(c.header, at, c.cl_lengths[cl_order(k)], 3);
#pragma nounroll
    for (int k = 0; k < n_tok; ++k) {
        const int sym = c.token[k] & 31, extra = c.token[k] >> 5;
        const uint32_t e = c.cl_table[sym];
        put_bits(c.header, at, e & 0xFFFFu, (int)(e >> 16));
        if (sym == 16) put_bits(c.header, at, (uint32_t)extra, 2);
        else if (sym == 17) put_bits(c.header, at, (uint32_t)extra, 3);
        else if (sym == 18) put_bits(c.header, at, (uint32_t)extra, 7);
    }
    c.header_bits = at;
}

// From c.counts (the end of block counted, force_two applied) to lengths, tables and header on ONE thread, the literal/length
// alphabet's sorted order in c.work.order already (m_lit symbols).  k_png_dcodes does the same with the pieces above spread
// over a workgroup; this is what a host program calls.
YSMR_HD_FORCE void build_codes(Codes &c, int m_lit)
{
    lengths_from_order(c.counts, N_LITLEN, m_lit, 15, c.lengths, c.work);
    code_lengths(c.counts + N_LITLEN, N_DIST, 15, c.lengths + N_LITLEN, c.work);
    canonical(c.lengths, N_LITLEN, c.table, c.work);
    canonical(c.lengths + N_LITLEN, N_DIST, c.table + N_LITLEN, c.work);
    header_tokens(c);
    header_codes(c);
    header_bits(c);
}

}  // namespace pngc
}  // namespace ysmr

// inflate_core.h -- the serial part of a raw DEFLATE decoder (RFC 1951), shared by the device kernel (kernel_inflate.hip, one lane of a wavefront runs it)
// and by the host model (host_check.cpp: hlala_host_inflate_model).  Written from the RFC: bit order (3.1.1), block header and stored blocks (3.2.3, 3.2.4),
// the length / distance alphabets (3.2.5), the fixed code (3.2.6), the dynamic code lengths (3.2.7) and the canonical code assignment (3.2.2).
//
// What it promises for ANY input bytes:
//   * it reads input through InfBits only, which never touches a byte at or beyond `n` (bits past the end read as zero and are counted: consuming one is
//     HLALA_INFLATE_INPUT_EXHAUSTED at the next check);
//   * every table index is masked (primary tables) or compared against the table's size (sorted symbol lists);
//   * every loop runs over a fixed range or consumes input bits, so the number of steps is bounded by 8 * n;
//   * it writes no output itself: a token says what to write, the caller (which knows how many bytes it has produced) checks distance and size.
//
// A Huffman code is held as a primary table over the next INF_ROOT bits (one 16-bit entry: symbol + code length) plus, for the codes longer than that, the
// canonical description of the RFC (per length: first code and count; the symbols sorted by code): a long code is found by reading on bit by bit.  BGZF blocks
// written by zlib / htslib rarely hold literal codes beyond 9 bits; full second-level tables would take 5.7 KB of LDS per wavefront against 2.9 KB here.
#ifndef HLALA_INFLATE_CORE_H_
#define HLALA_INFLATE_CORE_H_
#include <stdint.h>

#include "../../include/hlala_gpu.h"

#if defined(__HIPCC__)
#define HLALA_HD __host__ __device__ inline
#else
#define HLALA_HD inline
#endif

namespace hlala_inflate {

constexpr int INF_ROOT = 9;                       // bits of the primary tables
constexpr int INF_MAXBITS = 15;                   // longest code (RFC 3.2.7)
constexpr int INF_NLIT = 288, INF_NDIST = 32;     // alphabet sizes of the fixed code; a dynamic block sends at most 286 / 30 lengths
// results of token(): a status (>= 0, HLALA_INFLATE_*) or one of these
constexpr int INF_TOKEN = -1;                     // *tok holds a literal (< 256) or (length << 16 | distance)
constexpr int INF_END_OF_BLOCK = -2;

// ---- bit reader.  Byte `i` of the stream is p[(i - base) & mask]: the host reads the stream itself (base 0, mask all ones); the kernel reads a window of the
// stream staged in LDS (base = first byte of the window, mask = window size - 1, so that no index leaves the window whatever the stream says).
struct InfBits {
    const uint8_t* p; uint32_t n, base, mask;
    uint32_t pos;          // next byte of the stream to load
    uint32_t cnt, pad;     // bits held in buf; how many of them (the topmost) lie beyond the end of the stream
    uint64_t buf;
};
HLALA_HD void bits_init(InfBits& b, const uint8_t* p, uint32_t n, uint32_t base, uint32_t mask, uint64_t bit_offset)
{
    b.p = p; b.n = n; b.base = base; b.mask = mask; b.buf = 0; b.cnt = 0; b.pad = 0;
    const uint64_t byte = bit_offset >> 3;
    b.pos = byte < (uint64_t)n ? (uint32_t)byte : n;
    const uint32_t skip = (uint32_t)(bit_offset & 7);
    if(skip && b.pos < n) { b.buf = (uint64_t)(b.p[(b.pos - base) & mask] >> skip); b.cnt = 8 - skip; b.pos++; }
}
// at least k (<= 32) bits in buf
HLALA_HD void bits_need(InfBits& b, uint32_t k)
{
    while(b.cnt < k) {            // (at most four rounds: every round adds eight bits)
        if(b.pos < b.n) { b.buf |= (uint64_t)b.p[(b.pos - b.base) & b.mask] << b.cnt; b.pos++; }
        else b.pad += 8;
        b.cnt += 8;
    }
}
HLALA_HD uint32_t bits_peek(const InfBits& b, uint32_t k) { return (uint32_t)b.buf & ((1u << k) - 1u); }
HLALA_HD void bits_drop(InfBits& b, uint32_t k) { b.buf >>= k; b.cnt -= k; }
HLALA_HD uint32_t bits_get(InfBits& b, uint32_t k) { bits_need(b, k); const uint32_t v = bits_peek(b, k); bits_drop(b, k); return v; }
HLALA_HD bool bits_overrun(const InfBits& b) { return b.cnt < b.pad; }                    // a bit beyond the end of the stream has been consumed
HLALA_HD uint64_t bits_consumed(const InfBits& b) { return (uint64_t)b.pos * 8u + b.pad - b.cnt; }      // bit offset of the next unread bit (meaningful while !bits_overrun)

// ---- one Huffman code
struct InfCode {
    uint16_t tab[1 << INF_ROOT];            // indexed by the next INF_ROOT bits: symbol | length << 9 for codes of at most INF_ROOT bits, 0 = look further
    uint16_t first[INF_MAXBITS + 1];        // per length: the first code of that length (RFC 3.2.2, next_code) ...
    uint16_t count[INF_MAXBITS + 1];        // ... how many codes have it ...
    uint16_t index[INF_MAXBITS + 1];        // ... and where their symbols start in sym
};
struct InfTables {
    InfCode lit, dist;
    uint16_t litSym[INF_NLIT], distSym[INF_NDIST];      // symbols sorted by (code length, symbol) = by code
    uint8_t lens[INF_NLIT + INF_NDIST];                 // code lengths of a dynamic block while they are read
};

HLALA_HD uint32_t bit_reverse(uint32_t code, int len) { uint32_t r = 0; for(int i = 0; i < len; i++) { r = (r << 1) | (code & 1u); code >>= 1; } return r; }

// The canonical code of lens[0 .. n) (n <= symCap).  Returns false for an over-subscribed set and for an incomplete one, except -- allowOne -- the code of
// exactly one symbol of length 1, and -- allowNone -- no code at all; what such a code leaves unused decodes as an invalid symbol.
HLALA_HD bool build_code(const uint8_t* lens, int n, InfCode& c, uint16_t* sym, int symCap, bool allowOne, bool allowNone)
{
    for(int l = 0; l <= INF_MAXBITS; l++) c.count[l] = 0;
    for(int s = 0; s < n; s++) c.count[lens[s] & 15]++;
    const int used = n - c.count[0];
    c.count[0] = 0;
    int left = 1;
    for(int l = 1; l <= INF_MAXBITS; l++) { left = left * 2 - (int)c.count[l]; if(left < 0) return false; }
    if(left > 0) {
        const bool one = used == 1 && c.count[1] == 1;
        if(!((one && allowOne) || (used == 0 && allowNone))) return false;
    }
    uint32_t code = 0, idx = 0;
    c.first[0] = 0; c.index[0] = 0;
    for(int l = 1; l <= INF_MAXBITS; l++) { code = (code + c.count[l - 1]) << 1; c.first[l] = (uint16_t)code; c.index[l] = (uint16_t)idx; idx += c.count[l]; }
    for(int i = 0; i < (1 << INF_ROOT); i++) c.tab[i] = 0;
    // (first / index run along as the next code and the next place of every length, and are set back afterwards: no private arrays, which on the device are scratch memory)
    for(int s = 0; s < n; s++) {
        const int l = lens[s] & 15;
        if(l == 0) continue;
        const uint32_t cd = c.first[l]++;
        const uint32_t k = c.index[l]++;
        if((int)k < symCap) sym[k] = (uint16_t)s;
        if(l <= INF_ROOT) {
            const uint16_t e = (uint16_t)(s | (l << 9));
            for(uint32_t i = bit_reverse(cd, l); i < (1u << INF_ROOT); i += 1u << l) c.tab[i] = e;
        }
    }
    for(int l = 1; l <= INF_MAXBITS; l++) { c.first[l] = (uint16_t)(c.first[l] - c.count[l]); c.index[l] = (uint16_t)(c.index[l] - c.count[l]); }
    return true;
}

// the next symbol of code c, or -1: the bits are no code of it (possible only in the incomplete codes build_code lets through)
HLALA_HD int decode_symbol(InfBits& b, const InfCode& c, const uint16_t* sym, int symCap)
{
    bits_need(b, INF_MAXBITS);
    const uint32_t e = c.tab[bits_peek(b, INF_ROOT) & ((1u << INF_ROOT) - 1u)];
    if(e) { bits_drop(b, e >> 9); return (int)(e & 511u); }
    uint32_t code = 0, v = bits_peek(b, INF_MAXBITS);
    for(int l = 1; l <= INF_MAXBITS; l++) {
        code = (code << 1) | (v & 1u); v >>= 1;
        const uint32_t k = code - c.first[l];                       // (unsigned: a code below the first of its length wraps to a large number)
        if(k < c.count[l]) { const uint32_t i = c.index[l] + k; bits_drop(b, (uint32_t)l); return i < (uint32_t)symCap ? (int)sym[i] : -1; }
    }
    return -1;
}

// RFC 3.2.6
HLALA_HD void build_fixed(InfTables& T)
{
    for(int s = 0; s < 144; s++) T.lens[s] = 8;
    for(int s = 144; s < 256; s++) T.lens[s] = 9;
    for(int s = 256; s < 280; s++) T.lens[s] = 7;
    for(int s = 280; s < 288; s++) T.lens[s] = 8;
    for(int s = 0; s < 32; s++) T.lens[INF_NLIT + s] = 5;
    (void)build_code(T.lens, 288, T.lit, T.litSym, INF_NLIT, false, false);
    (void)build_code(T.lens + INF_NLIT, 32, T.dist, T.distSym, INF_NDIST, false, false);
}

// RFC 3.2.7: HLIT, HDIST, HCLEN, the code length code, the lengths of both alphabets as ONE sequence (a repeat may run from the literal / length
// lengths into the distance lengths), then both codes
HLALA_HD int read_dynamic(InfBits& b, InfTables& T)
{
    const int nlit = (int)bits_get(b, 5) + 257, ndist = (int)bits_get(b, 5) + 1, ncl = (int)bits_get(b, 4) + 4;
    if(bits_overrun(b)) return HLALA_INFLATE_INPUT_EXHAUSTED;
    if(nlit > 286 || ndist > 30) return HLALA_INFLATE_BAD_CODE;
    const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    // (the lengths of the code length code stand in T.lens and its code in the literal tables until it is built; both are filled anew below)
    for(int i = 0; i < 19; i++) T.lens[i] = 0;
    for(int i = 0; i < ncl; i++) T.lens[order[i]] = (uint8_t)bits_get(b, 3);
    if(bits_overrun(b)) return HLALA_INFLATE_INPUT_EXHAUSTED;
    if(!build_code(T.lens, 19, T.lit, T.litSym, INF_NLIT, false, false)) return HLALA_INFLATE_BAD_CODE;
    const int total = nlit + ndist;
    int i = 0;
    while(i < total) {                  // every round consumes at least one bit or returns
        const int s = decode_symbol(b, T.lit, T.litSym, 19);
        if(bits_overrun(b)) return HLALA_INFLATE_INPUT_EXHAUSTED;
        if(s < 0 || s > 18) return HLALA_INFLATE_BAD_CODE;
        if(s < 16) { T.lens[i++] = (uint8_t)s; continue; }
        int rep; uint8_t v = 0;
        if(s == 16) { if(i == 0) return HLALA_INFLATE_BAD_CODE; v = T.lens[i - 1]; rep = 3 + (int)bits_get(b, 2); }
        else if(s == 17) rep = 3 + (int)bits_get(b, 3);
        else rep = 11 + (int)bits_get(b, 7);
        if(bits_overrun(b)) return HLALA_INFLATE_INPUT_EXHAUSTED;
        if(i + rep > total) return HLALA_INFLATE_BAD_CODE;
        for(int k = 0; k < rep; k++) T.lens[i++] = v;
    }
    if(T.lens[256] == 0) return HLALA_INFLATE_BAD_CODE;                  // no end-of-block code
    if(!build_code(T.lens, nlit, T.lit, T.litSym, INF_NLIT, false, false)) return HLALA_INFLATE_BAD_CODE;
    if(!build_code(T.lens + nlit, ndist, T.dist, T.distSym, INF_NDIST, true, true)) return HLALA_INFLATE_BAD_CODE;
    return HLALA_INFLATE_OK;
}

// block header (RFC 3.2.3).  Returns a status; *final and *type (0 stored, 1 fixed, 2 dynamic) are set on HLALA_INFLATE_OK.  For a compressed block the
// tables are ready; for a stored block the reader stands behind LEN / NLEN at the byte offset *stored_at, *stored_len bytes follow (the caller checks
// that the stream holds them, copies them and continues at bit offset 8 * (*stored_at + *stored_len)).
HLALA_HD int read_block_header(InfBits& b, InfTables& T, int* final, int* type, uint32_t* stored_at, uint32_t* stored_len)
{
    *final = (int)bits_get(b, 1); *type = (int)bits_get(b, 2);
    if(bits_overrun(b)) return HLALA_INFLATE_INPUT_EXHAUSTED;
    if(*type == 3) return HLALA_INFLATE_RESERVED_BTYPE;
    if(*type == 0) {
        bits_drop(b, b.cnt & 7u);                                      // to the next byte boundary
        const uint32_t len = bits_get(b, 16), nlen = bits_get(b, 16);
        if(bits_overrun(b)) return HLALA_INFLATE_INPUT_EXHAUSTED;
        if(len != (~nlen & 0xFFFFu)) return HLALA_INFLATE_STORED_LEN;
        const uint64_t at = bits_consumed(b) >> 3;
        if(at + len > (uint64_t)b.n) return HLALA_INFLATE_INPUT_EXHAUSTED;
        *stored_at = (uint32_t)at; *stored_len = len;
        return HLALA_INFLATE_OK;
    }
    if(*type == 1) { build_fixed(T); return HLALA_INFLATE_OK; }
    return read_dynamic(b, T);
}

// one token of a compressed block (RFC 3.2.5): INF_TOKEN with *tok = literal byte, or length << 16 | distance (3 .. 258, 1 .. 32768); INF_END_OF_BLOCK;
// or a status.  Consumes at least one bit unless it returns a status.
HLALA_HD int token(InfBits& b, const InfTables& T, uint32_t* tok)
{
    const int s = decode_symbol(b, T.lit, T.litSym, INF_NLIT);
    if(bits_overrun(b)) return HLALA_INFLATE_INPUT_EXHAUSTED;
    if(s < 0 || s > 285) return HLALA_INFLATE_BAD_SYMBOL;
    if(s < 256) { *tok = (uint32_t)s; return INF_TOKEN; }
    if(s == 256) return INF_END_OF_BLOCK;
    uint32_t len;
    if(s < 265) len = (uint32_t)(s - 254);
    else if(s < 285) { const uint32_t eb = (uint32_t)(s - 261) >> 2; len = 3u + ((4u + ((uint32_t)(s - 265) & 3u)) << eb) + bits_get(b, eb); }
    else len = 258;
    const int d = decode_symbol(b, T.dist, T.distSym, INF_NDIST);
    if(bits_overrun(b)) return HLALA_INFLATE_INPUT_EXHAUSTED;
    if(d < 0 || d > 29) return HLALA_INFLATE_BAD_SYMBOL;
    uint32_t dist;
    if(d < 4) dist = (uint32_t)d + 1u;
    else { const uint32_t eb = ((uint32_t)d >> 1) - 1u; dist = 1u + ((2u + ((uint32_t)d & 1u)) << eb) + bits_get(b, eb); }
    if(bits_overrun(b)) return HLALA_INFLATE_INPUT_EXHAUSTED;
    *tok = (len << 16) | dist;
    return INF_TOKEN;
}

}  // namespace hlala_inflate
#endif

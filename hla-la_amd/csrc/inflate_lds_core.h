// inflate_lds_core.h -- the rules of the inflate kernel that keeps a block's history in LDS (kernel_inflate_lds.hip: k_bgzf_inflate_lds), shared with its host model
// (host_check.cpp: hlala_host_inflate_lds_model).  One text for g++ and hipcc, on top of inflate_core.h (block headers, code tables, the token rules).
//
//   * InfBitsW: a bit reader that refills with 4-byte-aligned 32-bit loads of a staged window of the stream (inflate_core.h's InfBits loads byte by byte).  The window
//     is staged from (first byte) & ~3 with every byte at or beyond `n` as zero: the reader itself never looks at the stream, so it cannot read beyond it.
//   * token_w: token() on that reader.  decode_symbol_t / token_t are the text of decode_symbol / token with the reader as a parameter; for every input they give the
//     same token, the same status and the same number of consumed bits (tests/test_inflate_lds_model.py steps both side by side).
//   * lds_decode_batch: what lane 0 does per batch.
//   * the ring: where output byte q of a block lives, and why the ring is longer than the longest distance.
#ifndef HLALA_INFLATE_LDS_CORE_H_
#define HLALA_INFLATE_LDS_CORE_H_
#include "inflate_core.h"

namespace hlala_inflate {

constexpr uint32_t LDS_BATCH_TOKENS = 64;       // one token per lane of the placing wave
// B: the most output one batch may hold.  Lane 0 closes a batch BEFORE the token that would take the batch's output beyond B (a token is at most 258 bytes, so a batch
// always holds one).  64 matches of 258 bytes would be 16 512: B bounds what the ring must keep beyond the longest distance.
constexpr uint32_t LDS_BATCH_BYTES = 3584;
// R: bytes of the ring.  Output byte q of the block lives at ring_at(q).  A match reads bytes back to q - 32768, so 32768 bytes of history must survive.  They must
// survive a whole BATCH, not one token: a batch is placed literals first, then the matches in token order, so a literal late in the batch is stored before an earlier
// match of the same batch is resolved.  That literal, at output offset q, overwrites ring byte q - R.  With R = 32768 exactly, an earlier match of the batch at a
// distance near 32768 would still need that byte.  A batch starting at p0 writes [p0, p0 + total), total <= B, and reads nothing before p0 - 32768; the slot of the last
// byte written held byte p0 + total - 1 - R < p0 - 32768 as long as R >= 32768 + B.  So with R >= 32768 + B any placement order within a batch is safe.
// R % 64 == 0: a stored block is copied by 64 lanes, lane l taking bytes l, l + 64, ...; two bytes of a stored block longer than R that share a ring slot are R apart,
// so they belong to the same lane, which stores them in order: the later byte stays.
constexpr uint32_t LDS_RING = 32768 + LDS_BATCH_BYTES;
static_assert(LDS_RING % 64 == 0 && LDS_RING >= 32768 + LDS_BATCH_BYTES, "ring rule");
static_assert(2 * LDS_RING > 65536, "the output of a block (isize <= 65536) wraps at most once, at offset R");
static_assert(LDS_BATCH_BYTES >= 258, "a batch holds at least one token");
HLALA_HD uint32_t ring_at(uint32_t q) { return q < LDS_RING ? q : q - LDS_RING; }      // q < 65536 < 2 R

// ---- the input window: LDS_WIN bytes of the stream from a 4-byte-aligned offset, as 32-bit little-endian words
constexpr uint32_t LDS_WIN = 512, LDS_WIN_WORDS = LDS_WIN / 4;
constexpr uint32_t LDS_WIN_SLACK = 16;      // a token is decoded only while this many bytes of the window lie ahead of the reader: a token takes at most 48 bits, which
                                            // are at most two refills (8 bytes); the word index is masked all the same
HLALA_HD uint32_t win_base(uint64_t bitpos) { return (uint32_t)(bitpos >> 3) & ~3u; }
// word k of the window at `base` over the stream in[0, n): bytes at or beyond n are zero and are not loaded
HLALA_HD uint32_t win_word(const uint8_t* in, uint32_t n, uint32_t base, uint32_t k)
{
    uint32_t w = 0;
    for(uint32_t j = 0; j < 4; j++) { const uint64_t i = (uint64_t)base + 4u * k + j; if(i < (uint64_t)n) w |= (uint32_t)in[i] << (8 * j); }
    return w;
}

// ---- the word-wise reader.  wp is the stream offset of the next word; bytes beyond n count as stream positions (they are zero in the window), so the next unread bit
// is simply 8 * wp - cnt, and a bit beyond the end has been consumed once that exceeds 8 * n -- what InfBits keeps as `pad`.
struct InfBitsW {
    const uint32_t* w; uint32_t n, base;
    uint32_t wp, cnt;
    uint64_t buf;
};
HLALA_HD uint32_t bitsw_load(const InfBitsW& b) { return b.w[((b.wp - b.base) >> 2) & (LDS_WIN_WORDS - 1u)]; }
// bit_offset <= 8 n; base = win_base(bit_offset) or below it (a multiple of 4)
HLALA_HD void bits_init_w(InfBitsW& b, const uint32_t* w, uint32_t n, uint32_t base, uint64_t bit_offset)
{
    b.w = w; b.n = n; b.base = base;
    b.wp = (uint32_t)(bit_offset >> 3) & ~3u;
    const uint32_t skip = (uint32_t)(bit_offset - 8ull * b.wp);      // < 32
    b.buf = (uint64_t)(bitsw_load(b) >> skip); b.cnt = 32u - skip; b.wp += 4;
}
// at least k (<= 32) bits in buf: one refill, since it adds 32
HLALA_HD void bits_need(InfBitsW& b, uint32_t k)
{
    if(b.cnt < k) { b.buf |= (uint64_t)bitsw_load(b) << b.cnt; b.cnt += 32; b.wp += 4; }
}
HLALA_HD uint32_t bits_peek(const InfBitsW& b, uint32_t k) { return (uint32_t)b.buf & ((1u << k) - 1u); }
HLALA_HD void bits_drop(InfBitsW& b, uint32_t k) { b.buf >>= k; b.cnt -= k; }
HLALA_HD uint32_t bits_get(InfBitsW& b, uint32_t k) { bits_need(b, k); const uint32_t v = bits_peek(b, k); bits_drop(b, k); return v; }
HLALA_HD uint64_t bits_consumed(const InfBitsW& b) { return 8ull * b.wp - b.cnt; }
HLALA_HD bool bits_overrun(const InfBitsW& b) { return bits_consumed(b) > 8ull * b.n; }

// ---- decode_symbol and token of inflate_core.h, word for word, over any reader with the functions above
template<class Bits> HLALA_HD int decode_symbol_t(Bits& b, const InfCode& c, const uint16_t* sym, int symCap)
{
    bits_need(b, INF_MAXBITS);
    const uint32_t e = c.tab[bits_peek(b, INF_ROOT) & ((1u << INF_ROOT) - 1u)];
    if(e) { bits_drop(b, e >> 9); return (int)(e & 511u); }
    uint32_t code = 0, v = bits_peek(b, INF_MAXBITS);
    for(int l = 1; l <= INF_MAXBITS; l++) {
        code = (code << 1) | (v & 1u); v >>= 1;
        const uint32_t k = code - c.first[l];
        if(k < c.count[l]) { const uint32_t i = c.index[l] + k; bits_drop(b, (uint32_t)l); return i < (uint32_t)symCap ? (int)sym[i] : -1; }
    }
    return -1;
}
// CHECK = false leaves the three tests for the end of the stream out: for a caller that knows that every bit this call can reach lies inside the stream
template<class Bits, bool CHECK = true> HLALA_HD int token_t(Bits& b, const InfTables& T, uint32_t* tok)
{
    const int s = decode_symbol_t(b, T.lit, T.litSym, INF_NLIT);
    if(CHECK && bits_overrun(b)) return HLALA_INFLATE_INPUT_EXHAUSTED;
    if(s < 0 || s > 285) return HLALA_INFLATE_BAD_SYMBOL;
    if(s < 256) { *tok = (uint32_t)s; return INF_TOKEN; }
    if(s == 256) return INF_END_OF_BLOCK;
    uint32_t len;
    if(s < 265) len = (uint32_t)(s - 254);
    else if(s < 285) { const uint32_t eb = (uint32_t)(s - 261) >> 2; len = 3u + ((4u + ((uint32_t)(s - 265) & 3u)) << eb) + bits_get(b, eb); }
    else len = 258;
    const int d = decode_symbol_t(b, T.dist, T.distSym, INF_NDIST);
    if(CHECK && bits_overrun(b)) return HLALA_INFLATE_INPUT_EXHAUSTED;
    if(d < 0 || d > 29) return HLALA_INFLATE_BAD_SYMBOL;
    uint32_t dist;
    if(d < 4) dist = (uint32_t)d + 1u;
    else { const uint32_t eb = ((uint32_t)d >> 1) - 1u; dist = 1u + ((2u + ((uint32_t)d & 1u)) << eb) + bits_get(b, eb); }
    if(CHECK && bits_overrun(b)) return HLALA_INFLATE_INPUT_EXHAUSTED;
    *tok = (len << 16) | dist;
    return INF_TOKEN;
}
// the contract of token(): same token, same status, same bits consumed; never a byte at or beyond n (the window holds zeros there); consumes a bit or ends
HLALA_HD int token_w(InfBitsW& b, const InfTables& T, uint32_t* tok) { return token_t(b, T, tok); }

// ---- one batch.  The window `win` stands at win_base(bitpos); `produced` bytes of the block are out already.  Tokens go to tok[0, *nTok); a batch ends at
// LDS_BATCH_TOKENS tokens, before the token that would take *total beyond LDS_BATCH_BYTES (its bits are given back: *bitposOut is where it starts), when fewer than
// LDS_WIN_SLACK bytes of the window lie ahead, at the end of the DEFLATE block (*end), or with a status: a distance beyond `produced`, more than isize bytes, or what
// token_w says.  Every token stored lies inside [0, isize) and every source inside [0, its own offset).  Returns HLALA_INFLATE_OK or that status.
// Lane 0 issues one instruction at a time, so the loop is kept short: the closing rule and the size check share one compare (cap = the smaller of B and the room left
// in the block), the place in front of the current token is kept as the reader's two counters, and a window that lies inside the stream as a whole (every window but a
// stream's last) is decoded without the tests for the end of the stream -- the reader cannot leave the window, so it cannot leave the stream.
template<bool CHECK> HLALA_HD int lds_batch_loop(InfBitsW& b, const InfTables& T, uint32_t produced, uint32_t isize, uint32_t* tok, uint32_t* nTok, uint32_t* total, int* end,
                                                 uint64_t* bitposOut)
{
    const uint32_t room = isize - produced, cap = room < LDS_BATCH_BYTES ? room : LDS_BATCH_BYTES;
    const uint32_t wpEnd = b.base + LDS_WIN - LDS_WIN_SLACK;
    uint32_t nt = 0, sum = 0, wp0 = b.wp, cnt0 = b.cnt; int rc = HLALA_INFLATE_OK;
    *end = 0;
    while(nt < LDS_BATCH_TOKENS && b.wp <= wpEnd) {
        uint32_t t = 0;
        const int r = token_t<InfBitsW, CHECK>(b, T, &t);
        if(r != INF_TOKEN) { if(r == INF_END_OF_BLOCK) { *end = 1; wp0 = b.wp; cnt0 = b.cnt; } else rc = r; break; }
        uint32_t len = 1;
        if(t >= 256u) { len = t >> 16; if((t & 0xFFFFu) > produced + sum) { rc = HLALA_INFLATE_FAR_DISTANCE; break; } }
        if(sum + len > cap) { if(len > room - sum) rc = HLALA_INFLATE_OUTPUT_SIZE; break; }      // (else the batch is full: (wp0, cnt0) still stands in front of this token)
        tok[nt++] = t; sum += len; wp0 = b.wp; cnt0 = b.cnt;
    }
    *nTok = nt; *total = sum; *bitposOut = 8ull * wp0 - cnt0;
    return rc;
}
HLALA_HD int lds_decode_batch(const uint32_t* win, uint32_t n, uint64_t bitpos, const InfTables& T, uint32_t produced, uint32_t isize, uint32_t* tok, uint32_t* nTok,
                              uint32_t* total, int* end, uint64_t* bitposOut)
{
    InfBitsW b; bits_init_w(b, win, n, win_base(bitpos), bitpos);
    if((uint64_t)b.base + LDS_WIN <= (uint64_t)n) return lds_batch_loop<false>(b, T, produced, isize, tok, nTok, total, end, bitposOut);
    return lds_batch_loop<true>(b, T, produced, isize, tok, nTok, total, end, bitposOut);
}

// ---- what the decoding side hands to the placing side, one per round
constexpr int LDS_UNIT_NONE = 0, LDS_UNIT_TOKENS = 1, LDS_UNIT_STORED = 2;

}  // namespace hlala_inflate
#endif

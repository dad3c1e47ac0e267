// inflate_lds_model.h -- host only: k_bgzf_inflate_lds run serially over its core (inflate_lds_core.h).  Behind hlala_host_inflate_lds_model (host_check.cpp) and
// tools/inflate_lds_check.cpp, which is the same text under sanitizers in a program of its own.
#ifndef HLALA_INFLATE_LDS_MODEL_H_
#define HLALA_INFLATE_LDS_MODEL_H_
#include "inflate_lds_core.h"

namespace hlala_inflate {

// k_bgzf_inflate_lds (kernel_inflate_lds.hip) run serially over the same core (inflate_lds_core.h): the same rounds -- the decoding side makes one unit per round (a
// stored block, a batch of tokens, or only the end), the placing side takes it one round later --, the same batching and closing rule, a real ring of R bytes, the
// placement in the kernel's order (all literals of a batch, then its matches in token order, every byte of a match from the ring) and the flush of every batch from
// the ring to out.  Same contract as hlala_host_inflate_model; *rounds (may be null) receives the number of rounds = workgroup barriers of the kernel.
inline int lds_model(const uint8_t* comp, uint32_t clen, uint8_t* out, uint32_t isize, int32_t* rounds)
{
    struct Unit { uint32_t tok[LDS_BATCH_TOKENS]; uint32_t nTok, base, at, len; int kind, last, status; };
    static thread_local InfTables T;
    static thread_local uint8_t ring[LDS_RING];
    static thread_local uint32_t win[LDS_WIN_WORDS];
    static thread_local Unit U[2];
    // the decoding side's state
    uint64_t bitpos = 0; uint32_t produced = 0; bool inBlock = false; int fin = 0;
    auto produce = [&](Unit& u) {
        u.kind = LDS_UNIT_NONE; u.last = 0; u.status = HLALA_INFLATE_OK; u.nTok = 0; u.base = produced; u.at = u.len = 0;
        if(!inBlock) {
            InfBits b; bits_init(b, comp, clen, 0, 0xFFFFFFFFu, bitpos);
            int type = 0; uint32_t at = 0, len = 0;
            const int rc = read_block_header(b, T, &fin, &type, &at, &len);
            if(rc != HLALA_INFLATE_OK) { u.last = 1; u.status = rc; return; }
            if(type == 0) {
                if(len > isize - produced) { u.last = 1; u.status = HLALA_INFLATE_OUTPUT_SIZE; return; }
                u.kind = LDS_UNIT_STORED; u.at = at; u.len = len;
                produced += len; bitpos = 8ull * ((uint64_t)at + len);
                if(fin) { u.last = 1; u.status = produced == isize ? HLALA_INFLATE_OK : HLALA_INFLATE_OUTPUT_SIZE; }
                return;
            }
            bitpos = bits_consumed(b); inBlock = true;
        }
        const uint32_t base = win_base(bitpos);
        for(uint32_t k = 0; k < LDS_WIN_WORDS; k++) win[k] = win_word(comp, clen, base, k);
        uint32_t total = 0; int end = 0; uint64_t next = bitpos;
        const int rc = lds_decode_batch(win, clen, bitpos, T, produced, isize, u.tok, &u.nTok, &total, &end, &next);
        if(rc != HLALA_INFLATE_OK) { u.nTok = 0; u.last = 1; u.status = rc; return; }      // (the batch is dropped, as k_bgzf_inflate drops it)
        u.kind = LDS_UNIT_TOKENS; produced += total; bitpos = next;
        if(end) { inBlock = false; if(fin) { u.last = 1; u.status = produced == isize ? HLALA_INFLATE_OK : HLALA_INFLATE_OUTPUT_SIZE; } }
    };
    auto place = [&](const Unit& u) {
        if(u.kind == LDS_UNIT_STORED) {
            for(uint32_t k = 0; k < u.len; k++) { const uint8_t v = comp[u.at + k]; out[u.base + k] = v; ring[ring_at(u.base + k)] = v; }
            return;
        }
        if(u.kind != LDS_UNIT_TOKENS) return;
        uint32_t off[LDS_BATCH_TOKENS], total = 0;
        for(uint32_t i = 0; i < u.nTok; i++) { off[i] = total; total += u.tok[i] < 256u ? 1u : (u.tok[i] >> 16); }
        for(uint32_t i = 0; i < u.nTok; i++) if(u.tok[i] < 256u) ring[ring_at(u.base + off[i])] = (uint8_t)u.tok[i];
        for(uint32_t i = 0; i < u.nTok; i++) {
            if(u.tok[i] < 256u) continue;
            const uint32_t L = u.tok[i] >> 16, D = u.tok[i] & 0xFFFFu, pos = u.base + off[i];
            for(uint32_t k = 0, m = 0; k < L; k++) { ring[ring_at(pos + k)] = ring[ring_at(pos - D + m)]; if(++m == D) m = 0; }      // byte k is byte k mod D of the D bytes before pos
        }
        for(uint32_t k = 0; k < total; k++) out[u.base + k] = ring[ring_at(u.base + k)];
    };
    int32_t r = 0; int prevLast = 0, st = HLALA_INFLATE_OK;
    for(;; r++) {
        if(!prevLast) produce(U[r & 1]);
        if(r > 0) place(U[(r - 1) & 1]);
        // (the kernel's workgroup barrier)
        if(prevLast) { st = U[(r - 1) & 1].status; break; }
        prevLast = U[r & 1].last;
    }
    if(rounds) *rounds = r + 1;
    return st;
}
// token() and token_w() side by side from bit offset `bit` of comp[0, clen), each on its own reader (the block header is read first: comp starts a DEFLATE block).  Up to
// `cap` steps: tok[2 i], rc[2 i], bits[2 i] are token()'s token, result and bit offset behind it, [2 i + 1] token_w()'s (its window staged anew whenever lds_decode_batch would close a batch for it).  Returns the
// number of steps taken (a step whose result is not INF_TOKEN is the last), or -1 if the header is no compressed block.
inline int lds_token_steps(const uint8_t* comp, uint32_t clen, int32_t cap, uint32_t* tok, int32_t* rc, uint64_t* bits)
{
    static thread_local InfTables T;
    InfBits b; bits_init(b, comp, clen, 0, 0xFFFFFFFFu, 0);
    int fin = 0, type = 0; uint32_t at = 0, len = 0;
    if(read_block_header(b, T, &fin, &type, &at, &len) != HLALA_INFLATE_OK || type == 0) return -1;
    uint32_t win[LDS_WIN_WORDS];
    int32_t i = 0;
    InfBitsW w; uint32_t base = 0; bool staged = false;
    for(; i < cap; ) {
        if(!staged || (w.wp - base) + LDS_WIN_SLACK > LDS_WIN) {      // (the batch rule of lds_decode_batch: the reader runs on through a window, then starts in the next)
            const uint64_t pos = staged ? bits_consumed(w) : bits_consumed(b);
            base = win_base(pos);
            for(uint32_t k = 0; k < LDS_WIN_WORDS; k++) win[k] = win_word(comp, clen, base, k);
            bits_init_w(w, win, clen, base, pos); staged = true;
        }
        uint32_t t0 = 0, t1 = 0;
        const int r0 = token(b, T, &t0), r1 = token_w(w, T, &t1);
        tok[2 * i] = t0; tok[2 * i + 1] = t1; rc[2 * i] = r0; rc[2 * i + 1] = r1;
        bits[2 * i] = r0 == INF_TOKEN || r0 == INF_END_OF_BLOCK ? bits_consumed(b) : 0; bits[2 * i + 1] = r1 == INF_TOKEN || r1 == INF_END_OF_BLOCK ? bits_consumed(w) : 0;
        i++;
        if(r0 != INF_TOKEN || r1 != INF_TOKEN) break;
    }
    return i;
}

}  // namespace hlala_inflate
#endif

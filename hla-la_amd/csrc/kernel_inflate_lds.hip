// kernel_inflate_lds.hip -- k_bgzf_inflate_lds: raw DEFLATE (RFC 1951) of BGZF blocks, one workgroup of two wavefronts per block, the block's history in LDS.
//
// k_bgzf_inflate (kernel_inflate.hip) places every match through HBM -- a global load of bytes the wave stored before, often behind an agent-scope fence -- and lets
// lane 0 refill its bit buffer byte by byte; placement and decode take turns.  Here (rules and reasons: inflate_lds_core.h)
//   * the output of the block lives in a ring of R = 32768 + B bytes of LDS.  A match reads the ring and writes the ring; after a batch is placed its bytes are flushed
//     from the ring to the block's range of the output buffer, consecutive lanes writing consecutive bytes (4-byte stores between an unaligned head and tail).
//     There is no global load of output bytes and no fence in this kernel;
//   * lane 0 reads bits through InfBitsW: 32-bit loads of a window staged from (first byte) & ~3;
//   * wave 0 decodes round r (its lane 0 reads block headers and tokens, the wave stages the window) while wave 1 places and flushes what round r - 1 decoded, out of
//     the other of two unit buffers.  Lane 0 counts `produced` itself for the distance and size checks, so the decode does not wait for the placement.
// The two waves meet at ONE workgroup barrier per round and nowhere else: no flag, no spinning.  Whether a round is the last is read from the unit in LDS behind the
// barrier by both waves, so both run the same number of rounds on every path (statuses, stored and empty blocks included; hlala_host_inflate_lds_rounds counts them).
// Only wave 1 touches the ring, only wave 0 the tables and the window.
//
// LDS: ring 36 352 + tables 3 200 + window 512 + two units 2 x 284 + state 36 (+ 4 of padding) = 40 672 B <= 40 960 = 160 KiB / 4: four blocks per CU.
//
// Bounds: the descriptors are validated on the host; lane 0 checks every token against the bytes produced and against isize BEFORE the unit is handed over, stored
// blocks likewise; ring indices go through ring_at (offsets < 65536 < 2 R); the window index of the bit reader is masked.  Every loop consumes input bits or ends.
#pragma once
#include "device_common.h"
#include "inflate_lds_core.h"

namespace hlala {

#ifndef HLALA_INFLATE_LDS_WAVES
#define HLALA_INFLATE_LDS_WAVES 2      // 1: the same rounds, one wave decoding and then placing (the form the two-wave one was measured against: DESIGN.md 4 I.1)
#endif
constexpr int INF_LDS_WAVES = HLALA_INFLATE_LDS_WAVES;
static_assert(INF_LDS_WAVES == 1 || INF_LDS_WAVES == 2, "one or two waves");

struct InfLdsUnit {
    uint32_t tok[hlala_inflate::LDS_BATCH_TOKENS];
    uint32_t nTok, base, at, len;       // tokens at output offset `base`; or a stored block: `len` bytes from stream offset `at` to output offset `base`
    int kind, last, status;             // LDS_UNIT_*; the block ends with this unit, with this status
};
struct InfLdsShared {
    alignas(16) uint8_t ring[hlala_inflate::LDS_RING];
    hlala_inflate::InfTables T;
    uint32_t win[hlala_inflate::LDS_WIN_WORDS];
    InfLdsUnit U[2];
    // lane 0 of the decoding wave to its wave
    uint32_t bitLo, bitHi, total, storedAt, storedLen;
    int status, final, type, end;
};
static_assert(sizeof(InfLdsShared) <= 40960, "four blocks per CU");

// ---- the decoding side: one unit.  All arguments but S and u are wave-uniform state of the decoding wave.
__device__ __forceinline__ void inflate_lds_produce(InfLdsShared& S, InfLdsUnit& u, const uint8_t* in, uint32_t n, uint32_t isize, int lane, u64& bitpos, uint32_t& produced,
                                                    bool& inBlock, int& fin)
{
    using namespace hlala_inflate;
    int kind = LDS_UNIT_NONE, last = 0, st = HLALA_INFLATE_OK; uint32_t at = 0, len = 0;
    const uint32_t base0 = produced;
    bool batch = inBlock;
    if(!inBlock) {
        if(lane == 0) {
            InfBits b; bits_init(b, in, n, 0, 0xFFFFFFFFu, bitpos);
            int f = 0, type = 0; uint32_t a = 0, l = 0;
            S.status = read_block_header(b, S.T, &f, &type, &a, &l);
            S.final = f; S.type = type; S.storedAt = a; S.storedLen = l;
            const u64 c = bits_consumed(b); S.bitLo = (uint32_t)c; S.bitHi = (uint32_t)(c >> 32);
        }
        WSYNC();
        st = uni(S.status);
        if(st != HLALA_INFLATE_OK) last = 1;
        else {
            fin = uni(S.final);
            if(uni(S.type) == 0) {
                at = (uint32_t)uni((int)S.storedAt); len = (uint32_t)uni((int)S.storedLen);      // (at + len <= n: read_block_header)
                if(len > isize - produced) { st = HLALA_INFLATE_OUTPUT_SIZE; last = 1; }
                else {
                    kind = LDS_UNIT_STORED; produced += len; bitpos = 8ull * ((u64)at + len);
                    if(fin) { last = 1; st = produced == isize ? HLALA_INFLATE_OK : HLALA_INFLATE_OUTPUT_SIZE; }
                }
            } else {
                bitpos = ((u64)(uint32_t)uni((int)S.bitHi) << 32) | (uint32_t)uni((int)S.bitLo);
                inBlock = true; batch = true;
            }
        }
        WSYNC();      // (lane 0 writes S.status again below)
    }
    if(batch) {
        const uint32_t wb = win_base(bitpos);
        for(uint32_t k = (uint32_t)lane; k < LDS_WIN_WORDS; k += 64) S.win[k] = win_word(in, n, wb, k);
        WSYNC();
        if(lane == 0) {
            uint32_t nt = 0, total = 0; int end = 0; uint64_t next = bitpos;
            const int rc = lds_decode_batch(S.win, n, bitpos, S.T, produced, isize, u.tok, &nt, &total, &end, &next);
            u.nTok = rc == HLALA_INFLATE_OK ? nt : 0u;            // (a batch with a status is dropped, as k_bgzf_inflate drops it)
            S.status = rc; S.total = total; S.end = end; S.bitLo = (uint32_t)next; S.bitHi = (uint32_t)(next >> 32);
        }
        WSYNC();
        st = uni(S.status);
        if(st != HLALA_INFLATE_OK) last = 1;
        else {
            kind = LDS_UNIT_TOKENS; produced += (uint32_t)uni((int)S.total);
            bitpos = ((u64)(uint32_t)uni((int)S.bitHi) << 32) | (uint32_t)uni((int)S.bitLo);
            if(uni(S.end)) { inBlock = false; if(fin) { last = 1; st = produced == isize ? HLALA_INFLATE_OK : HLALA_INFLATE_OUTPUT_SIZE; } }
        }
    }
    if(lane == 0) { if(kind != LDS_UNIT_TOKENS) u.nTok = 0; u.base = base0; u.at = at; u.len = len; u.kind = kind; u.last = last; u.status = st; }
}

// ---- the placing side: ring bytes [q0, q0 + total) of the block to o[q0 ...], any alignment of o + q0.  Nothing outside that range is written.
__device__ __forceinline__ void inflate_lds_flush(const uint8_t* ring, uint8_t* o, uint32_t q0, uint32_t total, int lane)
{
    using namespace hlala_inflate;
    uint8_t* g = o + q0;
    uint32_t head = (uint32_t)((4u - (uint32_t)((uintptr_t)g & 3u)) & 3u);
    if(head > total) head = total;
    const uint32_t words = (total - head) >> 2, tail = head + 4u * words;
    if((uint32_t)lane < head) g[lane] = ring[ring_at(q0 + (uint32_t)lane)];
    for(uint32_t w = (uint32_t)lane; w < words; w += 64) {
        const uint32_t q = q0 + head + 4u * w;
        uint32_t v;
        if((q & 3u) == 0u) v = *(const uint32_t*)(ring + ring_at(q));      // (ring and output aligned alike; R % 4 == 0: no wrap inside an aligned word)
        else v = (uint32_t)ring[ring_at(q)] | (uint32_t)ring[ring_at(q + 1)] << 8 | (uint32_t)ring[ring_at(q + 2)] << 16 | (uint32_t)ring[ring_at(q + 3)] << 24;
        *(uint32_t*)(g + head + 4u * w) = v;
    }
    if((uint32_t)lane < total - tail) g[tail + (uint32_t)lane] = ring[ring_at(q0 + tail + (uint32_t)lane)];
}

__device__ __forceinline__ void inflate_lds_place(InfLdsShared& S, const InfLdsUnit& u, const uint8_t* in, uint8_t* o, int lane)
{
    using namespace hlala_inflate;
    const int kind = uni(u.kind);
    const uint32_t base = (uint32_t)uni((int)u.base);
    if(kind == LDS_UNIT_STORED) {
        // from the compressed bytes to the output directly, and into the ring in stream order: lane l takes bytes l, l + 64, ... in ascending order, and R % 64 == 0,
        // so of two bytes that share a ring slot (a stored block longer than R) the later one is stored later by the same lane
        const uint32_t at = (uint32_t)uni((int)u.at), len = (uint32_t)uni((int)u.len);
        for(uint32_t k = (uint32_t)lane; k < len; k += 64) { const uint8_t v = in[at + k]; o[base + k] = v; S.ring[ring_at(base + k)] = v; }
        WSYNC();
        return;
    }
    if(kind != LDS_UNIT_TOKENS) return;
    const int nt = uni((int)u.nTok);
    const uint32_t t = lane < nt ? u.tok[lane] : 0u;
    const bool isMatch = lane < nt && t >= 256u;
    const int len = lane < nt ? (isMatch ? (int)(t >> 16) : 1) : 0;
    int total = 0;
    const int off = wave_excl_scan(len, total);
    if(lane < nt && !isMatch) S.ring[ring_at(base + (uint32_t)off)] = (uint8_t)t;
    WSYNC();
    u64 m = __ballot(isMatch);
    while(m) {                          // (wave-uniform: m is the same in all lanes)
        const int i = __builtin_ctzll(m); m &= m - 1;
        const uint32_t ti = (uint32_t)__builtin_amdgcn_readlane((int)t, i), pos = base + (uint32_t)__builtin_amdgcn_readlane(off, i);
        const uint32_t L = ti >> 16, D = ti & 0xFFFFu, src = pos - D;
        // byte k of the match is byte (k mod D) of the D bytes before pos, which the match does not write: no lane of one match depends on another.  A lane's k goes up by
        // 64 per step, so its (k mod D) goes up by (64 mod D) and wraps at most once: one division per match and one per lane, none per byte
        if(D >= L) { for(uint32_t k = (uint32_t)lane; k < L; k += 64) S.ring[ring_at(pos + k)] = S.ring[ring_at(src + k)]; }
        else {
            const uint32_t step = 64u % D;
            uint32_t r = (uint32_t)lane % D;
            for(uint32_t k = (uint32_t)lane; k < L; k += 64) { S.ring[ring_at(pos + k)] = S.ring[ring_at(src + r)]; r += step; if(r >= D) r -= D; }
        }
        WSYNC();
    }
    inflate_lds_flush(S.ring, o, base, (uint32_t)total, lane);
}

__global__ __launch_bounds__(64 * INF_LDS_WAVES) void k_bgzf_inflate_lds(const uint8_t* comp, const hlala_bgzf_block* blocks, int nBlocks, uint8_t* out, int* status)
{
    using namespace hlala_inflate;
    __shared__ InfLdsShared S;
    const int blk = blockIdx.x;
    if(blk >= nBlocks) return;          // (block-uniform: no wave of a workgroup that stays reaches a barrier alone)
    const int lane = lane_id(), wave = uni((int)(threadIdx.x >> 6));
    const hlala_bgzf_block d = blocks[blk];
    const uint8_t* in = comp + d.coff;
    uint8_t* o = out + d.uoff;
    const uint32_t n = d.clen, isize = d.isize;
    u64 bitpos = 0; uint32_t produced = 0; bool inBlock = false; int fin = 0;      // the decoding wave's
    int prevLast = 0, st = HLALA_INFLATE_OK;
    for(int r = 0;; r++) {              // one round: at least one bit consumed or a stored block taken, or the last
        if(INF_LDS_WAVES == 1) {
            if(!prevLast) inflate_lds_produce(S, S.U[r & 1], in, n, isize, lane, bitpos, produced, inBlock, fin);
            WSYNC();
            if(r > 0) inflate_lds_place(S, S.U[(r - 1) & 1], in, o, lane);
        } else if(wave == 0) {
            if(!prevLast) inflate_lds_produce(S, S.U[r & 1], in, n, isize, lane, bitpos, produced, inBlock, fin);
        } else {
            if(r > 0) inflate_lds_place(S, S.U[(r - 1) & 1], in, o, lane);
        }
        __syncthreads();
        // unit (r - 1) & 1 has been placed and is written again in round r + 1, behind this barrier; unit r & 1 is complete and stays until round r + 2
        if(prevLast) { st = uni(S.U[(r - 1) & 1].status); break; }
        prevLast = uni(S.U[r & 1].last);
    }
    if(threadIdx.x == 0) status[blk] = st;
}

}  // namespace hlala

// kernel_inflate.hip -- k_bgzf_inflate: raw DEFLATE (RFC 1951) of BGZF blocks, one 64-lane wavefront per block.
//
// A DEFLATE stream is serial in its bits (where a code ends is only known once it is decoded) but not in its bytes: lane 0 decodes a batch of up to 64 tokens
// with the shared core (inflate_core.h: bit reader, block headers, code tables, one token) into LDS, then the whole wave places the batch:
//   * output offsets of the tokens = wave prefix sum of their lengths;
//   * every literal of the batch is stored by its own lane;
//   * the matches are resolved in token order, all lanes copying one match: byte k of a match is byte (k mod distance) of its source, so a match that overlaps its
//     own output (distance < length, the periodic extension) never reads a byte it writes, and neither do two lanes of one match depend on each other.
// The compressed bytes of a batch are staged in an LDS window by all lanes (coalesced) before lane 0 reads them bit by bit.
//
// The output goes straight to the block's range of the output buffer in HBM: a 64 KiB window per wave in LDS would leave two waves per CU.  A match therefore
// loads bytes that lanes of this wave have stored before -- literals of the same batch, earlier matches, earlier batches.  Such a load must not overtake the
// store and must not be served from a line this CU's L1 fetched before the store.  `dirtyLo` is the lowest output offset stored since the last fence; a match
// whose source reaches beyond it runs an agent-scope release + acquire first (the stores have arrived in L2, the L1 is invalidated), every other match reads bytes
// that were fenced already.  Matches at short distances pay for the fence, matches into older data -- the common case in BAM records -- do not.
//
// Bounds: the descriptors are validated on the host (hlala_bgzf_inflate); lane 0 checks every token against the bytes produced and against isize BEFORE the
// batch is placed, stored blocks likewise; the window index of the bit reader is masked.  Every loop consumes input bits or ends: see inflate_core.h.
#pragma once
#include "device_common.h"
#include "inflate_core.h"

namespace hlala {

constexpr int INF_WIN = 512;        // bytes of the input window: 64 tokens take at most 64 * 48 bits = 384 bytes, the reader looks up to 8 bytes ahead
constexpr int INF_BATCH = 64;

struct InfShared {
    hlala_inflate::InfTables T;
    uint8_t win[INF_WIN];
    uint32_t tok[INF_BATCH];
    uint32_t bitLo, bitHi;          // bit offset of the next unread bit
    int status, final, type, nTok, endOfBlock;
    uint32_t storedAt, storedLen;
};

__device__ __forceinline__ void inflate_fence()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
}

__global__ __launch_bounds__(64) void k_bgzf_inflate(const uint8_t* comp, const hlala_bgzf_block* blocks, int nBlocks, uint8_t* out, int* status)
{
    using namespace hlala_inflate;
    __shared__ InfShared S;
    const int blk = blockIdx.x;
    if(blk >= nBlocks) return;
    const int lane = lane_id();
    const hlala_bgzf_block d = blocks[blk];
    const uint8_t* in = comp + d.coff;
    uint8_t* o = out + d.uoff;
    const uint32_t n = d.clen, isize = d.isize;
    u64 bitpos = 0;
    uint32_t produced = 0, dirtyLo = 0xFFFFFFFFu;
    int st = HLALA_INFLATE_OK;
    for(;;) {                                   // one DEFLATE block per round: at least three bits consumed, or a status
        if(lane == 0) {
            InfBits b; bits_init(b, in, n, 0, 0xFFFFFFFFu, bitpos);
            int fin = 0, type = 0; uint32_t at = 0, len = 0;
            S.status = read_block_header(b, S.T, &fin, &type, &at, &len);
            S.final = fin; S.type = type; S.storedAt = at; S.storedLen = len;
            const u64 c = bits_consumed(b); S.bitLo = (uint32_t)c; S.bitHi = (uint32_t)(c >> 32);
        }
        WSYNC();
        st = uni(S.status);
        if(st != HLALA_INFLATE_OK) break;
        const int fin = uni(S.final), type = uni(S.type);
        if(type == 0) {
            const uint32_t at = (uint32_t)uni((int)S.storedAt), len = (uint32_t)uni((int)S.storedLen);      // (at + len <= n: read_block_header)
            if(len > isize - produced) { st = HLALA_INFLATE_OUTPUT_SIZE; break; }
            for(uint32_t k = (uint32_t)lane; k < len; k += 64) o[produced + k] = in[at + k];
            if(len && produced < dirtyLo) dirtyLo = produced;
            produced += len; bitpos = 8ull * ((u64)at + len);
        } else {
            bitpos = ((u64)(uint32_t)uni((int)S.bitHi) << 32) | (uint32_t)uni((int)S.bitLo);
            for(;;) {                           // one batch per round: at least one token or the end of the block (at least one bit), or a status
                const uint32_t w0 = (uint32_t)(bitpos >> 3);
                for(int k = lane; k < INF_WIN; k += 64) { const u64 i = (u64)w0 + (u64)k; S.win[k] = i < (u64)n ? in[i] : (uint8_t)0; }
                WSYNC();
                if(lane == 0) {
                    InfBits b; bits_init(b, S.win, n, w0, INF_WIN - 1, bitpos);
                    int nt = 0, end = 0, rc = HLALA_INFLATE_OK; uint32_t p = produced;
                    while(nt < INF_BATCH && (b.pos - w0) + 16u <= (uint32_t)INF_WIN) {
                        uint32_t t = 0;
                        const int r = token(b, S.T, &t);
                        if(r == INF_END_OF_BLOCK) { end = 1; break; }
                        if(r != INF_TOKEN) { rc = r; break; }
                        const uint32_t len = t < 256u ? 1u : (t >> 16);
                        if(t >= 256u && (t & 0xFFFFu) > p) { rc = HLALA_INFLATE_FAR_DISTANCE; break; }
                        if(len > isize - p) { rc = HLALA_INFLATE_OUTPUT_SIZE; break; }
                        S.tok[nt++] = t; p += len;
                    }
                    S.nTok = nt; S.endOfBlock = end; S.status = rc;
                    const u64 c = bits_consumed(b); S.bitLo = (uint32_t)c; S.bitHi = (uint32_t)(c >> 32);
                }
                WSYNC();
                st = uni(S.status);
                if(st != HLALA_INFLATE_OK) break;
                const int nt = uni(S.nTok);
                // ---- place the batch: every token lies inside [0, isize) and every source inside [0, its own offset) -- lane 0 has checked
                const uint32_t t = lane < nt ? S.tok[lane] : 0u;
                const bool isMatch = lane < nt && t >= 256u;
                const int len = lane < nt ? (isMatch ? (int)(t >> 16) : 1) : 0;
                int total = 0;
                const int off = wave_excl_scan(len, total);
                if(lane < nt && !isMatch) o[produced + (uint32_t)off] = (uint8_t)t;
                if(total > 0 && produced < dirtyLo) dirtyLo = produced;
                u64 m = __ballot(isMatch);
                while(m) {                      // (wave-uniform: m is the same in all lanes)
                    const int i = __builtin_ctzll(m); m &= m - 1;
                    const uint32_t ti = (uint32_t)__builtin_amdgcn_readlane((int)t, i), pos = produced + (uint32_t)__builtin_amdgcn_readlane(off, i);
                    const uint32_t L = ti >> 16, D = ti & 0xFFFFu;
                    if(pos - D + (L < D ? L : D) > dirtyLo) { inflate_fence(); dirtyLo = 0xFFFFFFFFu; }
                    const uint8_t* src = o + (pos - D);
                    for(uint32_t k = (uint32_t)lane; k < L; k += 64) o[pos + k] = src[D >= L ? k : k % D];
                    if(pos < dirtyLo) dirtyLo = pos;
                }
                produced += (uint32_t)total;
                bitpos = ((u64)(uint32_t)uni((int)S.bitHi) << 32) | (uint32_t)uni((int)S.bitLo);
                if(uni(S.endOfBlock)) break;
            }
            if(st != HLALA_INFLATE_OK) break;
        }
        if(fin) { if(produced != isize) st = HLALA_INFLATE_OUTPUT_SIZE; break; }
    }
    if(lane == 0) status[blk] = st;
}

}  // namespace hlala

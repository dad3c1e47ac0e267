// kernel_crc32.hip -- k_bgzf_crc32: the CRC-32 of inflated BGZF blocks, one 64-lane wavefront per block, launched behind k_bgzf_inflate on the same stream with the
// same descriptors.  CRC-32 is linear over GF(2): the block is cut into 64 segments of L bytes aligned to its end (crc32_core.h), every lane computes the raw
// register of its own segment, six shuffle steps combine them.
//
// How the bytes reach the lanes: every lane streams its OWN segment -- byte loads up to the first 16-byte boundary of the address, aligned 16-byte loads, byte
// loads for the rest -- whatever uoff is.  Segments lie L <= 1024 bytes apart, so one load instruction of the wave touches 64 cache lines, but the eight
// consecutive 16-byte loads of a lane stay in one 128-byte line: every line is fetched from L2 once and then served by the CU's L1 (a wave holds 64 lines =
// 8 KiB there).  The alternative, coalesced tiles through LDS, needs the whole block (up to 64 KiB) per wave in LDS before a lane can start on its segment, or a
// transpose per tile whose LDS reads stride by L (a multiple of 256 B for the common full-size block: all lanes on one bank); it was not built.
// The slicing tables (4 x 256 words, 4 KiB) live in LDS, built by the wave from the polynomial; their reads are data dependent, so they spread over the banks as
// the data does.
//
// Bounds: a lane reads only bytes [lo, hi) of its own segment, which lies in [0, isize) of the block (crc_segment clips at 0); the host has checked
// uoff + isize against the buffer (inflate_run).  A block whose inflate status is not HLALA_INFLATE_OK is not read at all.  The kernel stores to status[] and
// crc_out[] only, one element per block, from lane 0.
#pragma once
#include "device_common.h"
#include "crc32_core.h"

namespace hlala {

// x^(8 * 2^k) mod P, k = 0..16: the factors of x^(8 n) for n <= 65536 and of x^(8 L); computed from the polynomial when the code object is built
struct CrcPow8 {
    uint32_t v[17];
    constexpr CrcPow8() : v{} { uint32_t s = hlala_crc32::CRC_X8; for(int k = 0; k < 17; k++) { v[k] = s; s = hlala_crc32::crc_mul(s, s); } }
};
__device__ const CrcPow8 g_crc_pow8{};

__device__ __forceinline__ uint32_t crc_word4(uint32_t reg, const uint4& v, const uint32_t* T)
{
    using namespace hlala_crc32;
    reg = crc_update_word(reg, v.x, T); reg = crc_update_word(reg, v.y, T); reg = crc_update_word(reg, v.z, T);
    return crc_update_word(reg, v.w, T);
}

__global__ __launch_bounds__(64) void k_bgzf_crc32(const uint8_t* out, const hlala_bgzf_block* blocks, int nBlocks, int* status, const uint32_t* expect, uint32_t* crcOut)
{
    using namespace hlala_crc32;
    __shared__ uint32_t T[CRC_TABLE_WORDS];
    const int blk = blockIdx.x;
    if(blk >= nBlocks) return;
    const int lane = lane_id();
    if(uni(status[blk]) != HLALA_INFLATE_OK) {          // rejected by the inflate kernel: its status stays, its bytes are not read
        if(lane == 0 && crcOut) crcOut[blk] = 0;
        return;
    }
    // ---- the tables: the byte table first (every later slice looks its entries up there)
    for(int k = 0; k < 4; k++) T[lane + 64 * k] = crc_table_entry((uint32_t)(lane + 64 * k));
    WSYNC();
    for(int t = 1; t < 4; t++) for(int k = 0; k < 4; k++) T[t * 256 + lane + 64 * k] = crc_table_next(T[(t - 1) * 256 + lane + 64 * k], T);       // (the entry of slice t - 1 is this lane's own store)
    WSYNC();
    const hlala_bgzf_block d = blocks[blk];
    const uint32_t n = d.isize <= 65536u ? d.isize : 65536u;          // (isize <= 65536: checked on the host; the powers below cover 17 bits)
    const uint32_t L = crc_seg_len(n);
    const uint8_t* p = out + d.uoff;
    // ---- this lane's segment
    uint32_t lo, hi;
    crc_segment(n, L, lane, &lo, &hi);
    uint32_t reg = 0, i = lo;
    while(i < hi && (((uintptr_t)(p + i)) & 15u)) { reg = crc_update_byte(reg, p[i], T); i++; }
    if(hi - i >= 16u) {                                  // (p + i is 16-byte aligned here; the next load is issued before this one is folded in)
        uint4 v = *(const uint4*)(p + i); i += 16;
        while(hi - i >= 16u) { const uint4 nx = *(const uint4*)(p + i); i += 16; reg = crc_word4(reg, v, T); v = nx; }
        reg = crc_word4(reg, v, T);
    }
    while(i < hi) { reg = crc_update_byte(reg, p[i], T); i++; }
    // ---- x^(8 n) * 0xFFFFFFFF (the initial value's share) in lanes 0..31 and x^(8 L) in lanes 32..63: products of the factors the set bits select, by halving
    const int kb = lane & 31;
    const uint32_t bits = lane < 32 ? n : L;
    uint32_t f = (kb < 17 && ((bits >> kb) & 1u)) ? g_crc_pow8.v[kb < 17 ? kb : 0] : CRC_ONE;
    if(lane == 17) f = 0xFFFFFFFFu;
    for(int step = 1; step < 32; step <<= 1) f = crc_mul(f, (uint32_t)__shfl_down((int)f, step));      // (lane 0 reads lanes < 32 only, lane 32 lanes < 64 only)
    const uint32_t initShare = (uint32_t)__shfl((int)f, 0);
    uint32_t s = (uint32_t)__shfl((int)f, 32);
    // ---- combine: part[j] = s * part[j] ^ part[j + step] for every j that is a multiple of 2 * step, then s = s * s.  Lane `step` is the upper half of a pair
    // from this step on: it squares s in the same multiplication
    for(int step = 1; step < 64; step <<= 1) {
        const bool lower = (lane & (2 * step - 1)) == 0;
        const uint32_t r = crc_mul(s, lower ? reg : s);
        const uint32_t upper = (uint32_t)__shfl_down((int)reg, step);
        if(lower) reg = r ^ upper;
        s = (uint32_t)__shfl((int)r, step);
    }
    if(lane == 0) {
        const uint32_t crc = reg ^ initShare ^ 0xFFFFFFFFu;
        if(crcOut) crcOut[blk] = crc;
        if(expect && expect[blk] != crc) status[blk] = HLALA_INFLATE_CRC_MISMATCH;
    }
}

}  // namespace hlala

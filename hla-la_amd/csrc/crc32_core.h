// crc32_core.h -- the CRC-32 of RFC 1952 (the one a BGZF block carries behind its payload), shared by the device kernel (kernel_crc32.hip) and by the host model
// (host_check.cpp: hlala_host_crc32_model).  Reflected polynomial 0xEDB88320, initial value and final xor 0xFFFFFFFF.
//
// A CRC register is a polynomial over GF(2) of degree < 32, reflected: bit 31 is the coefficient of x^0, bit 0 that of x^31.  A RAW register starts at 0 and takes
// no final xor; it is linear in the bytes, so for a byte string A || B
//     raw(A || B) = raw(A) * x^(8 |B|)  ^  raw(B)      (mod P),
// and a raw register is not changed by bytes it never sees in FRONT of its own (zero times anything).  The initial value contributes 0xFFFFFFFF * x^(8 n):
//     crc(data[0, n)) = raw(data) ^ mul(xpow8(n), 0xFFFFFFFF) ^ 0xFFFFFFFF.
//
// The split of a block of n bytes over 64 lanes (segments of L bytes aligned to the END of the block: the short or empty ones are the leading ones, whose raw
// registers need no correction) and the six-step combine are crc_seg_len / crc_segment / crc_of_block_model below; the kernel runs the same steps with one lane per
// segment.  Every table is built from the polynomial.
#ifndef HLALA_CRC32_CORE_H_
#define HLALA_CRC32_CORE_H_
#include <stdint.h>

#if defined(__HIPCC__)
#define HLALA_CRC_HD __host__ __device__ inline
#else
#define HLALA_CRC_HD inline
#endif

namespace hlala_crc32 {

constexpr uint32_t CRC_POLY = 0xEDB88320u;
constexpr uint32_t CRC_ONE = 0x80000000u;         // the polynomial 1
constexpr uint32_t CRC_X8 = 0x00800000u;          // x^8
constexpr int CRC_LANES = 64;
constexpr uint32_t CRC_TABLE_WORDS = 4 * 256;     // slicing by four: T[k * 256 + b] = raw register of byte b followed by k zero bytes

// b * x mod P
HLALA_CRC_HD constexpr uint32_t crc_times_x(uint32_t b) { return (b >> 1) ^ (CRC_POLY & (0u - (b & 1u))); }
// raw register of the single byte b (entry b of the byte table)
HLALA_CRC_HD constexpr uint32_t crc_table_entry(uint32_t b)
{
    uint32_t c = b;
    for(int k = 0; k < 8; k++) c = crc_times_x(c);
    return c;
}
// entry of the next slice from the entry of this one (t0: the byte table): one more zero byte behind
HLALA_CRC_HD uint32_t crc_table_next(uint32_t prev, const uint32_t* t0) { return (prev >> 8) ^ t0[prev & 0xFFu]; }
HLALA_CRC_HD void crc_build_tables(uint32_t* T)
{
    for(uint32_t b = 0; b < 256; b++) T[b] = crc_table_entry(b);
    for(uint32_t k = 1; k < 4; k++) for(uint32_t b = 0; b < 256; b++) T[k * 256 + b] = crc_table_next(T[(k - 1) * 256 + b], T);
}
// raw register update by one byte / by four bytes (w little-endian: its low byte is the first of the stream)
HLALA_CRC_HD uint32_t crc_update_byte(uint32_t reg, uint32_t byte, const uint32_t* T) { return (reg >> 8) ^ T[(reg ^ byte) & 0xFFu]; }
HLALA_CRC_HD uint32_t crc_update_word(uint32_t reg, uint32_t w, const uint32_t* T)
{
    const uint32_t x = reg ^ w;
    return T[768 + (x & 0xFFu)] ^ T[512 + ((x >> 8) & 0xFFu)] ^ T[256 + ((x >> 16) & 0xFFu)] ^ T[x >> 24];
}
// product of two reflected polynomials mod P: 32 shift / xor steps
HLALA_CRC_HD constexpr uint32_t crc_mul(uint32_t a, uint32_t b)
{
    uint32_t p = 0;
    for(int i = 0; i < 32; i++) { p ^= b & (0u - ((a >> (31 - i)) & 1u)); b = crc_times_x(b); }
    return p;
}
// x^(8 n) mod P by square-and-multiply
HLALA_CRC_HD constexpr uint32_t crc_xpow8(uint32_t n)
{
    uint32_t r = CRC_ONE, s = CRC_X8;
    while(n) { if(n & 1u) r = crc_mul(r, s); s = crc_mul(s, s); n >>= 1; }
    return r;
}
// bytes per lane for a block of n bytes: ceil(n / 64), rounded up to a multiple of 4, at least 4
HLALA_CRC_HD constexpr uint32_t crc_seg_len(uint32_t n)
{
    const uint32_t l = ((n >> 6) + ((n & 63u) ? 1u : 0u) + 3u) & ~3u;
    return l < 4u ? 4u : l;
}
// lane j owns bytes [lo, hi) = [n - (64 - j) L, n - (63 - j) L), clipped at 0
HLALA_CRC_HD void crc_segment(uint32_t n, uint32_t L, int j, uint32_t* lo, uint32_t* hi)
{
    const uint64_t behind = (uint64_t)(CRC_LANES - 1 - j) * L;      // bytes of the block behind this segment
    *hi = n > behind ? (uint32_t)(n - behind) : 0u;
    *lo = n > behind + L ? (uint32_t)(n - behind - L) : 0u;
}
// raw register of data[lo, hi)
HLALA_CRC_HD uint32_t crc_raw_bytes(const uint8_t* data, uint32_t lo, uint32_t hi, const uint32_t* T)
{
    uint32_t reg = 0;
    for(uint32_t i = lo; i < hi; i++) reg = crc_update_byte(reg, data[i], T);
    return reg;
}
// the combine of the 64 raw registers (part[j] of lane j), in place; returns the CRC-32 of the block
HLALA_CRC_HD uint32_t crc_combine_model(uint32_t* part, uint32_t n, uint32_t L)
{
    uint32_t s = crc_xpow8(L);
    for(int step = 1; step < CRC_LANES; step <<= 1) {
        for(int j = 0; j < CRC_LANES; j += 2 * step) part[j] = crc_mul(s, part[j]) ^ part[j + step];
        s = crc_mul(s, s);
    }
    return part[0] ^ crc_mul(crc_xpow8(n), 0xFFFFFFFFu) ^ 0xFFFFFFFFu;
}
// the whole split, serially: what one wavefront of k_bgzf_crc32 computes for a block
HLALA_CRC_HD uint32_t crc_of_block_model(const uint8_t* data, uint32_t n, const uint32_t* T)
{
    const uint32_t L = crc_seg_len(n);
    uint32_t part[CRC_LANES];
    for(int j = 0; j < CRC_LANES; j++) { uint32_t lo, hi; crc_segment(n, L, j, &lo, &hi); part[j] = crc_raw_bytes(data, lo, hi, T); }
    return crc_combine_model(part, n, L);
}

}  // namespace hlala_crc32
#endif

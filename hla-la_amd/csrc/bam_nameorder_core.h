// bam_nameorder_core.h -- ordering names (variable-length byte strings) as host_bam.cpp's name_less does, shared by the device kernels (kernel_bamnameorder.hip) and by
// the host model (bam_nameorder_model.h; host_check.cpp: hlala_host_bam_name_order_model).  Plain inline functions, no HIP types: g++ and hipcc compile the same text.
//
// The order: the first min(la, lb) bytes as unsigned bytes, then the shorter name first; equal names by ascending input index.  It is found by MSD refinement in
// rounds of NAM_W bytes.  Round r gives every unresolved name a 64-bit key: its bytes [r W, r W + W) big-endian in bits 63..8, zero-padded past the end of the name,
// and in bits 7..0 how many of them are the name's own (0..W).  Comparing keys as integers compares the padded bytes first and, where they are equal, the counts:
// the name with fewer valid bytes is a prefix of the other and comes first, which is what makes "ab" < "ab\0" < "ab\0\0" come out right.  A name whose count is
// below W has ended in this round: names that are still together with it after the round are equal to it.
//
// What it promises for ANY arguments: nam_key reads no byte at or beyond n_bytes (a name that leaves the buffer reads as zeros there); nam_check_args refuses, before
// anything runs, a name that leaves the byte buffer, has no byte or more than 65535.
#ifndef HLALA_BAM_NAMEORDER_CORE_H_
#define HLALA_BAM_NAMEORDER_CORE_H_
#include <stdint.h>
#include <string.h>

#include "../../include/hlala_gpu.h"

#ifndef HLALA_HD
#if defined(__HIPCC__)
#define HLALA_HD __host__ __device__ inline
#else
#define HLALA_HD inline
#endif
#endif

namespace hlala_nameorder {

constexpr uint32_t NAM_W = 7;                      // name bytes per round
constexpr uint32_t NAM_MAX_LEN = 65535;            // the longest name (a BAM record's l_read_name is 8 bits; the descriptors of the grouping stage carry 16)

// the key of the name at bytes[off, off + len) in round r
HLALA_HD uint64_t nam_key(const uint8_t* bytes, uint64_t n_bytes, uint64_t off, uint32_t len, uint32_t r)
{
    const uint64_t at = (uint64_t)r * NAM_W;
    if(at >= len) return 0;
    const uint32_t left = len - (uint32_t)at, cnt = left < NAM_W ? left : NAM_W;
    uint64_t key = cnt;
    for(uint32_t k = 0; k < cnt; k++) {
        const uint64_t p = off + at + k;
        const uint64_t b = (p >= off && p < n_bytes) ? bytes[p] : 0;       // (p >= off: an offset near 2^64 does not wrap into the buffer)
        key |= b << (56 - 8 * k);
    }
    return key;
}
HLALA_HD uint32_t nam_key_count(uint64_t key) { return (uint32_t)(key & 0xFFu); }
// the name has no byte beyond this round's
HLALA_HD bool nam_ended(uint64_t key) { return nam_key_count(key) < NAM_W; }
// sorted slot j (segment s, key k) against slot j - 1 (sp, kp): a new segment starts here
HLALA_HD bool nam_split(uint64_t j, uint32_t sp, uint32_t s, uint64_t kp, uint64_t k) { return j == 0 || sp != s || kp != k; }
// the round after which nothing can be unresolved: a name of len bytes ends in round len / W
HLALA_HD int64_t nam_max_rounds(uint32_t max_len) { return (int64_t)((max_len + NAM_W - 1) / NAM_W) + 1; }

// The arguments of hlala_bam_name_order / hlala_host_bam_name_order_model, checked before anything runs.  Returns null or what is wrong; *max_len: the longest name.
// Reads name_off[0, n) and name_len[0, n) only.
inline const char* nam_check_args(const uint64_t* name_off, const uint32_t* name_len, int64_t n, const uint8_t* bytes, uint64_t n_bytes, const uint32_t* order,
                                  const hlala_bam_name_order_stats* stats, uint32_t* max_len)
{
    if(max_len) *max_len = 0;
    if(n < 0) return "negative n";
    if(n >= ((int64_t)1 << 31)) return "2^31 names or more in one call";
    if(!stats || (n && (!name_off || !name_len || !order)) || (n_bytes && !bytes)) return "null argument";
    uint32_t longest = 0;
    for(int64_t i = 0; i < n; i++) {
        const uint32_t L = name_len[i];
        if(L == 0) return "a name with name_len 0";
        if(L > NAM_MAX_LEN) return "a name longer than 65535 bytes";
        if(name_off[i] > n_bytes || n_bytes - name_off[i] < L) return "a name that lies beyond the byte buffer";
        if(L > longest) longest = L;
    }
    if(max_len) *max_len = longest;
    return nullptr;
}

}  // namespace hlala_nameorder
#endif

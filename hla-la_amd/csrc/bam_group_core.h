// bam_group_core.h -- grouping BAM record descriptors by read name, shared by the device kernels (kernel_bamgroup.hip) and by the host model
// (bam_group_model.h; host_check.cpp: hlala_host_bam_group_model).  Plain inline functions, no HIP types: g++ and hipcc compile the same text.
//
// The rule is the group phase of host_bam.cpp: the descriptors of a sample in (hash, order) order; a RUN is a maximal stretch of equal hashes; a run is CLEAN when
// every record has the name of its predecessor in the run (same nameLen, same bytes), else COLLIDED; a clean run is one unit, COMPLETE when a primary record
// (flags & 2) exists for mate 0 and -- unless long_read_mode -- for mate 1.  Collided runs are left to the host (real samples have none).
//
// What it promises for ANY descriptor array: grp_same_name checks both ranges against the end of the bytes it is given before it reads one of them, and reads
// nothing else; grp_check_args refuses (before anything runs) a descriptor whose name leaves the byte buffer, has no byte, names a mate other than 0 / 1 or
// breaks the ascending order, so the passes never see one.
#ifndef HLALA_BAM_GROUP_CORE_H_
#define HLALA_BAM_GROUP_CORE_H_
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

namespace hlala_bamgroup {

constexpr uint32_t GRP_NAME_AT = 32;               // a name starts 32 bytes behind its descriptor's rec_off (the fixed part of a BAM record body)
// flag[] of hlala_bam_group
constexpr uint8_t GRP_START = 1, GRP_COLLIDED = 2, GRP_COMPLETE = 4;
// what a record contributes to the word of its run (k_grp_fold)
constexpr uint32_t RUN_NEQ = 1, RUN_PRIM0 = 2, RUN_PRIM1 = 4;
// per record on the device: nameLen | which << 16 | flags << 24
HLALA_HD uint32_t grp_meta(uint32_t nameLen, uint32_t which, uint32_t flags) { return (nameLen & 0xFFFFu) | ((which & 0xFFu) << 16) | ((flags & 0xFFu) << 24); }
HLALA_HD uint32_t meta_name_len(uint32_t m) { return m & 0xFFFFu; }
HLALA_HD uint32_t meta_which(uint32_t m) { return (m >> 16) & 0xFFu; }
HLALA_HD uint32_t meta_flags(uint32_t m) { return m >> 24; }

// are the la bytes at base + oa the lb bytes at base + ob?  Nothing at or beyond base + end is read: a name that leaves [0, end) equals no name.
HLALA_HD bool grp_same_name(const uint8_t* base, uint64_t end, uint64_t oa, uint32_t la, uint64_t ob, uint32_t lb)
{
    if(la != lb) return false;
    if(oa > end || end - oa < la || ob > end || end - ob < lb) return false;
    const uint8_t* a = base + oa; const uint8_t* b = base + ob;
    uint32_t i = 0;
    for(; i + 8 <= la; i += 8) { uint64_t x, y; __builtin_memcpy(&x, a + i, 8); __builtin_memcpy(&y, b + i, 8); if(x != y) return false; }      // (names start at any alignment)
    for(; i < la; i++) if(a[i] != b[i]) return false;
    return true;
}
// sorted record i (hash h, predecessor's hash hp) is the first of its run
HLALA_HD bool grp_run_start(uint64_t i, uint64_t hp, uint64_t h) { return i == 0 || hp != h; }
// what a record ORs into its run's word
HLALA_HD uint32_t grp_fold_bits(bool neq, uint32_t meta)
{
    const bool primary = (meta_flags(meta) & 2u) != 0;
    return (neq ? RUN_NEQ : 0u) | (primary && meta_which(meta) == 0 ? RUN_PRIM0 : 0u) | (primary && meta_which(meta) == 1 ? RUN_PRIM1 : 0u);
}
// flag[] of a run's first record from the run's word
HLALA_HD uint8_t grp_run_flag(uint32_t word, int32_t long_read_mode)
{
    if(word & RUN_NEQ) return (uint8_t)(GRP_START | GRP_COLLIDED);
    const bool complete = long_read_mode ? (word & RUN_PRIM0) != 0 : (word & RUN_PRIM0) && (word & RUN_PRIM1);
    return (uint8_t)(GRP_START | (complete ? GRP_COMPLETE : 0));
}

// The arguments of hlala_bam_group / hlala_host_bam_group_model, checked before anything runs.  Returns null or what is wrong.  Reads recs[0, n) only.
inline const char* grp_check_args(const hlala_bam_rec* recs, int64_t n, const uint8_t* bytes, uint64_t n_bytes, const uint32_t* perm, const uint8_t* flag, const hlala_bam_group_stats* stats)
{
    if(n < 0) return "negative n";
    if(n >= ((int64_t)1 << 31)) return "2^31 descriptors or more in one call";
    if(!stats || (n && (!recs || !perm || !flag)) || (n_bytes && !bytes)) return "null argument";
    for(int64_t i = 0; i < n; i++) {
        const hlala_bam_rec& r = recs[i];
        if(r.nameLen == 0) return "a descriptor with nameLen 0";
        if(r.rec_off > n_bytes || n_bytes - r.rec_off < (uint64_t)GRP_NAME_AT + r.nameLen) return "a descriptor whose name lies beyond the byte buffer";
        if(r.which > 1) return "a descriptor with a mate other than 0 or 1";
        if(i > 0 && r.order < recs[i - 1].order) return "descriptors not in ascending order";
    }
    return nullptr;
}
// the round sizes of hlala_bam_group_rounds: none negative, their sum n
inline const char* grp_check_rounds(const int64_t* round_recs, int32_t n_rounds, int64_t n)
{
    if(n_rounds < 0 || (n_rounds && !round_recs)) return "null or negative rounds";
    int64_t s = 0;
    for(int32_t k = 0; k < n_rounds; k++) { if(round_recs[k] < 0 || round_recs[k] > n - s) return "round sizes do not add up to n"; s += round_recs[k]; }
    return s == n ? nullptr : "round sizes do not add up to n";
}

}  // namespace hlala_bamgroup
#endif

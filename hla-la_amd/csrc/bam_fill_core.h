// bam_fill_core.h -- the layout and the fill of a seed batch as host_bam.cpp's layout loop and fill_units do them, shared by the device kernels (kernel_bamfill.hip) and
// by the host model (bam_fill_model.h; host_check.cpp: hlala_host_bam_fill_model).  Plain inline functions, no HIP types: g++ and hipcc compile the same text.
//
// The rule.  Read r = unit * nm + mate takes the unit's records of that mate in file order (the order they have in the grouped array) and puts them into the order
// sortChainsInSeeds leaves (sorted_mate in host_bam.cpp: std::sort ascending by AS, then std::reverse).  For at most 16 elements libstdc++'s std::sort is a plain
// insertion sort and therefore stable, so the result is descending AS, equal AS in descending file order: record a stands before record b where fil_before says so.
// That closed form is claimed up to FIL_MAX_MATE alignments only; a unit with a longer mate is a host unit.  The primary is the first record with flags & 2 in that
// order; the read's l_seq, bases and qualities are the primary's.  Chains and CIGARs are written in that order.
//
// What it promises for ANY arguments: fil_check_args refuses, before a record byte is read, a unit range that leaves the descriptors, a record extent that leaves the
// byte buffer, unit_count 0, a mate other than 0 / 1, a filled unit with a mate beyond FIL_MAX_MATE or without a primary on a required mate, and more than 2^31 - 1
// chains; fil_byte reads no byte at or beyond n_bytes.
#ifndef HLALA_BAM_FILL_CORE_H_
#define HLALA_BAM_FILL_CORE_H_
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

namespace hlala_bamfill {

constexpr uint32_t FIL_MAX_MATE = HLALA_BAM_FILL_MAX_MATE;      // alignments of one mate the closed form of the order is claimed for (and the lanes of a group)
constexpr uint32_t FIL_MAX_UNIT = 2 * FIL_MAX_MATE;             // records of a unit the device looks at: beyond, one mate is beyond FIL_MAX_MATE whatever the split
constexpr uint32_t FIL_HOST = HLALA_BAM_FILL_HOST;              // unit_first of a host unit; chain_src of a chain of a host unit
constexpr uint32_t FIL_NAME_AT = 32;                            // the name's place in a record body; the CIGAR follows l_read_name bytes on

HLALA_HD int fil_nm(int32_t long_read_mode) { return long_read_mode ? 1 : 2; }
// record a (score asA, place ka in file order) stands before record b in the order sortChainsInSeeds leaves
HLALA_HD bool fil_before(int32_t asA, uint32_t ka, int32_t asB, uint32_t kb) { return asA > asB || (asA == asB && ka > kb); }
// BuildCharData: 4-bit code -> character; Phred -> Phred + 33 modulo 256
HLALA_HD uint8_t fil_base(uint32_t code)
{
    // "=ACMGRSVTWYHKDBN" as two 64-bit words of eight characters each (no table in memory: the same text for both compilers)
    const uint64_t lo = 0x565352474d43413dull /* "=ACMGRSV" */, hi = 0x4e42444b48595754ull /* "TWYHKDBN" */;
    return (uint8_t)(((code & 8u) ? hi : lo) >> (8u * (code & 7u)));
}
HLALA_HD uint8_t fil_qual(uint8_t q) { return (uint8_t)(q + 33u); }
// the packed layout of hlala_batch_in: the first byte of read r (of the sample) whose bases start at base offset off
HLALA_HD int64_t fil_packed_at(int64_t off, int64_t r) { return (off + r + 1) >> 1; }
// where the parts of a record body lie in the byte buffer
HLALA_HD uint64_t fil_cigar_at(const hlala_bam_rec& x) { return x.rec_off + FIL_NAME_AT + x.l_read_name; }
HLALA_HD uint64_t fil_seq_at(const hlala_bam_rec& x) { return fil_cigar_at(x) + 4ull * x.n_cigar; }
HLALA_HD uint64_t fil_qual_at(const hlala_bam_rec& x, int32_t l_seq) { return fil_seq_at(x) + (((uint64_t)(uint32_t)l_seq + 1) >> 1); }
// the bytes of the buffer a record's parts occupy, from rec_off on
HLALA_HD uint64_t fil_extent(const hlala_bam_rec& x)
{
    const uint64_t ls = x.l_seq > 0 ? (uint64_t)x.l_seq : 0, nameEnd = FIL_NAME_AT + x.nameLen, body = FIL_NAME_AT + x.l_read_name + 4ull * x.n_cigar + ((ls + 1) >> 1) + ls;
    return nameEnd > body ? nameEnd : body;
}
HLALA_HD uint8_t fil_byte(const uint8_t* bytes, uint64_t n_bytes, uint64_t p) { return p < n_bytes ? bytes[p] : 0; }
// a CIGAR word at any alignment: four byte loads, little-endian
HLALA_HD uint32_t fil_word(const uint8_t* bytes, uint64_t n_bytes, uint64_t p)
{
    return (uint32_t)fil_byte(bytes, n_bytes, p) | ((uint32_t)fil_byte(bytes, n_bytes, p + 1) << 8) | ((uint32_t)fil_byte(bytes, n_bytes, p + 2) << 16) | ((uint32_t)fil_byte(bytes, n_bytes, p + 3) << 24);
}

// The arguments of hlala_bam_fill_create / hlala_host_bam_fill_model, checked before anything runs.  Returns null or what is wrong.  Reads the descriptors and the
// unit arrays only, never `bytes`.
// (fil_check_args_cap: the same checks with max_mate alignments on a mate allowed and `beyond` said of a mate with more -- bam_fill_wide_core.h)
inline const char* fil_check_args_cap(const hlala_bam_fill_in* in, const int64_t* read_off, const int64_t* chain_off, const int64_t* cigar_count, const int64_t* name_off,
                                      const hlala_bam_fill_stats* stats, uint32_t max_mate, const char* beyond)
{
    if(!in || !stats) return "null argument";
    if(in->n < 0 || in->n_units < 0 || in->n_host_units < 0) return "negative count";
    if(in->n >= ((int64_t)1 << 31) || in->n_units >= ((int64_t)1 << 30)) return "2^31 descriptors or 2^30 units or more in one call";
    if(in->n_units == 0) return nullptr;
    if(!in->unit_first || !in->unit_count || !read_off || !chain_off || !cigar_count || !name_off || (in->n && !in->recs) || (in->n_bytes && !in->bytes) || (in->n_host_units && !in->host_sizes))
        return "null argument";
    const int nm = fil_nm(in->long_read_mode);
    int64_t nHost = 0, nChains = 0;
    for(int64_t u = 0; u < in->n_units; u++) {
        const uint32_t first = in->unit_first[u], count = in->unit_count[u];
        if(first == FIL_HOST) {
            if(nHost >= in->n_host_units) return "more host units than n_host_units";
            const int64_t* hs = in->host_sizes + nHost * (3 * nm + 1);
            for(int k = 0; k < 3 * nm + 1; k++) if(hs[k] < 0 || hs[k] > 0x7FFFFFFFll) return "a host unit's size below 0 or above 2^31 - 1";
            for(int m = 0; m < nm; m++) nChains += hs[3 * m + 1];
            nHost++;
            if(nChains > 0x7FFFFFFFll) return "more than 2^31 - 1 chains";
            continue;
        }
        if(count == 0) return "a unit with unit_count 0";
        if((uint64_t)first + count > (uint64_t)in->n) return "a unit whose records lie beyond the descriptors";
        uint32_t mates[2] = {0, 0}; bool prim[2] = {false, false};
        for(uint32_t k = 0; k < count; k++) {
            const hlala_bam_rec& x = in->recs[first + k];
            if(x.which >= (uint8_t)nm) return "a record whose mate is not 0 / 1 (0 in long-read mode)";
            if(x.l_seq < 0) return "a record with a negative l_seq";
            if(x.rec_off > in->n_bytes || in->n_bytes - x.rec_off < fil_extent(x)) return "a record that lies beyond the byte buffer";
            mates[x.which]++; if(x.flags & 2) prim[x.which] = true;
            if(mates[x.which] > max_mate) return beyond;
        }
        for(int m = 0; m < nm; m++) if(!prim[m]) return "a filled unit without a primary on a required mate";
        nChains += count;
        if(nChains > 0x7FFFFFFFll) return "more than 2^31 - 1 chains";
    }
    if(nHost != in->n_host_units) return "fewer host units than n_host_units";
    return nullptr;
}
inline const char* fil_check_args(const hlala_bam_fill_in* in, const int64_t* read_off, const int64_t* chain_off, const int64_t* cigar_count, const int64_t* name_off,
                                  const hlala_bam_fill_stats* stats)
{
    return fil_check_args_cap(in, read_off, chain_off, cigar_count, name_off, stats, FIL_MAX_MATE, "a filled unit with more than 16 alignments on one mate");
}

}  // namespace hlala_bamfill
#endif

// bam_scan_core.h -- the record pass over inflated BAM bytes, shared by the device kernels (kernel_bamscan.hip) and by the host model
// (host_check.cpp: hlala_host_bam_scan_model).  Plain inline functions, no HIP types: g++ and hipcc compile the same text.
//
// What it promises for ANY input bytes [data, data + n):
//   * no byte at or beyond `n` is read: every function checks the range it is about to read against `n` (or against the record's own length, which was
//     checked against `n` before) first;
//   * every loop advances by at least 36 bytes (a hop over one record: 4 + block_size, block_size >= 32), runs over a fixed range (the chain of
//     BAM_SCAN_DEPTH records, the CIGAR operations, the intervals of a reference) or walks the bytes of ONE record (tags, the name);
//   * nothing is written but through the pointers the caller hands in, each with a capacity.
//
// The rules are those of host_bam.cpp, statement for statement: bam_hop is its `while(avail(4))` loop, bam_parse_record the loop body of its parse phase, in
// the same order of checks, so a file fails here with the status whose text (hlala_bam_scan_status_text) the host path throws.
#ifndef HLALA_BAM_SCAN_CORE_H_
#define HLALA_BAM_SCAN_CORE_H_
#include <stdint.h>

#include "../../include/hlala_gpu.h"

#ifndef HLALA_HD
#if defined(__HIPCC__)
#define HLALA_HD __host__ __device__ inline
#else
#define HLALA_HD inline
#endif
#endif

namespace hlala_bamscan {

constexpr int BAM_SCAN_DEPTH = 3;                   // a candidate offset is accepted when a chain of this many plausible records starts at it
constexpr uint32_t BAM_NONE = 0xFFFFFFFFu;          // no offset (offsets are 32-bit within a call: n < 2^32)
constexpr uint32_t BAM_HEAD = 36;                   // the length field + the fixed part of a record
constexpr int32_t BAM_MAX_BLOCK = 1 << 28;          // host_bam.cpp: a longer block_size is a bad length
constexpr uint32_t BAM_DEFAULT_SLICE = 16384;
constexpr int32_t BAM_DEFAULT_MAX_REHOPS = 1024;
// how a hop through a slice ended
constexpr int HOP_RAN = 0;                          // it reached the slice end: *q_out is the first start at or beyond it
constexpr int HOP_TAIL = 1;                         // fewer than 4 bytes, or a record that does not fit before n: the walk ends at *q_out
constexpr int HOP_BAD = 2;                          // a length below 32 or above 1 << 28 at *q_out

HLALA_HD uint32_t ld16(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }
HLALA_HD uint32_t ld32(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }

// could ONE record start at q?  The caller has checked q + BAM_HEAD <= n.  *bs is the block_size where the answer is yes.
HLALA_HD bool plausible_one(const uint8_t* d, uint64_t n, uint64_t q, int32_t n_ref, uint32_t* bs)
{
    const int32_t block = (int32_t)ld32(d + q);
    if(block < 32 || block > BAM_MAX_BLOCK) return false;
    const uint8_t* r = d + q + 4;
    const int32_t refID = (int32_t)ld32(r), pos = (int32_t)ld32(r + 4);
    const uint32_t l_read_name = r[8], n_cigar = ld16(r + 12);
    const int32_t l_seq = (int32_t)ld32(r + 16), next_ref = (int32_t)ld32(r + 20), next_pos = (int32_t)ld32(r + 24);
    if(refID < -1 || refID >= n_ref || pos < -1 || l_read_name < 1 || l_seq < 0) return false;
    const uint64_t need = 32ull + l_read_name + 4ull * n_cigar + ((uint64_t)l_seq + 1) / 2 + (uint64_t)l_seq;
    if(need > (uint64_t)block) return false;
    if(next_ref < -1 || next_ref >= n_ref || next_pos < -1) return false;
    const uint64_t z = q + 4 + 32 + l_read_name - 1;             // the name's last byte
    if(z < n && d[z] != 0) return false;
    *bs = (uint32_t)block;
    return true;
}

// could a record start at offset p of [d, d + n)?  A chain of BAM_SCAN_DEPTH plausible records; a chain that reaches n earlier passes with the records that fit
// (at least one).
HLALA_HD bool bam_plausible(const uint8_t* d, uint64_t n, uint64_t p, int32_t n_ref)
{
    uint64_t q = p;
    for(int k = 0; k < BAM_SCAN_DEPTH; k++) {
        if(q > n || n - q < BAM_HEAD) return k > 0;
        uint32_t bs = 0;
        if(!plausible_one(d, n, q, n_ref, &bs)) return false;
        q += 4ull + bs;
    }
    return true;
}

// The host's rule: from q (<= n) over the records that start below `limit`.  starts (may be null) receives the first `cap` starts.  Every round advances by
// 4 + block_size >= 36 bytes or ends.
HLALA_HD int bam_hop(const uint8_t* d, uint64_t n, uint64_t q, uint64_t limit, uint32_t* starts, uint64_t cap, uint64_t* q_out, uint32_t* count)
{
    uint32_t c = 0; int how = HOP_RAN;
    while(q < limit) {
        if(q > n || n - q < 4) { how = HOP_TAIL; break; }
        const int32_t bs = (int32_t)ld32(d + q);
        if(bs < 32 || bs > BAM_MAX_BLOCK) { how = HOP_BAD; break; }
        if(n - q - 4 < (uint64_t)bs) { how = HOP_TAIL; break; }
        if(starts && c < cap) starts[c] = (uint32_t)q;
        c++; q += 4ull + (uint64_t)bs;
    }
    *q_out = q; *count = c;
    return how;
}

// host_bam.cpp: hash_name
HLALA_HD uint64_t bam_hash_name(const uint8_t* s, uint32_t n)
{
    uint64_t h = 0xcbf29ce484222325ull;
    for(uint32_t i = 0; i < n; i++) { h ^= s[i]; h *= 0x100000001b3ull; }
    h ^= h >> 29; h *= 0xbf58476d1ce4e5b9ull; h ^= h >> 32;
    return h;
}

// Record `ri` of the call, whose length field is at `start`: the parse loop of the host decoder.  Returns a HLALA_BAMSCAN_* status.  With status OK:
// *n_desc descriptors (one per interval the record lies in), the first min(*n_desc, cap) of them written to out (may be null: the counting pass), each with
// rec_off; *compact = the bytes of the record that are kept (refID .. end of the qualities) if it yields a descriptor, else 0; *examined as the host counts it.
HLALA_HD int bam_parse_record(const uint8_t* d, uint64_t n, uint32_t start, const hlala_bam_scan_in& in, uint64_t ri, uint64_t rec_off, hlala_bam_rec* out, uint32_t cap,
                              uint32_t* n_desc, uint32_t* compact, uint32_t* examined)
{
    *n_desc = 0; *compact = 0; *examined = 0;
    if((uint64_t)start > n || n - start < BAM_HEAD) return HLALA_BAMSCAN_BAD_LENGTH;           // (never after bam_hop; the reads below rest on it)
    const uint64_t rn = ld32(d + start);
    if(rn < 32 || rn > n - start - 4) return HLALA_BAMSCAN_BAD_LENGTH;
    const uint8_t* rec = d + start + 4;
    const int32_t refID = (int32_t)ld32(rec), position = (int32_t)ld32(rec + 4);
    const uint32_t l_read_name = rec[8], n_cigar = ld16(rec + 12), flag = ld16(rec + 14);
    const int32_t l_seq = (int32_t)ld32(rec + 16);
    if(l_seq < 0) return HLALA_BAMSCAN_CORRUPT_RECORD;
    const uint64_t oName = 32, oCigar = oName + l_read_name, oSeq = oCigar + 4ull * n_cigar, oQual = oSeq + ((uint64_t)l_seq + 1) / 2, oTags = oQual + (uint64_t)l_seq;
    if(oTags > rn || l_read_name < 1) return HLALA_BAMSCAN_CORRUPT_RECORD;
    if(flag & 4) return HLALA_BAMSCAN_OK;
    if(in.long_read_mode && (flag & 256)) return HLALA_BAMSCAN_OK;
    if(refID < 0 || refID >= in.n_ref) return HLALA_BAMSCAN_OK;
    const int32_t iv0 = in.ref_iv_off[refID], iv1 = in.ref_iv_off[refID + 1];
    if(iv1 <= iv0) return HLALA_BAMSCAN_OK;
    bool haveLen = false, parsed = false; uint32_t refLen = 0;
    int32_t as = 0; uint64_t hash = 0; uint32_t nameLen = 0, rank = 0, nd = 0, ex = 0;
    for(int32_t k = iv0; k < iv1; k++) {
        const int32_t ii = in.ref_iv[k];
        ex++;
        if(n_cigar == 0) continue;
        if(!haveLen) {
            haveLen = true;
            for(uint32_t c = 0; c < n_cigar; c++) { const uint32_t w = ld32(rec + oCigar + 4ull * c); const uint32_t op = w & 15u; if(op == 0 || op == 2 || op == 3 || op == 7 || op == 8) refLen += w >> 4; }
        }
        const int32_t a = position, z = (int32_t)((uint32_t)position + refLen - 1u);
        const int32_t lo = in.iv_start[ii], hi = in.iv_stop[ii];
        if(!((a >= lo && a <= hi) && (z >= lo && z <= hi))) continue;
        if(!in.long_read_mode && !(flag & 1)) return HLALA_BAMSCAN_UNPAIRED;
        const bool primary = !(flag & 256);
        if(!parsed) {
            parsed = true;
            bool haveAS = false;
            for(uint64_t p = oTags; p + 3 <= rn;) {
                const uint8_t t0 = rec[p], t1 = rec[p + 1], ty = rec[p + 2]; p += 3;
                uint64_t sz = 0; int64_t v = 0; bool isInt = true;
                switch(ty) {
                    case 'c': sz = 1; if(p + 1 <= rn) v = (int8_t)rec[p]; break;
                    case 'C': sz = 1; if(p + 1 <= rn) v = rec[p]; break;
                    case 's': sz = 2; if(p + 2 <= rn) v = (int16_t)ld16(rec + p); break;
                    case 'S': sz = 2; if(p + 2 <= rn) v = (uint16_t)ld16(rec + p); break;
                    case 'i': sz = 4; if(p + 4 <= rn) v = (int32_t)ld32(rec + p); break;
                    case 'I': sz = 4; if(p + 4 <= rn) v = ld32(rec + p); break;
                    case 'A': sz = 1; isInt = false; break;
                    case 'f': sz = 4; isInt = false; break;
                    case 'Z': case 'H': { isInt = false; uint64_t q = p; while(q < rn && rec[q]) q++; sz = q - p + 1; break; }
                    case 'B': { isInt = false; if(p + 5 > rn) return HLALA_BAMSCAN_CORRUPT_TAG; const uint8_t et = rec[p]; const uint32_t cnt = ld32(rec + p + 1);
                                const uint64_t es = (et == 'c' || et == 'C') ? 1 : (et == 's' || et == 'S') ? 2 : 4; sz = 5 + es * (uint64_t)cnt; break; }
                    default: return HLALA_BAMSCAN_UNKNOWN_TAG_TYPE;
                }
                if(p + sz > rn) return HLALA_BAMSCAN_CORRUPT_TAG;
                if(t0 == 'A' && t1 == 'S' && isInt) { as = (int32_t)v; haveAS = true; break; }
                p += sz;
            }
            if(!haveAS) return HLALA_BAMSCAN_NO_AS;
            while(nameLen < l_read_name && rec[oName + nameLen]) nameLen++;
            hash = bam_hash_name(rec + oName, nameLen) & in.hash_mask;
        }
        if(out && nd < cap) {
            hlala_bam_rec r;
            r.hash = hash; r.order = ((in.first_seq + ri) << 8) | (uint64_t)(rank < 255 ? rank : 255); r.rec_off = rec_off;
            r.contig = in.iv_contig[ii]; r.pos = (int32_t)((uint32_t)position - (uint32_t)lo); r.as = as; r.l_seq = primary ? l_seq : 0;
            r.n_cigar = (uint16_t)n_cigar; r.nameLen = (uint16_t)nameLen; r.which = (uint8_t)(in.long_read_mode ? 0 : ((flag & 64) ? 0 : 1));
            r.flags = (uint8_t)(((flag & 16) ? 1 : 0) | (primary ? 2 : 0)); r.l_read_name = (uint8_t)l_read_name; r.pad1 = 0;
            out[nd] = r;
        }
        rank++; nd++;
    }
    *n_desc = nd; *examined = ex; *compact = nd ? (uint32_t)oTags : 0u;
    return HLALA_BAMSCAN_OK;
}

// the slice size and the re-hop cap a call runs with (hlala_bam_scan_in: 0 = default; a negative max_rehops allows none)
HLALA_HD uint32_t scan_slice(const hlala_bam_scan_in& in) { return in.slice_bytes ? in.slice_bytes : BAM_DEFAULT_SLICE; }
HLALA_HD uint32_t scan_max_rehops(const hlala_bam_scan_in& in) { return in.max_rehops == 0 ? (uint32_t)BAM_DEFAULT_MAX_REHOPS : in.max_rehops < 0 ? 0u : (uint32_t)in.max_rehops; }

// The arguments of hlala_bam_scan / hlala_host_bam_scan_model, checked before anything runs.  Returns null or what is wrong.
inline const char* scan_check_args(const uint8_t* data, uint64_t n, uint64_t first, const hlala_bam_scan_in* in, const hlala_bam_rec* recs, int64_t cap_recs, const uint8_t* compact,
                                   uint64_t cap_compact, const hlala_bam_scan_stats* stats)
{
    if(!in || !stats || (n && !data) || cap_recs < 0 || (cap_recs && !recs) || (cap_compact && !compact)) return "null argument";
    if(n >= (1ull << 32)) return "more than 2^32 - 1 bytes in one call";
    if(first > n) return "first lies beyond n";
    const uint32_t s = scan_slice(*in);
    if(s < 64 || (s & (s - 1)) != 0) return "slice_bytes is not a power of two of at least 64";
    if(in->n_ref < 0 || in->n_intervals < 0) return "negative n_ref or n_intervals";
    if(in->n_ref > 0 && !in->ref_iv_off) return "null ref_iv_off";
    if(in->n_ref > 0) {
        if(in->ref_iv_off[0] != 0) return "ref_iv_off does not start at 0";
        for(int32_t r = 0; r < in->n_ref; r++) if(in->ref_iv_off[r + 1] < in->ref_iv_off[r]) return "ref_iv_off decreases";
        const int32_t m = in->ref_iv_off[in->n_ref];
        if(m > 0 && (!in->ref_iv || !in->iv_start || !in->iv_stop || !in->iv_contig)) return "null interval arrays";
        for(int32_t k = 0; k < m; k++) if(in->ref_iv[k] < 0 || in->ref_iv[k] >= in->n_intervals) return "ref_iv names an interval outside [0, n_intervals)";
    }
    return nullptr;
}

// the verdict of a call from what the passes found: the failing record with the lowest index wins (a bad length on the true chain fails the record that
// carries it; with `last`, bytes left behind the last complete record fail the record they begin)
inline void scan_verdict(int link_status, uint64_t link_record, uint64_t fail_key /* (record << 8) | status of the lowest failing parse, or all ones */, bool last, uint64_t consumed,
                         uint64_t n, uint64_t n_records, int32_t* status, int64_t* status_record)
{
    *status = HLALA_BAMSCAN_OK; *status_record = -1;
    if(fail_key != ~0ull) { *status = (int32_t)(fail_key & 255u); *status_record = (int64_t)(fail_key >> 8); return; }
    if(link_status == HLALA_BAMSCAN_BAD_LENGTH) { *status = HLALA_BAMSCAN_BAD_LENGTH; *status_record = (int64_t)link_record; return; }
    if(last && consumed != n) { *status = HLALA_BAMSCAN_BAD_LENGTH; *status_record = (int64_t)n_records; }
}

}  // namespace hlala_bamscan
#endif

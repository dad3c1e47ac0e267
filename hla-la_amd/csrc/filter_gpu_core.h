// filter_gpu_core.h -- the read / allele filters between the exon positions and the likelihoods (host_filters.cpp is the specification) restated per exon-position
// bucket, shared by the device kernels (kernel_filter.hip) and by the host model (filter_gpu_model.h; host_check.cpp: hlala_host_filter_model).  Plain inline
// functions, no HIP types: g++ and hipcc compile the same text.
//
// What makes the stage reproducible off the host.  The "first 20" of an exon position are the first first20_n entries after std::sort (+ std::reverse) of the reads'
// weighted-OK fractions, and those tie all the time; the order among ties is whatever libstdc++'s introsort leaves.  bam_fill_wide_core.h: fil_sort_wide runs that
// introsort step by step on 32-bit integers compared with `<`.  A bucket's doubles map to such integers without changing the outcome of one comparison:
//     score[i] = #{k in the bucket : w[k] < w[i]}
// For non-NaN doubles w[a] < w[b] holds exactly when score[a] < score[b] (`<` on them is a strict weak order: the score is the number of elements in the classes
// below one's own), and equal values, +0.0 / -0.0 included, get equal scores.  std::sort's steps depend on the sequence only through those comparisons, so
// fil_sort_wide on the scores leaves the places std::sort + std::reverse leave on the doubles.
//
// The formulation.  A bucket holds the positions that pass the mapq test, keyed by pos_exon, in ascending position index (the host's (read, position) order).  An
// allele is named by its representative: the bucket-local index of the first entry with the same genotype bytes (flt_same_bytes).  Counters are indexed by the
// representative; every counter is an integer, so no result depends on the order of atomics.
#ifndef HLALA_FILTER_GPU_CORE_H_
#define HLALA_FILTER_GPU_CORE_H_
#include "bam_fill_wide_core.h"

namespace hlala_filter {

constexpr uint32_t FLT_MAX_BUCKET = HLALA_FILTER_GPU_MAX_BUCKET;
static_assert(FLT_MAX_BUCKET == hlala_bamfill::FIL_WIDE_MAX, "a bucket is sorted by fil_sort_wide: the two capacities are one");

// what a malformed input is refused for (HLALA_E_ARG); the last two are defects of the stage itself and no input reaches them
constexpr uint32_t FLT_BAD_MAPQ = 1u, FLT_BAD_EXON = 2u, FLT_BAD_POS_OFF = 4u, FLT_BAD_GENO_OFF = 8u, FLT_BAD_NAN = 16u, FLT_BAD_INDEX = 32u, FLT_BAD_SORT = 64u;
constexpr uint32_t FLT_NO_REP = 0xFFFFFFFFu;
// the twelve counters of hlala_filter_stats as an array of 64-bit words, in the struct's order
enum { FS_CONSIDERED_POS = 0, FS_POS_WITH_REMOVED, FS_CONSIDERED_ALLELES, FS_REMOVED_ALLELES, FS_READS_KICKED, FS_READS_KICKED_ROBUST, FS_HC_POSITIONS, FS_HC_REMOVED, FS_BASES_USED,
       FS_STRAND_ENOUGH, FS_STRAND_REMOVED, FS_STRAND_POS_REMOVED, FS_N };
static_assert(sizeof(hlala_filter_stats) == FS_N * sizeof(int64_t), "hlala_filter_stats is twelve 64-bit counters");
// counts[6] of hlala_filter_positions_gpu
enum { FC_BUCKETS = 0, FC_SORTED, FC_LARGEST, FC_HEAPS, FC_BYTES_UP, FC_BYTES_DOWN, FC_N };

inline const char* flt_bad_text(uint32_t bad)
{
    if(bad & FLT_BAD_POS_OFF) return "pos_off is not ascending";
    if(bad & FLT_BAD_GENO_OFF) return "geno_off is not ascending";
    if(bad & FLT_BAD_MAPQ) return "a quality byte whose PhredToPCorrect lies outside [0, 1]";
    if(bad & FLT_BAD_EXON) return "a negative pos_exon";
    if(bad & FLT_BAD_NAN) return "a NaN in read_weighted_ok (std::sort is undefined there)";
    if(bad & FLT_BAD_INDEX) return "an index left its range";
    if(bad & FLT_BAD_SORT) return "the bucket sort overflowed";
    return "";
}

// What can be said about the arguments before a single array element is looked at.  nullptr: fine.  The ends of the two offset arrays are pinned here, their
// monotony is checked element by element (flt_check_read / flt_check_pos), and between them every offset lies in its range.
inline const char* flt_check_args(const hlala_exon_positions_out* pos, const hlala_filter_params* prm, const uint8_t* pos_use)
{
    if(!pos || !prm || !pos_use) return "null argument";
    if(pos->n_reads < 0 || pos->n_pos < 0 || pos->n_chars < 0) return "negative size";
    if(pos->n_reads == 0) return pos->n_pos == 0 ? nullptr : "positions without reads";
    if(!pos->pos_off || !pos->pos_exon || !pos->pos_mapq || !pos->geno_off || !pos->geno_chars || !pos->read_weighted_ok) return "null array";
    if(prm->long_read_strand_filter && (!pos->read_reverse || !pos->pos_mate)) return "the strand filter needs read_reverse";
    if(pos->pos_off[0] != 0 || pos->pos_off[pos->n_reads] != pos->n_pos) return "pos_off does not span [0, n_pos]";
    if(pos->geno_off[0] < 0 || pos->geno_off[pos->n_pos] > pos->n_chars) return "geno_off leaves [0, n_chars]";
    return nullptr;
}
// bytes of the caller's arrays that the rule reads / writes (counts[4], counts[5])
inline int64_t flt_bytes_up(const hlala_exon_positions_out* pos, const hlala_filter_params* prm)
{
    const int64_t nr = pos->n_reads, np = pos->n_pos;
    if(nr == 0) return 0;
    return 4 * (nr + 1) + 4 * np + np + (pos->pos_mate ? np : 0) + 4 * (np + 1) + (int64_t)pos->n_chars + 16 * nr + (prm->long_read_strand_filter ? 2 * nr : 0);
}
inline int64_t flt_bytes_down(const hlala_exon_positions_out* pos, const uint8_t* read_ignored) { return pos->n_reads == 0 ? 0 : (int64_t)pos->n_pos + (read_ignored ? (int64_t)pos->n_reads : 0); }

// ---- per read / per position (k_flt_mapq)
HLALA_HD double flt_weight(const double* wok, uint32_t r) { return (wok[2 * (size_t)r] + wok[2 * (size_t)r + 1]) / 2.0; }      // completeRead_weightedCharactersOK, :1535
HLALA_HD uint32_t flt_check_read(const int32_t* pos_off, const double* wok, uint32_t r)
{
    uint32_t bad = 0;
    if(pos_off[r + 1] < pos_off[r]) bad |= FLT_BAD_POS_OFF;
    const double w = flt_weight(wok, r);
    if(w != w) bad |= FLT_BAD_NAN;
    return bad;
}
// the read that owns position j: pos_off[r] <= j < pos_off[r + 1].  Bounded by log2(n_reads) steps and inside [0, n_reads) for ANY pos_off.
HLALA_HD uint32_t flt_read_of(const int32_t* pos_off, uint32_t n_reads, uint32_t j)
{
    uint32_t lo = 0, hi = n_reads;
    while(hi - lo > 1u) { const uint32_t mid = lo + (hi - lo) / 2u; if(pos_off[mid] >= 0 && (uint32_t)pos_off[mid] <= j) lo = mid; else hi = mid; }
    return lo;
}
// position j: *ok = mapqOK.  pc: PhredToPCorrect of every byte, built on the host with the host's exp / log.
HLALA_HD uint32_t flt_check_pos(const double* pc, const uint8_t* pos_mapq, const int32_t* pos_exon, const int32_t* geno_off, double min_mapq, uint32_t j, bool* ok)
{
    uint32_t bad = 0;
    const double m = pc[pos_mapq[j]];
    if(!((m >= 0) && (m <= 1))) bad |= FLT_BAD_MAPQ;                  // assert, :1526
    if(pos_exon[j] < 0) bad |= FLT_BAD_EXON;
    if(geno_off[j + 1] < geno_off[j]) bad |= FLT_BAD_GENO_OFF;
    *ok = m >= min_mapq;
    return bad;
}

// ---- alleles
// the genotype of position j as a range of geno_chars; a range that leaves [0, n_chars] comes back empty with *bad set (flt_check_pos and flt_check_args have
// refused such an input before anything looks at its bytes: the test never fires)
struct FltGeno { uint32_t at, len; };
HLALA_HD FltGeno flt_geno(const int32_t* geno_off, uint32_t n_chars, uint32_t j, uint32_t* bad)
{
    const int32_t g0 = geno_off[j], g1 = geno_off[j + 1];
    if(g0 < 0 || g1 < g0 || (uint32_t)g1 > n_chars) { *bad |= FLT_BAD_GENO_OFF; return FltGeno{0u, 0u}; }
    return FltGeno{(uint32_t)g0, (uint32_t)(g1 - g0)};
}
HLALA_HD bool flt_same_bytes(const uint8_t* geno_chars, FltGeno a, FltGeno b)
{
    if(a.len != b.len) return false;
    for(uint32_t k = 0; k < a.len; k++) if(geno_chars[a.at + k] != geno_chars[b.at + k]) return false;
    return true;
}
// std::string's operator<: unsigned bytes, a proper prefix first
HLALA_HD bool flt_less_bytes(const uint8_t* geno_chars, FltGeno a, FltGeno b)
{
    const uint32_t m = a.len < b.len ? a.len : b.len;
    for(uint32_t k = 0; k < m; k++) { const uint8_t x = geno_chars[a.at + k], y = geno_chars[b.at + k]; if(x != y) return x < y; }
    return a.len < b.len;
}

// ---- filterFirst20
HLALA_HD bool flt_first20_runs(const hlala_filter_params& p, uint32_t n) { return p.filter_first20 && n > 0 && !((int64_t)n < (int64_t)p.first20_n); }
HLALA_HD int32_t flt_score(const double* w, uint32_t n, uint32_t i) { const double wi = w[i]; int32_t s = 0; for(uint32_t k = 0; k < n; k++) s += w[k] < wi ? 1 : 0; return s; }
HLALA_HD bool flt_first20_kicks(const hlala_filter_params& p, uint32_t first20)
{
    const double first20_prop = (double)first20 / (double)(p.filter_first20 != 0);                   // sic: the bool (:1593)
    return first20_prop < p.first20_min_prop;
}
// ---- second phase
HLALA_HD bool flt_high_coverage_removes(const hlala_filter_params& p, uint32_t cnt, uint32_t count_position)
{
    const double aF = (double)cnt / (double)count_position;
    return (aF < p.high_coverage_min_freq) && p.high_coverage_filter;
}
HLALA_HD bool flt_strand_enough(const hlala_filter_params& p, uint32_t total) { return (int64_t)total >= (int64_t)p.strand_min_allele_coverage; }
HLALA_HD bool flt_strand_removes(const hlala_filter_params& p, uint32_t total, uint32_t rev)
{
    const uint32_t minStrand = rev < total - rev ? rev : total - rev;
    const double minStrandFreq = (double)minStrand / (double)total;
    return flt_strand_enough(p, total) && minStrandFreq < p.strand_min_freq;
}

}  // namespace hlala_filter
#endif

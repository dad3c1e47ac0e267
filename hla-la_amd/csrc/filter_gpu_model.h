// filter_gpu_model.h -- hlala_filter_positions_gpu without a device: the launches of kernel_filter.hip run serially over filter_gpu_core.h, in the device's formulation
// (buckets from a stable key sort, alleles named by representatives, two bucket phases with the per-read step between them), NOT a copy of host_filters.cpp.  Same
// arguments, return codes and outputs as the entry point; host_check.cpp exports it as hlala_host_filter_model, tools/filter_gpu_check.cpp holds it against
// hlala_filter_positions under ASan / UBSan.
//
// tie_rule 0: a bucket is ordered by fil_sort_wide on the scores (the rule).  tie_rule 1 (tests only): by a STABLE descending sort of the weights -- what a
// reformulation that ignores the library's tie order would do; the suite uses it to show that its buckets can tell the two apart.
#ifndef HLALA_FILTER_GPU_MODEL_H_
#define HLALA_FILTER_GPU_MODEL_H_
#include <algorithm>
#include <string>
#include <vector>

#include "filter_gpu_core.h"
#include "host_internal.h"

namespace hlala_filter {

// representatives of a bucket: ent[0, n) are its position indices; rep[i] = bucket-local index of the first entry with the genotype bytes of entry i
inline void model_reps(const hlala_exon_positions_out* pos, const uint32_t* ent, uint32_t n, std::vector<uint32_t>& rep, std::vector<uint32_t>& longIdx)
{
    uint32_t first[256];
    for(uint32_t b = 0; b < 256; b++) first[b] = FLT_NO_REP;
    rep.assign(n, FLT_NO_REP); longIdx.clear();
    const uint32_t nch = (uint32_t)pos->n_chars; uint32_t bad = 0;
    for(uint32_t i = 0; i < n; i++) {
        const FltGeno g = flt_geno(pos->geno_off, nch, ent[i], &bad);
        if(g.len == 1) { const uint8_t b = pos->geno_chars[g.at]; if(i < first[b]) first[b] = i; }
        else longIdx.push_back(i);
    }
    for(uint32_t i = 0; i < n; i++) { const FltGeno g = flt_geno(pos->geno_off, nch, ent[i], &bad); if(g.len == 1) rep[i] = first[pos->geno_chars[g.at]]; }
    for(size_t q = 0; q < longIdx.size(); q++) {
        const uint32_t i = longIdx[q]; uint32_t r = i;
        const FltGeno g = flt_geno(pos->geno_off, nch, ent[i], &bad);
        for(size_t q2 = 0; q2 < q; q2++) if(flt_same_bytes(pos->geno_chars, flt_geno(pos->geno_off, nch, ent[longIdx[q2]], &bad), g)) { r = longIdx[q2]; break; }
        rep[i] = r;
    }
}

inline int filter_model(const hlala_exon_positions_out* pos, const hlala_filter_params* prm, uint8_t* pos_use, uint8_t* read_ignored, hlala_filter_stats* stats, int64_t* counts,
                        int tie_rule, std::string* why)
{
    using namespace hlala_bamfill;
    why->clear();
    if(const char* a = flt_check_args(pos, prm, pos_use)) { *why = a; return HLALA_E_ARG; }
    if(tie_rule != 0 && tie_rule != 1) { *why = "tie_rule is 0 or 1"; return HLALA_E_ARG; }
    int64_t S[FS_N] = {0}, Cn[FC_N] = {0};
    const hlala_filter_params& P = *prm;
    const uint32_t nr = (uint32_t)pos->n_reads, np = (uint32_t)pos->n_pos;
    auto finish = [&]() {
        if(stats) memcpy(stats, S, sizeof(S));
        if(counts) { Cn[FC_BYTES_UP] = flt_bytes_up(pos, prm); Cn[FC_BYTES_DOWN] = flt_bytes_down(pos, read_ignored); memcpy(counts, Cn, sizeof(Cn)); }
        return HLALA_OK;
    };
    if(nr == 0) return finish();
    double pc[256]; hlala_host::filter_phred_table(pc);
    // ---- k_flt_mapq: per read and per position; nothing is written for a malformed input
    uint32_t bad = 0; int64_t maxExon = -1;
    std::vector<uint8_t> ok(np, 0); std::vector<uint32_t> posRead(np, 0);
    for(uint32_t r = 0; r < nr; r++) bad |= flt_check_read(pos->pos_off, pos->read_weighted_ok, r);
    for(uint32_t j = 0; j < np; j++) {
        bool o = false;
        bad |= flt_check_pos(pc, pos->pos_mapq, pos->pos_exon, pos->geno_off, P.min_per_position_mapq, j, &o);
        ok[j] = o; posRead[j] = flt_read_of(pos->pos_off, nr, j);
        if(o && pos->pos_exon[j] > maxExon) maxExon = pos->pos_exon[j];
    }
    if(bad) { *why = flt_bad_text(bad); return HLALA_E_ARG; }
    // ---- the key sort: (exon, position index) ascending over the positions that pass; bOff: the buckets
    const size_t nb = (size_t)(maxExon + 1);
    std::vector<uint32_t> bOff(nb + 1, 0);
    for(uint32_t j = 0; j < np; j++) if(ok[j]) bOff[(size_t)pos->pos_exon[j] + 1]++;
    uint32_t largest = 0;
    for(size_t e = 0; e < nb; e++) { if(bOff[e + 1] > largest) largest = bOff[e + 1]; if(bOff[e + 1]) Cn[FC_BUCKETS]++; bOff[e + 1] += bOff[e]; }
    Cn[FC_LARGEST] = largest;
    if(largest > FLT_MAX_BUCKET) {
        *why = "not available: an exon position with " + std::to_string(largest) + " entries, more than HLALA_FILTER_GPU_MAX_BUCKET = " + std::to_string(FLT_MAX_BUCKET);
        return HLALA_E_CAPACITY;
    }
    const uint32_t nOK = bOff[nb];
    std::vector<uint32_t> sorted(nOK);
    { std::vector<uint32_t> fill(bOff.begin(), bOff.end() - 1); for(uint32_t j = 0; j < np; j++) if(ok[j]) sorted[fill[(size_t)pos->pos_exon[j]]++] = j; }
    // ---- k_flt_first20, a bucket at a time: representatives always; the sort and the kicks where the filter runs
    std::vector<uint32_t> entRep(nOK, 0), posFlag(np, 0);         // entRep: bucket-local representative; posFlag[j]: the slot of entIgnore that holds the allele of position j
    std::vector<uint8_t> entIgnore(nOK, 0);                        // per (bucket, representative), at slot b0 + rep
    std::vector<int32_t> kicked(nr, 0), kickedRobust(nr, 0);
    std::vector<uint32_t> rep, longIdx, cnt, rev; std::vector<double> w; std::vector<int32_t> score; std::vector<uint16_t> place; uint32_t stack[FIL_WIDE_STACK_WORDS];
    for(size_t e = 0; e < nb; e++) {
        const uint32_t b0 = bOff[e], n = bOff[e + 1] - b0;
        if(n == 0) continue;
        const uint32_t* ent = &sorted[b0];
        model_reps(pos, ent, n, rep, longIdx);
        for(uint32_t i = 0; i < n; i++) { entRep[b0 + i] = rep[i]; posFlag[ent[i]] = b0 + rep[i]; }
        if(!flt_first20_runs(P, n)) continue;
        w.resize(n); score.resize(n); place.resize(n);
        for(uint32_t i = 0; i < n; i++) w[i] = flt_weight(pos->read_weighted_ok, posRead[ent[i]]);
        for(uint32_t i = 0; i < n; i++) { score[i] = flt_score(w.data(), n, i); place[i] = (uint16_t)i; }
        if(tie_rule == 0) {
            const uint32_t h = fil_sort_wide(score.data(), place.data(), n, stack);
            if(h == FIL_WIDE_OVERFLOW) { *why = flt_bad_text(FLT_BAD_SORT); return HLALA_E_ARG; }
            Cn[FC_HEAPS] += h;
        } else std::stable_sort(place.begin(), place.end(), [&](uint16_t a, uint16_t b) { return w[a] > w[b]; });
        Cn[FC_SORTED]++;
        cnt.assign(n, 0);                                           // low half: among the first 20; high half: kicked entries
        for(int64_t i = 0; i < (int64_t)P.first20_n; i++) { const uint32_t pl = place[(size_t)i]; if(pl >= n) { *why = flt_bad_text(FLT_BAD_INDEX); return HLALA_E_ARG; } cnt[rep[pl]] += 1u; }
        bool kickedOne = false;
        for(uint32_t i = 0; i < n; i++) {
            S[FS_CONSIDERED_ALLELES]++;
            if(flt_first20_kicks(P, cnt[rep[i]] & 0xFFFFu)) { entIgnore[b0 + rep[i]] = 1; kicked[posRead[ent[i]]]++; cnt[rep[i]] += 1u << 16; kickedOne = true; S[FS_REMOVED_ALLELES]++; }
        }
        for(uint32_t i = 0; i < n; i++) if((cnt[rep[i]] >> 16) >= 2u) kickedRobust[posRead[ent[i]]]++;
        S[FS_CONSIDERED_POS]++;
        if(kickedOne) S[FS_POS_WITH_REMOVED]++;
    }
    // ---- k_flt_reads
    std::vector<uint8_t> ignoreRead(nr, 0);
    if(P.filter_first20) for(uint32_t r = 0; r < nr; r++) {
        if(kicked[r] > P.first20_limit_per_read) S[FS_READS_KICKED]++;
        if(kickedRobust[r] > P.first20_limit_per_read) { S[FS_READS_KICKED_ROBUST]++; ignoreRead[r] = 1; }
    }
    // ---- k_flt_coverage, a bucket at a time
    std::vector<uint32_t> removed;
    for(size_t e = 0; e < nb; e++) {
        const uint32_t b0 = bOff[e], n = bOff[e + 1] - b0;
        if(n == 0) continue;
        const uint32_t* ent = &sorted[b0];
        cnt.assign(n, 0); rev.assign(n, 0);
        uint32_t count_position = 0;
        for(uint32_t i = 0; i < n; i++) {
            const uint32_t j = ent[i], r = posRead[j], a = entRep[b0 + i];
            if(ignoreRead[r] || entIgnore[b0 + a]) continue;
            cnt[a]++; count_position++;
            if(P.long_read_strand_filter && pos->read_reverse[2 * (size_t)r + (pos->pos_mate[j] == 2 ? 1 : 0)]) rev[a]++;
        }
        if(count_position == 0) continue;
        if((int64_t)count_position >= (int64_t)P.high_coverage_min_coverage) {
            S[FS_HC_POSITIONS]++;
            for(uint32_t a = 0; a < n; a++) if(cnt[a] && flt_high_coverage_removes(P, cnt[a], count_position)) { entIgnore[b0 + a] = 1; S[FS_HC_REMOVED] += cnt[a]; }
        }
        if(P.long_read_strand_filter) {
            removed.clear();
            for(uint32_t a = 0; a < n; a++) {
                if(!cnt[a]) continue;
                if(flt_strand_enough(P, cnt[a])) S[FS_STRAND_ENOUGH]++;
                if(flt_strand_removes(P, cnt[a], rev[a])) { entIgnore[b0 + a] = 1; S[FS_STRAND_REMOVED]++; removed.push_back(a); }
            }
            // visited at or after the first removal in std::string order: some removed allele is not greater
            for(uint32_t a = 0; a < n; a++) {
                if(!cnt[a]) continue;
                bool after = false;
                uint32_t gb = 0;
                const FltGeno ga = flt_geno(pos->geno_off, (uint32_t)pos->n_chars, ent[a], &gb);
                for(uint32_t m : removed) if(!flt_less_bytes(pos->geno_chars, ga, flt_geno(pos->geno_off, (uint32_t)pos->n_chars, ent[m], &gb))) { after = true; break; }
                if(after) S[FS_STRAND_POS_REMOVED]++;
            }
        }
    }
    // ---- k_flt_use
    for(uint32_t j = 0; j < np; j++) {
        const bool use = ok[j] && !entIgnore[posFlag[j]] && !ignoreRead[posRead[j]];
        pos_use[j] = use ? 1 : 0;
        if(use) S[FS_BASES_USED]++;
    }
    if(read_ignored) for(uint32_t r = 0; r < nr; r++) read_ignored[r] = ignoreRead[r];
    return finish();
}

}  // namespace hlala_filter
#endif

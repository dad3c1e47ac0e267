// bam_fill_model.h -- the passes of kernel_bamfill.hip written serially over bam_fill_core.h: rank and sizes per read, the sizes of host units, four prefix sums, the
// chains' sources, then per window the chain scalars, CIGARs, names, bases and qualities -- a loop where the device has a grid.  What hlala_host_bam_fill_model
// (host_check.cpp) exports, what the CPU suite holds against a plain-Python statement of the rule, what the device is held against bit for bit -- and, built with
// sanitizers into tools/bam_fill_check.cpp, what shows the argument check refusing malformed inputs before a record byte is read.
//
// The wide layout (bam_fill_wide_core.h; hlala_host_bam_fill_model_wide): fill_model_create_wide orders both mates of a wide unit with fil_sort_wide, as k_fil_wide_rank
// does, and every other unit as above; the window passes follow chain_src and are the same.  fil_adversary makes the scores that drive std::sort into its heap sort.
#ifndef HLALA_BAM_FILL_MODEL_H_
#define HLALA_BAM_FILL_MODEL_H_
#include <algorithm>
#include <chrono>
#include <cstring>
#include <numeric>
#include <vector>

#include "bam_fill_core.h"
#include "bam_fill_wide_core.h"

namespace hlala_bamfill {

// what the device keeps between hlala_bam_fill_create and its windows
struct FillLayout {
    std::vector<uint32_t> chain_src;       // [chain] the descriptor the chain is written from; FIL_HOST for a chain of a host unit
    std::vector<int64_t> chain_cig;        // [chain] where its CIGAR starts
    std::vector<int32_t> read_primary;     // [read]
};

// the mate's records in the order sortChainsInSeeds leaves: by counting, as a lane of k_fil_rank does.  order[rank] = place in the unit; returns how many there are
inline uint32_t fil_rank_serial(const hlala_bam_rec* U, uint32_t count, int mate, uint32_t order[FIL_MAX_MATE])
{
    uint32_t at[FIL_MAX_MATE], n = 0;
    for(uint32_t k = 0; k < count; k++) if(U[k].which == mate && n < FIL_MAX_MATE) at[n++] = k;
    for(uint32_t a = 0; a < n; a++) {
        uint32_t rank = 0;
        for(uint32_t b = 0; b < n; b++) if(fil_before(U[at[b]].as, at[b], U[at[a]].as, at[a])) rank++;
        order[rank] = at[a];
    }
    return n;
}

// what a wide mate is sorted in: scores and places in file order, the stack of fil_sort_wide
struct WideScratch { std::vector<int32_t> score; std::vector<uint16_t> place; uint32_t stack[FIL_WIDE_STACK_WORDS]; };
// the mate's records of a wide unit in the order sortChainsInSeeds leaves, as k_fil_wide_rank finds it.  order[rank] = place in the unit; *heaps: heap sorts entered
inline uint32_t fil_order_wide(const hlala_bam_rec* U, uint32_t count, int mate, WideScratch& X, std::vector<uint32_t>& order, uint32_t* heaps)
{
    X.score.clear(); X.place.clear();
    for(uint32_t k = 0; k < count && X.score.size() < FIL_WIDE_MAX; k++) if(U[k].which == mate) { X.score.push_back(U[k].as); X.place.push_back((uint16_t)k); }
    const uint32_t n = (uint32_t)X.score.size();
    const uint32_t h = fil_sort_wide(X.score.data(), X.place.data(), n, X.stack);
    if(heaps) *heaps = h;
    order.resize(std::max<size_t>(order.size(), n));
    for(uint32_t k = 0; k < n; k++) order[k] = X.place[k];
    return n;
}
inline bool fil_unit_is_wide(const hlala_bam_rec* U, uint32_t count, uint32_t* longest)
{
    uint32_t m[2] = {0, 0};
    for(uint32_t k = 0; k < count; k++) m[U[k].which & 1]++;
    if(longest) *longest = std::max(m[0], m[1]);
    return fil_is_wide(count, m[0], m[1]);
}
// McIlroy's adversary ("A Killer Adversary for Quicksort") run against std::sort itself on the places 0 .. n - 1: every element is undecided until a comparison needs
// its value, and the one the sort seems to use as its pivot is given the next small value.  What is left in score[] makes std::sort's comparisons come out the same
// way again: for n >= 64 they spend its depth limit and enter the heap sort.
inline void fil_adversary(uint32_t n, int32_t* score)
{
    const int32_t gas = (int32_t)n;
    std::vector<int32_t> val(n, gas); std::vector<uint32_t> idx(n); std::iota(idx.begin(), idx.end(), 0u);
    int32_t solid = 0; uint32_t candidate = 0;
    std::sort(idx.begin(), idx.end(), [&](uint32_t x, uint32_t y) {
        if(val[x] == gas && val[y] == gas) val[x == candidate ? x : y] = solid++;
        if(val[x] == gas) candidate = x; else if(val[y] == gas) candidate = y;
        return val[x] < val[y];
    });
    for(uint32_t i = 0; i < n; i++) score[i] = val[i];
}

// max_mate 0: the layout of hlala_bam_fill_create; otherwise that of hlala_bam_fill_create_wide.  wide[4] (may be null): wide units, wide reads, the longest mate, 0
inline int fill_model_create_any(const hlala_bam_fill_in* in, int32_t max_mate, int64_t* read_off, int64_t* chain_off, int64_t* cigar_count, int64_t* name_off, FillLayout* L,
                                 hlala_bam_fill_stats* stats, int64_t* wide, const char** why)
{
    const char* bad = max_mate ? fil_check_args_wide(in, max_mate, read_off, chain_off, cigar_count, name_off, stats) : fil_check_args(in, read_off, chain_off, cigar_count, name_off, stats);
    if(wide) wide[0] = wide[1] = wide[2] = wide[3] = 0;
    if(why) *why = bad;
    if(bad) return HLALA_E_ARG;
    memset(stats, 0, sizeof(*stats));
    L->chain_src.clear(); L->chain_cig.clear(); L->read_primary.clear();
    if(in->n_units == 0) return HLALA_OK;
    const int nm = fil_nm(in->long_read_mode);
    const size_t nU = (size_t)in->n_units, nR = nU * (size_t)nm;
    // ---- rank + sizes, the sizes of host units
    read_off[0] = chain_off[0] = cigar_count[0] = name_off[0] = 0;
    int64_t host = 0;
    std::vector<uint32_t> order(FIL_MAX_MATE); WideScratch X;
    auto ordered = [&](const hlala_bam_rec* U, uint32_t count, int m, bool isWide) { return isWide ? fil_order_wide(U, count, m, X, order, nullptr) : fil_rank_serial(U, count, m, order.data()); };
    for(size_t u = 0; u < nU; u++) {
        if(in->unit_first[u] == FIL_HOST) {
            const int64_t* hs = in->host_sizes + host * (3 * nm + 1); host++;
            for(int m = 0; m < nm; m++) { const size_t r = u * (size_t)nm + (size_t)m; read_off[r + 1] = hs[3 * m]; chain_off[r + 1] = hs[3 * m + 1]; cigar_count[r + 1] = hs[3 * m + 2]; }
            name_off[u + 1] = hs[3 * nm];
            continue;
        }
        const hlala_bam_rec* U = in->recs + in->unit_first[u]; const uint32_t count = in->unit_count[u];
        name_off[u + 1] = (int64_t)U[0].nameLen + 1;
        uint32_t longest = 0;
        const bool isWide = max_mate != 0 && fil_unit_is_wide(U, count, &longest);
        if(isWide && wide) { wide[0]++; wide[1] += nm; wide[2] = std::max<int64_t>(wide[2], longest); }
        for(int m = 0; m < nm; m++) {
            const size_t r = u * (size_t)nm + (size_t)m;
            const uint32_t n = ordered(U, count, m, isWide);
            int64_t cg = 0, ls = 0; bool found = false;
            for(uint32_t k = 0; k < n; k++) { cg += U[order[k]].n_cigar; if(!found && (U[order[k]].flags & 2)) { found = true; ls = U[order[k]].l_seq; } }
            read_off[r + 1] = ls; chain_off[r + 1] = n; cigar_count[r + 1] = cg;
        }
    }
    // ---- the prefix sums
    for(size_t r = 0; r < nR; r++) { read_off[r + 1] += read_off[r]; chain_off[r + 1] += chain_off[r]; cigar_count[r + 1] += cigar_count[r]; }
    for(size_t u = 0; u < nU; u++) name_off[u + 1] += name_off[u];
    // ---- the chains' sources
    const size_t nC = (size_t)chain_off[nR];
    L->chain_src.assign(nC, FIL_HOST); L->chain_cig.assign(nC, 0); L->read_primary.assign(nR, 0);
    for(size_t u = 0; u < nU; u++) {
        if(in->unit_first[u] == FIL_HOST) continue;
        const hlala_bam_rec* U = in->recs + in->unit_first[u]; const uint32_t count = in->unit_count[u];
        const bool isWide = max_mate != 0 && fil_unit_is_wide(U, count, nullptr);
        for(int m = 0; m < nm; m++) {
            const size_t r = u * (size_t)nm + (size_t)m;
            const uint32_t n = ordered(U, count, m, isWide);
            int64_t cg = cigar_count[r]; bool found = false;
            for(uint32_t k = 0; k < n; k++) {
                const size_t c = (size_t)chain_off[r] + k;
                L->chain_src[c] = in->unit_first[u] + order[k]; L->chain_cig[c] = cg; cg += U[order[k]].n_cigar;
                if(!found && (U[order[k]].flags & 2)) { found = true; L->read_primary[r] = (int32_t)c; }
            }
        }
    }
    stats->n_units = in->n_units; stats->n_host_units = in->n_host_units; stats->n_reads = (int64_t)nR; stats->n_chains = (int64_t)nC; stats->n_cigar = cigar_count[nR];
    stats->n_bases = read_off[nR]; stats->n_name_bytes = name_off[nU];
    return HLALA_OK;
}

inline int fill_model_create(const hlala_bam_fill_in* in, int64_t* read_off, int64_t* chain_off, int64_t* cigar_count, int64_t* name_off, FillLayout* L, hlala_bam_fill_stats* stats,
                             const char** why)
{
    return fill_model_create_any(in, 0, read_off, chain_off, cigar_count, name_off, L, stats, nullptr, why);
}
inline int fill_model_create_wide(const hlala_bam_fill_in* in, int32_t max_mate, int64_t* read_off, int64_t* chain_off, int64_t* cigar_count, int64_t* name_off, FillLayout* L,
                                  hlala_bam_fill_stats* stats, int64_t* wide, const char** why)
{
    if(max_mate == 0) { if(why) *why = "max_mate outside (16, 4096]"; return HLALA_E_ARG; }
    return fill_model_create_any(in, max_mate, read_off, chain_off, cigar_count, name_off, L, stats, wide, why);
}

// the slices of units [u0, u0 + n); the offsets are those fill_model_create wrote
inline int fill_model_window(const hlala_bam_fill_in* in, const FillLayout* L, const int64_t* read_off, const int64_t* chain_off, const int64_t* cigar_count, const int64_t* name_off,
                             int64_t u0, int64_t n, const hlala_bam_fill_out* out, const char** why)
{
    if(why) *why = nullptr;
    if(u0 < 0 || n < 0 || u0 + n > in->n_units) { if(why) *why = "units outside the sample"; return HLALA_E_ARG; }
    if(n == 0) return HLALA_OK;
    const bool need = out && out->read_primary && out->read_quals && (in->packed ? out->read_bases_packed : out->read_bases) && out->chain_contig && out->chain_pos && out->chain_offset &&
                      out->chain_as && out->chain_reverse && out->cigar_off_end && out->cigar && out->name_chars;
    if(!need) { if(why) *why = "null argument"; return HLALA_E_ARG; }
    const int nm = fil_nm(in->long_read_mode);
    const size_t r0 = (size_t)u0 * (size_t)nm, r1 = (size_t)(u0 + n) * (size_t)nm;
    const int64_t b0 = read_off[r0], c0 = chain_off[r0], g0 = cigar_count[r0], n0 = name_off[u0], p0 = fil_packed_at(b0, (int64_t)r0);
    const uint8_t* B = in->bytes; const uint64_t nB = in->n_bytes;
    // the device clears a window's staging before its passes: the ranges of host units read as zeros
    memset(out->read_primary, 0, (r1 - r0) * 4); memset(out->read_quals, 0, (size_t)(read_off[r1] - b0));
    if(in->packed) memset(out->read_bases_packed, 0, (size_t)(fil_packed_at(read_off[r1], (int64_t)r1) - p0)); else memset(out->read_bases, 0, (size_t)(read_off[r1] - b0));
    const size_t nc = (size_t)(chain_off[r1] - c0);
    memset(out->chain_contig, 0, nc * 4); memset(out->chain_pos, 0, nc * 4); memset(out->chain_offset, 0, nc * 4); memset(out->chain_as, 0, nc * 4); memset(out->chain_reverse, 0, nc);
    memset(out->cigar_off_end, 0, nc * 8); memset(out->cigar, 0, (size_t)(cigar_count[r1] - g0) * 4); memset(out->name_chars, 0, (size_t)(name_off[u0 + n] - n0));
    // ---- chain scalars, CIGAR words
    for(size_t c = (size_t)c0; c < (size_t)c0 + nc; c++) {
        const uint32_t g = L->chain_src[c];
        if(g == FIL_HOST) continue;
        const hlala_bam_rec& x = in->recs[g]; const size_t k = c - (size_t)c0;
        out->chain_contig[k] = x.contig; out->chain_pos[k] = x.pos; out->chain_offset[k] = 0; out->chain_as[k] = x.as; out->chain_reverse[k] = (uint8_t)(x.flags & 1);
        out->cigar_off_end[k] = L->chain_cig[c] + x.n_cigar;
        for(uint32_t w = 0; w < x.n_cigar; w++) out->cigar[(size_t)(L->chain_cig[c] - g0) + w] = fil_word(B, nB, fil_cigar_at(x) + 4ull * w);
    }
    // ---- names
    for(int64_t u = u0; u < u0 + n; u++) {
        if(in->unit_first[u] == FIL_HOST) continue;
        const hlala_bam_rec& x = in->recs[in->unit_first[u]]; char* to = out->name_chars + (name_off[u] - n0);
        for(uint32_t i = 0; i < x.nameLen; i++) to[i] = (char)fil_byte(B, nB, x.rec_off + FIL_NAME_AT + i);
        to[x.nameLen] = 0;
    }
    // ---- bases and qualities of the primary
    for(size_t r = r0; r < r1; r++) {
        if(in->unit_first[r / (size_t)nm] == FIL_HOST) continue;
        out->read_primary[r - r0] = L->read_primary[r];
        const hlala_bam_rec& x = in->recs[L->chain_src[(size_t)L->read_primary[r]]];
        const int32_t ls = (int32_t)(read_off[r + 1] - read_off[r]);
        const uint64_t s4 = fil_seq_at(x), ql = fil_qual_at(x, ls);
        if(in->packed) { uint8_t* to = out->read_bases_packed + (fil_packed_at(read_off[r], (int64_t)r) - p0); for(int32_t i = 0; i < (ls + 1) / 2; i++) to[i] = fil_byte(B, nB, s4 + (uint64_t)i); }
        else { uint8_t* to = out->read_bases + (read_off[r] - b0); for(int32_t i = 0; i < ls; i++) { const uint8_t b = fil_byte(B, nB, s4 + (uint64_t)(i >> 1)); to[i] = fil_base((i & 1) ? (b & 15u) : (b >> 4)); } }
        uint8_t* qs = out->read_quals + (read_off[r] - b0);
        for(int32_t i = 0; i < ls; i++) qs[i] = fil_qual(fil_byte(B, nB, ql + (uint64_t)i));
    }
    return HLALA_OK;
}

}  // namespace hlala_bamfill
#endif

// bam_nameorder_model.h -- the ordering passes of kernel_bamnameorder.hip written serially over bam_nameorder_core.h: per round the keys of the unresolved names, a stable
// sort by (segment, key), mark, the scan, scatter -- a loop where the device has a grid.  What hlala_host_bam_name_order_model (host_check.cpp) exports, what the CPU
// suite holds against Python's own sorted(), what the device is held against bit for bit -- and, built with sanitizers into tools/bam_nameorder_check.cpp, what shows
// the argument check refusing malformed names before one of them is read.
#ifndef HLALA_BAM_NAMEORDER_MODEL_H_
#define HLALA_BAM_NAMEORDER_MODEL_H_
#include <algorithm>
#include <chrono>
#include <cstring>
#include <vector>

#include "bam_nameorder_core.h"

namespace hlala_nameorder {

inline int name_order_model(const uint64_t* name_off, const uint32_t* name_len, int64_t n, const uint8_t* bytes, size_t n_bytes, uint32_t* order, hlala_bam_name_order_stats* stats,
                            const char** why)
{
    uint32_t maxLen = 0;
    const char* bad = nam_check_args(name_off, name_len, n, bytes, n_bytes, order, stats, &maxLen);
    if(why) *why = bad;
    if(bad) return HLALA_E_ARG;
    const auto t0 = std::chrono::steady_clock::now();
    memset(stats, 0, sizeof(*stats));
    stats->n = n;
    // slot j of the working set: the name idx[j], its segment seg[j] (ascending with j), the place gp[j] of the final order the slot stands for.  A sort moves names
    // between the slots of one segment only, so gp stays with the slot.
    size_t a = (size_t)n;
    std::vector<uint32_t> idx(a), seg(a, 0), gp(a);
    for(size_t j = 0; j < a; j++) idx[j] = gp[j] = (uint32_t)j;
    const int64_t maxRounds = nam_max_rounds(maxLen);
    std::vector<uint64_t> key, k; std::vector<uint32_t> p, idx2, seg2, gp2, newIdx; std::vector<uint8_t> start, keep;
    for(uint32_t r = 0; a > 0; r++) {
        if((int64_t)r >= maxRounds) { if(why) *why = "names unresolved after the last round"; return HLALA_E_DEVICE; }      // (cannot happen)
        stats->n_rounds++;
        // ---- key
        key.resize(a);
        for(size_t j = 0; j < a; j++) key[j] = nam_key(bytes, n_bytes, name_off[idx[j]], name_len[idx[j]], r);
        // ---- sort: stable, by (segment, key)
        p.resize(a);
        for(size_t j = 0; j < a; j++) p[j] = (uint32_t)j;
        std::stable_sort(p.begin(), p.end(), [&](uint32_t x, uint32_t y) { return seg[x] != seg[y] ? seg[x] < seg[y] : key[x] < key[y]; });
        // ---- mark
        k.resize(a); newIdx.resize(a); start.resize(a); keep.resize(a);
        for(size_t j = 0; j < a; j++) { k[j] = key[p[j]]; newIdx[j] = idx[p[j]]; }
        for(size_t j = 0; j < a; j++) start[j] = nam_split(j, j ? seg[j - 1] : 0, seg[j], j ? k[j - 1] : 0, k[j]) ? 1 : 0;
        for(size_t j = 0; j < a; j++) {
            const bool next = j + 1 == a || start[j + 1], ended = nam_ended(k[j]);
            keep[j] = !((start[j] && next) || ended);
            if(!start[j] && ended) stats->n_equal_names++;
        }
        // ---- scan + scatter: final names to their places, the others to the front of the next round's working set
        idx2.clear(); seg2.clear(); gp2.clear();
        uint32_t segs = 0;
        for(size_t j = 0; j < a; j++) {
            if(!keep[j]) { order[gp[j]] = newIdx[j]; continue; }
            if(start[j]) segs++;
            idx2.push_back(newIdx[j]); seg2.push_back(segs - 1); gp2.push_back(gp[j]);
        }
        idx.swap(idx2); seg.swap(seg2); gp.swap(gp2);
        a = idx.size();
    }
    stats->ms_wall = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return HLALA_OK;
}

}  // namespace hlala_nameorder
#endif

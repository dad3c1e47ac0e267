// bam_group_model.h -- the grouping passes of kernel_bamgroup.hip written serially over bam_group_core.h: append (the per-record arrays and the name arena), a stable
// sort on the hash, mark, run ids, fold, emit -- a loop where the device has a grid.  What hlala_host_bam_group_model (host_check.cpp) exports, what the CPU suite
// holds against an expectation written in Python, what the device is held against bit for bit -- and, built with sanitizers into tools/bam_group_check.cpp, what
// shows the argument check refusing malformed descriptors before one of them is read through.
#ifndef HLALA_BAM_GROUP_MODEL_H_
#define HLALA_BAM_GROUP_MODEL_H_
#include <algorithm>
#include <chrono>
#include <cstring>
#include <vector>

#include "bam_group_core.h"

namespace hlala_bamgroup {

inline int group_model(const hlala_bam_rec* recs, int64_t n, const uint8_t* bytes, size_t n_bytes, int32_t long_read_mode, uint32_t* perm, uint8_t* flag, hlala_bam_group_stats* stats,
                       const char** why)
{
    const char* bad = grp_check_args(recs, n, bytes, n_bytes, perm, flag, stats);
    if(why) *why = bad;
    if(bad) return HLALA_E_ARG;
    const auto t0 = std::chrono::steady_clock::now();
    memset(stats, 0, sizeof(*stats));
    stats->n_recs = n;
    const size_t N = (size_t)n;
    // ---- append: hash, meta, the names one behind the other (offsets: the exclusive sum of nameLen)
    std::vector<uint64_t> hash(N), nameOff(N + 1, 0); std::vector<uint32_t> meta(N);
    for(size_t i = 0; i < N; i++) { hash[i] = recs[i].hash; meta[i] = grp_meta(recs[i].nameLen, recs[i].which, recs[i].flags); nameOff[i + 1] = nameOff[i] + recs[i].nameLen; }
    std::vector<uint8_t> arena((size_t)nameOff[N] + 1);
    for(size_t i = 0; i < N; i++) memcpy(arena.data() + nameOff[i], bytes + recs[i].rec_off + GRP_NAME_AT, recs[i].nameLen);
    const uint64_t arenaBytes = nameOff[N];
    // ---- sort: stable, on the hash alone (the descriptors come in ascending order)
    std::vector<uint32_t> p(N);
    for(size_t i = 0; i < N; i++) p[i] = (uint32_t)i;
    std::stable_sort(p.begin(), p.end(), [&](uint32_t a, uint32_t b) { return hash[a] < hash[b]; });
    // ---- mark: run starts, and records whose name is not their predecessor's
    std::vector<uint32_t> start(N + 1, 0); std::vector<uint8_t> neq(N, 0);
    for(size_t i = 0; i < N; i++) {
        const uint32_t g = p[i], gp = i ? p[i - 1] : g;
        const bool s = grp_run_start(i, hash[gp], hash[g]);
        start[i] = s ? 1u : 0u;
        neq[i] = !s && !grp_same_name(arena.data(), arenaBytes, nameOff[g], meta_name_len(meta[g]), nameOff[gp], meta_name_len(meta[gp]));
    }
    // ---- run ids: the exclusive sum of the start flags
    std::vector<uint32_t> runOff(N + 1, 0);
    for(size_t i = 0; i < N; i++) runOff[i + 1] = runOff[i] + start[i];
    const size_t nRuns = runOff[N];
    // ---- fold
    std::vector<uint32_t> word(nRuns, 0);
    for(size_t i = 0; i < N; i++) word[runOff[i] + start[i] - 1] |= grp_fold_bits(neq[i] != 0, meta[p[i]]);
    // ---- emit
    for(size_t i = 0; i < N; i++) {
        perm[i] = p[i];
        const uint8_t f = start[i] ? grp_run_flag(word[runOff[i]], long_read_mode) : (uint8_t)0;
        flag[i] = f;
        if(f & GRP_COLLIDED) stats->n_collided_runs++; else if(f & GRP_COMPLETE) stats->n_units_complete++; else if(f & GRP_START) stats->n_units_incomplete++;
    }
    stats->n_runs = (int64_t)nRuns;
    stats->ms_wall = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return HLALA_OK;
}

}  // namespace hlala_bamgroup
#endif

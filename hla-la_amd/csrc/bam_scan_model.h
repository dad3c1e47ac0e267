// bam_scan_model.h -- the BAM record pass of kernel_bamscan.hip written serially over bam_scan_core.h: the same passes (guess, link, starts, parse, two
// scans, emit) over the same per-slice and per-record arrays, a loop where the device has a grid.  What hlala_host_bam_scan_model (host_check.cpp) exports, what
// the CPU suite holds against an expectation written in Python, what the device is held against bit for bit -- and, built with sanitizers into
// tools/bam_scan_check.cpp, what shows the core bounded on malformed input before such input goes to a kernel.
#ifndef HLALA_BAM_SCAN_MODEL_H_
#define HLALA_BAM_SCAN_MODEL_H_
#include <chrono>
#include <cstring>
#include <vector>

#include "bam_scan_core.h"

namespace hlala_bamscan {

inline int scan_model(const uint8_t* data, size_t n, size_t first, int32_t last, const hlala_bam_scan_in* in, hlala_bam_rec* recs, int64_t cap_recs, uint8_t* compact, size_t cap_compact,
                      hlala_bam_scan_stats* stats, const char** why)
{
    const char* bad = scan_check_args(data, n, first, in, recs, cap_recs, compact, cap_compact, stats);
    if(why) *why = bad;
    if(bad) return HLALA_E_ARG;
    const auto t0 = std::chrono::steady_clock::now();
    memset(stats, 0, sizeof(*stats));
    stats->status_record = -1;
    const uint64_t S = scan_slice(*in), N = n;
    const uint32_t maxRehops = scan_max_rehops(*in);
    const size_t nSlices = (size_t)((N + S - 1) / S);
    stats->n_slices = (int64_t)nSlices;
    // ---- guess: per slice the lowest plausible offset, and the hop from it to the slice end
    std::vector<uint32_t> g(nSlices, BAM_NONE), x(nSlices, BAM_NONE), cf(nSlices, 0);
    for(size_t s = 0; s < nSlices; s++) {
        const uint64_t lim = (s + 1) * S, a = s * S > first ? s * S : first, z = lim < N ? lim : N;
        for(uint64_t p = a; p < z; p++)
            if(bam_plausible(data, N, p, in->n_ref)) { g[s] = (uint32_t)p; break; }
        if(g[s] == BAM_NONE) continue;
        uint64_t q = 0; uint32_t c = 0;
        const int how = bam_hop(data, N, g[s], lim, nullptr, 0, &q, &c);
        x[s] = (uint32_t)q; cf[s] = c | ((uint32_t)how << 30);
    }
    // ---- link: the true chain from `first`, slice by slice
    std::vector<uint32_t> entry(nSlices, BAM_NONE), prefix(nSlices, 0);
    uint64_t cur = first; uint32_t idx = 0, rehops = 0; bool ended = false; int linkStatus = HLALA_BAMSCAN_OK; uint64_t linkRecord = 0;
    for(size_t s = 0; s < nSlices; s++) {
        const uint64_t lim = (s + 1) * S;
        prefix[s] = idx;
        if(ended || cur >= lim) continue;
        uint64_t q = 0; uint32_t c = 0; int how = 0;
        if(g[s] != BAM_NONE && g[s] == (uint32_t)cur) { q = x[s]; c = cf[s] & 0x3FFFFFFFu; how = (int)(cf[s] >> 30); }
        else {
            if(++rehops > maxRehops) { linkStatus = HLALA_BAMSCAN_TOO_MANY_REHOPS; break; }
            how = bam_hop(data, N, cur, lim, nullptr, 0, &q, &c);
        }
        entry[s] = (uint32_t)cur;
        idx += c; cur = q;
        if(how == HOP_BAD) { linkStatus = HLALA_BAMSCAN_BAD_LENGTH; linkRecord = idx; ended = true; }
        else if(how == HOP_TAIL) ended = true;
    }
    stats->n_rehops = rehops;
    if(linkStatus == HLALA_BAMSCAN_TOO_MANY_REHOPS) {
        stats->status = linkStatus;
        stats->ms_wall = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        return HLALA_OK;
    }
    const size_t nRec = idx;
    stats->n_records = (int64_t)nRec; stats->consumed = (int64_t)cur;
    // ---- starts: every slice hops again from its true entry
    std::vector<uint32_t> recStart(nRec, 0);
    for(size_t s = 0; s < nSlices; s++) {
        if(entry[s] == BAM_NONE) continue;
        uint64_t q = 0; uint32_t c = 0;
        (void)bam_hop(data, N, entry[s], (s + 1) * S, recStart.data() + prefix[s], prefix[s] < nRec ? nRec - prefix[s] : 0, &q, &c);
    }
    // ---- parse: what every record yields
    std::vector<uint32_t> cnt(nRec, 0), csize(nRec, 0);
    uint64_t failKey = ~0ull, examined = 0, kept = 0;
    for(size_t ri = 0; ri < nRec; ri++) {
        uint32_t ex = 0;
        const int st = bam_parse_record(data, N, recStart[ri], *in, ri, 0, nullptr, 0, &cnt[ri], &csize[ri], &ex);
        if(st != HLALA_BAMSCAN_OK) { const uint64_t key = ((uint64_t)ri << 8) | (uint64_t)st; if(key < failKey) failKey = key; cnt[ri] = 0; csize[ri] = 0; continue; }
        examined += ex; kept += cnt[ri] ? 1 : 0;
    }
    // ---- the two exclusive scans
    std::vector<uint64_t> descOff(nRec + 1, 0), compOff(nRec + 1, 0);
    for(size_t ri = 0; ri < nRec; ri++) { descOff[ri + 1] = descOff[ri] + cnt[ri]; compOff[ri + 1] = compOff[ri] + csize[ri]; }
    stats->n_kept = (int64_t)kept; stats->n_recs = (int64_t)descOff[nRec]; stats->examined = (int64_t)examined; stats->compact_bytes = (int64_t)compOff[nRec];
    scan_verdict(linkStatus, linkRecord, failKey, last != 0, cur, N, nRec, &stats->status, &stats->status_record);
    int rc = HLALA_OK;
    if(stats->status == HLALA_BAMSCAN_OK) {
        if(stats->n_recs > cap_recs || (uint64_t)stats->compact_bytes > (uint64_t)cap_compact) rc = HLALA_E_CAPACITY;
        else {
            // ---- emit: descriptors in ascending order, the kept records' bytes up to their tags
            for(size_t ri = 0; ri < nRec; ri++) {
                if(!cnt[ri]) continue;
                uint32_t nd = 0, cs = 0, ex = 0;
                (void)bam_parse_record(data, N, recStart[ri], *in, ri, compOff[ri], recs + descOff[ri], cnt[ri], &nd, &cs, &ex);
                memcpy(compact + compOff[ri], data + recStart[ri] + 4, csize[ri]);
            }
        }
    }
    stats->ms_wall = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return rc;
}

}  // namespace hlala_bamscan
#endif

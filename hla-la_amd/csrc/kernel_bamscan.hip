// kernel_bamscan.hip -- the BAM record pass on inflated bytes resident in HBM: record boundaries, the decoder's parse (filters, CIGAR, AS tag, name hash) and
// compaction of the kept records.  The rules are bam_scan_core.h (shared with the host model, bam_scan_model.h); this file is how they are spread over lanes.
//
// Record boundaries are serial (a record's start is known from the length of the one before), so the buffer is cut into slices of S bytes, independent of BGZF
// blocks and of records, and the walk is speculated per slice:
//   k_bam_guess   one wavefront per slice: the lanes test 64 candidate offsets per step (bam_plausible: a chain of three plausible records), a ballot picks the
//                 lowest hit g(s); lane 0 hops from g(s) to the first start x(s) at or beyond the slice end and counts the starts c(s)
//   k_bam_link    ONE wavefront walks the slices in order from `first`: where the true entry of a slice equals g(s) it takes x(s) and c(s), otherwise lane 0 hops
//                 through the slice itself (a re-hop; at most max_rehops of them bound this wave's serial work).  Correctness never rests on a guess.  Per slice
//                 the true entry (none where a long record covers the slice) and the exclusive prefix of the counts
//   k_bam_starts  one lane per slice hops from the true entry and writes the record starts
//   k_bam_parse   one lane per record: what it yields (descriptors, compact bytes, examined) or its status; one atomic min per failing wave
//   k_bam_scan2   two exclusive scans (descriptor counts, compact sizes), one block each
//   k_bam_emit    descriptors in ascending order (lane per record), then the kept records' bytes up to their tags, all lanes of a wave on one record
// Every pass is a launch of its own on one stream: stream order is the only synchronisation, no workgroup waits for another.
//
// Bounds: every load of record bytes goes through the core, which checks against n; per-slice arrays are indexed below nSlices, per-record arrays below nRec;
// a start is stored only below the capacity left behind the slice's prefix; descriptors and compact bytes are written at the offsets of the scans, whose totals
// the host has checked against the buffers before k_bam_emit is launched.  Every hop advances by at least 36 bytes or ends.
#pragma once
#include "device_common.h"
#include "bam_scan_core.h"

namespace hlala {

struct BamScanTotals {
    u64 fail_key;                   // (record << 8) | status of the failing record with the lowest index; all ones: none
    u64 examined, kept;
    u64 n_desc, compact_bytes;
    u32 n_records, consumed, n_rehops, link_record;
    int link_status, pad;
};

__global__ __launch_bounds__(256) void k_bam_guess(const uint8_t* __restrict__ d, const u32 n, const u32 first, const u32 S, const u32 nSlices, const int n_ref,
                                                   u32* __restrict__ g, u32* __restrict__ x, u32* __restrict__ cf)
{
    using namespace hlala_bamscan;
    const u32 s = blockIdx.x * 4u + (threadIdx.x >> 6);
    if(s >= nSlices) return;                                // (wave-uniform)
    const int lane = lane_id();
    const u64 lo = (u64)s * S, lim = lo + S, a = lo > first ? lo : (u64)first, z = lim < n ? lim : (u64)n;
    u32 found = BAM_NONE;
    for(u64 base = a; base < z; base += 64) {               // (wave-uniform: base and the ballot are the same in all lanes)
        const u64 p = base + (u64)lane;
        const bool hit = p < z && bam_plausible(d, n, p, n_ref);
        const u64 m = __ballot(hit);
        if(m) { found = (u32)(base + (u64)__builtin_ctzll(m)); break; }
    }
    if(lane == 0) {
        u32 xs = BAM_NONE, cs = 0;
        if(found != BAM_NONE) {
            uint64_t q = 0; uint32_t c = 0;
            const int how = bam_hop(d, n, found, lim, nullptr, 0, &q, &c);          // a bad length on a speculative chain only ends the chain
            xs = (u32)q; cs = c | ((u32)how << 30);
        }
        g[s] = found; x[s] = xs; cf[s] = cs;
    }
}

__global__ __launch_bounds__(64) void k_bam_link(const uint8_t* __restrict__ d, const u32 n, const u32 first, const u32 S, const u32 nSlices, const u32 maxRehops,
                                                 const u32* __restrict__ g, const u32* __restrict__ x, const u32* __restrict__ cf, u32* __restrict__ entry, u32* __restrict__ prefix,
                                                 BamScanTotals* __restrict__ T)
{
    using namespace hlala_bamscan;
    const int lane = lane_id();
    // the state of the walk: the same value in every lane
    u32 cur = first, idx = 0, rehops = 0, linkRecord = 0; int ended = 0, status = HLALA_BAMSCAN_OK;
    for(u32 s0 = 0; s0 < nSlices && status != HLALA_BAMSCAN_TOO_MANY_REHOPS; s0 += 64) {
        const u32 s = s0 + (u32)lane;
        const u32 gv = s < nSlices ? g[s] : BAM_NONE, xv = s < nSlices ? x[s] : BAM_NONE, cv = s < nSlices ? cf[s] : 0u;      // a coalesced group of 64
        u32 myEntry = BAM_NONE, myPrefix = 0;
        const int cntJ = nSlices - s0 < 64u ? (int)(nSlices - s0) : 64;
        for(int j = 0; j < cntJ; j++) {
            const u64 lim = (u64)(s0 + (u32)j + 1u) * S;
            if(lane == j) myPrefix = idx;
            if(ended || (u64)cur >= lim) continue;
            const u32 gj = (u32)uni(__shfl((int)gv, j));
            u32 q, c; int how;
            if(gj != BAM_NONE && gj == cur) {
                q = (u32)uni(__shfl((int)xv, j)); c = (u32)uni(__shfl((int)cv, j));
                how = (int)(c >> 30); c &= 0x3FFFFFFFu;
            } else {
                if(++rehops > maxRehops) { status = HLALA_BAMSCAN_TOO_MANY_REHOPS; break; }
                uint64_t q64 = 0; uint32_t c0 = 0; int h = 0;
                if(lane == 0) h = bam_hop(d, n, cur, lim, nullptr, 0, &q64, &c0);
                q = (u32)uni((int)(u32)q64); c = (u32)uni((int)c0); how = uni(h);
            }
            if(lane == j) myEntry = cur;
            idx += c; cur = q;
            if(how == HOP_BAD) { status = HLALA_BAMSCAN_BAD_LENGTH; linkRecord = idx; ended = 1; }
            else if(how == HOP_TAIL) ended = 1;
        }
        if(s < nSlices) { entry[s] = myEntry; prefix[s] = myPrefix; }
    }
    if(lane == 0) { T->n_records = idx; T->consumed = cur; T->n_rehops = rehops; T->link_record = linkRecord; T->link_status = status; }
}

__global__ __launch_bounds__(256) void k_bam_starts(const uint8_t* __restrict__ d, const u32 n, const u32 S, const u32 nSlices, const u32 nRec, const u32* __restrict__ entry,
                                                    const u32* __restrict__ prefix, u32* __restrict__ recStart)
{
    using namespace hlala_bamscan;
    const u32 s = blockIdx.x * 256u + threadIdx.x;
    if(s >= nSlices) return;
    const u32 e = entry[s], p = prefix[s];
    if(e == BAM_NONE) return;
    uint64_t q = 0; uint32_t c = 0;
    (void)bam_hop(d, n, e, (u64)(s + 1u) * S, recStart + p, p < nRec ? (u64)(nRec - p) : 0ull, &q, &c);
}

__global__ __launch_bounds__(256) void k_bam_parse(const uint8_t* __restrict__ d, const u32 n, const u32 nRec, const hlala_bam_scan_in in, const u32* __restrict__ recStart,
                                                   u32* __restrict__ cnt, u32* __restrict__ csize, BamScanTotals* __restrict__ T)
{
    using namespace hlala_bamscan;
    const u32 ri = blockIdx.x * 256u + threadIdx.x;
    u64 key = ~0ull, ex64 = 0, kept = 0;
    if(ri < nRec) {
        uint32_t nd = 0, cs = 0, ex = 0;
        const int st = bam_parse_record(d, n, recStart[ri], in, ri, 0, nullptr, 0, &nd, &cs, &ex);
        if(st != HLALA_BAMSCAN_OK) { key = ((u64)ri << 8) | (u64)st; nd = 0; cs = 0; }
        else { ex64 = ex; kept = nd ? 1 : 0; }
        cnt[ri] = nd; csize[ri] = cs;
    }
    const u64 wkey = wave_min_u64(key), wex = wave_sum_u64(ex64), wkept = wave_sum_u64(kept);
    if(lane_id() == 0) {
        if(wkey != ~0ull) atomicMin(&T->fail_key, wkey);
        if(wex) atomicAdd(&T->examined, wex);
        if(wkept) atomicAdd(&T->kept, wkept);
    }
}

constexpr int BAM_SCAN_THREADS = 1024;
// block 0: descOff[0 .. nRec] = exclusive scan of cnt; block 1: compOff of csize.  Every thread sums a stretch, the block scans the sums.
__global__ __launch_bounds__(BAM_SCAN_THREADS) void k_bam_scan2(const u32 nRec, const u32* __restrict__ cnt, const u32* __restrict__ csize, u64* __restrict__ descOff, u64* __restrict__ compOff,
                                                                BamScanTotals* __restrict__ T)
{
    __shared__ u64 part[BAM_SCAN_THREADS];
    const u32* in = blockIdx.x == 0 ? cnt : csize; u64* out = blockIdx.x == 0 ? descOff : compOff;
    const u32 t = threadIdx.x;
    const u32 per = (nRec + BAM_SCAN_THREADS - 1) / BAM_SCAN_THREADS;
    const u64 a = (u64)t * per, z = a + per < nRec ? a + per : (u64)nRec;
    u64 s = 0;
    for(u64 i = a; i < z; i++) s += in[i];
    part[t] = s;
    __syncthreads();
    for(u32 o = 1; o < BAM_SCAN_THREADS; o <<= 1) {
        const u64 v = t >= o ? part[t - o] : 0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    u64 run = part[t] - s;
    for(u64 i = a; i < z; i++) { out[i] = run; run += in[i]; }
    if(t == BAM_SCAN_THREADS - 1) { out[nRec] = part[t]; if(blockIdx.x == 0) T->n_desc = part[t]; else T->compact_bytes = part[t]; }
}

// len bytes by the 64 lanes of a wave; dwords where source and destination share their alignment
__device__ __forceinline__ void bam_wave_copy(uint8_t* __restrict__ dst, const uint8_t* __restrict__ src, const u32 len, const int lane)
{
    u32 head = (u32)(0u - (u32)(uintptr_t)dst) & 3u; if(head > len) head = len;
    if((((uintptr_t)src + head) & 3u) == 0) {
        if((u32)lane < head) dst[lane] = src[lane];
        const u32 words = (len - head) >> 2;
        const u32* sw = (const u32*)(src + head); u32* dw = (u32*)(dst + head);
        for(u32 k = (u32)lane; k < words; k += 64) dw[k] = sw[k];
        const u32 done = head + 4u * words;
        if((u32)lane < len - done) dst[done + (u32)lane] = src[done + (u32)lane];
    } else
        for(u32 k = (u32)lane; k < len; k += 64) dst[k] = src[k];
}

__global__ __launch_bounds__(256) void k_bam_emit(const uint8_t* __restrict__ d, const u32 n, const u32 nRec, const hlala_bam_scan_in in, const u32* __restrict__ recStart,
                                                  const u32* __restrict__ cnt, const u32* __restrict__ csize, const u64* __restrict__ descOff, const u64* __restrict__ compOff,
                                                  hlala_bam_rec* __restrict__ recs, uint8_t* __restrict__ compact)
{
    using namespace hlala_bamscan;
    const u32 ri = blockIdx.x * 256u + threadIdx.x;
    const int lane = lane_id();
    u32 start = 0, cs = 0; u64 co = 0;
    if(ri < nRec && cnt[ri]) {
        start = recStart[ri]; cs = csize[ri]; co = compOff[ri];
        uint32_t nd = 0, c2 = 0, ex = 0;
        (void)bam_parse_record(d, n, start, in, ri, co, recs + descOff[ri], cnt[ri], &nd, &c2, &ex);
    }
    u64 m = __ballot(cs != 0);
    while(m) {                                               // (wave-uniform)
        const int i = __builtin_ctzll(m); m &= m - 1;
        const u32 st = (u32)uni(__shfl((int)start, i)), len = (u32)uni(__shfl((int)cs, i));
        const u64 to = ((u64)(u32)uni(__shfl((int)(u32)(co >> 32), i)) << 32) | (u32)uni(__shfl((int)(u32)co, i));
        bam_wave_copy(compact + to, d + st + 4, len, lane);              // (start + 4 + csize <= n: bam_parse_record checked oTags against the record's length)
    }
}

}  // namespace hlala

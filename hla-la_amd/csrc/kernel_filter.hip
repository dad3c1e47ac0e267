// kernel_filter.hip -- the read / allele filters between the exon positions and the likelihoods on the device (hlala_filter_positions_gpu; the rule and why it can
// be met off the host: filter_gpu_core.h; the specification: host_filters.cpp; the same launches run serially: filter_gpu_model.h).
//   k_flt_mapq      per read: pos_off ascends, no NaN weight; per position: the mapq test against the uploaded PhredToPCorrect table, its read, the checks of the
//                   host's loop (table value in [0, 1], pos_exon >= 0), geno_off ascends; the number of exon positions                   -> the host reads the flags
//   k_flt_keys      sort key of a position (its exon position; one past the last for a position that failed the mapq test) and the histogram of the buckets
//   (hipcub::DeviceRadixSort::SortPairs on the key: stable, so a bucket keeps ascending position index; hipcub::DeviceScan::ExclusiveSum: the buckets' starts)
//   k_flt_largest   the largest bucket and the number of non-empty ones                                                                -> the host refuses beyond 4096
//   k_flt_first20   one wavefront per exon position: representatives of the alleles; where filterFirst20 runs the wave stages the weights and scores them in LDS,
//                   lane 0 runs fil_sort_wide there, the wave counts the first 20 and kicks
//   k_flt_reads     per read: kicked / kickedRobust against the limit -> ignoreRead                 (needs every bucket of the first phase)
//   k_flt_coverage  one wavefront per exon position: the counts over what is not ignored, the high-coverage and the strand filter
//   k_flt_use       per position: the use test and bases_used                                       (needs every ignored allele)
// Every counter is an integer and every flag is only ever set: no result depends on the order of the atomics.  Every index taken from LDS or from an input array is
// checked against its range before it addresses anything; a check that fires sets a flag the host turns into HLALA_E_ARG (none does once k_flt_mapq has passed).
#include "device_common.h"
#include "filter_gpu_core.h"

namespace hlala {

struct FltIn {
    u32 nReads, nPos, nChars;
    const int32_t *posOff, *posExon, *genoOff; const uint8_t *posMapq, *posMate, *genoChars, *readReverse; const double *wok, *pc;
    hlala_filter_params P;
};
// misc words
enum { FM_BAD = 0, FM_NB, FM_LARGEST, FM_BUCKETS, FM_SORTED, FM_HEAPS, FM_N = 8 };
struct FltWork {
    uint8_t* ok; u32* posRead; u32 *key, *val;      // per position
    u32* hist; u32* bOff;                           // [nb + 1]
    u32* sorted;                                    // [nPos] position indices by (exon position, index); the first bOff[nb] passed the mapq test
    u32* entRep; uint8_t* entIgnore; u32* posFlag;  // entRep[b0 + i]: bucket-local representative; entIgnore[b0 + rep]: the allele is ignored; posFlag[j]: that slot for position j
    int32_t *kicked, *kickedRobust; uint8_t* ignoreRead; uint8_t* posUse;
    unsigned long long* stats; u32* misc;
};

__global__ __launch_bounds__(256) void k_flt_mapq(FltIn I, FltWork W)
{
    using namespace hlala_filter;
    const u64 t = (u64)blockIdx.x * 256u + threadIdx.x;
    u32 bad = 0;
    if(t < I.nReads) bad |= flt_check_read(I.posOff, I.wok, (u32)t);
    if(t < I.nPos) {
        const u32 j = (u32)t; bool ok = false;
        bad |= flt_check_pos(I.pc, I.posMapq, I.posExon, I.genoOff, I.P.min_per_position_mapq, j, &ok);
        W.ok[j] = ok ? 1 : 0; W.posRead[j] = flt_read_of(I.posOff, I.nReads, j);
        const int32_t e = I.posExon[j];
        if(ok && e >= 0) atomicMax(&W.misc[FM_NB], (u32)e + 1u);
    }
    if(bad) atomicOr(&W.misc[FM_BAD], bad);
}

__global__ __launch_bounds__(256) void k_flt_keys(FltIn I, FltWork W, u32 nb)
{
    const u64 t = (u64)blockIdx.x * 256u + threadIdx.x;
    if(t >= I.nPos) return;
    const u32 j = (u32)t; const int32_t e = I.posExon[j];
    const bool in = W.ok[j] && e >= 0 && (u32)e < nb;
    W.key[j] = in ? (u32)e : nb; W.val[j] = j;
    if(in) atomicAdd(&W.hist[e], 1u);
}

__global__ __launch_bounds__(256) void k_flt_largest(FltWork W, u32 nb)
{
    const u64 t = (u64)blockIdx.x * 256u + threadIdx.x;
    const u32 n = t < nb ? W.hist[t] : 0u;
    const int most = wave_max_i32((int)n);
    const int some = __popcll(__ballot(n != 0u));
    if(lane_id() == 0 && some) { atomicMax(&W.misc[FM_LARGEST], (u32)most); atomicAdd(&W.misc[FM_BUCKETS], (u32)some); }
}

// entry i of the bucket at b0: its position and read, held inside their ranges (a stray index: flagged, and entry 0's in its place)
struct FltEnt { u32 j, r; };
__device__ __forceinline__ FltEnt flt_ent(const FltIn& I, const FltWork& W, u32 slot, u32& bad)
{
    using namespace hlala_filter;
    FltEnt E; E.j = slot < I.nPos ? W.sorted[slot] : I.nPos;
    if(E.j >= I.nPos) { bad |= FLT_BAD_INDEX; E.j = 0; }
    E.r = W.posRead[E.j];
    if(E.r >= I.nReads) { bad |= FLT_BAD_INDEX; E.r = 0; }
    return E;
}

// dynamic LDS of the two bucket kernels for buckets of at most cap entries (cap: a multiple of 64): k_flt_first20 lays out [w: 8 cap | score: 4 cap | place: 2 cap]
// and reuses w for [rep: 2 cap | cnt: 4 cap] once the scores are made, place for the list of long alleles before the sort; k_flt_coverage [cnt | rev | list | rep]
HLALA_HD size_t flt_lds_bytes(uint32_t cap) { return (size_t)14 * cap; }

__global__ __launch_bounds__(64) void k_flt_first20(FltIn I, FltWork W, u32 nb, u32 cap)
{
    using namespace hlala_filter;
    using namespace hlala_bamfill;
    extern __shared__ __attribute__((aligned(16))) unsigned char sFlt[];
    __shared__ u32 sFirst[256];
    __shared__ u32 sStack[FIL_WIDE_STACK_WORDS];
    __shared__ u32 sHeaps;
    double* sW = (double*)sFlt;
    uint16_t* sRep = (uint16_t*)sFlt;                                 // behind the scores: the weights are dead
    u32* sCnt = (u32*)(sFlt + (size_t)2 * cap);                       // low half: among the first 20; high half: kicked entries
    int32_t* sScore = (int32_t*)(sFlt + (size_t)8 * cap);
    uint16_t* sPlace = (uint16_t*)(sFlt + (size_t)12 * cap);
    uint16_t* sLong = sPlace;                                         // before the sort
    const u32 e = blockIdx.x, lane = (u32)lane_id();
    if(e >= nb) return;
    // (every condition that ends the wavefront early is wave-uniform)
    const u32 b0 = W.bOff[e], b1 = W.bOff[e + 1];
    if(b1 <= b0) return;
    const u32 n = b1 - b0;
    if(b1 > I.nPos || n > cap || n > FLT_MAX_BUCKET) { if(lane == 0) atomicOr(&W.misc[FM_BAD], (u32)FLT_BAD_INDEX); return; }
    const bool runs = flt_first20_runs(I.P, n);
    u32 bad = 0;
    if(runs) {
        for(u32 base = 0; base < n; base += 64u) { const u32 i = base + lane; if(i < n) sW[i] = flt_weight(I.wok, flt_ent(I, W, b0 + i, bad).r); }
        WSYNC();
        for(u32 base = 0; base < n; base += 64u) { const u32 i = base + lane; if(i < n) sScore[i] = flt_score(sW, n, i); }
        WSYNC();
    }
    // representatives: genotypes of one byte through a first-occurrence table, the others against the earlier ones of their kind
    for(u32 t = lane; t < 256u; t += 64u) sFirst[t] = FLT_NO_REP;
    WSYNC();
    u32 nLong = 0;
    for(u32 base = 0; base < n; base += 64u) {
        const u32 i = base + lane; bool isLong = false;
        if(i < n) {
            const FltGeno g = flt_geno(I.genoOff, I.nChars, flt_ent(I, W, b0 + i, bad).j, &bad);
            if(g.len == 1u) atomicMin(&sFirst[I.genoChars[g.at]], i); else isLong = true;
        }
        const u64 b = __ballot(isLong);
        if(isLong) sLong[nLong + (u32)__popcll(b & ((1ull << lane) - 1ull))] = (uint16_t)i;
        nLong += (u32)__popcll(b);
    }
    WSYNC();
    for(u32 base = 0; base < n; base += 64u) {
        const u32 i = base + lane;
        if(i < n) {
            const FltGeno g = flt_geno(I.genoOff, I.nChars, flt_ent(I, W, b0 + i, bad).j, &bad);
            if(g.len == 1u) { u32 r = sFirst[I.genoChars[g.at]]; if(r >= n) { bad |= FLT_BAD_INDEX; r = i; } sRep[i] = (uint16_t)r; }
        }
    }
    for(u32 base = 0; base < nLong; base += 64u) {
        const u32 q = base + lane;
        if(q < nLong) {
            u32 i = sLong[q]; if(i >= n) { bad |= FLT_BAD_INDEX; i = 0; }
            const FltGeno g = flt_geno(I.genoOff, I.nChars, flt_ent(I, W, b0 + i, bad).j, &bad);
            u32 r = i;
            for(u32 q2 = 0; q2 < q; q2++) {
                u32 i2 = sLong[q2]; if(i2 >= n) { bad |= FLT_BAD_INDEX; i2 = 0; }
                if(flt_same_bytes(I.genoChars, flt_geno(I.genoOff, I.nChars, flt_ent(I, W, b0 + i2, bad).j, &bad), g)) { r = i2; break; }
            }
            sRep[i] = (uint16_t)r;
        }
    }
    WSYNC();
    for(u32 base = 0; base < n; base += 64u) {
        const u32 i = base + lane;
        if(i < n) { const u32 r = sRep[i]; W.entRep[b0 + i] = r; W.posFlag[flt_ent(I, W, b0 + i, bad).j] = b0 + r; }
    }
    if(!runs) { if(bad) atomicOr(&W.misc[FM_BAD], bad); return; }
    // the order std::sort + std::reverse leave, and its first first20_n
    for(u32 base = 0; base < n; base += 64u) { const u32 i = base + lane; if(i < n) { sPlace[i] = (uint16_t)i; sCnt[i] = 0u; } }
    WSYNC();
    if(lane == 0) sHeaps = fil_sort_wide(sScore, sPlace, n, sStack);
    WSYNC();
    if(sHeaps == FIL_WIDE_OVERFLOW) { if(lane == 0) atomicOr(&W.misc[FM_BAD], (u32)FLT_BAD_SORT); return; }
    const u32 first20 = I.P.first20_n > 0 ? (u32)I.P.first20_n : 0u;                  // (<= n: the filter runs)
    for(u32 base = 0; base < first20; base += 64u) {
        const u32 i = base + lane;
        if(i < first20 && i < n) { const u32 pl = sPlace[i]; if(pl < n) atomicAdd(&sCnt[sRep[pl]], 1u); else bad |= FLT_BAD_INDEX; }
    }
    WSYNC();
    int kicks = 0;
    for(u32 base = 0; base < n; base += 64u) {
        const u32 i = base + lane;
        if(i < n) {
            const u32 a = sRep[i];
            if(flt_first20_kicks(I.P, sCnt[a] & 0xFFFFu)) { W.entIgnore[b0 + a] = 1; atomicAdd(&W.kicked[flt_ent(I, W, b0 + i, bad).r], 1); atomicAdd(&sCnt[a], 1u << 16); kicks++; }
        }
    }
    WSYNC();
    for(u32 base = 0; base < n; base += 64u) {
        const u32 i = base + lane;
        if(i < n && (sCnt[sRep[i]] >> 16) >= 2u) atomicAdd(&W.kickedRobust[flt_ent(I, W, b0 + i, bad).r], 1);                 // :1628-1641
    }
    const int removed = wave_sum_i32(kicks);
    if(bad) atomicOr(&W.misc[FM_BAD], bad);
    if(lane != 0) return;
    atomicAdd(&W.stats[FS_CONSIDERED_ALLELES], (unsigned long long)n); atomicAdd(&W.stats[FS_CONSIDERED_POS], 1ull);
    if(removed) { atomicAdd(&W.stats[FS_REMOVED_ALLELES], (unsigned long long)removed); atomicAdd(&W.stats[FS_POS_WITH_REMOVED], 1ull); }
    atomicAdd(&W.misc[FM_SORTED], 1u);
    if(sHeaps) atomicAdd(&W.misc[FM_HEAPS], sHeaps);
}

__global__ __launch_bounds__(256) void k_flt_reads(FltIn I, FltWork W)
{
    const u64 t = (u64)blockIdx.x * 256u + threadIdx.x;
    bool k = false, kr = false;
    if(t < I.nReads) {
        k = W.kicked[t] > I.P.first20_limit_per_read; kr = W.kickedRobust[t] > I.P.first20_limit_per_read;
        W.ignoreRead[t] = kr ? 1 : 0;                                                   // ignore_readIDs, :1686-1690
    }
    const int nk = __popcll(__ballot(k)), nkr = __popcll(__ballot(kr));
    if(lane_id() != 0) return;
    if(nk) atomicAdd(&W.stats[hlala_filter::FS_READS_KICKED], (unsigned long long)nk);
    if(nkr) atomicAdd(&W.stats[hlala_filter::FS_READS_KICKED_ROBUST], (unsigned long long)nkr);
}

__global__ __launch_bounds__(64) void k_flt_coverage(FltIn I, FltWork W, u32 nb, u32 cap)
{
    using namespace hlala_filter;
    extern __shared__ __attribute__((aligned(16))) unsigned char sFlt[];
    u32* sCnt = (u32*)sFlt;
    u32* sRev = (u32*)(sFlt + (size_t)4 * cap);
    uint16_t* sRemoved = (uint16_t*)(sFlt + (size_t)8 * cap);
    const u32 e = blockIdx.x, lane = (u32)lane_id();
    if(e >= nb) return;
    const u32 b0 = W.bOff[e], b1 = W.bOff[e + 1];
    if(b1 <= b0) return;
    const u32 n = b1 - b0;
    if(b1 > I.nPos || n > cap) { if(lane == 0) atomicOr(&W.misc[FM_BAD], (u32)FLT_BAD_INDEX); return; }
    const bool strand = I.P.long_read_strand_filter != 0 && I.readReverse && I.posMate;
    u32 bad = 0;
    for(u32 base = 0; base < n; base += 64u) { const u32 i = base + lane; if(i < n) { sCnt[i] = 0u; sRev[i] = 0u; } }
    WSYNC();
    u32 countPosition = 0;
    for(u32 base = 0; base < n; base += 64u) {
        const u32 i = base + lane; bool live = false;
        if(i < n) {
            const FltEnt E = flt_ent(I, W, b0 + i, bad);
            u32 a = W.entRep[b0 + i]; if(a >= n) { bad |= FLT_BAD_INDEX; a = 0; }
            live = !W.ignoreRead[E.r] && !W.entIgnore[b0 + a];
            if(live) {
                atomicAdd(&sCnt[a], 1u);
                if(strand && I.readReverse[2 * (size_t)E.r + (I.posMate[E.j] == 2 ? 1 : 0)]) atomicAdd(&sRev[a], 1u);
            }
        }
        countPosition += (u32)__popcll(__ballot(live));
    }
    WSYNC();
    if(bad) atomicOr(&W.misc[FM_BAD], bad);
    if(countPosition == 0) return;
    const bool high = (int64_t)countPosition >= (int64_t)I.P.high_coverage_min_coverage;
    int hcRemoved = 0, enough = 0; u32 nRemoved = 0;
    for(u32 base = 0; base < n; base += 64u) {
        const u32 a = base + lane; const u32 c = a < n ? sCnt[a] : 0u;
        if(c && high && flt_high_coverage_removes(I.P, c, countPosition)) { W.entIgnore[b0 + a] = 1; hcRemoved += (int)c; }
        bool rem = false;
        if(c && strand) {
            if(flt_strand_enough(I.P, c)) enough++;
            rem = flt_strand_removes(I.P, c, sRev[a]);
            if(rem) W.entIgnore[b0 + a] = 1;
        }
        const u64 b = __ballot(rem);
        if(rem) sRemoved[nRemoved + (u32)__popcll(b & ((1ull << lane) - 1ull))] = (uint16_t)a;
        nRemoved += (u32)__popcll(b);
    }
    WSYNC();
    // the reference's position counter: once per allele visited, in std::string order, at or after the first removal -- some removed allele is not greater
    int after = 0; u32 bad2 = 0;
    if(nRemoved) for(u32 base = 0; base < n; base += 64u) {
        const u32 a = base + lane;
        if(a < n && sCnt[a]) {
            const FltGeno ga = flt_geno(I.genoOff, I.nChars, flt_ent(I, W, b0 + a, bad2).j, &bad2);
            for(u32 k = 0; k < nRemoved; k++) {
                u32 m = sRemoved[k]; if(m >= n) { bad2 |= FLT_BAD_INDEX; m = 0; }
                if(!flt_less_bytes(I.genoChars, ga, flt_geno(I.genoOff, I.nChars, flt_ent(I, W, b0 + m, bad2).j, &bad2))) { after++; break; }
            }
        }
    }
    const int sHc = wave_sum_i32(hcRemoved), sEnough = wave_sum_i32(enough), sAfter = wave_sum_i32(after);
    if(bad2) atomicOr(&W.misc[FM_BAD], bad2);
    if(lane != 0) return;
    if(high) atomicAdd(&W.stats[FS_HC_POSITIONS], 1ull);
    if(sHc) atomicAdd(&W.stats[FS_HC_REMOVED], (unsigned long long)sHc);
    if(sEnough) atomicAdd(&W.stats[FS_STRAND_ENOUGH], (unsigned long long)sEnough);
    if(nRemoved) atomicAdd(&W.stats[FS_STRAND_REMOVED], (unsigned long long)nRemoved);
    if(sAfter) atomicAdd(&W.stats[FS_STRAND_POS_REMOVED], (unsigned long long)sAfter);
}

__global__ __launch_bounds__(256) void k_flt_use(FltIn I, FltWork W, u32 nOK)
{
    const u64 t = (u64)blockIdx.x * 256u + threadIdx.x;
    bool use = false;
    if(t < I.nPos) {
        const u32 j = (u32)t, r = W.posRead[j], f = W.posFlag[j];
        use = W.ok[j] && f < nOK && r < I.nReads && !W.entIgnore[f] && !W.ignoreRead[r];                       // :2102-2120
        W.posUse[j] = use ? 1 : 0;
    }
    const int nu = __popcll(__ballot(use));
    if(lane_id() == 0 && nu) atomicAdd(&W.stats[hlala_filter::FS_BASES_USED], (unsigned long long)nu);
}

}  // namespace hlala

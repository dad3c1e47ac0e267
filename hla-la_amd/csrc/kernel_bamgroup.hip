// kernel_bamgroup.hip -- grouping the record descriptors of a sample by read name (include/hlala_gpu.h: hlala_bam_group; the rules are bam_group_core.h, which the host
// runs as a model).  One 64-lane wavefront per block, a lane per record in every kernel:
//   k_grp_len      the nameLen of a round's descriptors as 64-bit addends: their exclusive sum (hipcub) is where each name goes in the sample's name arena
//   k_grp_append   behind k_bam_emit on the same stream: (hash, nameLen | which | flags, name offset) of the round appended to the sample-long arrays, the name
//                  copied out of the round's compact buffer.  The one loop of a lane runs over the bytes of ONE name (<= 65535, in practice a few dozen)
//   k_grp_iota     the values of the sort: global descriptor indices
//   (hipcub::DeviceRadixSort::SortPairs on the 64-bit hash: stable, so equal hashes stay in ascending order)
//   k_grp_mark     sorted record i against i - 1: run start (another hash), or neq (the same hash, another name: grp_same_name streams both names from the arena)
//   (hipcub::DeviceScan::ExclusiveSum of the start flags: run ids)
//   k_grp_fold     every record ORs (neq, primary of mate 0, primary of mate 1) into its run's word: a segmented OR over the wave in six shuffle steps, then one
//                  atomicOr per run and wave -- a run of thousands of records is thousands of lanes, no lane walks it
//   k_grp_emit     flag[] from the words, and the three counts
// No kernel's serial depth depends on the length of a run.
//
// Bounds: every kernel guards i < n; k_grp_append reads bytes[rec_off + 32 .. + nameLen) only after checking it against nBytes (the host has checked the descriptors
// of hlala_bam_group; the decoder's come from k_bam_emit) and writes names[off .. off + nameLen) only when that lies inside namesCap; grp_same_name checks both names
// against the arena's end.  perm values are < n by construction (k_grp_iota, permuted by the sort).
#pragma once
#include "device_common.h"
#include "bam_group_core.h"

namespace hlala {

__global__ __launch_bounds__(64) void k_grp_len(const hlala_bam_rec* recs, u32 n, u64* len /* [n + 1] */)
{
    const u32 i = blockIdx.x * 64u + threadIdx.x;
    if(i < n) len[i] = recs[i].nameLen;
    else if(i == n) len[i] = 0;
}

__global__ __launch_bounds__(64) void k_grp_append(const hlala_bam_rec* recs, u32 n, const uint8_t* bytes, u64 nBytes, const u64* off /* [n]: within the round */, u64 nameBase,
                                                   u64* hash, u32* meta, u64* nameOff, uint8_t* names, u64 namesCap)
{
    using namespace hlala_bamgroup;
    const u32 i = blockIdx.x * 64u + threadIdx.x;
    if(i >= n) return;
    const hlala_bam_rec r = recs[i];
    const u64 to = nameBase + off[i];
    hash[i] = r.hash; meta[i] = grp_meta(r.nameLen, r.which, r.flags); nameOff[i] = to;
    const u32 L = r.nameLen;
    if(r.rec_off > nBytes || nBytes - r.rec_off < (u64)GRP_NAME_AT + L || to > namesCap || namesCap - to < L) return;
    const uint8_t* src = bytes + r.rec_off + GRP_NAME_AT;
    uint8_t* dst = names + to;
    for(u32 k = 0; k < L; k++) dst[k] = src[k];
}

__global__ __launch_bounds__(64) void k_grp_iota(u32 n, u32* v)
{
    const u32 i = blockIdx.x * 64u + threadIdx.x;
    if(i < n) v[i] = i;
}

__global__ __launch_bounds__(64) void k_grp_mark(u32 n, const u64* sortedHash, const u32* perm, const u32* meta, const u64* nameOff, const uint8_t* names, u64 nameBytes,
                                                 u32* start /* [n + 1] */, uint8_t* neq)
{
    using namespace hlala_bamgroup;
    const u32 i = blockIdx.x * 64u + threadIdx.x;
    if(i > n) return;
    if(i == n) { start[i] = 0; return; }
    const bool s = grp_run_start(i, i ? sortedHash[i - 1] : 0, sortedHash[i]);
    bool q = false;
    if(!s) {
        const u32 g = perm[i], gp = perm[i - 1];
        if(g < n && gp < n) q = !grp_same_name(names, nameBytes, nameOff[g], meta_name_len(meta[g]), nameOff[gp], meta_name_len(meta[gp]));
    }
    start[i] = s ? 1u : 0u; neq[i] = q ? 1 : 0;
}

__global__ __launch_bounds__(64) void k_grp_fold(u32 n, const u32* perm, const u32* meta, const u32* start, const u32* runOff, const uint8_t* neq, u32* word)
{
    using namespace hlala_bamgroup;
    const u32 i = blockIdx.x * 64u + threadIdx.x;
    const int lane = lane_id();
    u32 run = 0xFFFFFFFFu, w = 0;
    if(i < n) {
        const u32 g = perm[i];
        run = runOff[i] + start[i] - 1u;
        if(g < n) w = grp_fold_bits(neq[i] != 0, meta[g]);
    }
    // run ids ascend with the lane: after step d a lane holds the OR of the lanes [lane, lane + 2 d) that share its run
    for(int d = 1; d < 64; d <<= 1) {
        const u32 ow = (u32)__shfl_down((int)w, d), orun = (u32)__shfl_down((int)run, d);
        if(lane + d < 64 && orun == run) w |= ow;
    }
    const u32 before = (u32)__shfl_up((int)run, 1);
    const bool head = lane == 0 || before != run;
    if(i < n && head && w && run < n) atomicOr(word + run, w);
}

__global__ __launch_bounds__(64) void k_grp_emit(u32 n, const u32* start, const u32* runOff, const u32* word, int long_read_mode, uint8_t* flag, unsigned long long* counts /* [3] */)
{
    using namespace hlala_bamgroup;
    const u32 i = blockIdx.x * 64u + threadIdx.x;
    uint8_t f = 0;
    if(i < n) { if(start[i]) f = grp_run_flag(word[runOff[i]], long_read_mode); flag[i] = f; }
    const unsigned long long col = __ballot((f & GRP_COLLIDED) != 0), com = __ballot((f & GRP_COMPLETE) != 0), any = __ballot((f & GRP_START) != 0);
    if(lane_id() == 0) {
        const int a = __popcll(col), b = __popcll(com), c = __popcll(any) - a - b;
        if(a) atomicAdd(counts + 0, (unsigned long long)a);
        if(b) atomicAdd(counts + 1, (unsigned long long)b);
        if(c) atomicAdd(counts + 2, (unsigned long long)c);
    }
}

}  // namespace hlala

// kernel_bamnameorder.hip -- the read-name order of names in a byte arena (include/hlala_gpu.h: hlala_bam_name_order; the rules are bam_nameorder_core.h, which the host
// runs as a model).  MSD refinement in rounds of NAM_W bytes over a working set of SLOTS: slot j holds a name idx[j], its segment seg[j] (names equal on all bytes seen
// so far; ascending with j) and the place gp[j] of the final order it stands for -- a sort moves names between the slots of one segment only, so gp stays with the slot.
// One 64-lane wavefront per block, a lane per slot in every kernel:
//   k_nam_select   (decoder) sorted record i of the grouping stage is the first of a clean, complete run -- a unit: 1, else 0; their exclusive sum (hipcub) is the unit's
//   k_nam_units    place in run order, where its name's offset and length go
//   k_nam_init     slot j holds name j, segment 0, place j
//   k_nam_key      the round's 64-bit key of every slot's name (nam_key: at most NAM_W byte loads at any alignment, none at or beyond nBytes), and j as the sort's value
//   (hipcub::DeviceRadixSort::SortPairs on the key, then -- beyond the first round -- k_nam_seg and a second, stable sort on as many bits of the segment as the count
//    of unresolved names needs: together (segment, key, valid bytes), equal names in ascending index)
//   k_nam_mark     sorted slot j against j - 1 and j + 1: a new segment starts where segment or key differs; a name alone in its segment or ended in this round is
//                  final; packs (kept, kept and first of its segment) into one 64-bit addend for ONE exclusive sum (hipcub): new slot and new segment id
//   k_nam_scatter  final names to order[gp[j]], the others to the front of the next round's working set
// No kernel's serial depth depends on n or on the size of a segment; the one loop of a lane runs over at most NAM_W bytes.
//
// Bounds: every kernel guards j < a (the scan's extra element: j == a); permutation values come from the sort of k_nam_key's 0..a-1 and are still checked against a
// before they index; idx values are checked against n before they index the names' offsets, gp values before they index order; k_nam_units writes unit t only
// where t < cap.
#pragma once
#include "device_common.h"
#include "bam_group_core.h"
#include "bam_nameorder_core.h"

namespace hlala {

__global__ __launch_bounds__(64) void k_nam_select(u32 n, const uint8_t* flag, u32* sel /* [n + 1] */)
{
    using namespace hlala_bamgroup;
    const u32 i = blockIdx.x * 64u + threadIdx.x;
    if(i > n) return;
    const uint8_t want = GRP_START | GRP_COMPLETE;
    sel[i] = (i < n && (flag[i] & (want | GRP_COLLIDED)) == want) ? 1u : 0u;
}

__global__ __launch_bounds__(64) void k_nam_units(u32 n, const u32* sel, const u32* selOff, const u32* perm, const u32* meta, const u64* nameOff, u32 cap, u64* uOff, u32* uLen)
{
    const u32 i = blockIdx.x * 64u + threadIdx.x;
    if(i >= n || !sel[i]) return;
    const u32 t = selOff[i], g = perm[i];
    if(t >= cap || g >= n) return;
    uOff[t] = nameOff[g]; uLen[t] = hlala_bamgroup::meta_name_len(meta[g]);
}

__global__ __launch_bounds__(64) void k_nam_init(u32 n, u32* idx, u32* seg, u32* gp)
{
    const u32 j = blockIdx.x * 64u + threadIdx.x;
    if(j < n) { idx[j] = j; seg[j] = 0; gp[j] = j; }
}

__global__ __launch_bounds__(64) void k_nam_key(u32 a, u32 n, const u32* idx, const u64* off, const u32* len, const uint8_t* names, u64 nBytes, u32 r, u64* key, u32* val)
{
    const u32 j = blockIdx.x * 64u + threadIdx.x;
    if(j >= a) return;
    const u32 i = idx[j];
    key[j] = i < n ? hlala_nameorder::nam_key(names, nBytes, off[i], len[i], r) : 0;
    val[j] = j;
}

// the second sort's key: the segment of the slot a name came from
__global__ __launch_bounds__(64) void k_nam_seg(u32 a, const u32* p, const u32* seg, u32* out)
{
    const u32 j = blockIdx.x * 64u + threadIdx.x;
    if(j >= a) return;
    const u32 e = p[j];
    out[j] = e < a ? seg[e] : 0xFFFFFFFFu;
}

__global__ __launch_bounds__(64) void k_nam_mark(u32 a, const u32* p, const u64* key, const u32* seg, const u32* idx, u32* newIdx, u64* fl /* [a + 1] */, unsigned long long* nEqual)
{
    using namespace hlala_nameorder;
    const u32 j = blockIdx.x * 64u + threadIdx.x;
    bool equal = false;
    if(j == a) fl[j] = 0;
    else if(j < a) {
        const u32 e = p[j];
        const u64 k = e < a ? key[e] : 0;
        const u32 s = seg[j];
        bool start = true, next = true;
        if(j > 0) { const u32 ep = p[j - 1]; start = nam_split(j, seg[j - 1], s, ep < a ? key[ep] : 0, k); }
        if(j + 1 < a) { const u32 en = p[j + 1]; next = nam_split(j + 1, s, seg[j + 1], k, en < a ? key[en] : 0); }
        const bool ended = nam_ended(k), keep = !((start && next) || ended);
        equal = !start && ended;
        newIdx[j] = e < a ? idx[e] : 0xFFFFFFFFu;
        fl[j] = (keep ? 1ull : 0ull) | (keep && start ? 1ull << 32 : 0ull);
    }
    const unsigned long long eq = __ballot(equal);
    if(lane_id() == 0 && eq) atomicAdd(nEqual, (unsigned long long)__popcll(eq));
}

__global__ __launch_bounds__(64) void k_nam_scatter(u32 a, u32 n, const u64* fl, const u64* flOff, const u32* newIdx, const u32* gp, u32* order, u32* idx2, u32* seg2, u32* gp2)
{
    const u32 j = blockIdx.x * 64u + threadIdx.x;
    if(j >= a) return;
    const u64 f = fl[j], o = flOff[j];
    const u32 g = gp[j];
    if(!(f & 1u)) { if(g < n) order[g] = newIdx[j]; return; }
    const u32 t = (u32)o, s = (u32)(o >> 32) + (u32)(f >> 32);        // (kept slots before this one; kept segment starts up to and including this one)
    if(t >= a || s == 0) return;
    idx2[t] = newIdx[j]; seg2[t] = s - 1u; gp2[t] = g;
}

}  // namespace hlala

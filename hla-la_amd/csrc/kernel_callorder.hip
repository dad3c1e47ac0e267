// kernel_callorder.hip -- the order of the all-pairs table on gfx950 (opt-in: hlala_set_call_order_gpu, hlala_pair_order_gpu).  The rule is call_order_core.h: the
// steps of libstdc++'s std::sort, of which the ranges of one recursion level are independent and the two-cursor partition has a closed form.
//
//   k_ord_load   : keyed elements (integer images of LL and Mism_avg, the pair's index) from the device tables; a NaN in either key raises a flag
//   k_ord_level  : one workgroup per range of more than ORD_TILE elements: the median of three to `first`; ONE walk over the range from both ends, ORD_CHUNK elements
//                  per side and step, that ranks the elements stopping the left cursor (ascending) and the right cursor (descending) -- ballot + popcount per
//                  wavefront, the 64 wavefront sums of a step scanned by wavefront 0, the counts carried from step to step -- and writes their places to the
//                  range's slices of two lists; then swap k for every k with I[k] < J[k]; then the cut, and the two children appended to the list of their
//                  class: the next level, the tile kernel, the heap kernel, or refused.  No workgroup waits for another one: the host reads the list counters
//                  after each level and sizes the next launch with them.  The walk of a large range by a single workgroup is what bounds the first levels.
//   k_ord_tile   : one workgroup (one wavefront) per range that fits: the range goes to LDS, lane 0 runs the serial form (the remaining partitions with the depth
//                  carried, heap sort where the depth is spent, insertion per range of at most 16), the range goes back.  <ORD_TILE> for the tile list, six
//                  workgroups per CU; <ORD_MAX_HEAP> for the ranges above the tile size that were met with no depth left.
//   k_ord_emit   : order[n - 1 - i] = index of element i.
#include "device_common.h"
#include "call_order_core.h"

namespace hlala {

using hlala_order::OrdEl; using hlala_order::OrdRange;

// device counters of one order
enum { OD_NAN = 0, OD_NEXT, OD_TILES, OD_HEAPLIST, OD_LARGEST_TILE, OD_HEAPS, OD_LARGEST_HEAP, OD_REFUSED, OD_OVERFLOW, OD_N = 16 };

struct OrdLists { OrdRange *next, *tiles, *heaps; u32 capNext, capTiles, capHeaps; };

__global__ void k_ord_load(u32 n, const double* __restrict__ ll, const double* __restrict__ ma, OrdEl* __restrict__ a, u32* __restrict__ cnt)
{
    bool nan = false;
    for(u32 i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const double l = ll[i], m = ma[i];
        nan = nan || hlala_order::ord_is_nan(l) || hlala_order::ord_is_nan(m);
        a[i] = hlala_order::ord_element(l, m, i);
    }
    if(nan) atomicOr(&cnt[OD_NAN], 1u);
}

// a child of a partition to the list of its class
__device__ __forceinline__ void ord_place(u32 first, u32 last, u32 depth, const OrdLists& Ls, u32* cnt)
{
    using namespace hlala_order;
    const u32 len = last - first;
    OrdRange* list = nullptr; u32 cap = 0, at = 0;
    switch(ord_child_class(len, depth)) {
    case ORD_TO_LEVEL: list = Ls.next; cap = Ls.capNext; at = atomicAdd(&cnt[OD_NEXT], 1u); break;
    case ORD_TO_TILE: list = Ls.tiles; cap = Ls.capTiles; at = atomicAdd(&cnt[OD_TILES], 1u); atomicMax(&cnt[OD_LARGEST_TILE], len); break;
    case ORD_TO_HEAP: list = Ls.heaps; cap = Ls.capHeaps; at = atomicAdd(&cnt[OD_HEAPLIST], 1u); break;
    case ORD_TO_REFUSE: atomicAdd(&cnt[OD_HEAPS], 1u); atomicMax(&cnt[OD_LARGEST_HEAP], len); atomicOr(&cnt[OD_REFUSED], 1u); return;
    default: return;
    }
    if(at < cap) { list[at].first = first; list[at].last = last; list[at].depth = depth; }
    else atomicOr(&cnt[OD_OVERFLOW], 1u);                       // (no table reaches it: ord_list_capacity)
}
// the table itself is placed like a child
__global__ void k_ord_root(u32 n, OrdLists Ls, u32* __restrict__ cnt)
{
    if(blockIdx.x == 0 && threadIdx.x == 0) ord_place(0, n, hlala_order::ord_start_depth(n), Ls, cnt);
}

__global__ __launch_bounds__(hlala_order::ORD_BLOCK) void k_ord_level(OrdEl* a, u32* I, u32* J, const OrdRange* __restrict__ cur, OrdLists Ls,
                                                                      u32* __restrict__ cnt)
{
    using namespace hlala_order;
    constexpr u32 WAVES = ORD_BLOCK / 64, SUMS = ORD_ITEMS * WAVES;
    static_assert(SUMS == 64, "wavefront 0 scans the wavefront sums of one step, one per lane");
    __shared__ u32 sCnt[2][2][SUMS], sPre[2][2][SUMS], sTot[2], sSwaps;
    __shared__ OrdEl sPv;
    const u32 tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const u32 first = cur[blockIdx.x].first, last = cur[blockIdx.x].last, depth = cur[blockIdx.x].depth - 1;
    if(tid == 0) {
        const u32 m = ord_median(a, first, last);
        const OrdEl t = a[first]; a[first] = a[m]; a[m] = t;
        sPv = a[first]; sSwaps = 0;
    }
    __syncthreads();
    const OrdEl pv = sPv;
    const u32 side = last - first - 1;                          // places of [first + 1, last)
    const u64 below = lane ? (~0ull >> (64u - lane)) : 0ull;
    u32 baseI = 0, baseJ = 0;                                   // (carried by wavefront 0)
    for(u32 q0 = 0, p = 0; q0 < side; q0 += ORD_CHUNK, p ^= 1u) {
        bool stopI[ORD_ITEMS], stopJ[ORD_ITEMS]; u32 rankI[ORD_ITEMS], rankJ[ORD_ITEMS];
        u64 eL[ORD_ITEMS], eM[ORD_ITEMS], fL[ORD_ITEMS], fM[ORD_ITEMS];
#pragma unroll
        for(u32 k = 0; k < ORD_ITEMS; k++) {
            const u32 q = q0 + k * ORD_BLOCK + tid;
            if(q < side) { eL[k] = a[first + 1 + q].L; eM[k] = a[first + 1 + q].M; fL[k] = a[last - 1 - q].L; fM[k] = a[last - 1 - q].M; }
            else { eL[k] = eM[k] = fL[k] = fM[k] = 0; }
        }
#pragma unroll
        for(u32 k = 0; k < ORD_ITEMS; k++) {
            const u32 q = q0 + k * ORD_BLOCK + tid;
            stopI[k] = q < side && !ord_less(eL[k], eM[k], pv.L, pv.M);
            stopJ[k] = q < side && !ord_less(pv.L, pv.M, fL[k], fM[k]);
            const u64 bI = __ballot(stopI[k]), bJ = __ballot(stopJ[k]);
            rankI[k] = (u32)__popcll(bI & below); rankJ[k] = (u32)__popcll(bJ & below);
            if(lane == 0) { sCnt[p][0][k * WAVES + wave] = (u32)__popcll(bI); sCnt[p][1][k * WAVES + wave] = (u32)__popcll(bJ); }
        }
        __syncthreads();
        if(wave == 0) {
            const u32 cI = sCnt[p][0][lane], cJ = sCnt[p][1][lane];
            u32 xI = cI, xJ = cJ;
            for(u32 d = 1; d < 64; d <<= 1) { const u32 yI = __shfl_up(xI, d), yJ = __shfl_up(xJ, d); if(lane >= d) { xI += yI; xJ += yJ; } }
            sPre[p][0][lane] = baseI + xI - cI; sPre[p][1][lane] = baseJ + xJ - cJ;
            baseI += __shfl(xI, 63); baseJ += __shfl(xJ, 63);
        }
        __syncthreads();
#pragma unroll
        for(u32 k = 0; k < ORD_ITEMS; k++) {
            const u32 q = q0 + k * ORD_BLOCK + tid;
            if(stopI[k]) { const u32 r = sPre[p][0][k * WAVES + wave] + rankI[k]; if(r < side) I[first + r] = first + 1 + q; }
            if(stopJ[k]) { const u32 r = sPre[p][1][k * WAVES + wave] + rankJ[k]; if(r < side) J[first + r] = last - 1 - q; }
        }
    }
    if(tid == 0) { sTot[0] = baseI; sTot[1] = baseJ; }
    __threadfence();
    __syncthreads();
    const u32 nI = sTot[0], nJ = sTot[1], both = nI < nJ ? nI : nJ;
    u32 mine = 0;
    for(u32 k = tid; k < both; k += ORD_BLOCK) {
        const u32 i = I[first + k], j = J[first + k];
        if(!(i < j)) break;                                     // (the i ascend, the j descend: nothing beyond)
        const OrdEl t = a[i]; a[i] = a[j]; a[j] = t;
        mine++;
    }
    if(mine) atomicAdd(&sSwaps, mine);
    __syncthreads();
    if(tid == 0) {
        const u32 s = sSwaps;
        const u32 cut = ord_cut(s, nI, nJ, s < nI ? I[first + s] : last, s > 0 ? J[first + s - 1] : last, last);
        ord_place(cut, last, depth, Ls, cnt);
        ord_place(first, cut, depth, Ls, cnt);
    }
}

template<u32 CAP>
__global__ __launch_bounds__(64) void k_ord_tile(OrdEl* __restrict__ a, const OrdRange* __restrict__ list, u32* __restrict__ cnt)
{
    using namespace hlala_order;
    __shared__ OrdEl t[CAP];
    __shared__ u32 stack[3 * ORD_STACK];
    const u32 first = list[blockIdx.x].first, last = list[blockIdx.x].last, depth = list[blockIdx.x].depth, len = last - first;
    if(last < first || len > CAP) { if(threadIdx.x == 0) atomicOr(&cnt[OD_OVERFLOW], 2u); return; }
    for(u32 i = threadIdx.x; i < len; i += 64) t[i] = a[first + i];
    __syncthreads();
    if(threadIdx.x == 0) {
        u32 heaps = 0, largest = 0;
        if(ord_sort_serial(t, len, depth, stack, &heaps, &largest) == ORD_OVERFLOW) atomicOr(&cnt[OD_OVERFLOW], 4u);
        if(heaps) { atomicAdd(&cnt[OD_HEAPS], heaps); atomicMax(&cnt[OD_LARGEST_HEAP], largest); }
    }
    __syncthreads();
    for(u32 i = threadIdx.x; i < len; i += 64) a[first + i] = t[i];
}

__global__ void k_ord_emit(u32 n, const OrdEl* __restrict__ a, int* __restrict__ order)
{
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if(i < n) order[n - 1 - i] = (int)a[i].i;
}

}  // namespace hlala

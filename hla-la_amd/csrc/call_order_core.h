// call_order_core.h -- the order of the all-pairs table (hla/HLATyper.cpp:2381-2403: std::sort with the comparator below, then std::reverse), shared by the device
// kernels (kernel_callorder.hip) and by the host model (call_order_model.h; host_check.cpp: hlala_host_pair_order_model).  Plain inline functions, no HIP types: g++
// and hipcc compile the same text.
//
// The rule.  Pairs equal in both keys come out of libstdc++'s std::sort in the order its steps leave them in, so those steps are run here (bam_fill_wide_core.h has
// them for one small array; this header has them for a table of millions, in a form that a grid can work on):
//   * a range of more than ORD_CUT elements with depth left (2 * floor(log2 n) at the start, one less per cut): the median of the elements at first + 1, the middle and
//     last - 1 goes to `first`, [first + 1, last) is partitioned around it, and [cut, last) and [first, cut) go on independently with the depth left;
//   * the partition in CLOSED FORM.  Let i_0 < i_1 < .. be the places of [first + 1, last) with !(a[i] < pivot) and j_0 > j_1 > .. those with !(pivot < a[j]).  The
//     library's two cursors swap a[i_k] with a[j_k] for exactly the k with i_k < j_k -- the first s of them, since the i ascend and the j descend -- and return
//     cut = min(i_s, j_(s-1)), a missing one read as `last`.  (After s swaps the left cursor goes on over untouched elements until i_s, but a[j_(s-1)] now holds an
//     element it stops at.)  No swap depends on another: a level of the recursion is two rank scans and one pass of swaps;
//   * a range of more than ORD_CUT elements met with no depth left is heap-sorted;
//   * the final insertion sort never moves an element across the border of a range of the first step (the comparison is strict and nothing left of a range is
//     greater than anything in it), and guarded or not it leaves what a plain insertion sort leaves: one stable insertion sort per range of at most ORD_CUT;
//   * the result is reversed.
// An element carries its keys as integer images that compare as the doubles do (-0 == +0; no NaN: std::sort is undefined there and the callers refuse it) and its
// index: the sequence of comparisons and moves does not depend on the element type (hlala_api.hip: call_locus_impl says why), so the permutation is the reference's.
//
// Every loop is bounded for ANY keys: the cursors of the serial partition stop at the ends of their range, a sift moves one level of the heap per step, an insertion
// cursor stops at the range's first place, and the stack refuses to grow beyond ORD_STACK (which no input reaches: every range pushed carries a smaller depth than
// the one below it, and a depth is below 64).
#ifndef HLALA_CALL_ORDER_CORE_H_
#define HLALA_CALL_ORDER_CORE_H_
#include <stdint.h>
#include <string.h>

#include "../../include/hlala_gpu.h"

#ifndef HLALA_HD
#ifdef __HIPCC__
#define HLALA_HD __host__ __device__ inline
#else
#define HLALA_HD inline
#endif
#endif

namespace hlala_order {

constexpr uint32_t ORD_CUT = 16;                                // ranges up to here are left to the insertion pass
constexpr uint32_t ORD_TILE = 1024;                             // a range up to here is finished by one workgroup in LDS (24 KiB: six workgroups per CU); 1024 measured against 2048 and 4096
constexpr uint32_t ORD_MAX_HEAP = HLALA_CALL_ORDER_MAX_HEAP;    // the largest range with no depth left that the device heap-sorts (in LDS, 96 KiB)
constexpr uint32_t ORD_BLOCK = 1024;                            // threads of the workgroup that partitions one range of a grid level
constexpr uint32_t ORD_ITEMS = 4;                               // elements per thread and side of one step of its rank scans
constexpr uint32_t ORD_CHUNK = ORD_BLOCK * ORD_ITEMS;           // elements per side of one step
constexpr uint32_t ORD_STACK = 64;                              // ranges on the stack of the serial form
constexpr uint32_t ORD_OVERFLOW = 0xFFFFFFFFu;
static_assert(ORD_TILE >= 1024 && ORD_TILE <= 4096 && ORD_TILE <= ORD_MAX_HEAP && ORD_TILE > ORD_CUT, "the tile size");

// counts[8] of hlala_call_order_counts / hlala_pair_order_gpu / hlala_host_pair_order_model
enum { OC_PATH = 0, OC_LEVELS, OC_TILE_RANGES, OC_LARGEST_TILE, OC_HEAPS, OC_LARGEST_HEAP, OC_BYTES_UP, OC_BYTES_DOWN, OC_N };
static_assert(OC_N == HLALA_CALL_ORDER_COUNTS, "include/hlala_gpu.h: counts of the call order");

struct OrdEl { uint64_t L, M; uint32_t i, pad; };               // images of LL and Mism_avg, the pair's index
struct OrdRange { uint32_t first, last, depth; };

HLALA_HD uint64_t ord_image(double d)
{
    if(d == 0.0) d = 0.0;                                                       // -0 compares equal to +0
    uint64_t b; memcpy(&b, &d, sizeof(b));
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
HLALA_HD bool ord_is_nan(double d) { return d != d; }
// a.ll == b.ll ? b.ma < a.ma : a.ll < b.ll  --  M is the complement of Mism_avg's image
HLALA_HD OrdEl ord_element(double ll, double ma, uint32_t i) { OrdEl e; e.L = ord_image(ll); e.M = ~ord_image(ma); e.i = i; e.pad = 0; return e; }
HLALA_HD bool ord_less(uint64_t aL, uint64_t aM, uint64_t bL, uint64_t bM) { return aL == bL ? aM < bM : aL < bL; }
HLALA_HD bool ord_less(const OrdEl& a, const OrdEl& b) { return ord_less(a.L, a.M, b.L, b.M); }
HLALA_HD uint32_t ord_floor_log2(uint64_t n) { uint32_t k = 0; while(n > 1) { n >>= 1; k++; } return k; }
HLALA_HD uint32_t ord_start_depth(uint64_t n) { return 2 * ord_floor_log2(n); }

// the place of the median of a[first + 1], a[first + (last - first) / 2], a[last - 1] as the library picks it (it goes to `first`)
template<class A> HLALA_HD uint32_t ord_median(const A& a, uint32_t first, uint32_t last)
{
    const uint32_t x = first + 1, y = first + (last - first) / 2, z = last - 1;
    if(ord_less(a[x], a[y])) return ord_less(a[y], a[z]) ? y : (ord_less(a[x], a[z]) ? z : x);
    return ord_less(a[x], a[z]) ? x : (ord_less(a[y], a[z]) ? z : y);
}
// closed form: the element stops the left cursor / the right cursor
HLALA_HD bool ord_stops_left(const OrdEl& e, const OrdEl& pv) { return !ord_less(e, pv); }
HLALA_HD bool ord_stops_right(const OrdEl& e, const OrdEl& pv) { return !ord_less(pv, e); }
// closed form: with s swaps made, nI places that stop the left cursor and nJ that stop the right one: i_s (or last) and j_(s-1) (or last) -> the cut
HLALA_HD uint32_t ord_cut(uint32_t s, uint32_t nI, uint32_t nJ, uint32_t i_s, uint32_t j_s1, uint32_t last)
{
    (void)nJ;
    const uint32_t a = s < nI ? i_s : last, b = s > 0 ? j_s1 : last;
    return a < b ? a : b;
}
// where a child of a grid level goes
enum { ORD_TO_LEVEL = 0, ORD_TO_TILE = 1, ORD_TO_HEAP = 2, ORD_TO_REFUSE = 3, ORD_TO_NOTHING = 4 };
HLALA_HD int ord_child_class(uint32_t len, uint32_t depth)
{
    if(len < 2) return ORD_TO_NOTHING;
    if(len <= ORD_TILE) return ORD_TO_TILE;
    if(depth > 0) return ORD_TO_LEVEL;
    return len <= ORD_MAX_HEAP ? ORD_TO_HEAP : ORD_TO_REFUSE;
}

// ---- the serial form, for a range that fits a tile: a[0, n) with `depth` left
HLALA_HD void ord_sift(OrdEl* a, uint32_t base, uint32_t hole, uint32_t len, const OrdEl v)
{
    const uint32_t top = hole;
    uint32_t child = hole;
    while(child < (len - 1) / 2) {
        child = 2 * (child + 1);
        if(ord_less(a[base + child], a[base + child - 1])) child--;
        a[base + hole] = a[base + child]; hole = child;
    }
    if((len & 1u) == 0 && len >= 2 && child == (len - 2) / 2) {                 // an even heap: the last parent has a left child only
        child = 2 * (child + 1);
        a[base + hole] = a[base + child - 1]; hole = child - 1;
    }
    while(hole > top) {
        const uint32_t parent = (hole - 1) / 2;
        if(!ord_less(a[base + parent], v)) break;
        a[base + hole] = a[base + parent]; hole = parent;
    }
    a[base + hole] = v;
}
HLALA_HD void ord_heap_sort(OrdEl* a, uint32_t first, uint32_t last)
{
    const uint32_t len = last - first;
    if(len < 2) return;
    for(uint32_t parent = (len - 2) / 2 + 1; parent-- > 0;) ord_sift(a, first, parent, len, a[first + parent]);
    for(uint32_t end = len - 1; end >= 1; end--) {
        const OrdEl v = a[first + end];
        a[first + end] = a[first];
        ord_sift(a, first, 0, end, v);
    }
}
// stable insertion sort of [first, last)
HLALA_HD void ord_insertion(OrdEl* a, uint32_t first, uint32_t last)
{
    for(uint32_t i = first + 1; i < last; i++) {
        const OrdEl v = a[i];
        uint32_t j = i;
        while(j > first && ord_less(v, a[j - 1])) { a[j] = a[j - 1]; j--; }
        a[j] = v;
    }
}
// stack: 3 * ORD_STACK words of the caller's.  heaps / largest_heap: heap sorts entered and the largest range so sorted are ADDED / MAXED into them.  Returns 0, or
// ORD_OVERFLOW for a stack that would overflow (the elements are still the same ones then).  Not reversed: the caller reverses the whole table.
HLALA_HD uint32_t ord_sort_serial(OrdEl* a, uint32_t n, uint32_t depth, uint32_t* stack, uint32_t* heaps, uint32_t* largest_heap)
{
    uint32_t sp = 0, first = 0, last = n;
    for(;;) {
        while(last - first > ORD_CUT) {
            if(depth == 0) { ord_heap_sort(a, first, last); (*heaps)++; if(last - first > *largest_heap) *largest_heap = last - first; break; }
            depth--;
            const uint32_t m = ord_median(a, first, last);
            { const OrdEl t = a[first]; a[first] = a[m]; a[m] = t; }
            const OrdEl pv = a[first];
            uint32_t lo = first + 1, hi = last;
            for(;;) {
                while(lo < last && ord_less(a[lo], pv)) lo++;
                hi--;
                while(hi > first && ord_less(pv, a[hi])) hi--;
                if(!(lo < hi)) break;
                { const OrdEl t = a[lo]; a[lo] = a[hi]; a[hi] = t; }
                lo++;
            }
            if(sp >= ORD_STACK) return ORD_OVERFLOW;
            stack[3 * sp] = first; stack[3 * sp + 1] = lo; stack[3 * sp + 2] = depth; sp++;
            first = lo;
        }
        if(last - first <= ORD_CUT) ord_insertion(a, first, last);
        if(sp == 0) break;
        sp--; first = stack[3 * sp]; last = stack[3 * sp + 1]; depth = stack[3 * sp + 2];
    }
    return 0;
}

// most ranges the tile kernel can be handed: the ranges partitioned at one level are disjoint and larger than ORD_TILE, each leaves two children, and there are at
// most 2 * floor(log2 n) levels; plus the table itself
HLALA_HD uint64_t ord_list_capacity(uint64_t n) { return 2 * (n / ORD_TILE + 1) * (uint64_t)(ord_start_depth(n) + 1) + 1; }

}  // namespace hlala_order
#endif

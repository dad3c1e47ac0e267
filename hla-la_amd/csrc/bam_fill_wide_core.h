// bam_fill_wide_core.h -- the order sortChainsInSeeds leaves for a mate of MORE than 16 alignments, shared by the device kernel (kernel_bamfill.hip: k_fil_wide_rank) and
// by the host model (bam_fill_model.h; host_check.cpp: hlala_host_bam_fill_model_wide).  Plain inline functions, no HIP types: g++ and hipcc compile the same text.
//
// The rule.  The reference sorts the mate's alignments with std::sort ascending by AS and reverses the result (sorted_mate in host_bam.cpp).  Beyond 16 elements
// libstdc++'s std::sort is an introsort: not stable, and the order it leaves among equal scores is whatever its steps leave.  Equal scores are the normal case among
// secondary alignments, and the place of the first primary depends on them, so fil_sort_wide runs those steps, written down from the algorithm's description and
// checked against the library (tools/bam_fill_wide_check.cpp):
//   * while a range holds more than 16 elements and depth is left (2 * floor(log2 n) at the start, one less per cut): the median of the elements at first + 1, the
//     middle and last - 1 goes to `first`; the rest is partitioned around it by two cursors that swap what they stop at; the right part is a range of its own with the
//     depth left, the left part goes on;
//   * a range of more than 16 elements met with no depth left is heap-sorted: a max-heap built from the last parent down, then the top taken out until one is left;
//   * at the end one insertion sort over everything: guarded against the first element on the first 16 places, unguarded on the rest.
// The ranges of the first step are disjoint and each step touches its own range only, so the order in which the ranges are worked on does not change the result: the
// recursion is an explicit stack here.  Every range pushed carries a depth smaller than the one below it, and the depths lie in [0, 2 * floor(log2 n)): at most
// 2 * floor(log2 n) entries, FIL_WIDE_STACK for n <= FIL_WIDE_MAX.
//
// Every loop is bounded by n for ANY scores.  The comparison is `<` on 32-bit integers, a strict weak order whatever the values, which is what lets the library run its
// cursors unguarded; here every cursor is held inside its range all the same (a test that never fires and so does not change the result): a partition cursor stops at
// the range's ends and one of them advances in every round; a sift goes down one level of the heap per step and up one level per step; an insertion cursor stops at
// place 0; the stack refuses to grow beyond its capacity (FIL_WIDE_OVERFLOW, which no input reaches).
#ifndef HLALA_BAM_FILL_WIDE_CORE_H_
#define HLALA_BAM_FILL_WIDE_CORE_H_
#include "bam_fill_core.h"

namespace hlala_bamfill {

constexpr uint32_t FIL_WIDE_MAX = HLALA_BAM_FILL_WIDE_MAX;      // alignments of one mate the wide path takes: scores (4 bytes) and places (2 bytes) of one mate in 24 KB of LDS
constexpr uint32_t FIL_WIDE_STACK = 2 * 12 + 1;                 // ranges on the stack: 2 * floor(log2 FIL_WIDE_MAX) + 1
constexpr uint32_t FIL_WIDE_STACK_WORDS = 3 * FIL_WIDE_STACK;   // (first, last, depth) per range
constexpr uint32_t FIL_WIDE_CUT = 16;                           // ranges up to here are left to the final insertion sort
constexpr uint32_t FIL_WIDE_OVERFLOW = 0xFFFFFFFFu;
static_assert(FIL_WIDE_MAX == 4096, "FIL_WIDE_STACK states floor(log2 FIL_WIDE_MAX) = 12");
static_assert(FIL_WIDE_CUT == FIL_MAX_MATE, "the narrow path claims its closed form exactly where the library still sorts by insertion");

// a unit takes the wide path: more records than the narrow kernels look at, or more alignments on a mate than their closed form is claimed for
HLALA_HD bool fil_is_wide(uint32_t unit_count, uint32_t mate0, uint32_t mate1) { return unit_count > FIL_MAX_UNIT || mate0 > FIL_MAX_MATE || mate1 > FIL_MAX_MATE; }

HLALA_HD uint32_t fil_floor_log2(uint32_t n) { uint32_t k = 0; while(n > 1) { n >>= 1; k++; } return k; }
HLALA_HD void fil_w_swap(int32_t* s, uint16_t* p, uint32_t a, uint32_t b)
{
    const int32_t ts = s[a]; s[a] = s[b]; s[b] = ts;
    const uint16_t tp = p[a]; p[a] = p[b]; p[b] = tp;
}
// the heap s[base, base + len): the hole at `hole` sinks to a leaf along the greater children (the left one where they tie), then the value (vs, vp) rises from there
HLALA_HD void fil_w_sift(int32_t* s, uint16_t* p, uint32_t base, uint32_t hole, uint32_t len, int32_t vs, uint16_t vp)
{
    const uint32_t top = hole;
    uint32_t child = hole;
    while(child < (len - 1) / 2) {
        child = 2 * (child + 1);
        if(s[base + child] < s[base + child - 1]) child--;
        s[base + hole] = s[base + child]; p[base + hole] = p[base + child]; hole = child;
    }
    if((len & 1u) == 0 && len >= 2 && child == (len - 2) / 2) {                 // an even heap: the last parent has a left child only
        child = 2 * (child + 1);
        s[base + hole] = s[base + child - 1]; p[base + hole] = p[base + child - 1]; hole = child - 1;
    }
    while(hole > top) {
        const uint32_t parent = (hole - 1) / 2;
        if(!(s[base + parent] < vs)) break;
        s[base + hole] = s[base + parent]; p[base + hole] = p[base + parent]; hole = parent;
    }
    s[base + hole] = vs; p[base + hole] = vp;
}
HLALA_HD void fil_w_heap_sort(int32_t* s, uint16_t* p, uint32_t first, uint32_t last)
{
    const uint32_t len = last - first;
    if(len < 2) return;
    for(uint32_t parent = (len - 2) / 2 + 1; parent-- > 0;) fil_w_sift(s, p, first, parent, len, s[first + parent], p[first + parent]);
    for(uint32_t end = len - 1; end >= 1; end--) {
        const int32_t vs = s[first + end]; const uint16_t vp = p[first + end];
        s[first + end] = s[first]; p[first + end] = p[first];
        fil_w_sift(s, p, first, 0, end, vs, vp);
    }
}
// insertion sort of [0, m) guarded against place 0, then of [m, n) unguarded (every element there has a smaller-or-equal one before it; the cursor stops at 0 anyway)
HLALA_HD void fil_w_insertion(int32_t* s, uint16_t* p, uint32_t m, uint32_t n)
{
    for(uint32_t i = 1; i < n; i++) {
        const int32_t vs = s[i]; const uint16_t vp = p[i];
        uint32_t j = i;
        if(i < m && vs < s[0]) { for(; j > 0; j--) { s[j] = s[j - 1]; p[j] = p[j - 1]; } }
        else while(j > 0 && vs < s[j - 1]) { s[j] = s[j - 1]; p[j] = p[j - 1]; j--; }
        s[j] = vs; p[j] = vp;
    }
}

// score[0, n) and place[0, n) in file order -> the order sortChainsInSeeds leaves (std::sort ascending by score, then std::reverse).  stack: FIL_WIDE_STACK_WORDS words
// of the caller's.  Returns how often the heap-sort branch was entered, or FIL_WIDE_OVERFLOW (n beyond FIL_WIDE_MAX or a stack that would overflow: nothing is promised
// about the arrays' order then, but they still hold the same elements).
HLALA_HD uint32_t fil_sort_wide(int32_t* score, uint16_t* place, uint32_t n, uint32_t* stack)
{
    if(n > FIL_WIDE_MAX) return FIL_WIDE_OVERFLOW;
    uint32_t heaps = 0;
    if(n > FIL_WIDE_CUT) {
        uint32_t sp = 0, first = 0, last = n, depth = 2 * fil_floor_log2(n);
        for(;;) {
            while(last - first > FIL_WIDE_CUT) {
                if(depth == 0) { fil_w_heap_sort(score, place, first, last); heaps++; break; }
                depth--;
                // the median of three to `first`
                const uint32_t a = first + 1, b = first + (last - first) / 2, c = last - 1;
                const int32_t sa = score[a], sb = score[b], sc = score[c];
                uint32_t m;
                if(sa < sb) m = sb < sc ? b : (sa < sc ? c : a);
                else m = sa < sc ? a : (sb < sc ? c : b);
                fil_w_swap(score, place, first, m);
                // two cursors around the pivot, which stays at `first`
                const int32_t pv = score[first];
                uint32_t lo = first + 1, hi = last;
                for(;;) {
                    while(lo < last && score[lo] < pv) lo++;
                    hi--;
                    while(hi > first && pv < score[hi]) hi--;
                    if(!(lo < hi)) break;
                    fil_w_swap(score, place, lo, hi);
                    lo++;
                }
                // [lo, last) now, [first, lo) later
                if(sp >= FIL_WIDE_STACK) return FIL_WIDE_OVERFLOW;
                stack[3 * sp] = first; stack[3 * sp + 1] = lo; stack[3 * sp + 2] = depth; sp++;
                first = lo;
            }
            if(sp == 0) break;
            sp--; first = stack[3 * sp]; last = stack[3 * sp + 1]; depth = stack[3 * sp + 2];
        }
        fil_w_insertion(score, place, FIL_WIDE_CUT, n);
    } else fil_w_insertion(score, place, n, n);
    for(uint32_t i = 0, j = n; i + 1 < j; i++) { j--; fil_w_swap(score, place, i, j); }
    return heaps;
}

// The arguments of hlala_bam_fill_create_wide / hlala_host_bam_fill_model_wide: the checks of fil_check_args with max_mate, which lies in (FIL_MAX_MATE, FIL_WIDE_MAX],
// in the place of FIL_MAX_MATE.
inline const char* fil_check_args_wide(const hlala_bam_fill_in* in, int32_t max_mate, const int64_t* read_off, const int64_t* chain_off, const int64_t* cigar_count, const int64_t* name_off,
                                       const hlala_bam_fill_stats* stats)
{
    if(max_mate <= (int32_t)FIL_MAX_MATE || max_mate > (int32_t)FIL_WIDE_MAX) return "max_mate outside (16, 4096]";
    return fil_check_args_cap(in, read_off, chain_off, cigar_count, name_off, stats, (uint32_t)max_mate, "a filled unit with more alignments on one mate than max_mate");
}

}  // namespace hlala_bamfill
#endif

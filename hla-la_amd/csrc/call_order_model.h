// call_order_model.h -- the launches of the device path for the order of the pair table (kernel_callorder.hip) run serially on the host over the same core
// (call_order_core.h): grid levels with the closed form of the partition down to the tile size, then the serial form per tile, then the reversal.  Same counters as
// the device (levels, tile ranges, heap sorts), no cap on a heap range: the model sorts what the device refuses and says in counts[0] what the device would answer.
#ifndef HLALA_CALL_ORDER_MODEL_H_
#define HLALA_CALL_ORDER_MODEL_H_
#include <algorithm>
#include <string>
#include <vector>

#include "call_order_core.h"

namespace hlala_order {

// std::sort + std::reverse with the comparator of call_locus_impl (hlala_api.hip): the specification, for any n
inline void pair_order_reference(int64_t n, const double* ll, const double* ma, int32_t* order)
{
    struct Keyed { double ll, ma; int32_t i; };
    std::vector<Keyed> keyed((size_t)n);
    for(int64_t i = 0; i < n; i++) keyed[(size_t)i] = Keyed{ll[i], ma[i], (int32_t)i};
    std::sort(keyed.begin(), keyed.end(), [](const Keyed& a, const Keyed& b) {
        if(a.ll == b.ll) return (b.ma < a.ma);
        else return (a.ll < b.ll);
    });
    std::reverse(keyed.begin(), keyed.end());
    for(int64_t i = 0; i < n; i++) order[i] = keyed[(size_t)i].i;
}

inline const char* ord_check_args(int64_t n, const double* ll, const double* ma, const int32_t* order)
{
    if(n < 1) return "n below 1";
    if(n >= (int64_t)1 << 31) return "n beyond 31 bits";
    if(!ll || !ma || !order) return "a null pointer";
    return nullptr;
}

// one range of a grid level: the median to `first`, the two rank lists, the swaps, the cut.  I / J: scratch of the caller's
inline uint32_t ord_partition_closed(std::vector<OrdEl>& a, uint32_t first, uint32_t last, std::vector<uint32_t>& I, std::vector<uint32_t>& J)
{
    std::swap(a[first], a[ord_median(a, first, last)]);
    const OrdEl pv = a[first];
    I.clear(); J.clear();
    for(uint32_t q = 0; q + 1 < last - first; q++) {
        if(ord_stops_left(a[first + 1 + q], pv)) I.push_back(first + 1 + q);
        if(ord_stops_right(a[last - 1 - q], pv)) J.push_back(last - 1 - q);
    }
    const size_t m = std::min(I.size(), J.size());
    uint32_t s = 0;
    for(size_t k = 0; k < m; k++) if(I[k] < J[k]) { std::swap(a[I[k]], a[J[k]]); s++; }
    return ord_cut(s, (uint32_t)I.size(), (uint32_t)J.size(), s < I.size() ? I[s] : last, s > 0 ? J[s - 1] : last, last);
}

// returns HLALA_OK, HLALA_E_ARG, or HLALA_E_CAPACITY ("not available:", nothing written) for a NaN key
inline int pair_order_model(int64_t n, const double* ll, const double* ma, int32_t* order, int64_t* counts, std::string* why)
{
    if(const char* bad = ord_check_args(n, ll, ma, order)) { *why = bad; return HLALA_E_ARG; }
    for(int64_t i = 0; i < n; i++) if(ord_is_nan(ll[i]) || ord_is_nan(ma[i])) { *why = "not available: a NaN key at pair " + std::to_string(i) + " of " + std::to_string(n); return HLALA_E_CAPACITY; }
    int64_t Cn[OC_N] = {HLALA_CALL_ORDER_DEVICE, 0, 0, 0, 0, 0, 0, 0};
    std::vector<OrdEl> a((size_t)n);
    for(int64_t i = 0; i < n; i++) a[(size_t)i] = ord_element(ll[i], ma[i], (uint32_t)i);
    std::vector<OrdRange> cur, next, tiles, beyond;
    auto place = [&](uint32_t first, uint32_t last, uint32_t depth, std::vector<OrdRange>& level) {
        const uint32_t len = last - first;
        switch(ord_child_class(len, depth)) {
        case ORD_TO_LEVEL: level.push_back(OrdRange{first, last, depth}); break;
        case ORD_TO_TILE: tiles.push_back(OrdRange{first, last, depth}); Cn[OC_TILE_RANGES]++; if(len > Cn[OC_LARGEST_TILE]) Cn[OC_LARGEST_TILE] = len; break;
        case ORD_TO_HEAP: tiles.push_back(OrdRange{first, last, depth}); break;
        case ORD_TO_REFUSE: beyond.push_back(OrdRange{first, last, depth}); break;
        default: break;
        }
    };
    place(0, (uint32_t)n, ord_start_depth((uint64_t)n), cur);
    std::vector<uint32_t> I, J;
    while(!cur.empty()) {
        Cn[OC_LEVELS]++;
        next.clear();
        for(const OrdRange& r : cur) {
            const uint32_t cut = ord_partition_closed(a, r.first, r.last, I, J);
            place(cut, r.last, r.depth - 1, next);
            place(r.first, cut, r.depth - 1, next);
        }
        cur.swap(next);
    }
    std::vector<OrdEl> tile(ORD_MAX_HEAP);
    uint32_t stack[3 * ORD_STACK], heaps = 0, largest = 0;
    for(const OrdRange& r : tiles) {
        const uint32_t len = r.last - r.first;
        std::copy(a.begin() + r.first, a.begin() + r.last, tile.begin());
        if(ord_sort_serial(tile.data(), len, r.depth, stack, &heaps, &largest) == ORD_OVERFLOW) { *why = "the stack of the serial form overflowed"; return HLALA_E_ARG; }
        std::copy(tile.begin(), tile.begin() + len, a.begin() + r.first);
    }
    for(const OrdRange& r : beyond) { ord_heap_sort(a.data(), r.first, r.last); heaps++; if(r.last - r.first > largest) largest = r.last - r.first; }
    Cn[OC_HEAPS] = heaps; Cn[OC_LARGEST_HEAP] = largest;
    if(!beyond.empty()) Cn[OC_PATH] = HLALA_CALL_ORDER_REFUSED_HEAP;
    for(int64_t i = 0; i < n; i++) order[n - 1 - i] = (int32_t)a[(size_t)i].i;
    if(counts) memcpy(counts, Cn, sizeof(Cn));
    return HLALA_OK;
}

}  // namespace hlala_order
#endif

// call_order_check.cpp -- the host model of the device path for the order of the pair table (hla-la_amd/csrc/call_order_model.h over call_order_core.h) against
// the specification, std::sort + std::reverse with the comparator of hlala_call_locus, as a program of its own, so that it can be built with
// -fsanitize=address,undefined and run as a child process (tests/test_call_order_model.py does both).  Every array is a heap buffer of exactly its size.  The two
// orders must be equal element for element on
//   * keys drawn from 1, 3, 50 and 100 000 distinct values, ascending, descending, organ-pipe and alternating +0 / -0 keys, at n = 1, 2, 16, 17, 18, 31, 32, 33, 100,
//     1000, every constant of the device path at -1, exact and +1, 65 536 and 1 000 003                                                    (line "families <cases>")
//   * McIlroy's adversary against the std::sort this is built with, at 1024 .. 2^20                                    (line "adversary <n>:<heap sorts>:<largest> ...")
// and the program FAILS unless the heap sort was entered in an adversary case and in an organ-pipe case, unless a range larger than the tile was partitioned by the
// closed form (counts[1] > 0), and unless a NaN key is refused with nothing written: a branch that never ran is not pinned.
//   g++ -std=c++17 -fsanitize=address,undefined -o call_order_check tools/call_order_check.cpp
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>

#include "../hla-la_amd/csrc/call_order_model.h"

namespace {

using namespace hlala_order;

unsigned long long g_s = 88172645463325252ull;
unsigned long long next() { g_s ^= g_s << 13; g_s ^= g_s >> 7; g_s ^= g_s << 17; return g_s; }

template <class T> T* exact(const std::vector<T>& v) { T* p = (T*)malloc(v.size() * sizeof(T) ? v.size() * sizeof(T) : 1); if(!v.empty()) memcpy(p, v.data(), v.size() * sizeof(T)); return p; }

// 0: equal; 1: a difference.  counts: the model's
int compare(const std::vector<double>& ll, const std::vector<double>& ma, const char* what, int64_t counts[OC_N])
{
    const int64_t n = (int64_t)ll.size();
    double *L = exact(ll), *M = exact(ma);
    std::vector<int32_t> fill((size_t)n, -7);
    int32_t *oR = exact(fill), *oM = exact(fill);
    std::string why;
    pair_order_reference(n, L, M, oR);
    const int rc = pair_order_model(n, L, M, oM, counts, &why);
    int bad = 0;
    if(rc != HLALA_OK) { fprintf(stderr, "call_order_check: %s, n = %lld: the model answers %d (%s)\n", what, (long long)n, rc, why.c_str()); bad = 1; }
    else if(memcmp(oR, oM, (size_t)n * sizeof(int32_t))) {
        int64_t j = 0; while(j < n && oR[j] == oM[j]) j++;
        fprintf(stderr, "call_order_check: %s, n = %lld: the model differs from std::sort + std::reverse (first at %lld)\n", what, (long long)n, (long long)j); bad = 1;
    }
    free(L); free(M); free(oR); free(oM);
    return bad;
}

// McIlroy's adversary ("A Killer Adversary for Quicksort") run against std::sort itself with the comparator's shape: every element is undecided until a comparison
// needs its value, and the one the sort seems to use as its pivot is given the next small value
void adversary(size_t n, std::vector<double>& ll)
{
    const double gas = (double)n;
    std::vector<double> val(n, gas); std::vector<uint32_t> idx(n); std::iota(idx.begin(), idx.end(), 0u);
    double solid = 0; uint32_t candidate = 0;
    std::sort(idx.begin(), idx.end(), [&](uint32_t x, uint32_t y) {
        if(val[x] == gas && val[y] == gas) { val[x == candidate ? x : y] = solid; solid += 1; }
        if(val[x] == gas) candidate = x; else if(val[y] == gas) candidate = y;
        return val[x] < val[y];
    });
    ll = val;
}

}  // namespace

int main()
{
    std::vector<size_t> sizes = {1, 2, 16, 17, 18, 31, 32, 33, 100, 1000, 65536, 1000003};
    for(size_t c : {(size_t)ORD_TILE, (size_t)ORD_MAX_HEAP, (size_t)ORD_BLOCK, (size_t)ORD_CHUNK, (size_t)2 * ORD_TILE + 2}) for(size_t d = 0; d < 3; d++) sizes.push_back(c - 1 + d);
    long cases = 0; int64_t counts[OC_N]; bool closed = false, organHeap = false, advHeap = false;
    for(size_t n : sizes) {
        std::vector<double> ll(n), ma(n);
        for(int distinct : {1, 3, 50, 100000}) {
            for(size_t i = 0; i < n; i++) { ll[i] = -(double)(next() % (unsigned)distinct) * 0.37; ma[i] = (double)(next() % (unsigned)(distinct < 50 ? distinct : 7)) * 0.5; }
            if(compare(ll, ma, "random keys", counts)) return 1;
            cases++; closed = closed || counts[OC_LEVELS] > 0;
        }
        for(size_t i = 0; i < n; i++) { ll[i] = (double)i; ma[i] = 1.0; }
        if(compare(ll, ma, "ascending", counts)) return 1;
        for(size_t i = 0; i < n; i++) { ll[i] = -(double)i; ma[i] = (double)(i % 2); }
        if(compare(ll, ma, "descending", counts)) return 1;
        for(size_t i = 0; i < n; i++) { ll[i] = (double)(i < n / 2 ? i : n - i); ma[i] = (double)(i % 3); }
        if(compare(ll, ma, "organ-pipe", counts)) return 1;
        organHeap = organHeap || counts[OC_HEAPS] > 0;
        for(size_t i = 0; i < n; i++) { ll[i] = (i & 1) ? -0.0 : 0.0; ma[i] = (i & 2) ? 0.0 : -0.0; }
        if(compare(ll, ma, "alternating zeros", counts)) return 1;
        cases += 4;
    }
    printf("families %ld\n", cases);
    printf("adversary");
    for(size_t n = 1024; n <= ((size_t)1 << 20); n <<= 2) {
        std::vector<double> ll, ma(n, 0.0);
        adversary(n, ll);
        if(compare(ll, ma, "adversary", counts)) { printf("\n"); return 1; }
        printf(" %zu:%lld:%lld", n, (long long)counts[OC_HEAPS], (long long)counts[OC_LARGEST_HEAP]);
        advHeap = advHeap || counts[OC_HEAPS] > 0;
    }
    printf("\n");
    if(!closed) { fprintf(stderr, "call_order_check: no range larger than the tile was partitioned by the closed form\n"); return 1; }
    if(!organHeap || !advHeap) { fprintf(stderr, "call_order_check: the heap sort was not reached (organ-pipe %d, adversary %d): the branch is not pinned\n", (int)organHeap, (int)advHeap); return 1; }
    {
        std::vector<double> ll(40, 1.0), ma(40, 2.0); ma[17] = std::nan("");
        std::vector<int32_t> fill(40, -7); int32_t* o = exact(fill); std::string why;
        const int rc = pair_order_model(40, ll.data(), ma.data(), o, counts, &why);
        bool untouched = true; for(int i = 0; i < 40; i++) untouched = untouched && o[i] == -7;
        free(o);
        if(rc != HLALA_E_CAPACITY || !untouched || why.rfind("not available:", 0) != 0) { fprintf(stderr, "call_order_check: a NaN key: model %d (%s)\n", rc, why.c_str()); return 1; }
        printf("refused NaN\n");
    }
    return 0;
}

// bam_fill_wide_check.cpp -- the order rule of the wide fill path (hla-la_amd/csrc/bam_fill_wide_core.h: fil_sort_wide) and the wide layout of the host model
// (bam_fill_model.h) as a program of its own, so that it can be built with -fsanitize=address,undefined and run as a child process (tests/test_bam_fill_wide_model.py does
// both).  First the rule against the reference's own call, std::sort ascending by score + std::reverse on the places in file order, with scores and places in heap
// buffers of exactly n elements:
//   * n = 1 .. 600 and 1000, 2048, 4095, 4096: random scores of 1 to 1000 distinct values, ascending, descending and all-equal inputs   (line "order-rule <trials>")
//   * inputs made by McIlroy's adversary against the std::sort it is built with at n = 64, 100, 256, 1000 and 4096; the program counts the entries into the heap-sort branch
//     and FAILS where an adversary input does not reach it: a restatement whose fallback never ran is not pinned             (line "adversary <n>:<heap sorts> ...")
// Then it reads cases from a file in the format of bam_fill_check.cpp and prints per case what that program prints, from the wide layout with max_mate (second
// argument, default 4096), and the three wide counts behind it.
//   g++ -std=c++17 -fsanitize=address,undefined -o bam_fill_wide_check tools/bam_fill_wide_check.cpp
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../hla-la_amd/csrc/bam_fill_model.h"

static void need(FILE* f, void* p, size_t bytes)
{
    if(bytes && fread(p, 1, bytes, f) != bytes) { fprintf(stderr, "bam_fill_wide_check: truncated case file\n"); exit(2); }
}
template <class T> static T* exact(size_t count) { return (T*)malloc(count * sizeof(T) ? count * sizeof(T) : 1); }
static unsigned long long fnv(unsigned long long h, const void* q, size_t n)
{
    const uint8_t* p = (const uint8_t*)q;
    for(size_t i = 0; i < n; i++) { h ^= p[i]; h *= 0x100000001b3ull; }
    return h;
}

// one input: fil_sort_wide against std::sort + std::reverse.  Returns the heap sorts entered, -1 on a difference
static int one(const std::vector<int32_t>& as, const char* what)
{
    using namespace hlala_bamfill;
    const uint32_t n = (uint32_t)as.size();
    std::vector<uint32_t> idx(n);
    for(uint32_t k = 0; k < n; k++) idx[k] = k;
    std::sort(idx.begin(), idx.end(), [&](uint32_t a, uint32_t b) { return as[a] < as[b]; });
    std::reverse(idx.begin(), idx.end());
    int32_t* s = exact<int32_t>(n); uint16_t* p = exact<uint16_t>(n); uint32_t* stack = exact<uint32_t>(FIL_WIDE_STACK_WORDS);
    for(uint32_t k = 0; k < n; k++) { s[k] = as[k]; p[k] = (uint16_t)k; }
    const uint32_t heaps = fil_sort_wide(s, p, n, stack);
    int rc = heaps == FIL_WIDE_OVERFLOW ? -1 : (int)heaps;
    if(rc < 0) fprintf(stderr, "bam_fill_wide_check: %s, n %u: fil_sort_wide gave up\n", what, n);
    for(uint32_t k = 0; k < n && rc >= 0; k++) if(p[k] != idx[k] || s[k] != as[idx[k]]) { fprintf(stderr, "bam_fill_wide_check: %s, n %u, place %u: %u, std::sort + std::reverse give %u\n", what, n, k, (unsigned)p[k], idx[k]); rc = -1; }
    free(s); free(p); free(stack);
    return rc;
}

static int order_rule()
{
    unsigned long long s = 88172645463325252ull; long trials = 0, heaps = 0;
    auto next = [&]() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; };
    std::vector<uint32_t> sizes;
    for(uint32_t n = 1; n <= 600; n++) sizes.push_back(n);
    for(uint32_t n : {1000u, 2048u, 4095u, 4096u}) sizes.push_back(n);
    for(uint32_t n : sizes) {
        const int rounds = n <= 600 ? 12 : 40;
        for(int t = 0; t < rounds; t++) {
            const uint32_t distinct = t == 0 ? 1u : t == 1 ? 2u : t == 2 ? 1000u : 1u + (uint32_t)(next() % 1000);
            std::vector<int32_t> as(n);
            for(uint32_t k = 0; k < n; k++) as[k] = (int32_t)(next() % distinct) - (int32_t)(distinct / 3);
            int h = one(as, "random scores"); if(h < 0) return 1; heaps += h; trials++;
            if(t >= 4) continue;
            std::sort(as.begin(), as.end());
            h = one(as, "ascending scores"); if(h < 0) return 1; heaps += h; trials++;
            std::reverse(as.begin(), as.end());
            h = one(as, "descending scores"); if(h < 0) return 1; heaps += h; trials++;
        }
    }
    printf("order-rule %ld\n", trials);
    (void)heaps;
    // the adversary: the heap-sort branch must be reached at every size
    printf("adversary");
    for(uint32_t n : {64u, 100u, 256u, 1000u, 4096u}) {
        std::vector<int32_t> as(n);
        hlala_bamfill::fil_adversary(n, as.data());
        const int h = one(as, "adversary scores");
        if(h < 0) { printf("\n"); return 1; }
        printf(" %u:%d", n, h);
        if(h == 0) { printf("\n"); fprintf(stderr, "bam_fill_wide_check: the adversary input of %u elements did not reach the heap sort: the fallback is not pinned\n", n); return 1; }
        // ... and the same scores negated: one more input with long runs, compared only
        for(int32_t& v : as) v = -v;
        if(one(as, "negated adversary scores") < 0) { printf("\n"); return 1; }
    }
    printf("\n");
    return 0;
}

int main(int argc, char** argv)
{
    using namespace hlala_bamfill;
    if(argc != 2 && argc != 3) { fprintf(stderr, "usage: bam_fill_wide_check cases.bin [max_mate]\n"); return 2; }
    const int32_t maxMate = argc == 3 ? atoi(argv[2]) : (int32_t)FIL_WIDE_MAX;
    if(order_rule()) return 1;
    FILE* f = fopen(argv[1], "rb");
    if(!f) { fprintf(stderr, "bam_fill_wide_check: cannot open %s\n", argv[1]); return 2; }
    int32_t nCases = 0; need(f, &nCases, 4);
    for(int32_t c = 0; c < nCases; c++) {
        int64_t n = 0, nU = 0, nHost = 0; uint64_t nBytes = 0; int32_t lm = 0, packed = 0;
        need(f, &n, 8); need(f, &nBytes, 8); need(f, &nU, 8); need(f, &nHost, 8); need(f, &lm, 4); need(f, &packed, 4);
        if(n < 0 || n > (1 << 24) || nBytes > (1ull << 30) || nU < 0 || nU > (1 << 24) || nHost < 0 || nHost > nU) { fprintf(stderr, "bam_fill_wide_check: bad case header\n"); return 2; }
        const int nm = fil_nm(lm); const size_t nR = (size_t)nU * (size_t)nm;
        hlala_bam_rec* recs = exact<hlala_bam_rec>((size_t)n); need(f, recs, (size_t)n * sizeof(hlala_bam_rec));
        uint8_t* bytes = exact<uint8_t>((size_t)nBytes); need(f, bytes, (size_t)nBytes);
        uint32_t* first = exact<uint32_t>((size_t)nU); need(f, first, (size_t)nU * 4);
        uint32_t* count = exact<uint32_t>((size_t)nU); need(f, count, (size_t)nU * 4);
        int64_t* hs = exact<int64_t>((size_t)nHost * (3 * nm + 1)); need(f, hs, (size_t)nHost * (3 * nm + 1) * 8);
        int64_t* ro = exact<int64_t>(nR + 1); int64_t* co = exact<int64_t>(nR + 1); int64_t* gc = exact<int64_t>(nR + 1); int64_t* no = exact<int64_t>((size_t)nU + 1);
        hlala_bam_fill_in in; memset(&in, 0, sizeof(in));
        in.recs = n ? recs : nullptr; in.n = n; in.bytes = nBytes ? bytes : nullptr; in.n_bytes = (size_t)nBytes; in.unit_first = first; in.unit_count = count; in.n_units = nU;
        in.host_sizes = nHost ? hs : nullptr; in.n_host_units = nHost; in.long_read_mode = lm; in.packed = packed;
        hlala_bam_fill_stats st; memset(&st, 0, sizeof(st)); const char* why = nullptr; FillLayout L; int64_t wide[4] = {0, 0, 0, 0};
        int rc = fill_model_create_wide(&in, maxMate, ro, co, gc, no, &L, &st, wide, &why);
        unsigned long long h = 0xcbf29ce484222325ull;
        if(rc == HLALA_OK && nU > 0) {
            h = fnv(h, ro, (nR + 1) * 8); h = fnv(h, co, (nR + 1) * 8); h = fnv(h, gc, (nR + 1) * 8); h = fnv(h, no, ((size_t)nU + 1) * 8);
            const size_t nb = (size_t)ro[nR], nc = (size_t)co[nR], ng = (size_t)gc[nR], nn = (size_t)no[nU], np = (size_t)fil_packed_at(ro[nR], (int64_t)nR);
            hlala_bam_fill_out out; memset(&out, 0, sizeof(out));
            out.read_primary = exact<int32_t>(nR); out.read_bases = packed ? nullptr : exact<uint8_t>(nb); out.read_bases_packed = packed ? exact<uint8_t>(np) : nullptr; out.read_quals = exact<uint8_t>(nb);
            out.chain_contig = exact<int32_t>(nc); out.chain_pos = exact<int32_t>(nc); out.chain_offset = exact<int32_t>(nc); out.chain_as = exact<int32_t>(nc); out.chain_reverse = exact<uint8_t>(nc);
            out.cigar_off_end = exact<int64_t>(nc); out.cigar = exact<uint32_t>(ng); out.name_chars = exact<char>(nn);
            rc = fill_model_window(&in, &L, ro, co, gc, no, 0, nU, &out, &why);
            if(rc == HLALA_OK) {
                h = fnv(h, out.read_primary, nR * 4); h = packed ? fnv(h, out.read_bases_packed, np) : fnv(h, out.read_bases, nb); h = fnv(h, out.read_quals, nb);
                h = fnv(h, out.chain_contig, nc * 4); h = fnv(h, out.chain_pos, nc * 4); h = fnv(h, out.chain_offset, nc * 4); h = fnv(h, out.chain_as, nc * 4); h = fnv(h, out.chain_reverse, nc);
                h = fnv(h, out.cigar_off_end, nc * 8); h = fnv(h, out.cigar, ng * 4); h = fnv(h, out.name_chars, nn);
            }
            free(out.read_primary); free(out.read_bases); free(out.read_bases_packed); free(out.read_quals); free(out.chain_contig); free(out.chain_pos); free(out.chain_offset); free(out.chain_as);
            free(out.chain_reverse); free(out.cigar_off_end); free(out.cigar); free(out.name_chars);
        }
        printf("%d %lld %lld %lld %lld %lld %lld %lld %llu %lld %lld %lld\n", rc, (long long)st.n_units, (long long)st.n_host_units, (long long)st.n_reads, (long long)st.n_chains, (long long)st.n_cigar,
               (long long)st.n_bases, (long long)st.n_name_bytes, h, (long long)wide[0], (long long)wide[1], (long long)wide[2]);
        free(recs); free(bytes); free(first); free(count); free(hs); free(ro); free(co); free(gc); free(no);
    }
    fclose(f);
    return 0;
}

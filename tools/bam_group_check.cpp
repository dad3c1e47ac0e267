// bam_group_check.cpp -- the grouping passes of the host model (hla-la_amd/csrc/bam_group_core.h + bam_group_model.h) as a program of its own, so that it can be built with
// -fsanitize=address,undefined and run as a child process (tests/test_bam_group_model.py does both).  It reads cases from a file -- descriptors, bytes and both outputs
// in heap buffers of exactly their sizes, which is what lets the sanitizer see a read or a write one byte outside -- and prints per case one line:
//   return code, the five counts of hlala_bam_group_stats, FNV-1a of perm and of flag
// File: int32 number of cases; per case  i64 n, u64 n_bytes, i32 long_read_mode, recs[n], bytes[n_bytes].
//   g++ -std=c++17 -fsanitize=address,undefined -o bam_group_check tools/bam_group_check.cpp
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../hla-la_amd/csrc/bam_group_model.h"

static void need(FILE* f, void* p, size_t bytes)
{
    if(bytes && fread(p, 1, bytes, f) != bytes) { fprintf(stderr, "bam_group_check: truncated case file\n"); exit(2); }
}
template <class T> static T* exact(size_t count) { return (T*)malloc(count * sizeof(T) ? count * sizeof(T) : 1); }
static unsigned long long fnv(const uint8_t* p, size_t n)
{
    unsigned long long h = 0xcbf29ce484222325ull;
    for(size_t i = 0; i < n; i++) { h ^= p[i]; h *= 0x100000001b3ull; }
    return h;
}

int main(int argc, char** argv)
{
    if(argc != 2) { fprintf(stderr, "usage: bam_group_check cases.bin\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if(!f) { fprintf(stderr, "bam_group_check: cannot open %s\n", argv[1]); return 2; }
    int32_t nCases = 0; need(f, &nCases, 4);
    for(int32_t c = 0; c < nCases; c++) {
        int64_t n = 0; uint64_t nBytes = 0; int32_t longMode = 0;
        need(f, &n, 8); need(f, &nBytes, 8); need(f, &longMode, 4);
        if(n < 0 || n > (1 << 24) || nBytes > (1ull << 30)) { fprintf(stderr, "bam_group_check: bad case header\n"); return 2; }
        hlala_bam_rec* recs = exact<hlala_bam_rec>((size_t)n); need(f, recs, (size_t)n * sizeof(hlala_bam_rec));
        uint8_t* bytes = exact<uint8_t>((size_t)nBytes); need(f, bytes, (size_t)nBytes);
        uint32_t* perm = exact<uint32_t>((size_t)n); uint8_t* flag = exact<uint8_t>((size_t)n);
        hlala_bam_group_stats st; memset(&st, 0, sizeof(st)); const char* why = nullptr;
        const int rc = hlala_bamgroup::group_model(recs, n, nBytes ? bytes : nullptr, (size_t)nBytes, longMode, perm, flag, &st, &why);
        const bool ok = rc == 0;
        printf("%d %lld %lld %lld %lld %lld %llu %llu\n", rc, (long long)st.n_recs, (long long)st.n_runs, (long long)st.n_collided_runs, (long long)st.n_units_complete, (long long)st.n_units_incomplete,
               fnv((const uint8_t*)perm, ok ? (size_t)n * 4 : 0), fnv(flag, ok ? (size_t)n : 0));
        free(recs); free(bytes); free(perm); free(flag);
    }
    fclose(f);
    return 0;
}

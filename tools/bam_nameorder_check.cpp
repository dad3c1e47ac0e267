// bam_nameorder_check.cpp -- the ordering passes of the host model (hla-la_amd/csrc/bam_nameorder_core.h + bam_nameorder_model.h) as a program of its own, so that it can be
// built with -fsanitize=address,undefined and run as a child process (tests/test_bam_nameorder_model.py does both).  It reads cases from a file -- offsets, lengths, bytes
// and the output in heap buffers of exactly their sizes, which is what lets the sanitizer see a read or a write one byte outside -- and prints per case one line:
//   return code, n, n_rounds, n_equal_names of hlala_bam_name_order_stats, FNV-1a of order
// File: int32 number of cases; per case  i64 n, u64 n_bytes, name_off[n] (u64), name_len[n] (u32), bytes[n_bytes].
//   g++ -std=c++17 -fsanitize=address,undefined -o bam_nameorder_check tools/bam_nameorder_check.cpp
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../hla-la_amd/csrc/bam_nameorder_model.h"

static void need(FILE* f, void* p, size_t bytes)
{
    if(bytes && fread(p, 1, bytes, f) != bytes) { fprintf(stderr, "bam_nameorder_check: truncated case file\n"); exit(2); }
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
    if(argc != 2) { fprintf(stderr, "usage: bam_nameorder_check cases.bin\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if(!f) { fprintf(stderr, "bam_nameorder_check: cannot open %s\n", argv[1]); return 2; }
    int32_t nCases = 0; need(f, &nCases, 4);
    for(int32_t c = 0; c < nCases; c++) {
        int64_t n = 0; uint64_t nBytes = 0;
        need(f, &n, 8); need(f, &nBytes, 8);
        if(n < 0 || n > (1 << 24) || nBytes > (1ull << 30)) { fprintf(stderr, "bam_nameorder_check: bad case header\n"); return 2; }
        uint64_t* off = exact<uint64_t>((size_t)n); need(f, off, (size_t)n * 8);
        uint32_t* len = exact<uint32_t>((size_t)n); need(f, len, (size_t)n * 4);
        uint8_t* bytes = exact<uint8_t>((size_t)nBytes); need(f, bytes, (size_t)nBytes);
        uint32_t* order = exact<uint32_t>((size_t)n);
        hlala_bam_name_order_stats st; memset(&st, 0, sizeof(st)); const char* why = nullptr;
        const int rc = hlala_nameorder::name_order_model(off, len, n, nBytes ? bytes : nullptr, (size_t)nBytes, order, &st, &why);
        printf("%d %lld %lld %lld %llu\n", rc, (long long)st.n, (long long)st.n_rounds, (long long)st.n_equal_names, fnv((const uint8_t*)order, rc == 0 ? (size_t)n * 4 : 0));
        free(off); free(len); free(bytes); free(order);
    }
    fclose(f);
    return 0;
}

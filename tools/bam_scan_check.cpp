// bam_scan_check.cpp -- the BAM record pass of the host model (hla-la_amd/csrc/bam_scan_core.h + bam_scan_model.h) as a program of its own, so that it can be built with
// -fsanitize=address,undefined and run as a child process (tests/test_bam_scan_model.py does both).  It reads cases from a file -- every input and every output in a heap
// buffer of exactly its size, which is what lets the sanitizer see a read or a write one byte outside -- and prints per case one line:
//   return code, the integer fields of hlala_bam_scan_stats, FNV-1a of the descriptors and of the compact bytes
// File: int32 number of cases; per case  u64 n, u64 first, i32 last, i32 long_read_mode, i32 n_ref, i32 n_intervals, u64 hash_mask, u64 first_seq, u32 slice_bytes,
// i32 max_rehops, ref_iv_off[n_ref + 1], ref_iv[ref_iv_off[n_ref]], iv_start / iv_stop / iv_contig [n_intervals], data[n].
//   g++ -std=c++17 -fsanitize=address,undefined -o bam_scan_check tools/bam_scan_check.cpp
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../hla-la_amd/csrc/bam_scan_model.h"

static void need(FILE* f, void* p, size_t bytes)
{
    if(bytes && fread(p, 1, bytes, f) != bytes) { fprintf(stderr, "bam_scan_check: truncated case file\n"); exit(2); }
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
    if(argc != 2) { fprintf(stderr, "usage: bam_scan_check cases.bin\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if(!f) { fprintf(stderr, "bam_scan_check: cannot open %s\n", argv[1]); return 2; }
    int32_t nCases = 0; need(f, &nCases, 4);
    for(int32_t c = 0; c < nCases; c++) {
        uint64_t n = 0, first = 0; int32_t last = 0;
        hlala_bam_scan_in in; memset(&in, 0, sizeof(in));
        need(f, &n, 8); need(f, &first, 8); need(f, &last, 4); need(f, &in.long_read_mode, 4); need(f, &in.n_ref, 4); need(f, &in.n_intervals, 4);
        need(f, &in.hash_mask, 8); need(f, &in.first_seq, 8); need(f, &in.slice_bytes, 4); need(f, &in.max_rehops, 4);
        if(in.n_ref < 0 || in.n_intervals < 0 || n > (1ull << 31)) { fprintf(stderr, "bam_scan_check: bad case header\n"); return 2; }
        int32_t* off = exact<int32_t>((size_t)in.n_ref + 1); off[0] = 0; need(f, off, ((size_t)in.n_ref + 1) * 4);
        const size_t m = in.n_ref && off[in.n_ref] > 0 ? (size_t)off[in.n_ref] : 0;
        int32_t* flat = exact<int32_t>(m); need(f, flat, m * 4);
        int32_t* col[3];
        for(int k = 0; k < 3; k++) { col[k] = exact<int32_t>((size_t)in.n_intervals); need(f, col[k], (size_t)in.n_intervals * 4); }
        uint8_t* data = exact<uint8_t>((size_t)n); need(f, data, (size_t)n);
        in.ref_iv_off = off; in.ref_iv = flat; in.iv_start = col[0]; in.iv_stop = col[1]; in.iv_contig = col[2];
        const int64_t capRecs = (int64_t)(n / 36) * (in.n_intervals > 0 ? in.n_intervals : 1);
        hlala_bam_rec* recs = exact<hlala_bam_rec>((size_t)capRecs); uint8_t* compact = exact<uint8_t>((size_t)n);
        hlala_bam_scan_stats st; const char* why = nullptr;
        const int rc = hlala_bamscan::scan_model(n ? data : nullptr, (size_t)n, (size_t)first, last, &in, recs, capRecs, compact, (size_t)n, &st, &why);
        const bool ok = rc == 0 && st.status == 0;
        printf("%d %lld %lld %lld %lld %lld %lld %d %lld %lld %lld %llu %llu\n", rc, (long long)st.n_records, (long long)st.n_kept, (long long)st.n_recs, (long long)st.examined, (long long)st.consumed,
               (long long)st.compact_bytes, (int)st.status, (long long)st.status_record, (long long)st.n_slices, (long long)st.n_rehops,
               fnv((const uint8_t*)recs, ok ? (size_t)st.n_recs * sizeof(hlala_bam_rec) : 0), fnv(compact, ok ? (size_t)st.compact_bytes : 0));
        free(off); free(flat); for(int k = 0; k < 3; k++) free(col[k]); free(data); free(recs); free(compact);
    }
    fclose(f);
    return 0;
}

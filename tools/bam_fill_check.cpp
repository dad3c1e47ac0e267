// bam_fill_check.cpp -- the layout and fill passes of the host model (hla-la_amd/csrc/bam_fill_core.h + bam_fill_model.h) as a program of its own, so that it can be built
// with -fsanitize=address,undefined and run as a child process (tests/test_bam_fill_model.py does both).  First it holds the order rule against the reference's own call:
// for every count from 1 to 16 and scores with ties, std::sort ascending by score + std::reverse on the indices in file order must give what fil_rank_serial gives (one
// line "order-rule <trials>").  Then it reads cases from a file -- descriptors, bytes, unit arrays and every output in heap buffers of exactly their sizes, which is what
// lets the sanitizer see a read or a write one byte outside -- and prints per case one line:
//   return code, the seven counts of hlala_bam_fill_stats, FNV-1a over the four offset arrays and the twelve slices of a window over all units
// File: int32 number of cases; per case  i64 n, u64 n_bytes, i64 n_units, i64 n_host_units, i32 long_read_mode, i32 packed, recs[n], bytes[n_bytes], unit_first[n_units],
// unit_count[n_units], host_sizes[n_host_units * (3 nm + 1)].
//   g++ -std=c++17 -fsanitize=address,undefined -o bam_fill_check tools/bam_fill_check.cpp
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../hla-la_amd/csrc/bam_fill_model.h"

static void need(FILE* f, void* p, size_t bytes)
{
    if(bytes && fread(p, 1, bytes, f) != bytes) { fprintf(stderr, "bam_fill_check: truncated case file\n"); exit(2); }
}
template <class T> static T* exact(size_t count) { return (T*)malloc(count * sizeof(T) ? count * sizeof(T) : 1); }
static unsigned long long fnv(unsigned long long h, const void* q, size_t n)
{
    const uint8_t* p = (const uint8_t*)q;
    for(size_t i = 0; i < n; i++) { h ^= p[i]; h *= 0x100000001b3ull; }
    return h;
}

static int order_rule()
{
    using namespace hlala_bamfill;
    unsigned long long s = 88172645463325252ull; int trials = 0;
    auto next = [&]() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; };
    for(uint32_t count = 1; count <= FIL_MAX_MATE; count++) for(int t = 0; t < 400; t++) {
        hlala_bam_rec U[2 * FIL_MAX_MATE]; memset(U, 0, sizeof(U));
        const int spread = 1 + (int)(next() % 4);                            // 1: all scores equal
        // the mate's records interleaved with the other mate's in file order
        uint32_t total = 0, mine = 0;
        while(mine < count) { const bool me = total >= FIL_MAX_MATE || (next() & 1); U[total].which = me ? 0 : 1; U[total].as = (int32_t)(next() % (unsigned)spread) - 1; if(me) mine++; total++; }
        std::vector<uint32_t> idx;
        for(uint32_t k = 0; k < total; k++) if(U[k].which == 0) idx.push_back(k);
        std::sort(idx.begin(), idx.end(), [&](uint32_t a, uint32_t b) { return U[a].as < U[b].as; });
        std::reverse(idx.begin(), idx.end());
        uint32_t order[FIL_MAX_MATE];
        const uint32_t n = fil_rank_serial(U, total, 0, order);
        if(n != count) { fprintf(stderr, "bam_fill_check: order rule: %u alignments counted as %u\n", count, n); return 1; }
        for(uint32_t k = 0; k < n; k++) if(order[k] != idx[k]) { fprintf(stderr, "bam_fill_check: order rule: count %u, place %u: %u, std::sort + std::reverse give %u\n", count, k, order[k], idx[k]); return 1; }
        trials++;
    }
    printf("order-rule %d\n", trials);
    return 0;
}

int main(int argc, char** argv)
{
    using namespace hlala_bamfill;
    if(argc != 2) { fprintf(stderr, "usage: bam_fill_check cases.bin\n"); return 2; }
    if(order_rule()) return 1;
    FILE* f = fopen(argv[1], "rb");
    if(!f) { fprintf(stderr, "bam_fill_check: cannot open %s\n", argv[1]); return 2; }
    int32_t nCases = 0; need(f, &nCases, 4);
    for(int32_t c = 0; c < nCases; c++) {
        int64_t n = 0, nU = 0, nHost = 0; uint64_t nBytes = 0; int32_t lm = 0, packed = 0;
        need(f, &n, 8); need(f, &nBytes, 8); need(f, &nU, 8); need(f, &nHost, 8); need(f, &lm, 4); need(f, &packed, 4);
        if(n < 0 || n > (1 << 24) || nBytes > (1ull << 30) || nU < 0 || nU > (1 << 24) || nHost < 0 || nHost > nU) { fprintf(stderr, "bam_fill_check: bad case header\n"); return 2; }
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
        hlala_bam_fill_stats st; memset(&st, 0, sizeof(st)); const char* why = nullptr; FillLayout L;
        int rc = fill_model_create(&in, ro, co, gc, no, &L, &st, &why);
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
        printf("%d %lld %lld %lld %lld %lld %lld %lld %llu\n", rc, (long long)st.n_units, (long long)st.n_host_units, (long long)st.n_reads, (long long)st.n_chains, (long long)st.n_cigar,
               (long long)st.n_bases, (long long)st.n_name_bytes, h);
        free(recs); free(bytes); free(first); free(count); free(hs); free(ro); free(co); free(gc); free(no);
    }
    fclose(f);
    return 0;
}

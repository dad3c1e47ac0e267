// inflate_lds_check.cpp -- the serial model of k_bgzf_inflate_lds (hla-la_amd/csrc/inflate_lds_model.h over inflate_lds_core.h: word-wise bit reader, batches, ring,
// placement, flush) as a program of its own, so that it can be built with -fsanitize=address,undefined and run as a child process (tests/test_inflate_lds_model.py does
// both).  It reads cases from a file -- the stream and the output of every case in heap buffers of exactly their sizes, which is what lets the sanitizer see an access
// one byte outside -- and prints per case one line: the status, the rounds, and the CRC-32 (8 hex digits, bit by bit: no table to get wrong) of the isize output bytes of an accepted stream.  Every case also
// runs token() and token_w() side by side along its first block (exit code 1 on a difference).
// File: int32 number of cases; per case  u32 clen, u32 isize, stream[clen].
//   g++ -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -o inflate_lds_check tools/inflate_lds_check.cpp
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../hla-la_amd/csrc/inflate_lds_model.h"

static void need(FILE* f, void* p, size_t bytes)
{
    if(bytes && fread(p, 1, bytes, f) != bytes) { fprintf(stderr, "inflate_lds_check: truncated case file\n"); exit(2); }
}

int main(int argc, char** argv)
{
    using namespace hlala_inflate;
    if(argc != 2) { fprintf(stderr, "usage: inflate_lds_check cases.bin\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if(!f) { fprintf(stderr, "inflate_lds_check: cannot open %s\n", argv[1]); return 2; }
    const int32_t cap = 4096;
    uint32_t* tok = (uint32_t*)malloc(2 * cap * sizeof(uint32_t)); int32_t* rc = (int32_t*)malloc(2 * cap * sizeof(int32_t)); uint64_t* bits = (uint64_t*)malloc(2 * cap * sizeof(uint64_t));
    int32_t nCases = 0; need(f, &nCases, 4);
    for(int32_t c = 0; c < nCases; c++) {
        uint32_t clen = 0, isize = 0; need(f, &clen, 4); need(f, &isize, 4);
        if(clen > (1u << 26) || isize > 65536u) { fprintf(stderr, "inflate_lds_check: bad case header\n"); return 2; }
        // (malloc(0) may return null: a case without bytes gets a null pointer, which nothing may touch)
        uint8_t* comp = clen ? (uint8_t*)malloc(clen) : nullptr; need(f, comp, clen);
        uint8_t* out = isize ? (uint8_t*)malloc(isize) : nullptr;
        if(isize) memset(out, 0, isize);
        int32_t rounds = 0;
        const int st = lds_model(comp, clen, out, isize, &rounds);
        uint32_t h = 0xFFFFFFFFu;
        for(uint32_t i = 0; i < isize; i++) { h ^= out[i]; for(int k = 0; k < 8; k++) h = (h >> 1) ^ (0xEDB88320u & (0u - (h & 1u))); }
        printf("%d %d %08x\n", st, (int)rounds, st == HLALA_INFLATE_OK ? ~h : 0u);
        const int n = lds_token_steps(comp, clen, cap, tok, rc, bits);
        for(int i = 0; i < n; i++)
            if(rc[2 * i] != rc[2 * i + 1] || bits[2 * i] != bits[2 * i + 1] || (rc[2 * i] == INF_TOKEN && tok[2 * i] != tok[2 * i + 1])) {
                fprintf(stderr, "inflate_lds_check: case %d: token_w differs from token at step %d\n", (int)c, i); return 1;
            }
        free(comp); free(out);
    }
    free(tok); free(rc); free(bits);
    fclose(f);
    return 0;
}

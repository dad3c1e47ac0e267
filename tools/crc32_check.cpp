// crc32_check.cpp -- the CRC-32 split of the host model (hla-la_amd/csrc/crc32_core.h: 64 segments aligned to the end of the block, six combine steps) as a program of
// its own, so that it can be built with -fsanitize=address,undefined and run as a child process (tests/test_crc32_model.py does both).  It reads cases from a file --
// every case in a heap buffer of exactly its size, which is what lets the sanitizer see a read one byte outside -- and prints per case one line: the CRC as 8 hex
// digits.  It also checks every slicing step against the byte table on each case's bytes (exit code 1 on a difference).
// File: int32 number of cases; per case  u32 n, data[n].
//   g++ -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -o crc32_check tools/crc32_check.cpp
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../hla-la_amd/csrc/crc32_core.h"

static void need(FILE* f, void* p, size_t bytes)
{
    if(bytes && fread(p, 1, bytes, f) != bytes) { fprintf(stderr, "crc32_check: truncated case file\n"); exit(2); }
}

int main(int argc, char** argv)
{
    using namespace hlala_crc32;
    if(argc != 2) { fprintf(stderr, "usage: crc32_check cases.bin\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if(!f) { fprintf(stderr, "crc32_check: cannot open %s\n", argv[1]); return 2; }
    uint32_t* T = (uint32_t*)malloc(CRC_TABLE_WORDS * sizeof(uint32_t));
    crc_build_tables(T);
    int32_t nCases = 0; need(f, &nCases, 4);
    for(int32_t c = 0; c < nCases; c++) {
        uint32_t n = 0; need(f, &n, 4);
        if(n > (1u << 26)) { fprintf(stderr, "crc32_check: bad case header\n"); return 2; }
        uint8_t* data = (uint8_t*)malloc(n ? n : 1); need(f, data, n);
        printf("%08x\n", crc_of_block_model(data, n, T));
        // the word update against four byte updates, along the case's own bytes
        uint32_t a = 0, b = 0;
        for(uint32_t i = 0; i + 4 <= n; i += 4) {
            uint32_t w; memcpy(&w, data + i, 4);       // (little-endian host)
            a = crc_update_word(a, w, T);
            for(int k = 0; k < 4; k++) b = crc_update_byte(b, data[i + k], T);
        }
        if(a != b) { fprintf(stderr, "crc32_check: case %d: slicing by four differs from the byte table\n", (int)c); return 1; }
        free(data);
    }
    free(T);
    fclose(f);
    return 0;
}

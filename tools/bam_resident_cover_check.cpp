// bam_resident_cover_check.cpp -- the accounting of units handed out (hla-la_amd/csrc/bam_resident_cover.h) as a program of its own, so that it runs under ASan and UBSan
// (tests/test_bam_resident_cover.py builds it with -fsanitize=address,undefined and runs it as a child process):
//   g++ -std=c++17 -fsanitize=address,undefined -o bam_resident_cover_check tools/bam_resident_cover_check.cpp
// Random sequences of windows -- overlapping, empty, ending at nU, asked for twice, whole chunks as the host's fill hands them out -- against a count per unit: after
// every window the chunks reported complete are exactly those whose last unit has just been handed out, every chunk is reported once, and the sum reaches the number
// of chunks exactly when every unit has been handed out.  Prints one line per sample size; exit code 1 on the first difference.
#include <cstdio>
#include <cstdlib>

#include "../hla-la_amd/csrc/bam_resident_cover.h"

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() { g_state ^= g_state << 13; g_state ^= g_state >> 7; g_state ^= g_state << 17; return g_state; }
static int64_t below(int64_t n) { return n > 0 ? (int64_t)(rnd() % (uint64_t)n) : 0; }

static int run(int64_t nU, int64_t UCH, int rounds)
{
    hlala_bamres::ResidentCover cv; cv.init(nU, UCH);
    const int64_t nChunks = (nU + UCH - 1) / UCH;
    if(cv.nChunks != nChunks) { fprintf(stderr, "nU %lld UCH %lld: %lld chunks\n", (long long)nU, (long long)UCH, (long long)cv.nChunks); return 1; }
    // every count in a heap block of exactly its size
    uint32_t* times = (uint32_t*)calloc((size_t)(nU ? nU : 1), 4); uint8_t* counted = (uint8_t*)calloc((size_t)(nChunks ? nChunks : 1), 1);
    int64_t total = 0, windows = 0;
    auto window = [&](int64_t a, int64_t z, bool chunk) -> int {
        const int64_t got = chunk ? cv.mark_chunk(a / UCH) : cv.mark(a, z);
        for(int64_t u = a < 0 ? 0 : a; u < z && u < nU; u++) times[u]++;
        int64_t want = 0;
        for(int64_t c = 0; c < nChunks; c++) {
            if(counted[c]) continue;
            bool all = true;
            for(int64_t u = c * UCH; u < (c + 1) * UCH && u < nU; u++) all = all && times[u] > 0;
            if(all) { counted[c] = 1; want++; }
        }
        windows++;
        if(got != want) { fprintf(stderr, "nU %lld UCH %lld window %lld [%lld, %lld): %lld chunks complete, expected %lld\n", (long long)nU, (long long)UCH, (long long)windows, (long long)a, (long long)z, (long long)got, (long long)want); return 1; }
        for(int64_t u = a < 0 ? 0 : a; u < z && u < nU; u++) if(!cv.unit(u)) { fprintf(stderr, "nU %lld: unit %lld not marked\n", (long long)nU, (long long)u); return 1; }
        total += got;
        return 0;
    };
    int bad = 0;
    for(int i = 0; i < rounds && !bad; i++) {
        const int kind = (int)(rnd() % 8);
        int64_t a = below(nU + 1), z;
        if(kind == 0) z = a;                                            // empty, anywhere (the end included)
        else if(kind == 1) { z = nU; }                                  // ends at nU
        else if(kind == 2) { a = below(nChunks) * UCH; z = a + UCH; bad = window(a, z < nU ? z : nU, true); continue; }        // a whole chunk, as ensure_filled hands it out
        else if(kind == 3) { a = 0; z = below(nU + 1); }                // starts at 0
        else z = a + below(nU - a + 1 < 3 * UCH ? nU - a + 1 : 3 * UCH);       // a few chunks at the most: the sample fills slowly
        bad = window(a, z, false);
        if(!bad && kind == 4) bad = window(a, z, false);                // the same window twice
        if(!bad && (total == nChunks) != [&]() { for(int64_t u = 0; u < nU; u++) if(!times[u]) return false; return true; }()) { fprintf(stderr, "nU %lld UCH %lld: %lld of %lld chunks counted\n", (long long)nU, (long long)UCH, (long long)total, (long long)nChunks); bad = 1; }
    }
    if(!bad) bad = window(0, nU, false);                                // the whole sample: whatever is left
    if(!bad && total != nChunks) { fprintf(stderr, "nU %lld UCH %lld: %lld of %lld chunks counted at the end\n", (long long)nU, (long long)UCH, (long long)total, (long long)nChunks); bad = 1; }
    if(!bad && (cv.unit(-1) || cv.unit(nU))) { fprintf(stderr, "a unit outside the sample reads as handed out\n"); bad = 1; }
    if(!bad && (cv.mark(-5, 0) || cv.mark(nU, nU + 7) || cv.mark_chunk(nChunks) || cv.mark_chunk(-1))) { fprintf(stderr, "a window outside the sample completes a chunk\n"); bad = 1; }
    if(!bad) printf("%lld units in chunks of %lld: %lld windows, %lld chunks counted once each\n", (long long)nU, (long long)UCH, (long long)windows, (long long)total);
    free(times); free(counted);
    return bad;
}

int main()
{
    const int64_t sizes[][2] = {{0, 16}, {1, 16}, {15, 16}, {16, 16}, {17, 16}, {63, 17}, {64, 64}, {65, 64}, {128, 64}, {129, 1}, {201, 16}, {400, 17}, {1000, 100}, {4099, 128}, {777, 8192}};
    for(const auto& s : sizes) for(int rep = 0; rep < 6; rep++) if(run(s[0], s[1], 40 + 20 * rep)) return 1;
    return 0;
}

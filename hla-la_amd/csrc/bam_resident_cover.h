// bam_resident_cover.h -- which units of a sample have been handed out, by the host's fill (whole chunks: ensure_filled of host_bam.cpp) or as a resident window
// (any range: seed_batch_resident), and when a chunk of UCH units counts towards the release of the decoder's working memory: once, when the last of its units has
// been handed out either way.  Windows need not fall on chunk bounds, may overlap and may be asked for twice.  Plain C++, no HIP and nothing of the decoder: the
// stand-alone program tools/bam_resident_cover_check.cpp runs it under sanitizers against a per-unit count.
#ifndef HLALA_BAM_RESIDENT_COVER_H_
#define HLALA_BAM_RESIDENT_COVER_H_
#include <cstdint>
#include <vector>

namespace hlala_bamres {

struct ResidentCover {
    int64_t nU = 0, UCH = 1, nChunks = 0;
    std::vector<uint64_t> bits;          // bit u: unit u has been handed out
    std::vector<int64_t> covered;        // per chunk: its units handed out so far
    std::vector<uint8_t> counted;        // per chunk: it has counted towards the release

    void init(int64_t n_units, int64_t chunk)
    {
        nU = n_units < 0 ? 0 : n_units; UCH = chunk < 1 ? 1 : chunk; nChunks = (nU + UCH - 1) / UCH;
        bits.assign((size_t)((nU + 63) / 64), 0); covered.assign((size_t)nChunks, 0); counted.assign((size_t)nChunks, 0);
    }
    int64_t chunk_units(int64_t c) const { const int64_t a = c * UCH, z = a + UCH < nU ? a + UCH : nU; return z - a; }
    bool unit(int64_t u) const { return u >= 0 && u < nU && ((bits[(size_t)(u >> 6)] >> (u & 63)) & 1u) != 0; }
    // the units [a, z) (clamped to the sample) are handed out; returns how many chunks have become complete by this call (each chunk once, ever)
    int64_t mark(int64_t a, int64_t z)
    {
        if(a < 0) a = 0;
        if(z > nU) z = nU;
        int64_t completed = 0;
        for(int64_t u = a; u < z;) {
            const int64_t c = u / UCH, ce = (c + 1) * UCH < z ? (c + 1) * UCH : z;       // the part of [a, z) inside chunk c
            int64_t fresh = 0;
            for(int64_t v = u; v < ce;) {
                const int64_t w = v >> 6, lo = v & 63, hi = (ce - (w << 6)) < 64 ? ce - (w << 6) : 64;       // bits [lo, hi) of word w
                const uint64_t m = (hi == 64 ? ~(uint64_t)0 : (((uint64_t)1 << hi) - 1)) & ~(((uint64_t)1 << lo) - 1);
                fresh += __builtin_popcountll(m & ~bits[(size_t)w]);
                bits[(size_t)w] |= m;
                v = (w << 6) + hi;
            }
            covered[(size_t)c] += fresh;
            if(!counted[(size_t)c] && covered[(size_t)c] == chunk_units(c)) { counted[(size_t)c] = 1; completed++; }
            u = ce;
        }
        return completed;
    }
    int64_t mark_chunk(int64_t c) { return c < 0 || c >= nChunks ? 0 : mark(c * UCH, c * UCH + UCH); }
};

}  // namespace hlala_bamres
#endif

// bam_scan_hook_model.cpp -- the two hooks of the GPU library (hla-la_amd/csrc/host_internal.h) stood in for on the CPU, so that the decoder's side of HLALA_SEEDS_GPU_PARSE runs without
// a device (tests/test_bam_scan_decoder_model.py): the header read by the host, the bytes carried from round to round, descriptors turned into records, the fall-back to the
// host's hop and parse.  The round buffer is a vector, the blocks are inflated by zlib, the record pass is the host model (bam_scan_model.h), which the device equals bit for bit.
#include <zlib.h>
#include <cstring>
#include <string>
#include <vector>
#include "../../hla-la_amd/csrc/host_internal.h"
#include "../../hla-la_amd/csrc/bam_scan_model.h"
static std::vector<uint8_t> g_round;
static int dummy_inflate(void*, const uint8_t*, size_t, const hlala_bgzf_block*, int64_t, uint8_t*, size_t, int32_t*, int (*)(void*, int64_t, int64_t), void*, std::string*) { return HLALA_E_STATE; }
static int scan_hook(void*, hlala_host::bam_scan_round* R, std::string* err)
{
    std::vector<uint8_t> next(R->carry + R->seg_bytes);
    if(R->carry > g_round.size()) { *err = "carry"; return HLALA_E_STATE; }
    memcpy(next.data(), g_round.data() + g_round.size() - R->carry, R->carry);
    for(int64_t k = 0; k < R->n_blocks; k++) {
        const hlala_bgzf_block& b = R->blocks[k];
        z_stream zs; memset(&zs, 0, sizeof(zs)); inflateInit2(&zs, -15);
        zs.next_in = (Bytef*)R->comp + b.coff; zs.avail_in = b.clen; zs.next_out = next.data() + R->carry + b.uoff; zs.avail_out = b.isize;
        int rc = inflate(&zs, Z_FINISH); inflateEnd(&zs);
        if(rc != Z_STREAM_END) { if(R->host_inflate(R->user, k, next.data() + R->carry + b.uoff)) return HLALA_E_STATE; R->n_retried++; } else R->n_gpu++;
    }
    g_round.swap(next);
    const size_t n = g_round.size();
    hlala_bam_scan_stats st; const char* why = nullptr;
    int rc = hlala_bamscan::scan_model(g_round.data(), n, R->first, R->last, R->in, nullptr, 0, nullptr, 0, &st, &why);
    if(rc == HLALA_E_CAPACITY) {
        hlala_bam_rec* recs = R->alloc_recs(R->user, st.n_recs); uint8_t* c = R->alloc_compact(R->user, st.compact_bytes);
        rc = hlala_bamscan::scan_model(g_round.data(), n, R->first, R->last, R->in, recs, st.n_recs, c, st.compact_bytes, &st, &why);
    }
    if(rc != HLALA_OK) { *err = why ? why : "model"; return rc; }
    R->stats = st; R->fell_back = false;
    if(st.status == HLALA_BAMSCAN_TOO_MANY_REHOPS) { uint8_t* fb = R->alloc_fallback(R->user, n ? n : 1); memcpy(fb, g_round.data(), n); R->fell_back = true; }
    return HLALA_OK;
}
extern "C" int dec_emul(const char* path, int32_t n, const hlala_bam_interval* iv, int32_t lm, int32_t threads, int32_t flags, hlala_seed_batch** out)
{
    // (the library's own hooks, if it has set them already, are put back: GPU tests may follow in the same process)
    const hlala_host::bam_inflate_hook_t keepInflate = hlala_host::g_bam_inflate_hook; const hlala_host::bam_scan_hook_t keepScan = hlala_host::g_bam_scan_hook;
    hlala_host::g_bam_inflate_hook = dummy_inflate; hlala_host::g_bam_scan_hook = scan_hook; g_round.clear();
    const int rc = hlala_host::bam_extract_seeds_impl(path, n, iv, lm, threads, flags, true, (void*)1, out);
    hlala_host::g_bam_inflate_hook = keepInflate; hlala_host::g_bam_scan_hook = keepScan;
    return rc;
}

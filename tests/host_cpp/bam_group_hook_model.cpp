// bam_group_hook_model.cpp -- the three hooks of the GPU library (hla-la_amd/csrc/host_internal.h) stood in for on the CPU, so that the decoder's side of HLALA_SEEDS_GPU_GROUP runs
// without a device (tests/test_bam_group_decoder_model.py): rounds kept instead of scattered, the gather through perm, units built by walking flag, collided runs handed to the
// host's re-sort, and every way back to the host's own grouping.  The scan hook is that of bam_scan_hook_model.cpp (zlib, the scan model, a vector for the round buffer) plus
// what k_grp_append does: the round's descriptors and compact bytes join sample-long vectors.  The group hook is the host model (bam_group_model.h), which the device equals
// bit for bit.  g_refuse makes the group hook answer "not available", as a failed device allocation does.
#include <zlib.h>
#include <cstring>
#include <string>
#include <vector>
#include "../../hla-la_amd/csrc/host_internal.h"
#include "../../hla-la_amd/csrc/bam_scan_model.h"
#include "../../hla-la_amd/csrc/bam_group_model.h"
static std::vector<uint8_t> g_round, g_bytes;
static std::vector<hlala_bam_rec> g_recs;
static bool g_ok = true; static int g_refuse = 0;
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
    hlala_bam_rec* recs = nullptr; uint8_t* c = nullptr;
    int rc = hlala_bamscan::scan_model(g_round.data(), n, R->first, R->last, R->in, nullptr, 0, nullptr, 0, &st, &why);
    if(rc == HLALA_E_CAPACITY) {
        recs = R->alloc_recs(R->user, st.n_recs); c = R->alloc_compact(R->user, st.compact_bytes);
        rc = hlala_bamscan::scan_model(g_round.data(), n, R->first, R->last, R->in, recs, st.n_recs, c, st.compact_bytes, &st, &why);
    }
    if(rc != HLALA_OK) { *err = why ? why : "model"; return rc; }
    R->stats = st; R->fell_back = false; R->group_appended = false;
    if(st.status == HLALA_BAMSCAN_TOO_MANY_REHOPS) { uint8_t* fb = R->alloc_fallback(R->user, n ? n : 1); memcpy(fb, g_round.data(), n); R->fell_back = true; }
    if(R->group) {
        if(R->group_first) { g_recs.clear(); g_bytes.clear(); g_ok = true; }
        if(st.status == HLALA_BAMSCAN_OK && g_ok) {
            const uint64_t base = g_bytes.size();
            if(recs) { g_bytes.insert(g_bytes.end(), c, c + st.compact_bytes); for(int64_t i = 0; i < st.n_recs; i++) { hlala_bam_rec r = recs[i]; r.rec_off += base; g_recs.push_back(r); } }
            R->group_appended = true;
        } else g_ok = false;
    }
    return HLALA_OK;
}
static int group_hook(void*, int64_t n, int32_t long_read_mode, uint32_t* perm, uint8_t* flag, hlala_bam_group_stats* stats, bool* available, std::string* err)
{
    memset(stats, 0, sizeof(*stats));
    *available = g_ok && !g_refuse && (int64_t)g_recs.size() == n;
    if(!*available || n == 0) return HLALA_OK;
    const char* why = nullptr;
    const int rc = hlala_bamgroup::group_model(g_recs.data(), n, g_bytes.data(), g_bytes.size(), long_read_mode, perm, flag, stats, &why);
    if(rc != HLALA_OK) *err = why ? why : "model";
    return rc;
}
extern "C" int grp_emul(const char* path, int32_t n, const hlala_bam_interval* iv, int32_t lm, int32_t threads, int32_t flags, int32_t refuse, hlala_seed_batch** out)
{
    // (the library's own hooks, if it has set them already, are put back: GPU tests may follow in the same process)
    const hlala_host::bam_inflate_hook_t keepInflate = hlala_host::g_bam_inflate_hook; const hlala_host::bam_scan_hook_t keepScan = hlala_host::g_bam_scan_hook;
    const hlala_host::bam_group_hook_t keepGroup = hlala_host::g_bam_group_hook;
    hlala_host::g_bam_inflate_hook = dummy_inflate; hlala_host::g_bam_scan_hook = scan_hook; hlala_host::g_bam_group_hook = group_hook; g_round.clear(); g_refuse = refuse;
    const int rc = hlala_host::bam_extract_seeds_impl(path, n, iv, lm, threads, flags, true, (void*)1, out);
    hlala_host::g_bam_inflate_hook = keepInflate; hlala_host::g_bam_scan_hook = keepScan; hlala_host::g_bam_group_hook = keepGroup;
    return rc;
}

// bam_sort_hook_model.cpp -- the four hooks of the GPU library (hla-la_amd/csrc/host_internal.h) stood in for on the CPU, so that the decoder's side of HLALA_SEEDS_GPU_SORT runs
// without a device (tests/test_bam_nameorder_decoder_model.py): the units of clean runs permuted through the device's order once it is seen to be a permutation, the units
// of collided runs merged in by the host, and every way back to the host's own sort.  The first three hooks are those of bam_group_hook_model.cpp.  The sort hook does what
// the device does behind its grouping passes: the sorted records whose flag has bits 1 and 4, in run order, their names where they lie, through the host model
// (bam_nameorder_model.h), which the device equals bit for bit.  g_sort_mode: 1 answers "not available", 2 a value twice, 3 a value beyond m.
#include "bam_group_hook_model.cpp"
#include "../../hla-la_amd/csrc/bam_nameorder_model.h"
static int g_sort_mode = 0, g_long = 0;
static int sort_hook(void*, int64_t m, uint32_t* order, hlala_bam_name_order_stats* stats, bool* available, std::string* err)
{
    memset(stats, 0, sizeof(*stats));
    *available = g_ok && g_sort_mode != 1;
    if(!*available) return HLALA_OK;
    const int64_t n = (int64_t)g_recs.size();
    std::vector<uint32_t> perm((size_t)n + 1); std::vector<uint8_t> flag((size_t)n + 1);
    hlala_bam_group_stats gs; const char* why = nullptr;
    int rc = hlala_bamgroup::group_model(g_recs.data(), n, g_bytes.data(), g_bytes.size(), g_long, perm.data(), flag.data(), &gs, &why);
    if(rc != HLALA_OK) { *err = why ? why : "group model"; return rc; }
    std::vector<uint64_t> off; std::vector<uint32_t> len;
    for(int64_t i = 0; i < n; i++) if((flag[(size_t)i] & 5) == 5) { const hlala_bam_rec& r = g_recs[perm[(size_t)i]]; off.push_back(r.rec_off + 32); len.push_back(r.nameLen); }
    if((int64_t)off.size() != m) { *err = "the host's units of clean runs are not the device's"; return HLALA_E_DEVICE; }
    if(m == 0) return HLALA_OK;
    rc = hlala_nameorder::name_order_model(off.data(), len.data(), m, g_bytes.data(), g_bytes.size(), order, stats, &why);
    if(rc != HLALA_OK) { *err = why ? why : "name order model"; return rc; }
    if(g_sort_mode == 2 && m > 1) order[m - 1] = order[0];
    if(g_sort_mode == 3) order[m / 2] = (uint32_t)m;
    return HLALA_OK;
}
extern "C" int nam_emul(const char* path, int32_t n, const hlala_bam_interval* iv, int32_t lm, int32_t threads, int32_t flags, int32_t refuse_group, int32_t sort_mode, hlala_seed_batch** out)
{
    const hlala_host::bam_sort_hook_t keepSort = hlala_host::g_bam_sort_hook;
    hlala_host::g_bam_sort_hook = sort_hook; g_sort_mode = sort_mode; g_long = lm ? 1 : 0;
    const int rc = grp_emul(path, n, iv, lm, threads, flags, refuse_group, out);
    hlala_host::g_bam_sort_hook = keepSort;
    return rc;
}

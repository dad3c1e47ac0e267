// bam_fill_wide_hook_model.cpp -- the SIXTH hook of the GPU library (hla-la_amd/csrc/host_internal.h: g_bam_fill_wide_hook) stood in for on the CPU beside the five of
// bam_fill_hook_model.cpp, so that the decoder's side of HLALA_SEEDS_GPU_FILL_WIDE runs without a device (tests/test_bam_fill_wide_decoder_model.py): which units the host
// still keeps for itself, the list of wide units it hands over, the way back to the fifth hook.  The hook does what the device does: the descriptors gathered through the
// grouping permutation, then the WIDE host model (bam_fill_model.h), which the device equals bit for bit; it checks the list it is handed against the descriptors.
// g_wide_mode: 1 answers "not available" (the decoder must then mark as without the flag and call the fifth hook), 2 installs no sixth hook at all.
#include "bam_fill_hook_model.cpp"
static int g_wide_mode = 0;
static int g_wide_calls = 0, g_narrow_calls = 0;
static int fill_hook_counting(void* inf, const hlala_bam_fill_in* in, int64_t* read_off, int64_t* chain_off, int64_t* cigar_count, int64_t* name_off, hlala_host::bam_fill_handle* handle,
                              hlala_bam_fill_stats* stats, bool* available, std::string* err)
{
    g_narrow_calls++;
    return fill_hook(inf, in, read_off, chain_off, cigar_count, name_off, handle, stats, available, err);
}
static int fill_wide_hook(void*, const hlala_bam_fill_in* in, int32_t max_mate, const uint32_t* wide_units, int64_t n_wide, int64_t longest, int64_t* read_off, int64_t* chain_off,
                          int64_t* cigar_count, int64_t* name_off, hlala_host::bam_fill_handle* handle, hlala_bam_fill_stats* stats, bool* available, std::string* err)
{
    g_wide_calls++;
    memset(stats, 0, sizeof(*stats));
    const int64_t n = (int64_t)g_recs.size();
    *available = g_ok && g_wide_mode != 1 && in->n == n && in->n_units > 0;
    if(!*available) return HLALA_OK;
    std::vector<uint32_t> perm((size_t)n + 1); std::vector<uint8_t> flag((size_t)n + 1);
    hlala_bam_group_stats gs; const char* why = nullptr;
    int rc = hlala_bamgroup::group_model(g_recs.data(), n, g_bytes.data(), g_bytes.size(), g_long, perm.data(), flag.data(), &gs, &why);
    if(rc != HLALA_OK) { *err = why ? why : "group model"; return rc; }
    FillState* F = new FillState(); g_fill_states++;
    F->recs.resize((size_t)n);
    for(int64_t i = 0; i < n; i++) F->recs[(size_t)i] = g_recs[perm[(size_t)i]];
    F->bytes = g_bytes;
    F->first.assign(in->unit_first, in->unit_first + in->n_units); F->count.assign(in->unit_count, in->unit_count + in->n_units);
    const int per = 3 * (in->long_read_mode ? 1 : 2) + 1;
    F->hostSizes.assign(in->host_sizes, in->host_sizes + in->n_host_units * per);
    F->in = *in; F->in.recs = F->recs.data(); F->in.n = n; F->in.bytes = F->bytes.data(); F->in.n_bytes = F->bytes.size(); F->in.unit_first = F->first.data(); F->in.unit_count = F->count.data();
    F->in.host_sizes = F->hostSizes.data();
    // the list the decoder hands over is the one the descriptors give
    std::vector<uint32_t> want; uint32_t wantLongest = 0;
    for(int64_t u = 0; u < in->n_units; u++) {
        if(F->first[(size_t)u] == hlala_bamfill::FIL_HOST) continue;
        uint32_t lg = 0;
        if(hlala_bamfill::fil_unit_is_wide(F->recs.data() + F->first[(size_t)u], F->count[(size_t)u], &lg)) { want.push_back((uint32_t)u); wantLongest = std::max(wantLongest, lg); }
    }
    if((int64_t)want.size() != n_wide || !std::equal(want.begin(), want.end(), wide_units) || (n_wide && longest != (int64_t)wantLongest)) { *err = "the wide units listed are not the wide units"; fill_destroy(F); return HLALA_E_ARG; }
    int64_t wide[4];
    rc = hlala_bamfill::fill_model_create_wide(&F->in, max_mate, read_off, chain_off, cigar_count, name_off, &F->L, stats, wide, &why);
    if(rc != HLALA_OK) { *err = why ? why : "fill model"; fill_destroy(F); return rc; }
    const size_t nR = (size_t)in->n_units * (in->long_read_mode ? 1 : 2);
    F->readOff.assign(read_off, read_off + nR + 1); F->chainOff.assign(chain_off, chain_off + nR + 1); F->cigCount.assign(cigar_count, cigar_count + nR + 1); F->nameOff.assign(name_off, name_off + in->n_units + 1);
    handle->state = F; handle->window = fill_window; handle->destroy = fill_destroy;
    return HLALA_OK;
}
extern "C" int filw_calls(int which) { return which ? g_wide_calls : g_narrow_calls; }
extern "C" int filw_emul(const char* path, int32_t n, const hlala_bam_interval* iv, int32_t lm, int32_t threads, int32_t flags, int32_t fill_mode, int32_t wide_mode, hlala_seed_batch** out)
{
    const hlala_host::bam_inflate_hook_t keepInflate = hlala_host::g_bam_inflate_hook; const hlala_host::bam_scan_hook_t keepScan = hlala_host::g_bam_scan_hook;
    const hlala_host::bam_group_hook_t keepGroup = hlala_host::g_bam_group_hook; const hlala_host::bam_sort_hook_t keepSort = hlala_host::g_bam_sort_hook;
    const hlala_host::bam_fill_hook_t keepFill = hlala_host::g_bam_fill_hook; const hlala_host::bam_fill_wide_hook_t keepWide = hlala_host::g_bam_fill_wide_hook;
    hlala_host::g_bam_inflate_hook = dummy_inflate; hlala_host::g_bam_scan_hook = scan_hook_keeping; hlala_host::g_bam_group_hook = group_hook; hlala_host::g_bam_sort_hook = sort_hook;
    hlala_host::g_bam_fill_hook = fill_hook_counting; hlala_host::g_bam_fill_wide_hook = wide_mode == 2 ? nullptr : fill_wide_hook;
    g_round.clear(); g_refuse = 0; g_sort_mode = 0; g_long = lm ? 1 : 0; g_fill_mode = fill_mode; g_wide_mode = wide_mode; g_wide_calls = 0; g_narrow_calls = 0;
    const int rc = hlala_host::bam_extract_seeds_impl(path, n, iv, lm, threads, flags, true, (void*)1, out);
    hlala_host::g_bam_inflate_hook = keepInflate; hlala_host::g_bam_scan_hook = keepScan; hlala_host::g_bam_group_hook = keepGroup; hlala_host::g_bam_sort_hook = keepSort;
    hlala_host::g_bam_fill_hook = keepFill; hlala_host::g_bam_fill_wide_hook = keepWide;
    return rc;
}

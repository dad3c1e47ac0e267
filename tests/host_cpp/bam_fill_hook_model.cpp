// bam_fill_hook_model.cpp -- the five hooks of the GPU library (hla-la_amd/csrc/host_internal.h) stood in for on the CPU, so that the decoder's side of HLALA_SEEDS_GPU_FILL runs
// without a device (tests/test_bam_fill_decoder_model.py): which units the host keeps for itself, their sizes, the offsets taken from the hook, the contiguous ranges asked
// for, the slices written where they belong, the host units filled behind them, and every way back to the host's own layout and fill.  The first four hooks are those of
// bam_sort_hook_model.cpp; the scan hook is wrapped so that it reports a round as kept (its descriptors and compact bytes already join the sample-long vectors there).
// The fill hook does what the device does: the descriptors gathered through the grouping permutation, then the host model (bam_fill_model.h), which the device equals
// bit for bit.  Its state owns copies of everything and needs no hook installed: it lives until the sample is filled or freed.  g_fill_mode: 1 answers "not available".
#include "bam_sort_hook_model.cpp"
#include "../../hla-la_amd/csrc/bam_fill_model.h"
static int g_fill_mode = 0;
static int g_fill_states = 0;            // states alive (the test sees that none outlives its sample)
struct FillState {
    std::vector<hlala_bam_rec> recs; std::vector<uint8_t> bytes; std::vector<uint32_t> first, count; std::vector<int64_t> hostSizes, readOff, chainOff, cigCount, nameOff;
    hlala_bam_fill_in in; hlala_bamfill::FillLayout L;
};
static int fill_window(void* state, int64_t u0, int64_t n, const hlala_bam_fill_out* out, hlala_bam_fill_stats* stats, std::string* err)
{
    FillState* F = (FillState*)state;
    memset(stats, 0, sizeof(*stats));
    const char* why = nullptr;
    const int rc = hlala_bamfill::fill_model_window(&F->in, &F->L, F->readOff.data(), F->chainOff.data(), F->cigCount.data(), F->nameOff.data(), u0, n, out, &why);
    if(rc != HLALA_OK && err) *err = why ? why : "fill model";
    return rc;
}
static void fill_destroy(void* state) { delete (FillState*)state; g_fill_states--; }
static int fill_hook(void*, const hlala_bam_fill_in* in, int64_t* read_off, int64_t* chain_off, int64_t* cigar_count, int64_t* name_off, hlala_host::bam_fill_handle* handle,
                     hlala_bam_fill_stats* stats, bool* available, std::string* err)
{
    memset(stats, 0, sizeof(*stats));
    const int64_t n = (int64_t)g_recs.size();
    *available = g_ok && g_fill_mode != 1 && in->n == n && in->n_units > 0;
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
    rc = hlala_bamfill::fill_model_create(&F->in, read_off, chain_off, cigar_count, name_off, &F->L, stats, &why);
    if(rc != HLALA_OK) { *err = why ? why : "fill model"; fill_destroy(F); return rc; }
    const size_t nR = (size_t)in->n_units * (in->long_read_mode ? 1 : 2);
    F->readOff.assign(read_off, read_off + nR + 1); F->chainOff.assign(chain_off, chain_off + nR + 1); F->cigCount.assign(cigar_count, cigar_count + nR + 1); F->nameOff.assign(name_off, name_off + in->n_units + 1);
    handle->state = F; handle->window = fill_window; handle->destroy = fill_destroy;
    return HLALA_OK;
}
static int scan_hook_keeping(void* inflater, hlala_host::bam_scan_round* R, std::string* err)
{
    const int rc = scan_hook(inflater, R, err);
    R->kept = rc == HLALA_OK && R->keep && R->group && R->group_appended;
    return rc;
}
extern "C" int fil_states() { return g_fill_states; }
extern "C" int fil_emul(const char* path, int32_t n, const hlala_bam_interval* iv, int32_t lm, int32_t threads, int32_t flags, int32_t refuse_group, int32_t sort_mode, int32_t fill_mode,
                        hlala_seed_batch** out)
{
    const hlala_host::bam_inflate_hook_t keepInflate = hlala_host::g_bam_inflate_hook; const hlala_host::bam_scan_hook_t keepScan = hlala_host::g_bam_scan_hook;
    const hlala_host::bam_group_hook_t keepGroup = hlala_host::g_bam_group_hook; const hlala_host::bam_sort_hook_t keepSort = hlala_host::g_bam_sort_hook;
    const hlala_host::bam_fill_hook_t keepFill = hlala_host::g_bam_fill_hook;
    hlala_host::g_bam_inflate_hook = dummy_inflate; hlala_host::g_bam_scan_hook = scan_hook_keeping; hlala_host::g_bam_group_hook = group_hook; hlala_host::g_bam_sort_hook = sort_hook;
    hlala_host::g_bam_fill_hook = fill_hook;
    g_round.clear(); g_refuse = refuse_group; g_sort_mode = sort_mode; g_long = lm ? 1 : 0; g_fill_mode = fill_mode;
    const int rc = hlala_host::bam_extract_seeds_impl(path, n, iv, lm, threads, flags, true, (void*)1, out);
    hlala_host::g_bam_inflate_hook = keepInflate; hlala_host::g_bam_scan_hook = keepScan; hlala_host::g_bam_group_hook = keepGroup; hlala_host::g_bam_sort_hook = keepSort;
    hlala_host::g_bam_fill_hook = keepFill;
    return rc;
}

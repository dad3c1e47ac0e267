// bam_resident_hook_model.cpp -- the `resident` function of a fill handle (hla-la_amd/csrc/host_internal.h: bam_fill_handle) stood in for on the CPU beside the six hooks of
// bam_fill_wide_hook_model.cpp, so that the decoder's side of hlala_seed_batch_create_resident (host_bam.cpp: seed_batch_resident) runs without a device
// (tests/test_bam_resident_decoder_model.py): which host units it fills and hands over, the source descriptor, the names it copies, the accounting of units handed out
// by either route, the release.  `resident` does what the device does: the window by the fill model (the ranges of host units read as zeros), the ranges of the
// window's host units placed from src->host -- of the units the STATE knows as host units, whatever the decoder filled --, then resident_model of bam_resident_model.h,
// the function hlala_host_batch_resident_model of libhlala_host.so exports.  The "batch" it hands back is the window's arrays (offsets from 0, bases unpacked, as
// SeedBatch.to_dict gives them) and the model's answer.  Every call's arguments are recorded.  g_res_mode: 1 leaves the handle without a `resident` function.
#include "bam_fill_wide_hook_model.cpp"
#include "../../hla-la_amd/csrc/bam_resident_model.h"
static int g_res_mode = 0, g_res_contigs = 0, g_res_destroyed = 0, g_res_refuse = 0;
struct ResCall { int64_t ctx, u0, n, host_null, host_units, rc; };
static std::vector<ResCall> g_res_calls;
struct ResBatch {
    std::vector<int64_t> read_off, chain_off, cigar_off; std::vector<int32_t> read_primary, chain_contig, chain_pos, chain_offset, chain_as; std::vector<uint8_t> bases, quals, chain_reverse;
    std::vector<uint32_t> cigar; std::vector<int32_t> m_read_off, m_chain_off, m_primary, m_chain_read, m_cigar_off; int64_t first[5]; int32_t rc; std::string text;
};
static void res_destroy(void* state) { g_res_destroyed++; fill_destroy(state); }
static int res_resident(void* state, hlala_ctx* ctx, int64_t u0, int64_t n, const hlala_batch_fill_src* src, hlala_batch** out, hlala_batch_fill_stats* stats, std::string* err)
{
    using namespace hlala_bamfill;
    FillState* F = (FillState*)state;
    ResCall call{(int64_t)(intptr_t)ctx, u0, n, src && !src->host, 0, 0};
    auto done = [&](int rc, const char* why) { call.rc = rc; g_res_calls.push_back(call); if(why && err) *err = why; return rc; };
    if(g_res_refuse) return done(HLALA_E_STATE, "not available: the stand-in was told to say so");
    if(!src || !src->read_off || !src->chain_off || !src->cigar_count || !out || !stats || u0 < 0 || n < 0 || u0 + n > F->in.n_units) return done(HLALA_E_ARG, "stand-in: arguments");
    if((memcmp(src->read_off, F->readOff.data(), F->readOff.size() * 8) || memcmp(src->chain_off, F->chainOff.data(), F->chainOff.size() * 8) ||
       memcmp(src->cigar_count, F->cigCount.data(), F->cigCount.size() * 8))) return done(HLALA_E_ARG, "stand-in: the offsets handed over are not the sample's");
    memset(stats, 0, sizeof(*stats));
    const int nm = fil_nm(F->in.long_read_mode);
    const size_t r0 = (size_t)u0 * nm, r1 = (size_t)(u0 + n) * nm, nr = r1 - r0;
    const int64_t* ro = F->readOff.data(); const int64_t* co = F->chainOff.data(); const int64_t* gc = F->cigCount.data();
    const int64_t b0 = ro[r0], c0 = co[r0], g0 = gc[r0], p0 = fil_packed_at(b0, (int64_t)r0);
    const size_t nb = (size_t)(ro[r1] - b0), nc = (size_t)(co[r1] - c0), ng = (size_t)(gc[r1] - g0), np = (size_t)(fil_packed_at(ro[r1], (int64_t)r1) - p0);
    ResBatch* B = new ResBatch();
    std::vector<uint8_t> raw(F->in.packed ? np + 2 : nb + 1), names((size_t)(F->nameOff[(size_t)(u0 + n)] - F->nameOff[(size_t)u0]) + 1);
    std::vector<int64_t> cigEnd(nc + 1);
    B->read_primary.assign(nr + 1, 0); B->quals.assign(nb + 1, 0); B->chain_contig.assign(nc + 1, 0); B->chain_pos.assign(nc + 1, 0); B->chain_offset.assign(nc + 1, 0); B->chain_as.assign(nc + 1, 0);
    B->chain_reverse.assign(nc + 1, 0); B->cigar.assign(ng + 1, 0);
    hlala_bam_fill_out w; memset(&w, 0, sizeof(w));
    w.read_primary = B->read_primary.data(); w.read_quals = B->quals.data(); (F->in.packed ? w.read_bases_packed : w.read_bases) = raw.data();
    w.chain_contig = B->chain_contig.data(); w.chain_pos = B->chain_pos.data(); w.chain_offset = B->chain_offset.data(); w.chain_as = B->chain_as.data(); w.chain_reverse = B->chain_reverse.data();
    w.cigar_off_end = cigEnd.data(); w.cigar = B->cigar.data(); w.name_chars = (char*)names.data();
    const char* why = nullptr;
    int rc = fill_model_window(&F->in, &F->L, ro, co, gc, F->nameOff.data(), u0, n, &w, &why);
    if(rc != HLALA_OK) { delete B; return done(rc, why ? why : "fill model"); }
    // ---- the ranges of the window's host units, from the slices handed over
    const hlala_bam_fill_out* hs = src->host;
    for(int64_t u = u0; u < u0 + n; u++) {
        if(F->first[(size_t)u] != FIL_HOST) continue;
        call.host_units++;
        if(!hs) { delete B; return done(HLALA_E_ARG, "stand-in: the window holds host units and src->host is NULL"); }
        const size_t ra = (size_t)u * nm, rb = ra + nm;
        const size_t b_ = (size_t)(ro[ra] - b0), bn = (size_t)(ro[rb] - ro[ra]), c_ = (size_t)(co[ra] - c0), cn = (size_t)(co[rb] - co[ra]), g_ = (size_t)(gc[ra] - g0), gn = (size_t)(gc[rb] - gc[ra]);
        memcpy(B->read_primary.data() + (ra - r0), hs->read_primary + (ra - r0), (size_t)nm * 4); memcpy(B->quals.data() + b_, hs->read_quals + b_, bn);
        if(!F->in.packed) memcpy(raw.data() + b_, hs->read_bases + b_, bn);
        else for(size_t r = ra; r < rb; r++) { const size_t at = (size_t)(fil_packed_at(ro[r], (int64_t)r) - p0); memcpy(raw.data() + at, hs->read_bases_packed + at, ((size_t)(ro[r + 1] - ro[r]) + 1) / 2); }
        memcpy(B->chain_contig.data() + c_, hs->chain_contig + c_, cn * 4); memcpy(B->chain_pos.data() + c_, hs->chain_pos + c_, cn * 4); memcpy(B->chain_offset.data() + c_, hs->chain_offset + c_, cn * 4);
        memcpy(B->chain_as.data() + c_, hs->chain_as + c_, cn * 4); memcpy(B->chain_reverse.data() + c_, hs->chain_reverse + c_, cn); memcpy(cigEnd.data() + c_, hs->cigar_off_end + c_, cn * 8);
        memcpy(B->cigar.data() + g_, hs->cigar + g_, gn * 4);
    }
    // ---- the window as SeedBatch.to_dict gives it: offsets from 0, bases unpacked
    static const char SEQ16[] = "=ACMGRSVTWYHKDBN";
    B->read_off.resize(nr + 1); B->chain_off.resize(nr + 1); B->cigar_off.assign(nc + 1, 0);
    for(size_t r = 0; r <= nr; r++) { B->read_off[r] = ro[r0 + r] - b0; B->chain_off[r] = co[r0 + r] - c0; }
    for(size_t r = 0; r < nr; r++) B->read_primary[r] -= (int32_t)c0;
    for(size_t k = 0; k < nc; k++) B->cigar_off[k + 1] = cigEnd[k] - g0;
    if(!F->in.packed) B->bases.assign(raw.begin(), raw.begin() + (std::ptrdiff_t)nb);
    else {
        B->bases.assign(nb, 0);
        for(size_t r = r0; r < r1; r++) {
            const size_t at = (size_t)(fil_packed_at(ro[r], (int64_t)r) - p0), a = (size_t)(ro[r] - b0), ls = (size_t)(ro[r + 1] - ro[r]);
            for(size_t i = 0; i < ls; i++) { const unsigned by = raw[at + i / 2]; B->bases[a + i] = (uint8_t)SEQ16[(i & 1) ? (by & 15) : (by >> 4)]; }
        }
    }
    B->read_primary.resize(nr); B->quals.resize(nb); B->chain_contig.resize(nc); B->chain_pos.resize(nc); B->chain_offset.resize(nc); B->chain_as.resize(nc); B->chain_reverse.resize(nc); B->cigar.resize(ng);
    // ---- what hlala_batch_create makes of it
    hlala_batch_in in; memset(&in, 0, sizeof(in));
    in.n_pairs = (int32_t)n; in.read_off = B->read_off.data(); in.read_bases = B->bases.data(); in.read_quals = B->quals.data(); in.chain_off = B->chain_off.data(); in.read_primary = B->read_primary.data();
    in.n_chains = (int32_t)nc; in.chain_contig = B->chain_contig.data(); in.chain_pos = B->chain_pos.data(); in.chain_offset = B->chain_offset.data(); in.chain_as = B->chain_as.data();
    in.chain_reverse = B->chain_reverse.data(); in.cigar_off = B->cigar_off.data(); in.cigar = B->cigar.data();
    B->m_read_off.assign(nr + 1, 0); B->m_chain_off.assign(nr + 1, 0); B->m_primary.assign(nr + 1, 0); B->m_chain_read.assign(nc + 1, 0); B->m_cigar_off.assign(nc + 1, 0);
    B->rc = hlala_bamres::resident_model(&in, g_res_contigs, nm == 1, B->m_read_off.data(), B->m_chain_off.data(), B->m_primary.data(), B->m_chain_read.data(), B->m_cigar_off.data(), B->first, &B->text);
    if(B->rc != HLALA_OK) { const int r = B->rc; if(err) *err = B->text; delete B; return done(r, nullptr); }       // (what hlala_batch_create refuses: its code and text)
    stats->n_units = n; stats->n_host_units = call.host_units; stats->n_reads = (int64_t)nr; stats->n_chains = (int64_t)nc; stats->n_cigar = (int64_t)ng; stats->n_bases = (int64_t)nb;
    stats->n_pieces = call.host_units * 10;
    *out = (hlala_batch*)B;
    return done(HLALA_OK, nullptr);
}
static int fill_hook_res(void* inf, const hlala_bam_fill_in* in, int64_t* read_off, int64_t* chain_off, int64_t* cigar_count, int64_t* name_off, hlala_host::bam_fill_handle* handle,
                         hlala_bam_fill_stats* stats, bool* available, std::string* err)
{
    const int rc = fill_hook_counting(inf, in, read_off, chain_off, cigar_count, name_off, handle, stats, available, err);
    if(rc == HLALA_OK && *available) { handle->destroy = res_destroy; if(g_res_mode != 1) handle->resident = res_resident; }
    return rc;
}
static int fill_wide_hook_res(void* inf, const hlala_bam_fill_in* in, int32_t max_mate, const uint32_t* wide_units, int64_t n_wide, int64_t longest, int64_t* read_off, int64_t* chain_off,
                              int64_t* cigar_count, int64_t* name_off, hlala_host::bam_fill_handle* handle, hlala_bam_fill_stats* stats, bool* available, std::string* err)
{
    const int rc = fill_wide_hook(inf, in, max_mate, wide_units, n_wide, longest, read_off, chain_off, cigar_count, name_off, handle, stats, available, err);
    if(rc == HLALA_OK && *available) { handle->destroy = res_destroy; if(g_res_mode != 1) handle->resident = res_resident; }
    return rc;
}
extern "C" int res_emul(const char* path, int32_t n, const hlala_bam_interval* iv, int32_t lm, int32_t threads, int32_t flags, int32_t fill_mode, int32_t res_mode, int32_t n_contigs,
                        hlala_seed_batch** out)
{
    const hlala_host::bam_inflate_hook_t keepInflate = hlala_host::g_bam_inflate_hook; const hlala_host::bam_scan_hook_t keepScan = hlala_host::g_bam_scan_hook;
    const hlala_host::bam_group_hook_t keepGroup = hlala_host::g_bam_group_hook; const hlala_host::bam_sort_hook_t keepSort = hlala_host::g_bam_sort_hook;
    const hlala_host::bam_fill_hook_t keepFill = hlala_host::g_bam_fill_hook; const hlala_host::bam_fill_wide_hook_t keepWide = hlala_host::g_bam_fill_wide_hook;
    hlala_host::g_bam_inflate_hook = dummy_inflate; hlala_host::g_bam_scan_hook = scan_hook_keeping; hlala_host::g_bam_group_hook = group_hook; hlala_host::g_bam_sort_hook = sort_hook;
    hlala_host::g_bam_fill_hook = fill_hook_res; hlala_host::g_bam_fill_wide_hook = fill_wide_hook_res;
    g_round.clear(); g_refuse = 0; g_sort_mode = 0; g_long = lm ? 1 : 0; g_fill_mode = fill_mode; g_wide_mode = 0; g_wide_calls = 0; g_narrow_calls = 0;
    g_res_mode = res_mode; g_res_contigs = n_contigs; g_res_destroyed = 0; g_res_refuse = 0; g_res_calls.clear();
    const int rc = hlala_host::bam_extract_seeds_impl(path, n, iv, lm, threads, flags, true, (void*)1, out);
    hlala_host::g_bam_inflate_hook = keepInflate; hlala_host::g_bam_scan_hook = keepScan; hlala_host::g_bam_group_hook = keepGroup; hlala_host::g_bam_sort_hook = keepSort;
    hlala_host::g_bam_fill_hook = keepFill; hlala_host::g_bam_fill_wide_hook = keepWide;
    return rc;
}
// hlala_seed_batch_create_resident as the GPU library calls the decoder; text[cap] receives the error text
extern "C" int res_create(hlala_seed_batch* S, void* ctx, int64_t u0, int64_t n, void** out, hlala_batch_fill_stats* stats, char* text, int32_t cap)
{
    std::string err; hlala_batch* b = nullptr;
    const int rc = hlala_host::seed_batch_resident(S, (hlala_ctx*)ctx, u0, u0 + n, &b, stats, &err);
    if(out) *out = b;
    if(text && cap > 0) { strncpy(text, err.c_str(), (size_t)cap - 1); text[cap - 1] = 0; }
    return rc;
}
extern "C" void res_set_refuse(int on) { g_res_refuse = on; }
extern "C" int res_destroyed() { return g_res_destroyed; }
extern "C" int res_n_calls() { return (int)g_res_calls.size(); }
extern "C" void res_call(int i, int64_t out[6]) { const ResCall& c = g_res_calls.at((size_t)i); out[0] = c.ctx; out[1] = c.u0; out[2] = c.n; out[3] = c.host_null; out[4] = c.host_units; out[5] = c.rc; }
// array `which` of a stand-in batch: 0..12 the window (read_off, read_bases, read_quals, chain_off, read_primary, chain_contig, chain_pos, chain_offset, chain_as, chain_reverse,
// cigar_off, cigar), 13..17 the model's read_off, chain_off, read_primary, chain_read, cigar_off; returns the number of elements
extern "C" int64_t res_batch_array(void* batch, int which, const void** p)
{
    ResBatch* B = (ResBatch*)batch;
#define ARR(k, v) if(which == k) { *p = B->v.data(); return (int64_t)B->v.size(); }
    ARR(0, read_off) ARR(1, bases) ARR(2, quals) ARR(3, chain_off) ARR(4, read_primary) ARR(5, chain_contig) ARR(6, chain_pos) ARR(7, chain_offset) ARR(8, chain_as) ARR(9, chain_reverse)
    ARR(10, cigar_off) ARR(11, cigar) ARR(13, m_read_off) ARR(14, m_chain_off) ARR(15, m_primary) ARR(16, m_chain_read) ARR(17, m_cigar_off)
#undef ARR
    *p = nullptr; return -1;
}
extern "C" void res_batch_free(void* batch) { delete (ResBatch*)batch; }

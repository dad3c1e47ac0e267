// host_check.cpp -- host-only view of the one-time graph flatten (no device needed), so the CPU test
// suite can check the host logic of libhlala_gpu.so against the oracle.  Built as libhlala_host.so.
#include <cstring>
#include <string>

#include "flat_graph.hpp"
#include "inflate_core.h"
#include "inflate_lds_model.h"
#include "crc32_core.h"
#include "bam_scan_model.h"
#include "bam_group_model.h"
#include "bam_nameorder_model.h"
#include "bam_fill_model.h"
#include "bam_resident_model.h"
#include "filter_gpu_model.h"
#include "call_order_model.h"

static thread_local std::string g_err;

extern "C" {
const char* hlala_host_last_error() { return g_err.c_str(); }

hlala::FlatGraph* hlala_host_flatten(const hlala_graph_desc* g, const hlala_contigs_desc* c)
{
    hlala::FlatGraph* F = new hlala::FlatGraph();
    g_err = hlala::flatten_graph(g, c, *F);
    if(!g_err.empty()) { delete F; return nullptr; }
    return F;
}
void hlala_host_free(hlala::FlatGraph* F) { delete F; }

int hlala_host_info(const hlala::FlatGraph* F, hlala_graph_info* info)
{
    memset(info, 0, sizeof(*info));
    info->n_levels = F->L; info->n_nodes = F->N; info->n_edges = F->E; info->n_paths = (int)F->path_len.size();
    info->n_jump_entries = (int64_t)F->jf_node.size(); info->n_path_edges = (int64_t)F->path_edges.size();
    info->n_levelpos_entries = (int64_t)F->lp_seqid.size();
    info->max_nodes_per_level = F->max_nodes_per_level; info->max_out_degree = F->max_out_degree; info->max_in_degree = F->max_in_degree; info->max_jumps = F->max_jumps; info->max_parallel = F->max_parallel;
    for(uint8_t b : F->gap_stretch) info->n_gap_stretch_levels += b;
    return 0;
}
int hlala_host_paths(const hlala::FlatGraph* F, int32_t* first_node, int32_t* last_node, int32_t* length)
{
    for(size_t p = 0; p < F->path_len.size(); p++) { first_node[p] = F->node_orig[F->path_first[p]]; last_node[p] = F->node_orig[F->path_last[p]]; length[p] = F->path_len[p]; }
    return 0;
}
int hlala_host_gap_stretch(const hlala::FlatGraph* F, uint8_t* out) { memcpy(out, F->gap_stretch.data(), F->gap_stretch.size()); return 0; }
// forward jump table of the node with creation index `node`: targets (creation idx) and path ids, in table order
int hlala_host_jumps(const hlala::FlatGraph* F, int node, int forward, int cap, int32_t* target, int32_t* path)
{
    int n = F->node_new[node];
    const auto& off = forward ? F->jf_off : F->jb_off; const auto& nd = forward ? F->jf_node : F->jb_node; const auto& pp = forward ? F->jf_path : F->jb_path;
    int k = 0;
    for(int i = off[n]; i < off[n + 1] && k < cap; i++, k++) { target[k] = F->node_orig[nd[i]]; path[k] = pp[i]; }
    return off[n + 1] - off[n];
}
// linear steps and their run lengths (flat_graph.hpp; kernel_dp_band.hip), [L] each
int hlala_host_linear(const hlala::FlatGraph* F, uint32_t* lin_label, int32_t* lin_eid, uint8_t* lin_out, uint8_t* lin_in)
{
    memcpy(lin_label, F->lin_label.data(), F->lin_label.size() * 4); memcpy(lin_eid, F->lin_eid.data(), F->lin_eid.size() * 4);
    memcpy(lin_out, F->lin_out.data(), F->lin_out.size()); memcpy(lin_in, F->lin_in.data(), F->lin_in.size());
    return 0;
}
// node paths of one direction (flat_graph.hpp; kernel_dp_band.hip), [N] each: label word, first edge, node and steps by position, position by node
int hlala_host_node_paths(const hlala::FlatGraph* F, int forward, uint32_t* label, int32_t* eid, int32_t* node, uint8_t* steps, int32_t* pos)
{
    const size_t n = (size_t)F->N;
    memcpy(label, (forward ? F->npf_label : F->npb_label).data(), n * 4); memcpy(eid, (forward ? F->npf_eid : F->npb_eid).data(), n * 4);
    memcpy(node, (forward ? F->npf_node : F->npb_node).data(), n * 4); memcpy(steps, (forward ? F->npf_steps : F->npb_steps).data(), n);
    memcpy(pos, (forward ? F->npf_pos : F->npb_pos).data(), n * 4);
    return 0;
}
// The DEFLATE decoder core of the device kernel (inflate_core.h) with a serial copy loop around it: raw DEFLATE bytes comp[0, clen) -> out[0, isize).
// Returns a HLALA_INFLATE_* status; never reads or writes outside the two ranges.
int hlala_host_inflate_model(const uint8_t* comp, uint32_t clen, uint8_t* out, uint32_t isize)
{
    using namespace hlala_inflate;
    static thread_local InfTables T;
    InfBits b; bits_init(b, comp, clen, 0, 0xFFFFFFFFu, 0);
    uint32_t produced = 0;
    for(;;) {
        int final = 0, type = 0; uint32_t at = 0, len = 0;
        const int rc = read_block_header(b, T, &final, &type, &at, &len);
        if(rc != HLALA_INFLATE_OK) return rc;
        if(type == 0) {
            if(len > isize - produced) return HLALA_INFLATE_OUTPUT_SIZE;
            for(uint32_t k = 0; k < len; k++) out[produced + k] = comp[at + k];
            produced += len;
            bits_init(b, comp, clen, 0, 0xFFFFFFFFu, 8ull * ((uint64_t)at + len));
        } else {
            for(;;) {
                uint32_t tok = 0;
                const int r = token(b, T, &tok);
                if(r == INF_END_OF_BLOCK) break;
                if(r != INF_TOKEN) return r;
                if(tok < 256) { if(produced >= isize) return HLALA_INFLATE_OUTPUT_SIZE; out[produced++] = (uint8_t)tok; continue; }
                const uint32_t n = tok >> 16, d = tok & 0xFFFFu;
                if(d > produced) return HLALA_INFLATE_FAR_DISTANCE;
                if(n > isize - produced) return HLALA_INFLATE_OUTPUT_SIZE;
                for(uint32_t k = 0; k < n; k++) out[produced + k] = out[produced + k - d];
                produced += n;
            }
        }
        if(final) return produced == isize ? HLALA_INFLATE_OK : HLALA_INFLATE_OUTPUT_SIZE;
    }
}
// k_bgzf_inflate_lds (kernel_inflate_lds.hip) run serially over the same core (inflate_lds_model.h): same contract as hlala_host_inflate_model; _rounds also says how
// many rounds (workgroup barriers) the kernel takes for the stream.
int hlala_host_inflate_lds_model(const uint8_t* comp, uint32_t clen, uint8_t* out, uint32_t isize) { return hlala_inflate::lds_model(comp, clen, out, isize, nullptr); }
int hlala_host_inflate_lds_rounds(const uint8_t* comp, uint32_t clen, uint8_t* out, uint32_t isize, int32_t* rounds) { return hlala_inflate::lds_model(comp, clen, out, isize, rounds); }
// the constants the vectors of tests/inflate_lds_vectors.py are built from: bytes of the ring, most bytes and most tokens of one batch
void hlala_host_inflate_lds_params(int32_t* R, int32_t* B, int32_t* batch_tokens)
{
    if(R) *R = (int32_t)hlala_inflate::LDS_RING;
    if(B) *B = (int32_t)hlala_inflate::LDS_BATCH_BYTES;
    if(batch_tokens) *batch_tokens = (int32_t)hlala_inflate::LDS_BATCH_TOKENS;
}
// token() and token_w() side by side along the first DEFLATE block of comp (inflate_lds_model.h: lds_token_steps)
int hlala_host_inflate_lds_token_steps(const uint8_t* comp, uint32_t clen, int32_t cap, uint32_t* tok, int32_t* rc, uint64_t* bits) { return hlala_inflate::lds_token_steps(comp, clen, cap, tok, rc, bits); }
// The CRC-32 split of the device kernel (kernel_crc32.hip; crc32_core.h) run serially, the 64 lanes in a loop: the CRC-32 (RFC 1952) of data[0, n).  Reads nothing else.
uint32_t hlala_host_crc32_model(const uint8_t* data, uint32_t n)
{
    struct Tables { uint32_t v[hlala_crc32::CRC_TABLE_WORDS]; };
    static const Tables tables = [] { Tables t; hlala_crc32::crc_build_tables(t.v); return t; }();
    return hlala_crc32::crc_of_block_model(data, n, tables.v);
}
// The BAM record pass of the device (kernel_bamscan.hip) run serially over the same core (bam_scan_model.h): the arguments, the return codes and every output of
// hlala_bam_scan, without a device.  hlala_host_last_error() says what HLALA_E_ARG objects to.
int hlala_host_bam_scan_model(const uint8_t* data, size_t n, size_t first, int32_t last, const hlala_bam_scan_in* in, hlala_bam_rec* recs, int64_t cap_recs, uint8_t* compact,
                              size_t cap_compact, hlala_bam_scan_stats* stats)
{
    const char* why = nullptr;
    const int rc = hlala_bamscan::scan_model(data, n, first, last, in, recs, cap_recs, compact, cap_compact, stats, &why);
    g_err = why ? std::string("hlala_host_bam_scan_model: ") + why : std::string();
    return rc;
}
// The grouping passes of the device (kernel_bamgroup.hip) run serially over the same core (bam_group_model.h): the arguments, the return codes and every output of
// hlala_bam_group but the device times, without a device.
int hlala_host_bam_group_model(const hlala_bam_rec* recs, int64_t n, const uint8_t* bytes, size_t n_bytes, int32_t long_read_mode, uint32_t* perm, uint8_t* flag, hlala_bam_group_stats* stats)
{
    const char* why = nullptr;
    const int rc = hlala_bamgroup::group_model(recs, n, bytes, n_bytes, long_read_mode, perm, flag, stats, &why);
    g_err = why ? std::string("hlala_host_bam_group_model: ") + why : std::string();
    return rc;
}
// The ordering passes of the device (kernel_bamnameorder.hip) run serially over the same core (bam_nameorder_model.h): the arguments, the return codes and every output
// of hlala_bam_name_order but the device times, without a device.
int hlala_host_bam_name_order_model(const uint64_t* name_off, const uint32_t* name_len, int64_t n, const uint8_t* bytes, size_t n_bytes, uint32_t* order, hlala_bam_name_order_stats* stats)
{
    const char* why = nullptr;
    const int rc = hlala_nameorder::name_order_model(name_off, name_len, n, bytes, n_bytes, order, stats, &why);
    g_err = why ? std::string("hlala_host_bam_name_order_model: ") + why : std::string();
    return rc;
}
// The layout and fill passes of the device (kernel_bamfill.hip) run serially over the same core (bam_fill_model.h): hlala_bam_fill_create followed by one
// hlala_bam_fill_window over units [first_unit, first_unit + n_units) (n_units < 0: no window), every output but the device times, without a device.
int hlala_host_bam_fill_model(const hlala_bam_fill_in* in, int64_t* read_off, int64_t* chain_off, int64_t* cigar_count, int64_t* name_off, int64_t first_unit, int64_t n_units,
                              const hlala_bam_fill_out* out, hlala_bam_fill_stats* stats)
{
    const char* why = nullptr;
    hlala_bamfill::FillLayout L;
    int rc = hlala_bamfill::fill_model_create(in, read_off, chain_off, cigar_count, name_off, &L, stats, &why);
    if(rc == HLALA_OK && n_units >= 0 && in->n_units > 0) rc = hlala_bamfill::fill_model_window(in, &L, read_off, chain_off, cigar_count, name_off, first_unit, n_units, out, &why);
    g_err = why ? std::string("hlala_host_bam_fill_model: ") + why : std::string();
    return rc;
}
// The same with the wide layout (bam_fill_wide_core.h): hlala_bam_fill_create_wide followed by one window.  wide[4] (may be null): what hlala_bam_fill_wide_stats
// reports, the device time 0.  For a sample without wide units every output equals hlala_host_bam_fill_model's.
int hlala_host_bam_fill_model_wide(const hlala_bam_fill_in* in, int32_t max_mate, int64_t* read_off, int64_t* chain_off, int64_t* cigar_count, int64_t* name_off, int64_t first_unit,
                                   int64_t n_units, const hlala_bam_fill_out* out, hlala_bam_fill_stats* stats, int64_t* wide)
{
    const char* why = nullptr;
    hlala_bamfill::FillLayout L;
    int rc = hlala_bamfill::fill_model_create_wide(in, max_mate, read_off, chain_off, cigar_count, name_off, &L, stats, wide, &why);
    if(rc == HLALA_OK && n_units >= 0 && in->n_units > 0) rc = hlala_bamfill::fill_model_window(in, &L, read_off, chain_off, cigar_count, name_off, first_unit, n_units, out, &why);
    g_err = why ? std::string("hlala_host_bam_fill_model_wide: ") + why : std::string();
    return rc;
}
// fil_sort_wide on scores in file order: order[rank] = place; returns the heap sorts entered, -1 for n beyond HLALA_BAM_FILL_WIDE_MAX
int hlala_host_bam_fill_wide_order(const int32_t* score, int32_t n, uint32_t* order)
{
    if(n < 0 || n > (int32_t)hlala_bamfill::FIL_WIDE_MAX || (n && (!score || !order))) return -1;
    std::vector<int32_t> s(score, score + n); std::vector<uint16_t> p((size_t)n); uint32_t stack[hlala_bamfill::FIL_WIDE_STACK_WORDS];
    for(int32_t i = 0; i < n; i++) p[(size_t)i] = (uint16_t)i;
    const uint32_t h = hlala_bamfill::fil_sort_wide(s.data(), p.data(), (uint32_t)n, stack);
    for(int32_t i = 0; i < n; i++) order[i] = p[(size_t)i];
    return h == hlala_bamfill::FIL_WIDE_OVERFLOW ? -1 : (int)h;
}
// scores that drive std::sort into its heap sort (bam_fill_model.h: fil_adversary), made against the library this was built with
int hlala_host_bam_fill_wide_adversary(int32_t n, int32_t* score)
{
    if(n < 0 || (n && !score)) return -1;
    hlala_bamfill::fil_adversary((uint32_t)n, score);
    return 0;
}
// The launches of hlala_filter_positions_gpu (kernel_filter.hip) run serially over the same core (filter_gpu_model.h): its arguments, return codes and every output,
// counts[6] included, without a device.  tie_rule 0: the rule; 1 (tests only): a stable descending sort in fil_sort_wide's place.
int hlala_host_filter_model(const hlala_exon_positions_out* pos, const hlala_filter_params* prm, uint8_t* pos_use, uint8_t* read_ignored, hlala_filter_stats* stats, int64_t* counts,
                            int32_t tie_rule)
{
    std::string why;
    int rc = HLALA_E_ARG;
    try { rc = hlala_filter::filter_model(pos, prm, pos_use, read_ignored, stats, counts, tie_rule, &why); }
    catch(const std::exception&) { why = "out of memory"; rc = HLALA_E_ARG; }
    g_err = why.empty() ? std::string() : (why.rfind("not available:", 0) == 0 ? why : "hlala_host_filter_model: " + why);
    return rc;
}
// The launches of the device path for the order of the pair table (kernel_callorder.hip) run serially over the same core (call_order_model.h): order[n] and
// counts[8] (may be null) as hlala_pair_order_gpu fills them, except that a range beyond HLALA_CALL_ORDER_MAX_HEAP met with no depth left is sorted all the same and
// counts[0] says that the device refuses it.  HLALA_E_CAPACITY ("not available:") for a NaN key, nothing written.
int hlala_host_pair_order_model(int64_t n, const double* ll, const double* ma, int32_t* order, int64_t* counts)
{
    std::string why;
    int rc = HLALA_E_ARG;
    try { rc = hlala_order::pair_order_model(n, ll, ma, order, counts, &why); }
    catch(const std::exception&) { why = "out of memory"; rc = HLALA_E_ARG; }
    g_err = why.empty() ? std::string() : (why.rfind("not available:", 0) == 0 ? why : "hlala_host_pair_order_model: " + why);
    return rc;
}
// The specification of that order for any n: std::sort + std::reverse with the comparator of hlala_call_locus, as the library this is built with runs them.
int hlala_host_pair_order_reference(int64_t n, const double* ll, const double* ma, int32_t* order)
{
    if(const char* bad = hlala_order::ord_check_args(n, ll, ma, order)) { g_err = std::string("hlala_host_pair_order_reference: ") + bad; return HLALA_E_ARG; }
    try { hlala_order::pair_order_reference(n, ll, ma, order); }
    catch(const std::exception&) { g_err = "hlala_host_pair_order_reference: out of memory"; return HLALA_E_ARG; }
    g_err.clear();
    return HLALA_OK;
}
// the constants of the device path that the tests place their sizes at: tile, heap cap, threads of a level's workgroup, elements of one step of its scans
void hlala_host_pair_order_params(int32_t* tile, int32_t* max_heap, int32_t* block, int32_t* chunk)
{
    *tile = (int32_t)hlala_order::ORD_TILE; *max_heap = (int32_t)hlala_order::ORD_MAX_HEAP; *block = (int32_t)hlala_order::ORD_BLOCK; *chunk = (int32_t)hlala_order::ORD_CHUNK;
}
// What hlala_batch_create / _unpaired does to a window before it uploads it, and so what hlala_batch_create_from_fill's kernels (kernel_bamresident.hip) must leave in
// the batch: the five 32-bit arrays, the smallest index of every violation class, the return code and (hlala_host_last_error) its text, without a device.
int hlala_host_batch_resident_model(const hlala_batch_in* in, int32_t n_contigs, int32_t unpaired, int32_t* read_off32, int32_t* chain_off32, int32_t* primary32, int32_t* chain_read,
                                    int32_t* cigar_off32, int64_t first[5])
{
    int64_t spare[hlala_bamres::RES_CLASSES];
    return hlala_bamres::resident_model(in, n_contigs, unpaired != 0, read_off32, chain_off32, primary32, chain_read, cigar_off32, first ? first : spare, &g_err);
}
}

// host_internal.h -- shared between the host-side translation units of the library (not part of the ABI)
#ifndef HLALA_HOST_INTERNAL_H_
#define HLALA_HOST_INTERNAL_H_
#include <string>
#include <utility>
#include <vector>
#include <mutex>

#include "../../include/hlala_gpu.h"

namespace hlala_host {

// one allele of one exon position as counted before the high-coverage / strand filters (hla/HLATyper.cpp:1731-1786)
struct AlleleTally {
    std::string allele;
    int count = 0, reverse = 0, from_first = 0;
    int post_filtering = -1;       // perPosition_allele_counts_postFiltering (:1821); -1 = no entry
};

// hlala_filter_positions; tallies (optional) is indexed by exon position, alleles in order of first appearance
int filter_positions_impl(const hlala_exon_positions_out* pos, const hlala_filter_params* prm, uint8_t* pos_use, uint8_t* read_ignored, hlala_filter_stats* stats,
                          std::vector<std::vector<AlleleTally>>* tallies);
// the table of Utilities::PhredToPCorrect that filter_positions_impl tests mapQ_position with (-1 for byte 0, negative for bytes below 33)
void filter_phred_table(double pc[256]);

// CPUs this process may keep busy: the hardware threads, or fewer under a CFS quota of its control group (cgroup v2 cpu.max, v1 cpu.cfs_quota_us) -- a
// container on a 256-thread host may own 16 of them, and threads beyond twice the quota only get each other throttled (measured: the decoder of an
// 8.4 M-pair sample on such a host takes 5.2 / 3.5 / 2.85 / 3.0 / 3.3-3.7 s on 8 / 16 / 32 / 64 / 128 threads)
int host_cpu_budget();

// the bulk arrays of a seed batch (host_bam.cpp) for hlala_seed_batch_pin, its pinned flag, and the hook hlala_seed_batch_free calls for a pinned batch
void seed_batch_bulk_arrays(hlala_seed_batch* S, std::vector<std::pair<void*, size_t>>& out);
void seed_batch_bulk_arrays(hlala_seed_batch* S, std::vector<std::pair<void*, size_t>>& out, int64_t unit_end, std::vector<size_t>* upto);       // ... + bytes of each that the units before unit_end occupy
bool& seed_batch_pinned_flag(hlala_seed_batch* S);
bool& seed_batch_pin_lazy(hlala_seed_batch* S);
std::mutex& seed_batch_pin_mutex(hlala_seed_batch* S);
std::vector<size_t>& seed_batch_pin_cursor(hlala_seed_batch* S);
std::vector<std::pair<void*, size_t>>& seed_batch_pin_regions(hlala_seed_batch* S);
extern void (*g_seed_batch_pin_upto)(hlala_seed_batch*, int64_t);
extern void (*g_seed_batch_unpin)(hlala_seed_batch*);

// The BAM decoder with its blocks inflated on the GPU (hlala_bam_extract_seeds_gpu).  host_bam.cpp holds no device code (it is part of libhlala_host.so as well), so
// the GPU library sets this hook: inflate blocks[0, n) of comp into out in ascending order, write their statuses, and call landed(user, first, count) for every
// chunk of blocks that has arrived (non-zero: stop).  Returns HLALA_OK or a HLALA_E_* code with its text in *err.
typedef int (*bam_inflate_hook_t)(void* inflater, const uint8_t* comp, size_t comp_bytes, const hlala_bgzf_block* blocks, int64_t n, uint8_t* out, size_t out_bytes, int32_t* status,
                                  int (*landed)(void*, int64_t, int64_t), void* user, std::string* err);
extern bam_inflate_hook_t g_bam_inflate_hook;
// ... with HLALA_SEEDS_VERIFY_CRC: the same call plus the CRC-32 every block carries; a block whose inflated bytes have another one lands with HLALA_INFLATE_CRC_MISMATCH
typedef int (*bam_inflate_crc_hook_t)(void* inflater, const uint8_t* comp, size_t comp_bytes, const hlala_bgzf_block* blocks, int64_t n, uint8_t* out, size_t out_bytes, int32_t* status,
                                      int (*landed)(void*, int64_t, int64_t), void* user, const uint32_t* crc_expect /* [n] */, std::string* err);
extern bam_inflate_crc_hook_t g_bam_inflate_crc_hook;
// The record pass of a round on the GPU (HLALA_SEEDS_GPU_PARSE): the second hook of the GPU library.  The device keeps the round's buffer [carry | this round's blocks]:
// the last `carry` bytes of the previous round's buffer move to its front (device to device), the blocks are inflated into it (a block the kernel rejects is
// inflated by host_inflate and uploaded into place), then hlala_bam_scan's passes run on it.  Descriptors and compact bytes come back through alloc_recs /
// alloc_compact.  Where the scan ends with HLALA_BAMSCAN_TOO_MANY_REHOPS the round's bytes are downloaded into alloc_fallback's buffer for the host's own hop and parse.
struct bam_scan_round {
    const uint8_t* comp; size_t comp_bytes; const hlala_bgzf_block* blocks; int64_t n_blocks;      // uoff: from the first block of the round, without gaps
    size_t seg_bytes, carry, first; int32_t last; const hlala_bam_scan_in* in;
    const uint32_t* crc_expect;                                        // [n_blocks] or null (HLALA_SEEDS_VERIFY_CRC): checked on the device; host_inflate checks what it inflates itself
    void* user;
    int (*host_inflate)(void* user, int64_t k, uint8_t* out);          // block k by the host engine into out[0, isize); non-zero: it failed, the caller holds the exception
    hlala_bam_rec* (*alloc_recs)(void* user, int64_t n);
    uint8_t* (*alloc_compact)(void* user, size_t bytes);
    uint8_t* (*alloc_fallback)(void* user, size_t bytes);              // carry + seg_bytes
    int32_t group, group_first;                                        // HLALA_SEEDS_GPU_GROUP: the round's descriptors are appended to the sample-long device arrays behind k_bam_emit (group_first: a new sample)
    int32_t keep;                                                      // HLALA_SEEDS_GPU_FILL (with group): the round's descriptors and compact bytes stay on the device as well, for the fill hook
    // results
    bool group_appended;                                               // false: they could not be (a device allocation failed, or the round fell back): the host groups the sample itself
    bool kept;                                                         // false: they were not kept (a device allocation failed, the round fell back, or a hook that knows no fill): the host fills the sample itself
    hlala_bam_scan_stats stats; int64_t n_gpu, n_retried, n_crc_recheck; bool fell_back; double s_inflate, s_scan; int64_t bytes_h2d, bytes_d2h;
};
typedef int (*bam_scan_hook_t)(void* inflater, bam_scan_round* R, std::string* err);
extern bam_scan_hook_t g_bam_scan_hook;
// The group phase on the GPU (HLALA_SEEDS_GPU_GROUP): the third hook.  After the last round: perm[n] / flag[n] of hlala_bam_group over the n descriptors the scan hook has
// appended (in the order of the rounds).  *available = false (with HLALA_OK): the device holds another count or could not allocate -- the host groups the sample itself.
typedef int (*bam_group_hook_t)(void* inflater, int64_t n, int32_t long_read_mode, uint32_t* perm, uint8_t* flag, hlala_bam_group_stats* stats, bool* available, std::string* err);
extern bam_group_hook_t g_bam_group_hook;
// The sort phase on the GPU (HLALA_SEEDS_GPU_SORT): the fourth hook.  Directly behind the group hook's passes: order[m] of hlala_bam_name_order over the m first records of
// clean, complete runs -- the host's units of clean runs, in run order.  *available = false (with HLALA_OK): the device holds no grouped sample or could not allocate
// -- the host orders the sample itself.
typedef int (*bam_sort_hook_t)(void* inflater, int64_t m, uint32_t* order, hlala_bam_name_order_stats* stats, bool* available, std::string* err);
extern bam_sort_hook_t g_bam_sort_hook;
// The layout and the fill on the GPU (HLALA_SEEDS_GPU_FILL): the fifth hook.  Behind the sort hook: a fill state over the descriptors and compact bytes the scan hook has kept
// (in->recs and in->bytes are null, in->n is the host's count of them) and the grouping permutation: in->unit_first[u] is the place of the unit's first record in the
// grouped order, HLALA_BAM_FILL_HOST for a host unit.  Writes the four offset arrays as hlala_bam_fill_create does and hands back a state of its own -- device buffers, a
// stream, page-locked staging -- that does not refer to the inflater; the seed batch owns it and calls window / destroy through the pointers in the handle, from whichever
// thread asks for a window.  *available = false (with HLALA_OK): the device does not hold the sample or could not allocate -- the host lays out and fills it itself.
// HLALA_E_ARG: the device met a unit it cannot fill (a mate beyond 16 alignments, no primary).
struct bam_fill_handle {
    void* state = nullptr;
    int (*window)(void* state, int64_t first_unit, int64_t n_units, const hlala_bam_fill_out* out, hlala_bam_fill_stats* stats, std::string* err) = nullptr;
    void (*destroy)(void* state) = nullptr;
    // the units as a batch of ctx built on the device (hlala_batch_create_from_fill on the state); HLALA_E_STATE with a text that starts "not available:" where the
    // context cannot take it (another device): the caller takes the host route.  Null: a library that knows no resident windows.
    int (*resident)(void* state, hlala_ctx* ctx, int64_t first_unit, int64_t n_units, const hlala_batch_fill_src* src, hlala_batch** out_batch, hlala_batch_fill_stats* stats, std::string* err) = nullptr;
};
// The decoder's side of hlala_seed_batch_create_resident (host_bam.cpp): the units [u0, u1) of a sample whose fill state is alive, handed to handle.resident -- the host
// units inside them filled by the host into the sample's own arrays and passed as slices, the names copied by the host from its working memory, the units accounted as
// handed out (bam_resident_cover.h).  HLALA_E_STATE with "not available: ..." in *err and nothing changed: no working memory, no live fill state, no resident function.
int seed_batch_resident(hlala_seed_batch* S, hlala_ctx* ctx, int64_t u0, int64_t u1, hlala_batch** out_batch, hlala_batch_fill_stats* stats, std::string* err);
typedef int (*bam_fill_hook_t)(void* inflater, const hlala_bam_fill_in* in, int64_t* read_off, int64_t* chain_off, int64_t* cigar_count, int64_t* name_off, bam_fill_handle* handle,
                               hlala_bam_fill_stats* stats, bool* available, std::string* err);
extern bam_fill_hook_t g_bam_fill_hook;
// The same with the wide units on the device as well (HLALA_SEEDS_GPU_FILL_WIDE): the sixth hook, called in the fifth's place.  wide_units[n_wide]: the units, ascending,
// with unit_count > 32 or a mate beyond 16 alignments (none beyond max_mate: those are host units); longest: the longest mate among them.  *available = false (with
// HLALA_OK) BEFORE anything was taken over: the decoder marks its host units as without the flag and calls the fifth hook.
typedef int (*bam_fill_wide_hook_t)(void* inflater, const hlala_bam_fill_in* in, int32_t max_mate, const uint32_t* wide_units, int64_t n_wide, int64_t longest, int64_t* read_off,
                                    int64_t* chain_off, int64_t* cigar_count, int64_t* name_off, bam_fill_handle* handle, hlala_bam_fill_stats* stats, bool* available, std::string* err);
extern bam_fill_wide_hook_t g_bam_fill_wide_hook;
// hlala_bam_extract_seeds_opt (gpu = false) and hlala_bam_extract_seeds_gpu (gpu = true: the hook above inflates with `inflater`)
int bam_extract_seeds_impl(const char* path, int32_t n_intervals, const hlala_bam_interval* iv, int32_t long_read_mode, int32_t n_threads, int32_t flags, bool gpu, void* inflater, hlala_seed_batch** out);

}  // namespace hlala_host
#endif

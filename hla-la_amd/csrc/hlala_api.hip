// hlala_api.hip -- the C ABI of include/hlala_gpu.h: device memory management, host tables, launches.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <algorithm>
#include <atomic>
#include <map>
#include <mutex>
#include <chrono>
#include <thread>
#include <set>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/hlala_gpu.h"
#include "batch.h"
#include "flat_graph.hpp"
#include "host_internal.h"

// unity build: the kernels live in their own files but are compiled in this translation unit
#include "kernel_dp.hip"
#include "kernel_project.hip"
#include "kernel_order.hip"
#include "kernel_pair.hip"
#include "kernel_pair_overflow.hip"
#include "kernel_typer.hip"
#include "kernel_call.hip"
#include "kernel_exonpos.hip"
#include "kernel_kmer.hip"
#include "kernel_dp_band.hip"
#include "kernel_inflate.hip"
#include "kernel_inflate_lds.hip"
#include "kernel_crc32.hip"
#include "kernel_bamscan.hip"
#include "kernel_bamgroup.hip"
#include "kernel_bamnameorder.hip"
#include "kernel_bamfill.hip"
#include "kernel_bamresident.hip"
#include "kernel_filter.hip"
#include "kernel_callorder.hip"

namespace hlala {
size_t proj_slab_bytes_host(int stride, int maxNodesPerLevel) { return proj_slab_bytes(stride, maxNodesPerLevel); }
}  // namespace hlala

using namespace hlala;

static thread_local std::string g_create_error;

struct DevBuf {
    void* p = nullptr; size_t bytes = 0;
};

// One DP class of the extension stage (kernel_dp.hip): launch geometry, slab pool and the instantiation of k_dp that runs it.  `launch` queues the kernel on `ws` for
// the batch `b` (its descriptor, items, seed and read bases are the kernel's plain arguments) with `pool` = the list of batches the classes from DP_POOL_TIER on walk.
struct DpClass {
    int grid = 0, block = 0;
    char* slabs = nullptr; size_t slab_bytes = 0;      // first slab of the class; bytes from one slab to the next
    const char* name = "";                             // for error messages
    void (*launch)(hlala_ctx* c, const DpClass& k, hipStream_t ws, hlala_batch* b, const DpPoolArgs& pool) = nullptr;
};

struct hlala_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    // hlala_align_batch (fused, paired batches) runs the DP classes from DP_SIDE_TIER on -- few, long DP calls that leave most of the chip idle --
    // on this second, low-priority stream, then the second stitch / pairing pass over the pairs that waited for them; the main stream goes on with the
    // pairs they do not concern and, when the caller has more than one batch in flight, with the next batch
    hipStream_t side = nullptr;
    // `up` carries the uploads of hlala_batch_create, `rs` everything that only READS a batch or works on caller data (getters, post-processing, exon
    // positions, typer scoring): neither waits for alignments of OTHER batches queued on the main stream, so a caller with two batches in flight
    // uploads the next batch and fetches the previous one while the current one is being aligned.  `active` = the stream the helpers use right now.
    hipStream_t up = nullptr, rs = nullptr, active = nullptr;
    // tail pool (round 6, hlala_set_tail_pool): fused alignments leave their broad / large / in-memory DP classes pending; flush_tail runs them ONCE for the pooled batches
    int tail_pool_k = 1; std::vector<hlala_batch*> tail;
    hipEvent_t evSideTail = nullptr; bool sideTailValid = false;      // end of the last work queued on the side stream: a non-fused launch of the classes that share its slabs waits for it
    hlala_params params{};
    FlatGraph F;
    DevGraph G{};
    DevGraph* dG = nullptr;       // device copy of G (kernels take descriptors by pointer)
    DevTables* dT = nullptr;
    double* d_islog = nullptr;
    long long* d_contig_off = nullptr; uint8_t* d_contig_seq = nullptr; int* d_contig_level = nullptr;
    int n_contigs = 0; std::vector<long long> contig_off;
    std::vector<void*> allocs;
    // Device buffers of destroyed batches are kept for the next batch (hipMalloc of the ~35 GB of column arrays of a 1 M-pair batch
    // costs 0.6-1.1 s): block sizes by pointer, free blocks by size.
    std::unordered_map<void*, size_t> block_bytes;
    std::multimap<size_t, void*> pool;
    size_t pool_bytes = 0;
    size_t pool_cap = (size_t)176 << 30;      // bytes the pool may keep parked (HLALA_POOL_CAP_GB: several processes sharing one device, e.g. the N-rank dry runs on a one-GPU box)
    std::mutex pool_mu;              // the pool and block_bytes: this context's thread, and any thread that meets an out-of-memory error on the device (device_malloc_retry)
    std::set<struct hlala_batch*> batches;     // live batches: detached (not dangling) if the context is destroyed first
    // DP scratch slabs: one per DpTiny group (4 per wave), one per DpSmall / DpLarge wave (same pool, same layout size)
    int dp_long_bases = 48;  // read bases left from which a DP call is long: drawn first from its list, so that the persistent DP kernels do not end on it (batch.h: dpl_list, retry_entry); HLALA_DP_LONG_BASES, 0: list order as without
                             // (resident step at 0 / 16 / 32 / 48: 183.46 / 181.03 / 180.39 / 179.95 ms, profiles/dp_long_first.txt)
    int jf_margin = 16;      // (measured 4 / 8 / 16 / 48: 16-lane + 32-lane class 105.6 / 104.1 / 103.4 / 104.1 ms -- a tight bound sends more calls to the cheap instantiation and more of them on to the 32-lane class) levels beyond the read bases left that a jump-free call is taken to reach (kernel_dp.hip: k_dp_items)
    int stitch_by_row = 1;     // k_stitch_chains draws column rows (position order, only chains that hold one) instead of chain numbers (HLALA_STITCH_BY_ROW=0; 6.9 -> 6.65 ms)
    int stitch_draw = 12;      // chains per draw of k_stitch_chains (8: 9.1 ms per million pairs, the rate of the draws themselves; 12 / 16: 6.7 / 6.6 ms; 64: 15 ms -- kernel_dp.hip)
    bool side_after_pair = false; // HLALA_SIDE_AFTER_PAIR=1: the side-stream classes are queued behind the main stream's stitch and pairing passes instead of beside them (measured: the pairing pass 20.9 -> 4.1 ms, but the next batch's projection 35.5 -> 54.8 ms beside the wide class instead; step 183.4 -> 185.5 ms)
    bool rows_all = false;        // HLALA_ROWS_ALL=1: column rows for every chain of a batch, the filters run with the projection (rounds 1-4)
    bool band_risky = false;      // HLALA_DP_BAND_RISKY=1 (tests: force fail-overs of the band kernel)
    bool band_nodes = true;       // HLALA_DP_BAND_NODES=0: a call is listed for the band kernel by the linear run of its start LEVEL, not by the path of its start node (A/B and parity)
    int band_grid = 0, band_margin = 8;      // the band kernel in front of the 16-lane class (kernel_dp_band.hip): blocks (0: HLALA_DP_BAND=0) and the levels beyond the read bases left a call is taken to reach (HLALA_DP_BAND_MARGIN)
    // The DP classes by tier (0 DpTiny, 1 DpMid, 2 DpSmall, 3 DpWide, 4 DpBroad, 5 DpLarge, 6 DpHuge), filled once by hlala_create; dp_jf = the jump-free instantiation of
    // the 16-lane class, launched in front of tier 0 on tier 0's slabs.  INVARIANT: the slabs of the tiers >= DP_SIDE_TIER belong to the context, not to a batch, and are
    // used by ONE stream at a time: by the side stream for fused alignments, each forked from the main stream (side_fork) or queued behind the last one (flush_tail); by
    // the main stream for a non-fused extension stage, which first flushes the tail pool and then waits for evSideTail, the end of everything queued on the side stream.
    DpClass dp[DP_LAST_TIER + 1]; DpClass dp_jf;
    int stitch_grid = 0;
    char* proj_slabs = nullptr; size_t proj_slab_bytes = 0; int proj_grid = 0, pair_grid = 0, pair_lean_grid = 0;
    char* rethread_slabs = nullptr; size_t rethread_slab_bytes = 0; int rethread_grid = 0;      // k_rethread_chains: back pointers of one chain per wave (short reads; HLALA_RETHREAD=0 turns the kernel off)
    double* pair_scratch = nullptr;   // [2 * pair_grid][PAIR_COMB]: combination tables of the rare pairs with more than PAIR_COMB_LDS combinations (main- and side-stream pass)
    // the overflow class of the pairing stage (hlala_set_pair_overflow; kernel_pair_overflow.hip): [2 passes][PAIR_OVER_WAVES] slabs of pair_over_slab_bytes; null: off
    char* pair_over_slabs = nullptr; long long pair_over_scratch = 0, pair_over_slab_bytes = 0;
    char* proj_long_slabs = nullptr; size_t proj_long_slab_bytes = 0;      // long reads only (max_columns > 512): column / window arrays of k_project_chains<ProjLdsLong>
    void* create_scratch = nullptr; size_t create_scratch_bytes = 0; bool create_scratch_pinned = false;      // host scratch of hlala_batch_create (page-locked when the runtime grants it; one caller thread per context)
    int long_chunk_nodes = 1 << 20, long_max_segs = 1 << 20;      // (batch.h; the kernel clamps them to its array sizes)
    int order_cost = 0;                     // long-read layout: heaviest windows first (batch.h: order_cost; HLALA_LONG_ORDER=0: position order)
    int order_shift = 8, order_nb = 0;      // position buckets of a batch's chains (kernel_order.hip); order_nb 0: input order (HLALA_LOCALITY=0)
    int* dbg_host = nullptr;      // (device memory) non-null with HLALA_DEBUG=1: kernels accumulate phase clocks into the batch counters (hlala_debug_counters)
    // per-pair post-processing: coverage counters [L-1] and gene intervals
    int* d_cov = nullptr; int n_cov = 0; int* d_gene_first = nullptr; int* d_gene_last = nullptr; int n_genes = 0;
    // reads kept for the k-mer questions (hlala_kmer_keep_reads): one chunk per call, blocks of the pool
    struct KeptReads { uint8_t* store = nullptr; long long* start = nullptr; int* length = nullptr; int n = 0; };
    std::vector<KeptReads> kept;
    bool flt_timed = false; double flt_ms[6] = {0, 0, 0, 0, 0, 0};      // hlala_filter_gpu_times: the launches of the last hlala_filter_positions_gpu, timed only on request
    // the order of the pair table on the device (hlala_set_call_order_gpu; kernel_callorder.hip): the switch, the counters of the last order, its phases when timed
    bool ord_gpu = false, ord_timed = false; int64_t ord_counts[HLALA_CALL_ORDER_COUNTS] = {0, 0, 0, 0, 0, 0, 0, 0}; double ord_ms[4] = {0, 0, 0, 0};
    std::string err;
};

// The events of a batch.  All but the last two time the batch's stages (hlala_batch_get_stats) and are recorded on the stream their work runs on.
enum BatchEvent {
    EV_PROJECT_BEGIN, EV_PROJECT_END, EV_EXTEND_BEGIN, EV_EXTEND_END, EV_PAIR_BEGIN, EV_PAIR_END,      // the three stages, on the main stream
    EV_DP_BAND_BEGIN, EV_DP_BAND_END,      // the band kernels
    EV_DP_BEGIN, EV_DP_CLASS0_END, EV_DP_CLASS2_END, EV_DP_END,      // main stream: in front of the 16-lane class, behind it, behind the 64-lane class, behind the last class of a non-fused extension
    EV_DP_JUMP_FREE_END,                   // between the jump-free instantiation of the 16-lane class and the general one
    EV_DP_CLASS_BEGIN,                                       // + tier: start of a DP class, on the stream it ran on
    EV_DP_CLASS_END = EV_DP_CLASS_BEGIN + DP_LAST_TIER + 1,  // + tier: its end
    EV_SIDE_FORK = EV_DP_CLASS_END + DP_LAST_TIER + 1,       // main stream: the point the side stream's work of this batch waits for
    EV_SIDE_BEGIN, EV_SIDE_END,            // side stream: in front of its first class, behind the second pairing pass
    EV_TIMED_N, EV_MAIN = EV_TIMED_N,                  // end of the last work of this batch on the main stream (readers on `rs` wait for it; valid while mainValid)
    EV_DONE,                               // end of its last work on the side stream (side_mark; whoever touches the batch while side_inflight waits for it)
    EV_N
};

struct hlala_batch {
    hlala_ctx* ctx = nullptr;
    DevBatch B{};
    DevBatch* dB = nullptr;       // device copy of B
    std::vector<void*> allocs;
    int staged = 0;   // bit0 seeds available, bit1 extended, bit2 paired
    bool prepared = false;           // the filters and the position order ran when the batch was created; B.n_rows = chains that hold column rows (batch.h: chain_row)
    int n_rows_host = 0;             // ... read back with the upload's synchronisation
    bool outputs_ready = false;      // the output arrays (50 GB for a 1 M-pair batch) exist: allocated by the first stage call, not by hlala_batch_create (ensure_outputs)
    // The four side flags.  Every extension stage starts from side_used = side_pending = false (dp_prepare); only a fused alignment (hlala_align_batch) sets any.
    //   side_used     the last extension ran classes on the side stream (side_fork): their times lie between EV_SIDE_BEGIN and EV_SIDE_END.  Kept until the next extension.
    //   side_pending  the first stitch pass left the deferred pairs out and their second pairing pass is not queued yet: set in front of stitch_main, cleared by pair_side.
    //                 Between calls it is true only together with tail_pooled (or after an alignment that failed half way: the pairing stage then pairs every pair itself).
    //   tail_pooled   the batch is in c->tail: its classes from DP_POOL_TIER on, its second stitch and pairing pass wait for flush_tail.  Cleared by flush_tail, which
    //                 everything that reads, re-runs or destroys the batch calls first (join_side, ReaderScope, hlala_batch_destroy).
    //   side_inflight side_mark recorded EV_DONE behind work of this batch on the side stream and nothing has waited for it since: set by side_mark, cleared by join_side
    //                 (the main stream then waits; readers and hlala_batch_destroy wait for EV_DONE themselves).  A pooled batch is in flight too: its wide class.
    bool side_used = false, side_pending = false, tail_pooled = false, side_inflight = false;
    hipEvent_t ev[EV_N]{}; bool eventsMade = false;      // (created with the batch's first stage call: batch_events)
    bool mainValid = false /* EV_MAIN has been recorded */, band_used = false;
    uint32_t first_chain = 0;    // absolute index of the batch's chain 0 in the caller's numbering (hlala_batch_set_first_chain): offsets the random seeds
    float ms[3] = {0, 0, 0};
};

// Every entry point runs with the context's device current and restores the caller's device on return: several contexts (one per GPU)
// may live in one process, and the host program (or torch) may switch devices between calls.
struct DevGuard {
    int prev = -1, want = -1;
    explicit DevGuard(int device) : want(device) { if(device >= 0 && hipGetDevice(&prev) == hipSuccess && prev != device) (void)hipSetDevice(device); else prev = -1; }
    ~DevGuard() { if(prev >= 0 && prev != want) (void)hipSetDevice(prev); }
    DevGuard(const DevGuard&) = delete; DevGuard& operator=(const DevGuard&) = delete;
};
#define DEV_GUARD(c) DevGuard dev_guard_((c) ? (c)->device : -1)

#define HIP_TRY(ctx, call) do { hipError_t e_ = (call); if(e_ != hipSuccess) { (ctx)->err = std::string(#call) + ": " + hipGetErrorString(e_); return HLALA_E_DEVICE; } } while(0)
// the same inside a function that owns temporaries or a half-built object: `cleanup` (a lambda int -> int) releases them and passes the code through
#define HIP_TRY_F(ctx, call, cleanup) do { hipError_t e_ = (call); if(e_ != hipSuccess) { (ctx)->err = std::string(#call) + ": " + hipGetErrorString(e_); return cleanup(HLALA_E_DEVICE); } } while(0)

template<class C, int TIER> static void launch_dp(hlala_ctx* c, const DpClass& k, hipStream_t ws, hlala_batch* b, const DpPoolArgs& pool)
{
    hipLaunchKernelGGL((k_dp<C, TIER>), dim3(k.grid), dim3(k.block), 0, ws, c->dG, b->dB, (DpItem*)b->B.dp_items, k.slabs, k.slab_bytes, c->params.rng_seed + 2u * b->first_chain,
                       c->G.nrec_out, c->G.nrec_in, b->B.read_bases, pool);
}
template<class C, int TIER> static DpClass dp_class(int grid, size_t slab_bytes, const char* name) { return DpClass{grid, C::THREADS, nullptr, slab_bytes, name, launch_dp<C, TIER>}; }      // (hlala_create allocates the slabs)

// everything on the main stream that reads or rewrites a batch goes behind the side-stream work of its last fused alignment
static int flush_tail(hlala_ctx* c);
static int join_side(hlala_ctx* c, hlala_batch* b)
{
    if(b->tail_pooled) { int rf = flush_tail(c); if(rf) return rf; }
    if(b->side_inflight) {
        HIP_TRY(c, hipStreamWaitEvent(c->stream, b->ev[EV_DONE], 0));
        // EV_MAIN is what hlala_batch_destroy and the readers wait for once side_inflight is cleared: it has to lie BEHIND the wait just queued even if the
        // stage call that joined returns early (state / launch error) and never reaches its own mark_main
        if(b->ev[EV_MAIN]) { HIP_TRY(c, hipEventRecord(b->ev[EV_MAIN], c->stream)); b->mainValid = true; b->side_inflight = false; }
    }
    return HLALA_OK;
}
static int batch_events(hlala_ctx* c, hlala_batch* b)
{
    if(b->eventsMade) return HLALA_OK;
    for(int i = 0; i < EV_N; i++) HIP_TRY(c, hipEventCreateWithFlags(&b->ev[i], i < EV_TIMED_N ? hipEventDefault : hipEventDisableTiming));
    b->eventsMade = true;
    return HLALA_OK;
}
// end of a stage call: what readers of the batch on the reader stream wait for
static int mark_main(hlala_ctx* c, hlala_batch* b) { HIP_TRY(c, hipEventRecord(b->ev[EV_MAIN], c->stream)); b->mainValid = true; return HLALA_OK; }
// A call that only reads a batch (or works on caller data) runs on the context's reader stream, behind the batch's own work on the main and the side
// stream -- not behind whatever the caller queued for other batches since.  (Calls on one context are serialised by the caller: `active` is plain state.)
struct ReaderScope {
    hlala_ctx* c; int rc = HLALA_OK;
    ReaderScope(hlala_ctx* c_, hlala_batch* b) : c(c_)
    {
        if(!c) return;
        if(b && b->tail_pooled) { rc = flush_tail(c); if(rc) return; }          // the batch's tail classes are still pooled: run them now (with whatever the pool holds)
        c->active = c->rs;
        hipError_t e = hipSuccess;
        if(b && b->mainValid) e = hipStreamWaitEvent(c->rs, b->ev[EV_MAIN], 0);
        if(e == hipSuccess && b && b->side_inflight) e = hipStreamWaitEvent(c->rs, b->ev[EV_DONE], 0);
        if(e != hipSuccess) { c->err = std::string("hipStreamWaitEvent: ") + hipGetErrorString(e); rc = HLALA_E_DEVICE; }
    }
    ~ReaderScope() { if(c) c->active = c->stream; }
    ReaderScope(const ReaderScope&) = delete; ReaderScope& operator=(const ReaderScope&) = delete;
};
struct UploadScope {
    hlala_ctx* c;
    explicit UploadScope(hlala_ctx* c_) : c(c_) { if(c) c->active = c->up; }
    ~UploadScope() { if(c) c->active = c->stream; }
    UploadScope(const UploadScope&) = delete; UploadScope& operator=(const UploadScope&) = delete;
};

// hipMalloc, or a block of a destroyed batch that is large enough and wastes at most a quarter
// Sizes are rounded up to classes a sixteenth of a power of two apart (at most 6 % more than asked for): the arrays of consecutive batches differ by a fraction of a
// per cent in size, and with exact sizes a batch kept finding the blocks of the batch before it a little too small for some of its arrays -- a few hipMalloc and
// hipFree of gigabyte blocks in every step, 8-16 ms per hlala_align_batch in the first process on a freshly booted device (0.4 ms once the driver has handed the
// memory out before), which is the step the next batch's kernels are launched from.
static size_t pool_class(size_t bytes)
{
    bytes = (bytes + 255) & ~(size_t)255;
    if(bytes <= 4096) return bytes;
    const int lg = 63 - __builtin_clzll((unsigned long long)bytes);
    const size_t g = (size_t)1 << (lg - 4);
    return (bytes + g - 1) & ~(g - 1);
}
// Every live context is registered: a context parks up to 176 GB of a 288 GB device, and an allocation of ANOTHER context on the same device (a second hlala_create,
// its slabs, its batches) must be able to get that memory back.  A context's pool is touched by its own thread (pool_malloc / pool_release) and, on an out-of-memory
// error anywhere on the device, by the thread that met the error: pool_mu orders the two.
static std::mutex g_ctx_mu;
static std::vector<hlala_ctx*> g_ctxs;
static void pool_trim_locked(hlala_ctx* c)
{
    for(auto& kv : c->pool) { c->block_bytes.erase(kv.second); (void)hipFree(kv.second); }
    c->pool.clear(); c->pool_bytes = 0;
}
// hipMalloc; on failure the blocks parked by every context of this device are released and the call is tried once more (`self`: the caller's context when it
// already holds its own pool_mu, else null)
static hipError_t device_malloc_retry(int device, hlala_ctx* self, void** p, size_t bytes)
{
    hipError_t e = hipMalloc(p, bytes);
    if(e == hipSuccess) return e;
    (void)hipGetLastError();
    bool freed = false;
    {
        std::lock_guard<std::mutex> g(g_ctx_mu);
        for(hlala_ctx* o : g_ctxs) {
            if(o->device != device) continue;
            if(o == self) { if(!o->pool.empty()) { pool_trim_locked(o); freed = true; } continue; }
            std::lock_guard<std::mutex> g2(o->pool_mu);
            if(!o->pool.empty()) { pool_trim_locked(o); freed = true; }
        }
    }
    if(!freed) return e;
    return hipMalloc(p, bytes);
}
static int pool_malloc(hlala_ctx* c, void** out, size_t bytes)
{
    bytes = pool_class(bytes);
    std::lock_guard<std::mutex> g(c->pool_mu);
    auto it = c->pool.lower_bound(bytes);
    if(it != c->pool.end() && it->first <= bytes + bytes / 4 + 4096) {
        *out = it->second; c->pool_bytes -= it->first; c->pool.erase(it);
        return 0;
    }
    void* p = nullptr;
    hipError_t e = device_malloc_retry(c->device, c, &p, bytes);       // out of memory with blocks parked (here or in another context of the device): released, then retried
    if(e != hipSuccess) { c->err = std::string("hipMalloc: ") + hipGetErrorString(e); return HLALA_E_DEVICE; }
    c->block_bytes[p] = bytes;
    *out = p;
    return 0;
}
static void pool_release(hlala_ctx* c, void* p)
{
    if(!p) return;
    std::lock_guard<std::mutex> g(c->pool_mu);
    auto it = c->block_bytes.find(p);
    if(it == c->block_bytes.end()) { (void)hipFree(p); return; }
    if(c->pool_bytes + it->second > c->pool_cap) { c->block_bytes.erase(it); (void)hipFree(p); return; }      // keep at most 176 GB parked (three 1 M-pair batches' arrays: a caller with three sets of outputs live gives them all back between two runs)
    c->pool.emplace(it->second, p); c->pool_bytes += it->second;
}

constexpr size_t PIN_GRANULE = (size_t)64 << 20;
template <class T>
static int dev_upload(hlala_ctx* c, std::vector<void*>& allocs, const T* host, size_t n, T** out)
{
    *out = nullptr;
    size_t bytes = (n ? n : 1) * sizeof(T);
    void* p = nullptr;
    { int rc_ = pool_malloc(c, &p, bytes); if(rc_) return rc_; }
    allocs.push_back(p);
    // A caller's array may be page-locked piece by piece (hlala_seed_batch_pin(S, 2): pieces that begin and end on multiples of PIN_GRANULE bytes of address); the
    // runtime refuses a copy whose source straddles two registrations, so no copy crosses such an address -- a dozen copies per GB instead of one.
    if(n && host) {
        const char* src = (const char*)host; char* dst = (char*)p; size_t left = n * sizeof(T);
        while(left) {
            const size_t toEdge = PIN_GRANULE - (size_t)((uintptr_t)src & (PIN_GRANULE - 1)), k = left < toEdge ? left : toEdge;
            HIP_TRY(c, hipMemcpyAsync(dst, src, k, hipMemcpyHostToDevice, c->active));
            src += k; dst += k; left -= k;
        }
    }
    *out = (T*)p;
    return 0;
}
template <class T>
static int dev_alloc(hlala_ctx* c, std::vector<void*>& allocs, size_t n, T** out, bool zero = false)
{
    *out = nullptr;
    size_t bytes = (n ? n : 1) * sizeof(T);
    void* p = nullptr;
    { int rc_ = pool_malloc(c, &p, bytes); if(rc_) return rc_; }
    allocs.push_back(p);
    if(zero) HIP_TRY(c, hipMemsetAsync(p, 0, bytes, c->active));
    *out = (T*)p;
    return 0;
}
#define UP(vec, field) do { int rc_ = dev_upload(c, c->allocs, (vec).data(), (vec).size(), &tmp_##field); if(rc_) return rc_; } while(0)

// ---- host-side constant tables (host libm => bit-identical to a CPU evaluation of the reference formulas)

/* Utilities::PhredToPCorrect, Utilities.cpp:357-377 */
static double host_PhredToPCorrect(unsigned char q)
{
    if(q == 0) return -1;
    int illuminaPhred = (int)q - 33;
    double log10_pWrong = (double)illuminaPhred / (double)-10;
    double pWrong = exp(log(10) * log10_pWrong);
    return 1 - pWrong;
}
/* Utilities::PCorrectToPhred (Utilities.cpp:178-203) as a function of pWrong */
static int host_phred_of_pwrong(double pWrong)
{
    if(pWrong == 0) pWrong = 1e-100;
    double phred1 = -10.0 * log10(pWrong);
    if((phred1 + 33) > 255) phred1 = 255 - 33;
    return (int)round(phred1 + 33);
}
/* boost::math::pdf(normal) closed form, see oracle header note; processBAM.cpp:2343, 3446 */
static double host_normal_pdf(double mean, double sd, double x)
{
    double exponent = x - mean;
    exponent *= -exponent;
    exponent /= 2 * sd * sd;
    double result = exp(exponent);
    result /= sd * sqrt(2 * 3.141592653589793238462643383279502884);
    return result;
}

static int build_tables(hlala_ctx* c)
{
    DevTables T;
    memset(&T, 0, sizeof(T));
    for(int q = 0; q < 256; q++) {
        double pCorrect = host_PhredToPCorrect((unsigned char)q);
        if(q < 33) pCorrect = host_PhredToPCorrect(33);         // the reference asserts illuminaPhred >= 0; never indexed for valid input
        if(pCorrect > 0.999) pCorrect = 0.999;                    // conservativeReadQualities, extensionAligner.cpp:128-131
        if(pCorrect == 0) pCorrect = 0.00001;
        T.ll_match[q] = log(pCorrect);
        double pIncorrect = 1 - pCorrect; pIncorrect *= (1.0 / 3.0);
        T.ll_mismatch[q] = log(pIncorrect);
        T.pcorrect[q] = host_PhredToPCorrect((unsigned char)q);
    }
    double rate = c->params.long_read_mode ? log(0.075) : log(0.001);
    T.rate_indel = rate;
    T.rate_ins_quarter = rate + log(1.0 / 4.0);
    T.rate_match_mismatch = log(1 - exp(rate) - exp(rate));
    // PCorrectToPhred thresholds: phred_thr[k] = largest pWrong (as a double) that still maps to a Phred char >= k
    for(int k = 0; k < 256; k++) {
        if(host_phred_of_pwrong(1.0) >= k) { T.phred_thr[k] = 1.0; continue; }
        double lo = 1e-300, hi = 1.0;      // f(lo) >= k (= 255), f(hi) < k
        uint64_t blo, bhi; memcpy(&blo, &lo, 8); memcpy(&bhi, &hi, 8);
        while(bhi - blo > 1) {
            uint64_t mid = blo + (bhi - blo) / 2; double m; memcpy(&m, &mid, 8);
            if(host_phred_of_pwrong(m) >= k) blo = mid; else bhi = mid;
        }
        double r; memcpy(&r, &blo, 8);
        T.phred_thr[k] = r;
    }
    // insert-size log pdf over every integer distance with a positive density
    double mean = c->params.insert_mean, sd = c->params.insert_sd;
    std::vector<double> tbl;
    T.is_dmin = 0; T.is_n = 0;
    if(sd > 0) {
        T.is_penalty = log(host_normal_pdf(mean, sd, mean + 8 * sd));
        long long dmin = (long long)floor(mean - 40 * sd) - 2, dmax = (long long)ceil(mean + 40 * sd) + 2;
        if(dmax - dmin > 50000000) { c->err = "insert size sd too large for the log-pdf table"; return HLALA_E_ARG; }
        if(host_normal_pdf(mean, sd, (double)dmin) > 0 || host_normal_pdf(mean, sd, (double)dmax) > 0) { c->err = "log-pdf table does not reach zero density"; return HLALA_E_ARG; }
        tbl.resize((size_t)(dmax - dmin + 1));
        for(long long d = dmin; d <= dmax; d++) {
            double p = host_normal_pdf(mean, sd, (double)d);
            tbl[(size_t)(d - dmin)] = (p <= 0) ? T.is_penalty : log(p);             // processBAM.cpp:3447-3464
        }
        T.is_dmin = (int)dmin; T.is_n = (int)tbl.size();
    }
    int rc = dev_upload(c, c->allocs, tbl.data(), tbl.size(), &c->d_islog); if(rc) return rc;
    T.is_logpdf = c->d_islog;
    rc = dev_upload(c, c->allocs, &T, 1, &c->dT); if(rc) return rc;
    return 0;
}

template <class T>
static int dl(hlala_ctx* c, T* host, const T* dev, size_t n)
{
    if(!host || !n) return 0;
    HIP_TRY(c, hipMemcpyAsync(host, dev, n * sizeof(T), hipMemcpyDeviceToHost, c->active));
    return 0;
}

extern "C" {

const char* hlala_last_error(const hlala_ctx* ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

int hlala_create(hlala_ctx** out, int device, void* stream, const hlala_graph_desc* graph, const hlala_contigs_desc* contigs, const hlala_params* params)
{
    if(!out || !graph || !params) { g_create_error = "null argument"; return HLALA_E_ARG; }
    *out = nullptr;
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if(e != hipSuccess || ndev <= 0 || device >= ndev) {
        g_create_error = std::string("no HIP device available (") + (e != hipSuccess ? hipGetErrorString(e) : "device index out of range") + "); this library has no CPU fallback";
        return HLALA_E_DEVICE;
    }
    hlala_ctx* c = new hlala_ctx();
    c->device = device; c->stream = (hipStream_t)stream; c->active = c->stream; c->params = *params;
    auto fail = [&](int rc) { g_create_error = c->err; hlala_destroy(c); return rc; };
    if(c->params.max_columns < 16 || c->params.max_columns > 65536) { c->err = "params.max_columns out of range"; return fail(HLALA_E_ARG); }
    DevGuard dev_guard_(device);       // the caller's current device is restored on return
    { int cur_ = -1; if(hipGetDevice(&cur_) != hipSuccess || cur_ != device) { c->err = "hipSetDevice failed"; return fail(HLALA_E_DEVICE); } }
    const bool keepUnitJumps = [] { const char* e = getenv("HLALA_UNIT_JUMPS"); return e && atoi(e) != 0; }();       // (A/B and parity: the one-edge gap paths stay in the device's jump tables)
    std::string ferr = flatten_graph(graph, contigs, c->F, keepUnitJumps);
    if(!ferr.empty()) { c->err = ferr; return fail(HLALA_E_GRAPH); }
    FlatGraph& F = c->F;
    if(F.N >= (1 << 28) || F.L >= (1 << 24)) { c->err = "graph exceeds 2^28 nodes or 2^24 levels (DP cell key layout)"; return fail(HLALA_E_CAPACITY); }
    // the push index of a DP candidate holds the rank of its edge among the PARALLEL edges (same two nodes) in 7 bits: a node may have any number of
    // edges and gap-path jumps, but more than 127 parallel ones between two nodes are refused here instead of dropping pairs later
    if(F.max_parallel > DP_MAX_PARALLEL) {
        c->err = "graph has " + std::to_string(F.max_parallel) + " parallel edges or gap paths between one pair of nodes: more than the " + std::to_string(DP_MAX_PARALLEL) + " the DP's push-index field ranks";
        return fail(HLALA_E_CAPACITY);
    }
    if(F.max_nodes_per_level > PROJ_NODES) { c->err = "more nodes in one level than this build holds in LDS (PROJ_NODES)"; return fail(HLALA_E_CAPACITY); }
    if(c->params.max_columns > PROJL_CAP) { c->err = "params.max_columns exceeds the column capacity of this build (16384)"; return fail(HLALA_E_ARG); }
    DevGraph& G = c->G;
    G.L = F.L; G.N = F.N; G.E = F.E; G.P = (int)F.path_len.size();
    std::vector<uint8_t> edge_label(graph->edge_label, graph->edge_label + graph->n_edges);
    int rc = 0;
#define UPG(field, vec) do { rc = dev_upload(c, c->allocs, (vec).data(), (vec).size(), (std::remove_const<std::remove_pointer<decltype(G.field)>::type>::type**)&G.field); if(rc) return fail(rc); } while(0)
    UPG(level_off, F.level_off); UPG(node_level, F.node_level); UPG(node_orig, F.node_orig);
    UPG(out_off, F.out_off); UPG(out_to, F.out_to); UPG(out_label, F.out_label); UPG(out_eid, F.out_eid);
    UPG(in_off, F.in_off); UPG(in_from, F.in_from); UPG(in_label, F.in_label); UPG(in_eid, F.in_eid); UPG(in_rec, F.in_rec); UPG(level_fast, F.level_fast);
    UPG(edge_from_new, F.edge_from_new); UPG(edge_to_new, F.edge_to_new); UPG(edge_label, edge_label);
    // (the device's jump tables hold the gap paths of two and more edges only: a one-edge path is a no-op for the DP, flat_graph.hpp)
    UPG(jf_off, F.djf_off); UPG(jf_node, F.djf_node); UPG(jf_path, F.djf_path);
    UPG(jb_off, F.djb_off); UPG(jb_node, F.djb_node); UPG(jb_path, F.djb_path);
    UPG(jf_lvl, F.djf_lvl); UPG(jb_lvl, F.djb_lvl);
    UPG(jfree_out, F.jfree_out); UPG(jfree_in, F.jfree_in);
    UPG(lin_out, F.lin_out); UPG(lin_in, F.lin_in);
    UPG(npf_label, F.npf_label); UPG(npf_eid, F.npf_eid); UPG(npf_node, F.npf_node); UPG(npf_steps, F.npf_steps); UPG(npf_pos, F.npf_pos);
    UPG(npb_label, F.npb_label); UPG(npb_eid, F.npb_eid); UPG(npb_node, F.npb_node); UPG(npb_steps, F.npb_steps); UPG(npb_pos, F.npb_pos);
    UPG(out_prank, F.out_prank); UPG(in_prank, F.in_prank); UPG(jf_prank, F.jf_prank); UPG(jb_prank, F.jb_prank);
    { int* p_ = nullptr; rc = dev_upload(c, c->allocs, F.nrec_out.data(), F.nrec_out.size(), &p_); if(rc) return fail(rc); G.nrec_out = (const int4*)p_;
      rc = dev_upload(c, c->allocs, F.nrec_in.data(), F.nrec_in.size(), &p_); if(rc) return fail(rc); G.nrec_in = (const int4*)p_; }
    UPG(path_len, F.path_len); UPG(path_edges, F.path_edges);
    {
        std::vector<long long> po(F.path_off.begin(), F.path_off.end());
        rc = dev_upload(c, c->allocs, po.data(), po.size(), (long long**)&G.path_off); if(rc) return fail(rc);
        std::vector<long long> lo(F.lp_off.begin(), F.lp_off.end());
        rc = dev_upload(c, c->allocs, lo.data(), lo.size(), (long long**)&G.lp_off); if(rc) return fail(rc);
    }
    UPG(gap_stretch, F.gap_stretch); UPG(lp_seqid, F.lp_seqid); UPG(lp_pos, F.lp_pos);
#undef UPG
    if(contigs && contigs->n_contigs > 0) {
        c->n_contigs = contigs->n_contigs;
        c->contig_off.assign(contigs->contig_off, contigs->contig_off + contigs->n_contigs + 1);
        size_t total = (size_t)c->contig_off.back();
        std::vector<long long> co(c->contig_off.begin(), c->contig_off.end());
        rc = dev_upload(c, c->allocs, co.data(), co.size(), &c->d_contig_off); if(rc) return fail(rc);
        rc = dev_upload(c, c->allocs, contigs->contig_seq, total, &c->d_contig_seq); if(rc) return fail(rc);
        rc = dev_upload(c, c->allocs, contigs->contig_level, total, &c->d_contig_level); if(rc) return fail(rc);
    }
    rc = build_tables(c); if(rc) return fail(rc);
    rc = dev_upload(c, c->allocs, &c->G, 1, &c->dG); if(rc) return fail(rc);
    // scratch slabs: one per resident wavefront (persistent grid, dynamic work distribution)
    hipDeviceProp_t prop;
    if(hipGetDeviceProperties(&prop, device) != hipSuccess) { c->err = "hipGetDeviceProperties failed"; return fail(HLALA_E_DEVICE); }
    int cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    // DP slab pools, one per class and zeroed once: a slab's early-cell table is cleared by the first DP call that needs it and kept clean from then on
    // (kernel_dp.hip: DP_SLAB_READY), which only holds while no other class lays its own arrays over the same memory
    auto slab_pool = [&](char** out, size_t bytes, const char* what) -> int {
        if(device_malloc_retry(c->device, nullptr, (void**)out, bytes) != hipSuccess) { c->err = std::string("hipMalloc(") + what + ") failed"; return HLALA_E_DEVICE; }
        c->allocs.push_back(*out);
        if(hipMemsetAsync(*out, 0, bytes, c->active) != hipSuccess) { c->err = std::string("hipMemset(") + what + ") failed"; return HLALA_E_DEVICE; }
        return 0;
    };
    c->band_grid = cus * 20;          // a few KB of LDS per block, five waves per SIMD (96 VGPRs, nothing spilled)
    if(const char* e = getenv("HLALA_DP_BAND")) { if(atoi(e) == 0) c->band_grid = 0; }      // (A/B and parity: every call in the hashed-frontier classes)
    if(const char* e = getenv("HLALA_DP_BAND_RISKY")) c->band_risky = atoi(e) != 0;
    if(const char* e = getenv("HLALA_DP_BAND_NODES")) c->band_nodes = atoi(e) != 0;
    if(const char* e = getenv("HLALA_ROWS_ALL")) c->rows_all = atoi(e) != 0;
    if(const char* e = getenv("HLALA_SIDE_AFTER_PAIR")) c->side_after_pair = atoi(e) != 0;
    if(const char* e = getenv("HLALA_POOL_CAP_GB")) { const long g = atol(e); if(g >= 0 && g <= 1024) c->pool_cap = (size_t)g << 30; }
    if(const char* e = getenv("HLALA_DP_BAND_MARGIN")) { const int m = atoi(e); if(m >= 0 && m <= 24) c->band_margin = m; }
    if(const char* e = getenv("HLALA_DP_JF_MARGIN")) { const int m = atoi(e); if(m >= 0 && m <= 200) c->jf_margin = m; }      // (A/B: levels beyond the read bases left that a jump-free call may reach)
    if(const char* e = getenv("HLALA_DP_LONG_BASES")) { const int m = atoi(e); if(m >= 0 && m <= 4096) c->dp_long_bases = m; }
    c->stitch_grid = cus * 20;        // k_stitch_chains: five waves per SIMD (92 VGPRs, nothing spilled)
    if(const char* e = getenv("HLALA_STITCH_BY_ROW")) c->stitch_by_row = atoi(e) != 0;
    // The table of DP classes: blocks, bytes per slab, then one pool per slab layout.  The 64-lane and the wide class have slabs of one size (the larger layout of the two),
    // so have the broad and the large class, which also share a pool: broad blocks first, then the large ones.
    const size_t extBytes = std::max(dp_slab_bytes<DpSmall>(), dp_slab_bytes<DpWide>()), largeBytes = std::max(dp_slab_bytes<DpLarge>(), dp_slab_bytes<DpBroad>());      // (large: one / three blocks per CU, a few MB each)
    DpClass* const dp = c->dp;
    c->dp_jf = dp_class<DpTinyJF, 0>(cus * 4 * DpTinyJF::WAVES, dp_slab_bytes<DpTiny>(), "k_dp<DpTinyJF>");
    dp[0] = dp_class<DpTiny, 0>(cus * 4 * DpTiny::WAVES, dp_slab_bytes<DpTiny>(), "k_dp<DpTiny>");
    dp[1] = dp_class<DpMid, 1>(cus * 16, dp_slab_bytes<DpMid>(), "k_dp<DpMid>");
    dp[2] = dp_class<DpSmall, 2>(cus * 20, extBytes, "k_dp<DpSmall>");
    dp[3] = dp_class<DpWide, 3>(cus * 7, extBytes, "k_dp<DpWide>");              // LDS: seven DpWide blocks per CU (22 KB each)
    dp[4] = dp_class<DpBroad, 4>(cus * 3, largeBytes, "k_dp<DpBroad>");          // three DpBroad blocks per CU (48 KB of LDS each)
    dp[5] = dp_class<DpLarge, 5>(cus, largeBytes, "k_dp<DpLarge>");
    dp[6] = dp_class<DpHuge, 6>(cus / 4 > 0 ? cus / 4 : 1, dp_inmemory_bytes<DpHuge>(), "k_dp<DpHuge>");      // the in-memory backstop class: a handful of DP calls per million pairs
    if((rc = slab_pool(&dp[0].slabs, dp[0].slab_bytes * (size_t)(64 / DpTiny::GW) * (size_t)std::max(dp[0].grid, c->dp_jf.grid), "16-lane DP slabs"))) return fail(rc);
    c->dp_jf.slabs = dp[0].slabs;
    if((rc = slab_pool(&dp[1].slabs, dp[1].slab_bytes * (size_t)(64 / DpMid::GW) * (size_t)dp[1].grid, "32-lane DP slabs"))) return fail(rc);
    if((rc = slab_pool(&dp[2].slabs, extBytes * (size_t)dp[2].grid, "64-lane DP slabs"))) return fail(rc);
    if((rc = slab_pool(&dp[3].slabs, extBytes * (size_t)dp[3].grid, "wide-class DP slabs"))) return fail(rc);
    if((rc = slab_pool(&dp[4].slabs, largeBytes * (size_t)(dp[4].grid + dp[5].grid), "large-class DP slabs"))) return fail(rc);
    dp[5].slabs = dp[4].slabs + largeBytes * (size_t)dp[4].grid;
    if((rc = slab_pool(&dp[6].slabs, dp[6].slab_bytes * (size_t)dp[6].grid, "in-memory DP class"))) return fail(rc);
    // k_project_chains<384 columns>: 143 VGPRs = three waves per SIMD = 12 resident blocks per CU (its 11.7 KB of LDS would allow 13); the 512-column
    // layout: 173 VGPRs = two per SIMD (-Rpass-analysis=kernel-resource-usage; a cap of 128 VGPRs for a fourth wave costs 287 spilled SGPRs and wins one block)
    c->proj_grid = cus * (c->params.max_columns <= PROJ_CAP_SHORT ? 12 : 8); c->pair_grid = cus * 16; c->pair_lean_grid = cus * 24;      // k_pair_multi<., false>: four waves per SIMD (125 registers, nothing spilled); k_pair_chains (0.7 KB of LDS, 80 registers): six
    { int rcp = dev_alloc(c, c->allocs, (size_t)2 * c->pair_grid * PAIR_COMB, &c->pair_scratch, false); if(rcp) return fail(rcp); }
    if(c->params.max_columns > PROJ_CAP) {       // long reads: the projection keeps its column / window arrays in HBM, fewer and bigger blocks
        c->proj_grid = cus * 20;       // (round 6: 20 waves per CU -- 95 VGPRs, five per SIMD, 6.3 KB of LDS each; round 5: 16 waves per CU -- 103 VGPRs, four per SIMD; with 4 per CU the kernel ran one wave per SIMD, waiting 72 % of its cycles: 71 k -> 82 k reads/s in batches of 10 000, 223 k in one batch of 50 000)
        c->proj_long_slab_bytes = proj_long_slab_bytes();
        c->stitch_draw = 1;       // rows of 16 384 columns: one chain per draw (12: 11.0 ms per 50 000 reads, 1: 8.8; a batch of 12 500: 7.9 -> 4.0 ms)
        if(device_malloc_retry(c->device, nullptr, (void**)&c->proj_long_slabs, c->proj_long_slab_bytes * (size_t)c->proj_grid) != hipSuccess) { c->err = "hipMalloc(long-read projection slabs) failed"; return fail(HLALA_E_DEVICE); }
        c->allocs.push_back(c->proj_long_slabs);
    }
    c->proj_slab_bytes = proj_slab_bytes_host(c->params.max_columns, F.max_nodes_per_level);
    if(device_malloc_retry(c->device, nullptr, (void**)&c->proj_slabs, c->proj_slab_bytes * (size_t)c->proj_grid) != hipSuccess) { c->err = "hipMalloc(projection slabs) failed"; return fail(HLALA_E_DEVICE); }
    c->allocs.push_back(c->proj_slabs);
    if(!c->proj_long_slabs) {
        const char* e = getenv("HLALA_RETHREAD");
        if(!(e && atoi(e) == 0)) {
            // a chain of that kernel has at most RT_SN nodes per level: its window holds at most max_columns * RT_SN nodes
            size_t ent = (size_t)c->params.max_columns * (size_t)RT_SN; if(ent < 1024) ent = 1024;
            c->rethread_slab_bytes = (ent * sizeof(ChoiceRec) + 255) & ~(size_t)255;
            if(c->rethread_slab_bytes > c->proj_slab_bytes) c->rethread_slab_bytes = c->proj_slab_bytes;
            c->rethread_grid = cus * 24;
            if(device_malloc_retry(c->device, nullptr, (void**)&c->rethread_slabs, c->rethread_slab_bytes * (size_t)c->rethread_grid) != hipSuccess) { c->err = "hipMalloc(re-threading slabs) failed"; return fail(HLALA_E_DEVICE); }
            c->allocs.push_back(c->rethread_slabs);
        }
    }
    // position buckets: a few hundred levels each, at most 16 384 of them (the scan is one block)
    { const char* e = getenv("HLALA_LOCALITY");
      if(!(e && atoi(e) == 0)) { int sh = 8; if(e && atoi(e) >= 2 && atoi(e) <= 20) sh = atoi(e); while((F.L >> sh) + 2 > 16384) sh++; c->order_shift = sh; c->order_nb = (F.L >> sh) + 2; } }
    if(const char* e = getenv("HLALA_LONG_CHUNK_NODES")) { const int v = atoi(e); if(v >= 1) c->long_chunk_nodes = v; }
    if(const char* e = getenv("HLALA_LONG_MAXSEGS")) { const int v = atoi(e); if(v >= 0) c->long_max_segs = v; }
    if(c->proj_long_slabs && c->order_nb > 0) { const char* e = getenv("HLALA_LONG_ORDER"); c->order_cost = (e && atoi(e) == 0) ? 0 : 1; }
    // (the debug buffer is DEVICE memory since round 6: host-mapped, every counter a kernel added to it was an atomic over PCIe -- the wavefronts of the long-read projection queued
    //  behind each other's, and the clocks they were meant to read showed that queue)
    if(getenv("HLALA_DEBUG")) { if(hipMalloc((void**)&c->dbg_host, 8192 * sizeof(int)) != hipSuccess) c->dbg_host = nullptr; else { (void)hipMemset(c->dbg_host, 0, 8192 * sizeof(int)); c->allocs.push_back(c->dbg_host); } }
    if(hipEventCreateWithFlags(&c->evSideTail, hipEventDisableTiming) != hipSuccess) { c->err = "hipEventCreate failed"; return fail(HLALA_E_DEVICE); }
    { int prLow = 0, prHigh = 0; (void)hipDeviceGetStreamPriorityRange(&prLow, &prHigh);       // (numerically greatest = lowest priority)
      // the upload and the reader stream carry copies and a few small kernels (filters, position order, unpacking; export, packing) that the host WAITS for beside the
      // persistent kernels of the alignment streams: highest priority, so that they get the first wave slots that come free.  The side stream's classes: lowest
      if(hipStreamCreateWithPriority(&c->up, hipStreamNonBlocking, prHigh) != hipSuccess || hipStreamCreateWithPriority(&c->rs, hipStreamNonBlocking, prHigh) != hipSuccess ||
         hipStreamCreateWithPriority(&c->side, hipStreamNonBlocking, prLow) != hipSuccess) { c->err = "hipStreamCreate failed"; return fail(HLALA_E_DEVICE); } }
    if(hipStreamSynchronize(c->active) != hipSuccess) { c->err = "upload failed"; return fail(HLALA_E_DEVICE); }
    { std::lock_guard<std::mutex> g(g_ctx_mu); g_ctxs.push_back(c); }
    *out = c;
    return HLALA_OK;
}

void hlala_destroy(hlala_ctx* c)
{
    if(!c) return;
    DEV_GUARD(c);
    { std::lock_guard<std::mutex> g(g_ctx_mu); g_ctxs.erase(std::remove(g_ctxs.begin(), g_ctxs.end(), c), g_ctxs.end()); }
    if(!c->tail.empty()) (void)flush_tail(c);
    for(hlala_batch* b : c->batches) b->ctx = nullptr;       // a batch that outlives its context frees its own buffers
    for(void* p : c->allocs) if(p) (void)hipFree(p);
    if(c->pair_over_slabs) (void)hipFree(c->pair_over_slabs);
    if(c->create_scratch) { if(c->create_scratch_pinned) (void)hipHostFree(c->create_scratch); else free(c->create_scratch); }
    for(hlala_ctx::KeptReads& kr : c->kept) { (void)hipFree(kr.store); (void)hipFree(kr.start); (void)hipFree(kr.length); }
    for(auto& kv : c->pool) (void)hipFree(kv.second);
    if(c->side) { (void)hipStreamSynchronize(c->side); (void)hipStreamDestroy(c->side); }
    if(c->up) { (void)hipStreamSynchronize(c->up); (void)hipStreamDestroy(c->up); }
    if(c->rs) { (void)hipStreamSynchronize(c->rs); (void)hipStreamDestroy(c->rs); }
    if(c->evSideTail) (void)hipEventDestroy(c->evSideTail);
    delete c;
}

int hlala_graph_get_info(const hlala_ctx* c, hlala_graph_info* info)
{
    if(!c || !info) return HLALA_E_ARG;
    const FlatGraph& F = c->F;
    memset(info, 0, sizeof(*info));
    info->n_levels = F.L; info->n_nodes = F.N; info->n_edges = F.E; info->n_paths = (int)F.path_len.size();
    info->n_jump_entries = (int64_t)F.jf_node.size(); info->n_path_edges = (int64_t)F.path_edges.size();
    info->n_levelpos_entries = (int64_t)F.lp_seqid.size();
    info->max_nodes_per_level = F.max_nodes_per_level; info->max_out_degree = F.max_out_degree; info->max_in_degree = F.max_in_degree; info->max_jumps = F.max_jumps; info->max_parallel = F.max_parallel;
    for(uint8_t b : F.gap_stretch) info->n_gap_stretch_levels += b;
    return HLALA_OK;
}
int hlala_graph_get_nodes(const hlala_ctx* c, int32_t* node_orig, int32_t* level_off)
{
    if(!c) return HLALA_E_ARG;
    if(node_orig) memcpy(node_orig, c->F.node_orig.data(), c->F.node_orig.size() * 4);
    if(level_off) memcpy(level_off, c->F.level_off.data(), c->F.level_off.size() * 4);
    return HLALA_OK;
}
int hlala_graph_get_paths(const hlala_ctx* c, int32_t* first_node, int32_t* last_node, int32_t* length)
{
    if(!c) return HLALA_E_ARG;
    const FlatGraph& F = c->F;
    for(size_t p = 0; p < F.path_len.size(); p++) {
        if(first_node) first_node[p] = F.node_orig[F.path_first[p]];
        if(last_node) last_node[p] = F.node_orig[F.path_last[p]];
        if(length) length[p] = F.path_len[p];
    }
    return HLALA_OK;
}
int hlala_graph_get_gap_stretch(const hlala_ctx* c, uint8_t* in_stretch)
{
    if(!c || !in_stretch) return HLALA_E_ARG;
    memcpy(in_stretch, c->F.gap_stretch.data(), c->F.gap_stretch.size());
    return HLALA_OK;
}

// ------------------------------------------------------------------------------------ batches

static int batch_alloc_outputs(hlala_ctx* c, hlala_batch* b)
{
    DevBatch& B = b->B;
    size_t nc = (size_t)B.n_chains, nr = (size_t)B.n_reads, np = (size_t)B.n_pairs;
    // column rows: one per chain that passed the filters when they ran at creation (batch.h: chain_row), else one per chain
    if(!b->prepared) { B.n_rows = B.n_chains; B.chain_row = nullptr; }
    // (the column arrays are sized for the row count rounded up to a 64th of the chain count: consecutive batches of a sample differ by a per cent in the chains that
    //  pass the filters, and with exact sizes their arrays fell into different size classes of the pool every few batches -- a hipMalloc / hipFree pair of gigabytes, each a
    //  device-wide synchronisation, in front of the next launch)
    size_t rowsAlloc = (size_t)(B.n_rows > 0 ? B.n_rows : 1);
    if(b->prepared && nc >= 4096) { const size_t gran = nc / 64; rowsAlloc = (rowsAlloc + gran - 1) / gran * gran; if(rowsAlloc > nc) rowsAlloc = nc; }
    const size_t cs = rowsAlloc * (size_t)B.stride;
    int rc = 0;
#define AL(field, n, zero) do { rc = dev_alloc(c, b->allocs, (n), &B.field, zero); if(rc) return rc; } while(0)
    if(!b->prepared) { AL(seed_status, nc, true); AL(seed_ncols, nc, true); }
    AL(seed_begin, nc, true); AL(seed_end, nc, true); AL(seed_removed, nc, true);
    AL(seed_level, cs, false); AL(seed_edge, cs, false); AL(seed_g, cs, false); AL(seed_s, cs, false);
    AL(ext_status, nc, true); AL(ext_ncols, nc, true); AL(ext_begin, nc, true); AL(ext_end, nc, true); AL(ext_ll, nc, true);
    AL(dp_iters, 2 * nc, true); AL(dp_score, 2 * nc, true); AL(dp_ncols, 2 * nc, true); AL(dp_sb, 2 * nc, true); AL(dp_se, 2 * nc, true); AL(dp_err, 2 * nc, true);
    AL(dp_alias_head, 2 * nc, false); AL(dp_alias_next, 2 * nc, false);
    AL(ext_level, cs, false); AL(ext_edge, cs, false); AL(ext_g, cs, false); AL(ext_s, cs, false); AL(ext_fromseed, cs, false);
    AL(ext_firstlast, 4 * nc, true);
    AL(pair_status, np, true); AL(best_chain, nr, true); AL(n_comb, np, true); AL(pair_ll, np, true); AL(pair_mapq, np, true);
    AL(mate_mapq, nr, true); AL(strands_valid, np, true); AL(sel_mapq, nr * (size_t)B.stride, true);
    AL(pair_deferred, np, true); AL(pair_multi, 7 * np, false); AL(counters, 32, true); AL(work_counter, WC_N, true); AL(retry_list, 16 * nc, false);
    { DpItem* it = nullptr; rc = dev_alloc(c, b->allocs, 2 * nc, &it, false); if(rc) return rc; B.dp_items = it; }
    B.dp_nblk = (int)((nc + 255) / 256); if(B.dp_nblk < 1) B.dp_nblk = 1;
    B.dp_jf = c->jf_margin + 1; B.dp_long = c->dp_long_bases;
    B.dp_band = c->band_grid > 0 ? c->band_margin + 1 : 0;
    B.dp_band_risky = c->band_risky ? 1 : 0;
    B.dp_band_nodes = c->band_nodes ? 1 : 0;
    AL(dp_blk, (size_t)DPL_N * B.dp_nblk + 1, false); AL(dp_list, 2 * nc, false);
    if(!b->prepared) {
        B.chain_order = nullptr; B.chain_bucket = nullptr; B.order_hist = nullptr; B.order_shift = c->order_shift; B.order_nb = c->order_nb; B.order_cost = c->order_cost; B.long_chunk_nodes = c->long_chunk_nodes; B.long_max_segs = c->long_max_segs;
        if(c->order_nb > 0 && !B.from_seeds && nc > 0) { AL(chain_order, nc, false); AL(chain_bucket, nc, false); AL(order_hist, (size_t)c->order_nb + 1, false); }
    }
    B.dbg = c->dbg_host;
#undef AL
    return 0;
}

// The context's host scratch of a batch creation (page-locked when the runtime grants it), grown to `need` bytes.  Nothing may be in flight from it: every batch
// creation ends synchronised.
static int ctx_scratch(hlala_ctx* c, size_t need)
{
    if(need <= c->create_scratch_bytes) return HLALA_OK;
    if(c->create_scratch) { if(c->create_scratch_pinned) (void)hipHostFree(c->create_scratch); else free(c->create_scratch); c->create_scratch = nullptr; c->create_scratch_bytes = 0; }
    const size_t want = need + need / 8;
    void* p = nullptr;
    if(hipHostMalloc(&p, want, hipHostMallocDefault) == hipSuccess) c->create_scratch_pinned = true;
    else { (void)hipGetLastError(); p = malloc(want); c->create_scratch_pinned = false; }
    if(!p) { c->err = "out of host memory (batch scratch)"; return HLALA_E_ARG; }
    c->create_scratch = p; c->create_scratch_bytes = want;
    return HLALA_OK;
}

// The tail of every batch creation whose inputs are in place on the device (uploaded: batch_create_impl; written there: hlala_batch_create_from_fill): the per-chain
// arrays of the filters and the position order, the device descriptor, k_filter_chains / k_order_scan / k_order_scatter on the active stream, the synchronisation the
// creation ends on and, with it, the number of column rows.  *queued: when everything was queued (host timing).  The caller destroys the batch where this fails.
static int batch_create_tail(hlala_ctx* c, hlala_batch* b, std::chrono::steady_clock::time_point* queued)
{
    DevBatch& B = b->B;
    const int nr = B.n_reads, nc = B.n_chains;
    int rc = 0;
    // The OUTPUT arrays are allocated by the first stage call (ensure_outputs): a caller that uploads batch i+2 while batches i and i+1 are aligned and read back
    // (two alignments in flight, one upload ahead) then holds the inputs of three batches -- 0.9 GB each -- but the outputs of two, and the outputs of the batch it
    // destroys are the pool blocks the next alignment takes.  Until then the device descriptor holds the inputs only (what hlala_kmer_presence reads).
    // ... except the few per-chain arrays of the FILTERS and the POSITION ORDER, which read inputs only and run here, on the upload stream: the number of chains that
    // passed -- a third of them on an MHC-scale graph -- comes back with the synchronisation this function ends on anyway, and the column arrays (20 bytes per column slot:
    // 47 GB for the 6.1 M chains of a 1 M-pair batch) are then sized for those chains alone (batch.h: chain_row; HLALA_ROWS_ALL=1: a row per chain, filters at the stage call)
    if(c->order_nb > 0 && nc > 0 && !c->rows_all) {
#define AL(field, n, zero) do { rc = dev_alloc(c, b->allocs, (n), &B.field, zero); if(rc) return rc; } while(0)
        AL(seed_status, (size_t)nc, true); AL(seed_ncols, (size_t)nc, true);
        AL(chain_order, (size_t)nc, false); AL(chain_bucket, (size_t)nc, false); AL(chain_row, (size_t)nc, false); AL(order_hist, (size_t)c->order_nb + 1, true);
#undef AL
        B.order_shift = c->order_shift; B.order_nb = c->order_nb; B.order_cost = c->order_cost; B.long_chunk_nodes = c->long_chunk_nodes; B.long_max_segs = c->long_max_segs;
        b->prepared = true;
    }
    rc = dev_upload(c, b->allocs, &b->B, 1, &b->dB); if(rc) return rc;
    if(b->prepared) {
        hipLaunchKernelGGL(k_filter_chains, dim3((nr + 255) / 256), dim3(256), 0, c->active, c->dG, b->dB, c->d_contig_off, c->d_contig_level);
        hipLaunchKernelGGL(k_order_scan, dim3(1), dim3(ORDER_SCAN_THREADS), 0, c->active, B.order_hist, B.order_nb);
        hipLaunchKernelGGL(k_order_scatter, dim3((nc + 255) / 256), dim3(256), 0, c->active, b->dB);
        { hipError_t el = hipGetLastError(); if(el != hipSuccess) { c->err = std::string("k_order_scatter: ") + hipGetErrorString(el); return HLALA_E_DEVICE; } }
        HIP_TRY(c, hipMemcpyAsync(&b->n_rows_host, B.order_hist + (B.order_nb - 1), sizeof(int), hipMemcpyDeviceToHost, c->active));
    }
    if(queued) *queued = std::chrono::steady_clock::now();
    HIP_TRY(c, hipStreamSynchronize(c->active));
    if(b->prepared) {
        if(b->n_rows_host < 0 || b->n_rows_host > nc) { c->err = "position order counted " + std::to_string(b->n_rows_host) + " chains of " + std::to_string(nc); return HLALA_E_DEVICE; }
        B.n_rows = b->n_rows_host;        // (the device descriptor gets it with the output arrays: ensure_outputs)
    }
    return HLALA_OK;
}

static int batch_create_impl(hlala_ctx* c, const hlala_batch_in* in, hlala_batch** out, bool unpaired);
int hlala_batch_create(hlala_ctx* c, const hlala_batch_in* in, hlala_batch** out) { return batch_create_impl(c, in, out, false); }
int hlala_batch_create_unpaired(hlala_ctx* c, const hlala_batch_in* in, hlala_batch** out) { return batch_create_impl(c, in, out, true); }

static int batch_create_impl(hlala_ctx* c, const hlala_batch_in* in, hlala_batch** out, bool unpaired)
{
    DEV_GUARD(c);
    if(!c || !in || !out) return HLALA_E_ARG;
    UploadScope upscope_(c);           // uploads and the zeroing of the outputs run on the upload stream: beside the alignment of an earlier batch
    *out = nullptr;
    if(in->n_pairs < 0 || in->n_chains < 0) { c->err = "negative batch sizes"; return HLALA_E_ARG; }
    if(!c->d_contig_off) { c->err = "hlala_batch_create needs contigs (hlala_create was called without them)"; return HLALA_E_STATE; }
    static const bool hostTiming = getenv("HLALA_HOST_TIMING") != nullptr;       // (stderr: where hlala_batch_create spends the host thread's time)
    const auto tc0 = std::chrono::steady_clock::now(); auto tc1 = tc0, tc2 = tc0;
    hlala_batch* b = new hlala_batch(); b->ctx = c; c->batches.insert(b);
    DevBatch& B = b->B;
    B.n_pairs = in->n_pairs; B.n_reads = (unpaired ? 1 : 2) * in->n_pairs; B.n_chains = in->n_chains; B.stride = c->params.max_columns; B.from_seeds = 0; B.unpaired = unpaired ? 1 : 0;
    int nr = B.n_reads, nc = B.n_chains;
    auto fail = [&](int rc) { (void)hipStreamSynchronize(c->active); hlala_batch_destroy(b); return rc; };      // (uploads already queued -- from the caller's arrays, from the context's scratch -- end before their blocks go back to the pool)
    // the batch is a window into the caller's arrays (include/hlala_gpu.h: hlala_batch_in): 64-bit offsets that need not start at 0 are rebased here
    const int64_t rb0 = nr > 0 ? in->read_off[0] : 0, cb0 = nr > 0 ? in->chain_off[0] : 0;
    if(nr > 0) {
        const int64_t nbases64 = in->read_off[nr] - rb0, nc64 = in->chain_off[nr] - cb0;
        if(nbases64 < 0 || nc64 != (int64_t)nc || cb0 < 0 || rb0 < 0) { c->err = "inconsistent batch offsets"; return fail(HLALA_E_ARG); }
        if(nbases64 > 0x7FFFFFFFll) { c->err = "batch of " + std::to_string(nbases64) + " read bases: one batch holds at most 2^31 - 1 (cut the sample into more batches: hlala_seed_batch_window)"; return fail(HLALA_E_CAPACITY); }
    } else if(nc != 0) { c->err = "inconsistent batch offsets"; return fail(HLALA_E_ARG); }
    const int64_t gb0 = nc > 0 ? in->cigar_off[cb0] : 0;
    if(nc > 0) { const int64_t ng64 = in->cigar_off[cb0 + nc] - gb0; if(ng64 < 0) { c->err = "inconsistent batch offsets"; return fail(HLALA_E_ARG); }
                 if(ng64 > 0x7FFFFFFFll) { c->err = "batch of " + std::to_string(ng64) + " CIGAR operations: one batch holds at most 2^31 - 1"; return fail(HLALA_E_CAPACITY); } }
    b->first_chain = (uint32_t)cb0;
    // validation the reference would assert on, and the 32-bit arrays of the window (offsets rebased, the read of every chain).  Round 6: two fused passes -- one over the reads, one over
    // the chains -- on a few host threads into page-locked scratch of the context (five passes on the calling thread into fresh vectors before: 30 ms of hlala_batch_create's 75 for a
    // 1 M-pair batch, and their uploads from pageable memory were staged copies the caller waited for).  The FIRST violation in the order of the old passes is the one reported.
    int* chain_read = nullptr; int* read_off32 = nullptr; int* chain_off32 = nullptr; int* primary32 = nullptr; int* cigar_off32 = nullptr;
    {
        const size_t need = ((size_t)nc + (size_t)nr + 1 + (size_t)nr + 1 + (size_t)nr + (size_t)nc + 1 + 16) * sizeof(int);
        { const int rs = ctx_scratch(c, need); if(rs) return fail(rs); }
        int* q = (int*)c->create_scratch;
        chain_read = q; q += nc; read_off32 = q; q += (size_t)nr + 1; chain_off32 = q; q += (size_t)nr + 1; primary32 = q; q += nr; cigar_off32 = q;
    }
    const int32_t* w_contig = in->chain_contig + cb0; const int32_t* w_pos = in->chain_pos + cb0; const int32_t* w_offset = in->chain_offset + cb0; const int32_t* w_as = in->chain_as + cb0;
    const uint8_t* w_rev = in->chain_reverse + cb0;
    {
        // violations by the pass that used to find them: 0 offsets of a read not ascending, 1 per-read checks (the smallest read decides, then the order of the checks within it),
        // 2 CIGAR offsets not ascending, 3 contig out of range, 4 paired read too long
        struct Viol { long long at[5]; int kind1; };
        const int nt = (nr + nc) >= (1 << 18) ? 4 : 1;
        std::vector<Viol> viol((size_t)nt);
        const int n_contigs = c->n_contigs;
        auto work = [&](int t) {
            Viol v; for(int i = 0; i < 5; i++) v.at[i] = -1; v.kind1 = 0;
            const int r0 = (int)((long long)nr * t / nt), r1 = (int)((long long)nr * (t + 1) / nt);
            for(int r = r0; r < r1; r++) {
                const int64_t ro0 = in->read_off[r] - rb0, ro1 = in->read_off[r + 1] - rb0, co0 = in->chain_off[r] - cb0, co1 = in->chain_off[r + 1] - cb0;
                if((ro1 < ro0 || co1 < co0) && v.at[0] < 0) v.at[0] = r;
                read_off32[r] = (int)ro0; chain_off32[r] = (int)co0;
                int kind = 0;
                if((int)co1 <= (int)co0) kind = 1;                         // read without alignments
                else if((int)ro1 < (int)ro0) kind = 2;                     // inconsistent batch offsets
                const int64_t pr = (int64_t)in->read_primary[r] - cb0;
                if(!kind && (pr < (int)co0 || pr >= (int)co1)) kind = 3;    // read_primary outside the read's chains
                if(kind && v.at[1] < 0) { v.at[1] = r; v.kind1 = kind; }
                primary32[r] = (int)pr;
                if(co0 >= 0 && co1 <= (int64_t)nc) for(int64_t k = co0; k < co1; k++) chain_read[k] = r;
                if(!unpaired && (int)ro1 - (int)ro0 > DP_SEQCAP && v.at[4] < 0) v.at[4] = r;
            }
            const int k0 = (int)((long long)nc * t / nt), k1 = (int)((long long)nc * (t + 1) / nt);
            for(int k = k0; k < k1; k++) {
                if(in->cigar_off[cb0 + k + 1] < in->cigar_off[cb0 + k] && v.at[2] < 0) v.at[2] = k;
                cigar_off32[k] = (int)(in->cigar_off[cb0 + k] - gb0);
                if((w_contig[k] < 0 || w_contig[k] >= n_contigs) && v.at[3] < 0) v.at[3] = k;
            }
            viol[(size_t)t] = v;
        };
        if(nt == 1) work(0);
        else {
            // (no exception may leave a C entry point: a thread that cannot be started -- a process at its thread limit -- leaves its share to the calling thread)
            std::vector<std::thread> th; int started = 0;
            try { th.reserve((size_t)nt); for(int t = 1; t < nt; t++) { th.emplace_back(work, t); started++; } } catch(...) { }
            work(0);
            for(int t = started + 1; t < nt; t++) work(t);
            for(std::thread& x : th) x.join();
        }
        if(nr > 0) { read_off32[nr] = (int)(in->read_off[nr] - rb0); chain_off32[nr] = (int)(in->chain_off[nr] - cb0); } else { read_off32[0] = 0; chain_off32[0] = 0; }      // (an empty batch: no stale word of the scratch goes up)
        if(nc > 0) cigar_off32[nc] = (int)(in->cigar_off[cb0 + nc] - gb0); else cigar_off32[0] = 0;
        long long first[5] = {-1, -1, -1, -1, -1}; int kind1 = 0;
        for(int t = 0; t < nt; t++) for(int i = 0; i < 5; i++) if(viol[(size_t)t].at[i] >= 0 && (first[i] < 0 || viol[(size_t)t].at[i] < first[i])) { first[i] = viol[(size_t)t].at[i]; if(i == 1) kind1 = viol[(size_t)t].kind1; }
        if(first[0] >= 0) { c->err = "inconsistent batch offsets"; return fail(HLALA_E_ARG); }
        if(first[1] >= 0) { c->err = kind1 == 1 ? "read without alignments" : (kind1 == 2 ? "inconsistent batch offsets" : "read_primary outside the read's chains"); return fail(HLALA_E_ARG); }
        if(first[2] >= 0) { c->err = "inconsistent batch offsets"; return fail(HLALA_E_ARG); }
        if(first[3] >= 0) { c->err = "chain_contig out of range"; return fail(HLALA_E_ARG); }
        // the extension DP of paired reads keys its cells with a 12-bit read coordinate (kernel_dp.hip: mk_key): longer reads belong in an unpaired batch
        if(first[4] >= 0) {
            const int r = (int)first[4];
            c->err = "paired read of " + std::to_string(read_off32[r + 1] - read_off32[r]) + " bases: the paired path holds reads of at most " + std::to_string(DP_SEQCAP) + " (use hlala_batch_create_unpaired for long reads)";
            return fail(HLALA_E_CAPACITY);
        }
    }
    size_t nbases = nr ? (size_t)read_off32[nr] : 0, ncig = nc ? (size_t)cigar_off32[nc] : 0;
    int rc = 0;
    tc1 = std::chrono::steady_clock::now();
#define UPB(field, ptr, n) do { rc = dev_upload(c, b->allocs, (ptr), (n), (std::remove_const<std::remove_pointer<decltype(B.field)>::type>::type**)&B.field); if(rc) return fail(rc); } while(0)
    UPB(read_off, read_off32, (size_t)nr + 1); UPB(read_quals, in->read_quals + rb0, nbases);
    if(in->read_bases_packed && nr > 0) {
        // 4-bit packed bases (half the upload): read R of the sample starts at byte (base offset + R + 1) >> 1; unpacked on the device into the array the kernels read
        const int64_t R0 = in->first_read;
        if(R0 < 0) { c->err = "first_read is negative"; return fail(HLALA_E_ARG); }
        const int64_t p0 = (rb0 + R0 + 1) >> 1, p1 = ((in->read_off[nr] + R0 + (int64_t)nr + 1) >> 1) + 1;
        uint8_t* dPacked = nullptr; uint8_t* dBases = nullptr;
        rc = dev_upload(c, b->allocs, in->read_bases_packed + p0, (size_t)(p1 - p0), &dPacked); if(rc) return fail(rc);
        rc = dev_alloc(c, b->allocs, nbases, &dBases, false); if(rc) return fail(rc);
        hipLaunchKernelGGL(k_unpack_bases, dim3((unsigned)nr), dim3(64), 0, c->active, (const uint8_t*)dPacked, B.read_off, nr, (long long)rb0, (long long)R0, (long long)p0, dBases);
        { hipError_t el = hipGetLastError(); if(el != hipSuccess) { c->err = std::string("k_unpack_bases: ") + hipGetErrorString(el); return fail(HLALA_E_DEVICE); } }
        B.read_bases = dBases;
    } else {
        if(!in->read_bases && nbases > 0) { c->err = "neither read_bases nor read_bases_packed"; return fail(HLALA_E_ARG); }
        UPB(read_bases, in->read_bases + rb0, nbases);
    }
    UPB(chain_off, chain_off32, (size_t)nr + 1); UPB(read_primary, primary32, (size_t)nr);
    UPB(chain_read, chain_read, (size_t)nc);
    UPB(chain_contig, w_contig, (size_t)nc); UPB(chain_pos, w_pos, (size_t)nc); UPB(chain_offset, w_offset, (size_t)nc);
    UPB(chain_as, w_as, (size_t)nc); UPB(chain_reverse, w_rev, (size_t)nc);
    UPB(cigar_off, cigar_off32, (size_t)nc + 1); UPB(cigar, in->cigar + gb0, ncig);
#undef UPB
    rc = batch_create_tail(c, b, &tc2); if(rc) return fail(rc);
    if(hostTiming) { const auto tc3 = std::chrono::steady_clock::now(); auto ms = [](std::chrono::steady_clock::duration d) { return std::chrono::duration<double, std::milli>(d).count(); };
                     fprintf(stderr, "hlala_batch_create: checks and rebasing %.1f ms, allocations + uploads + kernels queued %.1f ms, waiting for the upload stream %.1f ms\n", ms(tc1 - tc0), ms(tc2 - tc1), ms(tc3 - tc2)); }
    *out = b;
    return HLALA_OK;
}

// output arrays of a batch that came through hlala_batch_create / _unpaired: allocated (pool) and zeroed on the stream of the stage call that needs them first, then the
// device descriptor is written again with their addresses
static int ensure_outputs(hlala_ctx* c, hlala_batch* b)
{
    if(b->outputs_ready) return HLALA_OK;
    int rc = batch_alloc_outputs(c, b); if(rc) return rc;
    HIP_TRY(c, hipMemcpyAsync(b->dB, &b->B, sizeof(DevBatch), hipMemcpyHostToDevice, c->active));
    b->outputs_ready = true;
    return HLALA_OK;
}

int hlala_batch_create_from_seeds(hlala_ctx* c, const hlala_seeds_in* in, hlala_batch** out)
{
    DEV_GUARD(c);
    if(!c || !in || !out) return HLALA_E_ARG;
    UploadScope upscope_(c);
    *out = nullptr;
    hlala_batch* b = new hlala_batch(); b->ctx = c; c->batches.insert(b);
    DevBatch& B = b->B;
    B.n_pairs = 0; B.n_reads = in->n_reads; B.n_chains = in->n_chains; B.stride = c->params.max_columns; B.from_seeds = 1;
    int nr = B.n_reads, nc = B.n_chains; int stride = B.stride;
    auto fail = [&](int rc) { hlala_batch_destroy(b); return rc; };
    size_t nbases = nr ? (size_t)in->read_off[nr] : 0;
    int rc = 0;
    rc = dev_upload(c, b->allocs, in->read_off, (size_t)nr + 1, (int**)&B.read_off); if(rc) return fail(rc);
    rc = dev_upload(c, b->allocs, in->read_bases, nbases, (uint8_t**)&B.read_bases); if(rc) return fail(rc);
    rc = dev_upload(c, b->allocs, in->read_quals, nbases, (uint8_t**)&B.read_quals); if(rc) return fail(rc);
    rc = dev_upload(c, b->allocs, in->chain_read, (size_t)nc, (int**)&B.chain_read); if(rc) return fail(rc);
    rc = dev_upload(c, b->allocs, in->chain_reverse, (size_t)nc, (uint8_t**)&B.chain_reverse); if(rc) return fail(rc);
    rc = batch_alloc_outputs(c, b); if(rc) return fail(rc);
    rc = dev_upload(c, b->allocs, &b->B, 1, &b->dB); if(rc) return fail(rc);
    // scatter the ragged seed columns into the fixed-stride layout
    std::vector<int> st((size_t)nc, HLALA_CHAIN_OK), ncols((size_t)nc), lev((size_t)nc * stride, -1), edg((size_t)nc * stride, -1);
    std::vector<uint8_t> g((size_t)nc * stride, 0), s((size_t)nc * stride, 0);
    for(int k = 0; k < nc; k++) {
        int n = in->col_off[k + 1] - in->col_off[k];
        if(in->chain_read[k] < 0 || in->chain_read[k] >= nr) { c->err = "chain_read out of range"; return fail(HLALA_E_ARG); }
        if(n > stride || n < 1) { st[k] = HLALA_CHAIN_ERR_COLUMNS; ncols[k] = 0; continue; }
        ncols[k] = n;
        for(int j = 0; j < n; j++) {
            size_t o = (size_t)k * stride + j; int i = in->col_off[k] + j;
            lev[o] = in->col_level[i]; edg[o] = in->col_edge[i]; g[o] = in->col_gchar[i]; s[o] = in->col_schar[i];
        }
    }
    HIP_TRY_F(c, hipMemcpyAsync(B.seed_status, st.data(), (size_t)nc * 4, hipMemcpyHostToDevice, c->active), fail);
    HIP_TRY_F(c, hipMemcpyAsync(B.seed_ncols, ncols.data(), (size_t)nc * 4, hipMemcpyHostToDevice, c->active), fail);
    HIP_TRY_F(c, hipMemcpyAsync(B.seed_begin, in->chain_seq_begin, (size_t)nc * 4, hipMemcpyHostToDevice, c->active), fail);
    HIP_TRY_F(c, hipMemcpyAsync(B.seed_end, in->chain_seq_end, (size_t)nc * 4, hipMemcpyHostToDevice, c->active), fail);
    HIP_TRY_F(c, hipMemcpyAsync(B.seed_level, lev.data(), lev.size() * 4, hipMemcpyHostToDevice, c->active), fail);
    HIP_TRY_F(c, hipMemcpyAsync(B.seed_edge, edg.data(), edg.size() * 4, hipMemcpyHostToDevice, c->active), fail);
    HIP_TRY_F(c, hipMemcpyAsync(B.seed_g, g.data(), g.size(), hipMemcpyHostToDevice, c->active), fail);
    HIP_TRY_F(c, hipMemcpyAsync(B.seed_s, s.data(), s.size(), hipMemcpyHostToDevice, c->active), fail);
    HIP_TRY_F(c, hipStreamSynchronize(c->active), fail);
    b->staged = 1; b->outputs_ready = true;
    *out = b;
    return HLALA_OK;
}

int hlala_batch_set_first_chain(hlala_batch* b, uint32_t first_chain)
{
    if(!b) return HLALA_E_ARG;
    b->first_chain = first_chain;
    return HLALA_OK;
}

void hlala_batch_destroy(hlala_batch* b)
{
    if(!b) return;
    hlala_ctx* c = b->ctx;
    DEV_GUARD(c);
    if(c) {
        if(b->tail_pooled) (void)flush_tail(c);       // (its pending classes run with whatever the pool holds; should that fail, the batch leaves the pool below)
        c->tail.erase(std::remove(c->tail.begin(), c->tail.end(), b), c->tail.end());
        c->batches.erase(b);
        if(b->side_inflight) (void)hipEventSynchronize(b->ev[EV_DONE]);
        if(b->mainValid) (void)hipEventSynchronize(b->ev[EV_MAIN]);       // nothing of this batch may still be running when its buffers are handed to the next one (readers and uploads return synchronised)
        for(void* p : b->allocs) pool_release(c, p);
    } else for(void* p : b->allocs) if(p) (void)hipFree(p);
    for(hipEvent_t e : b->ev) if(e) (void)hipEventDestroy(e);
    delete b;
}

static int check_launch(hlala_ctx* c, const char* what)
{
    hipError_t e = hipGetLastError();
    if(e != hipSuccess) { c->err = std::string(what) + ": " + hipGetErrorString(e); return HLALA_E_DEVICE; }
    return 0;
}

int hlala_project_chains(hlala_ctx* c, hlala_batch* b)
{
    DEV_GUARD(c);
    if(!c || !b) return HLALA_E_ARG;
    { int rj = join_side(c, b); if(rj) return rj; }
    if(b->B.from_seeds) { c->err = "batch was created from seeds: stage A not available"; return HLALA_E_STATE; }
    { int re = batch_events(c, b); if(re) return re; }
    { int ro = ensure_outputs(c, b); if(ro) return ro; }
    DevBatch& B = b->B;
    HIP_TRY(c, hipMemsetAsync(B.work_counter, 0, WC_N * sizeof(int), c->active));
    HIP_TRY(c, hipMemsetAsync(B.counters, 0, 32 * sizeof(u64), c->active));
    HIP_TRY(c, hipEventRecord(b->ev[EV_PROJECT_BEGIN], c->active));
    if(B.n_chains > 0) {
        int threads = 256, blocks = (B.n_reads + threads - 1) / threads;
        // (the filters and the position order of a batch ran when it was created, hlala_batch_create: they read inputs only)
        if(!b->prepared && B.order_hist) HIP_TRY(c, hipMemsetAsync(B.order_hist, 0, ((size_t)B.order_nb + 1) * sizeof(int), c->active));
        if(!b->prepared) hipLaunchKernelGGL(k_filter_chains, dim3(blocks), dim3(threads), 0, c->active, c->dG, b->dB, c->d_contig_off, c->d_contig_level);
        if(!b->prepared && B.order_hist) {
            // chains into position order (kernel_order.hip): every later kernel that walks the graph takes them from B.chain_order
            hipLaunchKernelGGL(k_order_scan, dim3(1), dim3(ORDER_SCAN_THREADS), 0, c->active, B.order_hist, B.order_nb);
            hipLaunchKernelGGL(k_order_scatter, dim3((B.n_chains + 255) / 256), dim3(256), 0, c->active, b->dB);
            int rco = check_launch(c, "k_order_scatter"); if(rco) return rco;
        }
        int grid = B.n_chains < c->proj_grid ? B.n_chains : c->proj_grid;
        if(c->proj_long_slabs)
            hipLaunchKernelGGL((k_project_chains<ProjLdsLong>), dim3(grid), dim3(64), 0, c->active, c->G, b->B, c->dG, b->dB, c->d_contig_off, c->d_contig_seq, c->d_contig_level,
                               c->proj_slabs, c->proj_slab_bytes, c->proj_long_slabs, c->proj_long_slab_bytes, 0);
        else
            if(c->params.max_columns <= PROJ_CAP_SHORT)
                hipLaunchKernelGGL((k_project_chains<ProjLdsShort>), dim3(grid), dim3(64), 0, c->active, c->G, b->B, c->dG, b->dB, c->d_contig_off, c->d_contig_seq, c->d_contig_level,
                                   c->proj_slabs, c->proj_slab_bytes, (char*)nullptr, (size_t)0, c->rethread_slabs ? 1 : 0);
            else
                hipLaunchKernelGGL((k_project_chains<ProjLds>), dim3(grid), dim3(64), 0, c->active, c->G, b->B, c->dG, b->dB, c->d_contig_off, c->d_contig_seq, c->d_contig_level,
                               c->proj_slabs, c->proj_slab_bytes, (char*)nullptr, (size_t)0, c->rethread_slabs ? 1 : 0);
        int rc = check_launch(c, "k_project_chains"); if(rc) return rc;
        if(c->rethread_slabs) {
            hipLaunchKernelGGL(k_rethread_chains, dim3(c->rethread_grid), dim3(64), 0, c->active, c->dG, b->dB, c->rethread_slabs, c->rethread_slab_bytes);
            rc = check_launch(c, "k_rethread_chains"); if(rc) return rc;
        }
    }
    HIP_TRY(c, hipEventRecord(b->ev[EV_PROJECT_END], c->active));
    b->staged |= 1;
    return mark_main(c, b);
}

#define STEP(call) do { int rc_ = (call); if(rc_) return rc_; } while(0)
// Extension and pairing are written as STEPS -- each queues one thing on one stream; without a stream argument, on the main stream (c->active) -- and as five SCHEDULES,
// plain sequences of steps: the stage calls, the three fused alignments of hlala_align_batch (default, HLALA_SIDE_AFTER_PAIR=1, tail pool) and flush_tail.
// Fused (hlala_align_batch on a paired batch).  The 16- / 32- / 64-lane classes hold all but a few percent of the DP calls; the rest (wide, broad, large, in-memory) are
// few, long calls that cannot fill the chip.  Fused, they run on the side stream, followed there by a second stitch / pairing pass over the pairs that own them
// (pair_deferred, set by the DP kernels when they hand an item to one of these classes), while the main stream stitches and pairs everything else and is then free for
// the caller's next batch.  EV_DONE orders later users of the batch behind the side work.
static bool fusable(const hlala_batch* b) { const DevBatch& B = b->B; return !(B.unpaired || B.from_seeds || B.n_pairs <= 0 || B.n_chains <= 0); }
// start of every extension: the stage's counters, then (a batch with chains) the DP items and their lists
static int dp_prepare(hlala_ctx* c, hlala_batch* b)
{
    DevBatch& B = b->B;
    b->side_used = false; b->side_pending = false;
    if(B.n_pairs > 0) HIP_TRY(c, hipMemsetAsync(B.pair_deferred, 0, (size_t)B.n_pairs, c->active));
    HIP_TRY(c, hipMemsetAsync(B.work_counter + 1, 0, sizeof(int), c->active));
    HIP_TRY(c, hipMemsetAsync(B.work_counter + 4, 0, (WC_N - 4) * sizeof(int), c->active));       // [4..6] jump-free lists, [7..] stitch, DP items, retry lists, band / fail-over lists
    if(B.from_seeds) HIP_TRY(c, hipMemsetAsync(B.counters, 0, 32 * sizeof(u64), c->active));
    HIP_TRY(c, hipEventRecord(b->ev[EV_EXTEND_BEGIN], c->active));
    if(B.n_chains <= 0) return HLALA_OK;
    DpItem* items = (DpItem*)B.dp_items;
    HIP_TRY(c, hipMemsetAsync(B.dp_alias_head, 0xFF, (size_t)2 * B.n_chains * sizeof(int), c->active));       // -1: k_dp_items links the duplicates of a DP to it
    HIP_TRY(c, hipMemsetAsync(B.dp_alias_next, 0xFF, (size_t)2 * B.n_chains * sizeof(int), c->active));
    // items, then the fourteen dense lists of the first classes (three band lists, left / right each; jump-free and general, long / short per direction) in position order: counts per block, their scan, the slots
    HIP_TRY(c, hipMemsetAsync(B.dp_blk, 0, ((size_t)DPL_N * B.dp_nblk + 1) * sizeof(int), c->active));
    hipLaunchKernelGGL(k_dp_items, dim3(B.dp_nblk), dim3(256), 0, c->active, c->G, b->B, items);
    STEP(check_launch(c, "k_dp_items"));
    hipLaunchKernelGGL(k_order_scan, dim3(1), dim3(ORDER_SCAN_THREADS), 0, c->active, B.dp_blk, DPL_N * B.dp_nblk + 1);
    hipLaunchKernelGGL(k_dp_lists, dim3(B.dp_nblk), dim3(256), 0, c->active, b->B, (const DpItem*)items);
    return check_launch(c, "k_dp_lists");
}
// calls on linear stretches of the graph first: anti-diagonals in registers, four calls per wavefront (kernel_dp_band.hip); what it cannot finish is on the
// fail-over list the general 16-lane instantiation draws after its own
static int dp_band(hlala_ctx* c, hlala_batch* b)
{
    DevBatch& B = b->B;
    b->band_used = c->band_grid > 0;
    if(!b->band_used) return HLALA_OK;
    const DpItem* items = (const DpItem*)B.dp_items; const u32 seed = c->params.rng_seed + 2u * b->first_chain;
    HIP_TRY(c, hipEventRecord(b->ev[EV_DP_BAND_BEGIN], c->active));
    hipLaunchKernelGGL((k_dp_band<16>), dim3(c->band_grid), dim3(64), 0, c->active, c->G, b->B, items, seed, (const uint8_t*)B.read_bases);
    hipLaunchKernelGGL((k_dp_band<32>), dim3(c->band_grid), dim3(64), 0, c->active, c->G, b->B, items, seed, (const uint8_t*)B.read_bases);
    hipLaunchKernelGGL((k_dp_band<64>), dim3(c->band_grid), dim3(64), 0, c->active, c->G, b->B, items, seed, (const uint8_t*)B.read_bases);
    STEP(check_launch(c, "k_dp_band"));
    HIP_TRY(c, hipEventRecord(b->ev[EV_DP_BAND_END], c->active)); return HLALA_OK;
}
// The DP classes `first` .. `last` on `ws`, for the n batches of `bs`: one batch, or (tiers from DP_POOL_TIER on only) the batches of a tail pool in one launch per class.
// Every DP item first runs in the 16-lane class; the item count lives on the device, idle groups leave at once.  Items that outgrew it: two DPs per wave, then one wave
// per DP, then the classes with wider frontiers (fewer blocks per CU).  Each class is timed with its own pair of events on the stream it runs on; EV_DP_BEGIN /
// EV_DP_CLASS0_END / EV_DP_CLASS2_END mark the start of the 16-lane class, its end and the end of the 64-lane class on the main stream.
static int dp_classes(hlala_ctx* c, hlala_batch* const* bs, int n, int first, int last, hipStream_t ws)
{
    const DpPoolArgs noPool{};       // classes before DP_POOL_TIER take the batch of their plain arguments, the later ones a list of batches
    DpPoolArgs pool{}; pool.n = n; hlala_batch* b0 = bs[0];
    for(int i = 0; i < n; i++) { const hlala_batch* b = bs[i]; pool.seed[i] = c->params.rng_seed + 2u * b->first_chain; pool.B[i] = b->dB; pool.items[i] = (const DpItem*)b->B.dp_items; pool.bases[i] = (const uint8_t*)b->B.read_bases; }
    for(int tier = first; tier <= last; tier++) {
        const DpClass& k = c->dp[tier];
        if(tier == 0) HIP_TRY(c, hipEventRecord(b0->ev[EV_DP_BEGIN], c->active));
        for(int i = 0; i < n; i++) HIP_TRY(c, hipEventRecord(bs[i]->ev[EV_DP_CLASS_BEGIN + tier], ws));
        if(tier == 0) {
            // the calls that meet no gap-path jump in the instantiation without the early-cell machinery, then the others (same slabs: one after the other)
            c->dp_jf.launch(c, c->dp_jf, ws, b0, noPool);
            STEP(check_launch(c, c->dp_jf.name));
            HIP_TRY(c, hipEventRecord(b0->ev[EV_DP_JUMP_FREE_END], ws));
        }
        k.launch(c, k, ws, b0, tier < DP_POOL_TIER ? noPool : pool);
        STEP(check_launch(c, k.name));
        for(int i = 0; i < n; i++) HIP_TRY(c, hipEventRecord(bs[i]->ev[EV_DP_CLASS_END + tier], ws));
        if(tier == 0 || tier == 2) HIP_TRY(c, hipEventRecord(b0->ev[tier == 0 ? EV_DP_CLASS0_END : EV_DP_CLASS2_END], c->active));
    }
    return HLALA_OK;
}
// the side stream goes on from here: whatever the batch has queued on the main stream so far lies in front of its side-stream work
static int side_fork(hlala_ctx* c, hlala_batch* b)
{
    HIP_TRY(c, hipEventRecord(b->ev[EV_SIDE_FORK], c->active)); HIP_TRY(c, hipStreamWaitEvent(c->side, b->ev[EV_SIDE_FORK], 0));
    HIP_TRY(c, hipEventRecord(b->ev[EV_SIDE_BEGIN], c->side)); b->side_used = true;
    return HLALA_OK;
}
// The end of a sequence of side-stream work of `b`, and the only place that says so: EV_DONE for whoever touches the batch next, evSideTail for a later launch on the
// main stream of the classes whose slabs the side stream uses (hlala_ctx::dp).  Every sequence that queued anything on the side stream ends here.
static int side_mark(hlala_ctx* c, hlala_batch* b)
{
    HIP_TRY(c, hipEventRecord(b->ev[EV_DONE], c->side)); b->side_inflight = true;
    HIP_TRY(c, hipEventRecord(c->evSideTail, c->side)); c->sideTailValid = true;
    return HLALA_OK;
}
// first stitch pass (work counter 7).  mode 0: every chain; 1: all but the chains of the deferred pairs, which stitch_side takes behind their DP classes
static int stitch_main(hlala_ctx* c, hlala_batch* b, int mode)
{
    const int sgrid = b->B.n_chains < c->stitch_grid ? b->B.n_chains : c->stitch_grid;
    hipLaunchKernelGGL(k_stitch_chains, dim3(sgrid), dim3(64), 0, c->active, c->G, c->dT, b->B, (const uint8_t*)b->B.pair_deferred, mode, c->stitch_draw, c->stitch_by_row);
    return check_launch(c, "k_stitch_chains");
}
// second stitch pass, on the side stream: the chains of the deferred pairs (work counter 36)
static int stitch_side(hlala_ctx* c, hlala_batch* b)
{
    const int pgrid = (b->B.n_pairs + 63) / 64, cap = c->stitch_grid / 20;       // it sweeps the pairs' flags, 64 per wave and round: one wave per CU finds room beside the next batch's persistent kernels
    hipLaunchKernelGGL(k_stitch_chains, dim3(pgrid < cap ? (pgrid > 0 ? pgrid : 1) : cap), dim3(64), 0, c->side, c->G, c->dT, b->B, (const uint8_t*)b->B.pair_deferred, 2, 0, 0);
    return check_launch(c, "k_stitch_chains (side)");
}
static int extend_end(hlala_ctx* c, hlala_batch* b) { HIP_TRY(c, hipEventRecord(b->ev[EV_EXTEND_END], c->active)); b->staged |= 2; return mark_main(c, b); }
static int pair_begin(hlala_ctx* c, hlala_batch* b) { HIP_TRY(c, hipMemsetAsync(b->B.work_counter + 2, 0, sizeof(int), c->active)); HIP_TRY(c, hipEventRecord(b->ev[EV_PAIR_BEGIN], c->active)); return HLALA_OK; }
// One pairing pass on `st`.  mode 0: every pair (a stage call); 1: all but the deferred pairs; 2: those (the side stream's pass, behind stitch_side).  k_pair_chains
// finishes the pairs with one combination and lists the others, k_pair_multi<., false / true> runs the two lists (kernel_pair.hip); the main- and the side-stream pass
// have their own work counter (2 / 37), lists, list counters and combination scratch.  With the overflow class on (hlala_set_pair_overflow) k_pair_chains lists the
// pairs that only a capacity keeps from these kernels in a third list of the pass, and k_pair_overflow runs it behind the general class, on the pass's own slabs.
static int pair_pass(hlala_ctx* c, hlala_batch* b, hipStream_t st, int mode)
{
    DevBatch& B = b->B;
    const int grid = B.n_pairs < c->pair_grid ? B.n_pairs : c->pair_grid, lean = B.n_pairs < c->pair_lean_grid ? B.n_pairs : c->pair_lean_grid;
    const int pass = st == c->side ? 1 : 0, counterIdx = pass ? 37 : 2, multiBase = WC_PAIR_MULTI + 4 * pass;
    int* multiList = B.pair_multi + (size_t)pass * 2 * (size_t)B.n_pairs; double* scratch = c->pair_scratch + (pass ? (size_t)c->pair_grid * PAIR_COMB : 0);
    // (the lists' counters are among those the extension stage clears; a pairing stage called again on its own clears them here.  Not on the side stream: a fill
    //  kernel queued there waits 13-36 ms for a wave slot beside the persistent kernels -- profiles/r06_experiments.txt)
    if(mode == 0) HIP_TRY(c, hipMemsetAsync(B.work_counter + multiBase, 0, 4 * sizeof(int), st));
    if(mode == 0) HIP_TRY(c, hipMemsetAsync(B.work_counter + WC_PAIR_OVER, 0, 8 * sizeof(int), st));          // (both passes': hlala_batch_get_pair_overflow sums them)
    const int ovBase = WC_PAIR_OVER + 4 * pass;
    int* ovList = c->pair_over_slabs ? multiList + (size_t)4 * (size_t)B.n_pairs : nullptr;          // (k_pair_chains: at that distance from the pass's lists, as ovBase from multiBase)
    const int g0 = mode == 2 ? (grid < c->pair_grid / 5 ? grid : c->pair_grid / 5) : grid, g1 = grid < c->pair_grid / 5 ? grid : c->pair_grid / 5;      // (the second pass and the general class hold a few thousand pairs at most)
    const auto chains = ovList ? (B.unpaired ? k_pair_chains<true, true> : k_pair_chains<false, true>) : (B.unpaired ? k_pair_chains<true, false> : k_pair_chains<false, false>);
    const auto multi = B.unpaired ? k_pair_multi<true, false> : k_pair_multi<false, false>, multiBig = B.unpaired ? k_pair_multi<true, true> : k_pair_multi<false, true>;
    hipLaunchKernelGGL(chains, dim3(lean), dim3(64), 0, st, c->dG, c->dT, b->dB, (const uint8_t*)B.pair_deferred, mode, counterIdx, multiList, multiBase);
    hipLaunchKernelGGL(multi, dim3(g0), dim3(64), 0, st, c->G, b->B, c->dG, c->dT, b->dB, (const int*)multiList, multiBase, scratch);
    hipLaunchKernelGGL(multiBig, dim3(g1), dim3(64), 0, st, c->G, b->B, c->dG, c->dT, b->dB, (const int*)multiList, multiBase, scratch);
    if(ovList) {
        const auto over = B.unpaired ? k_pair_overflow<true> : k_pair_overflow<false>;
        hipLaunchKernelGGL(over, dim3(PAIR_OVER_WAVES), dim3(64), 0, st, c->dG, c->dT, b->dB, (const int*)ovList, ovBase,
                           c->pair_over_slabs + (size_t)pass * PAIR_OVER_WAVES * (size_t)c->pair_over_slab_bytes, c->pair_over_slab_bytes);
    }
    return check_launch(c, "k_pair_chains / k_pair_multi");
}
// second pairing pass, behind the side-stream classes and the second stitch pass: the deferred pairs
static int pair_side(hlala_ctx* c, hlala_batch* b)
{
    STEP(pair_pass(c, b, c->side, 2));
    HIP_TRY(c, hipEventRecord(b->ev[EV_SIDE_END], c->side)); b->side_pending = false;
    return HLALA_OK;
}
static int pair_end(hlala_ctx* c, hlala_batch* b) { HIP_TRY(c, hipEventRecord(b->ev[EV_PAIR_END], c->active)); b->staged |= 4; return mark_main(c, b); }

// In the schedules below one line = consecutive steps on ONE stream (named at its end), so the lines also give the order in which the host alternates between the streams.
// Schedule 1, the stage calls: everything on the main stream (unpaired, from-seeds and empty batches take them from hlala_align_batch as well).  The slabs of the
// classes from DP_SIDE_TIER on may still be in use on the side stream (hlala_ctx::dp): pending pooled launches are queued first, and the main stream waits for the end
// of the side stream's queue in front of the first of these classes.
int hlala_extend_chains(hlala_ctx* c, hlala_batch* b)
{
    DEV_GUARD(c);
    if(!c || !b) return HLALA_E_ARG;
    if(!(b->staged & 1)) { c->err = "hlala_extend_chains before seed chains exist"; return HLALA_E_STATE; }
    STEP(flush_tail(c));                                                                                                        // side
    STEP(join_side(c, b)); STEP(batch_events(c, b)); STEP(dp_prepare(c, b));                                                    // main, as all below
    if(b->B.n_chains > 0) {
        STEP(dp_band(c, b)); STEP(dp_classes(c, &b, 1, 0, DP_SIDE_TIER - 1, c->active));
        if(c->sideTailValid) HIP_TRY(c, hipStreamWaitEvent(c->stream, c->evSideTail, 0));
        STEP(dp_classes(c, &b, 1, DP_SIDE_TIER, DP_LAST_TIER, c->active)); HIP_TRY(c, hipEventRecord(b->ev[EV_DP_END], c->active));
        STEP(stitch_main(c, b, 0));
    }
    return extend_end(c, b);
}
int hlala_pair_chains(hlala_ctx* c, hlala_batch* b)
{
    DEV_GUARD(c);
    if(!c || !b) return HLALA_E_ARG;
    if(b->B.from_seeds) { c->err = "batch was created from seeds: stage C not available"; return HLALA_E_STATE; }
    if(!(b->staged & 2)) { c->err = "hlala_pair_chains before hlala_extend_chains"; return HLALA_E_STATE; }
    STEP(batch_events(c, b)); STEP(join_side(c, b));
    b->side_pending = false;       // (still set only after a fused alignment that failed between its stages: its chains are stitched, this pass takes every pair)
    STEP(pair_begin(c, b));
    if(b->B.n_pairs > 0) STEP(pair_pass(c, b, c->active, 0));
    return pair_end(c, b);
}
// Schedule 2, the default fused alignment: the side stream's classes are forked off as soon as the 64-lane class is queued, and its whole extension part is queued
// before the main stream's stitch pass.
static int align_default(hlala_ctx* c, hlala_batch* b)
{
    STEP(dp_prepare(c, b)); STEP(dp_band(c, b)); STEP(dp_classes(c, &b, 1, 0, DP_SIDE_TIER - 1, c->active)); STEP(side_fork(c, b));        // main
    STEP(dp_classes(c, &b, 1, DP_SIDE_TIER, DP_LAST_TIER, c->side)); STEP(stitch_side(c, b)); STEP(side_mark(c, b));                       // side
    b->side_pending = true;
    STEP(stitch_main(c, b, 1)); STEP(extend_end(c, b)); STEP(pair_begin(c, b)); STEP(pair_pass(c, b, c->active, 1));                       // main
    STEP(pair_side(c, b)); STEP(side_mark(c, b));                                                                                          // side
    return pair_end(c, b);                                                                                                                 // main
}
// Schedule 3, HLALA_SIDE_AFTER_PAIR=1: the main stream's part of the batch first -- DP classes up to the 64-lane one, stitch, pairing --, then the side stream's classes
// and its second stitch / pairing pass.  k_pair_chains is a short, latency-bound kernel that needs 6 KB of LDS per wavefront, and beside the wide class (seven blocks of
// 22 KB per CU: 154 of a CU's 160 KB) hardly a block of it fits: 20.9 ms for a pairing pass that takes 4.1 ms alone (profiles/r05_experiments.txt, 19).  Not the
// default: the next batch's projection (11.7 KB per block) then meets the wide class instead.
static int align_side_after_pair(hlala_ctx* c, hlala_batch* b)
{
    STEP(dp_prepare(c, b)); STEP(dp_band(c, b)); STEP(dp_classes(c, &b, 1, 0, DP_SIDE_TIER - 1, c->active));                               // main, down to side_fork
    b->side_pending = true;
    STEP(stitch_main(c, b, 1)); STEP(extend_end(c, b)); STEP(pair_begin(c, b)); STEP(pair_pass(c, b, c->active, 1)); STEP(pair_end(c, b));
    STEP(side_fork(c, b));
    STEP(dp_classes(c, &b, 1, DP_SIDE_TIER, DP_LAST_TIER, c->side)); STEP(stitch_side(c, b)); STEP(side_mark(c, b));                       // side
    STEP(pair_side(c, b)); return side_mark(c, b);
}
// The tail pool.  The broad, large and in-memory DP classes hold 0.07 % of a batch's DP calls and took 100 ms of side stream per batch: their cost is the latency of
// their slowest calls, paid per launch, while their blocks hold most of every CU's LDS beside the next batch's kernels.  With hlala_set_tail_pool(ctx, k) a fused
// alignment runs its main-stream part and its wide class as before and leaves those three classes PENDING; the k-th pending batch (or hlala_flush, or any call that
// reads or re-runs a pending batch, or a non-fused extension stage on the context) launches each of them once over all pending batches (k_dp: DpPoolArgs), then the
// second stitch / pairing pass of every batch.  Results do not depend on k (tests/test_graph_m.py).
// Schedule 4, the pooled alignment: as the default one up to the classes before DP_POOL_TIER; the batch then waits in c->tail with its second passes pending.
static int align_pooled(hlala_ctx* c, hlala_batch* b)
{
    STEP(dp_prepare(c, b)); STEP(dp_band(c, b)); STEP(dp_classes(c, &b, 1, 0, DP_SIDE_TIER - 1, c->active)); STEP(side_fork(c, b));        // main
    STEP(dp_classes(c, &b, 1, DP_SIDE_TIER, DP_POOL_TIER - 1, c->side)); STEP(side_mark(c, b));                                            // side
    b->side_pending = true;
    STEP(stitch_main(c, b, 1)); STEP(extend_end(c, b)); STEP(pair_begin(c, b)); STEP(pair_pass(c, b, c->active, 1)); STEP(pair_end(c, b)); // main
    c->tail.push_back(b); b->tail_pooled = true;
    return (int)c->tail.size() >= c->tail_pool_k ? flush_tail(c) : HLALA_OK;
}
// Schedule 5: the pooled classes once for all pending batches, then every batch's second passes.  All on the side stream, behind the batches' wide classes.
static int flush_tail(hlala_ctx* c)
{
    if(c->tail.empty()) return HLALA_OK;
    DEV_GUARD(c);
    std::vector<hlala_batch*> pool; pool.swap(c->tail);
    for(hlala_batch* b : pool) b->tail_pooled = false;           // (whatever happens below, nobody waits for this flush again)
    STEP(dp_classes(c, pool.data(), (int)pool.size(), DP_POOL_TIER, DP_LAST_TIER, c->side));
    for(hlala_batch* b : pool) { STEP(stitch_side(c, b)); STEP(side_mark(c, b)); STEP(pair_side(c, b)); STEP(side_mark(c, b)); }
    return HLALA_OK;
}

int hlala_set_tail_pool(hlala_ctx* c, int k)
{
    if(!c || k < 1 || k > DP_POOL_MAX) { if(c) c->err = "hlala_set_tail_pool: k must be 1 .. " + std::to_string(DP_POOL_MAX); return HLALA_E_ARG; }
    if(k < (int)c->tail.size() || k == 1) { int rf = flush_tail(c); if(rf) return rf; }
    c->tail_pool_k = k;
    return HLALA_OK;
}
int hlala_flush(hlala_ctx* c) { return c ? flush_tail(c) : HLALA_E_ARG; }

// The overflow class of the pairing stage.  The slabs belong to the context; the pairing passes of the main and of the side stream use one half each.
int hlala_set_pair_overflow(hlala_ctx* c, int64_t scratch_bytes)
{
    if(!c) return HLALA_E_ARG;
    if(scratch_bytes < 0) { c->err = "hlala_set_pair_overflow: scratch_bytes must not be negative"; return HLALA_E_ARG; }
    DEV_GUARD(c);
    STEP(flush_tail(c));
    if(scratch_bytes == c->pair_over_scratch) return HLALA_OK;
    // nothing queued may still use the slabs that go away
    HIP_TRY(c, hipStreamSynchronize(c->stream)); HIP_TRY(c, hipStreamSynchronize(c->side));
    if(c->pair_over_slabs) { (void)hipFree(c->pair_over_slabs); c->pair_over_slabs = nullptr; }
    c->pair_over_scratch = 0; c->pair_over_slab_bytes = 0;
    if(scratch_bytes == 0) return HLALA_OK;
    const long long slab = (scratch_bytes / HLALA_PAIR_OVERFLOW_WAVES) & ~15ll;
    char* p = nullptr;
    if(device_malloc_retry(c->device, c, (void**)&p, (size_t)(slab > 0 ? slab : 16) * HLALA_PAIR_OVERFLOW_WAVES) != hipSuccess) { c->err = "hipMalloc(pair overflow slabs) failed"; return HLALA_E_DEVICE; }
    c->pair_over_slabs = p; c->pair_over_scratch = scratch_bytes; c->pair_over_slab_bytes = slab;
    return HLALA_OK;
}
int hlala_get_pair_overflow(hlala_ctx* c, int64_t* scratch_bytes, int64_t* slab_bytes)
{
    if(!c) return HLALA_E_ARG;
    if(scratch_bytes) *scratch_bytes = c->pair_over_scratch;
    if(slab_bytes) *slab_bytes = c->pair_over_slab_bytes;
    return HLALA_OK;
}
int64_t hlala_pair_overflow_need(int64_t n1, int64_t n2, int32_t max_columns, int unpaired)
{
    if(n1 < 0) n1 = 0; if(n2 < 0) n2 = 0; if(max_columns < 0) max_columns = 0;
    return pair_overflow_need(n1, n2, max_columns, unpaired != 0);
}
int hlala_batch_get_pair_overflow(hlala_ctx* c, hlala_batch* b, int64_t out[3])
{
    DEV_GUARD(c);
    ReaderScope rscope_(c, b); if(rscope_.rc) return rscope_.rc;
    if(!c || !b || !out) return HLALA_E_ARG;
    out[0] = out[1] = out[2] = 0;
    if(!b->outputs_ready || !(b->staged & 4)) return HLALA_OK;
    int wc[8];
    HIP_TRY(c, hipMemcpyAsync(wc, b->B.work_counter + WC_PAIR_OVER, sizeof(wc), hipMemcpyDeviceToHost, c->active)); HIP_TRY(c, hipStreamSynchronize(c->active));
    for(int pass = 0; pass < 2; pass++) { out[0] += wc[4 * pass]; out[1] += wc[4 * pass + 2]; out[2] += wc[4 * pass + 3]; }
    return HLALA_OK;
}

int hlala_align_batch(hlala_ctx* c, hlala_batch* b)
{
    int rc = hlala_project_chains(c, b); if(rc) return rc;
    if(!fusable(b)) { rc = hlala_extend_chains(c, b); return rc ? rc : hlala_pair_chains(c, b); }
    DEV_GUARD(c);
    if(c->tail_pool_k > 1 && DP_POOL_TIER > DP_SIDE_TIER) return align_pooled(c, b);
    return c->side_after_pair ? align_side_after_pair(c, b) : align_default(c, b);
}

int hlala_batch_get_chains(hlala_ctx* c, hlala_batch* b, int stage, hlala_chains_out* o)
{
    DEV_GUARD(c);
    ReaderScope rscope_(c, b); if(rscope_.rc) return rscope_.rc;
    if(!c || !b || !o) return HLALA_E_ARG;
    DevBatch& B = b->B;
    size_t nc = (size_t)B.n_chains, cs = nc * (size_t)B.stride;
    int rc = 0;
    // the column arrays hold a row per chain that passed the filters (batch.h: chain_row); the caller's arrays hold one per chain: rows are copied to their chains'
    // places on the host (chains without a row: zeros)
    std::vector<int> rowOf;
    if(B.chain_row && nc > 0) { rowOf.resize(nc); HIP_TRY(c, hipMemcpyAsync(rowOf.data(), B.chain_row, nc * sizeof(int), hipMemcpyDeviceToHost, c->active)); HIP_TRY(c, hipStreamSynchronize(c->active)); }
    auto dlRows = [&](auto* host, const auto* dev) -> int {
        typedef typename std::remove_pointer<decltype(host)>::type T;
        if(!host || !cs) return 0;
        if(rowOf.empty()) return dl(c, host, dev, cs);
        const size_t stride = (size_t)B.stride, nrows = (size_t)B.n_rows;
        std::vector<T> tmp(nrows * stride + 1);
        if(nrows) { HIP_TRY(c, hipMemcpyAsync(tmp.data(), dev, nrows * stride * sizeof(T), hipMemcpyDeviceToHost, c->active)); HIP_TRY(c, hipStreamSynchronize(c->active)); }
        for(size_t k = 0; k < nc; k++) {
            const int r = rowOf[k];
            if(r >= 0 && (size_t)r < nrows) memcpy(host + k * stride, tmp.data() + (size_t)r * stride, stride * sizeof(T)); else memset(host + k * stride, 0, stride * sizeof(T));
        }
        return 0;
    };
    if(stage == 0) {
        if(!(b->staged & 1)) { c->err = "seed chains not computed"; return HLALA_E_STATE; }
        if((rc = dl(c, o->status, B.seed_status, nc))) return rc; if((rc = dl(c, o->n_cols, B.seed_ncols, nc))) return rc;
        if((rc = dl(c, o->seq_begin, B.seed_begin, nc))) return rc; if((rc = dl(c, o->seq_end, B.seed_end, nc))) return rc;
        if((rc = dl(c, o->removed_cols, B.seed_removed, nc))) return rc;
        if((rc = dlRows(o->col_level, (const int*)B.seed_level))) return rc; if((rc = dlRows(o->col_edge, (const int*)B.seed_edge))) return rc;
        if((rc = dlRows(o->col_gchar, (const uint8_t*)B.seed_g))) return rc; if((rc = dlRows(o->col_schar, (const uint8_t*)B.seed_s))) return rc;
        HIP_TRY(c, hipStreamSynchronize(c->active));
        if(o->col_fromseed) memset(o->col_fromseed, 1, cs);
        if(o->ll) memset(o->ll, 0, nc * 8);
        if(o->dp_iters) memset(o->dp_iters, 0, nc * 8);
        if(o->dp_score) memset(o->dp_score, 0, nc * 8);
    } else if(stage == 1) {
        if(!(b->staged & 2)) { c->err = "extended chains not computed"; return HLALA_E_STATE; }
        if((rc = dl(c, o->status, B.ext_status, nc))) return rc; if((rc = dl(c, o->n_cols, B.ext_ncols, nc))) return rc;
        if((rc = dl(c, o->seq_begin, B.ext_begin, nc))) return rc; if((rc = dl(c, o->seq_end, B.ext_end, nc))) return rc;
        if((rc = dl(c, o->removed_cols, B.seed_removed, nc))) return rc; if((rc = dl(c, o->ll, B.ext_ll, nc))) return rc;
        if((rc = dl(c, o->dp_iters, B.dp_iters, 2 * nc))) return rc; if((rc = dl(c, o->dp_score, B.dp_score, 2 * nc))) return rc;
        if((rc = dlRows(o->col_level, (const int*)B.ext_level))) return rc; if((rc = dlRows(o->col_edge, (const int*)B.ext_edge))) return rc;
        if((rc = dlRows(o->col_gchar, (const uint8_t*)B.ext_g))) return rc; if((rc = dlRows(o->col_schar, (const uint8_t*)B.ext_s))) return rc;
        if((rc = dlRows(o->col_fromseed, (const uint8_t*)B.ext_fromseed))) return rc;
        HIP_TRY(c, hipStreamSynchronize(c->active));
    } else { c->err = "stage must be 0 or 1"; return HLALA_E_ARG; }
    return HLALA_OK;
}

int hlala_batch_get_pairs(hlala_ctx* c, hlala_batch* b, hlala_pairs_out* o)
{
    DEV_GUARD(c);
    ReaderScope rscope_(c, b); if(rscope_.rc) return rscope_.rc;
    if(!c || !b || !o) return HLALA_E_ARG;
    if(!(b->staged & 4)) { c->err = "pairs not computed"; return HLALA_E_STATE; }
    DevBatch& B = b->B;
    size_t np = (size_t)B.n_pairs, nr = (size_t)B.n_reads, stride = (size_t)B.stride;
    int rc = 0;
    if((rc = dl(c, o->best_chain, B.best_chain, nr))) return rc;
    if((rc = dl(c, o->pair_status, B.pair_status, np))) return rc; if((rc = dl(c, o->n_combinations, B.n_comb, np))) return rc;
    if((rc = dl(c, o->pair_ll, B.pair_ll, np))) return rc; if((rc = dl(c, o->pair_mapq, B.pair_mapq, np))) return rc;
    if((rc = dl(c, o->mate_mapq, B.mate_mapq, nr))) return rc; if((rc = dl(c, o->strands_valid, B.strands_valid, np))) return rc;
    if((rc = dl(c, o->col_mapq, B.sel_mapq, nr * stride))) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->active));
    // columns of the selected chains: gathered on the device into read-major staging rows, one bulk copy per array and chunk
    // (columns beyond n_cols come back as zero)
    const bool wantCols = o->n_cols || o->col_level || o->col_edge || o->col_gchar || o->col_schar || o->col_fromseed;
    if(wantCols && nr > 0) {
        const size_t CH = nr < 65536 ? nr : 65536;
        std::vector<void*> tmp;
        auto done = [&](int r_) { for(void* p : tmp) pool_release(c, p); return r_; };
        int* dN = nullptr; int* dL = nullptr; int* dE = nullptr; uint8_t* dG = nullptr; uint8_t* dS = nullptr; uint8_t* dF = nullptr;
        if((rc = dev_alloc(c, tmp, CH, &dN, false)) || (rc = dev_alloc(c, tmp, CH * stride, &dL, false)) || (rc = dev_alloc(c, tmp, CH * stride, &dE, false)) ||
           (rc = dev_alloc(c, tmp, CH * stride, &dG, false)) || (rc = dev_alloc(c, tmp, CH * stride, &dS, false)) || (rc = dev_alloc(c, tmp, CH * stride, &dF, false))) return done(rc);
        for(size_t r0 = 0; r0 < nr; r0 += CH) {
            const size_t rows = nr - r0 < CH ? nr - r0 : CH;
            hipLaunchKernelGGL(k_gather_selected, dim3((unsigned)rows), dim3(128), 0, c->active, b->dB, (int)r0, (int)rows, dN, dL, dE, dG, dS, dF);
            if((rc = check_launch(c, "k_gather_selected"))) return done(rc);
            const size_t cols = rows * stride, o0 = r0 * stride;
            hipError_t e = hipSuccess;
            if(o->n_cols && e == hipSuccess) e = hipMemcpyAsync(o->n_cols + r0, dN, rows * 4, hipMemcpyDeviceToHost, c->active);
            if(o->col_level && e == hipSuccess) e = hipMemcpyAsync(o->col_level + o0, dL, cols * 4, hipMemcpyDeviceToHost, c->active);
            if(o->col_edge && e == hipSuccess) e = hipMemcpyAsync(o->col_edge + o0, dE, cols * 4, hipMemcpyDeviceToHost, c->active);
            if(o->col_gchar && e == hipSuccess) e = hipMemcpyAsync(o->col_gchar + o0, dG, cols, hipMemcpyDeviceToHost, c->active);
            if(o->col_schar && e == hipSuccess) e = hipMemcpyAsync(o->col_schar + o0, dS, cols, hipMemcpyDeviceToHost, c->active);
            if(o->col_fromseed && e == hipSuccess) e = hipMemcpyAsync(o->col_fromseed + o0, dF, cols, hipMemcpyDeviceToHost, c->active);
            if(e == hipSuccess) e = hipStreamSynchronize(c->active);
            if(e != hipSuccess) { c->err = std::string("hlala_batch_get_pairs: ") + hipGetErrorString(e); return done(HLALA_E_DEVICE); }
        }
        done(0);
    }
    return HLALA_OK;
}

int hlala_batch_get_pairs_packed(hlala_ctx* c, hlala_batch* b, hlala_pairs_packed_out* o)
{
    DEV_GUARD(c);
    ReaderScope rscope_(c, b); if(rscope_.rc) return rscope_.rc;
    if(!c || !b || !o || !o->col_off) return HLALA_E_ARG;
    if(!(b->staged & 4)) { c->err = "pairs not computed"; return HLALA_E_STATE; }
    DevBatch& B = b->B;
    const size_t nr = (size_t)B.n_reads;
    o->n_cols_total = 0;
    if(nr == 0) { o->col_off[0] = 0; return HLALA_OK; }
    std::vector<void*> tmp;
    auto done = [&](int r_) { for(void* p : tmp) pool_release(c, p); return r_; };
    int rc = 0; long long *dN = nullptr, *dOff = nullptr; char* dCub = nullptr;
    if((rc = dev_alloc(c, tmp, nr + 1, &dN)) || (rc = dev_alloc(c, tmp, nr + 1, &dOff))) return done(rc);
    hipStream_t st = c->active;
    hipLaunchKernelGGL(k_selected_ncols, dim3((unsigned)((nr + 1 + 255) / 256)), dim3(256), 0, st, b->dB, (int)nr, dN);
    if((rc = check_launch(c, "k_selected_ncols"))) return done(rc);
    size_t cubBytes = 0;
    HIP_TRY_F(c, hipcub::DeviceScan::ExclusiveSum(nullptr, cubBytes, dN, dOff, (int)(nr + 1), st), done);
    if((rc = dev_alloc(c, tmp, cubBytes ? cubBytes : 1, &dCub))) return done(rc);
    HIP_TRY_F(c, hipcub::DeviceScan::ExclusiveSum(dCub, cubBytes, dN, dOff, (int)(nr + 1), st), done);
    long long total = 0;
    HIP_TRY_F(c, hipMemcpyAsync(&total, dOff + nr, sizeof(total), hipMemcpyDeviceToHost, st), done);
    HIP_TRY_F(c, hipStreamSynchronize(st), done);
    o->n_cols_total = total;
    { std::vector<long long> ho(nr + 1); if((rc = dl(c, ho.data(), dOff, nr + 1))) return done(rc); HIP_TRY_F(c, hipStreamSynchronize(st), done); for(size_t i = 0; i <= nr; i++) o->col_off[i] = ho[i]; }
    if(total > o->cap_cols) { c->err = "hlala_batch_get_pairs_packed: cap_cols too small (n_cols_total holds the need)"; return done(HLALA_E_CAPACITY); }
    if(total == 0) return done(HLALA_OK);
    int *dL = nullptr, *dE = nullptr; uint8_t *dG = nullptr, *dS = nullptr, *dF = nullptr, *dQ = nullptr;
    const size_t T = (size_t)total;
    if((o->col_level && (rc = dev_alloc(c, tmp, T, &dL))) || (o->col_edge && (rc = dev_alloc(c, tmp, T, &dE))) || (o->col_gchar && (rc = dev_alloc(c, tmp, T, &dG))) ||
       (o->col_schar && (rc = dev_alloc(c, tmp, T, &dS))) || (o->col_fromseed && (rc = dev_alloc(c, tmp, T, &dF))) || (o->col_mapq && (rc = dev_alloc(c, tmp, T, &dQ)))) return done(rc);
    const unsigned grid = (unsigned)std::min<size_t>(nr, (size_t)c->stitch_grid * 4);
    hipLaunchKernelGGL(k_gather_packed, dim3(grid), dim3(64), 0, st, b->dB, (int)nr, (const long long*)dOff, dL, dE, dG, dS, dF, dQ);
    if((rc = check_launch(c, "k_gather_packed"))) return done(rc);
    if((rc = dl(c, o->col_level, dL, T)) || (rc = dl(c, o->col_edge, dE, T)) || (rc = dl(c, o->col_gchar, dG, T)) || (rc = dl(c, o->col_schar, dS, T)) ||
       (rc = dl(c, o->col_fromseed, dF, T)) || (rc = dl(c, o->col_mapq, dQ, T))) return done(rc);
    HIP_TRY_F(c, hipStreamSynchronize(st), done);
    return done(HLALA_OK);
}

int hlala_estimate_insert_size(hlala_ctx* c, const hlala_batch_in* in, hlala_insert_size_out* out)
{
    DEV_GUARD(c);
    if(!c || !in || !out) return HLALA_E_ARG;
    memset(out, 0, sizeof(*out));
    const int np = in->n_pairs, nr = 2 * np;
    if(np <= 0) { c->err = "hlala_estimate_insert_size: no pairs"; return HLALA_E_ARG; }
    // the batch of primaries: one chain per read (chain indices of `in` are those of the caller's numbering: the window convention of hlala_batch_in)
    std::vector<int64_t> chain_off(nr + 1), cigar_off(nr + 1, 0); std::vector<int32_t> read_primary(nr), contig(nr), pos(nr), offset(nr), as(nr); std::vector<uint8_t> rev(nr); std::vector<uint32_t> cigar;
    for(int r = 0; r < nr; r++) {
        const int64_t ch = in->read_primary[r];
        if(ch < in->chain_off[r] || ch >= in->chain_off[r + 1]) { c->err = "read_primary outside the read's chains"; return HLALA_E_ARG; }
        chain_off[r] = r; read_primary[r] = r; contig[r] = in->chain_contig[ch]; pos[r] = in->chain_pos[ch]; offset[r] = in->chain_offset[ch]; as[r] = in->chain_as[ch]; rev[r] = in->chain_reverse[ch];
        cigar.insert(cigar.end(), in->cigar + in->cigar_off[ch], in->cigar + in->cigar_off[ch + 1]); cigar_off[r + 1] = (int64_t)cigar.size();
    }
    chain_off[nr] = nr;
    hlala_batch_in pb = *in;
    pb.chain_off = chain_off.data(); pb.read_primary = read_primary.data(); pb.n_chains = nr; pb.chain_contig = contig.data(); pb.chain_pos = pos.data();
    pb.chain_offset = offset.data(); pb.chain_as = as.data(); pb.chain_reverse = rev.data(); pb.cigar_off = cigar_off.data(); pb.cigar = cigar.data();
    hlala_batch* b = nullptr;
    int rc = hlala_batch_create(c, &pb, &b); if(rc) return rc;
    auto done = [&](int r_) { hlala_batch_destroy(b); return r_; };
    if((rc = hlala_project_chains(c, b)) || (rc = hlala_extend_chains(c, b))) return done(rc);
    std::vector<void*> tmp; int *dN = nullptr, *dD = nullptr;
    auto done2 = [&](int r_) { for(void* p : tmp) pool_release(c, p); return done(r_); };
    if((rc = dev_alloc(c, tmp, (size_t)np, &dN)) || (rc = dev_alloc(c, tmp, (size_t)np * PAIR_MAXDIST, &dD))) return done2(rc);
    hipLaunchKernelGGL(k_pair_distances, dim3((unsigned)((np + 127) / 128)), dim3(128), 0, c->active, c->dG, b->dB, dN, dD);
    if((rc = check_launch(c, "k_pair_distances"))) return done2(rc);
    std::vector<int> hN((size_t)np), hD((size_t)np * PAIR_MAXDIST);
    if((rc = dl(c, hN.data(), dN, (size_t)np)) || (rc = dl(c, hD.data(), dD, (size_t)np * PAIR_MAXDIST))) return done2(rc);
    hipError_t e = hipStreamSynchronize(c->active);
    if(e != hipSuccess) { c->err = hipGetErrorString(e); return done2(HLALA_E_DEVICE); }
    // histogram in pair order (processBAM.cpp:1135-1146), then calculateInsertSizeFromHistogram (:991-1069)
    std::map<int, double> IS_combined_counts;
    for(int p = 0; p < np; p++) {
        if(hN[p] == -1) { out->n_skipped++; continue; }                       // flagged chain: the reference would have asserted
        out->n_used++;
        if(hN[p] == -2) { out->n_skipped++; continue; }                       // strands not valid, :1149
        if(hN[p] > PAIR_MAXDIST) { c->err = "more distinct insert-size distances for one pair than this build holds"; return done2(HLALA_E_CAPACITY); }
        std::set<int> dist(hD.begin() + (size_t)p * PAIR_MAXDIST, hD.begin() + (size_t)p * PAIR_MAXDIST + hN[p]);
        for(int IS : dist) { if(IS_combined_counts.count(IS) == 0) IS_combined_counts[IS] = 0; IS_combined_counts[IS] += 1.0 / (double)dist.size(); }
    }
    double total = 0; for(auto& kv : IS_combined_counts) total += kv.second;
    double cum = 0, med = 0, p20 = 0, p80 = 0; bool sm = false, s2 = false, s8 = false;
    for(auto& kv : IS_combined_counts) {
        cum += kv.second;
        if(!sm && cum >= total * 0.5) { med = kv.first; sm = true; }
        if(!s2 && cum >= total * 0.2) { p20 = kv.first; s2 = true; }
        if(!s8 && cum >= total * 0.8) { p80 = kv.first; s8 = true; }
    }
    if(!(sm && s2 && s8)) { c->err = "hlala_estimate_insert_size: no pair with valid strands and a common underlying sequence"; return done2(HLALA_E_STATE); }
    const double d20 = std::fabs(med - p20), d80 = std::fabs(med - p80);
    out->mean = med; out->sd = d20 > d80 ? d20 : d80; out->total_weight = total;
    return done2(HLALA_OK);
}

int hlala_set_insert_size(hlala_ctx* c, double insert_mean, double insert_sd)
{
    DEV_GUARD(c);
    if(!c) return HLALA_E_ARG;
    HIP_TRY(c, hipStreamSynchronize(c->stream)); HIP_TRY(c, hipStreamSynchronize(c->side));
    const double m0 = c->params.insert_mean, s0 = c->params.insert_sd;
    double* oldLog = c->d_islog; DevTables* oldT = c->dT;
    c->params.insert_mean = insert_mean; c->params.insert_sd = insert_sd;
    // (the kernels read the tables through c->dT, which batches do not cache: the new tables go to the same device address)
    std::vector<void*> keep; keep.swap(c->allocs);
    int rc = build_tables(c);
    std::vector<void*> made; made.swap(c->allocs); c->allocs.swap(keep);
    if(rc) { for(void* p : made) if(p) pool_release(c, p); c->params.insert_mean = m0; c->params.insert_sd = s0; c->d_islog = oldLog; c->dT = oldT; return rc; }
    // copy the new table struct over the old one so that every holder of the old pointer sees it; the log-pdf array it points to stays alive in allocs
    hipError_t e = hipMemcpyAsync(oldT, c->dT, sizeof(DevTables), hipMemcpyDeviceToDevice, c->stream);
    if(e == hipSuccess) e = hipStreamSynchronize(c->stream);
    for(void* p : made) { if(p == (void*)c->dT) pool_release(c, p); else c->allocs.push_back(p); }
    c->dT = oldT;
    if(e != hipSuccess) { c->err = std::string("hlala_set_insert_size: ") + hipGetErrorString(e); return HLALA_E_DEVICE; }
    return HLALA_OK;
}

int hlala_set_gene_intervals(hlala_ctx* c, int32_t n, const int32_t* first_level, const int32_t* last_level)
{
    DEV_GUARD(c);
    if(!c || n < 0 || (n > 0 && (!first_level || !last_level))) return HLALA_E_ARG;
    for(int i = 0; i < n; i++) if(first_level[i] < 0 || last_level[i] < first_level[i]) { c->err = "gene interval with first > last or negative level"; return HLALA_E_ARG; }
    c->n_genes = 0;
    if(n > 0) {
        int rc = dev_upload(c, c->allocs, first_level, (size_t)n, &c->d_gene_first); if(rc) return rc;
        rc = dev_upload(c, c->allocs, last_level, (size_t)n, &c->d_gene_last); if(rc) return rc;
        HIP_TRY(c, hipStreamSynchronize(c->active));
    }
    c->n_genes = n;
    return HLALA_OK;
}

int hlala_postprocess_pairs(hlala_ctx* c, hlala_batch* b, uint8_t* include_in_hla)
{
    DEV_GUARD(c);
    ReaderScope rscope_(c, b); if(rscope_.rc) return rscope_.rc;
    if(!c || !b) return HLALA_E_ARG;
    if(!(b->staged & 4)) { c->err = "hlala_postprocess_pairs before hlala_pair_chains"; return HLALA_E_STATE; }
    DevBatch& B = b->B;
    if(!c->d_cov) {
        c->n_cov = c->F.L > 1 ? c->F.L - 1 : 1;
        int rc = dev_alloc(c, c->allocs, (size_t)c->n_cov, &c->d_cov, true); if(rc) return rc;
    }
    if(B.n_pairs <= 0) return HLALA_OK;
    uint8_t* dInc = nullptr; std::vector<void*> tmp;
    auto done = [&](int r_) { for(void* p : tmp) pool_release(c, p); return r_; };
    if(include_in_hla) { int rc = dev_alloc(c, tmp, (size_t)B.n_pairs, &dInc, false); if(rc) return done(rc); }
    hipError_t e = hipMemsetAsync(B.work_counter + 11, 0, sizeof(int), c->active);
    if(e != hipSuccess) { c->err = hipGetErrorString(e); return done(HLALA_E_DEVICE); }
    int grid = B.n_pairs < c->stitch_grid ? B.n_pairs : c->stitch_grid;
    hipLaunchKernelGGL(k_post_pairs, dim3(grid), dim3(64), 0, c->active, b->dB, c->d_cov, c->n_cov, c->d_gene_first, c->d_gene_last, c->n_genes, dInc);
    int rc = check_launch(c, "k_post_pairs"); if(rc) return done(rc);
    if(include_in_hla) e = hipMemcpyAsync(include_in_hla, dInc, (size_t)B.n_pairs, hipMemcpyDeviceToHost, c->active);
    if(e == hipSuccess) e = hipStreamSynchronize(c->active);
    if(e != hipSuccess) { c->err = std::string("hlala_postprocess_pairs: ") + hipGetErrorString(e); return done(HLALA_E_DEVICE); }
    return done(HLALA_OK);
}

int hlala_get_coverage(hlala_ctx* c, int32_t* bases_per_level, int reset)
{
    DEV_GUARD(c);
    ReaderScope rscope_(c, nullptr);
    if(!c || !bases_per_level) return HLALA_E_ARG;
    const int n = c->F.L > 1 ? c->F.L - 1 : 1;
    if(!c->d_cov) { memset(bases_per_level, 0, (size_t)n * 4); return HLALA_OK; }
    HIP_TRY(c, hipMemcpyAsync(bases_per_level, c->d_cov, (size_t)n * 4, hipMemcpyDeviceToHost, c->active));
    if(reset) HIP_TRY(c, hipMemsetAsync(c->d_cov, 0, (size_t)n * 4, c->active));
    HIP_TRY(c, hipStreamSynchronize(c->active));
    return HLALA_OK;
}

int hlala_batch_export_pair_records(hlala_ctx* c, hlala_batch* b, double* device_out)
{
    DEV_GUARD(c);
    // a reader like the getters: on the reader stream, behind THIS batch's work on the main and the side stream -- not behind the alignment of the next batch the
    // caller has queued on the main stream since (it ran there until round 4: with two batches in flight the records of batch i waited for batch i+1) -- and
    // synchronised on return, so that a collective the caller issues next on any stream of its own finds the records in place
    ReaderScope rscope_(c, b); if(rscope_.rc) return rscope_.rc;
    if(!c || !b || !device_out) return HLALA_E_ARG;
    if(!(b->staged & 4)) { c->err = "pairs not computed"; return HLALA_E_STATE; }
    if(b->B.n_pairs > 0) {
        hipLaunchKernelGGL(k_export_pairs, dim3((b->B.n_pairs + 255) / 256), dim3(256), 0, c->active, b->dB, device_out);
        int rc = check_launch(c, "k_export_pairs"); if(rc) return rc;
        HIP_TRY(c, hipStreamSynchronize(c->active));
    }
    return HLALA_OK;
}

// ---- several GPUs in ONE process (the host program's --devices: one context per GPU): the exchange steps of the path over RCCL.
// The reference merges its per-thread results on the host (mapper/processBAM.cpp:1866-1887: the per-thread alignment vectors are appended, the per-level read
// counters added up); with one context per GPU the same two steps are a gather of the per-pair records and a sum-reduce of the coverage counters to the first
// context's device.  RCCL is looked up at run time (dlopen: a one-GPU run never loads it) and used when the communicator's contexts sit on different devices;
// contexts that share a device (tests on a one-GPU box) or a communicator of one take device-to-device copies on the same arrays.
#include <rccl/rccl.h>
#include <dlfcn.h>
namespace {
struct RcclApi {
    void* lib = nullptr; bool tried = false; std::string err;
    ncclResult_t (*CommInitAll)(ncclComm_t*, int, const int*) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*GroupStart)() = nullptr; ncclResult_t (*GroupEnd)() = nullptr;
    ncclResult_t (*Send)(const void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*Recv)(void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*Reduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, int, ncclComm_t, hipStream_t) = nullptr;
    const char* (*GetErrorString)(ncclResult_t) = nullptr;
    bool load()
    {
        if(tried) return lib != nullptr;
        tried = true;
        for(const char* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) { lib = dlopen(name, RTLD_NOW | RTLD_LOCAL); if(lib) break; }
        if(!lib) { err = std::string("librccl.so not found: ") + dlerror(); return false; }
#define RSYM(field, sym) do { *(void**)(&field) = dlsym(lib, sym); if(!field) { err = std::string("librccl.so lacks ") + sym; dlclose(lib); lib = nullptr; return false; } } while(0)
        RSYM(CommInitAll, "ncclCommInitAll"); RSYM(CommDestroy, "ncclCommDestroy"); RSYM(GroupStart, "ncclGroupStart"); RSYM(GroupEnd, "ncclGroupEnd");
        RSYM(Send, "ncclSend"); RSYM(Recv, "ncclRecv"); RSYM(Reduce, "ncclReduce"); RSYM(GetErrorString, "ncclGetErrorString");
#undef RSYM
        return true;
    }
};
RcclApi g_rccl; std::mutex g_rccl_mu;
}
struct hlala_comm {
    std::vector<hlala_ctx*> ctxs;
    std::vector<ncclComm_t> comms;            // empty: device-to-device copies (one context, or contexts that share a device)
    std::vector<hipStream_t> streams;         // one per context, for the collectives
    std::vector<double*> send; std::vector<size_t> sendCap;      // per context: its batch's records
    double* recv = nullptr; size_t recvCap = 0;                  // on the first context's device: every context's records, in context order
    int* covAcc = nullptr; size_t covN = 0;                      // ... and the summed coverage counters
    std::string err;
};
static thread_local std::string g_comm_error;
const char* hlala_comm_last_error(const hlala_comm* m) { return m ? m->err.c_str() : g_comm_error.c_str(); }
int hlala_comm_uses_rccl(const hlala_comm* m) { return m && !m->comms.empty() ? 1 : 0; }

void hlala_comm_destroy(hlala_comm* m)
{
    if(!m) return;
    for(size_t i = 0; i < m->ctxs.size(); i++) {
        DevGuard g(m->ctxs[i]->device);
        if(i < m->streams.size() && m->streams[i]) { (void)hipStreamSynchronize(m->streams[i]); (void)hipStreamDestroy(m->streams[i]); }
        if(i < m->send.size() && m->send[i]) (void)hipFree(m->send[i]);
        if(i == 0) { if(m->recv) (void)hipFree(m->recv); if(m->covAcc) (void)hipFree(m->covAcc); }
    }
    for(ncclComm_t q : m->comms) if(q) (void)g_rccl.CommDestroy(q);
    delete m;
}

int hlala_comm_create(hlala_ctx* const* ctxs, int n, hlala_comm** out)
{
    if(out) *out = nullptr;
    if(!ctxs || n < 1 || !out) { g_comm_error = "hlala_comm_create: no contexts"; return HLALA_E_ARG; }
    for(int i = 0; i < n; i++) if(!ctxs[i]) { g_comm_error = "hlala_comm_create: null context"; return HLALA_E_ARG; }
    hlala_comm* m = new hlala_comm;
    m->ctxs.assign(ctxs, ctxs + n); m->streams.assign((size_t)n, nullptr); m->send.assign((size_t)n, nullptr); m->sendCap.assign((size_t)n, 0);
    auto fail = [&](int rc, const std::string& e) { g_comm_error = e; hlala_comm_destroy(m); return rc; };
    for(int i = 0; i < n; i++) { DevGuard g(ctxs[i]->device); if(hipStreamCreateWithFlags(&m->streams[(size_t)i], hipStreamNonBlocking) != hipSuccess) return fail(HLALA_E_DEVICE, "hlala_comm_create: hipStreamCreate failed"); }
    std::set<int> distinct; for(int i = 0; i < n; i++) distinct.insert(ctxs[i]->device);
    const char* force = getenv("HLALA_COMM_RCCL");          // 1: RCCL even for a communicator of one (tests); 0: never
    const bool want = force ? atoi(force) != 0 : n > 1;
    if(want && (int)distinct.size() == n) {
        std::lock_guard<std::mutex> g(g_rccl_mu);
        if(!g_rccl.load()) return fail(HLALA_E_DEVICE, "hlala_comm_create: " + g_rccl.err);
        std::vector<int> devs((size_t)n); for(int i = 0; i < n; i++) devs[(size_t)i] = ctxs[i]->device;
        m->comms.assign((size_t)n, nullptr);
        const ncclResult_t r = g_rccl.CommInitAll(m->comms.data(), n, devs.data());
        if(r != ncclSuccess) { m->comms.clear(); return fail(HLALA_E_DEVICE, std::string("ncclCommInitAll: ") + g_rccl.GetErrorString(r)); }
    }
    *out = m;
    return HLALA_OK;
}

static int comm_buf(hlala_comm* m, int device, double** p, size_t* cap, size_t need)
{
    if(*cap >= need && *p) return HLALA_OK;
    DevGuard g(device);
    if(*p) (void)hipFree(*p);
    *p = nullptr; *cap = 0;
    if(device_malloc_retry(device, nullptr, (void**)p, (need ? need : 1) * sizeof(double)) != hipSuccess) { m->err = "hipMalloc (gather buffers) failed"; return HLALA_E_DEVICE; }
    *cap = need;
    return HLALA_OK;
}

// The per-pair records (8 doubles per pair: hlala_batch_export_pair_records) of one batch per context -- batches[i] belongs to context i of the communicator, NULL:
// that context has none this round -- gathered to the first context's device and copied to host_out in context order; counts_out[i] = pairs of context i.
// The counts are known on the host (the batches live in this process: the "counts first" step of the multi-process protocol in hla-la_amd/dist.py needs no
// collective here); the payload is ONE grouped exchange: every context sends its records, the first one posts a receive per peer at that peer's offset.
int hlala_gather_pair_records(hlala_comm* m, hlala_batch* const* batches, double* host_out, int64_t host_capacity_pairs, int64_t* counts_out)
{
    if(!m || !batches || !host_out) return HLALA_E_ARG;
    const int n = (int)m->ctxs.size();
    std::vector<size_t> cnt((size_t)n, 0), off((size_t)n + 1, 0);
    for(int i = 0; i < n; i++) { if(batches[i]) { if(batches[i]->ctx != m->ctxs[(size_t)i]) { m->err = "hlala_gather_pair_records: batch " + std::to_string(i) + " does not belong to context " + std::to_string(i); return HLALA_E_ARG; } cnt[(size_t)i] = (size_t)batches[i]->B.n_pairs; } off[(size_t)i + 1] = off[(size_t)i] + cnt[(size_t)i]; if(counts_out) counts_out[i] = (int64_t)cnt[(size_t)i]; }
    const size_t total = off[(size_t)n];
    if((int64_t)total > host_capacity_pairs) { m->err = "hlala_gather_pair_records: " + std::to_string(total) + " pairs, room for " + std::to_string(host_capacity_pairs); return HLALA_E_CAPACITY; }
    if(total == 0) return HLALA_OK;
    int rc = comm_buf(m, m->ctxs[0]->device, &m->recv, &m->recvCap, 8 * total); if(rc) return rc;
    const bool rccl = !m->comms.empty();
    // every context's records into its send buffer (the first context's straight into its place in the receive buffer when no RCCL exchange follows)
    for(int i = 0; i < n; i++) {
        if(!cnt[(size_t)i]) continue;
        double* dst = nullptr;
        if(!rccl && m->ctxs[(size_t)i]->device == m->ctxs[0]->device) dst = m->recv + 8 * off[(size_t)i];
        else { rc = comm_buf(m, m->ctxs[(size_t)i]->device, &m->send[(size_t)i], &m->sendCap[(size_t)i], 8 * cnt[(size_t)i]); if(rc) return rc; dst = m->send[(size_t)i]; }
        rc = hlala_batch_export_pair_records(m->ctxs[(size_t)i], batches[i], dst);      // (returns synchronised: the records are in place)
        if(rc) { m->err = std::string("hlala_batch_export_pair_records: ") + m->ctxs[(size_t)i]->err; return rc; }
    }
    if(rccl) {
        ncclResult_t r = g_rccl.GroupStart();
        for(int i = 0; i < n && r == ncclSuccess; i++) {
            if(!cnt[(size_t)i]) continue;
            r = g_rccl.Send(m->send[(size_t)i], 8 * cnt[(size_t)i], ncclDouble, 0, m->comms[(size_t)i], m->streams[(size_t)i]);
            if(r == ncclSuccess) r = g_rccl.Recv(m->recv + 8 * off[(size_t)i], 8 * cnt[(size_t)i], ncclDouble, i, m->comms[0], m->streams[0]);
        }
        const ncclResult_t re = g_rccl.GroupEnd();
        if(r == ncclSuccess) r = re;
        if(r != ncclSuccess) { m->err = std::string("RCCL gather: ") + g_rccl.GetErrorString(r); return HLALA_E_DEVICE; }
        for(int i = 1; i < n; i++) if(cnt[(size_t)i]) { DevGuard g(m->ctxs[(size_t)i]->device); if(hipStreamSynchronize(m->streams[(size_t)i]) != hipSuccess) { m->err = "RCCL gather: send stream failed"; return HLALA_E_DEVICE; } }
    } else {
        // contexts on other devices without RCCL (HLALA_COMM_RCCL=0): peer copies into the receive buffer
        for(int i = 0; i < n; i++) if(cnt[(size_t)i] && m->ctxs[(size_t)i]->device != m->ctxs[0]->device) {
            DevGuard g(m->ctxs[0]->device);
            if(hipMemcpyPeerAsync(m->recv + 8 * off[(size_t)i], m->ctxs[0]->device, m->send[(size_t)i], m->ctxs[(size_t)i]->device, 8 * cnt[(size_t)i] * sizeof(double), m->streams[0]) != hipSuccess) { m->err = "hipMemcpyPeerAsync failed"; return HLALA_E_DEVICE; }
        }
    }
    DevGuard g0(m->ctxs[0]->device);
    if(hipMemcpyAsync(host_out, m->recv, 8 * total * sizeof(double), hipMemcpyDeviceToHost, m->streams[0]) != hipSuccess || hipStreamSynchronize(m->streams[0]) != hipSuccess) { m->err = "gather: copy to the host failed"; return HLALA_E_DEVICE; }
    return HLALA_OK;
}

// bases_per_level of every context of the communicator added up on the first context's device (ncclReduce, sum of int32 -- integer sums do not depend on the
// order) and copied to bases_per_level; reset: the contexts' counters are cleared afterwards (hlala_get_coverage).  processBAM.cpp:1866-1887, :1902-1913.
int hlala_reduce_coverage(hlala_comm* m, int32_t* bases_per_level, int reset)
{
    if(!m || !bases_per_level) return HLALA_E_ARG;
    const int n = (int)m->ctxs.size();
    hlala_ctx* c0 = m->ctxs[0];
    const size_t nl = (size_t)(c0->F.L > 1 ? c0->F.L - 1 : 1);
    for(int i = 0; i < n; i++) if(m->ctxs[(size_t)i]->F.L != c0->F.L) { m->err = "hlala_reduce_coverage: the contexts hold different graphs"; return HLALA_E_ARG; }
    if(m->comms.empty() || n == 1) {
        // one context, or contexts sharing a device: the host adds the counters up
        std::vector<int32_t> one(nl);
        std::fill(bases_per_level, bases_per_level + nl, 0);
        for(int i = 0; i < n; i++) { int rc = hlala_get_coverage(m->ctxs[(size_t)i], one.data(), reset); if(rc) { m->err = m->ctxs[(size_t)i]->err; return rc; } for(size_t k = 0; k < nl; k++) bases_per_level[k] += one[k]; }
        return HLALA_OK;
    }
    { DevGuard g(c0->device); if(m->covN < nl) { if(m->covAcc) (void)hipFree(m->covAcc); m->covAcc = nullptr; if(device_malloc_retry(c0->device, nullptr, (void**)&m->covAcc, nl * sizeof(int)) != hipSuccess) { m->err = "hipMalloc (coverage) failed"; return HLALA_E_DEVICE; } m->covN = nl; } }
    // every context's counters exist and are final: its queued work is waited for first (post-processing adds to them on the reader stream)
    for(int i = 0; i < n; i++) { hlala_ctx* c = m->ctxs[(size_t)i]; DevGuard g(c->device);
        if(!c->d_cov) { c->n_cov = (int)nl; int rc = dev_alloc(c, c->allocs, nl, &c->d_cov, true); if(rc) { m->err = c->err; return rc; } }
        if(hipStreamSynchronize(c->rs) != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess) { m->err = "hlala_reduce_coverage: a context's stream failed"; return HLALA_E_DEVICE; } }
    ncclResult_t r = g_rccl.GroupStart();
    for(int i = 0; i < n && r == ncclSuccess; i++) r = g_rccl.Reduce(m->ctxs[(size_t)i]->d_cov, i == 0 ? (void*)m->covAcc : nullptr, nl, ncclInt32, ncclSum, 0, m->comms[(size_t)i], m->streams[(size_t)i]);
    const ncclResult_t re = g_rccl.GroupEnd();
    if(r == ncclSuccess) r = re;
    if(r != ncclSuccess) { m->err = std::string("RCCL reduce: ") + g_rccl.GetErrorString(r); return HLALA_E_DEVICE; }
    for(int i = 0; i < n; i++) { hlala_ctx* c = m->ctxs[(size_t)i]; DevGuard g(c->device);
        if(hipStreamSynchronize(m->streams[(size_t)i]) != hipSuccess) { m->err = "RCCL reduce: stream failed"; return HLALA_E_DEVICE; }
        if(reset && hipMemset(c->d_cov, 0, nl * sizeof(int)) != hipSuccess) { m->err = "hipMemset failed"; return HLALA_E_DEVICE; } }
    DevGuard g0(c0->device);
    if(hipMemcpy(bases_per_level, m->covAcc, nl * sizeof(int), hipMemcpyDeviceToHost) != hipSuccess) { m->err = "coverage: copy to the host failed"; return HLALA_E_DEVICE; }
    return HLALA_OK;
}


int hlala_batch_get_stats(hlala_ctx* c, hlala_batch* b, hlala_batch_stats* out)
{
    DEV_GUARD(c);
    ReaderScope rscope_(c, b); if(rscope_.rc) return rscope_.rc;
    if(!c || !b || !out) return HLALA_E_ARG;
    memset(out, 0, sizeof(*out));
    if(!b->outputs_ready) return HLALA_OK;       // only uploaded so far: no stage has run, the counters do not exist yet (zeros, as before the outputs were allocated lazily)
    HIP_TRY(c, hipStreamSynchronize(c->active));
    u64 cnt[16];
    HIP_TRY(c, hipMemcpyAsync(cnt, b->B.counters, sizeof(cnt), hipMemcpyDeviceToHost, c->active)); HIP_TRY(c, hipStreamSynchronize(c->active));
    if((b->staged & 1) && !b->B.from_seeds) (void)hipEventElapsedTime(&out->ms_project, b->ev[EV_PROJECT_BEGIN], b->ev[EV_PROJECT_END]);
    if(b->staged & 2) { (void)hipEventElapsedTime(&out->ms_extend, b->ev[EV_EXTEND_BEGIN], b->ev[EV_EXTEND_END]); if(b->B.n_chains > 0) { (void)hipEventElapsedTime(&out->ms_extend_retry, b->ev[EV_DP_CLASS0_END], b->ev[b->side_used ? EV_DP_CLASS2_END : EV_DP_END]); (void)hipEventElapsedTime(&out->ms_dp_main, b->ev[EV_DP_BEGIN], b->ev[EV_DP_CLASS0_END]);
          for(int k = 0; k <= DP_LAST_TIER; k++) (void)hipEventElapsedTime(&out->ms_dp_class[k], b->ev[EV_DP_CLASS_BEGIN + k], b->ev[EV_DP_CLASS_END + k]);
          (void)hipEventElapsedTime(&out->ms_dp_jump_free, b->ev[EV_DP_CLASS_BEGIN], b->ev[EV_DP_JUMP_FREE_END]);
          if(b->band_used) (void)hipEventElapsedTime(&out->ms_dp_band, b->ev[EV_DP_BAND_BEGIN], b->ev[EV_DP_BAND_END]);
          if(b->side_used) (void)hipEventElapsedTime(&out->ms_side, b->ev[EV_SIDE_BEGIN], b->ev[EV_SIDE_END]); } }
    { int wc[WC_N]; HIP_TRY(c, hipMemcpyAsync(wc, b->B.work_counter, sizeof(wc), hipMemcpyDeviceToHost, c->active)); HIP_TRY(c, hipStreamSynchronize(c->active)); out->n_chains_retried = 0; for(int k = 1; k <= 6; k++) out->n_dp_class[k] = wc[wc_retry_short(k, 0)] + wc[wc_retry_short(k, 1)] + wc[wc_retry_long(k, 0)] + wc[wc_retry_long(k, 1)];          // (short and long calls of a retry row: batch.h)
      for(int k = 1; k <= 6; k++) out->n_chains_retried += out->n_dp_class[k]; out->n_dp_retried_large = out->n_dp_class[5];
      out->n_dp_band = b->band_used ? wc[WC_BAND_CALLS] : 0; out->n_dp_band_failed = b->band_used ? wc[WC_BAND_FAILED] : 0; out->n_dp_jump_free_failed = wc[WC_JF_FAILED];
      out->n_dp_class[0] = wc[8] + wc[9] - out->n_dp_band + out->n_dp_band_failed; out->n_dp_jump_free = wc[6]; }
    if(b->staged & 4) (void)hipEventElapsedTime(&out->ms_pair, b->ev[EV_PAIR_BEGIN], b->ev[EV_PAIR_END]);
    out->n_chains_extended = (int64_t)cnt[CNT_CHAINS_EXT]; out->n_dp_calls = (int64_t)cnt[CNT_DP_CALLS];
    out->n_dp_iterations = (int64_t)cnt[CNT_DP_ITERS]; out->n_dp_cells = (int64_t)cnt[CNT_DP_CELLS];
    out->n_seed_columns = (int64_t)cnt[CNT_SEED_COLS]; out->n_out_columns = (int64_t)cnt[CNT_OUT_COLS];
    out->n_edges_touched = (int64_t)cnt[CNT_EDGES]; out->n_errors = (int64_t)cnt[CNT_ERRORS]; out->n_dp_shared = (int64_t)cnt[CNT_DP_SHARED];
    return HLALA_OK;
}

}  // extern "C"

// ------------------------------------------------------------------------------------ HLATyper scoring
static int typer_tables(hlala_ctx* c, std::vector<void*>& tmp, TyperTables** out)
{
    TyperTables T;
    double insertionP = c->params.long_read_mode ? 0.075 : 0.001, deletionP = insertionP;          // HLATyper.cpp:935-942
    T.ll_ins_actual = log(insertionP) + log(1.0 / 4.0);                                            // :952-954
    T.ll_deletion = log(deletionP);                                                                // :956
    T.ll_match_mismatch = log(1 - insertionP - deletionP);                                         // :959
    for(int q = 0; q < 256; q++) {
        double pCorrect = host_PhredToPCorrect((unsigned char)(q < 33 ? 33 : q));
        if(pCorrect > 0.999) pCorrect = 0.999;                                                     // veryConservativeReadLikelihoods, :2190-2194
        if(pCorrect == 0) pCorrect = 0.001;                                                        // :2197-2200
        T.ll_match[q] = log(pCorrect);
        double pIncorrect = (1 - pCorrect) * (1.0 / 3.0);
        T.ll_mismatch[q] = log(pIncorrect);
    }
    return dev_upload(c, tmp, &T, 1, out);
}

// The three steps of a locus (hla/HLATyper.cpp:2067-2541) on tables that may stay on the device between them: `keep` (non-null) receives the device tables
// of a step instead of the pool, and a step whose device inputs are given uploads nothing (hlala_type_locus).  Host outputs that are null are not downloaded.
static void hand_over(std::vector<void*>& from, std::vector<void*>* to, void* p)
{
    for(size_t i = 0; i < from.size(); i++) if(from[i] == p) { from.erase(from.begin() + (ptrdiff_t)i); break; }
    to->push_back(p);
}
static int exon_loglik_impl(hlala_ctx* c, const hlala_exon_in* in, double* LL, int32_t* mism, std::vector<void*>* keep, double** dLLout, int** dMout)
{
    if(!c || !in || (!keep && (!LL || !mism))) return HLALA_E_ARG;
    const int C = in->n_clusters, P = in->exon_length, R = in->n_reads;
    if(C < 0 || P < 0 || R < 0) { c->err = "negative sizes"; return HLALA_E_ARG; }
    if(C == 0 || R == 0) return HLALA_OK;
    const size_t npos = (size_t)in->pos_off[R];
    for(size_t i = 0; i < npos; i++) if(in->pos_exon[i] < 0 || in->pos_exon[i] >= P || in->pos_glen[i] < 1) { c->err = "exon position out of range / empty genotype"; return HLALA_E_ARG; }
    std::vector<void*> tmp; int rc = 0;
    auto done = [&](int r) { for(void* p : tmp) pool_release(c, p); return r; };
    TyperTables* dT = nullptr; if((rc = typer_tables(c, tmp, &dT))) return done(rc);
    // cluster sequences transposed to [P][C] on the host side of the upload (one-time per locus)
    std::vector<uint8_t> seqT((size_t)C * P);
    for(int cc = 0; cc < C; cc++) for(int p = 0; p < P; p++) seqT[(size_t)p * C + cc] = in->cluster_seq[(size_t)cc * P + p];
    uint8_t *dSeq, *dG0, *dQ, *dUse; int *dOff, *dExon, *dGlen, *dM; double* dLL;
    if((rc = dev_upload(c, tmp, seqT.data(), seqT.size(), &dSeq))) return done(rc);
    if((rc = dev_upload(c, tmp, in->pos_off, (size_t)R + 1, &dOff))) return done(rc);
    if((rc = dev_upload(c, tmp, in->pos_exon, npos, &dExon))) return done(rc);
    if((rc = dev_upload(c, tmp, in->pos_g0, npos, &dG0))) return done(rc);
    if((rc = dev_upload(c, tmp, in->pos_glen, npos, &dGlen))) return done(rc);
    if((rc = dev_upload(c, tmp, in->pos_qual, npos, &dQ))) return done(rc);
    if((rc = dev_upload(c, tmp, in->pos_use, npos, &dUse))) return done(rc);
    if((rc = dev_alloc(c, tmp, (size_t)C * R, &dLL))) return done(rc);
    if((rc = dev_alloc(c, tmp, (size_t)C * R, &dM))) return done(rc);
    hipLaunchKernelGGL(k_exon_loglik, dim3((C + 255) / 256, R), dim3(256), 0, c->active, dT, C, P, R, dSeq, dOff, dExon, dG0, dGlen, dQ, dUse, dLL, dM);
    if((rc = check_launch(c, "k_exon_loglik"))) return done(rc);
    if((LL && hipMemcpyAsync(LL, dLL, (size_t)C * R * 8, hipMemcpyDeviceToHost, c->active) != hipSuccess) || (mism && hipMemcpyAsync(mism, dM, (size_t)C * R * 4, hipMemcpyDeviceToHost, c->active) != hipSuccess) ||
       hipStreamSynchronize(c->active) != hipSuccess) { c->err = "hlala_exon_loglik: download failed"; return done(HLALA_E_DEVICE); }       // (synchronised either way: the host arrays uploaded above are the caller's)
    if(keep) { hand_over(tmp, keep, dLL); hand_over(tmp, keep, dM); *dLLout = dLL; *dMout = dM; }
    return done(HLALA_OK);
}
extern "C" int hlala_exon_loglik(hlala_ctx* c, const hlala_exon_in* in, double* LL, int32_t* mism)
{
    DEV_GUARD(c);
    ReaderScope rscope_(c, nullptr);
    if(!c || !in || !LL || !mism) return HLALA_E_ARG;
    return exon_loglik_impl(c, in, LL, mism, nullptr, nullptr, nullptr);
}

static int pair_loglik_impl(hlala_ctx* c, const double* LL, const int32_t* mism, const double* dLLin, const int* dMin, int32_t C, int32_t R, double* pairLL, double* misAvg, double* misMin,
                           std::vector<void*>* keep, double** dPout, double** dAout, double** dMnout)
{
    if(!c || (!dLLin && (!LL || !mism)) || !pairLL || !misAvg || !misMin || C < 0 || R < 0) return HLALA_E_ARG;
    if(C == 0) return HLALA_OK;
    std::vector<void*> tmp; int rc = 0;
    auto done = [&](int r) { for(void* p : tmp) pool_release(c, p); return r; };
    const size_t npairs = (size_t)C * (C + 1) / 2, nCR = (size_t)C * R;
    double *dLL, *dLLT, *dP, *dA, *dMn; int *dM, *dMT;
    if(dLLin) { dLL = const_cast<double*>(dLLin); dM = const_cast<int*>(dMin); }
    else {
        if((rc = dev_upload(c, tmp, LL, nCR, &dLL))) return done(rc);
        if((rc = dev_upload(c, tmp, mism, nCR, &dM))) return done(rc);
    }
    if((rc = dev_alloc(c, tmp, nCR, &dLLT))) return done(rc);
    if((rc = dev_alloc(c, tmp, nCR, &dMT))) return done(rc);
    if((rc = dev_alloc(c, tmp, npairs, &dP))) return done(rc);
    if((rc = dev_alloc(c, tmp, npairs, &dA))) return done(rc);
    if((rc = dev_alloc(c, tmp, npairs, &dMn))) return done(rc);
    if(R > 0) {
        dim3 tb(32, 32), tg((R + 31) / 32, (C + 31) / 32);
        hipLaunchKernelGGL(k_transpose<double>, tg, tb, 0, c->active, C, R, dLL, dLLT);
        hipLaunchKernelGGL(k_transpose<int>, tg, tb, 0, c->active, C, R, dM, dMT);
    }
    hipLaunchKernelGGL(k_pair_loglik, dim3((C + 255) / 256, (C + PAIRLL_ROWS - 1) / PAIRLL_ROWS), dim3(256), 0, c->active, C, R, dLL, dLLT, dM, dMT, dP, dA, dMn);
    if((rc = check_launch(c, "k_pair_loglik"))) return done(rc);
    if(hipMemcpyAsync(pairLL, dP, npairs * 8, hipMemcpyDeviceToHost, c->active) != hipSuccess || hipMemcpyAsync(misAvg, dA, npairs * 8, hipMemcpyDeviceToHost, c->active) != hipSuccess ||
       hipMemcpyAsync(misMin, dMn, npairs * 8, hipMemcpyDeviceToHost, c->active) != hipSuccess || (!keep && hipStreamSynchronize(c->active) != hipSuccess)) { c->err = "hlala_pair_loglik: download failed"; return done(HLALA_E_DEVICE); }
    if(keep) { hand_over(tmp, keep, dP); hand_over(tmp, keep, dA); hand_over(tmp, keep, dMn); *dPout = dP; *dAout = dA; *dMnout = dMn;
               hand_over(tmp, keep, dLLT); hand_over(tmp, keep, dMT); }      // (not synchronised: the caller's next step runs behind this one on the same stream; its scratch stays allocated until then)
    return done(HLALA_OK);
}
extern "C" int hlala_pair_loglik(hlala_ctx* c, const double* LL, const int32_t* mism, int32_t C, int32_t R, double* pairLL, double* misAvg, double* misMin)
{
    DEV_GUARD(c);
    ReaderScope rscope_(c, nullptr);
    if(!c || !LL || !mism) return HLALA_E_ARG;
    return pair_loglik_impl(c, LL, mism, nullptr, nullptr, C, R, pairLL, misAvg, misMin, nullptr, nullptr, nullptr, nullptr);
}

// ---- the typer's read / allele filters on the device (kernel_filter.hip; filter_gpu_core.h; the host's hlala_filter_positions is the specification)
extern "C" int hlala_filter_positions_gpu(hlala_ctx* c, const hlala_exon_positions_out* pos, const hlala_filter_params* prm, uint8_t* pos_use, uint8_t* read_ignored, hlala_filter_stats* stats,
                                          int64_t* counts)
{
    using namespace hlala_filter;
    DEV_GUARD(c);
    ReaderScope rscope_(c, nullptr);
    if(!c) return HLALA_E_ARG;
    if(const char* a = flt_check_args(pos, prm, pos_use)) { c->err = std::string("hlala_filter_positions_gpu: ") + a; return HLALA_E_ARG; }
    int64_t Cn[FC_N] = {0, 0, 0, 0, 0, 0};
    for(double& m : c->flt_ms) m = 0;
    if(pos->n_reads == 0) {                                     // the host writes nothing but zeroed counters
        if(stats) memset(stats, 0, sizeof(*stats));
        if(counts) memcpy(counts, Cn, sizeof(Cn));
        return HLALA_OK;
    }
    const u32 nr = (u32)pos->n_reads, np = (u32)pos->n_pos, nch = (u32)pos->n_chars;
    std::vector<void*> tmp; int rc = 0;
    hipEvent_t ev[7] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    // (everything queued -- uploads from the caller's arrays, kernels on the scratch -- ends before the blocks go back to the pool)
    auto done = [&](int r) { (void)hipStreamSynchronize(c->active); for(void* p : tmp) pool_release(c, p); for(hipEvent_t e : ev) if(e) (void)hipEventDestroy(e); return r; };
    auto mark = [&](int k) { if(c->flt_timed && ev[k]) (void)hipEventRecord(ev[k], c->active); };
    if(c->flt_timed) for(hipEvent_t& e : ev) HIP_TRY_F(c, hipEventCreate(&e), done);
    double pc[256]; hlala_host::filter_phred_table(pc);        // the host's exp / log: the device only compares
    FltIn I; memset(&I, 0, sizeof(I)); I.nReads = nr; I.nPos = np; I.nChars = nch; I.P = *prm;
    int32_t *dPosOff, *dPosExon, *dGenoOff; uint8_t *dMapq, *dMate = nullptr, *dChars, *dRev = nullptr; double *dWok, *dPc;
    if((rc = dev_upload(c, tmp, pos->pos_off, (size_t)nr + 1, &dPosOff))) return done(rc);
    if((rc = dev_upload(c, tmp, pos->pos_exon, (size_t)np, &dPosExon))) return done(rc);
    if((rc = dev_upload(c, tmp, pos->pos_mapq, (size_t)np, &dMapq))) return done(rc);
    if(pos->pos_mate && (rc = dev_upload(c, tmp, pos->pos_mate, (size_t)np, &dMate))) return done(rc);
    if((rc = dev_upload(c, tmp, pos->geno_off, (size_t)np + 1, &dGenoOff))) return done(rc);
    if((rc = dev_upload(c, tmp, pos->geno_chars, (size_t)nch, &dChars))) return done(rc);
    if((rc = dev_upload(c, tmp, pos->read_weighted_ok, (size_t)2 * nr, &dWok))) return done(rc);
    if(prm->long_read_strand_filter && (rc = dev_upload(c, tmp, pos->read_reverse, (size_t)2 * nr, &dRev))) return done(rc);
    if((rc = dev_upload(c, tmp, pc, (size_t)256, &dPc))) return done(rc);
    I.posOff = dPosOff; I.posExon = dPosExon; I.posMapq = dMapq; I.posMate = dMate; I.genoOff = dGenoOff; I.genoChars = dChars; I.wok = dWok; I.readReverse = dRev; I.pc = dPc;
    Cn[FC_BYTES_UP] = flt_bytes_up(pos, prm); Cn[FC_BYTES_DOWN] = flt_bytes_down(pos, read_ignored);
    FltWork W; memset(&W, 0, sizeof(W));
    if((rc = dev_alloc(c, tmp, (size_t)np, &W.ok))) return done(rc);
    if((rc = dev_alloc(c, tmp, (size_t)np, &W.posRead))) return done(rc);
    if((rc = dev_alloc(c, tmp, (size_t)np, &W.key))) return done(rc);
    if((rc = dev_alloc(c, tmp, (size_t)np, &W.val))) return done(rc);
    if((rc = dev_alloc(c, tmp, (size_t)np, &W.sorted))) return done(rc);
    if((rc = dev_alloc(c, tmp, (size_t)np, &W.entRep))) return done(rc);
    if((rc = dev_alloc(c, tmp, (size_t)np, &W.entIgnore, true))) return done(rc);
    if((rc = dev_alloc(c, tmp, (size_t)np, &W.posFlag, true))) return done(rc);
    if((rc = dev_alloc(c, tmp, (size_t)np, &W.posUse))) return done(rc);
    if((rc = dev_alloc(c, tmp, (size_t)nr, &W.kicked, true))) return done(rc);
    if((rc = dev_alloc(c, tmp, (size_t)nr, &W.kickedRobust, true))) return done(rc);
    if((rc = dev_alloc(c, tmp, (size_t)nr, &W.ignoreRead, true))) return done(rc);
    if((rc = dev_alloc(c, tmp, (size_t)FS_N, &W.stats, true))) return done(rc);
    if((rc = dev_alloc(c, tmp, (size_t)FM_N, &W.misc, true))) return done(rc);
    u32 misc[FM_N];
    auto read_misc = [&]() -> int {
        HIP_TRY(c, hipMemcpyAsync(misc, W.misc, sizeof(misc), hipMemcpyDeviceToHost, c->active)); HIP_TRY(c, hipStreamSynchronize(c->active));
        if(misc[FM_BAD]) { c->err = std::string("hlala_filter_positions_gpu: ") + flt_bad_text(misc[FM_BAD]); return HLALA_E_ARG; }
        return HLALA_OK;
    };
    mark(0);
    hipLaunchKernelGGL(k_flt_mapq, dim3(((nr > np ? nr : np) + 255u) / 256u), dim3(256), 0, c->active, I, W);
    if((rc = check_launch(c, "k_flt_mapq"))) return done(rc);
    if((rc = read_misc())) return done(rc);
    const u32 nb = misc[FM_NB];                                 // exon positions up to the last one with an entry; 0: no position passed the mapq test
    u32 nOK = 0;
    if(nb > (1u << 26)) { c->err = "not available: hlala_filter_positions_gpu takes exon positions below 2^26, the locus has one of " + std::to_string(nb - 1); return done(HLALA_E_CAPACITY); }
    if(nb > 0) {
        if((rc = dev_alloc(c, tmp, (size_t)nb + 1, &W.hist, true))) return done(rc);
        if((rc = dev_alloc(c, tmp, (size_t)nb + 1, &W.bOff))) return done(rc);
        hipLaunchKernelGGL(k_flt_keys, dim3((np + 255u) / 256u), dim3(256), 0, c->active, I, W, nb);
        hipLaunchKernelGGL(k_flt_largest, dim3((nb + 255u) / 256u), dim3(256), 0, c->active, W, nb);
        if((rc = check_launch(c, "k_flt_keys / k_flt_largest"))) return done(rc);
        mark(1);
        int bits = 1; while(bits < 32 && (nb >> bits)) bits++;
        size_t cubSort = 0, cubScan = 0; void* dCub = nullptr; u32* dKeyOut = nullptr;
        if((rc = dev_alloc(c, tmp, (size_t)np, &dKeyOut))) return done(rc);
        HIP_TRY_F(c, hipcub::DeviceRadixSort::SortPairs(nullptr, cubSort, (const u32*)W.key, dKeyOut, (const u32*)W.val, W.sorted, (int)np, 0, bits, c->active), done);
        HIP_TRY_F(c, hipcub::DeviceScan::ExclusiveSum(nullptr, cubScan, (const u32*)W.hist, W.bOff, (int)(nb + 1), c->active), done);
        const size_t cubBytes = cubSort > cubScan ? cubSort : cubScan;
        { unsigned char* q = nullptr; if((rc = dev_alloc(c, tmp, cubBytes ? cubBytes : 1, &q))) return done(rc); dCub = q; }
        size_t cb = cubBytes;
        HIP_TRY_F(c, hipcub::DeviceRadixSort::SortPairs(dCub, cb, (const u32*)W.key, dKeyOut, (const u32*)W.val, W.sorted, (int)np, 0, bits, c->active), done);
        cb = cubBytes;
        HIP_TRY_F(c, hipcub::DeviceScan::ExclusiveSum(dCub, cb, (const u32*)W.hist, W.bOff, (int)(nb + 1), c->active), done);
        HIP_TRY_F(c, hipMemcpyAsync(&nOK, W.bOff + nb, sizeof(u32), hipMemcpyDeviceToHost, c->active), done);
        if((rc = read_misc())) return done(rc);
        Cn[FC_BUCKETS] = misc[FM_BUCKETS]; Cn[FC_LARGEST] = misc[FM_LARGEST];
        if(misc[FM_LARGEST] > FLT_MAX_BUCKET) {
            c->err = "not available: an exon position with " + std::to_string(misc[FM_LARGEST]) + " entries, more than HLALA_FILTER_GPU_MAX_BUCKET = " + std::to_string(FLT_MAX_BUCKET);
            return done(HLALA_E_CAPACITY);
        }
        if(nOK > np) { c->err = "hlala_filter_positions_gpu: the buckets hold more entries than there are positions"; return done(HLALA_E_DEVICE); }
    }
    const u32 cap = ((misc[FM_LARGEST] + 63u) / 64u) * 64u;     // LDS of the bucket kernels: what the largest bucket needs
    mark(2);
    if(nb > 0 && nOK > 0) {
        hipLaunchKernelGGL(k_flt_first20, dim3(nb), dim3(64), flt_lds_bytes(cap), c->active, I, W, nb, cap);
        if((rc = check_launch(c, "k_flt_first20"))) return done(rc);
    }
    mark(3);
    if(prm->filter_first20) {
        hipLaunchKernelGGL(k_flt_reads, dim3((nr + 255u) / 256u), dim3(256), 0, c->active, I, W);
        if((rc = check_launch(c, "k_flt_reads"))) return done(rc);
    }
    mark(4);
    if(nb > 0 && nOK > 0) {
        hipLaunchKernelGGL(k_flt_coverage, dim3(nb), dim3(64), flt_lds_bytes(cap), c->active, I, W, nb, cap);
        if((rc = check_launch(c, "k_flt_coverage"))) return done(rc);
    }
    mark(5);
    if(np > 0) {
        hipLaunchKernelGGL(k_flt_use, dim3((np + 255u) / 256u), dim3(256), 0, c->active, I, W, nOK);
        if((rc = check_launch(c, "k_flt_use"))) return done(rc);
    }
    mark(6);
    unsigned long long S[FS_N];
    HIP_TRY_F(c, hipMemcpyAsync(S, W.stats, sizeof(S), hipMemcpyDeviceToHost, c->active), done);
    if((rc = read_misc())) return done(rc);                     // (nothing of the caller's has been written yet)
    Cn[FC_SORTED] = misc[FM_SORTED]; Cn[FC_HEAPS] = misc[FM_HEAPS];
    if(np > 0) HIP_TRY_F(c, hipMemcpyAsync(pos_use, W.posUse, (size_t)np, hipMemcpyDeviceToHost, c->active), done);
    if(read_ignored) HIP_TRY_F(c, hipMemcpyAsync(read_ignored, W.ignoreRead, (size_t)nr, hipMemcpyDeviceToHost, c->active), done);
    HIP_TRY_F(c, hipStreamSynchronize(c->active), done);
    if(c->flt_timed) for(int k = 0; k < 6; k++) { float ms = 0; if(hipEventElapsedTime(&ms, ev[k], ev[k + 1]) == hipSuccess) c->flt_ms[k] = ms; }
    if(stats) { int64_t* o = (int64_t*)stats; for(int k = 0; k < FS_N; k++) o[k] = (int64_t)S[k]; }
    if(counts) memcpy(counts, Cn, sizeof(Cn));
    return done(HLALA_OK);
}
// the launches of the last hlala_filter_positions_gpu as the header lists them (zeros when that call was not timed); enable: whether the next calls are timed
extern "C" int hlala_filter_gpu_times(hlala_ctx* c, int enable, double* ms)
{
    if(!c) return HLALA_E_ARG;
    if(ms) memcpy(ms, c->flt_ms, sizeof(c->flt_ms));
    c->flt_timed = enable != 0;
    return HLALA_OK;
}

// ---- known-answer kernels
namespace hlala {
__global__ void k_kat_phred(const DevTables* T, int n, const double* p, uint8_t* out)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if(i < n) out[i] = phred_from_pcorrect(*T, p[i]);
}
__global__ void k_kat_rand(int n, u32* seeds, int* vals)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if(i < n) { unsigned int s = seeds[i]; vals[i] = glibc_rand_r(&s); seeds[i] = s; }
}
__global__ void k_kat_exp(int n, const double* x, double* y)
{
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if(i < n) y[i] = exp_cr_nonpos(x[i]);
}
}  // namespace hlala

// HLALA_DEBUG=1: the debug buffer of the context (8192 ints in device memory, copied out here); clear != 0 zeroes it afterwards
extern "C" int hlala_debug_buffer(hlala_ctx* c, int* out8192, int clear)
{
    if(!c || !c->dbg_host) return HLALA_E_STATE;
    DEV_GUARD(c);
    HIP_TRY(c, hipStreamSynchronize(c->active));
    if(out8192) HIP_TRY(c, hipMemcpy(out8192, c->dbg_host, 8192 * sizeof(int), hipMemcpyDeviceToHost));
    if(clear) HIP_TRY(c, hipMemset(c->dbg_host, 0, 8192 * sizeof(int)));
    return HLALA_OK;
}

extern "C" int hlala_debug_counters(hlala_ctx* c, hlala_batch* b, unsigned long long* out32)
{
    DEV_GUARD(c);
    ReaderScope rscope_(c, b); if(rscope_.rc) return rscope_.rc;
    if(!c || !b || !out32) return HLALA_E_ARG;
    if(!b->outputs_ready) { memset(out32, 0, 32 * sizeof(u64)); return HLALA_OK; }      // only uploaded so far: the counters do not exist yet
    HIP_TRY(c, hipStreamSynchronize(c->active));
    HIP_TRY(c, hipMemcpyAsync(out32, b->B.counters, 32 * sizeof(u64), hipMemcpyDeviceToHost, c->active)); HIP_TRY(c, hipStreamSynchronize(c->active));
    return HLALA_OK;
}

// device memory of a batch and of its context (diagnostics; bench.py reports them): out[0] = bytes of the batch's blocks (inputs + outputs, pool size classes included),
// out[1] = chains that hold column rows (batch.h: chain_row; n_chains when every chain does), out[2] = bytes parked in the context's pool, out[3] = bytes of every block the
// context has handed out or parked (graph, tables, slabs, batches)
extern "C" int hlala_debug_memory(hlala_ctx* c, hlala_batch* b, unsigned long long* out4)
{
    if(!c || !out4) return HLALA_E_ARG;
    out4[0] = out4[1] = 0;
    if(b) {
        for(void* p : b->allocs) { auto it = c->block_bytes.find(p); if(it != c->block_bytes.end()) out4[0] += it->second; }
        out4[1] = (unsigned long long)(b->prepared ? b->B.n_rows : b->B.n_chains);
    }
    out4[2] = c->pool_bytes; out4[3] = 0;
    for(auto& kv : c->block_bytes) out4[3] += kv.second;
    return HLALA_OK;
}

// the batch's work counters (diagnostics: item counts of the lists, fail-over reasons of the band kernel -- batch.h)
extern "C" int hlala_debug_work_counters(hlala_ctx* c, hlala_batch* b, int* out, int capacity)
{
    static_assert(WC_N >= HLALA_DEBUG_WC_N && WC_BAND_FETCH == HLALA_DEBUG_WC_BAND_FETCH && WC_BAND_WHY == HLALA_DEBUG_WC_BAND_WHY && WC_BAND_TIED == HLALA_DEBUG_WC_BAND_TIED && WC_BAND_NODES == HLALA_DEBUG_WC_BAND_NODES, "include/hlala_gpu.h: debug section");
    DEV_GUARD(c);
    ReaderScope rscope_(c, b); if(rscope_.rc) return rscope_.rc;
    if(!c || !b || !out || capacity < 0) return HLALA_E_ARG;
    const int n = capacity < HLALA_DEBUG_WC_N ? capacity : HLALA_DEBUG_WC_N;          // (a caller built against an older header gets the counters it has room for; the counters behind the exported ones are the kernels' own)
    if(!b->outputs_ready) { memset(out, 0, (size_t)n * sizeof(int)); return HLALA_OK; }
    HIP_TRY(c, hipStreamSynchronize(c->active));
    HIP_TRY(c, hipMemcpyAsync(out, b->B.work_counter, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, c->active)); HIP_TRY(c, hipStreamSynchronize(c->active));
    return HLALA_OK;
}

// diagnostics (tools/tier_predict.py): the DP items of the batch's last extension stage ([2 * n_chains] records of 8 ints: item, read offset, read length, start offset,
// start level, start node, class | steps of the band run << 8, start position on the node path; item < 0: no call) and its retry lists ([16 * n_chains] slots of dp_items; counts in the work counters)
extern "C" int hlala_debug_dp_items(hlala_ctx* c, hlala_batch* b, int* items_out, long long items_capacity_bytes, int* retry_out, long long retry_capacity_bytes)
{
    DEV_GUARD(c);
    ReaderScope rscope_(c, b); if(rscope_.rc) return rscope_.rc;
    if(!c || !b) return HLALA_E_ARG;
    if(!b->outputs_ready || !(b->staged & 2)) { c->err = "hlala_debug_dp_items before the extension stage"; return HLALA_E_STATE; }
    const size_t nc = (size_t)b->B.n_chains;
    if((items_out && items_capacity_bytes < (long long)(2 * nc * 32)) || (retry_out && retry_capacity_bytes < (long long)(16 * nc * sizeof(int)))) {
        c->err = "hlala_debug_dp_items: buffer too small (items 64 bytes per chain, retry lists 64 bytes per chain)"; return HLALA_E_ARG; }
    if(items_out) HIP_TRY(c, hipMemcpyAsync(items_out, b->B.dp_items, 2 * nc * 32, hipMemcpyDeviceToHost, c->active));
    if(retry_out) HIP_TRY(c, hipMemcpyAsync(retry_out, b->B.retry_list, 16 * nc * sizeof(int), hipMemcpyDeviceToHost, c->active));
    HIP_TRY(c, hipStreamSynchronize(c->active));
    return HLALA_OK;
}

extern "C" int hlala_kat_phred(hlala_ctx* c, int n, const double* p_correct, uint8_t* phred_out, const uint8_t* phred_in, double* p_out)
{
    DEV_GUARD(c);
    if(!c || n < 0) return HLALA_E_ARG;
    if(p_correct && phred_out && n) {
        double* dp = nullptr; uint8_t* dq = nullptr; std::vector<void*> tmp;
        int rc = dev_upload(c, tmp, p_correct, (size_t)n, &dp); if(rc) return rc;
        rc = dev_alloc(c, tmp, (size_t)n, &dq); if(rc) return rc;
        hipLaunchKernelGGL(k_kat_phred, dim3((n + 255) / 256), dim3(256), 0, c->active, c->dT, n, dp, dq);
        HIP_TRY(c, hipMemcpyAsync(phred_out, dq, (size_t)n, hipMemcpyDeviceToHost, c->active));
        HIP_TRY(c, hipStreamSynchronize(c->active));
        for(void* p : tmp) pool_release(c, p);
    }
    if(phred_in && p_out) {
        // PhredToPCorrect feeds the host-built likelihood tables: report the table entries' pre-image
        for(int i = 0; i < n; i++) p_out[i] = host_PhredToPCorrect(phred_in[i]);
    }
    return HLALA_OK;
}

// ---- the order of the pair table on the device (kernel_callorder.hip; call_order_core.h; std::sort + std::reverse on the host is the specification)
// dLL / dMA: the tables on the device, n entries; dOrder: n indices on the device.  Everything runs on c->active.  HLALA_OK: dOrder written.  HLALA_E_CAPACITY: "not
// available" -- Cn[OC_PATH] and `why` say which way -- and dOrder not written.  Anything else is an error of the device.  Cn: the eight counters, always filled.
static int order_on_device(hlala_ctx* c, long long n, const double* dLL, const double* dMA, int* dOrder, int64_t* Cn, std::string* why)
{
    using namespace hlala_order;
    for(int k = 0; k < OC_N; k++) Cn[k] = 0;
    for(double& m : c->ord_ms) m = 0;
    std::vector<void*> tmp;
    hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    auto done = [&](int r) { (void)hipStreamSynchronize(c->active); for(void* p : tmp) pool_release(c, p); for(hipEvent_t e : ev) if(e) (void)hipEventDestroy(e); return r; };
    auto mark = [&](int k) { if(c->ord_timed && ev[k]) (void)hipEventRecord(ev[k], c->active); };
    auto refuse = [&](int path, const std::string& text) { Cn[OC_PATH] = path; *why = "not available: " + text; return done(HLALA_E_CAPACITY); };
    if(c->ord_timed) for(hipEvent_t& e : ev) HIP_TRY_F(c, hipEventCreate(&e), done);
    const u32 un = (u32)n;
    const size_t capNext = (size_t)(n / ORD_TILE + 1), capTiles = (size_t)ord_list_capacity((uint64_t)n), capHeaps = (size_t)(n / ORD_TILE + 1);
    OrdEl* dA = nullptr; u32 *dI = nullptr, *dJ = nullptr, *dCnt = nullptr; OrdRange *dCur = nullptr, *dNext = nullptr, *dTiles = nullptr, *dHeaps = nullptr;
    if(dev_alloc(c, tmp, (size_t)n, &dA) || dev_alloc(c, tmp, (size_t)n, &dI) || dev_alloc(c, tmp, (size_t)n, &dJ) || dev_alloc(c, tmp, capNext, &dCur) || dev_alloc(c, tmp, capNext, &dNext) ||
       dev_alloc(c, tmp, capTiles, &dTiles) || dev_alloc(c, tmp, capHeaps, &dHeaps) || dev_alloc(c, tmp, (size_t)OD_N, &dCnt, true)) {
        (void)hipGetLastError();
        return refuse(HLALA_CALL_ORDER_REFUSED_ALLOC, "no device scratch for the order of " + std::to_string(n) + " pairs (" + c->err + ")");
    }
    u32 cnt[OD_N];
    auto read_counters = [&]() -> int {
        HIP_TRY(c, hipMemcpyAsync(cnt, dCnt, sizeof(cnt), hipMemcpyDeviceToHost, c->active)); HIP_TRY(c, hipStreamSynchronize(c->active));
        Cn[OC_BYTES_DOWN] += (int64_t)sizeof(cnt);
        if(cnt[OD_OVERFLOW]) { c->err = "the order of the pair table: a list or a stack of the device path overflowed (" + std::to_string(cnt[OD_OVERFLOW]) + ")"; return HLALA_E_DEVICE; }
        return HLALA_OK;
    };
    int rc = 0;
    mark(0);
    { const u32 g = (un + 255u) / 256u; hipLaunchKernelGGL(k_ord_load, dim3(g < 4096u ? g : 4096u), dim3(256), 0, c->active, un, dLL, dMA, dA, dCnt); }
    OrdLists Ls; Ls.tiles = dTiles; Ls.heaps = dHeaps; Ls.capNext = (u32)capNext; Ls.capTiles = (u32)capTiles; Ls.capHeaps = (u32)capHeaps;
    Ls.next = dCur;
    hipLaunchKernelGGL(k_ord_root, dim3(1), dim3(64), 0, c->active, un, Ls, dCnt);
    if((rc = check_launch(c, "k_ord_load / k_ord_root"))) return done(rc);
    mark(1);
    if((rc = read_counters())) return done(rc);
    if(cnt[OD_NAN]) return refuse(HLALA_CALL_ORDER_REFUSED_NAN, "a NaN among the keys of " + std::to_string(n) + " pairs: std::sort is undefined there");
    for(u32 nCur = cnt[OD_NEXT]; nCur > 0; nCur = cnt[OD_NEXT]) {
        if(nCur > capNext || Cn[OC_LEVELS] > 2 * 64) { c->err = "the order of the pair table: the list of a level is inconsistent"; return done(HLALA_E_DEVICE); }
        Cn[OC_LEVELS]++;
        HIP_TRY_F(c, hipMemsetAsync(dCnt + OD_NEXT, 0, sizeof(u32), c->active), done);
        Ls.next = dNext;
        hipLaunchKernelGGL(k_ord_level, dim3(nCur), dim3(ORD_BLOCK), 0, c->active, dA, dI, dJ, (const OrdRange*)dCur, Ls, dCnt);
        if((rc = check_launch(c, "k_ord_level"))) return done(rc);
        if((rc = read_counters())) return done(rc);
        std::swap(dCur, dNext);
    }
    mark(2);
    Cn[OC_TILE_RANGES] = cnt[OD_TILES]; Cn[OC_LARGEST_TILE] = cnt[OD_LARGEST_TILE];
    if(cnt[OD_REFUSED]) {
        Cn[OC_HEAPS] = cnt[OD_HEAPS]; Cn[OC_LARGEST_HEAP] = cnt[OD_LARGEST_HEAP];
        return refuse(HLALA_CALL_ORDER_REFUSED_HEAP, "of " + std::to_string(n) + " pairs a range of " + std::to_string(cnt[OD_LARGEST_HEAP]) +
                      " was met with no depth left, more than HLALA_CALL_ORDER_MAX_HEAP = " + std::to_string(ORD_MAX_HEAP));
    }
    if(cnt[OD_TILES] > capTiles || cnt[OD_HEAPLIST] > capHeaps) { c->err = "the order of the pair table: a list is inconsistent"; return done(HLALA_E_DEVICE); }
    if(cnt[OD_TILES]) hipLaunchKernelGGL((k_ord_tile<ORD_TILE>), dim3(cnt[OD_TILES]), dim3(64), 0, c->active, dA, (const OrdRange*)dTiles, dCnt);
    if(cnt[OD_HEAPLIST]) hipLaunchKernelGGL((k_ord_tile<ORD_MAX_HEAP>), dim3(cnt[OD_HEAPLIST]), dim3(64), 0, c->active, dA, (const OrdRange*)dHeaps, dCnt);
    mark(3);
    hipLaunchKernelGGL(k_ord_emit, dim3((un + 255u) / 256u), dim3(256), 0, c->active, un, (const OrdEl*)dA, dOrder);
    if((rc = check_launch(c, "k_ord_tile / k_ord_emit"))) return done(rc);
    mark(4);
    if((rc = read_counters())) return done(rc);
    Cn[OC_HEAPS] = cnt[OD_HEAPS]; Cn[OC_LARGEST_HEAP] = cnt[OD_LARGEST_HEAP];
    Cn[OC_PATH] = HLALA_CALL_ORDER_DEVICE;
    if(c->ord_timed) for(int k = 0; k < 4; k++) { float ms = 0; if(hipEventElapsedTime(&ms, ev[k], ev[k + 1]) == hipSuccess) c->ord_ms[k] = ms; }
    return done(HLALA_OK);
}
extern "C" int hlala_set_call_order_gpu(hlala_ctx* c, int on)
{
    if(!c) return HLALA_E_ARG;
    c->ord_gpu = on != 0;
    return HLALA_OK;
}
extern "C" int hlala_call_order_counts(hlala_ctx* c, int64_t* counts)
{
    if(!c || !counts) return HLALA_E_ARG;
    memcpy(counts, c->ord_counts, sizeof(c->ord_counts));
    return HLALA_OK;
}
extern "C" int hlala_call_order_times(hlala_ctx* c, int enable, double* ms)
{
    if(!c) return HLALA_E_ARG;
    if(ms) memcpy(ms, c->ord_ms, sizeof(c->ord_ms));
    c->ord_timed = enable != 0;
    return HLALA_OK;
}
extern "C" int hlala_pair_order_gpu(hlala_ctx* c, int64_t n, const double* ll, const double* ma, int32_t* order, int64_t* counts)
{
    DEV_GUARD(c);
    ReaderScope rscope_(c, nullptr);
    if(!c) return HLALA_E_ARG;
    if(n < 1 || n >= ((int64_t)1 << 31) || !ll || !ma || !order) { c->err = "hlala_pair_order_gpu: n outside [1, 2^31) or a null pointer"; return HLALA_E_ARG; }
    std::vector<void*> tmp;
    auto done = [&](int r) { (void)hipStreamSynchronize(c->active); for(void* p : tmp) pool_release(c, p); return r; };
    double *dLL = nullptr, *dMA = nullptr; int* dOrder = nullptr; int rc = 0;
    if((rc = dev_upload(c, tmp, ll, (size_t)n, &dLL)) || (rc = dev_upload(c, tmp, ma, (size_t)n, &dMA)) || (rc = dev_alloc(c, tmp, (size_t)n, &dOrder))) return done(rc);
    std::string why;
    rc = order_on_device(c, n, dLL, dMA, dOrder, c->ord_counts, &why);
    c->ord_counts[hlala_order::OC_BYTES_UP] = 16 * n;
    if(rc == HLALA_OK) {
        HIP_TRY_F(c, hipMemcpyAsync(order, dOrder, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, c->active), done);
        HIP_TRY_F(c, hipStreamSynchronize(c->active), done);
        c->ord_counts[hlala_order::OC_BYTES_DOWN] += 4 * n;
    } else if(rc == HLALA_E_CAPACITY) c->err = why;
    if(counts) memcpy(counts, c->ord_counts, sizeof(c->ord_counts));
    return done(rc);
}

static int call_locus_impl(hlala_ctx* c, int32_t C, const double* pairLL, const double* misAvg, const double* misMin, const double* dLLin, const double* dMAin, const double* dMMin,
                          int32_t* order, double* p_normalized, double* cluster_marginal, hlala_call_out* out)
{
    if(!c || C < 1 || !pairLL || !misAvg || (!dLLin && !misMin) || !out) return HLALA_E_ARG;
    if(C > 46000) { c->err = "hlala_call_locus: more than 46000 clusters (pair index exceeds 31 bits)"; return HLALA_E_CAPACITY; }
    const long long nP = (long long)C * (C + 1) / 2, n2 = 2 * nP;
    std::vector<void*> tmp;
    auto done = [&](int r_) { for(void* p : tmp) pool_release(c, p); return r_; };       // scratch is parked for the next locus
    int rc = 0;
    double *dLL = nullptr, *dMA = nullptr, *dMM = nullptr, *dP = nullptr, *dPart = nullptr, *dScal = nullptr, *dVal = nullptr, *dVal2 = nullptr, *dMarg = nullptr;
    u64 *dCK = nullptr, *dCK2 = nullptr; int *dI1 = nullptr, *dC1 = nullptr, *dC2 = nullptr, *dTies = nullptr;
    long long* dPidx = nullptr; hlala_call_out* dOut = nullptr;
    const int NB = 1024;
    if(dLLin) { dLL = const_cast<double*>(dLLin); dMA = const_cast<double*>(dMAin); dMM = const_cast<double*>(dMMin); }
    else if((rc = dev_upload(c, tmp, pairLL, (size_t)nP, &dLL)) || (rc = dev_upload(c, tmp, misAvg, (size_t)nP, &dMA)) || (rc = dev_upload(c, tmp, misMin, (size_t)nP, &dMM))) return done(rc);
    if((rc = dev_alloc(c, tmp, (size_t)nP, &dP)) || (rc = dev_alloc(c, tmp, (size_t)NB, &dPart)) || (rc = dev_alloc(c, tmp, (size_t)NB, &dPidx)) || (rc = dev_alloc(c, tmp, 4, &dScal)) ||
       (rc = dev_alloc(c, tmp, (size_t)nP, &dI1)) ||
       (rc = dev_alloc(c, tmp, (size_t)nP, &dC1)) || (rc = dev_alloc(c, tmp, (size_t)nP, &dC2)) || (rc = dev_alloc(c, tmp, (size_t)n2, &dCK)) || (rc = dev_alloc(c, tmp, (size_t)n2, &dCK2)) ||
       (rc = dev_alloc(c, tmp, (size_t)n2, &dVal)) || (rc = dev_alloc(c, tmp, (size_t)n2, &dVal2)) || (rc = dev_alloc(c, tmp, (size_t)C, &dMarg)) || (rc = dev_alloc(c, tmp, 1, &dTies, true)) ||
       (rc = dev_alloc(c, tmp, 1, &dOut))) return done(rc);
    long long* dMaxIdx = (long long*)(dScal + 2);      // dScal[0] = LL max, dScal[1] = P sum, dScal[2..3] as one long long = index of the maximum
    hipStream_t st = c->active;
    const int T = 256; const unsigned gP = (unsigned)((nP + T - 1) / T);
    hipLaunchKernelGGL(k_call_max, dim3(NB), dim3(T), 0, st, dLL, nP, dPart, dPidx);
    hipLaunchKernelGGL(k_call_max_final, dim3(1), dim3(1), 0, st, dPart, dPidx, NB, dScal, dMaxIdx);
    hipLaunchKernelGGL(k_call_p, dim3(NB), dim3(T), 0, st, dLL, nP, dScal, dP, dPart);
    hipLaunchKernelGGL(k_call_psum_final, dim3(1), dim3(1), 0, st, dPart, NB, dScal + 1);
    hipLaunchKernelGGL(k_call_normalize, dim3(gP), dim3(T), 0, st, dP, nP, dScal + 1);
    // order: the reference's own two library calls -- std::sort with its comparator, then std::reverse (hla/HLATyper.cpp:2381-2403) -- on the HOST.  Pairs equal in both
    // keys come out in the order libstdc++'s std::sort leaves them in, which depends on every comparison it makes on the way over the whole sequence: only the same routine
    // over the same sequence reproduces it, and R1_PP_<locus>_pairs.txt prints that order (through the accumulation order of the marginals below, the call on exactly tied
    // marginals depends on it too).  A stable device sort agrees with the reference everywhere except inside such groups, which is where the reference pin of the typer found
    // it (tests/test_gpu_reference_pin_typer.py).  The tables the sort reads are the caller's (hlala_call_locus: it then runs beside the kernels queued above) or the host
    // copies hlala_type_locus has queued; those have to have arrived, so that path drains the stream first and nothing overlaps.  One thread, nP log nP comparisons
    // (DESIGN.md section D-H has the measured time).  The elements carry their keys: std::sort's sequence of comparisons and moves does not depend on the element type, so
    // the permutation is the one the reference's sort of bare indices produces, at half the time of looking the keys up through the index; 24 bytes per pair of host memory.
    // With hlala_set_call_order_gpu the same order is made on the device from the tables that are there already (kernel_callorder.hip: the library's steps level by
    // level); where that path answers "not available" the host path below runs on the same call, and the counters say why.
    bool ordered = false;
    if(c->ord_gpu) {
        std::string why;
        rc = order_on_device(c, nP, dLL, dMA, dI1, c->ord_counts, &why);
        if(rc == HLALA_OK) ordered = true;
        else if(rc != HLALA_E_CAPACITY) return done(rc);
    } else for(int64_t& k : c->ord_counts) k = 0;
    if(!ordered) {
    if(dLLin) HIP_TRY_F(c, hipStreamSynchronize(st), done);
    struct Keyed { double ll, ma; int32_t i; };
    std::vector<Keyed> keyed; std::vector<int32_t> hOrder;
    try { keyed.resize((size_t)nP); hOrder.resize((size_t)nP); } catch(const std::exception&) { c->err = "hlala_call_locus: no host memory for the order of the pair table"; return done(HLALA_E_CAPACITY); }
    for(long long i = 0; i < nP; i++) keyed[(size_t)i] = Keyed{pairLL[i], misAvg[i], (int32_t)i};
    std::sort(keyed.begin(), keyed.end(), [](const Keyed& a, const Keyed& b) {
        if(a.ll == b.ll) return (b.ma < a.ma);
        else return (a.ll < b.ll);
    });
    std::reverse(keyed.begin(), keyed.end());
    for(long long i = 0; i < nP; i++) hOrder[(size_t)i] = keyed[(size_t)i].i;
    HIP_TRY_F(c, hipMemcpyAsync(dI1, hOrder.data(), (size_t)nP * sizeof(int32_t), hipMemcpyHostToDevice, st), done);
    HIP_TRY_F(c, hipStreamSynchronize(st), done);                                                                            // (hOrder is a local)
    c->ord_counts[hlala_order::OC_BYTES_UP] = 4 * nP;
    }
    size_t cubBytes = 0;
    HIP_TRY_F(c, hipcub::DeviceRadixSort::SortPairs(nullptr, cubBytes, dCK, dCK2, dVal, dVal2, (int)n2, 0, 64, st), done);
    char* dCub = nullptr; if((rc = dev_alloc(c, tmp, cubBytes ? cubBytes : 1, &dCub))) return done(rc);
    // marginals in the reference's accumulation order
    hipLaunchKernelGGL(k_call_clusters, dim3((unsigned)C), dim3(128), 0, st, (int)C, dC1, dC2);
    hipLaunchKernelGGL(k_call_contrib, dim3(gP), dim3(T), 0, st, dI1, dC1, dC2, dP, nP, dCK, dVal, dTies, dLL, dMA);
    HIP_TRY_F(c, hipcub::DeviceRadixSort::SortPairs(dCub, cubBytes, dCK, dCK2, dVal, dVal2, (int)n2, 0, 64, st), done);
    hipLaunchKernelGGL(k_call_marginals, dim3((unsigned)((C + 63) / 64)), dim3(64), 0, st, dCK2, dVal2, n2, (int)C, dMarg);
    hipLaunchKernelGGL(k_call_decide, dim3(1), dim3(64), 0, st, (int)C, dMarg, dP, dMM, dScal, dMaxIdx, dTies, dOut);
    rc = check_launch(c, "hlala_call_locus kernels"); if(rc) return done(rc);
    if((rc = dl(c, order, dI1, (size_t)nP)) || (rc = dl(c, p_normalized, dP, (size_t)nP)) || (rc = dl(c, cluster_marginal, dMarg, (size_t)C)) || (rc = dl(c, out, dOut, 1))) return done(rc);
    HIP_TRY_F(c, hipStreamSynchronize(st), done);
    return done(HLALA_OK);
}
extern "C" int hlala_call_locus(hlala_ctx* c, int32_t C, const double* pairLL, const double* misAvg, const double* misMin,
                                int32_t* order, double* p_normalized, double* cluster_marginal, hlala_call_out* out)
{
    DEV_GUARD(c);
    ReaderScope rscope_(c, nullptr);
    if(!c || !pairLL || !misAvg || !misMin) return HLALA_E_ARG;
    return call_locus_impl(c, C, pairLL, misAvg, misMin, nullptr, nullptr, nullptr, order, p_normalized, cluster_marginal, out);
}

// hlala_exon_loglik -> hlala_pair_loglik -> hlala_call_locus with the tables left on the device in between: the per-read table (clusters x reads) is neither
// downloaded nor uploaded again, the all-pairs tables go down once (the caller's files need them) and are not uploaded for the call.
extern "C" int hlala_type_locus(hlala_ctx* c, const hlala_exon_in* in, double* LL, int32_t* mism, double* pairLL, double* misAvg, double* misMin,
                                int32_t* order, double* p_normalized, double* cluster_marginal, hlala_call_out* out)
{
    DEV_GUARD(c);
    ReaderScope rscope_(c, nullptr);
    if(!c || !in || !pairLL || !misAvg || !misMin || !order || !p_normalized || !cluster_marginal || !out) return HLALA_E_ARG;
    if(in->n_clusters < 1) { c->err = "hlala_type_locus: no clusters"; return HLALA_E_ARG; }
    std::vector<void*> keep;
    // (the steps run unsynchronised in keep mode: on ANY failure the stream is drained before the kept device blocks go back to the pool and before the caller, who
    //  sees the error, may free the host buffers the queued copies write to)
    auto done = [&](int r_) { if(r_) (void)hipStreamSynchronize(c->active); for(void* p : keep) pool_release(c, p); return r_; };
    const int C = in->n_clusters, R = in->n_reads < 0 ? 0 : in->n_reads;
    double *dLL = nullptr, *dP = nullptr, *dA = nullptr, *dMn = nullptr; int* dM = nullptr;
    int rc = exon_loglik_impl(c, in, LL, mism, &keep, &dLL, &dM); if(rc) return done(rc);
    if(!dLL) {                                                     // no reads at the locus: empty per-read tables (hlala_exon_loglik writes nothing either)
        if((rc = dev_alloc(c, keep, 1, &dLL)) || (rc = dev_alloc(c, keep, 1, &dM))) return done(rc);
    }
    if((rc = pair_loglik_impl(c, nullptr, nullptr, dLL, dM, C, R, pairLL, misAvg, misMin, &keep, &dP, &dA, &dMn))) return done(rc);
    rc = call_locus_impl(c, C, pairLL, misAvg, misMin, dP, dA, dMn, order, p_normalized, cluster_marginal, out);          // (host copies for the sort of the order; ends synchronised)
    return done(rc);
}

extern "C" int hlala_exon_positions(hlala_ctx* c, hlala_batch* b, const hlala_locus_desc* L, hlala_exon_positions_out* o)
{
    DEV_GUARD(c);
    ReaderScope rscope_(c, b); if(rscope_.rc) return rscope_.rc;
    if(!c || !b || !L || !o) return HLALA_E_ARG;
    if(!(b->staged & 4)) { c->err = "hlala_exon_positions before hlala_pair_chains"; return HLALA_E_STATE; }
    if(L->level_max < L->level_min || !L->level_to_exon) { c->err = "locus: empty level range or no level_to_exon table"; return HLALA_E_ARG; }
    DevBatch& B = b->B;
    const int np = B.n_pairs;
    o->n_reads = o->n_pos = o->n_chars = 0; o->n_pairs_ok = o->n_pairs_broken = 0;
    if(np <= 0) { if(o->pos_off && o->cap_reads >= 0) o->pos_off[0] = 0; if(o->geno_off && o->cap_pos >= 0) o->geno_off[0] = 0; return HLALA_OK; }
    std::vector<void*> tmp;
    auto done = [&](int r_) { for(void* p : tmp) pool_release(c, p); return r_; };
    int rc = 0;
    ExonLocus EL; EL.level_min = L->level_min; EL.level_max = L->level_max; EL.insert_mean = L->insert_mean; EL.insert_sd = L->insert_sd;
    EL.min_mapq = L->min_mapq; EL.min_weighted_ok = L->min_weighted_ok; EL.level_to_exon = nullptr; EL.pair_mask = nullptr; EL.min_alignment_columns = L->min_alignment_columns;
    int* dL2E = nullptr; uint8_t* dMask = nullptr; int *dCnt = nullptr, *dOff = nullptr, *dOB = nullptr; char* dCub = nullptr;
    if((rc = dev_upload(c, tmp, L->level_to_exon, (size_t)(L->level_max - L->level_min + 1), &dL2E))) return done(rc);
    EL.level_to_exon = dL2E;
    if(L->pair_mask) { if((rc = dev_upload(c, tmp, L->pair_mask, (size_t)np, &dMask))) return done(rc); EL.pair_mask = dMask; }
    if((rc = dev_alloc(c, tmp, (size_t)3 * np + 3, &dCnt)) || (rc = dev_alloc(c, tmp, (size_t)3 * np + 3, &dOff)) || (rc = dev_alloc(c, tmp, 2, &dOB, true))) return done(rc);
    hipStream_t st = c->active;
    hlala_exon_positions_out dO; memset(&dO, 0, sizeof(dO));
    const unsigned grid = (unsigned)((np + 127) / 128);
    hipLaunchKernelGGL((k_exon_positions<0>), dim3(grid), dim3(128), 0, st, b->dB, c->dT, EL, dCnt, (const int*)nullptr, dOB, dO);
    if((rc = check_launch(c, "k_exon_positions<0>"))) return done(rc);
    // interleaved (read, positions, characters) counts -> three exclusive sums in one scan over 3-vectors: scan each column separately
    // with a strided view is not what the library offers, so the counts are de-interleaved by scanning the flat array three times with
    // a transform; simpler and still tiny: one scan over the flat array of a struct of three ints
    struct I3 { int a, b, c; };
    struct I3Add { __host__ __device__ I3 operator()(const I3& x, const I3& y) const { I3 r; r.a = x.a + y.a; r.b = x.b + y.b; r.c = x.c + y.c; return r; } };
    size_t cubBytes = 0; I3 zero; zero.a = zero.b = zero.c = 0;
    HIP_TRY_F(c, hipcub::DeviceScan::ExclusiveScan(nullptr, cubBytes, (I3*)dCnt, (I3*)dOff, I3Add(), zero, np + 1, st), done);
    if((rc = dev_alloc(c, tmp, cubBytes ? cubBytes : 1, &dCub))) return done(rc);
    HIP_TRY_F(c, hipMemsetAsync(dCnt + 3 * (size_t)np, 0, 3 * sizeof(int), st), done);
    HIP_TRY_F(c, hipcub::DeviceScan::ExclusiveScan(dCub, cubBytes, (I3*)dCnt, (I3*)dOff, I3Add(), zero, np + 1, st), done);
    int totals[3] = {0, 0, 0}, ob[2] = {0, 0};
    HIP_TRY_F(c, hipMemcpyAsync(totals, dOff + 3 * (size_t)np, sizeof(totals), hipMemcpyDeviceToHost, st), done);
    HIP_TRY_F(c, hipMemcpyAsync(ob, dOB, sizeof(ob), hipMemcpyDeviceToHost, st), done);
    HIP_TRY_F(c, hipStreamSynchronize(st), done);
    o->n_reads = totals[0]; o->n_pos = totals[1]; o->n_chars = totals[2]; o->n_pairs_ok = ob[0]; o->n_pairs_broken = ob[1];
    if(totals[0] > o->cap_reads || totals[1] > o->cap_pos || totals[2] > o->cap_chars) { c->err = "hlala_exon_positions: output capacity too small (needed sizes are in n_reads / n_pos / n_chars)"; return done(HLALA_E_CAPACITY); }
    const size_t nR = (size_t)totals[0], nPz = (size_t)totals[1], nC = (size_t)totals[2];
    if((rc = dev_alloc(c, tmp, nR, &dO.read_pair)) || (rc = dev_alloc(c, tmp, 2 * nR, &dO.read_weighted_ok)) || (rc = dev_alloc(c, tmp, 2 * nR, &dO.read_fraction_ok)) ||
       (rc = dev_alloc(c, tmp, nR, &dO.read_distance)) || (rc = dev_alloc(c, tmp, 2 * nR, &dO.read_cols_nongap)) || (rc = dev_alloc(c, tmp, nR + 1, &dO.pos_off)) ||
       (rc = dev_alloc(c, tmp, nPz, &dO.pos_exon)) || (rc = dev_alloc(c, tmp, nPz, &dO.pos_level)) || (rc = dev_alloc(c, tmp, nPz, &dO.pos_mate)) || (rc = dev_alloc(c, tmp, nPz, &dO.pos_mapq)) ||
       (rc = dev_alloc(c, tmp, nPz, &dO.pos_novel_gap)) || (rc = dev_alloc(c, tmp, nPz + 1, &dO.geno_off)) || (rc = dev_alloc(c, tmp, nC, &dO.geno_chars)) || (rc = dev_alloc(c, tmp, nC, &dO.qual_chars)) ||
       (rc = dev_alloc(c, tmp, 2 * nR, &dO.read_reverse)) || (rc = dev_alloc(c, tmp, 2 * nR, &dO.read_mapq))) return done(rc);
    hipLaunchKernelGGL((k_exon_positions<1>), dim3(grid), dim3(128), 0, st, b->dB, c->dT, EL, dCnt, (const int*)dOff, dOB, dO);
    if((rc = check_launch(c, "k_exon_positions<1>"))) return done(rc);
    if((rc = dl(c, o->read_pair, dO.read_pair, nR)) || (rc = dl(c, o->read_weighted_ok, dO.read_weighted_ok, 2 * nR)) || (rc = dl(c, o->read_fraction_ok, dO.read_fraction_ok, 2 * nR)) ||
       (rc = dl(c, o->read_distance, dO.read_distance, nR)) || (rc = dl(c, o->read_cols_nongap, dO.read_cols_nongap, 2 * nR)) || (rc = dl(c, o->pos_off, dO.pos_off, nR)) ||
       (rc = dl(c, o->pos_exon, dO.pos_exon, nPz)) || (rc = dl(c, o->pos_level, dO.pos_level, nPz)) || (rc = dl(c, o->pos_mate, dO.pos_mate, nPz)) || (rc = dl(c, o->pos_mapq, dO.pos_mapq, nPz)) ||
       (rc = dl(c, o->pos_novel_gap, dO.pos_novel_gap, nPz)) || (rc = dl(c, o->geno_off, dO.geno_off, nPz)) || (rc = dl(c, o->geno_chars, dO.geno_chars, nC)) || (rc = dl(c, o->qual_chars, dO.qual_chars, nC)) ||
       (rc = dl(c, o->read_reverse, dO.read_reverse, 2 * nR)) || (rc = dl(c, o->read_mapq, dO.read_mapq, 2 * nR))) return done(rc);
    HIP_TRY_F(c, hipStreamSynchronize(st), done);
    if(o->pos_off) o->pos_off[nR] = (int32_t)nPz;
    if(o->geno_off) o->geno_off[nPz] = (int32_t)nC;
    return done(HLALA_OK);
}

extern "C" int hlala_unit_alignment_stats(hlala_ctx* c, hlala_batch* b, hlala_unit_stats_out* o)
{
    DEV_GUARD(c);
    ReaderScope rscope_(c, b); if(rscope_.rc) return rscope_.rc;
    if(!c || !b || !o || !o->valid || !o->strands_valid || !o->distance || !o->fraction_ok || !o->weighted_ok || !o->n_columns || !o->mate_mapq) return HLALA_E_ARG;
    if(!(b->staged & 4)) { c->err = "hlala_unit_alignment_stats before hlala_pair_chains"; return HLALA_E_STATE; }
    const size_t n = (size_t)b->B.n_pairs;
    if(n == 0) return HLALA_OK;
    std::vector<void*> tmp;
    auto done = [&](int r_) { for(void* p : tmp) pool_release(c, p); return r_; };
    int rc = 0; hlala_unit_stats_out d; memset(&d, 0, sizeof(d));
    if((rc = dev_alloc(c, tmp, n, &d.valid)) || (rc = dev_alloc(c, tmp, n, &d.strands_valid)) || (rc = dev_alloc(c, tmp, n, &d.distance)) || (rc = dev_alloc(c, tmp, 2 * n, &d.fraction_ok)) ||
       (rc = dev_alloc(c, tmp, 2 * n, &d.weighted_ok)) || (rc = dev_alloc(c, tmp, 2 * n, &d.n_columns)) || (rc = dev_alloc(c, tmp, 2 * n, &d.mate_mapq))) return done(rc);
    hipLaunchKernelGGL(k_unit_stats, dim3((unsigned)((n + 127) / 128)), dim3(128), 0, c->active, b->dB, c->dT, d);
    if((rc = check_launch(c, "k_unit_stats"))) return done(rc);
    if((rc = dl(c, o->valid, d.valid, n)) || (rc = dl(c, o->strands_valid, d.strands_valid, n)) || (rc = dl(c, o->distance, d.distance, n)) || (rc = dl(c, o->fraction_ok, d.fraction_ok, 2 * n)) ||
       (rc = dl(c, o->weighted_ok, d.weighted_ok, 2 * n)) || (rc = dl(c, o->n_columns, d.n_columns, 2 * n)) || (rc = dl(c, o->mate_mapq, d.mate_mapq, 2 * n))) return done(rc);
    HIP_TRY_F(c, hipStreamSynchronize(c->active), done);
    return done(HLALA_OK);
}

// canonical codes of the query k-mers and the sorted set of the distinct ones; a query with a character outside ACGT cannot occur in a read k-mer over ACGT
static int kmer_queries(hlala_ctx* c, const char* who, int32_t k, int32_t n_queries, const char* queries, std::vector<u64>& canon, std::vector<u64>& uniq)
{
    if(k < 1 || k > 31) { c->err = std::string(who) + ": k must be in 1..31 (2-bit codes in one 64-bit word)"; return HLALA_E_ARG; }
    canon.assign((size_t)n_queries, ~0ull); uniq.clear();
    for(int i = 0; i < n_queries; i++) {
        u64 f = 0, rc = 0; bool ok = true;
        for(int j = 0; j < k; j++) {
            const char ch = queries[(size_t)i * k + j];
            const int cj = ch == 'A' ? 0 : ch == 'C' ? 1 : ch == 'G' ? 2 : ch == 'T' ? 3 : 4;
            if(cj > 3) { ok = false; break; }
            f = (f << 2) | (u64)cj; rc |= (u64)(3 - cj) << (2 * j);
        }
        if(ok) { canon[i] = rc < f ? rc : f; uniq.push_back(canon[i]); }
    }
    std::sort(uniq.begin(), uniq.end()); uniq.erase(std::unique(uniq.begin(), uniq.end()), uniq.end());
    if(uniq.size() > (size_t)hlala::KMER_QCAP) { c->err = std::string(who) + ": more than 4096 distinct query k-mers in one call"; return HLALA_E_CAPACITY; }
    return HLALA_OK;
}

extern "C" int hlala_kmer_presence(hlala_ctx* c, hlala_batch* b, const uint8_t* pair_mask, int32_t k, int32_t n_queries, const char* queries, uint8_t* present)
{
    DEV_GUARD(c);
    ReaderScope rscope_(c, b); if(rscope_.rc) return rscope_.rc;
    if(!c || !b || n_queries < 0 || (n_queries > 0 && (!queries || !present))) return HLALA_E_ARG;
    std::vector<u64> canon, uniq;
    int rc = kmer_queries(c, "hlala_kmer_presence", k, n_queries, queries, canon, uniq); if(rc) return rc;
    if(n_queries == 0) return HLALA_OK;
    memset(present, 0, (size_t)n_queries);
    if(uniq.empty() || b->B.n_pairs <= 0) return HLALA_OK;
    std::vector<void*> tmp;
    auto done = [&](int r_) { for(void* p : tmp) pool_release(c, p); return r_; };
    u64* dQ = nullptr; uint8_t *dP = nullptr, *dMask = nullptr;
    if((rc = dev_upload(c, tmp, uniq.data(), uniq.size(), &dQ)) || (rc = dev_alloc(c, tmp, uniq.size(), &dP, true))) return done(rc);
    if(pair_mask && (rc = dev_upload(c, tmp, pair_mask, (size_t)b->B.n_pairs, &dMask))) return done(rc);
    const int nReads = b->B.unpaired ? b->B.n_pairs : 2 * b->B.n_pairs;
    const unsigned grid = (unsigned)std::min<long long>((long long)nReads, (long long)c->stitch_grid);
    hipLaunchKernelGGL(k_kmer_presence, dim3(grid), dim3(64), 0, c->active, b->dB, (const uint8_t*)dMask, (int)k, (int)uniq.size(), (const u64*)dQ, dP);
    if((rc = check_launch(c, "k_kmer_presence"))) return done(rc);
    std::vector<uint8_t> hp(uniq.size());
    if((rc = dl(c, hp.data(), dP, uniq.size()))) return done(rc);
    HIP_TRY_F(c, hipStreamSynchronize(c->active), done);
    for(int i = 0; i < n_queries; i++) if(canon[i] != ~0ull) present[i] = hp[(size_t)(std::lower_bound(uniq.begin(), uniq.end(), canon[i]) - uniq.begin())];
    return done(HLALA_OK);
}

extern "C" void hlala_kmer_forget_reads(hlala_ctx* c)
{
    if(!c) return;
    DEV_GUARD(c);
    if(!c->kept.empty() && c->rs) (void)hipStreamSynchronize(c->rs);
    for(hlala_ctx::KeptReads& kr : c->kept) { pool_release(c, kr.store); pool_release(c, kr.start); pool_release(c, kr.length); }
    c->kept.clear();
}

extern "C" int hlala_kmer_keep_reads(hlala_ctx* c, hlala_batch* b, const uint8_t* pair_mask, int64_t* n_reads_kept)
{
    DEV_GUARD(c);
    ReaderScope rscope_(c, b); if(rscope_.rc) return rscope_.rc;
    if(!c || !b) return HLALA_E_ARG;
    if(n_reads_kept) *n_reads_kept = 0;
    if(b->B.n_pairs <= 0) return HLALA_OK;
    std::vector<void*> tmp;
    auto done = [&](int r_) { for(void* p : tmp) pool_release(c, p); return r_; };
    int rc = 0; uint8_t* dMask = nullptr; unsigned long long* dTot = nullptr;
    if((rc = dev_alloc(c, tmp, 4, &dTot, true))) return done(rc);
    if(pair_mask && (rc = dev_upload(c, tmp, pair_mask, (size_t)b->B.n_pairs, &dMask))) return done(rc);
    const int nReads = b->B.unpaired ? b->B.n_pairs : 2 * b->B.n_pairs;
    hipLaunchKernelGGL(k_kmer_count_kept, dim3((unsigned)std::min<long long>(((long long)nReads + 255) / 256, 4096)), dim3(256), 0, c->active, b->dB, (const uint8_t*)dMask, dTot);
    if((rc = check_launch(c, "k_kmer_count_kept"))) return done(rc);
    unsigned long long tot[2] = {0, 0};
    if((rc = dl(c, tot, dTot, 2))) return done(rc);
    HIP_TRY_F(c, hipStreamSynchronize(c->active), done);
    if(tot[0] == 0) return done(HLALA_OK);
    hlala_ctx::KeptReads kr; kr.n = (int)tot[0];
    void* p = nullptr;
    if((rc = pool_malloc(c, &p, (size_t)tot[1] + 64))) return done(rc); kr.store = (uint8_t*)p;
    if((rc = pool_malloc(c, &p, (size_t)tot[0] * sizeof(long long)))) { pool_release(c, kr.store); return done(rc); } kr.start = (long long*)p;
    if((rc = pool_malloc(c, &p, (size_t)tot[0] * sizeof(int)))) { pool_release(c, kr.store); pool_release(c, kr.start); return done(rc); } kr.length = (int*)p;
    // (the chunk joins the context's list only once it is filled: a failed launch or copy must not leave an entry with undefined start[] / length[] behind,
    //  which hlala_kmer_presence_kept would index the store with)
    auto drop = [&](int r_) { (void)hipStreamSynchronize(c->active); pool_release(c, kr.store); pool_release(c, kr.start); pool_release(c, kr.length); return done(r_); };
    const unsigned grid = (unsigned)std::min<long long>((long long)nReads, (long long)c->stitch_grid);
    hipLaunchKernelGGL(k_kmer_keep, dim3(grid), dim3(64), 0, c->active, b->dB, (const uint8_t*)dMask, dTot + 2, kr.start, kr.length, kr.store);
    if((rc = check_launch(c, "k_kmer_keep"))) return drop(rc);
    if(hipStreamSynchronize(c->active) != hipSuccess) { c->err = "hlala_kmer_keep_reads: the device reported an error"; return drop(HLALA_E_DEVICE); }      // (the mask and the cursors go back to the pool)
    c->kept.push_back(kr);                                                          // (owned by the context from here on)
    if(n_reads_kept) *n_reads_kept = (int64_t)tot[0];
    return done(HLALA_OK);
}

extern "C" int hlala_kmer_presence_kept(hlala_ctx* c, int32_t k, int32_t n_queries, const char* queries, uint8_t* present)
{
    DEV_GUARD(c);
    ReaderScope rscope_(c, nullptr); if(rscope_.rc) return rscope_.rc;
    if(!c || n_queries < 0 || (n_queries > 0 && (!queries || !present))) return HLALA_E_ARG;
    std::vector<u64> canon, uniq;
    int rc = kmer_queries(c, "hlala_kmer_presence_kept", k, n_queries, queries, canon, uniq); if(rc) return rc;
    if(n_queries == 0) return HLALA_OK;
    memset(present, 0, (size_t)n_queries);
    if(uniq.empty() || c->kept.empty()) return HLALA_OK;
    std::vector<void*> tmp;
    auto done = [&](int r_) { for(void* p : tmp) pool_release(c, p); return r_; };
    u64* dQ = nullptr; uint8_t* dP = nullptr;
    if((rc = dev_upload(c, tmp, uniq.data(), uniq.size(), &dQ)) || (rc = dev_alloc(c, tmp, uniq.size(), &dP, true))) return done(rc);
    for(const hlala_ctx::KeptReads& kr : c->kept) {
        const unsigned grid = (unsigned)std::min<long long>((long long)kr.n, (long long)c->stitch_grid);
        hipLaunchKernelGGL(k_kmer_presence_kept, dim3(grid), dim3(64), 0, c->active, (const long long*)kr.start, (const int*)kr.length, (const uint8_t*)kr.store, kr.n, (int)k, (int)uniq.size(), (const u64*)dQ, dP);
        if((rc = check_launch(c, "k_kmer_presence_kept"))) return done(rc);
    }
    std::vector<uint8_t> hp(uniq.size());
    if((rc = dl(c, hp.data(), dP, uniq.size()))) return done(rc);
    HIP_TRY_F(c, hipStreamSynchronize(c->active), done);
    for(int i = 0; i < n_queries; i++) if(canon[i] != ~0ull) present[i] = hp[(size_t)(std::lower_bound(uniq.begin(), uniq.end(), canon[i]) - uniq.begin())];
    return done(HLALA_OK);
}

// ---- page-locked host memory (include/hlala_gpu.h)
extern "C" void* hlala_pinned_alloc(size_t bytes)
{
    void* p = nullptr;
    if(hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    return p;
}
extern "C" void hlala_pinned_free(void* p) { if(p) (void)hipHostFree(p); }
extern "C" int hlala_host_register(void* p, size_t bytes)
{
    if(!p || !bytes) return HLALA_E_ARG;
    if(hipHostRegister(p, bytes, hipHostRegisterDefault) != hipSuccess) { (void)hipGetLastError(); return HLALA_E_DEVICE; }
    return HLALA_OK;
}
extern "C" int hlala_host_unregister(void* p)
{
    if(!p) return HLALA_E_ARG;
    if(hipHostUnregister(p) != hipSuccess) { (void)hipGetLastError(); return HLALA_E_DEVICE; }
    return HLALA_OK;
}
static void seed_batch_unpin(hlala_seed_batch* S)
{
    if(hlala_host::seed_batch_pin_lazy(S)) {
        std::lock_guard<std::mutex> g(hlala_host::seed_batch_pin_mutex(S));
        for(auto& r : hlala_host::seed_batch_pin_regions(S)) { if(hipHostUnregister(r.first) != hipSuccess) (void)hipGetLastError(); }
        hlala_host::seed_batch_pin_regions(S).clear(); hlala_host::seed_batch_pin_cursor(S).clear();
        hlala_host::seed_batch_pin_lazy(S) = false;
    } else {
        std::vector<std::pair<void*, size_t>> arr; hlala_host::seed_batch_bulk_arrays(S, arr);
        for(auto& a : arr) { if(hipHostUnregister(a.first) != hipSuccess) (void)hipGetLastError(); }
    }
    hlala_host::seed_batch_pinned_flag(S) = false;
}
// window by window (pin = 2): what the units before unit_end occupy of every bulk array, rounded up to the next multiple of 64 MB, beyond what is locked already.  Called by
// hlala_seed_batch_window after it has filled the window; a refusal only costs speed (the upload of that window goes through the driver's staging buffer).
static void seed_batch_pin_upto(hlala_seed_batch* S, int64_t unit_end)
{
    std::lock_guard<std::mutex> g(hlala_host::seed_batch_pin_mutex(S));
    std::vector<std::pair<void*, size_t>> arr; std::vector<size_t> upto;
    hlala_host::seed_batch_bulk_arrays(S, arr, unit_end, &upto);
    std::vector<size_t>& cur = hlala_host::seed_batch_pin_cursor(S);
    if(cur.size() != arr.size()) cur.assign(arr.size(), 0);
    // pieces begin and end on multiples of PIN_GRANULE bytes of ADDRESS (the array's own start and end excepted): dev_upload cuts its copies there
    for(size_t i = 0; i < arr.size(); i++) {
        const uintptr_t base = (uintptr_t)arr[i].first;
        const size_t target = std::min(arr[i].second, (size_t)(((base + upto[i] + PIN_GRANULE - 1) & ~(uintptr_t)(PIN_GRANULE - 1)) - base));
        if(target <= cur[i]) continue;
        void* p = (char*)arr[i].first + cur[i];
        if(hipHostRegister(p, target - cur[i], hipHostRegisterDefault) == hipSuccess) hlala_host::seed_batch_pin_regions(S).emplace_back(p, target - cur[i]);
        else (void)hipGetLastError();
        cur[i] = target;
    }
}
extern "C" int hlala_seed_batch_pin(hlala_seed_batch* S, int pin)
{
    if(!S || pin < 0 || pin > 2) return HLALA_E_ARG;
    bool& flag = hlala_host::seed_batch_pinned_flag(S);
    const int now = !flag ? 0 : hlala_host::seed_batch_pin_lazy(S) ? 2 : 1;
    if(pin == now) return HLALA_OK;
    if(flag) seed_batch_unpin(S);
    if(!pin) return HLALA_OK;
    hlala_host::g_seed_batch_unpin = seed_batch_unpin;
    if(pin == 2) { hlala_host::g_seed_batch_pin_upto = seed_batch_pin_upto; hlala_host::seed_batch_pin_lazy(S) = true; flag = true; return HLALA_OK; }
    std::vector<std::pair<void*, size_t>> arr; hlala_host::seed_batch_bulk_arrays(S, arr);
    for(size_t i = 0; i < arr.size(); i++)
        if(hipHostRegister(arr[i].first, arr[i].second, hipHostRegisterDefault) != hipSuccess) {
            (void)hipGetLastError();
            for(size_t k = 0; k < i; k++) (void)hipHostUnregister(arr[k].first);
            return HLALA_E_DEVICE;
        }
    flag = true;
    return HLALA_OK;
}

// ---- BGZF inflate on the GPU (include/hlala_gpu.h; kernel_inflate.hip).  A call is cut into chunks of consecutive blocks (at most `chunk` compressed bytes, `outCap`
// inflated bytes, `maxBlocks` blocks); chunk k uses slot k % 3, every slot has a stream of its own: gather the compressed bytes into the slot's page-locked
// staging buffer -> upload -> kernel -> download into page-locked staging, all queued at once; the slot is drained (synchronise, copy the accepted blocks to their
// places in the caller's pageable buffer) before it is used again, so the upload of chunk k + 1 and the download of chunk k - 1 run beside the kernel of chunk k.
struct InflateSlot {
    hipStream_t stream = nullptr; hipEvent_t ev[4]{};      // before the upload, before the kernel, after it, after the download
    uint8_t* hComp = nullptr; uint8_t* dComp = nullptr; uint8_t* hOut = nullptr; uint8_t* dOut = nullptr;
    hlala_bgzf_block* hDesc = nullptr; hlala_bgzf_block* dDesc = nullptr; int* hStatus = nullptr; int* dStatus = nullptr;
    int64_t first = 0, count = 0; size_t outBytes = 0; bool busy = false;
    // hlala_bgzf_inflate_crc: expected and computed CRCs of the chunk's blocks and the event behind k_bgzf_crc32; allocated by the first call that asks for CRCs
    uint32_t* hCrcIn = nullptr; uint32_t* dCrcIn = nullptr; uint32_t* hCrcOut = nullptr; uint32_t* dCrcOut = nullptr; hipEvent_t evCrc = nullptr; bool crc = false;
};
// device buffers of hlala_bam_scan: grown on demand, kept by the handle
struct ScanBuf { void* p = nullptr; size_t cap = 0; };
enum { SCAN_DATA, SCAN_CARRY, SCAN_SLICES, SCAN_TOTALS, SCAN_INTERVALS, SCAN_RECORDS, SCAN_OFFSETS, SCAN_RECS, SCAN_COMPACT, SCAN_NBUF };
constexpr int SCAN_NEV = 11;
// device state of the grouping stage (hlala_bam_group; HLALA_SEEDS_GPU_GROUP): the sample-long arrays k_grp_append fills round by round (hash, meta, name offsets, name arena: they
// grow geometrically, by device-to-device copy), the scratch of the passes behind them, how many descriptors and name bytes they hold
enum { GRP_HASH, GRP_META, GRP_NAMEOFF, GRP_NAMES, GRP_LEN, GRP_OFF, GRP_CUB, GRP_KEYS, GRP_VAL_IN, GRP_VAL_OUT, GRP_START, GRP_RUNOFF, GRP_NEQ, GRP_WORD, GRP_FLAG, GRP_COUNTS, GRP_IN_RECS, GRP_IN_BYTES, GRP_NBUF };
constexpr int GRP_NEV = 8;
struct GroupState {
    ScanBuf buf[GRP_NBUF]; hipEvent_t ev[GRP_NEV]{}; bool evReady = false;
    int64_t n = 0; uint64_t nameBytes = 0; double msAppend = 0;
    bool ok = true;                 // false: a round could not be appended (allocation, 2^31 descriptors): the sample is not grouped here
    bool finished = false; int64_t nComplete = 0;      // group_finish has run over the n descriptors and found this many clean, complete runs (what HLALA_SEEDS_GPU_SORT orders)
};
// device buffers of the ordering stage (hlala_bam_name_order; HLALA_SEEDS_GPU_SORT): the names' offsets and lengths, the double-buffered working set (idx, seg, gp), the
// scratch of a round; grown on demand, kept by the handle
enum { NAM_IN_OFF, NAM_IN_LEN, NAM_IN_BYTES, NAM_SEL, NAM_SELOFF, NAM_IDX0, NAM_IDX1, NAM_SEG0, NAM_SEG1, NAM_GP0, NAM_GP1, NAM_KEY, NAM_KEYS, NAM_VAL, NAM_P1, NAM_K2, NAM_K2S, NAM_P2, NAM_NEWIDX,
       NAM_FL, NAM_FLOFF, NAM_ORDER, NAM_COUNT, NAM_CUB, NAM_NBUF };
constexpr int NAM_NEV = 7;
struct NameOrderState { ScanBuf buf[NAM_NBUF]; hipEvent_t ev[NAM_NEV]{}; bool evReady = false; };
// HLALA_SEEDS_GPU_FILL: the sample's descriptors (rec_off into `bytes`) and compact bytes, kept round by round behind the scan; the fill hook takes them over
struct FillKeep { ScanBuf recs, bytes; int64_t n = 0; uint64_t nBytes = 0; bool ok = false; };
struct hlala_inflater {
    int device = 0; size_t chunk = 0, outCap = 0; int64_t maxBlocks = 0;
    int32_t kernel = HLALA_INFLATE_KERNEL_HBM;      // hlala_inflater_set_kernel: read at the one launch site of inflate_run
    InflateSlot slot[3];
    ScanBuf scan[SCAN_NBUF]; hipEvent_t scanEv[SCAN_NEV]{}; bool scanEvReady = false;
    size_t roundBytes = 0;          // bytes of the decoder's last round in scan[SCAN_DATA] (hlala_host::bam_scan_round: their tail is the next round's carry)
    GroupState grp;
    NameOrderState nam;
    FillKeep keep;
    std::string err;
};
static thread_local std::string g_inflater_create_error;

extern "C" const char* hlala_inflater_last_error(const hlala_inflater* f) { return f ? f->err.c_str() : g_inflater_create_error.c_str(); }
extern "C" int hlala_inflater_set_kernel(hlala_inflater* f, int32_t kind)
{
    if(!f || (kind != HLALA_INFLATE_KERNEL_HBM && kind != HLALA_INFLATE_KERNEL_LDS)) { if(f) f->err = "hlala_inflater_set_kernel: unknown kind " + std::to_string(kind); return HLALA_E_ARG; }
    f->kernel = kind;
    return HLALA_OK;
}
extern "C" int32_t hlala_inflater_get_kernel(const hlala_inflater* f) { return f ? f->kernel : -1; }
extern "C" void hlala_inflater_destroy(hlala_inflater* f)
{
    if(!f) return;
    DevGuard g(f->device);
    for(InflateSlot& s : f->slot) {
        if(s.stream) { (void)hipStreamSynchronize(s.stream); (void)hipStreamDestroy(s.stream); }
        for(hipEvent_t e : s.ev) if(e) (void)hipEventDestroy(e);
        if(s.hComp) (void)hipHostFree(s.hComp); if(s.hOut) (void)hipHostFree(s.hOut); if(s.hDesc) (void)hipHostFree(s.hDesc); if(s.hStatus) (void)hipHostFree(s.hStatus);
        if(s.dComp) (void)hipFree(s.dComp); if(s.dOut) (void)hipFree(s.dOut); if(s.dDesc) (void)hipFree(s.dDesc); if(s.dStatus) (void)hipFree(s.dStatus);
        if(s.evCrc) (void)hipEventDestroy(s.evCrc); if(s.hCrcIn) (void)hipHostFree(s.hCrcIn); if(s.hCrcOut) (void)hipHostFree(s.hCrcOut); if(s.dCrcIn) (void)hipFree(s.dCrcIn); if(s.dCrcOut) (void)hipFree(s.dCrcOut);
    }
    for(ScanBuf& b : f->scan) if(b.p) (void)hipFree(b.p);
    for(hipEvent_t e : f->scanEv) if(e) (void)hipEventDestroy(e);
    for(ScanBuf& b : f->grp.buf) if(b.p) (void)hipFree(b.p);
    for(hipEvent_t e : f->grp.ev) if(e) (void)hipEventDestroy(e);
    for(ScanBuf& b : f->nam.buf) if(b.p) (void)hipFree(b.p);
    for(hipEvent_t e : f->nam.ev) if(e) (void)hipEventDestroy(e);
    if(f->keep.recs.p) (void)hipFree(f->keep.recs.p);
    if(f->keep.bytes.p) (void)hipFree(f->keep.bytes.p);
    delete f;
}
extern "C" int hlala_inflater_create(int32_t device, size_t chunk_bytes, hlala_inflater** out)
{
    if(!out) { g_inflater_create_error = "null argument"; return HLALA_E_ARG; }
    *out = nullptr;
    if(chunk_bytes == 0) chunk_bytes = HLALA_INFLATE_DEFAULT_CHUNK;
    if(device < 0 || chunk_bytes < HLALA_INFLATE_MIN_CHUNK || chunk_bytes > ((size_t)1 << 30)) { g_inflater_create_error = "hlala_inflater_create: chunk_bytes outside [128 KiB, 1 GiB] or a negative device"; return HLALA_E_ARG; }
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if(e != hipSuccess || ndev <= 0 || device >= ndev) {
        g_inflater_create_error = std::string("no HIP device available (") + (e != hipSuccess ? hipGetErrorString(e) : "device index out of range") + "); this library has no CPU fallback";
        (void)hipGetLastError();
        return HLALA_E_DEVICE;
    }
    hlala_inflater* f = new hlala_inflater();
    f->device = device; f->chunk = chunk_bytes; f->outCap = 4 * chunk_bytes + 65536; f->maxBlocks = (int64_t)(chunk_bytes / 256) + 64;
    DevGuard g(device);
    auto fail = [&](const char* what) { g_inflater_create_error = std::string("hlala_inflater_create: ") + what + " failed"; (void)hipGetLastError(); hlala_inflater_destroy(f); return HLALA_E_DEVICE; };
    { int cur = -1; if(hipGetDevice(&cur) != hipSuccess || cur != device) return fail("hipSetDevice"); }
    for(InflateSlot& s : f->slot) {
        if(hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking) != hipSuccess) return fail("hipStreamCreate");
        for(hipEvent_t& ev : s.ev) if(hipEventCreate(&ev) != hipSuccess) return fail("hipEventCreate");
        const size_t nd = (size_t)f->maxBlocks;
        if(hipHostMalloc((void**)&s.hComp, f->chunk, hipHostMallocDefault) != hipSuccess || hipHostMalloc((void**)&s.hOut, f->outCap, hipHostMallocDefault) != hipSuccess ||
           hipHostMalloc((void**)&s.hDesc, nd * sizeof(hlala_bgzf_block), hipHostMallocDefault) != hipSuccess || hipHostMalloc((void**)&s.hStatus, nd * sizeof(int), hipHostMallocDefault) != hipSuccess) return fail("hipHostMalloc");
        if(hipMalloc((void**)&s.dComp, f->chunk) != hipSuccess || hipMalloc((void**)&s.dOut, f->outCap) != hipSuccess ||
           hipMalloc((void**)&s.dDesc, nd * sizeof(hlala_bgzf_block)) != hipSuccess || hipMalloc((void**)&s.dStatus, nd * sizeof(int)) != hipSuccess) return fail("hipMalloc");
    }
    *out = f;
    return HLALA_OK;
}

// `landed` (may be null) is told about every chunk, in ascending block order, once its accepted blocks stand in `out` and its statuses in `status`; a non-zero
// answer ends the call (HLALA_E_STATE) after the chunks in flight have been drained.
static int inflate_run(hlala_inflater* f, const uint8_t* comp, size_t comp_bytes, const hlala_bgzf_block* blocks, int64_t n, uint8_t* out, size_t out_bytes, int32_t* status,
                       hlala_inflate_stats* stats, int (*landed)(void*, int64_t, int64_t), void* user, uint8_t* dOutBase = nullptr,
                       const uint32_t* crcExpect = nullptr, uint32_t* crcOut = nullptr, double* msCrc = nullptr)
{
    // crcExpect / crcOut (either non-null: k_bgzf_crc32 runs behind the inflate kernel of every chunk, on the chunk's stream, with the chunk's descriptors): a block
    // whose CRC-32 is not crcExpect[i] comes back with HLALA_INFLATE_CRC_MISMATCH and its bytes; with both null nothing below differs from a call without them.
    // dOutBase (device memory of out_bytes bytes; `out` is not used then): the blocks' output stays on the device -- block i goes to dOutBase + blocks[i].uoff, straight
    // from the kernel; only the statuses come back.  The output ranges must follow one another without gaps (a chunk's kernel writes one contiguous range).
    if(!f) return HLALA_E_ARG;
    f->err.clear();
    if(dOutBase) { uint64_t at = 0; for(int64_t i = 0; i < n && blocks; i++) { if(blocks[i].uoff != at) { f->err = "hlala_bgzf_inflate: output ranges with gaps cannot stay on the device"; return HLALA_E_ARG; } at += blocks[i].isize; } }
    if(n < 0 || (n > 0 && (!blocks || !status)) || (comp_bytes && !comp) || (out_bytes && !out && !dOutBase)) { f->err = "hlala_bgzf_inflate: null argument"; return HLALA_E_ARG; }
    const auto tWall = std::chrono::steady_clock::now();
    // ---- the descriptors, before anything is launched
    for(int64_t i = 0; i < n; i++) {
        const hlala_bgzf_block& b = blocks[i];
        if(b.isize > 65536u || b.coff > comp_bytes || b.clen > comp_bytes - b.coff || b.uoff > out_bytes || b.isize > out_bytes - b.uoff || b.clen > f->chunk) {
            f->err = "hlala_bgzf_inflate: block " + std::to_string(i) + ": a range outside its buffer, more than 65536 bytes of payload, or more compressed bytes than a chunk holds";
            return HLALA_E_ARG;
        }
    }
    {
        std::vector<int64_t> by; by.reserve((size_t)n);
        for(int64_t i = 0; i < n; i++) if(blocks[i].isize) by.push_back(i);
        std::sort(by.begin(), by.end(), [&](int64_t a, int64_t b) { return blocks[a].uoff < blocks[b].uoff; });
        for(size_t k = 1; k < by.size(); k++)
            if(blocks[by[k - 1]].uoff + blocks[by[k - 1]].isize > blocks[by[k]].uoff) { f->err = "hlala_bgzf_inflate: the output ranges of blocks " + std::to_string(by[k - 1]) + " and " + std::to_string(by[k]) + " overlap"; return HLALA_E_ARG; }
    }
    DevGuard g(f->device);
    hlala_inflate_stats st{}; st.n_blocks = n;
    int rc = HLALA_OK;
    const bool wantCrc = crcExpect || crcOut;
    double crcMs = 0;
    if(msCrc) *msCrc = 0;
    if(wantCrc) for(InflateSlot& s : f->slot) {
        if(s.evCrc) continue;
        const size_t nd = (size_t)f->maxBlocks * sizeof(uint32_t);
        if((!s.hCrcIn && hipHostMalloc((void**)&s.hCrcIn, nd, hipHostMallocDefault) != hipSuccess) || (!s.hCrcOut && hipHostMalloc((void**)&s.hCrcOut, nd, hipHostMallocDefault) != hipSuccess) ||
           (!s.dCrcIn && hipMalloc((void**)&s.dCrcIn, nd) != hipSuccess) || (!s.dCrcOut && hipMalloc((void**)&s.dCrcOut, nd) != hipSuccess) || hipEventCreate(&s.evCrc) != hipSuccess) {
            (void)hipGetLastError(); f->err = "hlala_bgzf_inflate_crc: no memory for the CRC arrays"; return HLALA_E_DEVICE;      // (what was allocated is kept and freed with the handle)
        }
    }
    auto drain = [&](InflateSlot& s, bool deliver) {
        if(!s.busy) return;
        s.busy = false;
        const hipError_t e = hipStreamSynchronize(s.stream);
        if(e != hipSuccess) { if(rc == HLALA_OK) { f->err = std::string("hlala_bgzf_inflate: ") + hipGetErrorString(e); rc = HLALA_E_DEVICE; } return; }
        float ms = 0;
        if(hipEventElapsedTime(&ms, s.ev[0], s.ev[1]) == hipSuccess) st.ms_h2d += ms;
        if(hipEventElapsedTime(&ms, s.ev[1], s.ev[2]) == hipSuccess) st.ms_kernel += ms;
        if(hipEventElapsedTime(&ms, s.crc ? s.evCrc : s.ev[2], s.ev[3]) == hipSuccess) st.ms_d2h += ms;
        if(s.crc && hipEventElapsedTime(&ms, s.ev[2], s.evCrc) == hipSuccess) crcMs += ms;
        if(!deliver || rc != HLALA_OK) return;
        for(int64_t k = 0; k < s.count; k++) {
            const hlala_bgzf_block& b = blocks[s.first + k];
            const int v = s.hStatus[k];
            status[s.first + k] = v;
            if(v == HLALA_INFLATE_OK) st.n_ok++; else st.n_rejected++;
            if((v == HLALA_INFLATE_OK || v == HLALA_INFLATE_CRC_MISMATCH) && b.isize && !dOutBase) memcpy(out + b.uoff, s.hOut + s.hDesc[k].uoff, b.isize);
            if(s.crc && crcOut) crcOut[s.first + k] = s.hCrcOut[k];
        }
        if(landed && landed(user, s.first, s.count) != 0) { f->err = "hlala_bgzf_inflate: ended by the caller"; rc = HLALA_E_STATE; }
    };
    int64_t i = 0; int k = 0;
    while(i < n && rc == HLALA_OK) {
        InflateSlot& s = f->slot[k % 3]; k++;
        drain(s, true);
        if(rc != HLALA_OK) break;
        size_t cb = 0, ob = 0; int64_t cnt = 0;
        while(i + cnt < n && cnt < f->maxBlocks) {
            const hlala_bgzf_block& b = blocks[i + cnt];
            const size_t ca = (cb + 15) & ~(size_t)15;      // (every block starts on 16 bytes of the staging buffer)
            if(ca + b.clen > f->chunk || ob + b.isize > f->outCap) break;
            if(b.clen) memcpy(s.hComp + ca, comp + b.coff, b.clen);
            hlala_bgzf_block& d = s.hDesc[cnt]; d.coff = ca; d.clen = b.clen; d.isize = b.isize; d.uoff = ob;
            if(crcExpect) s.hCrcIn[cnt] = crcExpect[i + cnt];
            cb = ca + b.clen; ob += b.isize; cnt++;
        }
        // (cnt >= 1: a single block fits an empty chunk -- clen <= chunk was checked, isize <= 65536 < outCap)
        s.first = i; s.count = cnt; s.outBytes = ob; s.crc = wantCrc; i += cnt;
        hipError_t e = hipEventRecord(s.ev[0], s.stream);
        if(e == hipSuccess && cb) e = hipMemcpyAsync(s.dComp, s.hComp, cb, hipMemcpyHostToDevice, s.stream);
        if(e == hipSuccess) e = hipMemcpyAsync(s.dDesc, s.hDesc, (size_t)cnt * sizeof(hlala_bgzf_block), hipMemcpyHostToDevice, s.stream);
        if(e == hipSuccess && crcExpect) e = hipMemcpyAsync(s.dCrcIn, s.hCrcIn, (size_t)cnt * sizeof(uint32_t), hipMemcpyHostToDevice, s.stream);
        if(e == hipSuccess) e = hipEventRecord(s.ev[1], s.stream);
        if(e == hipSuccess) {
            uint8_t* dst = dOutBase ? dOutBase + blocks[s.first].uoff : s.dOut;
            if(f->kernel == HLALA_INFLATE_KERNEL_LDS) hipLaunchKernelGGL(k_bgzf_inflate_lds, dim3((unsigned)cnt), dim3(64 * INF_LDS_WAVES), 0, s.stream, (const uint8_t*)s.dComp, (const hlala_bgzf_block*)s.dDesc, (int)cnt, dst, s.dStatus);
            else hipLaunchKernelGGL(k_bgzf_inflate, dim3((unsigned)cnt), dim3(64), 0, s.stream, (const uint8_t*)s.dComp, (const hlala_bgzf_block*)s.dDesc, (int)cnt, dst, s.dStatus);
            e = hipGetLastError();
        }
        if(e == hipSuccess) e = hipEventRecord(s.ev[2], s.stream);
        if(e == hipSuccess && wantCrc) {
            hipLaunchKernelGGL(k_bgzf_crc32, dim3((unsigned)cnt), dim3(64), 0, s.stream, (const uint8_t*)(dOutBase ? dOutBase + blocks[s.first].uoff : s.dOut), (const hlala_bgzf_block*)s.dDesc, (int)cnt, s.dStatus,
                               crcExpect ? (const uint32_t*)s.dCrcIn : (const uint32_t*)nullptr, s.dCrcOut);
            e = hipGetLastError();
            if(e == hipSuccess) e = hipEventRecord(s.evCrc, s.stream);
            if(e == hipSuccess && crcOut) e = hipMemcpyAsync(s.hCrcOut, s.dCrcOut, (size_t)cnt * sizeof(uint32_t), hipMemcpyDeviceToHost, s.stream);
        }
        if(e == hipSuccess && ob && !dOutBase) e = hipMemcpyAsync(s.hOut, s.dOut, ob, hipMemcpyDeviceToHost, s.stream);
        if(e == hipSuccess) e = hipMemcpyAsync(s.hStatus, s.dStatus, (size_t)cnt * sizeof(int), hipMemcpyDeviceToHost, s.stream);
        if(e == hipSuccess) e = hipEventRecord(s.ev[3], s.stream);
        s.busy = true;
        if(e != hipSuccess) { f->err = std::string("hlala_bgzf_inflate: ") + hipGetErrorString(e); rc = HLALA_E_DEVICE; }
    }
    // the chunks still in flight, oldest first (slots are used round-robin: the oldest is the one that would be used next)
    for(int j = 0; j < 3; j++) drain(f->slot[(k + j) % 3], rc == HLALA_OK);
    st.ms_wall = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tWall).count();
    if(stats) *stats = st;
    if(msCrc) *msCrc = crcMs;
    return rc;
}
extern "C" int hlala_bgzf_inflate(hlala_inflater* f, const uint8_t* comp, size_t comp_bytes, const hlala_bgzf_block* blocks, int64_t n_blocks, uint8_t* out, size_t out_bytes,
                                  int32_t* status, hlala_inflate_stats* stats)
{
    return inflate_run(f, comp, comp_bytes, blocks, n_blocks, out, out_bytes, status, stats, nullptr, nullptr);
}
extern "C" int hlala_bgzf_inflate_crc(hlala_inflater* f, const uint8_t* comp, size_t comp_bytes, const hlala_bgzf_block* blocks, int64_t n_blocks, uint8_t* out, size_t out_bytes,
                                      const uint32_t* crc_expect, uint32_t* crc_out, int32_t* status, hlala_inflate_stats* stats, double* ms_crc)
{
    return inflate_run(f, comp, comp_bytes, blocks, n_blocks, out, out_bytes, status, stats, nullptr, nullptr, nullptr, crc_expect, crc_out, ms_crc);
}
static int bam_inflate_crc_hook(void* inflater, const uint8_t* comp, size_t comp_bytes, const hlala_bgzf_block* blocks, int64_t n, uint8_t* out, size_t out_bytes, int32_t* status,
                                int (*landed)(void*, int64_t, int64_t), void* user, const uint32_t* crc_expect, std::string* err)
{
    hlala_inflater* f = (hlala_inflater*)inflater;
    const int rc = inflate_run(f, comp, comp_bytes, blocks, n, out, out_bytes, status, nullptr, landed, user, nullptr, crc_expect);
    if(rc != HLALA_OK && err) *err = f->err;
    return rc;
}
static int bam_inflate_hook(void* inflater, const uint8_t* comp, size_t comp_bytes, const hlala_bgzf_block* blocks, int64_t n, uint8_t* out, size_t out_bytes, int32_t* status,
                            int (*landed)(void*, int64_t, int64_t), void* user, std::string* err)
{
    return bam_inflate_crc_hook(inflater, comp, comp_bytes, blocks, n, out, out_bytes, status, landed, user, nullptr, err);
}
static int bam_scan_hook(void* inflater, hlala_host::bam_scan_round* R, std::string* err);      // (behind hlala_bam_scan, below)
static int bam_group_hook(void* inflater, int64_t n, int32_t long_read_mode, uint32_t* perm, uint8_t* flag, hlala_bam_group_stats* stats, bool* available, std::string* err);      // (behind hlala_bam_group, below)
static int bam_sort_hook(void* inflater, int64_t m, uint32_t* order, hlala_bam_name_order_stats* stats, bool* available, std::string* err);      // (behind hlala_bam_name_order, below)
static int bam_fill_hook(void* inflater, const hlala_bam_fill_in* in, int64_t* read_off, int64_t* chain_off, int64_t* cigar_count, int64_t* name_off, hlala_host::bam_fill_handle* handle,
                         hlala_bam_fill_stats* stats, bool* available, std::string* err);      // (behind hlala_bam_fill_create, below)
static int bam_fill_wide_hook(void* inflater, const hlala_bam_fill_in* in, int32_t max_mate, const uint32_t* wide_units, int64_t n_wide, int64_t longest, int64_t* read_off, int64_t* chain_off,
                              int64_t* cigar_count, int64_t* name_off, hlala_host::bam_fill_handle* handle, hlala_bam_fill_stats* stats, bool* available, std::string* err);
extern "C" int hlala_bam_extract_seeds_gpu(hlala_inflater* f, const char* path, int32_t n_intervals, const hlala_bam_interval* iv, int32_t long_read_mode, int32_t n_threads, int32_t flags,
                                           hlala_seed_batch** out)
{
    static std::once_flag hookOnce;                  // (samples may decode on several threads)
    std::call_once(hookOnce, []() { hlala_host::g_bam_inflate_hook = bam_inflate_hook; hlala_host::g_bam_inflate_crc_hook = bam_inflate_crc_hook; hlala_host::g_bam_scan_hook = bam_scan_hook; hlala_host::g_bam_group_hook = bam_group_hook; hlala_host::g_bam_sort_hook = bam_sort_hook; hlala_host::g_bam_fill_hook = bam_fill_hook; hlala_host::g_bam_fill_wide_hook = bam_fill_wide_hook; });
    return hlala_host::bam_extract_seeds_impl(path, n_intervals, iv, long_read_mode, n_threads, flags, true, f, out);
}

// ---- the BAM record pass (include/hlala_gpu.h; kernel_bamscan.hip).  Three stretches of one stream, the host looking at the totals between them: upload, guess, link
// (how many records: the size of the per-record arrays; too many re-hops end the call here) -- starts, parse, the two scans (the verdict, and what the caller's
// arrays must hold) -- emit, download.
static hipError_t scan_grow(hlala_inflater* f, int which, size_t bytes)
{
    ScanBuf& b = f->scan[which];
    if(bytes <= b.cap) return hipSuccess;
    if(b.p) { (void)hipFree(b.p); b.p = nullptr; b.cap = 0; }
    const size_t want = bytes + bytes / 4 + 256;
    const hipError_t r = hipMalloc(&b.p, want);
    if(r == hipSuccess) b.cap = want; else b.p = nullptr;
    return r;
}
// where the results of a scan go: asked for once their sizes are known (null: they do not fit, HLALA_E_CAPACITY)
struct ScanSink { void* user; hlala_bam_rec* (*recs)(void*, int64_t); uint8_t* (*compact)(void*, size_t); };
// data == null: the n bytes stand in scan[SCAN_DATA] already (the decoder's round buffer); the arguments have been checked
static int scan_run(hlala_inflater* f, const uint8_t* data, size_t n, size_t first, int32_t last, const hlala_bam_scan_in* in, const ScanSink& sink, hlala_bam_scan_stats* stats)
{
    using namespace hlala_bamscan;
    const auto tWall = std::chrono::steady_clock::now();
    memset(stats, 0, sizeof(*stats));
    stats->status_record = -1;
    const uint32_t S = scan_slice(*in), maxRehops = scan_max_rehops(*in);
    const uint32_t nSlices = (uint32_t)(((uint64_t)n + S - 1) / S);
    stats->n_slices = nSlices;
    if(nSlices == 0) return HLALA_OK;                          // no byte, no record
    DevGuard g(f->device);
    hipStream_t st = f->slot[0].stream;
    hipError_t e = hipSuccess;
    auto failed = [&](const char* what) { f->err = std::string("hlala_bam_scan: ") + what + ": " + hipGetErrorString(e); (void)hipStreamSynchronize(st); (void)hipGetLastError(); return HLALA_E_DEVICE; };
    if(!f->scanEvReady) {
        for(hipEvent_t& ev : f->scanEv) if(!ev && (e = hipEventCreate(&ev)) != hipSuccess) return failed("hipEventCreate");
        f->scanEvReady = true;
    }
    auto grow = [&](int which, size_t bytes) -> hipError_t { return scan_grow(f, which, bytes); };
    hipEvent_t* ev = f->scanEv;
    auto ms = [&](int a, int b) { float t = 0; return hipEventElapsedTime(&t, ev[a], ev[b]) == hipSuccess ? (double)t : 0.0; };
    // the intervals as one array: ref_iv_off | ref_iv | iv_start | iv_stop | iv_contig
    const size_t nOff = in->n_ref > 0 ? (size_t)in->n_ref + 1 : 0, nIv = nOff ? (size_t)in->ref_iv_off[in->n_ref] : 0, nI = nIv ? (size_t)in->n_intervals : 0;
    std::vector<int32_t> hIv(nOff + nIv + 3 * nI + 1, 0);
    if(nOff) memcpy(hIv.data(), in->ref_iv_off, nOff * 4);
    if(nIv) { memcpy(hIv.data() + nOff, in->ref_iv, nIv * 4); memcpy(hIv.data() + nOff + nIv, in->iv_start, nI * 4); memcpy(hIv.data() + nOff + nIv + nI, in->iv_stop, nI * 4); memcpy(hIv.data() + nOff + nIv + 2 * nI, in->iv_contig, nI * 4); }
    if((data && (e = grow(SCAN_DATA, n)) != hipSuccess) || (e = grow(SCAN_SLICES, (size_t)nSlices * 5 * 4)) != hipSuccess || (e = grow(SCAN_TOTALS, sizeof(BamScanTotals))) != hipSuccess ||
       (e = grow(SCAN_INTERVALS, hIv.size() * 4)) != hipSuccess) return failed("hipMalloc");
    const uint8_t* dData = (const uint8_t*)f->scan[SCAN_DATA].p;
    u32* dG = (u32*)f->scan[SCAN_SLICES].p; u32* dX = dG + nSlices; u32* dCf = dX + nSlices; u32* dEntry = dCf + nSlices; u32* dPrefix = dEntry + nSlices;
    BamScanTotals* dT = (BamScanTotals*)f->scan[SCAN_TOTALS].p;
    const int32_t* dIv = (const int32_t*)f->scan[SCAN_INTERVALS].p;
    hlala_bam_scan_in din = *in;
    din.ref_iv_off = dIv; din.ref_iv = dIv + nOff; din.iv_start = dIv + nOff + nIv; din.iv_stop = dIv + nOff + nIv + nI; din.iv_contig = dIv + nOff + nIv + 2 * nI;
    BamScanTotals hT{}; hT.fail_key = ~0ull;
    // ---- upload, guess, link
    e = hipEventRecord(ev[0], st);
    if(e == hipSuccess && data) e = hipMemcpyAsync((void*)dData, data, n, hipMemcpyHostToDevice, st);
    if(e == hipSuccess) e = hipMemcpyAsync((void*)dIv, hIv.data(), hIv.size() * 4, hipMemcpyHostToDevice, st);
    if(e == hipSuccess) e = hipMemcpyAsync(dT, &hT, sizeof(hT), hipMemcpyHostToDevice, st);
    if(e == hipSuccess) e = hipEventRecord(ev[1], st);
    if(e == hipSuccess) { hipLaunchKernelGGL(k_bam_guess, dim3((nSlices + 3) / 4), dim3(256), 0, st, dData, (u32)n, (u32)first, S, nSlices, (int)in->n_ref, dG, dX, dCf); e = hipGetLastError(); }
    if(e == hipSuccess) e = hipEventRecord(ev[2], st);
    if(e == hipSuccess) { hipLaunchKernelGGL(k_bam_link, dim3(1), dim3(64), 0, st, dData, (u32)n, (u32)first, S, nSlices, maxRehops, (const u32*)dG, (const u32*)dX, (const u32*)dCf, dEntry, dPrefix, dT); e = hipGetLastError(); }
    if(e == hipSuccess) e = hipEventRecord(ev[3], st);
    if(e == hipSuccess) e = hipMemcpyAsync(&hT, dT, sizeof(hT), hipMemcpyDeviceToHost, st);
    if(e == hipSuccess) e = hipStreamSynchronize(st);
    if(e != hipSuccess) return failed("upload / k_bam_guess / k_bam_link");
    stats->ms_h2d = ms(0, 1); stats->ms_guess = ms(1, 2); stats->ms_link = ms(2, 3);
    stats->n_rehops = hT.n_rehops;
    auto done = [&](int rc) { stats->ms_wall = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tWall).count(); return rc; };
    if(hT.link_status == HLALA_BAMSCAN_TOO_MANY_REHOPS) { stats->status = HLALA_BAMSCAN_TOO_MANY_REHOPS; return done(HLALA_OK); }
    const uint32_t nRec = hT.n_records;
    if((uint64_t)nRec > (uint64_t)n / BAM_HEAD || hT.consumed > n) { f->err = "hlala_bam_scan: k_bam_link counted more records than the bytes hold"; return HLALA_E_DEVICE; }      // (cannot happen; sizes below rest on it)
    stats->n_records = nRec; stats->consumed = hT.consumed;
    // ---- starts, parse, the two scans
    if((e = grow(SCAN_RECORDS, ((size_t)nRec * 3 + 1) * 4)) != hipSuccess || (e = grow(SCAN_OFFSETS, ((size_t)nRec + 1) * 2 * 8)) != hipSuccess) return failed("hipMalloc");
    u32* dStart = (u32*)f->scan[SCAN_RECORDS].p; u32* dCnt = dStart + nRec; u32* dCsize = dCnt + nRec;
    u64* dDescOff = (u64*)f->scan[SCAN_OFFSETS].p; u64* dCompOff = dDescOff + nRec + 1;
    e = hipEventRecord(ev[4], st);
    if(e == hipSuccess && nRec) { hipLaunchKernelGGL(k_bam_starts, dim3((nSlices + 255) / 256), dim3(256), 0, st, dData, (u32)n, S, nSlices, nRec, (const u32*)dEntry, (const u32*)dPrefix, dStart); e = hipGetLastError(); }
    if(e == hipSuccess) e = hipEventRecord(ev[5], st);
    if(e == hipSuccess && nRec) { hipLaunchKernelGGL(k_bam_parse, dim3((nRec + 255) / 256), dim3(256), 0, st, dData, (u32)n, nRec, din, (const u32*)dStart, dCnt, dCsize, dT); e = hipGetLastError(); }
    if(e == hipSuccess) e = hipEventRecord(ev[6], st);
    if(e == hipSuccess) { hipLaunchKernelGGL(k_bam_scan2, dim3(2), dim3(BAM_SCAN_THREADS), 0, st, nRec, (const u32*)dCnt, (const u32*)dCsize, dDescOff, dCompOff, dT); e = hipGetLastError(); }
    if(e == hipSuccess) e = hipEventRecord(ev[7], st);
    if(e == hipSuccess) e = hipMemcpyAsync(&hT, dT, sizeof(hT), hipMemcpyDeviceToHost, st);
    if(e == hipSuccess) e = hipStreamSynchronize(st);
    if(e != hipSuccess) return failed("k_bam_starts / k_bam_parse / k_bam_scan2");
    stats->ms_starts = ms(4, 5); stats->ms_parse = ms(5, 6); stats->ms_scan = ms(6, 7);
    stats->n_kept = (int64_t)hT.kept; stats->n_recs = (int64_t)hT.n_desc; stats->examined = (int64_t)hT.examined; stats->compact_bytes = (int64_t)hT.compact_bytes;
    scan_verdict(hT.link_status, hT.link_record, hT.fail_key, last != 0, hT.consumed, n, nRec, &stats->status, &stats->status_record);
    if(stats->status != HLALA_BAMSCAN_OK) return done(HLALA_OK);
    if(hT.compact_bytes > (uint64_t)n) { f->err = "hlala_bam_scan: more compact bytes than bytes"; return HLALA_E_DEVICE; }                                                       // (cannot happen)
    if(stats->n_recs == 0) return done(HLALA_OK);
    hlala_bam_rec* recs = sink.recs(sink.user, stats->n_recs); uint8_t* compact = recs ? sink.compact(sink.user, (size_t)hT.compact_bytes) : nullptr;
    if(!recs || !compact) {
        f->err = "hlala_bam_scan: " + std::to_string(stats->n_recs) + " descriptors and " + std::to_string(stats->compact_bytes) + " compact bytes do not fit the caller's arrays";
        return done(HLALA_E_CAPACITY);
    }
    // ---- emit, download
    const size_t recBytes = (size_t)stats->n_recs * sizeof(hlala_bam_rec), compBytes = (size_t)hT.compact_bytes;
    if((e = grow(SCAN_RECS, recBytes)) != hipSuccess || (e = grow(SCAN_COMPACT, compBytes)) != hipSuccess) return failed("hipMalloc");
    hlala_bam_rec* dRecs = (hlala_bam_rec*)f->scan[SCAN_RECS].p; uint8_t* dCompact = (uint8_t*)f->scan[SCAN_COMPACT].p;
    e = hipEventRecord(ev[8], st);
    if(e == hipSuccess) { hipLaunchKernelGGL(k_bam_emit, dim3((nRec + 255) / 256), dim3(256), 0, st, dData, (u32)n, nRec, din, (const u32*)dStart, (const u32*)dCnt, (const u32*)dCsize, (const u64*)dDescOff, (const u64*)dCompOff, dRecs, dCompact); e = hipGetLastError(); }
    if(e == hipSuccess) e = hipEventRecord(ev[9], st);
    if(e == hipSuccess) e = hipMemcpyAsync(recs, dRecs, recBytes, hipMemcpyDeviceToHost, st);
    if(e == hipSuccess && compBytes) e = hipMemcpyAsync(compact, dCompact, compBytes, hipMemcpyDeviceToHost, st);
    if(e == hipSuccess) e = hipEventRecord(ev[10], st);
    if(e == hipSuccess) e = hipStreamSynchronize(st);
    if(e != hipSuccess) return failed("k_bam_emit / download");
    stats->ms_emit = ms(8, 9); stats->ms_d2h = ms(9, 10);
    return done(HLALA_OK);
}
extern "C" int hlala_bam_scan(hlala_inflater* f, const uint8_t* data, size_t n, size_t first, int32_t last, const hlala_bam_scan_in* in, hlala_bam_rec* recs, int64_t cap_recs,
                              uint8_t* compact, size_t cap_compact, hlala_bam_scan_stats* stats)
{
    if(!f) return HLALA_E_ARG;
    f->err.clear();
    if(const char* bad = hlala_bamscan::scan_check_args(data, n, first, in, recs, cap_recs, compact, cap_compact, stats)) { f->err = std::string("hlala_bam_scan: ") + bad; return HLALA_E_ARG; }
    struct Caller { hlala_bam_rec* recs; int64_t cap_recs; uint8_t* compact; size_t cap_compact; } c{recs, cap_recs, compact, cap_compact};
    ScanSink sink{&c, [](void* u, int64_t k) -> hlala_bam_rec* { Caller* c = (Caller*)u; return k <= c->cap_recs ? c->recs : nullptr; },
                  [](void* u, size_t k) -> uint8_t* { Caller* c = (Caller*)u; return k <= c->cap_compact ? c->compact : nullptr; }};
    f->roundBytes = 0;
    uint8_t none = 0;
    return scan_run(f, n ? data : &none, n, first, last, in, sink, stats);
}
static void group_reset(hlala_inflater* f);
static void keep_reset(hlala_inflater* f);
static void keep_drop(hlala_inflater* f);
static int keep_append(hlala_inflater* f, const hlala_bam_rec* dRecs, int64_t n, const uint8_t* dBytes, size_t nBytes);
static int group_append(hlala_inflater* f, const hlala_bam_rec* dRecs, int64_t n, const uint8_t* dBytes, size_t nBytes);
// One round of the decoder with HLALA_SEEDS_GPU_PARSE (hlala_host::bam_scan_round): carry to the front, inflate into the device round buffer, the record pass on it.
static int bam_scan_hook(void* inflater, hlala_host::bam_scan_round* R, std::string* err)
{
    hlala_inflater* f = (hlala_inflater*)inflater;
    if(!f || !R) return HLALA_E_ARG;
    f->err.clear();
    auto out = [&](int rc) { if(rc != HLALA_OK && err) *err = f->err; return rc; };
    const size_t n = R->carry + R->seg_bytes;
    R->n_gpu = R->n_retried = R->n_crc_recheck = 0; R->fell_back = false; R->s_inflate = R->s_scan = 0; R->bytes_h2d = R->bytes_d2h = 0;
    if(n >= ((size_t)1 << 32)) { f->err = "a round of 2^32 bytes or more: lower HLALA_BAM_SEGMENT_BYTES"; return out(HLALA_E_CAPACITY); }
    if(R->carry > f->roundBytes) { f->err = "more bytes carried than the last round held"; return out(HLALA_E_STATE); }
    const auto t0 = std::chrono::steady_clock::now();
    DevGuard g(f->device);
    hipStream_t st = f->slot[0].stream;
    hipError_t e = hipSuccess;
    auto failed = [&](const char* what) { f->err = std::string("BAM record pass: ") + what + ": " + hipGetErrorString(e); (void)hipStreamSynchronize(st); (void)hipGetLastError(); return out(HLALA_E_DEVICE); };
    // the carried bytes: aside first (the round buffer may have to grow), then to the front
    if(R->carry) {
        if((e = scan_grow(f, SCAN_CARRY, R->carry)) != hipSuccess) return failed("hipMalloc");
        e = hipMemcpyAsync(f->scan[SCAN_CARRY].p, (const uint8_t*)f->scan[SCAN_DATA].p + (f->roundBytes - R->carry), R->carry, hipMemcpyDeviceToDevice, st);
        if(e == hipSuccess) e = hipStreamSynchronize(st);
        if(e != hipSuccess) return failed("carry");
    }
    if((e = scan_grow(f, SCAN_DATA, n ? n : 1)) != hipSuccess) return failed("hipMalloc");
    uint8_t* dData = (uint8_t*)f->scan[SCAN_DATA].p;
    if(R->carry) {
        e = hipMemcpyAsync(dData, f->scan[SCAN_CARRY].p, R->carry, hipMemcpyDeviceToDevice, st);
        if(e == hipSuccess) e = hipStreamSynchronize(st);
        if(e != hipSuccess) return failed("carry");
    }
    f->roundBytes = n;
    std::vector<int32_t> status((size_t)R->n_blocks + 1, 0);
    int rc = inflate_run(f, R->comp, R->comp_bytes, R->blocks, R->n_blocks, nullptr, R->seg_bytes, status.data(), nullptr, nullptr, nullptr, dData + R->carry, R->crc_expect);      // (crc_expect: k_bgzf_crc32 on the round buffer, before the scan passes)
    if(rc != HLALA_OK) return out(rc);
    std::vector<uint8_t> tmp;
    for(int64_t k = 0; k < R->n_blocks; k++) {
        const hlala_bgzf_block& b = R->blocks[k];
        R->bytes_h2d += b.clen;
        if(status[(size_t)k] == HLALA_INFLATE_OK) { R->n_gpu++; continue; }
        // the host engine's verdict stands (with crc_expect, host_inflate checks the CRC of what it inflated); its bytes go into place before the scan
        if(status[(size_t)k] == HLALA_INFLATE_CRC_MISMATCH) R->n_crc_recheck++;
        tmp.resize(b.isize ? b.isize : 1);
        if(R->host_inflate(R->user, k, tmp.data()) != 0) { f->err = "the host engine rejected the block as well"; return out(HLALA_E_STATE); }
        if(b.isize && (e = hipMemcpy(dData + R->carry + b.uoff, tmp.data(), b.isize, hipMemcpyHostToDevice)) != hipSuccess) return failed("upload of a block inflated on the host");
        R->n_retried++; R->bytes_h2d += b.isize;
    }
    R->s_inflate = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    const auto t1 = std::chrono::steady_clock::now();
    if(const char* bad = hlala_bamscan::scan_check_args(dData, n, R->first, R->in, nullptr, 0, nullptr, 0, &R->stats)) { f->err = std::string("BAM record pass: ") + bad; return out(HLALA_E_ARG); }
    ScanSink sink{R->user, R->alloc_recs, R->alloc_compact};
    rc = scan_run(f, nullptr, n, R->first, R->last, R->in, sink, &R->stats);
    if(rc != HLALA_OK) return out(rc);
    if(R->stats.status == HLALA_BAMSCAN_OK) R->bytes_d2h += R->stats.n_recs * (int64_t)sizeof(hlala_bam_rec) + R->stats.compact_bytes;
    if(R->stats.status == HLALA_BAMSCAN_TOO_MANY_REHOPS) {
        uint8_t* fb = R->alloc_fallback(R->user, n ? n : 1);
        if(!fb) { f->err = "no memory for the round's bytes"; return out(HLALA_E_STATE); }
        if(n && (e = hipMemcpy(fb, dData, n, hipMemcpyDeviceToHost)) != hipSuccess) return failed("download of the round");
        R->fell_back = true; R->bytes_d2h += (int64_t)n;
    }
    // HLALA_SEEDS_GPU_GROUP: the round's descriptors and names join the sample-long arrays while both still stand in the scan's device buffers
    R->group_appended = false;
    if(R->group) {
        if(R->group_first) group_reset(f);
        if(R->stats.status == HLALA_BAMSCAN_OK && f->grp.ok) {
            rc = R->stats.n_recs ? group_append(f, (const hlala_bam_rec*)f->scan[SCAN_RECS].p, R->stats.n_recs, (const uint8_t*)f->scan[SCAN_COMPACT].p, (size_t)R->stats.compact_bytes) : HLALA_OK;
            if(rc != HLALA_OK) return out(rc);
            R->group_appended = f->grp.ok;
        } else f->grp.ok = false;
    }
    // HLALA_SEEDS_GPU_FILL: ... and stay on the device whole, for the fill hook
    R->kept = false;
    if(R->keep && R->group) {
        if(R->group_first) keep_reset(f);
        if(R->group_appended && f->keep.ok) {
            rc = R->stats.n_recs ? keep_append(f, (const hlala_bam_rec*)f->scan[SCAN_RECS].p, R->stats.n_recs, (const uint8_t*)f->scan[SCAN_COMPACT].p, (size_t)R->stats.compact_bytes) : HLALA_OK;
            if(rc != HLALA_OK) return out(rc);
            R->kept = f->keep.ok;
        } else if(f->keep.ok || f->keep.recs.p) keep_drop(f);
    }
    R->s_scan = std::chrono::duration<double>(std::chrono::steady_clock::now() - t1).count();
    return HLALA_OK;
}

// ---- grouping by read name (include/hlala_gpu.h; kernel_bamgroup.hip).  Append per round on the scan's stream; after the last round one stretch of that stream: sort, mark,
// run ids, fold, emit, download.  The host looks at the device twice per round (how many name bytes the round brings: the arena may have to grow) and once at the end.
static void group_reset(hlala_inflater* f) { f->grp.n = 0; f->grp.nameBytes = 0; f->grp.msAppend = 0; f->grp.ok = true; f->grp.finished = false; f->grp.nComplete = 0; }
// `keep` bytes of the old buffer survive (device to device); the stream is idle when the old buffer is freed
static hipError_t group_grow(hlala_inflater* f, int which, size_t bytes, size_t keep, hipStream_t st)
{
    ScanBuf& b = f->grp.buf[which];
    if(bytes <= b.cap) return hipSuccess;
    const size_t want = keep ? 2 * bytes + 256 : bytes + bytes / 4 + 256;
    void* p = nullptr;
    hipError_t r = hipMalloc(&p, want);
    if(r != hipSuccess) return r;
    if(keep && b.p) { r = hipMemcpyAsync(p, b.p, keep, hipMemcpyDeviceToDevice, st); if(r == hipSuccess) r = hipStreamSynchronize(st); if(r != hipSuccess) { (void)hipFree(p); return r; } }
    if(b.p) (void)hipFree(b.p);
    b.p = p; b.cap = want;
    return hipSuccess;
}
static hipError_t group_events(hlala_inflater* f)
{
    if(f->grp.evReady) return hipSuccess;
    for(hipEvent_t& ev : f->grp.ev) if(!ev) { const hipError_t e = hipEventCreate(&ev); if(e != hipSuccess) return e; }
    f->grp.evReady = true;
    return hipSuccess;
}
// n (> 0) descriptors in device memory, their names in dBytes[0, nBytes), appended.  An allocation that fails is no error of the call: grp.ok = false, the caller decides.
static int group_append(hlala_inflater* f, const hlala_bam_rec* dRecs, int64_t n, const uint8_t* dBytes, size_t nBytes)
{
    GroupState& G = f->grp;
    if(G.n + n >= ((int64_t)1 << 31)) { G.ok = false; return HLALA_OK; }
    DevGuard g(f->device);
    hipStream_t st = f->slot[0].stream;
    hipError_t e = hipSuccess;
    auto failed = [&](const char* what) { f->err = std::string("BAM grouping: ") + what + ": " + hipGetErrorString(e); (void)hipStreamSynchronize(st); (void)hipGetLastError(); return HLALA_E_DEVICE; };
    auto no_memory = [&]() { (void)hipGetLastError(); G.ok = false; return HLALA_OK; };
    if((e = group_events(f)) != hipSuccess) return failed("hipEventCreate");
    const u32 N = (u32)n, nb = (N + 63u) / 64u, nb1 = (N + 64u) / 64u;
    size_t cubBytes = 0;
    if((e = group_grow(f, GRP_LEN, ((size_t)N + 1) * 8, 0, st)) != hipSuccess || (e = group_grow(f, GRP_OFF, ((size_t)N + 1) * 8, 0, st)) != hipSuccess) return no_memory();
    u64* dLen = (u64*)G.buf[GRP_LEN].p; u64* dOff = (u64*)G.buf[GRP_OFF].p;
    if((e = hipcub::DeviceScan::ExclusiveSum(nullptr, cubBytes, dLen, dOff, (int)N, st)) != hipSuccess) return failed("hipcub::DeviceScan::ExclusiveSum");
    if((e = group_grow(f, GRP_CUB, cubBytes + 16, 0, st)) != hipSuccess) return no_memory();
    e = hipEventRecord(G.ev[0], st);
    if(e == hipSuccess) { hipLaunchKernelGGL(k_grp_len, dim3(nb1), dim3(64), 0, st, dRecs, N, dLen); e = hipGetLastError(); }
    if(e == hipSuccess) e = hipcub::DeviceScan::ExclusiveSum(G.buf[GRP_CUB].p, cubBytes, dLen, dOff, (int)N, st);
    u64 last[2] = {0, 0};
    if(e == hipSuccess) e = hipMemcpyAsync(&last[0], dOff + (N - 1), 8, hipMemcpyDeviceToHost, st);
    if(e == hipSuccess) e = hipMemcpyAsync(&last[1], dLen + (N - 1), 8, hipMemcpyDeviceToHost, st);
    if(e == hipSuccess) e = hipStreamSynchronize(st);
    if(e != hipSuccess) return failed("k_grp_len / the scan of the name lengths");
    const u64 roundNames = last[0] + last[1];
    if(roundNames > (u64)N * 65535u) { f->err = "BAM grouping: more name bytes than the descriptors can hold"; return HLALA_E_DEVICE; }      // (cannot happen)
    const size_t have = (size_t)G.n, total = have + (size_t)N;
    if((e = group_grow(f, GRP_HASH, total * 8, have * 8, st)) != hipSuccess || (e = group_grow(f, GRP_META, total * 4, have * 4, st)) != hipSuccess ||
       (e = group_grow(f, GRP_NAMEOFF, total * 8, have * 8, st)) != hipSuccess || (e = group_grow(f, GRP_NAMES, (size_t)(G.nameBytes + roundNames) + 1, (size_t)G.nameBytes, st)) != hipSuccess) return no_memory();
    hipLaunchKernelGGL(k_grp_append, dim3(nb), dim3(64), 0, st, dRecs, N, dBytes, (u64)nBytes, (const u64*)dOff, (u64)G.nameBytes, (u64*)G.buf[GRP_HASH].p + have, (u32*)G.buf[GRP_META].p + have,
                       (u64*)G.buf[GRP_NAMEOFF].p + have, (uint8_t*)G.buf[GRP_NAMES].p, (u64)(G.nameBytes + roundNames));
    e = hipGetLastError();
    if(e == hipSuccess) e = hipEventRecord(G.ev[1], st);
    if(e == hipSuccess) e = hipStreamSynchronize(st);
    if(e != hipSuccess) return failed("k_grp_append");
    { float t = 0; if(hipEventElapsedTime(&t, G.ev[0], G.ev[1]) == hipSuccess) G.msAppend += (double)t; }
    G.n = (int64_t)total; G.nameBytes += roundNames;
    return HLALA_OK;
}
// the passes over the G.n (> 0) appended descriptors; perm / flag are host memory.  *noMemory: a device allocation failed, nothing ran.
static int group_finish(hlala_inflater* f, int32_t long_read_mode, uint32_t* perm, uint8_t* flag, hlala_bam_group_stats* stats, bool* noMemory)
{
    GroupState& G = f->grp;
    *noMemory = false; G.finished = false;
    DevGuard g(f->device);
    hipStream_t st = f->slot[0].stream;
    hipError_t e = hipSuccess;
    auto failed = [&](const char* what) { f->err = std::string("BAM grouping: ") + what + ": " + hipGetErrorString(e); (void)hipStreamSynchronize(st); (void)hipGetLastError(); return HLALA_E_DEVICE; };
    if((e = group_events(f)) != hipSuccess) return failed("hipEventCreate");
    const u32 N = (u32)G.n, nb = (N + 63u) / 64u, nb1 = (N + 64u) / 64u;
    const u64* dHash = (const u64*)G.buf[GRP_HASH].p; const u32* dMeta = (const u32*)G.buf[GRP_META].p; const u64* dNameOff = (const u64*)G.buf[GRP_NAMEOFF].p; const uint8_t* dNames = (const uint8_t*)G.buf[GRP_NAMES].p;
    size_t cubSort = 0, cubScan = 0;
    if((e = hipcub::DeviceRadixSort::SortPairs(nullptr, cubSort, dHash, (u64*)nullptr, (const u32*)nullptr, (u32*)nullptr, (int)N, 0, 64, st)) != hipSuccess) return failed("hipcub::DeviceRadixSort::SortPairs");
    if((e = hipcub::DeviceScan::ExclusiveSum(nullptr, cubScan, (u32*)nullptr, (u32*)nullptr, (int)N, st)) != hipSuccess) return failed("hipcub::DeviceScan::ExclusiveSum");
    if((e = group_grow(f, GRP_CUB, std::max(cubSort, cubScan) + 16, 0, st)) != hipSuccess || (e = group_grow(f, GRP_KEYS, (size_t)N * 8, 0, st)) != hipSuccess ||
       (e = group_grow(f, GRP_VAL_IN, (size_t)N * 4, 0, st)) != hipSuccess || (e = group_grow(f, GRP_VAL_OUT, (size_t)N * 4, 0, st)) != hipSuccess ||
       (e = group_grow(f, GRP_START, ((size_t)N + 1) * 4, 0, st)) != hipSuccess || (e = group_grow(f, GRP_RUNOFF, ((size_t)N + 1) * 4, 0, st)) != hipSuccess ||
       (e = group_grow(f, GRP_NEQ, (size_t)N, 0, st)) != hipSuccess || (e = group_grow(f, GRP_WORD, (size_t)N * 4, 0, st)) != hipSuccess || (e = group_grow(f, GRP_FLAG, (size_t)N, 0, st)) != hipSuccess ||
       (e = group_grow(f, GRP_COUNTS, 3 * 8, 0, st)) != hipSuccess) { (void)hipGetLastError(); *noMemory = true; return HLALA_OK; }
    u64* dKeys = (u64*)G.buf[GRP_KEYS].p; u32* dVin = (u32*)G.buf[GRP_VAL_IN].p; u32* dPerm = (u32*)G.buf[GRP_VAL_OUT].p; u32* dStart = (u32*)G.buf[GRP_START].p; u32* dRunOff = (u32*)G.buf[GRP_RUNOFF].p;
    uint8_t* dNeq = (uint8_t*)G.buf[GRP_NEQ].p; u32* dWord = (u32*)G.buf[GRP_WORD].p; uint8_t* dFlag = (uint8_t*)G.buf[GRP_FLAG].p; unsigned long long* dCounts = (unsigned long long*)G.buf[GRP_COUNTS].p;
    hipEvent_t* ev = G.ev;
    auto ms = [&](int a, int b) { float t = 0; return hipEventElapsedTime(&t, ev[a], ev[b]) == hipSuccess ? (double)t : 0.0; };
    e = hipEventRecord(ev[2], st);
    if(e == hipSuccess) { hipLaunchKernelGGL(k_grp_iota, dim3(nb), dim3(64), 0, st, N, dVin); e = hipGetLastError(); }
    if(e == hipSuccess) e = hipcub::DeviceRadixSort::SortPairs(G.buf[GRP_CUB].p, cubSort, dHash, dKeys, (const u32*)dVin, dPerm, (int)N, 0, 64, st);
    if(e == hipSuccess) e = hipEventRecord(ev[3], st);
    if(e == hipSuccess) { hipLaunchKernelGGL(k_grp_mark, dim3(nb1), dim3(64), 0, st, N, (const u64*)dKeys, (const u32*)dPerm, dMeta, dNameOff, dNames, (u64)G.nameBytes, dStart, dNeq); e = hipGetLastError(); }
    if(e == hipSuccess) e = hipcub::DeviceScan::ExclusiveSum(G.buf[GRP_CUB].p, cubScan, dStart, dRunOff, (int)N, st);
    if(e == hipSuccess) e = hipEventRecord(ev[4], st);
    if(e == hipSuccess) e = hipMemsetAsync(dWord, 0, (size_t)N * 4, st);
    if(e == hipSuccess) e = hipMemsetAsync(dCounts, 0, 3 * 8, st);
    if(e == hipSuccess) { hipLaunchKernelGGL(k_grp_fold, dim3(nb), dim3(64), 0, st, N, (const u32*)dPerm, dMeta, (const u32*)dStart, (const u32*)dRunOff, (const uint8_t*)dNeq, dWord); e = hipGetLastError(); }
    if(e == hipSuccess) e = hipEventRecord(ev[5], st);
    if(e == hipSuccess) { hipLaunchKernelGGL(k_grp_emit, dim3(nb), dim3(64), 0, st, N, (const u32*)dStart, (const u32*)dRunOff, (const u32*)dWord, (int)(long_read_mode ? 1 : 0), dFlag, dCounts); e = hipGetLastError(); }
    if(e == hipSuccess) e = hipEventRecord(ev[6], st);
    unsigned long long hCounts[3] = {0, 0, 0}; u32 lastRun[2] = {0, 0};
    if(e == hipSuccess) e = hipMemcpyAsync(perm, dPerm, (size_t)N * 4, hipMemcpyDeviceToHost, st);
    if(e == hipSuccess) e = hipMemcpyAsync(flag, dFlag, (size_t)N, hipMemcpyDeviceToHost, st);
    if(e == hipSuccess) e = hipMemcpyAsync(hCounts, dCounts, sizeof(hCounts), hipMemcpyDeviceToHost, st);
    if(e == hipSuccess) e = hipMemcpyAsync(&lastRun[0], dRunOff + (N - 1), 4, hipMemcpyDeviceToHost, st);
    if(e == hipSuccess) e = hipMemcpyAsync(&lastRun[1], dStart + (N - 1), 4, hipMemcpyDeviceToHost, st);
    if(e == hipSuccess) e = hipEventRecord(ev[7], st);
    if(e == hipSuccess) e = hipStreamSynchronize(st);
    if(e != hipSuccess) return failed("sort / k_grp_mark / k_grp_fold / k_grp_emit / download");
    stats->n_recs = G.n; stats->n_runs = (int64_t)lastRun[0] + lastRun[1]; stats->n_collided_runs = (int64_t)hCounts[0]; stats->n_units_complete = (int64_t)hCounts[1]; stats->n_units_incomplete = (int64_t)hCounts[2];
    stats->ms_append = G.msAppend; stats->ms_sort = ms(2, 3); stats->ms_mark = ms(3, 4); stats->ms_fold = ms(4, 5); stats->ms_emit = ms(5, 6); stats->ms_d2h = ms(6, 7);
    G.finished = true; G.nComplete = stats->n_units_complete;
    return HLALA_OK;
}
extern "C" int hlala_bam_group_rounds(hlala_inflater* f, const hlala_bam_rec* recs, int64_t n, const uint8_t* bytes, size_t n_bytes, const int64_t* round_recs, int32_t n_rounds,
                                      int32_t long_read_mode, uint32_t* perm, uint8_t* flag, hlala_bam_group_stats* stats)
{
    if(!f) { int ndev = 0; if(hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { (void)hipGetLastError(); return HLALA_E_DEVICE; } return HLALA_E_ARG; }
    f->err.clear();
    const char* bad = hlala_bamgroup::grp_check_args(recs, n, bytes, n_bytes, perm, flag, stats);
    if(!bad) bad = hlala_bamgroup::grp_check_rounds(round_recs, n_rounds, n);
    if(bad) { f->err = std::string("hlala_bam_group: ") + bad; return HLALA_E_ARG; }
    const auto tWall = std::chrono::steady_clock::now();
    memset(stats, 0, sizeof(*stats));
    group_reset(f);
    if(n == 0) return HLALA_OK;
    DevGuard g(f->device);
    hipStream_t st = f->slot[0].stream;
    hipError_t e = hipSuccess;
    auto failed = [&](const char* what) { f->err = std::string("hlala_bam_group: ") + what + ": " + hipGetErrorString(e); (void)hipStreamSynchronize(st); (void)hipGetLastError(); return HLALA_E_DEVICE; };
    if((e = group_events(f)) != hipSuccess) return failed("hipEventCreate");
    if((e = group_grow(f, GRP_IN_RECS, (size_t)n * sizeof(hlala_bam_rec), 0, st)) != hipSuccess || (e = group_grow(f, GRP_IN_BYTES, n_bytes ? n_bytes : 1, 0, st)) != hipSuccess) return failed("hipMalloc");
    const hlala_bam_rec* dRecs = (const hlala_bam_rec*)f->grp.buf[GRP_IN_RECS].p; const uint8_t* dBytes = (const uint8_t*)f->grp.buf[GRP_IN_BYTES].p;
    e = hipEventRecord(f->grp.ev[2], st);
    if(e == hipSuccess) e = hipMemcpyAsync((void*)dRecs, recs, (size_t)n * sizeof(hlala_bam_rec), hipMemcpyHostToDevice, st);
    if(e == hipSuccess && n_bytes) e = hipMemcpyAsync((void*)dBytes, bytes, n_bytes, hipMemcpyHostToDevice, st);
    if(e == hipSuccess) e = hipEventRecord(f->grp.ev[3], st);
    if(e == hipSuccess) e = hipStreamSynchronize(st);
    if(e != hipSuccess) return failed("upload");
    float tUp = 0; (void)hipEventElapsedTime(&tUp, f->grp.ev[2], f->grp.ev[3]);
    int64_t at = 0;
    for(int32_t k = 0; k < n_rounds; k++) {
        if(round_recs[k] == 0) continue;
        const int rc = group_append(f, dRecs + at, round_recs[k], dBytes, n_bytes);
        if(rc != HLALA_OK) return rc;
        if(!f->grp.ok) { f->err = "hlala_bam_group: no device memory for the sample-long arrays"; return HLALA_E_DEVICE; }
        at += round_recs[k];
    }
    bool noMemory = false;
    const int rc = group_finish(f, long_read_mode, perm, flag, stats, &noMemory);
    if(rc != HLALA_OK) return rc;
    if(noMemory) { f->err = "hlala_bam_group: no device memory for the passes"; return HLALA_E_DEVICE; }
    stats->ms_h2d = (double)tUp;
    stats->ms_wall = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tWall).count();
    return HLALA_OK;
}
extern "C" int hlala_bam_group(hlala_inflater* f, const hlala_bam_rec* recs, int64_t n, const uint8_t* bytes, size_t n_bytes, int32_t long_read_mode, uint32_t* perm, uint8_t* flag,
                               hlala_bam_group_stats* stats)
{
    const int64_t one = n;
    return hlala_bam_group_rounds(f, recs, n, bytes, n_bytes, &one, n > 0 ? 1 : 0, long_read_mode, perm, flag, stats);
}
// The decoder's group phase with HLALA_SEEDS_GPU_GROUP: the passes over what the scan hook has appended round by round.
static int bam_group_hook(void* inflater, int64_t n, int32_t long_read_mode, uint32_t* perm, uint8_t* flag, hlala_bam_group_stats* stats, bool* available, std::string* err)
{
    hlala_inflater* f = (hlala_inflater*)inflater;
    if(!f || !stats || !available || n < 0 || (n && (!perm || !flag))) return HLALA_E_ARG;
    f->err.clear();
    memset(stats, 0, sizeof(*stats));
    *available = f->grp.ok && f->grp.n == n;
    if(!*available || n == 0) return HLALA_OK;
    const auto tWall = std::chrono::steady_clock::now();
    bool noMemory = false;
    const int rc = group_finish(f, long_read_mode, perm, flag, stats, &noMemory);
    if(rc != HLALA_OK) { if(err) *err = f->err; return rc; }
    if(noMemory) *available = false;
    stats->ms_wall = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tWall).count();
    return HLALA_OK;
}

// ---- the read-name order of names on the device (include/hlala_gpu.h; kernel_bamnameorder.hip).  One stretch of the scan's stream per round: key, sort (by key, then --
// beyond the first round -- stably by segment), mark, the scan, scatter; the host reads one count per round (the names still unresolved) and stops at zero.
static hipError_t nam_grow(hlala_inflater* f, int which, size_t bytes)
{
    ScanBuf& b = f->nam.buf[which];
    if(bytes <= b.cap) return hipSuccess;
    if(b.p) { (void)hipFree(b.p); b.p = nullptr; b.cap = 0; }
    const size_t want = bytes + bytes / 4 + 256;
    const hipError_t r = hipMalloc(&b.p, want);
    if(r != hipSuccess) { b.p = nullptr; return r; }
    b.cap = want;
    return hipSuccess;
}
static hipError_t nam_events(hlala_inflater* f)
{
    if(f->nam.evReady) return hipSuccess;
    for(hipEvent_t& ev : f->nam.ev) if(!ev) { const hipError_t e = hipEventCreate(&ev); if(e != hipSuccess) return e; }
    f->nam.evReady = true;
    return hipSuccess;
}
// n (> 0) names in device memory: name i is dNames[dOff[i] .. + dLen[i]).  order is host memory.  *noMemory: a device allocation failed, nothing ran.
static int nam_run(hlala_inflater* f, const u64* dOff, const u32* dLen, u32 n, const uint8_t* dNames, u64 nBytes, int64_t maxRounds, uint32_t* order, hlala_bam_name_order_stats* stats, bool* noMemory)
{
    NameOrderState& S = f->nam;
    *noMemory = false;
    hipStream_t st = f->slot[0].stream;
    hipError_t e = hipSuccess;
    auto failed = [&](const char* what) { f->err = std::string("BAM name order: ") + what + ": " + hipGetErrorString(e); (void)hipStreamSynchronize(st); (void)hipGetLastError(); return HLALA_E_DEVICE; };
    if((e = nam_events(f)) != hipSuccess) return failed("hipEventCreate");
    const size_t N = n;
    size_t cubKey = 0, cubSeg = 0, cubScan = 0;
    if((e = hipcub::DeviceRadixSort::SortPairs(nullptr, cubKey, (const u64*)nullptr, (u64*)nullptr, (const u32*)nullptr, (u32*)nullptr, N, 0, 64, st)) != hipSuccess) return failed("hipcub::DeviceRadixSort::SortPairs");
    if((e = hipcub::DeviceRadixSort::SortPairs(nullptr, cubSeg, (const u32*)nullptr, (u32*)nullptr, (const u32*)nullptr, (u32*)nullptr, N, 0, 32, st)) != hipSuccess) return failed("hipcub::DeviceRadixSort::SortPairs");
    if((e = hipcub::DeviceScan::ExclusiveSum(nullptr, cubScan, (u64*)nullptr, (u64*)nullptr, N + 1, st)) != hipSuccess) return failed("hipcub::DeviceScan::ExclusiveSum");
    const size_t cubBytes = std::max(std::max(cubKey, cubSeg), cubScan) + 16;
    static const int four[] = {NAM_IDX0, NAM_IDX1, NAM_SEG0, NAM_SEG1, NAM_GP0, NAM_GP1, NAM_VAL, NAM_P1, NAM_K2, NAM_K2S, NAM_P2, NAM_NEWIDX, NAM_ORDER};
    for(int w : four) if((e = nam_grow(f, w, N * 4)) != hipSuccess) break;
    if(e != hipSuccess || (e = nam_grow(f, NAM_KEY, N * 8)) != hipSuccess || (e = nam_grow(f, NAM_KEYS, N * 8)) != hipSuccess || (e = nam_grow(f, NAM_FL, (N + 1) * 8)) != hipSuccess ||
       (e = nam_grow(f, NAM_FLOFF, (N + 1) * 8)) != hipSuccess || (e = nam_grow(f, NAM_COUNT, 8)) != hipSuccess || (e = nam_grow(f, NAM_CUB, cubBytes)) != hipSuccess) { (void)hipGetLastError(); *noMemory = true; return HLALA_OK; }
    auto u32buf = [&](int w) { return (u32*)S.buf[w].p; };
    u32 *idx = u32buf(NAM_IDX0), *idx2 = u32buf(NAM_IDX1), *seg = u32buf(NAM_SEG0), *seg2 = u32buf(NAM_SEG1), *gp = u32buf(NAM_GP0), *gp2 = u32buf(NAM_GP1);
    u32 *dVal = u32buf(NAM_VAL), *dP1 = u32buf(NAM_P1), *dK2 = u32buf(NAM_K2), *dK2s = u32buf(NAM_K2S), *dP2 = u32buf(NAM_P2), *dNewIdx = u32buf(NAM_NEWIDX), *dOrder = u32buf(NAM_ORDER);
    u64 *dKey = (u64*)S.buf[NAM_KEY].p, *dKeys = (u64*)S.buf[NAM_KEYS].p, *dFl = (u64*)S.buf[NAM_FL].p, *dFlOff = (u64*)S.buf[NAM_FLOFF].p;
    unsigned long long* dEqual = (unsigned long long*)S.buf[NAM_COUNT].p;
    void* dCub = S.buf[NAM_CUB].p;
    hipEvent_t* ev = S.ev;
    auto ms = [&](int a, int b) { float t = 0; return hipEventElapsedTime(&t, ev[a], ev[b]) == hipSuccess ? (double)t : 0.0; };
    e = hipMemsetAsync(dEqual, 0, 8, st);
    if(e == hipSuccess) { hipLaunchKernelGGL(k_nam_init, dim3((n + 63u) / 64u), dim3(64), 0, st, n, idx, seg, gp); e = hipGetLastError(); }
    if(e != hipSuccess) return failed("k_nam_init");
    u32 a = n;
    for(u32 r = 0; a > 0; r++) {
        if((int64_t)r >= maxRounds) { (void)hipStreamSynchronize(st); f->err = "BAM name order: names unresolved after the last round"; return HLALA_E_DEVICE; }      // (cannot happen)
        const u32 nb = (a + 63u) / 64u, nb1 = (a + 64u) / 64u;
        // after a round every segment of the working set has two names or more: at most a / 2 segments, so many bits of the second sort's key count
        const u32 maxSegs = r == 0 ? 1u : a / 2u;
        int segBits = 0; while(segBits < 32 && (1ull << segBits) < maxSegs) segBits++;
        const u32* p = dP1;
        e = hipEventRecord(ev[0], st);
        if(e == hipSuccess) { hipLaunchKernelGGL(k_nam_key, dim3(nb), dim3(64), 0, st, a, n, (const u32*)idx, dOff, dLen, dNames, nBytes, r, dKey, dVal); e = hipGetLastError(); }
        if(e == hipSuccess) e = hipEventRecord(ev[1], st);
        if(e == hipSuccess) e = hipcub::DeviceRadixSort::SortPairs(dCub, cubKey, (const u64*)dKey, dKeys, (const u32*)dVal, dP1, (size_t)a, 0, 64, st);
        if(e == hipSuccess && segBits > 0) {
            hipLaunchKernelGGL(k_nam_seg, dim3(nb), dim3(64), 0, st, a, (const u32*)dP1, (const u32*)seg, dK2); e = hipGetLastError();
            if(e == hipSuccess) e = hipcub::DeviceRadixSort::SortPairs(dCub, cubSeg, (const u32*)dK2, dK2s, (const u32*)dP1, dP2, (size_t)a, 0, segBits, st);
            p = dP2;
        }
        if(e == hipSuccess) e = hipEventRecord(ev[2], st);
        if(e == hipSuccess) { hipLaunchKernelGGL(k_nam_mark, dim3(nb1), dim3(64), 0, st, a, p, (const u64*)dKey, (const u32*)seg, (const u32*)idx, dNewIdx, dFl, dEqual); e = hipGetLastError(); }
        if(e == hipSuccess) e = hipcub::DeviceScan::ExclusiveSum(dCub, cubScan, dFl, dFlOff, (size_t)a + 1, st);
        if(e == hipSuccess) e = hipEventRecord(ev[3], st);
        if(e == hipSuccess) { hipLaunchKernelGGL(k_nam_scatter, dim3(nb), dim3(64), 0, st, a, n, (const u64*)dFl, (const u64*)dFlOff, (const u32*)dNewIdx, (const u32*)gp, dOrder, idx2, seg2, gp2); e = hipGetLastError(); }
        if(e == hipSuccess) e = hipEventRecord(ev[4], st);
        u64 total = 0;
        if(e == hipSuccess) e = hipMemcpyAsync(&total, dFlOff + a, 8, hipMemcpyDeviceToHost, st);
        if(e == hipSuccess) e = hipStreamSynchronize(st);
        if(e != hipSuccess) return failed("k_nam_key / sort / k_nam_mark / k_nam_scatter");
        stats->n_rounds++; stats->ms_key += ms(0, 1); stats->ms_sort += ms(1, 2); stats->ms_mark += ms(2, 3); stats->ms_scatter += ms(3, 4);
        const u32 left = (u32)total;
        if(left > a || left == 1) { f->err = "BAM name order: an impossible count of unresolved names"; return HLALA_E_DEVICE; }      // (cannot happen)
        std::swap(idx, idx2); std::swap(seg, seg2); std::swap(gp, gp2);
        a = left;
    }
    unsigned long long hEqual = 0;
    e = hipEventRecord(ev[5], st);
    if(e == hipSuccess) e = hipMemcpyAsync(order, dOrder, N * 4, hipMemcpyDeviceToHost, st);
    if(e == hipSuccess) e = hipMemcpyAsync(&hEqual, dEqual, 8, hipMemcpyDeviceToHost, st);
    if(e == hipSuccess) e = hipEventRecord(ev[6], st);
    if(e == hipSuccess) e = hipStreamSynchronize(st);
    if(e != hipSuccess) return failed("download");
    stats->n = (int64_t)n; stats->n_equal_names = (int64_t)hEqual; stats->ms_d2h = ms(5, 6);
    return HLALA_OK;
}
extern "C" int hlala_bam_name_order(hlala_inflater* f, const uint64_t* name_off, const uint32_t* name_len, int64_t n, const uint8_t* bytes, size_t n_bytes, uint32_t* order,
                                    hlala_bam_name_order_stats* stats)
{
    if(!f) { int ndev = 0; if(hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { (void)hipGetLastError(); return HLALA_E_DEVICE; } return HLALA_E_ARG; }
    f->err.clear();
    uint32_t maxLen = 0;
    const char* bad = hlala_nameorder::nam_check_args(name_off, name_len, n, bytes, n_bytes, order, stats, &maxLen);
    if(bad) { f->err = std::string("hlala_bam_name_order: ") + bad; return HLALA_E_ARG; }
    const auto tWall = std::chrono::steady_clock::now();
    memset(stats, 0, sizeof(*stats));
    if(n == 0) return HLALA_OK;
    DevGuard g(f->device);
    hipStream_t st = f->slot[0].stream;
    hipError_t e = hipSuccess;
    auto failed = [&](const char* what) { f->err = std::string("hlala_bam_name_order: ") + what + ": " + hipGetErrorString(e); (void)hipStreamSynchronize(st); (void)hipGetLastError(); return HLALA_E_DEVICE; };
    if((e = nam_events(f)) != hipSuccess) return failed("hipEventCreate");
    if((e = nam_grow(f, NAM_IN_OFF, (size_t)n * 8)) != hipSuccess || (e = nam_grow(f, NAM_IN_LEN, (size_t)n * 4)) != hipSuccess || (e = nam_grow(f, NAM_IN_BYTES, n_bytes)) != hipSuccess) return failed("hipMalloc");
    u64* dOff = (u64*)f->nam.buf[NAM_IN_OFF].p; u32* dLen = (u32*)f->nam.buf[NAM_IN_LEN].p; uint8_t* dBytes = (uint8_t*)f->nam.buf[NAM_IN_BYTES].p;
    e = hipEventRecord(f->nam.ev[5], st);
    if(e == hipSuccess) e = hipMemcpyAsync(dOff, name_off, (size_t)n * 8, hipMemcpyHostToDevice, st);
    if(e == hipSuccess) e = hipMemcpyAsync(dLen, name_len, (size_t)n * 4, hipMemcpyHostToDevice, st);
    if(e == hipSuccess) e = hipMemcpyAsync(dBytes, bytes, n_bytes, hipMemcpyHostToDevice, st);
    if(e == hipSuccess) e = hipEventRecord(f->nam.ev[6], st);
    if(e == hipSuccess) e = hipStreamSynchronize(st);
    if(e != hipSuccess) return failed("upload");
    float tUp = 0; (void)hipEventElapsedTime(&tUp, f->nam.ev[5], f->nam.ev[6]);
    bool noMemory = false;
    const int rc = nam_run(f, dOff, dLen, (u32)n, dBytes, (u64)n_bytes, hlala_nameorder::nam_max_rounds(maxLen), order, stats, &noMemory);
    if(rc != HLALA_OK) return rc;
    if(noMemory) { f->err = "hlala_bam_name_order: no device memory for the passes"; return HLALA_E_DEVICE; }
    stats->ms_h2d = (double)tUp;
    stats->ms_wall = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tWall).count();
    return HLALA_OK;
}
// The decoder's sort phase with HLALA_SEEDS_GPU_SORT: directly behind group_finish, on its stream and over its arrays -- the first records of clean, complete runs are
// selected in run order (k_nam_select, a scan, k_nam_units), their names ordered where they lie in the arena.  Nothing is uploaded.  *available = false (with HLALA_OK):
// the grouping passes have not run over this sample, or a device allocation failed -- the host orders the sample itself.
static int bam_sort_hook(void* inflater, int64_t m, uint32_t* order, hlala_bam_name_order_stats* stats, bool* available, std::string* err)
{
    hlala_inflater* f = (hlala_inflater*)inflater;
    if(!f || !stats || !available || m < 0 || (m && !order)) return HLALA_E_ARG;
    f->err.clear();
    memset(stats, 0, sizeof(*stats));
    GroupState& G = f->grp;
    *available = G.ok && (G.finished || G.n == 0);
    if(!*available) return HLALA_OK;
    auto fail = [&](int rc) { if(err) *err = f->err; return rc; };
    if(m != G.nComplete) { f->err = "BAM name order: the host holds " + std::to_string(m) + " units of clean runs, the grouping passes found " + std::to_string(G.nComplete); return fail(HLALA_E_DEVICE); }
    if(m == 0) return HLALA_OK;
    const auto tWall = std::chrono::steady_clock::now();
    DevGuard g(f->device);
    hipStream_t st = f->slot[0].stream;
    hipError_t e = hipSuccess;
    auto failed = [&](const char* what) { f->err = std::string("BAM name order: ") + what + ": " + hipGetErrorString(e); (void)hipStreamSynchronize(st); (void)hipGetLastError(); return fail(HLALA_E_DEVICE); };
    const u32 N = (u32)G.n, M = (u32)m;
    size_t cubScan = 0;
    if((e = hipcub::DeviceScan::ExclusiveSum(nullptr, cubScan, (u32*)nullptr, (u32*)nullptr, (size_t)N + 1, st)) != hipSuccess) return failed("hipcub::DeviceScan::ExclusiveSum");
    if((e = nam_grow(f, NAM_SEL, ((size_t)N + 1) * 4)) != hipSuccess || (e = nam_grow(f, NAM_SELOFF, ((size_t)N + 1) * 4)) != hipSuccess || (e = nam_grow(f, NAM_IN_OFF, (size_t)M * 8)) != hipSuccess ||
       (e = nam_grow(f, NAM_IN_LEN, (size_t)M * 4)) != hipSuccess || (e = nam_grow(f, NAM_CUB, cubScan + 16)) != hipSuccess) { (void)hipGetLastError(); *available = false; return HLALA_OK; }
    u32* dSel = (u32*)f->nam.buf[NAM_SEL].p; u32* dSelOff = (u32*)f->nam.buf[NAM_SELOFF].p; u64* dOff = (u64*)f->nam.buf[NAM_IN_OFF].p; u32* dLen = (u32*)f->nam.buf[NAM_IN_LEN].p;
    hipLaunchKernelGGL(k_nam_select, dim3((N + 64u) / 64u), dim3(64), 0, st, N, (const uint8_t*)G.buf[GRP_FLAG].p, dSel); e = hipGetLastError();
    if(e == hipSuccess) e = hipcub::DeviceScan::ExclusiveSum(f->nam.buf[NAM_CUB].p, cubScan, dSel, dSelOff, (size_t)N + 1, st);
    if(e == hipSuccess) { hipLaunchKernelGGL(k_nam_units, dim3((N + 63u) / 64u), dim3(64), 0, st, N, (const u32*)dSel, (const u32*)dSelOff, (const u32*)G.buf[GRP_VAL_OUT].p, (const u32*)G.buf[GRP_META].p,
                                                (const u64*)G.buf[GRP_NAMEOFF].p, M, dOff, dLen); e = hipGetLastError(); }
    u32 found = 0;
    if(e == hipSuccess) e = hipMemcpyAsync(&found, dSelOff + N, 4, hipMemcpyDeviceToHost, st);
    if(e == hipSuccess) e = hipStreamSynchronize(st);
    if(e != hipSuccess) return failed("k_nam_select / k_nam_units");
    if(found != M) { f->err = "BAM name order: " + std::to_string(found) + " first records of clean, complete runs, the grouping passes counted " + std::to_string(m); return fail(HLALA_E_DEVICE); }
    bool noMemory = false;
    const int rc = nam_run(f, dOff, dLen, M, (const uint8_t*)G.buf[GRP_NAMES].p, (u64)G.nameBytes, hlala_nameorder::nam_max_rounds(hlala_nameorder::NAM_MAX_LEN), order, stats, &noMemory);
    if(rc != HLALA_OK) return fail(rc);
    if(noMemory) *available = false;
    stats->ms_wall = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tWall).count();
    return HLALA_OK;
}

// ---- the layout and the fill on the device (include/hlala_gpu.h; kernel_bamfill.hip).  A handle of its own: the sample's descriptors, bytes, permutation and unit
// arrays, what the layout passes leave (offsets, chain sources, primaries), a stream, events, one device block and one page-locked block for a window's slices.
enum { FIL_RECS, FIL_BYTES, FIL_PERM, FIL_UFIRST, FIL_UCOUNT, FIL_SIZES, FIL_OFFS, FIL_CHAINSRC, FIL_CHAINCIG, FIL_PRIMARY, FIL_WIN, FIL_WIDE, FIL_NBUF };      // FIL_WIDE: only for a sample with wide units
// the wide units of a sample as the host found them (hlala_bam_fill_create_wide from the descriptors, the decoder from its own records); null: the narrow layout
struct FillWideIn { int32_t maxMate; const u32* units; size_t n; int64_t longest; };
constexpr int FIL_NEV = 8;
struct hlala_bam_fill {
    int device = 0; hipStream_t st = nullptr; hipEvent_t ev[FIL_NEV]{};
    ScanBuf buf[FIL_NBUF];
    FilSample S{}; int packed = 0; u64 nReads = 0, nChains = 0;
    uint8_t* hStage = nullptr; size_t stageCap = 0; int64_t* hBounds = nullptr;
    std::vector<u32> hostUnit;       // the host units, ascending (hlala_batch_create_from_fill places their ranges)
    hipEvent_t wev[4]{}; int64_t wideStats[4] = {0, 0, 0, 0};      // wide units, wide reads, the longest mate, device microseconds of k_fil_wide_rank + k_fil_wide_src
    std::string err;
    int64_t* off(int which) const { return (int64_t*)buf[FIL_OFFS].p + (size_t)which * (nReads + 1); }      // 0 read_off, 1 chain_off, 2 cigar_count, 3 name_off
};
static void fill_free(hlala_bam_fill* H)
{
    if(!H) return;
    DevGuard g(H->device);
    if(H->st) (void)hipStreamSynchronize(H->st);
    for(ScanBuf& b : H->buf) if(b.p) (void)hipFree(b.p);
    for(hipEvent_t e : H->ev) if(e) (void)hipEventDestroy(e);
    for(hipEvent_t e : H->wev) if(e) (void)hipEventDestroy(e);
    if(H->hStage) (void)hipHostFree(H->hStage);
    if(H->hBounds) (void)hipHostFree(H->hBounds);
    if(H->st) (void)hipStreamDestroy(H->st);
    delete H;
}
static hipError_t fill_alloc(hlala_bam_fill* H, int which, size_t bytes)
{
    ScanBuf& b = H->buf[which];
    if(bytes <= b.cap && b.p) return hipSuccess;
    if(b.p) { (void)hipFree(b.p); b.p = nullptr; b.cap = 0; }
    const hipError_t r = hipMalloc(&b.p, bytes ? bytes : 1);
    if(r != hipSuccess) { b.p = nullptr; return r; }
    b.cap = bytes ? bytes : 1;
    return hipSuccess;
}
// The layout passes.  H holds FIL_RECS / FIL_BYTES (/ FIL_PERM) and S.n, S.nBytes; the unit arrays and the host units' sizes are host memory and are uploaded here.
// *noMemory: a device allocation failed, nothing of the sample is laid out (the decoder's hook hands the sample back; the entry point fails).
// wide (may be null): the sample's wide units, ascending; the scratch arrays, the bitmap and two more kernels exist only where it lists one.
static int fill_layout(hlala_bam_fill* H, const hlala_bam_fill_in* in, int64_t* read_off, int64_t* chain_off, int64_t* cigar_count, int64_t* name_off, hlala_bam_fill_stats* stats, bool* noMemory,
                       const FillWideIn* wide = nullptr)
{
    using namespace hlala_bamfill;
    *noMemory = false;
    hipStream_t st = H->st;
    hipError_t e = hipSuccess;
    auto failed = [&](const char* what) { H->err = std::string("BAM fill: ") + what + ": " + hipGetErrorString(e); (void)hipStreamSynchronize(st); (void)hipGetLastError(); return HLALA_E_DEVICE; };
    const u32 nm = (u32)fil_nm(in->long_read_mode);
    const size_t nU = (size_t)in->n_units, nR = nU * nm, nHost = (size_t)in->n_host_units, perHost = 3 * nm + 1;
    H->nReads = nR; H->packed = in->packed ? 1 : 0;
    std::vector<u32> hostUnit; hostUnit.reserve(nHost);
    for(size_t u = 0; u < nU; u++) if(in->unit_first[u] == FIL_HOST) hostUnit.push_back((u32)u);
    if(hostUnit.size() != nHost) { H->err = "BAM fill: the host units marked are not n_host_units"; return HLALA_E_ARG; }
    H->hostUnit = hostUnit;
    // ---- the wide units: list, slots per wide read (unit_count each), primaries, the bitmap, then the two scratch arrays -- one block of 32-bit words
    const size_t nWide = wide ? wide->n : 0, nWR = nWide * nm;
    std::vector<u32> wideWords; size_t wUnitAt = 0, wOffAt = 0, wPrimAt = 0, wMapAt = 0, wDescAt = 0, wCigAt = 0; u64 nSlots = 0;
    if(nWide) {
        const size_t mapWords = (nU + 31) / 32;
        wUnitAt = 0; wOffAt = nWide; wPrimAt = wOffAt + nWR + 1; wMapAt = wPrimAt + nWR; wDescAt = wMapAt + mapWords;
        wideWords.assign(wDescAt, 0u);
        for(size_t w = 0; w < nWide; w++) {
            const u32 u = wide->units[w];
            if(u >= nU || in->unit_first[u] == FIL_HOST || (w && u <= wide->units[w - 1])) { H->err = "BAM fill: the wide units are not an ascending list of filled units"; return HLALA_E_ARG; }
            wideWords[wUnitAt + w] = u; wideWords[wMapAt + (u >> 5)] |= 1u << (u & 31u);
            for(u32 m = 0; m < nm; m++) { wideWords[wOffAt + w * nm + m] = (u32)nSlots; nSlots += in->unit_count[u]; }
        }
        if(nSlots >= ((u64)1 << 32)) { H->err = "BAM fill: 2^32 or more alignments in wide units"; return HLALA_E_ARG; }
        wideWords[wOffAt + nWR] = (u32)nSlots; wCigAt = wDescAt + (size_t)nSlots;
        if((e = fill_alloc(H, FIL_WIDE, (wCigAt + (size_t)nSlots) * 4)) != hipSuccess) { (void)hipGetLastError(); *noMemory = true; return HLALA_OK; }
        for(hipEvent_t& ev : H->wev) if(!ev && (e = hipEventCreate(&ev)) != hipSuccess) { ev = nullptr; (void)hipGetLastError(); *noMemory = true; return HLALA_OK; }
    }
    FilWide Wd{};
    size_t cubBytes = 0;
    if((e = hipcub::DeviceScan::ExclusiveSum(nullptr, cubBytes, (int64_t*)nullptr, (int64_t*)nullptr, nR + 1, st)) != hipSuccess) return failed("hipcub::DeviceScan::ExclusiveSum");
    // FIL_SIZES: the four size arrays [nR + 1] each (name sizes use nU + 1 of theirs); behind them the host units' numbers and sizes, then the scan's scratch and the bad bits
    const size_t sizesBytes = 4 * (nR + 1) * 8, hostBytes = nHost * 4 + 8 + nHost * perHost * 8;
    if((e = fill_alloc(H, FIL_UFIRST, nU * 4)) != hipSuccess || (e = fill_alloc(H, FIL_UCOUNT, nU * 4)) != hipSuccess || (e = fill_alloc(H, FIL_SIZES, sizesBytes + hostBytes + cubBytes + 64)) != hipSuccess ||
       (e = fill_alloc(H, FIL_OFFS, sizesBytes)) != hipSuccess || (e = fill_alloc(H, FIL_PRIMARY, nR * 4)) != hipSuccess) { (void)hipGetLastError(); *noMemory = true; return HLALA_OK; }
    int64_t* dSize = (int64_t*)H->buf[FIL_SIZES].p;
    int64_t* dHostSizes = dSize + 4 * (nR + 1); u32* dHostUnit = (u32*)(dHostSizes + nHost * perHost); u32* dBad = dHostUnit + nHost + (nHost & 1);
    void* dCub = (void*)(((uintptr_t)(dBad + 2) + 15) & ~(uintptr_t)15);
    H->S.unitFirst = (const u32*)H->buf[FIL_UFIRST].p; H->S.unitCount = (const u32*)H->buf[FIL_UCOUNT].p; H->S.nUnits = (u32)nU; H->S.nm = nm; H->S.wide = nullptr;
    if(nWide) {
        u32* dW = (u32*)H->buf[FIL_WIDE].p;
        H->S.wide = dW + wMapAt;
        Wd.unit = dW + wUnitAt; Wd.off = dW + wOffAt; Wd.nUnits = (u32)nWide; Wd.maxMate = (u32)wide->maxMate; Wd.desc = dW + wDescAt; Wd.cig = dW + wCigAt; Wd.prim = dW + wPrimAt;
    }
    auto ms = [&](int a, int b) { float t = 0; return hipEventElapsedTime(&t, H->ev[a], H->ev[b]) == hipSuccess ? (double)t : 0.0; };
    e = hipEventRecord(H->ev[0], st);
    if(e == hipSuccess) e = hipMemcpyAsync(H->buf[FIL_UFIRST].p, in->unit_first, nU * 4, hipMemcpyHostToDevice, st);
    if(e == hipSuccess) e = hipMemcpyAsync(H->buf[FIL_UCOUNT].p, in->unit_count, nU * 4, hipMemcpyHostToDevice, st);
    if(e == hipSuccess && nHost) e = hipMemcpyAsync(dHostSizes, in->host_sizes, nHost * perHost * 8, hipMemcpyHostToDevice, st);
    if(e == hipSuccess && nHost) e = hipMemcpyAsync(dHostUnit, hostUnit.data(), nHost * 4, hipMemcpyHostToDevice, st);
    if(e == hipSuccess && nWide) e = hipMemcpyAsync(H->buf[FIL_WIDE].p, wideWords.data(), wideWords.size() * 4, hipMemcpyHostToDevice, st);      // (the stream is synchronised before wideWords goes)
    if(e == hipSuccess) e = hipMemsetAsync(dSize, 0, sizesBytes, st);
    if(e == hipSuccess) e = hipMemsetAsync(dBad, 0, 8, st);
    if(e == hipSuccess) e = hipMemsetAsync(H->buf[FIL_PRIMARY].p, 0, nR * 4, st);
    if(e == hipSuccess) e = hipEventRecord(H->ev[1], st);
    const u32 rankBlocks = (u32)((nR * 16 + 255) / 256);
    int64_t *sL = dSize, *sC = dSize + (nR + 1), *sG = dSize + 2 * (nR + 1), *sN = dSize + 3 * (nR + 1);
    if(e == hipSuccess) { hipLaunchKernelGGL(k_fil_rank, dim3(rankBlocks), dim3(256), 0, st, H->S, (u64)nR, sL, sC, sG, sN, dBad); e = hipGetLastError(); }
    if(e == hipSuccess && nWide) {                       // (inside ms_rank, and timed on its own)
        e = hipEventRecord(H->wev[0], st);
        if(e == hipSuccess) { hipLaunchKernelGGL(k_fil_wide_rank, dim3((u32)nWR), dim3(64), 0, st, H->S, Wd, sL, sC, sG, sN, dBad); e = hipGetLastError(); }
        if(e == hipSuccess) e = hipEventRecord(H->wev[1], st);
    }
    if(e == hipSuccess) e = hipEventRecord(H->ev[2], st);
    if(e == hipSuccess && nHost) { hipLaunchKernelGGL(k_fil_host, dim3((u32)((nHost + 63) / 64)), dim3(64), 0, st, (u32)nHost, (u32)nU, nm, (const u32*)dHostUnit, (const int64_t*)dHostSizes, sL, sC, sG, sN); e = hipGetLastError(); }
    if(e == hipSuccess) e = hipEventRecord(H->ev[3], st);
    for(int w = 0; w < 4 && e == hipSuccess; w++) e = hipcub::DeviceScan::ExclusiveSum(dCub, cubBytes, dSize + (size_t)w * (nR + 1), H->off(w), w == 3 ? nU + 1 : nR + 1, st);
    if(e == hipSuccess) e = hipEventRecord(H->ev[4], st);
    u32 hBad[2] = {0, 0}; int64_t totals[4] = {0, 0, 0, 0};
    if(e == hipSuccess) e = hipMemcpyAsync(hBad, dBad, 8, hipMemcpyDeviceToHost, st);
    for(int w = 0; w < 4 && e == hipSuccess; w++) e = hipMemcpyAsync(&totals[w], H->off(w) + (w == 3 ? nU : nR), 8, hipMemcpyDeviceToHost, st);
    if(e == hipSuccess) e = hipStreamSynchronize(st);
    if(e != hipSuccess) return failed("upload / k_fil_rank / k_fil_wide_rank / k_fil_host / the scans");
    if(hBad[0]) {
        H->err = std::string("BAM fill: ") + ((hBad[0] & FIL_BAD_MATE) ? (wide ? "a filled unit with more alignments on one mate than max_mate" : "a filled unit with more than 16 alignments on one mate") : (hBad[0] & FIL_BAD_PRIMARY) ? "a filled unit without a primary on a required mate"
                                                                       : "a unit whose records lie beyond the descriptors");
        return HLALA_E_ARG;
    }
    if(totals[1] < 0 || totals[1] > 0x7FFFFFFFll) { H->err = "BAM fill: more than 2^31 - 1 chains"; return HLALA_E_ARG; }
    const size_t nC = (size_t)totals[1];
    H->nChains = nC;
    if((e = fill_alloc(H, FIL_CHAINSRC, nC * 4)) != hipSuccess || (e = fill_alloc(H, FIL_CHAINCIG, nC * 8)) != hipSuccess) { (void)hipGetLastError(); *noMemory = true; return HLALA_OK; }
    e = hipMemsetAsync(H->buf[FIL_CHAINSRC].p, 0xFF, nC * 4, st);
    if(e == hipSuccess) e = hipMemsetAsync(H->buf[FIL_CHAINCIG].p, 0, nC * 8, st);
    if(e == hipSuccess) e = hipEventRecord(H->ev[5], st);
    if(e == hipSuccess) { hipLaunchKernelGGL(k_fil_src, dim3(rankBlocks), dim3(256), 0, st, H->S, (u64)nR, (const int64_t*)H->off(1), (const int64_t*)H->off(2), (u64)nC, (u32*)H->buf[FIL_CHAINSRC].p,
                                             (int64_t*)H->buf[FIL_CHAINCIG].p, (int32_t*)H->buf[FIL_PRIMARY].p); e = hipGetLastError(); }
    if(e == hipSuccess && nWide) {                       // (inside ms_src, and timed on its own)
        e = hipEventRecord(H->wev[2], st);
        if(e == hipSuccess) { hipLaunchKernelGGL(k_fil_wide_src, dim3((u32)((nSlots + 255) / 256)), dim3(256), 0, st, H->S, Wd, (u32)nWR, (u32)nSlots, (const int64_t*)H->off(1), (const int64_t*)H->off(2), (u64)nC,
                                                 (u32*)H->buf[FIL_CHAINSRC].p, (int64_t*)H->buf[FIL_CHAINCIG].p, (int32_t*)H->buf[FIL_PRIMARY].p); e = hipGetLastError(); }
        if(e == hipSuccess) e = hipEventRecord(H->wev[3], st);
    }
    if(e == hipSuccess) e = hipEventRecord(H->ev[6], st);
    if(e == hipSuccess) e = hipMemcpyAsync(read_off, H->off(0), (nR + 1) * 8, hipMemcpyDeviceToHost, st);
    if(e == hipSuccess) e = hipMemcpyAsync(chain_off, H->off(1), (nR + 1) * 8, hipMemcpyDeviceToHost, st);
    if(e == hipSuccess) e = hipMemcpyAsync(cigar_count, H->off(2), (nR + 1) * 8, hipMemcpyDeviceToHost, st);
    if(e == hipSuccess) e = hipMemcpyAsync(name_off, H->off(3), (nU + 1) * 8, hipMemcpyDeviceToHost, st);
    if(e == hipSuccess) e = hipEventRecord(H->ev[7], st);
    if(e == hipSuccess) e = hipStreamSynchronize(st);
    if(e != hipSuccess) return failed("k_fil_src / k_fil_wide_src / download");
    if(nWide) {
        float a = 0, b = 0;
        if(hipEventElapsedTime(&a, H->wev[0], H->wev[1]) != hipSuccess) a = 0;
        if(hipEventElapsedTime(&b, H->wev[2], H->wev[3]) != hipSuccess) b = 0;
        H->wideStats[0] = (int64_t)nWide; H->wideStats[1] = (int64_t)nWR; H->wideStats[2] = wide->longest; H->wideStats[3] = (int64_t)(((double)a + (double)b) * 1e3 + 0.5);
        stats->bytes_h2d += (int64_t)(wideWords.size() * 4);
    }
    stats->n_units = (int64_t)nU; stats->n_host_units = (int64_t)nHost; stats->n_reads = (int64_t)nR; stats->n_chains = totals[1]; stats->n_cigar = totals[2]; stats->n_bases = totals[0]; stats->n_name_bytes = totals[3];
    stats->ms_h2d += ms(0, 1); stats->ms_rank = ms(1, 2); stats->ms_host = ms(2, 3); stats->ms_scan = ms(3, 4); stats->ms_src = ms(5, 6); stats->ms_d2h = ms(6, 7);
    stats->bytes_h2d += (int64_t)(nU * 8 + nHost * (perHost * 8 + 4)); stats->bytes_d2h += (int64_t)((3 * (nR + 1) + nU + 1) * 8);
    return HLALA_OK;
}
static hlala_bam_fill* fill_new(int device, std::string* why)
{
    hlala_bam_fill* H = new hlala_bam_fill(); H->device = device;
    DevGuard g(device);
    hipError_t e = hipStreamCreateWithFlags(&H->st, hipStreamNonBlocking);
    for(hipEvent_t& ev : H->ev) if(e == hipSuccess) e = hipEventCreate(&ev);
    if(e == hipSuccess) e = hipHostMalloc((void**)&H->hBounds, 8 * 8, hipHostMallocDefault);
    if(e != hipSuccess) { if(why) *why = std::string("BAM fill: stream / events / staging: ") + hipGetErrorString(e); (void)hipGetLastError(); fill_free(H); return nullptr; }
    return H;
}
// The slices of a window from the staging block to where they belong.  The destination's pages are often first touched here (the arrays of a seed batch are not
// cleared), which one thread does at a fraction of the rate the copy engine delivers: beyond a few MiB the pieces are cut across the CPUs this process may keep busy.
struct FillPiece { void* to; const void* from; size_t bytes; };
static void fill_scatter(const std::vector<FillPiece>& slices)
{
    constexpr size_t CUT = (size_t)2 << 20;
    std::vector<FillPiece> pieces; size_t total = 0;
    for(const FillPiece& s : slices) { total += s.bytes; for(size_t o = 0; o < s.bytes; o += CUT) pieces.push_back(FillPiece{(uint8_t*)s.to + o, (const uint8_t*)s.from + o, std::min(CUT, s.bytes - o)}); }
    int T = std::min(16, hlala_host::host_cpu_budget()); if((size_t)T > pieces.size()) T = (int)pieces.size();
    if(total < 4 * CUT || T <= 1) { for(const FillPiece& q : pieces) memcpy(q.to, q.from, q.bytes); return; }
    std::atomic<size_t> next(0);
    auto work = [&]() { for(;;) { const size_t i = next.fetch_add(1); if(i >= pieces.size()) break; memcpy(pieces[i].to, pieces[i].from, pieces[i].bytes); } };
    std::vector<std::thread> th;
    try { for(int t = 1; t < T; t++) th.emplace_back(work); } catch(...) {}       // (a thread that cannot be started: the others and this one do its share)
    work();
    for(std::thread& x : th) x.join();
}
static int fill_window(hlala_bam_fill* H, int64_t first_unit, int64_t n_units, const hlala_bam_fill_out* out, hlala_bam_fill_stats* stats)
{
    using namespace hlala_bamfill;
    H->err.clear();
    if(!stats) { H->err = "hlala_bam_fill_window: null argument"; return HLALA_E_ARG; }
    memset(stats, 0, sizeof(*stats));
    if(first_unit < 0 || n_units < 0 || first_unit + n_units > (int64_t)H->S.nUnits) { H->err = "hlala_bam_fill_window: units outside the sample"; return HLALA_E_ARG; }
    if(n_units == 0) return HLALA_OK;
    const bool need = out && out->read_primary && out->read_quals && (H->packed ? out->read_bases_packed : out->read_bases) && out->chain_contig && out->chain_pos && out->chain_offset && out->chain_as &&
                      out->chain_reverse && out->cigar_off_end && out->cigar && out->name_chars;
    if(!need) { H->err = "hlala_bam_fill_window: null argument"; return HLALA_E_ARG; }
    const auto tWall = std::chrono::steady_clock::now();
    DevGuard g(H->device);
    hipStream_t st = H->st;
    hipError_t e = hipSuccess;
    auto failed = [&](const char* what) { H->err = std::string("hlala_bam_fill_window: ") + what + ": " + hipGetErrorString(e); (void)hipStreamSynchronize(st); (void)hipGetLastError(); return HLALA_E_DEVICE; };
    const u64 nm = H->S.nm, u0 = (u64)first_unit, u1 = u0 + (u64)n_units, r0 = u0 * nm, r1 = u1 * nm;
    // the window's bounds in the four offset arrays
    const u64 at[8] = {r0, r1, r0, r1, r0, r1, u0, u1};
    for(int k = 0; k < 8 && e == hipSuccess; k++) e = hipMemcpyAsync(H->hBounds + k, H->off(k / 2) + at[k], 8, hipMemcpyDeviceToHost, st);
    if(e == hipSuccess) e = hipStreamSynchronize(st);
    if(e != hipSuccess) return failed("the window's bounds");
    const int64_t* hb = H->hBounds;
    for(int k = 0; k < 4; k++) if(hb[2 * k] < 0 || hb[2 * k + 1] < hb[2 * k]) { H->err = "hlala_bam_fill_window: offsets that do not ascend"; return HLALA_E_DEVICE; }      // (cannot happen)
    FilWindow W{};
    W.r0 = r0; W.nr = r1 - r0; W.b0 = (u64)hb[0]; W.nb = (u64)(hb[1] - hb[0]); W.c0 = (u64)hb[2]; W.nc = (u64)(hb[3] - hb[2]); W.g0 = (u64)hb[4]; W.ng = (u64)(hb[5] - hb[4]);
    W.u0 = u0; W.nu = u1 - u0; W.n0 = (u64)hb[6]; W.nn = (u64)(hb[7] - hb[6]);
    W.p0 = (u64)fil_packed_at(hb[0], (int64_t)r0); W.np = H->packed ? (u64)fil_packed_at(hb[1], (int64_t)r1) - W.p0 : 0;
    if(W.c0 + W.nc > H->nChains) { H->err = "hlala_bam_fill_window: chains beyond the sample"; return HLALA_E_DEVICE; }      // (cannot happen)
    // one block for the window's slices, every slice on a 16-byte boundary
    size_t total = 0;
    auto place = [&](size_t bytes) { const size_t o = total; total += (bytes + 15) & ~(size_t)15; return o; };
    const size_t oContig = place(W.nc * 4), oPos = place(W.nc * 4), oOffset = place(W.nc * 4), oAs = place(W.nc * 4), oRev = place(W.nc), oCigEnd = place(W.nc * 8), oCigar = place(W.ng * 4), oNames = place(W.nn),
                 oBases = place(H->packed ? W.np : W.nb), oQuals = place(W.nb), oPrim = place(W.nr * 4);
    if((e = fill_alloc(H, FIL_WIN, total)) != hipSuccess) return failed("hipMalloc");
    if(total > H->stageCap) {
        if(H->hStage) { (void)hipHostFree(H->hStage); H->hStage = nullptr; H->stageCap = 0; }
        if((e = hipHostMalloc((void**)&H->hStage, total + total / 4, hipHostMallocDefault)) != hipSuccess) { H->hStage = nullptr; return failed("hipHostMalloc"); }
        H->stageCap = total + total / 4;
    }
    uint8_t* d = (uint8_t*)H->buf[FIL_WIN].p;
    W.chainContig = (int32_t*)(d + oContig); W.chainPos = (int32_t*)(d + oPos); W.chainOffset = (int32_t*)(d + oOffset); W.chainAs = (int32_t*)(d + oAs); W.chainReverse = d + oRev;
    W.cigarOffEnd = (int64_t*)(d + oCigEnd); W.cigar = (u32*)(d + oCigar); W.names = d + oNames; W.bases = H->packed ? nullptr : d + oBases; W.packed = H->packed ? d + oBases : nullptr; W.quals = d + oQuals;
    const u32* dSrc = (const u32*)H->buf[FIL_CHAINSRC].p; const int64_t* dCig = (const int64_t*)H->buf[FIL_CHAINCIG].p; const int32_t* dPrim = (const int32_t*)H->buf[FIL_PRIMARY].p;
    auto ms = [&](int a, int b) { float t = 0; return hipEventElapsedTime(&t, H->ev[a], H->ev[b]) == hipSuccess ? (double)t : 0.0; };
    e = hipMemsetAsync(d, 0, total, st);
    if(e == hipSuccess) e = hipMemcpyAsync(d + oPrim, dPrim + r0, W.nr * 4, hipMemcpyDeviceToDevice, st);
    if(e == hipSuccess) e = hipEventRecord(H->ev[0], st);
    if(e == hipSuccess && W.nc) { hipLaunchKernelGGL(k_fil_chain, dim3((u32)((W.nc + 255) / 256)), dim3(256), 0, st, H->S, W, dSrc, dCig); e = hipGetLastError(); }
    if(e == hipSuccess) e = hipEventRecord(H->ev[1], st);
    if(e == hipSuccess && W.nc) { hipLaunchKernelGGL(k_fil_cigar, dim3((u32)((W.nc * 16 + 255) / 256)), dim3(256), 0, st, H->S, W, dSrc, dCig); e = hipGetLastError(); }
    if(e == hipSuccess) e = hipEventRecord(H->ev[2], st);
    if(e == hipSuccess) { hipLaunchKernelGGL(k_fil_names, dim3((u32)((W.nu * 16 + 255) / 256)), dim3(256), 0, st, H->S, W, (const int64_t*)H->off(3)); e = hipGetLastError(); }
    if(e == hipSuccess) e = hipEventRecord(H->ev[3], st);
    if(e == hipSuccess) { hipLaunchKernelGGL(k_fil_bases, dim3((u32)((W.nr + 3) / 4)), dim3(256), 0, st, H->S, W, (const int64_t*)H->off(0), dPrim, dSrc, (u64)H->nChains); e = hipGetLastError(); }
    if(e == hipSuccess) e = hipEventRecord(H->ev[4], st);
    if(e == hipSuccess) e = hipMemcpyAsync(H->hStage, d, total, hipMemcpyDeviceToHost, st);
    if(e == hipSuccess) e = hipEventRecord(H->ev[5], st);
    if(e == hipSuccess) e = hipStreamSynchronize(st);
    if(e != hipSuccess) return failed("k_fil_chain / k_fil_cigar / k_fil_names / k_fil_bases / download");
    const uint8_t* h = H->hStage;
    fill_scatter({{out->chain_contig, h + oContig, W.nc * 4}, {out->chain_pos, h + oPos, W.nc * 4}, {out->chain_offset, h + oOffset, W.nc * 4}, {out->chain_as, h + oAs, W.nc * 4}, {out->chain_reverse, h + oRev, W.nc},
                  {out->cigar_off_end, h + oCigEnd, W.nc * 8}, {out->cigar, h + oCigar, W.ng * 4}, {out->name_chars, h + oNames, W.nn},
                  {H->packed ? out->read_bases_packed : out->read_bases, h + oBases, H->packed ? W.np : W.nb}, {out->read_quals, h + oQuals, W.nb}, {out->read_primary, h + oPrim, W.nr * 4}});
    stats->n_units = n_units; stats->n_reads = (int64_t)W.nr; stats->n_chains = (int64_t)W.nc; stats->n_cigar = (int64_t)W.ng; stats->n_bases = (int64_t)W.nb; stats->n_name_bytes = (int64_t)W.nn;
    stats->ms_chain = ms(0, 1); stats->ms_cigar = ms(1, 2); stats->ms_names = ms(2, 3); stats->ms_bases = ms(3, 4); stats->ms_d2h = ms(4, 5); stats->bytes_d2h = (int64_t)total + 64;
    stats->ms_wall = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tWall).count();
    return HLALA_OK;
}
// max_mate 0: hlala_bam_fill_create; otherwise hlala_bam_fill_create_wide, which looks for the wide units in the descriptors it has just checked
static int fill_create(const char* fn, hlala_inflater* f, const hlala_bam_fill_in* in, int32_t max_mate, bool isWide, int64_t* read_off, int64_t* chain_off, int64_t* cigar_count, int64_t* name_off,
                       hlala_bam_fill** out, hlala_bam_fill_stats* stats)
{
    if(!f) { int ndev = 0; if(hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) { (void)hipGetLastError(); return HLALA_E_DEVICE; } return HLALA_E_ARG; }
    f->err.clear();
    if(out) *out = nullptr;
    const char* bad = !out ? "null argument" : isWide ? hlala_bamfill::fil_check_args_wide(in, max_mate, read_off, chain_off, cigar_count, name_off, stats)
                                                      : hlala_bamfill::fil_check_args(in, read_off, chain_off, cigar_count, name_off, stats);
    if(bad) { f->err = std::string(fn) + ": " + bad; return HLALA_E_ARG; }
    std::vector<u32> wideUnits; FillWideIn wide{max_mate, nullptr, 0, 0};
    if(isWide) {
        for(int64_t u = 0; u < in->n_units; u++) {
            if(in->unit_first[u] == hlala_bamfill::FIL_HOST) continue;
            u32 m[2] = {0, 0};
            for(u32 k = 0; k < in->unit_count[u]; k++) m[in->recs[in->unit_first[u] + k].which & 1]++;
            if(hlala_bamfill::fil_is_wide(in->unit_count[u], m[0], m[1])) { wideUnits.push_back((u32)u); wide.longest = std::max<int64_t>(wide.longest, std::max(m[0], m[1])); }
        }
        wide.units = wideUnits.data(); wide.n = wideUnits.size();
    }
    const auto tWall = std::chrono::steady_clock::now();
    memset(stats, 0, sizeof(*stats));
    if(in->n_units == 0) return HLALA_OK;
    hlala_bam_fill* H = fill_new(f->device, &f->err);
    if(!H) return HLALA_E_DEVICE;
    DevGuard g(f->device);
    hipError_t e = hipSuccess;
    auto failed = [&](const char* what) { f->err = std::string(fn) + ": " + what + ": " + hipGetErrorString(e); (void)hipGetLastError(); fill_free(H); return HLALA_E_DEVICE; };
    const size_t recBytes = (size_t)in->n * sizeof(hlala_bam_rec);
    if((e = fill_alloc(H, FIL_RECS, recBytes)) != hipSuccess || (e = fill_alloc(H, FIL_BYTES, in->n_bytes)) != hipSuccess) return failed("hipMalloc");
    e = hipEventRecord(H->ev[0], H->st);
    if(e == hipSuccess && recBytes) e = hipMemcpyAsync(H->buf[FIL_RECS].p, in->recs, recBytes, hipMemcpyHostToDevice, H->st);
    if(e == hipSuccess && in->n_bytes) e = hipMemcpyAsync(H->buf[FIL_BYTES].p, in->bytes, in->n_bytes, hipMemcpyHostToDevice, H->st);
    if(e == hipSuccess) e = hipEventRecord(H->ev[1], H->st);
    if(e == hipSuccess) e = hipStreamSynchronize(H->st);
    if(e != hipSuccess) return failed("upload");
    { float t = 0; if(hipEventElapsedTime(&t, H->ev[0], H->ev[1]) == hipSuccess) stats->ms_h2d = (double)t; }
    stats->bytes_h2d = (int64_t)(recBytes + in->n_bytes);
    H->S.recs = (const hlala_bam_rec*)H->buf[FIL_RECS].p; H->S.n = (u32)in->n; H->S.bytes = (const uint8_t*)H->buf[FIL_BYTES].p; H->S.nBytes = (u64)in->n_bytes; H->S.perm = nullptr;
    bool noMemory = false;
    const int rc = fill_layout(H, in, read_off, chain_off, cigar_count, name_off, stats, &noMemory, isWide ? &wide : nullptr);
    if(rc != HLALA_OK || noMemory) { f->err = noMemory ? std::string(fn) + ": no device memory for the passes" : H->err; fill_free(H); return noMemory ? HLALA_E_DEVICE : rc; }
    stats->ms_wall = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tWall).count();
    *out = H;
    return HLALA_OK;
}
extern "C" int hlala_bam_fill_create(hlala_inflater* f, const hlala_bam_fill_in* in, int64_t* read_off, int64_t* chain_off, int64_t* cigar_count, int64_t* name_off, hlala_bam_fill** out,
                                     hlala_bam_fill_stats* stats)
{
    return fill_create("hlala_bam_fill_create", f, in, 0, false, read_off, chain_off, cigar_count, name_off, out, stats);
}
extern "C" int hlala_bam_fill_create_wide(hlala_inflater* f, const hlala_bam_fill_in* in, int32_t max_mate, int64_t* read_off, int64_t* chain_off, int64_t* cigar_count, int64_t* name_off,
                                          hlala_bam_fill** out, hlala_bam_fill_stats* stats)
{
    return fill_create("hlala_bam_fill_create_wide", f, in, max_mate, true, read_off, chain_off, cigar_count, name_off, out, stats);
}
extern "C" int hlala_bam_fill_wide_stats(const hlala_bam_fill* h, int64_t out[4])
{
    if(!h || !out) return HLALA_E_ARG;
    for(int k = 0; k < 4; k++) out[k] = h->wideStats[k];
    return HLALA_OK;
}
extern "C" int hlala_bam_fill_window(hlala_bam_fill* h, int64_t first_unit, int64_t n_units, const hlala_bam_fill_out* out, hlala_bam_fill_stats* stats)
{
    if(!h) return HLALA_E_ARG;
    return fill_window(h, first_unit, n_units, out, stats);
}
extern "C" const char* hlala_bam_fill_last_error(const hlala_bam_fill* h) { return h ? h->err.c_str() : ""; }
extern "C" void hlala_bam_fill_destroy(hlala_bam_fill* h) { fill_free(h); }

// The decoder with HLALA_SEEDS_GPU_FILL.  The scan hook keeps a round's descriptors (rec_off moved by where its compact bytes go) and compact bytes in sample-long
// device buffers of the inflater; the fill hook moves those buffers into a fill state, copies the grouping permutation beside them and runs the layout passes.  From
// then on the state stands alone.  An allocation that fails is no error: keep.ok = false, or *available = false, and the host fills the sample itself.
static void keep_reset(hlala_inflater* f) { f->keep.n = 0; f->keep.nBytes = 0; f->keep.ok = true; }
static void keep_drop(hlala_inflater* f)
{
    for(ScanBuf* b : {&f->keep.recs, &f->keep.bytes}) { if(b->p) (void)hipFree(b->p); b->p = nullptr; b->cap = 0; }
    f->keep.n = 0; f->keep.nBytes = 0; f->keep.ok = false;
}
static hipError_t keep_grow(ScanBuf& b, size_t bytes, size_t keep, hipStream_t st)
{
    if(bytes <= b.cap) return hipSuccess;
    const size_t want = 2 * bytes + 256;
    void* p = nullptr;
    hipError_t r = hipMalloc(&p, want);
    if(r != hipSuccess) return r;
    if(keep && b.p) { r = hipMemcpyAsync(p, b.p, keep, hipMemcpyDeviceToDevice, st); if(r == hipSuccess) r = hipStreamSynchronize(st); if(r != hipSuccess) { (void)hipFree(p); return r; } }
    if(b.p) (void)hipFree(b.p);
    b.p = p; b.cap = want;
    return hipSuccess;
}
static int keep_append(hlala_inflater* f, const hlala_bam_rec* dRecs, int64_t n, const uint8_t* dBytes, size_t nBytes)
{
    FillKeep& K = f->keep;
    if(K.n + n >= ((int64_t)1 << 31)) { keep_drop(f); return HLALA_OK; }
    DevGuard g(f->device);
    hipStream_t st = f->slot[0].stream;
    hipError_t e = hipSuccess;
    const size_t have = (size_t)K.n, total = have + (size_t)n;
    if((e = keep_grow(K.recs, total * sizeof(hlala_bam_rec), have * sizeof(hlala_bam_rec), st)) != hipSuccess || (e = keep_grow(K.bytes, (size_t)K.nBytes + nBytes + 1, (size_t)K.nBytes, st)) != hipSuccess) {
        (void)hipGetLastError(); keep_drop(f); return HLALA_OK;
    }
    hipLaunchKernelGGL(k_fil_append, dim3((u32)((n + 255) / 256)), dim3(256), 0, st, (u32)n, dRecs, (u64)K.nBytes, (hlala_bam_rec*)K.recs.p + have);
    e = hipGetLastError();
    if(e == hipSuccess && nBytes) e = hipMemcpyAsync((uint8_t*)K.bytes.p + K.nBytes, dBytes, nBytes, hipMemcpyDeviceToDevice, st);
    if(e == hipSuccess) e = hipStreamSynchronize(st);
    if(e != hipSuccess) { f->err = std::string("BAM fill: k_fil_append: ") + hipGetErrorString(e); (void)hipGetLastError(); return HLALA_E_DEVICE; }
    K.n = (int64_t)total; K.nBytes += nBytes;
    return HLALA_OK;
}
static int fill_state_window(void* state, int64_t first_unit, int64_t n_units, const hlala_bam_fill_out* out, hlala_bam_fill_stats* stats, std::string* err)
{
    hlala_bam_fill* H = (hlala_bam_fill*)state;
    const int rc = fill_window(H, first_unit, n_units, out, stats);
    if(rc != HLALA_OK && err) *err = H->err;
    return rc;
}
static void fill_state_destroy(void* state) { fill_free((hlala_bam_fill*)state); }
// a window of the decoder's fill state as a batch of ctx (hlala_seed_batch_create_resident): hlala_batch_create_from_fill; a context on another device is no error of
// the sample -- the caller takes the host route for it
static int fill_state_resident(void* state, hlala_ctx* c, int64_t first_unit, int64_t n_units, const hlala_batch_fill_src* src, hlala_batch** out, hlala_batch_fill_stats* stats, std::string* err)
{
    hlala_bam_fill* H = (hlala_bam_fill*)state;
    if(!H || !c) { if(err) *err = "hlala_seed_batch_create_resident: null argument"; return HLALA_E_ARG; }
    if(c->device != H->device) {
        c->err = "not available: the context is on device " + std::to_string(c->device) + ", the sample's fill state on device " + std::to_string(H->device);
        if(err) *err = c->err;
        return HLALA_E_STATE;
    }
    const int rc = hlala_batch_create_from_fill(c, H, first_unit, n_units, src, out, stats);
    if(rc != HLALA_OK && err) *err = c->err;
    return rc;
}
static int fill_hook_any(void* inflater, const hlala_bam_fill_in* in, const FillWideIn* wide, int64_t* read_off, int64_t* chain_off, int64_t* cigar_count, int64_t* name_off,
                         hlala_host::bam_fill_handle* handle, hlala_bam_fill_stats* stats, bool* available, std::string* err)
{
    hlala_inflater* f = (hlala_inflater*)inflater;
    if(!f || !in || !handle || !stats || !available) return HLALA_E_ARG;
    f->err.clear();
    memset(stats, 0, sizeof(*stats));
    GroupState& G = f->grp; FillKeep& K = f->keep;
    *available = K.ok && G.ok && G.finished && K.n == G.n && in->n == K.n && in->n_units > 0 && in->n_units < ((int64_t)1 << 30);
    if(!*available) return HLALA_OK;
    const auto tWall = std::chrono::steady_clock::now();
    auto fail = [&](int rc) { if(err) *err = f->err; return rc; };
    hlala_bam_fill* H = fill_new(f->device, &f->err);
    if(!H) { (void)hipGetLastError(); *available = false; return HLALA_OK; }
    DevGuard g(f->device);
    // the kept buffers change hands; the permutation is copied (the grouping state keeps its own)
    H->buf[FIL_RECS] = K.recs; H->buf[FIL_BYTES] = K.bytes; K.recs = ScanBuf(); K.bytes = ScanBuf();
    H->S.recs = (const hlala_bam_rec*)H->buf[FIL_RECS].p; H->S.n = (u32)K.n; H->S.bytes = (const uint8_t*)H->buf[FIL_BYTES].p; H->S.nBytes = (u64)K.nBytes;
    K.n = 0; K.nBytes = 0; K.ok = false;
    hipError_t e = fill_alloc(H, FIL_PERM, (size_t)H->S.n * 4);
    if(e != hipSuccess) { (void)hipGetLastError(); fill_free(H); *available = false; return HLALA_OK; }
    e = hipStreamSynchronize(f->slot[0].stream);
    if(e == hipSuccess) e = hipMemcpyAsync(H->buf[FIL_PERM].p, G.buf[GRP_VAL_OUT].p, (size_t)H->S.n * 4, hipMemcpyDeviceToDevice, H->st);
    if(e == hipSuccess) e = hipStreamSynchronize(H->st);
    if(e != hipSuccess) { f->err = std::string("BAM fill: the permutation: ") + hipGetErrorString(e); (void)hipGetLastError(); fill_free(H); return fail(HLALA_E_DEVICE); }
    H->S.perm = (const u32*)H->buf[FIL_PERM].p;
    bool noMemory = false;
    const int rc = fill_layout(H, in, read_off, chain_off, cigar_count, name_off, stats, &noMemory, wide);
    if(rc != HLALA_OK) { f->err = H->err; fill_free(H); return fail(rc); }
    if(noMemory) { fill_free(H); *available = false; return HLALA_OK; }
    stats->ms_wall = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tWall).count();
    handle->state = H; handle->window = fill_state_window; handle->destroy = fill_state_destroy; handle->resident = fill_state_resident;
    return HLALA_OK;
}
static int bam_fill_hook(void* inflater, const hlala_bam_fill_in* in, int64_t* read_off, int64_t* chain_off, int64_t* cigar_count, int64_t* name_off, hlala_host::bam_fill_handle* handle,
                         hlala_bam_fill_stats* stats, bool* available, std::string* err)
{
    return fill_hook_any(inflater, in, nullptr, read_off, chain_off, cigar_count, name_off, handle, stats, available, err);
}
static int bam_fill_wide_hook(void* inflater, const hlala_bam_fill_in* in, int32_t max_mate, const uint32_t* wide_units, int64_t n_wide, int64_t longest, int64_t* read_off, int64_t* chain_off,
                              int64_t* cigar_count, int64_t* name_off, hlala_host::bam_fill_handle* handle, hlala_bam_fill_stats* stats, bool* available, std::string* err)
{
    if(max_mate <= (int32_t)hlala_bamfill::FIL_MAX_MATE || max_mate > (int32_t)hlala_bamfill::FIL_WIDE_MAX || n_wide < 0 || (n_wide && !wide_units)) return HLALA_E_ARG;
    const FillWideIn wide{max_mate, wide_units, (size_t)n_wide, longest};
    return fill_hook_any(inflater, in, &wide, read_off, chain_off, cigar_count, name_off, handle, stats, available, err);
}

// ---- a batch from a window of a fill state, built on the device (include/hlala_gpu.h; kernel_bamresident.hip).  Everything runs on the context's upload stream: the
// fill state's own stream is idle between its calls (each ends synchronised) and its buffers do not change after hlala_bam_fill_create.
extern "C" int hlala_batch_create_from_fill(hlala_ctx* c, hlala_bam_fill* H, int64_t first_unit, int64_t n_units, const hlala_batch_fill_src* src, hlala_batch** out, hlala_batch_fill_stats* stats)
{
    using namespace hlala_bamfill;
    using namespace hlala_bamres;
    static_assert(RES_SEQCAP == DP_SEQCAP, "bam_resident_core.h states the cap of the paired path");
    static_assert(sizeof(ResPiece) == 32, "a piece is four 64-bit words");
    DEV_GUARD(c);
    if(!c) return HLALA_E_ARG;
    if(out) *out = nullptr;
    if(!H || !src || !out || !stats || !src->read_off || !src->chain_off || !src->cigar_count) { c->err = "hlala_batch_create_from_fill: null argument"; return HLALA_E_ARG; }
    memset(stats, 0, sizeof(*stats));
    if(c->device != H->device) { c->err = "hlala_batch_create_from_fill: the context is on device " + std::to_string(c->device) + ", the fill state on device " + std::to_string(H->device); return HLALA_E_ARG; }
    if(first_unit < 0 || n_units < 0 || first_unit + n_units > (int64_t)H->S.nUnits) { c->err = "hlala_batch_create_from_fill: units outside the sample"; return HLALA_E_ARG; }
    if(!c->d_contig_off) { c->err = "hlala_batch_create needs contigs (hlala_create was called without them)"; return HLALA_E_STATE; }
    const auto tWall = std::chrono::steady_clock::now();
    UploadScope upscope_(c);
    const u64 nm = H->S.nm, u0 = (u64)first_unit, u1 = u0 + (u64)n_units, r0 = u0 * nm, r1 = u1 * nm;
    const bool unpaired = nm == 1;
    const int64_t nr64 = (int64_t)(r1 - r0);
    if(nr64 > 0x7FFFFFFFll) { c->err = "batch of " + std::to_string(nr64) + " reads: one batch holds at most 2^31 - 1"; return HLALA_E_CAPACITY; }
    const int64_t* ro = src->read_off; const int64_t* co = src->chain_off; const int64_t* gc = src->cigar_count;
    const int64_t rb0 = nr64 ? ro[r0] : 0, rb1 = nr64 ? ro[r1] : 0, cb0 = nr64 ? co[r0] : 0, cb1 = nr64 ? co[r1] : 0, nc64 = cb1 - cb0;
    if(nc64 > 0x7FFFFFFFll) { c->err = "batch of " + std::to_string(nc64) + " chains: one batch holds at most 2^31 - 1"; return HLALA_E_CAPACITY; }
    int rc = res_bounds_reads(n_units, nr64, nc64, rb0, rb1, cb0, cb1, &c->err);
    if(rc) return rc;
    const int64_t gb0 = nc64 > 0 ? gc[r0] : 0, gb1 = nc64 > 0 ? gc[r1] : 0;
    rc = res_bounds_cigar(nc64, gb0, gb1, &c->err);
    if(rc) return rc;
    const int nr = (int)nr64, nc = (int)nc64;
    const size_t nbases = (size_t)(rb1 - rb0), ncig = (size_t)(gb1 - gb0);
    // ---- the window's host units and the slices their ranges come from
    const auto hFirst = std::lower_bound(H->hostUnit.begin(), H->hostUnit.end(), (u32)u0), hEnd = std::lower_bound(H->hostUnit.begin(), H->hostUnit.end(), (u32)u1);
    const size_t nHostW = (size_t)(hEnd - hFirst);
    const hlala_bam_fill_out* hs = src->host;
    if(nHostW) {
        if(!hs) { c->err = "hlala_batch_create_from_fill: the window holds host units and src->host is NULL"; return HLALA_E_ARG; }
        if(!hs->read_primary || !hs->read_quals || !(H->packed ? hs->read_bases_packed : hs->read_bases) || !hs->chain_contig || !hs->chain_pos || !hs->chain_offset || !hs->chain_as ||
           !hs->chain_reverse || !hs->cigar_off_end || !hs->cigar) { c->err = "hlala_batch_create_from_fill: null argument"; return HLALA_E_ARG; }
    }
    hlala_batch* b = new hlala_batch(); b->ctx = c; c->batches.insert(b);
    DevBatch& B = b->B;
    B.n_pairs = (int)n_units; B.n_reads = nr; B.n_chains = nc; B.stride = c->params.max_columns; B.from_seeds = 0; B.unpaired = unpaired ? 1 : 0;
    b->first_chain = (uint32_t)cb0;
    std::vector<void*> tmp;       // device blocks this call alone needs: back to the pool once the stream has passed them
    auto fail = [&](int code) { (void)hipStreamSynchronize(c->active); for(void* p : tmp) pool_release(c, p); hlala_batch_destroy(b); return code; };
    // ---- the batch's own arrays (cleared: a range no pass writes reads as zeros) and what only this call needs
    ResArrays A{};
    int *dReadOff = nullptr, *dChainOff = nullptr, *dPrimary = nullptr, *dChainRead = nullptr, *dContig = nullptr, *dPos = nullptr, *dOffset = nullptr, *dAs = nullptr, *dCigarOff = nullptr;
    uint8_t *dBases = nullptr, *dQuals = nullptr, *dReverse = nullptr; u32* dCigar = nullptr; int64_t* dCigEnd = nullptr; u64* dSlots = nullptr;
#define ALB(ptr, n, list) do { rc = dev_alloc(c, list, (n), &ptr, true); if(rc) return fail(rc); } while(0)
    ALB(dReadOff, (size_t)nr + 1, b->allocs); ALB(dQuals, nbases, b->allocs); ALB(dBases, nbases, b->allocs); ALB(dChainOff, (size_t)nr + 1, b->allocs); ALB(dPrimary, (size_t)nr, b->allocs);
    ALB(dChainRead, (size_t)nc, b->allocs); ALB(dContig, (size_t)nc, b->allocs); ALB(dPos, (size_t)nc, b->allocs); ALB(dOffset, (size_t)nc, b->allocs); ALB(dAs, (size_t)nc, b->allocs);
    ALB(dReverse, (size_t)nc, b->allocs); ALB(dCigarOff, (size_t)nc + 1, b->allocs); ALB(dCigar, ncig, b->allocs);
    ALB(dCigEnd, (size_t)nc, tmp); ALB(dSlots, (size_t)RES_CLASSES, tmp);
#undef ALB
    B.read_off = dReadOff; B.read_quals = dQuals; B.read_bases = dBases; B.chain_off = dChainOff; B.read_primary = dPrimary; B.chain_read = dChainRead; B.chain_contig = dContig; B.chain_pos = dPos;
    B.chain_offset = dOffset; B.chain_as = dAs; B.chain_reverse = dReverse; B.cigar_off = dCigarOff; B.cigar = dCigar;
    A.p[RES_A_PRIMARY] = (uint8_t*)dPrimary; A.bytes[RES_A_PRIMARY] = (u64)nr * 4; A.p[RES_A_BASES] = dBases; A.bytes[RES_A_BASES] = nbases; A.p[RES_A_QUALS] = dQuals; A.bytes[RES_A_QUALS] = nbases;
    A.p[RES_A_CONTIG] = (uint8_t*)dContig; A.p[RES_A_POS] = (uint8_t*)dPos; A.p[RES_A_OFFSET] = (uint8_t*)dOffset; A.p[RES_A_AS] = (uint8_t*)dAs;
    for(int a : {RES_A_CONTIG, RES_A_POS, RES_A_OFFSET, RES_A_AS}) A.bytes[a] = (u64)nc * 4;
    A.p[RES_A_REVERSE] = dReverse; A.bytes[RES_A_REVERSE] = (u64)nc; A.p[RES_A_CIGEND] = (uint8_t*)dCigEnd; A.bytes[RES_A_CIGEND] = (u64)nc * 8; A.p[RES_A_CIGAR] = (uint8_t*)dCigar; A.bytes[RES_A_CIGAR] = (u64)ncig * 4;
    // ---- the staging block of the host units: the piece table, then the bytes of every piece.  Two passes over the same list: sizes, then (into the context's
    // page-locked scratch) the copies.  A piece that leaves its array -- offsets that are not the sample's -- is refused.
    const int64_t p0 = fil_packed_at(rb0, (int64_t)r0);
    size_t nPieces = 0, dataBytes = 0; bool outside = false;
    ResPiece* pieces = nullptr; uint8_t* stage = nullptr; size_t tableBytes = 0;
    auto add = [&](int arr, int kind, int64_t dst, int64_t bytes, const void* from, int64_t fromBytes) {
        if(bytes <= 0) return;
        if(dst < 0 || (u64)dst + (u64)bytes > A.bytes[arr] || fromBytes < 0) { outside = true; return; }
        if(pieces) { pieces[nPieces] = ResPiece{(u32)arr, (u32)kind, (u64)dst, (u64)(tableBytes + dataBytes), (u64)bytes}; memcpy(stage + tableBytes + dataBytes, from, (size_t)fromBytes); }
        nPieces++; dataBytes += ((size_t)fromBytes + 3) & ~(size_t)3;       // (every piece starts on a word of the block: k_res_patch moves words where it can)
    };
    auto walk = [&]() {
        nPieces = 0; dataBytes = 0;
        for(auto it = hFirst; it != hEnd; ++it) {
            const u64 ra = (u64)*it * nm, rb = ra + nm;
            const int64_t b_ = ro[ra] - rb0, bn = ro[rb] - ro[ra], c_ = co[ra] - cb0, cn = co[rb] - co[ra], g_ = gc[ra] - gb0, gn = gc[rb] - gc[ra];
            if(b_ < 0 || bn < 0 || c_ < 0 || cn < 0 || g_ < 0 || gn < 0) { outside = true; return; }
            add(RES_A_PRIMARY, RES_PIECE_BYTES, (int64_t)(ra - r0) * 4, (int64_t)nm * 4, hs->read_primary + (ra - r0), (int64_t)nm * 4);
            add(RES_A_QUALS, RES_PIECE_BYTES, b_, bn, hs->read_quals + b_, bn);
            if(!H->packed) add(RES_A_BASES, RES_PIECE_BYTES, b_, bn, hs->read_bases + b_, bn);
            else for(u64 r = ra; r < rb; r++) {
                const int64_t ls = ro[r + 1] - ro[r];
                if(ls < 0) { outside = true; return; }
                add(RES_A_BASES, RES_PIECE_PACKED, ro[r] - rb0, ls, hs->read_bases_packed + (fil_packed_at(ro[r], (int64_t)r) - p0), (ls + 1) / 2);
            }
            add(RES_A_CONTIG, RES_PIECE_BYTES, c_ * 4, cn * 4, hs->chain_contig + c_, cn * 4); add(RES_A_POS, RES_PIECE_BYTES, c_ * 4, cn * 4, hs->chain_pos + c_, cn * 4);
            add(RES_A_OFFSET, RES_PIECE_BYTES, c_ * 4, cn * 4, hs->chain_offset + c_, cn * 4); add(RES_A_AS, RES_PIECE_BYTES, c_ * 4, cn * 4, hs->chain_as + c_, cn * 4);
            add(RES_A_REVERSE, RES_PIECE_BYTES, c_, cn, hs->chain_reverse + c_, cn); add(RES_A_CIGEND, RES_PIECE_BYTES, c_ * 8, cn * 8, hs->cigar_off_end + c_, cn * 8);
            add(RES_A_CIGAR, RES_PIECE_BYTES, g_ * 4, gn * 4, hs->cigar + g_, gn * 4);
        }
    };
    uint8_t* dStage = nullptr; size_t stageBytes = 0;
    if(nHostW) {
        walk();
        if(outside) { c->err = "inconsistent batch offsets"; return fail(HLALA_E_ARG); }
        if(nPieces > 0xFFFFFFFFull / 4) { c->err = "hlala_batch_create_from_fill: too many pieces of host units in one window"; return fail(HLALA_E_CAPACITY); }
        tableBytes = nPieces * sizeof(ResPiece); stageBytes = tableBytes + dataBytes;
        if(nPieces) {
            rc = ctx_scratch(c, stageBytes); if(rc) return fail(rc);
            stage = (uint8_t*)c->create_scratch; pieces = (ResPiece*)stage;
            walk();
            rc = dev_alloc(c, tmp, stageBytes, &dStage, false); if(rc) return fail(rc);
        }
    }
    // ---- the passes
    FilWindow W{};
    W.r0 = r0; W.nr = (u64)nr; W.b0 = (u64)rb0; W.nb = nbases; W.c0 = (u64)cb0; W.nc = (u64)nc; W.g0 = (u64)gb0; W.ng = ncig; W.u0 = u0; W.nu = u1 - u0;
    W.chainContig = dContig; W.chainPos = dPos; W.chainOffset = dOffset; W.chainAs = dAs; W.chainReverse = dReverse; W.cigarOffEnd = dCigEnd; W.cigar = dCigar; W.bases = dBases; W.quals = dQuals;      // (names, packed: null)
    if(W.c0 + W.nc > H->nChains || r1 > H->nReads) { c->err = "inconsistent batch offsets"; return fail(HLALA_E_ARG); }
    ResWindow RW{}; RW.r0 = r0; RW.nr = (u64)nr; RW.nc = (u64)nc; RW.rb0 = rb0; RW.nb = (long long)nbases; RW.cb0 = cb0; RW.gb0 = gb0; RW.ng = (long long)ncig; RW.nContigs = c->n_contigs; RW.unpaired = unpaired ? 1 : 0;
    const u32* dSrc = (const u32*)H->buf[FIL_CHAINSRC].p; const int64_t* dCig = (const int64_t*)H->buf[FIL_CHAINCIG].p; const int32_t* dPrim = (const int32_t*)H->buf[FIL_PRIMARY].p;
    hipStream_t st = c->active;
    hipError_t e = hipMemsetAsync(dSlots, 0xFF, RES_CLASSES * sizeof(u64), st);
    if(e == hipSuccess && nr) e = hipMemcpyAsync(dPrimary, dPrim + r0, (size_t)nr * 4, hipMemcpyDeviceToDevice, st);
    if(e == hipSuccess && nPieces) e = hipMemcpyAsync(dStage, stage, stageBytes, hipMemcpyHostToDevice, st);
    if(e == hipSuccess) e = hipEventRecord(H->ev[0], st);
    if(e == hipSuccess && nc) { hipLaunchKernelGGL(k_fil_chain, dim3((u32)((W.nc + 255) / 256)), dim3(256), 0, st, H->S, W, dSrc, dCig); e = hipGetLastError(); }
    if(e == hipSuccess) e = hipEventRecord(H->ev[1], st);
    if(e == hipSuccess && nc) { hipLaunchKernelGGL(k_fil_cigar, dim3((u32)((W.nc * 16 + 255) / 256)), dim3(256), 0, st, H->S, W, dSrc, dCig); e = hipGetLastError(); }
    if(e == hipSuccess) e = hipEventRecord(H->ev[2], st);
    if(e == hipSuccess && nr) { hipLaunchKernelGGL(k_fil_bases, dim3((u32)((W.nr + 3) / 4)), dim3(256), 0, st, H->S, W, (const int64_t*)H->off(0), dPrim, dSrc, (u64)H->nChains); e = hipGetLastError(); }
    if(e == hipSuccess) e = hipEventRecord(H->ev[3], st);
    if(e == hipSuccess && nPieces) { hipLaunchKernelGGL(k_res_patch, dim3((u32)((nPieces + 3) / 4)), dim3(256), 0, st, A, (const ResPiece*)dStage, (u32)nPieces, (const uint8_t*)dStage, (u64)stageBytes); e = hipGetLastError(); }
    if(e == hipSuccess) e = hipEventRecord(H->ev[4], st);
    if(e == hipSuccess && nr) { hipLaunchKernelGGL(k_res_reads, dim3((u32)((nr + 255) / 256)), dim3(256), 0, st, RW, (const int64_t*)H->off(0), (const int64_t*)H->off(1), dReadOff, dChainOff, dPrimary, dSlots); e = hipGetLastError(); }
    if(e == hipSuccess) e = hipEventRecord(H->ev[5], st);
    if(e == hipSuccess && nc) { hipLaunchKernelGGL(k_res_chains, dim3((u32)((nc + 255) / 256)), dim3(256), 0, st, RW, (const int64_t*)dCigEnd, (const int*)dContig, dCigarOff, dSlots); e = hipGetLastError(); }
    if(e == hipSuccess) e = hipEventRecord(H->ev[6], st);
    if(e == hipSuccess && nr && nc) { hipLaunchKernelGGL(k_res_chain_read, dim3((u32)(((u64)nr * 16 + 255) / 256)), dim3(256), 0, st, RW, (const int64_t*)H->off(1), dChainRead); e = hipGetLastError(); }
    if(e == hipSuccess) e = hipEventRecord(H->ev[7], st);
    u64 slots[RES_CLASSES];
    if(e == hipSuccess) e = hipMemcpyAsync(slots, dSlots, sizeof(slots), hipMemcpyDeviceToHost, st);
    // the one synchronisation of this call's own: the filters behind it index with what the kernels have just checked
    if(e == hipSuccess) e = hipStreamSynchronize(st);
    if(e != hipSuccess) { c->err = std::string("hlala_batch_create_from_fill: k_fil_chain / k_fil_cigar / k_fil_bases / k_res_patch / k_res_reads / k_res_chains / k_res_chain_read: ") + hipGetErrorString(e); (void)hipGetLastError(); return fail(HLALA_E_DEVICE); }
    for(void* p : tmp) pool_release(c, p);
    tmp.clear();
    {
        int64_t first[RES_CLASSES]; int kind1 = 0, len4 = 0;
        for(int i = 0; i < RES_CLASSES; i++) first[i] = slots[i] == RES_NONE ? -1 : (int64_t)(i == 1 ? slots[i] >> 2 : slots[i]);
        if(first[1] >= 0) kind1 = (int)(slots[1] & 3u);
        if(first[4] >= 0 && first[4] < nr) len4 = (int)(ro[r0 + (u64)first[4] + 1] - rb0) - (int)(ro[r0 + (u64)first[4]] - rb0);
        rc = res_verdict(first, kind1, len4, &c->err);
        if(rc) return fail(rc);
    }
    auto ms = [&](int a, int b2) { float t = 0; return hipEventElapsedTime(&t, H->ev[a], H->ev[b2]) == hipSuccess ? (double)t : 0.0; };
    stats->ms_chain = ms(0, 1); stats->ms_cigar = ms(1, 2); stats->ms_bases = ms(2, 3); stats->ms_patch = ms(3, 4); stats->ms_reads = ms(4, 5); stats->ms_chains = ms(5, 6); stats->ms_chain_read = ms(6, 7);
    rc = batch_create_tail(c, b, nullptr);
    if(rc) return fail(rc);
    stats->n_units = n_units; stats->n_host_units = (int64_t)nHostW; stats->n_reads = nr; stats->n_chains = nc; stats->n_cigar = (int64_t)ncig; stats->n_bases = (int64_t)nbases; stats->n_pieces = (int64_t)nPieces;
    stats->bytes_h2d = (int64_t)(stageBytes + sizeof(DevBatch)); stats->bytes_d2h = (int64_t)(sizeof(slots) + (b->prepared ? sizeof(int) : 0));
    stats->ms_wall = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tWall).count();
    *out = b;
    return HLALA_OK;
}

extern "C" int hlala_seed_batch_create_resident(hlala_seed_batch* S, hlala_ctx* c, int64_t first_unit, int32_t n_units, hlala_batch** out, hlala_batch_fill_stats* stats)
{
    if(!c) return HLALA_E_ARG;
    if(out) *out = nullptr;
    if(!S || !out || !stats) { c->err = "hlala_seed_batch_create_resident: null argument"; return HLALA_E_ARG; }
    memset(stats, 0, sizeof(*stats));
    std::string err;
    const int rc = hlala_host::seed_batch_resident(S, c, first_unit, first_unit + (int64_t)n_units, out, stats, &err);
    if(rc != HLALA_OK) c->err = err;
    return rc;
}

extern "C" int hlala_debug_batch_inputs(hlala_ctx* c, hlala_batch* b, hlala_batch_inputs_out* out)
{
    DEV_GUARD(c);
    if(!c || !b || !out) return HLALA_E_ARG;
    if(b->ctx != c) { c->err = "hlala_debug_batch_inputs: the batch belongs to another context"; return HLALA_E_ARG; }
    const DevBatch& B = b->B;
    if(B.from_seeds) { c->err = "hlala_debug_batch_inputs: the batch was created from seeds"; return HLALA_E_STATE; }
    ReaderScope rs(c, b); if(rs.rc) return rs.rc;
    const size_t nr = (size_t)B.n_reads, nc = (size_t)B.n_chains;
    int nb = 0, ng = 0;
    if(nr) HIP_TRY(c, hipMemcpyAsync(&nb, B.read_off + nr, 4, hipMemcpyDeviceToHost, c->active));
    if(nc) HIP_TRY(c, hipMemcpyAsync(&ng, B.cigar_off + nc, 4, hipMemcpyDeviceToHost, c->active));
    HIP_TRY(c, hipStreamSynchronize(c->active));
    if(nb < 0 || ng < 0) { c->err = "hlala_debug_batch_inputs: the batch holds negative sizes"; return HLALA_E_DEVICE; }
    out->n_reads = (int64_t)nr; out->n_chains = (int64_t)nc; out->n_bases = nb; out->n_cigar = ng;
#define DN(field, n) do { if(out->field && (n)) HIP_TRY(c, hipMemcpyAsync(out->field, B.field, (size_t)(n) * sizeof(*out->field), hipMemcpyDeviceToHost, c->active)); } while(0)
    DN(read_off, nr + 1); DN(read_bases, nb); DN(read_quals, nb); DN(chain_off, nr + 1); DN(read_primary, nr); DN(chain_read, nc); DN(chain_contig, nc); DN(chain_pos, nc); DN(chain_offset, nc);
    DN(chain_as, nc); DN(chain_reverse, nc); DN(cigar_off, nc + 1); DN(cigar, ng);
#undef DN
    HIP_TRY(c, hipStreamSynchronize(c->active));
    return HLALA_OK;
}

extern "C" int hlala_abi_sizeof(const char* name)
{
    if(!name) return -1;
    const std::string n(name);
#define SZ(t) if(n == #t) return (int)sizeof(t);
    SZ(hlala_graph_desc) SZ(hlala_contigs_desc) SZ(hlala_params) SZ(hlala_graph_info) SZ(hlala_batch_in) SZ(hlala_seeds_in)
    SZ(hlala_chains_out) SZ(hlala_pairs_out) SZ(hlala_batch_stats) SZ(hlala_exon_in) SZ(hlala_call_out) SZ(hlala_locus_desc) SZ(hlala_exon_positions_out) SZ(hlala_filter_params) SZ(hlala_filter_stats) SZ(hlala_insert_size_out) SZ(hlala_locus_info) SZ(hlala_locus_report_in) SZ(hlala_locus_report_out) SZ(hlala_unit_stats_out) SZ(hlala_pairs_packed_out) SZ(hlala_bgzf_block) SZ(hlala_inflate_stats) SZ(hlala_bam_rec) SZ(hlala_bam_scan_in) SZ(hlala_bam_scan_stats) SZ(hlala_bam_group_stats) SZ(hlala_bam_name_order_stats) SZ(hlala_bam_fill_in) SZ(hlala_bam_fill_out) SZ(hlala_bam_fill_stats) SZ(hlala_batch_fill_src) SZ(hlala_batch_fill_stats) SZ(hlala_batch_inputs_out)
#undef SZ
    return -1;
}

extern "C" int hlala_abi_version(void) { return HLALA_ABI_VERSION; }
extern "C" int hlala_build_flags(void)
{
    int f = 0;
#ifdef HLALA_DP_AGENT_RELEASE
    f |= HLALA_BUILD_AGENT_RELEASE;
#endif
    return f;
}

extern "C" int hlala_kat_exp(hlala_ctx* c, int n, const double* x, double* y)
{
    DEV_GUARD(c);
    if(!c || n < 0 || !x || !y) return HLALA_E_ARG;
    if(!n) return HLALA_OK;
    double *dx = nullptr, *dy = nullptr; std::vector<void*> tmp;
    int rc = dev_upload(c, tmp, x, (size_t)n, &dx); if(rc) return rc;
    rc = dev_alloc(c, tmp, (size_t)n, &dy); if(rc) return rc;
    hipLaunchKernelGGL(k_kat_exp, dim3((n + 255) / 256), dim3(256), 0, c->active, n, (const double*)dx, dy);
    HIP_TRY(c, hipMemcpyAsync(y, dy, (size_t)n * 8, hipMemcpyDeviceToHost, c->active));
    HIP_TRY(c, hipStreamSynchronize(c->active));
    for(void* p : tmp) pool_release(c, p);
    return HLALA_OK;
}

extern "C" int hlala_kat_rand_r(hlala_ctx* c, int n, uint32_t* seeds_inout, int32_t* values_out)
{
    DEV_GUARD(c);
    if(!c || n < 0 || !seeds_inout || !values_out) return HLALA_E_ARG;
    if(!n) return HLALA_OK;
    u32* ds = nullptr; int* dv = nullptr; std::vector<void*> tmp;
    int rc = dev_upload(c, tmp, seeds_inout, (size_t)n, &ds); if(rc) return rc;
    rc = dev_alloc(c, tmp, (size_t)n, &dv); if(rc) return rc;
    hipLaunchKernelGGL(k_kat_rand, dim3((n + 255) / 256), dim3(256), 0, c->active, n, ds, dv);
    HIP_TRY(c, hipMemcpyAsync(seeds_inout, ds, (size_t)n * 4, hipMemcpyDeviceToHost, c->active));
    HIP_TRY(c, hipMemcpyAsync(values_out, dv, (size_t)n * 4, hipMemcpyDeviceToHost, c->active));
    HIP_TRY(c, hipStreamSynchronize(c->active));
    for(void* p : tmp) pool_release(c, p);
    return HLALA_OK;
}

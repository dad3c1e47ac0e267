// batch.h -- device-resident batch of read pairs / chains (SoA, fixed column stride per chain).
#pragma once
#include "device_common.h"

namespace hlala {

template <template <class> class Ptr> struct DevBatchT {
    int n_pairs, n_reads, n_chains, stride;
    int from_seeds;                 // 1: seed chains were uploaded directly (no stage A / C inputs)
    int unpaired;                   // 1: one read per unit (long-read / unpaired mode): n_reads == n_pairs, no extension DP
    // ---- inputs
    Ptr<const int> read_off;            // [n_reads+1]
    Ptr<const uint8_t> read_bases;      // alignment orientation of the primary
    Ptr<const uint8_t> read_quals;
    Ptr<const int> chain_off;           // [n_reads+1]
    Ptr<const int> read_primary;        // [n_reads]
    Ptr<const int> chain_read;          // [n_chains]
    Ptr<const int> chain_contig;
    Ptr<const int> chain_pos;
    Ptr<const int> chain_offset;
    Ptr<const int> chain_as;
    Ptr<const uint8_t> chain_reverse;
    Ptr<const int> cigar_off;
    Ptr<const u32> cigar;
    // ---- stage A: seed chains (verboseSeedChain after alignment2Chain)
    Ptr<int> seed_status;               // [n_chains] HLALA_CHAIN_*
    Ptr<int> seed_ncols;
    Ptr<int> seed_begin;
    Ptr<int> seed_end;
    Ptr<int> seed_removed;
    Ptr<int> seed_level;                // [n_rows*stride]: the column rows of a chain start at row_base(B, chain)
    Ptr<int> seed_edge;
    Ptr<uint8_t> seed_g;
    Ptr<uint8_t> seed_s;
    // ---- stage B: extended chains
    Ptr<int> ext_status;
    Ptr<int> ext_ncols;
    Ptr<int> ext_begin;
    Ptr<int> ext_end;
    Ptr<double> ext_ll;
    Ptr<int> dp_iters;                  // [2*n_chains]
    Ptr<int> dp_score;                  // [2*n_chains]
    Ptr<int> dp_ncols;                  // [2*n_chains] extension columns of the DP (-1: no extension)
    Ptr<int> dp_sb;                     // [2*n_chains] read interval covered by the extension
    Ptr<int> dp_se;
    Ptr<int> dp_err;                    // [2*n_chains] 0, kernel line of a capacity failure, or -1000000 - columns
    Ptr<int> dp_alias_head;             // [2*n_chains] items whose DP starts from the same cell of the same read as this item's: head of the list (-1: none)
    Ptr<int> dp_alias_next;             // [2*n_chains] ... next entry of the list an item is on
    Ptr<int> ext_level;                 // [n_rows*stride]
    Ptr<int> ext_edge;
    Ptr<uint8_t> ext_g;
    Ptr<uint8_t> ext_s;
    Ptr<uint8_t> ext_fromseed;
    Ptr<int> ext_firstlast;             // [n_chains*4]: first level, second level, last level, second-last level (-1 = none)
    // ---- stage C: selected pair
    Ptr<int> pair_status;               // [n_pairs]
    Ptr<int> best_chain;                // [n_reads]
    Ptr<int> n_comb;                    // [n_pairs]
    Ptr<double> pair_ll;
    Ptr<double> pair_mapq;
    Ptr<double> mate_mapq;              // [n_reads]
    Ptr<uint8_t> strands_valid;
    Ptr<uint8_t> sel_mapq;              // [n_reads*stride] mapQ_perPosition of the selected chain
    // ---- counters (device): see hlala_batch_stats
    Ptr<u64> counters;                  // [32]
    Ptr<int> work_counter;              // [WC_N] dynamic work distribution: [0] stage A, [2] stage C, [7] chains stitched, [8]/[9] left / right DP items,
                                    //      [1]/[10] left / right items fetched, [12..35] retry lists (count, fetched) per tier 1..6 and direction
    Ptr<int> retry_list;                // [16*n_chains] DP items that outgrew a capacity class: (tier 1..6) x (left, right) x n_chains, the long calls from the front of a row and the short ones from its back (retry_entry); rows 14 / 15: the fail-over lists of the band kernels and the
                                    //      jump-free instantiation (WC_FO_COUNT)
    Ptr<int> pair_multi;                // [2 passes][2 classes][n_pairs] pairs with several combinations, listed by k_pair_chains for k_pair_multi (kernel_pair.hip; counts in work_counter[WC_PAIR_MULTI ...]);
                                    //      and, 4 n_pairs behind the lists of its pass ([4 n_pairs ...] main, [6 n_pairs ...] side stream), the pairs beyond the capacities, listed for
                                    //      k_pair_overflow (counts in work_counter[WC_PAIR_OVER ...]): 7 n_pairs entries in all
    Ptr<uint8_t> pair_deferred;         // [n_pairs] 1: a DP call of the pair went to the in-memory class; with the fused entry point its chains are stitched and
                                    //           the pair is scored in a second pass, after that class (which runs on a side stream next to the first pass)
    // ---- position order of the chains (kernel_order.hip): the kernels that walk the graph take their chains in this order, so that the work in flight at
    //      one time sits on neighbouring levels and its share of the graph arrays stays in the L2 (input order = read-name order = random positions)
    Ptr<int> chain_order;               // [n_chains] chain numbers sorted by position bucket; null: input order
    Ptr<int> chain_bucket;              // [n_chains] position bucket = first level >> order_shift (the last bucket: chains filtered out)
    Ptr<int> order_hist;                // [order_nb + 1] bucket counts -> bucket starts -> scatter cursors
    int order_shift, order_nb;
    int long_chunk_nodes, long_max_segs;      // long-read layout, level-by-level form of the re-threading DP (kernel_project.hip): nodes a chunk of levels may hold (<= RT_SN) and long segments a read may
                                    // have beside its short ones (<= PROJL_LONGSEG); HLALA_LONG_CHUNK_NODES / HLALA_LONG_MAXSEGS shrink them so that small tests walk every branch
    int order_cost;                 // long-read layout: buckets by DESCENDING size of the chain's window (nodes between its first and last level) instead of position -- the reads that
                                    // cross a gene window take a hundred times a backbone read's time and must not be the last ones a wavefront draws (kernel_project.hip: k_filter_chains)
    // ---- column rows only for the chains that passed the filters (round 5): two thirds of a batch's chains end at k_filter_chains (strand, duplicate coordinates,
    //      processBAM.cpp:3200-3240) and never hold a column.  The filter and the position order run when the batch is CREATED (they read inputs only), the count of the
    //      ordered chains comes back with the upload's synchronisation, and the column arrays (seed_* / ext_*: 20 bytes per column slot) are sized by it: row k belongs to
    //      chain_order[k] -- rows are in position order -- and chain_row is the inverse (-1: no row).  null: row = chain number (batches made from seeds, no position order).
    Ptr<int> chain_row;                 // [n_chains]
    int n_rows;
    Ptr<int> dp_blk;                    // [DPL_N * dp_nblk + 1] items per block of k_dp_items and list (band left / right; jump-free and general: left long / left short / right long / right short); after the scan: where they start
    Ptr<int> dp_list;                   // [2*n_chains] the fourteen dense lists of the first DP classes: slots of dp_items in position order (k_dp_lists)
    int dp_nblk;                    // blocks of k_dp_items
    int dp_band;                    // > 0: calls whose reach (read bases left + dp_band - 1 levels) stays inside a linear run of the graph go to the band kernel's lists (kernel_dp_band.hip); 0: HLALA_DP_BAND=0
    int dp_band_risky;              // tests (HLALA_DP_BAND_RISKY=1): a call is listed for the band kernel as soon as the linear run covers its read bases -- many then walk past it and exercise the fail-over
    int dp_band_nodes;              // 1: the run of a band call is the unary path of its start NODE (FlatGraph::npf_steps / npb_steps); 0 (HLALA_DP_BAND_NODES=0): the linear run of its start level, which such a path always covers
    int dp_jf;                      // > 0: calls that meet no gap-path jump go to the lists of the jump-free instantiations, reach = read bases left + dp_jf - 1 levels (HLALA_DP_JF_MARGIN + 1)
    int dp_long;                    // > 0: a call with at least this many read bases left is LONG -- drawn before the short calls of its list (dpl_list, retry_long_counter); 0: no call is (HLALA_DP_LONG_BASES)
    Ptr<void> dp_items;                 // [2*n_chains] DpItem (kernel_dp.hip)
    Ptr<int> dbg;                       // non-null with HLALA_DEBUG=1: kernels add phase clocks to counters[16..31]
};
typedef DevBatchT<HostP> DevBatch;       // the host's form and the kernels' by-value form
typedef DevBatchT<GlobP> DevBatchG;      // the device view of a descriptor in device memory (device_common.h)
static_assert(sizeof(DevBatch) == sizeof(DevBatchG), "one layout");
__device__ __forceinline__ const DevBatchG& dev_view(const DevBatch* p) { return *(const DevBatchG*)p; }
// How a kernel gets a descriptor is chosen per kernel, and per instantiation of a kernel template, by what the compiler's report and the kernel trace say
// (profiles/flat_to_global.txt): by value, through the view of the device copy, or -- the form every kernel had before -- through the plain device copy, whose
// pointers are generic.  A template that mixes forms (k_project_chains, k_pair_multi: their names are what the profile tools match on) takes both arguments and picks one; the one an
// instantiation does not read costs its 0.4-0.6 KB of the kernel-argument segment per launch and no instruction.
enum { DESC_VALUE = 0, DESC_VIEW = 1, DESC_GENERIC = 2 };
template <int FORM, class D> __device__ __forceinline__ decltype(auto) desc_of(const D& byValue, const D* inMemory)
{
    if constexpr (FORM == DESC_VIEW) return dev_view(inMemory);
    else if constexpr (FORM == DESC_GENERIC) return (*inMemory);
    else return (byValue);
}

// number of entries of B.chain_order: the chains that passed the filters (k_filter_chains); without a position order every chain is listed.
// (order_hist[order_nb - 1] is the start of a bucket nothing is put into = the end of the last real bucket, before and after the scatter)
template <class BT> __device__ __forceinline__ int ordered_chains(const BT& B) { return B.chain_order ? __builtin_amdgcn_readfirstlane(B.order_hist[B.order_nb - 1]) : B.n_chains; }

// first column slot of a chain's rows in seed_* / ext_* (only chains that passed the filters have rows: callers look at the chain's status first)
template <class BT> __device__ __forceinline__ size_t row_base(const BT& B, int c) { return (size_t)(B.chain_row ? B.chain_row[c] : c) * (size_t)B.stride; }

// ---- the first DP classes' dense item lists (k_dp_items / k_dp_lists): list k occupies dp_list[dp_blk[k * dp_nblk] .. dp_blk[(k + 1) * dp_nblk]).  A band list: k + 1 = the right
// extensions.  The jump-free and the general class have FOUR lists each -- left long, left short, right long, right short --: the two lists of a direction are one contiguous
// segment under one fetch counter, [dp_blk[k * dp_nblk], dp_blk[(k + 2) * dp_nblk]), in which the long calls (B.dp_long) come first.  A persistent kernel ends on its slowest
// call: a call of 150 bases runs seven times the trips of the typical one and must not be among the last ones drawn.
enum { DPL_BAND16 = 0, DPL_BAND32 = 2, DPL_BAND64 = 4, DPL_JF = 6, DPL_GEN = 10, DPL_N = 14 };
// the list an item is put on, by the class k_dp_items gives it (0 general, 1 jump-free, 2 / 3 / 4 band kernel with 16 / 32 / 64 lanes per call), its direction (1: right) and whether it is long
__host__ __device__ inline int dpl_list(int cls, int dir, bool isLong)
{
    if(cls >= 2) return (cls == 2 ? DPL_BAND16 : (cls == 3 ? DPL_BAND32 : DPL_BAND64)) + dir;
    return (cls == 1 ? DPL_JF : DPL_GEN) + 2 * dir + (isLong ? 0 : 1);
}
// read bases a call can consume: what lies before the seed for a left extension, behind it for a right one
__host__ __device__ inline int dp_bases_left(int dir, int seqLen, int start_seq) { return dir ? seqLen - start_seq : start_seq; }
__host__ __device__ inline bool dp_is_long(int dpLong, int dir, int seqLen, int start_seq) { return dpLong > 0 && dp_bases_left(dir, seqLen, start_seq) >= dpLong; }
// ---- B.work_counter (WC_N ints): [0] stage A, [1] / [10] left / right general items fetched, [2] stage C, [4] / [5] jump-free items fetched, [6] jump-free calls (statistics),
// [7] chains stitched, [8] / [9] left / right DP calls, [12..35] retry lists of tiers 1..6 (count, fetched) x (left, right), [36] / [37] second stitch / pairing pass,
// [40..47] round 6: the lists of the pairs with several combinations (k_pair_chains -> k_pair_multi): per pass (main / side stream) count and fetched of class 0, of class 1; round 5: items fetched by the three band kernels (left, right each), the fail-over list's counts and fetch counters, band calls that
// failed over, band calls listed, jump-free calls that met a jump, and why band calls failed ([WC_BAND_WHY + 2 .. + 5]: past the staged levels, past the linear run, too
// many iterations, too many tied end cells); [WC_BAND_NODES]: band calls listed through the path of their start node that the linear run of its level does not cover
// [72..79] the overflow lists of the pairing passes (k_pair_chains -> k_pair_overflow, kernel_pair_overflow.hip): per pass (main / side stream) pairs listed, fetched,
// scored, refused for want of slab
// [80..87] unused: [72..87] counted the calls of the two-track band kernels of round 6, which were removed; the debug export (include/hlala_gpu.h: HLALA_DEBUG_WC_N) stays at
// these 88
// [88..99] the LONG calls on the retry lists of tiers 1..6 x (left, right).  A row of retry_list is filled from both ends: a long call takes entry q of
// work_counter[WC_RETRY_LONG + ...] from the front, a short one entry n_chains - 1 - q of the row's old counter ([12 + 4(k-1) + 2p], which with B.dp_long = 0 counts every call,
// as it always did) from the back; the class that draws the row takes the long ones first (retry_entry).  A row holds a direction's items at most once each: the ends never meet.
enum { WC_PAIR_MULTI = 40, WC_PAIR_OVER = 72, WC_BAND_FETCH = 48, WC_FO_COUNT = 54, WC_FO_FETCH = 56, WC_BAND_FAILED = 58, WC_BAND_CALLS = 59, WC_JF_FAILED = 60, WC_BAND_WHY = 62, WC_BAND_TIED = 68, WC_BAND_NODES = 69,
       WC_RETRY_LONG = 88, WC_N = 100 };
// counters of the retry list of tier k = 1..6 and direction p: the short calls pushed (from the back), the fetch counter of the whole row, the long calls pushed (from the front)
__host__ __device__ inline int wc_retry_short(int tier, int dir) { return 12 + 4 * (tier - 1) + 2 * dir; }
__host__ __device__ inline int wc_retry_fetch(int tier, int dir) { return 13 + 4 * (tier - 1) + 2 * dir; }
__host__ __device__ inline int wc_retry_long(int tier, int dir) { return WC_RETRY_LONG + 2 * (tier - 1) + dir; }
// where the w-th draw of a retry row with nLong long calls lies: the long calls from the front, then the short ones from the back
__host__ __device__ inline int retry_entry(int w, int nLong, int nChains) { return w < nLong ? w : nChains - 1 - (w - nLong); }
// the fail-over list of the first classes: calls the band kernel (kernel_dp_band.hip) or the jump-free instantiation could not finish; k_dp<DpTiny, 0> draws it after
// its own lists.  Entries (slots of dp_items) at retry_list[(14 + direction) * n_chains ...], counts in work_counter[WC_FO_COUNT + direction].
// ---- capacities of the band kernels (kernel_dp_band.hip): read bases a call may have left for the instantiation with 16 / 32 / 64 lanes per call; k_dp_items lists a call
// for one of them when the unary path ahead of its start node (dp_band_nodes = 0: the linear run ahead of its start level) covers bases left + margin + min(bases left + 6, 40) steps
constexpr int BAND_MAXJ16 = 15, BAND_MAXJ32 = 31, BAND_MAXJ64 = 48;

enum {
    CNT_CHAINS_EXT = 0, CNT_DP_CALLS, CNT_DP_ITERS, CNT_DP_CELLS, CNT_SEED_COLS, CNT_OUT_COLS, CNT_EDGES, CNT_ERRORS, CNT_DP_SHARED
};

}  // namespace hlala

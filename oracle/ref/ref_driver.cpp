/* C ABI over the reference aligner (mapper::aligner::extensionAligner of HLA*LA) and over the static members of
 * mapper::processBAM around it (projection, pairing, mapping qualities), linked from the reference's own sources by
 * oracle/ref/Makefile into oracle/_ref/libhlala_ref.so.  Test infrastructure: the referee of oracle/hlala_oracle.cpp and,
 * through the fixtures it writes, of the HIP kernels.  Nothing here restates the aligner; this file builds its inputs, calls
 * it and copies its outputs.  Three short passages of processBAM.cpp that sit inside non-static members are followed line by
 * line, each line citing the one it follows: the gap filling at the head of PRGContigAlignment2Seed (only for the optional
 * intermediate stages of ref_project_chains), the pairing double loop and the selection of alignOneReadPair (ref_pair_chains).
 * Everything they call is the reference's.  The typer (hla::HLATyper) is reached the same way: ref_typer_infer calls HLATypeInference
 * itself, ref_typer_exon_positions follows the two read loops at its head (hla/HLATyper.cpp:1386-1495) line by line around the
 * reference's protected members, ref_typer_include is its intervalOverlapsWithGenes.
 *
 * Order is pointer order in the reference (std::set<Node*>, std::set<Edge*>, std::map<Node*, ...>): all nodes live in
 * one array and all edges in one array, in the order of the graph description, so that pointer order is index order
 * and an Edge* turns back into an index by subtraction. */
#include "mapper/processBAM.h"
#include "mapper/aligner/extensionAligner.h"
#include "mapper/reads/PRGContigBAMAlignment.h"
#include "Utilities.h"
#include "mapper/reads/oneRead.h"
#include "mapper/reads/verboseSeedChain.h"
#include "Graph/Graph.h"
#include "Graph/Node.h"
#include "Graph/Edge.h"
#include "hla/HLATyper.h"
#include "hla/oneExonPosition.h"

#include "hlala_gpu.h"

#include <omp.h>
#include <unistd.h>

#include <algorithm>
#include <cmath>
#include <csetjmp>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <map>
#include <stdexcept>
#include <string>
#include <vector>

namespace {

std::string g_err;

/* The reference asserts (it is built without NDEBUG: its concordance checks are part of what is run).  A failed assert
 * inside a ref_* call must fail that call, not end the test process: the library is linked -Bsymbolic-functions, so the
 * reference objects bind to the __assert_fail below, which leaves through the jmp_buf armed by the running call. */
thread_local jmp_buf* t_armed = nullptr;
thread_local char t_assert_msg[512];

struct Quiet {          /* the constructor and computeGapEdgePaths write progress to std::cout / std::cerr */
    std::ios::iostate out, err;
    Quiet() : out(std::cout.rdstate()), err(std::cerr.rdstate()) { std::cout.setstate(std::ios::failbit); std::cerr.setstate(std::ios::failbit); }
    void restore() { std::cout.clear(out); std::cerr.clear(err); }
    ~Quiet() { restore(); }
};

}  // namespace

extern "C" void __assert_fail(const char* assertion, const char* file, unsigned int line, const char* function)
#if defined(__GNUC__)
    __attribute__((noreturn))
#endif
    ;
extern "C" void __assert_fail(const char* assertion, const char* file, unsigned int line, const char* function)
{
    snprintf(t_assert_msg, sizeof(t_assert_msg), "reference assert failed: %s (%s:%u, %s)", assertion, file, line, function ? function : "?");
    if(t_armed) longjmp(*t_armed, 1);
    fprintf(stderr, "%s\n", t_assert_msg);
    abort();
}

struct ref_handle {
    int n_levels = 0, n_nodes = 0, n_edges = 0;
    Node* nodes = nullptr;
    Edge* edges = nullptr;
    Graph* g = nullptr;
    mapper::aligner::extensionAligner* A = nullptr;

    int edge_index(const Edge* e) const
    {
        if(e == nullptr) return -1;
        if(e < edges || e >= edges + n_edges) throw std::runtime_error("a pseudo edge of computeGapEdgePaths reached an output column");
        return (int)(e - edges);
    }
    int node_index(const Node* n) const
    {
        if(n < nodes || n >= nodes + n_nodes) throw std::runtime_error("a pseudo node of computeGapEdgePaths reached an output");
        return (int)(n - nodes);
    }
};

/* runs f() with reference asserts turned into an error return */
template<class F> static int guarded(F f)
{
    jmp_buf jb;
    Quiet q;
    if(setjmp(jb)) { t_armed = nullptr; q.restore(); g_err = t_assert_msg; return -1; }
    t_armed = &jb;
    int rc;
    try { rc = f(); } catch(std::exception& e) { g_err = e.what(); rc = -1; }
    t_armed = nullptr;
    return rc;
}

/* one chain of a hlala_seeds_in as the reference's verboseSeedChain (is_from_BWAseed all true) */
static mapper::reads::verboseSeedChain chain_from_columns(const ref_handle* h, const hlala_seeds_in* in, int c)
{
    mapper::reads::verboseSeedChain s;
    s.sequence_begin = in->chain_seq_begin[c]; s.sequence_end = in->chain_seq_end[c]; s.reverse = in->chain_reverse[c] != 0;
    for(int j = in->col_off[c]; j < in->col_off[c + 1]; j++) {
        int e = in->col_edge[j];
        if(e < -1 || e >= h->n_edges) throw std::runtime_error("seed edge out of range");
        s.graph_aligned_levels.push_back(in->col_level[j]); s.graph_aligned_edges.push_back(e < 0 ? nullptr : &h->edges[e]);
        s.graph_aligned.push_back((char)in->col_gchar[j]); s.sequence_aligned.push_back((char)in->col_schar[j]);
        s.is_from_BWAseed.push_back(true);
    }
    return s;
}

/* extendSeedChain + scoreOneAlignment of chain c of `in`, the generator seeded from seedL (left DP) and seedR (right DP); see ref_extend_seeds for `mode` */
static mapper::reads::verboseSeedChain extend_and_score(ref_handle* h, const hlala_seeds_in* in, int c, unsigned seedL, unsigned seedR, int long_read_mode, int mode, double& ll)
{
    using mapper::reads::verboseSeedChain;
    mapper::aligner::extensionAligner& A = *h->A;
    int r = in->chain_read[c];
    std::string seq((const char*)in->read_bases + in->read_off[r], in->read_off[r + 1] - in->read_off[r]);
    std::string qual((const char*)in->read_quals + in->read_off[r], in->read_off[r + 1] - in->read_off[r]);
    verboseSeedChain s = chain_from_columns(h, in, c);
    const bool clipL = s.sequence_begin != 0, clipR = s.sequence_end != (int)seq.size() - 1;
    verboseSeedChain e;
    if(mode == 0 && clipL && clipR) {
        A.rng_seeds.at(0) = seedL;
        verboseSeedChain l = A.extendSeedChain(seq.substr(0, s.sequence_end + 1), s);
        A.rng_seeds.at(0) = seedR;
        e = A.extendSeedChain(seq, l);
    } else {
        A.rng_seeds.at(0) = clipL ? seedL : seedR;          /* the seed of the first DP that runs */
        e = A.extendSeedChain(seq, s);
    }
    e.checkLevelContiguity();
    mapper::reads::oneRead rd("read", seq, qual);         /* original orientation, as processBAM hands it over */
    if(s.reverse) rd.invert();
    ll = A.scoreOneAlignment(e, rd, long_read_mode ? "longReads" : "");
    return e;
}

/* columns of a reference chain into row `row` of strided arrays (any pointer may be NULL) */
static int store_columns(const ref_handle* h, const mapper::reads::verboseSeedChain& e, size_t row, int stride, int32_t* col_level, int32_t* col_edge, uint8_t* col_gchar,
                         uint8_t* col_schar, uint8_t* col_fromseed, uint8_t* col_mapq)
{
    int n = (int)e.graph_aligned_levels.size();
    if(n > stride) throw std::runtime_error("more alignment columns than the output stride");
    if((int)e.graph_aligned_edges.size() != n || (int)e.graph_aligned.size() != n || (int)e.sequence_aligned.size() != n || (int)e.is_from_BWAseed.size() != n)
        throw std::runtime_error("reference chain rows of unequal length");
    if(col_mapq && (int)e.mapQ_perPosition.size() != n) throw std::runtime_error("mapQ_perPosition of another length than the chain");
    size_t base = row * stride;
    for(int j = 0; j < n; j++) {
        int ei = h->edge_index(e.graph_aligned_edges[j]);
        if(col_level) col_level[base + j] = e.graph_aligned_levels[j];
        if(col_edge) col_edge[base + j] = ei;
        if(col_gchar) col_gchar[base + j] = (uint8_t)e.graph_aligned[j];
        if(col_schar) col_schar[base + j] = (uint8_t)e.sequence_aligned[j];
        if(col_fromseed) col_fromseed[base + j] = e.is_from_BWAseed[j] ? 1 : 0;
        if(col_mapq) col_mapq[base + j] = (uint8_t)e.mapQ_perPosition[j];
    }
    return n;
}

extern "C" {

const char* ref_last_error() { return g_err.c_str(); }

ref_handle* ref_create(const hlala_graph_desc* d)
{
    ref_handle* h = new ref_handle();
    int rc = guarded([&]() -> int {
        h->n_levels = d->n_levels; h->n_nodes = d->n_nodes; h->n_edges = d->n_edges;
        for(int i = 0; i < d->n_nodes; i++) if(d->node_level[i] < 0 || d->node_level[i] >= d->n_levels) throw std::runtime_error("node level out of range");
        for(int i = 0; i < d->n_edges; i++) {
            int a = d->edge_from[i], b = d->edge_to[i];
            if(a < 0 || a >= d->n_nodes || b < 0 || b >= d->n_nodes) throw std::runtime_error("edge endpoint out of range");
            if(d->node_level[b] != d->node_level[a] + 1) throw std::runtime_error("edge does not connect level l to l+1");
            if(d->edge_label[i] == 0) throw std::runtime_error("edge label 0");
        }
        h->nodes = new Node[d->n_nodes];
        h->edges = new Edge[d->n_edges];
        h->g = new Graph();
        for(int i = 0; i < d->n_nodes; i++) {
            Node* n = &h->nodes[i];
            n->level = (unsigned int)d->node_level[i];
            n->terminal = d->node_level[i] == d->n_levels - 1;
            h->g->registerNode(n, n->level);
        }
        for(int i = 0; i < d->n_edges; i++) {
            Edge* e = &h->edges[i];
            e->From = &h->nodes[d->edge_from[i]]; e->To = &h->nodes[d->edge_to[i]];
            e->emission = d->edge_label[i]; e->locus_id = "L"; e->count = 1;
            e->From->Outgoing_Edges.insert(e); e->To->Incoming_Edges.insert(e);
            h->g->registerEdge(e);
        }
        if((int)h->g->NodesPerLevel.size() != d->n_levels) throw std::runtime_error("a level without nodes");
        h->A = new mapper::aligner::extensionAligner(h->g);
        return 0;
    });
    if(rc != 0) return nullptr;          /* what was allocated stays allocated: the reference may hold pointers into it */
    return h;
}

void ref_destroy(ref_handle* h)
{
    if(!h) return;
    delete h->A; delete h->g; delete[] h->edges; delete[] h->nodes; delete h;
}

int ref_graph_n_paths(ref_handle* h) { return (int)h->g->completedGapEdgePaths.size(); }

/* Graph::completedGapEdgePaths as (first node, last node, length): the shape of orc_graph_get_paths */
int ref_graph_paths(ref_handle* h, int32_t* first_node, int32_t* last_node, int32_t* length)
{
    return guarded([&]() -> int {
        const auto& P = h->g->completedGapEdgePaths;
        for(size_t i = 0; i < P.size(); i++) {
            for(const Edge* e : P[i]) h->edge_index(e);
            first_node[i] = h->node_index(P[i].front()->From); last_node[i] = h->node_index(P[i].back()->To); length[i] = (int)P[i].size();
        }
        return 0;
    });
}

/* extendSeedChain + scoreOneAlignment per chain.  Chain c draws from rng_seed + 2c (left DP) and rng_seed + 2c + 1
 * (right DP) in mode 0, the discipline of the oracle and the product: a chain clipped at both ends takes two reference
 * calls, the first on the read's prefix up to the seed's end (no right extension is attempted), the second on the whole
 * read with the first call's result as its seed (no left extension is attempted).  mode 1 is one call per chain, seeded
 * for the first DP that runs: the reference's native discipline, where the right DP of a chain clipped at both ends
 * continues the generator state its left DP left.  Chains clipped at one end run the same in both modes.
 * dp_iters / dp_score / removed_cols of `out` are not written. */
int ref_extend_seeds(ref_handle* h, const hlala_seeds_in* in, hlala_chains_out* out, uint32_t rng_seed, int long_read_mode, int stride, int mode)
{
    return guarded([&]() -> int {
        for(int c = 0; c < in->n_chains; c++) {
            double ll;
            const unsigned seedL = rng_seed + 2u * (unsigned)c;
            mapper::reads::verboseSeedChain e = extend_and_score(h, in, c, seedL, seedL + 1u, long_read_mode, mode, ll);
            int n = store_columns(h, e, (size_t)c, stride, out->col_level, out->col_edge, out->col_gchar, out->col_schar, out->col_fromseed, nullptr);
            if(out->status) out->status[c] = HLALA_CHAIN_OK;
            if(out->n_cols) out->n_cols[c] = n;
            if(out->seq_begin) out->seq_begin[c] = e.sequence_begin;
            if(out->seq_end) out->seq_end[c] = e.sequence_end;
            if(out->ll) out->ll[c] = ll;
        }
        return 0;
    });
}

/* ------------------------------------------------------------------ projection: processBAM::alignment2Chain (processBAM.cpp:3050-3126)
 *
 * For every chain c of the batch with keep[c] != 0 (c counted from the batch's first chain; the keep mask is an INPUT: the strand and
 * identical-coordinate pre-filter of alignOneReadPair, :3200-3240, goes through a non-static member and is not pinned here) a
 * BamTools::BamAlignment is built from the batch row and handed to the reference in the order of alignment2Chain:
 * transformBAMreadToInternalAlignment, the sub-sequence check of :3062-3083, PRGContigBAMAlignment::checkAlignmentConcordanceWithSequence,
 * PRGContigAlignment2Seed(paranoid = true).
 * The protected statics are reached through a derived type with using-declarations; no processBAM object exists.
 *
 * AlignedBases encodes BamTools' semantics, not the reference's.  The rule used is that of BamAlignment::BuildCharData as BamTools
 * documents it: walking the CIGAR over QueryBases (the read without its hard-clipped ends), M / = / X / I copy their query bases,
 * S skips its query bases and writes nothing, D writes one '-' per base, P one '*' per base, N one 'N' per base, H nothing.
 *
 * inGraphGapStretch is the result of the constructor's scan (:91-149), which cannot be called; it is an argument (in_gap_stretch,
 * n_levels - 1 entries) and pinned by the CPU test against a NumPy statement of the rule.
 *
 * status: REF_PROJ_OK, or REF_PROJ_REFUSED when transformBAMreadToInternalAlignment returned false (nothing else is written then).
 * A reference assert or exception fails the call (ref_last_error has the text).
 * `stages`, when not NULL, points to three hlala_chains_out that take the columns (levels, both character rows, n_cols, seq_begin,
 * seq_end) after transformBAMreadToInternalAlignment, after cleanInitialAlignment and after restrictInitialAlignmentToNoGapAreas;
 * the last two are reached as PRGContigAlignment2Seed reaches them, by the gap filling of :2515-2577 and the two static functions. */
#define REF_PROJ_OK      0
#define REF_PROJ_REFUSED 1

namespace {
struct Access : mapper::processBAM {
    using mapper::processBAM::transformBAMreadToInternalAlignment;
    using mapper::processBAM::cleanInitialAlignment;
    using mapper::processBAM::restrictInitialAlignmentToNoGapAreas;
};
struct ContigTables {
    std::vector<std::string> seq; std::vector<std::vector<int>> level;
    explicit ContigTables(const hlala_contigs_desc* d)
    {
        for(int i = 0; i < d->n_contigs; i++) {
            seq.emplace_back((const char*)d->contig_seq + d->contig_off[i], (size_t)(d->contig_off[i + 1] - d->contig_off[i]));
            level.emplace_back(d->contig_level + d->contig_off[i], d->contig_level + d->contig_off[i + 1]);
        }
    }
};
const char* const CIGAR_OPS = "MIDNSHP=X";

void store_stage(hlala_chains_out* o, int row, int stride, const std::vector<int>& lv, const std::string& ga, const std::string& sa, int begin, int end)
{
    int n = (int)lv.size();
    if(n > stride) throw std::runtime_error("more alignment columns than the output stride");
    if((int)ga.size() != n || (int)sa.size() != n) throw std::runtime_error("reference alignment rows of unequal length");
    if(o->n_cols) o->n_cols[row] = n;
    if(o->seq_begin) o->seq_begin[row] = begin;
    if(o->seq_end) o->seq_end[row] = end;
    size_t base = (size_t)row * stride;
    for(int j = 0; j < n; j++) {
        if(o->col_level) o->col_level[base + j] = lv[j];
        if(o->col_gchar) o->col_gchar[base + j] = (uint8_t)ga[j];
        if(o->col_schar) o->col_schar[base + j] = (uint8_t)sa[j];
    }
}
}  // namespace

int ref_project_chains(ref_handle* h, const hlala_contigs_desc* contigs, const hlala_batch_in* in, int n_reads, const uint8_t* keep, const uint8_t* in_gap_stretch,
                       int stride, hlala_chains_out* out, hlala_chains_out* stages)
{
    return guarded([&]() -> int {
        using mapper::reads::verboseSeedChain;
        ContigTables T(contigs);
        std::vector<bool> inGraphGapStretch(in_gap_stretch, in_gap_stretch + (h->n_levels - 1));
        const int64_t c0 = in->chain_off[0];
        for(int r = 0; r < n_reads; r++) {
            const std::string seq((const char*)in->read_bases + in->read_off[r], (size_t)(in->read_off[r + 1] - in->read_off[r]));
            const std::string qual((const char*)in->read_quals + in->read_off[r], (size_t)(in->read_off[r + 1] - in->read_off[r]));
            for(int64_t c = in->chain_off[r]; c < in->chain_off[r + 1]; c++) {
                const int row = (int)(c - c0);
                if(!keep[row]) continue;
                const int contig = in->chain_contig[c];
                if(contig < 0 || contig >= contigs->n_contigs) throw std::runtime_error("chain contig out of range");

                BamTools::BamAlignment al;
                al.Name = "read"; al.RefID = contig; al.Position = in->chain_pos[c];
                al.SetIsReverseStrand(in->chain_reverse[c] != 0);
                size_t clipH[2] = {0, 0};
                const int64_t k0 = in->cigar_off[c], k1 = in->cigar_off[c + 1];
                for(int64_t k = k0; k < k1; k++) {
                    unsigned op = in->cigar[k] & 15u, len = in->cigar[k] >> 4;
                    if(op >= 9) throw std::runtime_error("CIGAR operation code out of range");
                    al.CigarData.push_back(BamTools::CigarOp(CIGAR_OPS[op], len));
                    if(CIGAR_OPS[op] == 'H' && k == k0) clipH[0] = len;
                    else if(CIGAR_OPS[op] == 'H' && k == k1 - 1) clipH[1] = len;
                }
                if(clipH[0] + clipH[1] > seq.size()) throw std::runtime_error("hard clips longer than the read");
                al.QueryBases = seq.substr(clipH[0], seq.size() - clipH[0] - clipH[1]);
                al.Qualities = qual.substr(clipH[0], seq.size() - clipH[0] - clipH[1]);
                al.Length = (int32_t)al.QueryBases.size();
                {   /* AlignedBases by the BuildCharData rule stated above */
                    size_t q = 0;
                    for(const BamTools::CigarOp& op : al.CigarData) {
                        switch(op.Type) {
                        case 'M': case '=': case 'X': case 'I':
                            if(q + op.Length > al.QueryBases.size()) throw std::runtime_error("CIGAR consumes more bases than the record has");
                            al.AlignedBases.append(al.QueryBases, q, op.Length); q += op.Length; break;
                        case 'S': q += op.Length; break;
                        case 'D': al.AlignedBases.append(op.Length, '-'); break;
                        case 'P': al.AlignedBases.append(op.Length, '*'); break;
                        case 'N': al.AlignedBases.append(op.Length, 'N'); break;
                        case 'H': break;
                        }
                    }
                }

                mapper::reads::PRGContigBAMAlignment PRGcontigAlignment;
                bool ok = Access::transformBAMreadToInternalAlignment(T.seq.at(contig), T.level.at(contig), in->chain_offset[c], al, seq, qual, PRGcontigAlignment);   /* :3051-3059 */
                if(!ok) { if(out->status) out->status[row] = REF_PROJ_REFUSED; if(out->n_cols) out->n_cols[row] = 0; continue; }
                {   /* the sub-sequence check of :3062-3083: the read between startInRaw and stopInRaw is sequence_aligned without its gaps */
                    if(seq.find('_') != std::string::npos) throw std::runtime_error("'_' in a read");                                              /* :3062 */
                    std::string subSequence = seq.substr(PRGcontigAlignment.sequence_aligned_startInRaw, PRGcontigAlignment.sequence_aligned_stopInRaw - PRGcontigAlignment.sequence_aligned_startInRaw + 1);   /* :3063 */
                    std::string sequence_aligned_noGaps = Utilities::removeGaps(PRGcontigAlignment.sequence_aligned);                              /* :3066 */
                    if(!(sequence_aligned_noGaps == subSequence)) throw std::runtime_error("Mismatch in sequence check!");                         /* :3068-3082 */
                }
                PRGcontigAlignment.checkAlignmentConcordanceWithSequence(seq);                                     /* :3114 */
                verboseSeedChain graphSeed, sequenceSeed;
                mapper::processBAM::PRGContigAlignment2Seed(h->g, PRGcontigAlignment, true, graphSeed, sequenceSeed, inGraphGapStretch);   /* :3121 */
                sequenceSeed.is_from_BWAseed.resize(sequenceSeed.graph_aligned_levels.size(), 1);               /* :3124 */

                int n = store_columns(h, sequenceSeed, (size_t)row, stride, out->col_level, out->col_edge, out->col_gchar, out->col_schar, out->col_fromseed, nullptr);
                if(out->status) out->status[row] = REF_PROJ_OK;
                if(out->n_cols) out->n_cols[row] = n;
                if(out->seq_begin) out->seq_begin[row] = sequenceSeed.sequence_begin;
                if(out->seq_end) out->seq_end[row] = sequenceSeed.sequence_end;
                if(out->removed_cols) out->removed_cols[row] = sequenceSeed.removed_columns_noGap_restriction;

                if(stages) {
                    const mapper::reads::PRGContigBAMAlignment& A = PRGcontigAlignment;
                    store_stage(&stages[0], row, stride, A.graph_aligned_levels, A.graph_aligned, A.sequence_aligned, A.sequence_aligned_startInRaw, A.sequence_aligned_stopInRaw);
                    std::vector<int> lv; std::string ga, sa;
                    int startInRaw = A.sequence_aligned_startInRaw, stopInRaw = A.sequence_aligned_stopInRaw;                   /* :2515-2516 */
                    unsigned int firstColumn = 0;
                    while(A.graph_aligned_levels.at(firstColumn) == -1) { firstColumn++; startInRaw++; }                      /* :2518-2523 */
                    unsigned int lastColumn = A.graph_aligned_levels.size() - 1;
                    while(A.graph_aligned_levels.at(lastColumn) == -1) { lastColumn--; stopInRaw--; }                         /* :2526-2531 */
                    int lastInserted_graphLevel = -1;
                    for(unsigned int columnI = firstColumn; columnI <= lastColumn; columnI++) {                                /* :2538 */
                        int l = A.graph_aligned_levels.at(columnI);
                        if(columnI != firstColumn && l != -1 && (lastInserted_graphLevel + 1) != l)                            /* :2561 */
                            for(int insertLevelI = lastInserted_graphLevel + 1; insertLevelI <= l - 1; insertLevelI++) { lv.push_back(insertLevelI); ga.push_back('_'); sa.push_back('_'); }   /* :2564-2569 */
                        lv.push_back(l); ga.push_back(A.graph_aligned.at(columnI)); sa.push_back(A.sequence_aligned.at(columnI));   /* :2546-2548, :2555-2557, :2572-2574 */
                        if(l != -1) lastInserted_graphLevel = l;                                                               /* :2549, :2575 */
                    }
                    Access::cleanInitialAlignment(lv, ga, sa);                                                                 /* :2590 */
                    store_stage(&stages[1], row, stride, lv, ga, sa, startInRaw, stopInRaw);
                    Access::restrictInitialAlignmentToNoGapAreas(lv, ga, sa, startInRaw, stopInRaw, inGraphGapStretch);        /* :2602 */
                    store_stage(&stages[2], row, stride, lv, ga, sa, startInRaw, stopInRaw);
                }
            }
        }
        return 0;
    });
}

/* ------------------------------------------------------------------ pairing: processBAM::alignOneReadPair from its pairing loop on (:3408-3550)
 *
 * `in` holds the seed chains that were kept (the product's keep decision is an input, see above), chain_read[c] = 2p + m for mate m of
 * pair p, chains of a read in their order in the batch; chain_abs[c] is the chain's absolute index in the batch, so that chain c is
 * extended with the product's seeds rng_seed + 2 * chain_abs[c] + d (mode 0 of ref_extend_seeds, the same code).  The double loop and the
 * selection follow :3408-3506 and :3538-3550; what they call -- alignedReadPair_strandsValid, alignedReadPair_pairsDistanceInGraphLevels,
 * alignedReadPair_pairsDistancesUnderlyingSequences, Utilities::findVectorMax, assignMappingQualities -- is the reference's, and
 * boost::math::pdf is the stand-in formula of standin/boost/math/distributions/normal.hpp (the insert-size density is pinned up to it).
 * graphLevel_2_underlyingSequencePositions is filled from the contigs as _loadMapping does (:4441-4456).
 * ext_out (may be NULL) takes the extended chains with their log-likelihoods, row = c; best_is_penalty[p] (may be NULL) says whether the
 * insert-size term of the selected combination is max_insertsize_penalty_log. */
int ref_pair_chains(ref_handle* h, const hlala_contigs_desc* contigs, const hlala_params* params, const hlala_seeds_in* in, const int32_t* chain_abs, int n_pairs,
                    hlala_chains_out* ext_out, hlala_pairs_out* out, uint8_t* best_is_penalty)
{
    return guarded([&]() -> int {
        using mapper::reads::verboseSeedChain;
        const int stride = params->max_columns;
        mapper::aligner::extensionAligner* eA = h->A;

        std::vector<std::map<int, int>> graphLevel_2_underlyingSequencePositions(h->n_levels);                                 /* :60-61 */
        {
            std::vector<int> order(contigs->n_contigs);
            for(int i = 0; i < contigs->n_contigs; i++) order[i] = i;
            std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return contigs->contig_seqid[a] < contigs->contig_seqid[b]; });
            for(int i : order) {
                const int ID = contigs->contig_seqid[i];
                for(int64_t p = contigs->contig_off[i]; p < contigs->contig_off[i + 1]; p++) {
                    int thisLevel = contigs->contig_level[p];
                    if(thisLevel < 0 || thisLevel >= h->n_levels) throw std::runtime_error("translation level out of range");
                    graphLevel_2_underlyingSequencePositions.at((unsigned int)thisLevel)[ID] = (int)(p - contigs->contig_off[i]);   /* :4454 */
                }
            }
        }

        boost::math::normal rnd_InsertSize(params->insert_mean, params->insert_sd);                                           /* :2342 */
        double max_insertsize_penalty = boost::math::pdf(rnd_InsertSize, params->insert_mean + 8 * params->insert_sd);         /* :2343 */
        if(!(max_insertsize_penalty > 0 && max_insertsize_penalty <= 1)) throw std::runtime_error("max_insertsize_penalty out of (0, 1]");   /* :2344-2345 */
        double max_insertsize_penalty_log = log(max_insertsize_penalty);                                                       /* :2346 */

        std::vector<std::vector<verboseSeedChain>> chains(2 * (size_t)n_pairs);
        std::vector<std::vector<double>> lls(2 * (size_t)n_pairs);
        std::vector<std::vector<int>> abs_index(2 * (size_t)n_pairs);
        for(int c = 0; c < in->n_chains; c++) {
            int r = in->chain_read[c];
            if(r < 0 || r >= 2 * n_pairs) throw std::runtime_error("chain_read out of range");
            if(c > 0 && in->chain_read[c - 1] > r) throw std::runtime_error("chains are not in read order");
            double ll;
            const unsigned seedL = params->rng_seed + 2u * (unsigned)chain_abs[c];
            verboseSeedChain e = extend_and_score(h, in, c, seedL, seedL + 1u, params->long_read_mode, 0, ll);
            if(ext_out) {
                int n = store_columns(h, e, (size_t)c, stride, ext_out->col_level, ext_out->col_edge, ext_out->col_gchar, ext_out->col_schar, ext_out->col_fromseed, nullptr);
                if(ext_out->status) ext_out->status[c] = HLALA_CHAIN_OK;
                if(ext_out->n_cols) ext_out->n_cols[c] = n;
                if(ext_out->seq_begin) ext_out->seq_begin[c] = e.sequence_begin;
                if(ext_out->seq_end) ext_out->seq_end[c] = e.sequence_end;
                if(ext_out->ll) ext_out->ll[c] = ll;
            }
            chains[r].push_back(e); lls[r].push_back(ll); abs_index[r].push_back(chain_abs[c]);
        }

        for(int p = 0; p < n_pairs; p++) {
            const std::vector<verboseSeedChain>& read1_extendedChains = chains[2 * p];
            const std::vector<verboseSeedChain>& read2_extendedChains = chains[2 * p + 1];
            const std::vector<double>& read1_extendedChains_log_likelihoods = lls[2 * p];
            const std::vector<double>& read2_extendedChains_log_likelihoods = lls[2 * p + 1];
            if(!(read1_extendedChains.size() > 0 && read2_extendedChains.size() > 0)) throw std::runtime_error("a mate without extended chains");   /* :3394-3395 */

            mapper::reads::verboseSeedChainPair forReturn;                                                                     /* :3393 */
            std::vector<std::pair<unsigned int, unsigned int>> combinations_indices;                                           /* :3398 */
            std::vector<double> combinations_LL;                                                                               /* :3399 */
            std::vector<double> combinations_LL_insertSizeOnly;                                                                /* :3400 */
            for(unsigned int read1_alignmentI = 0; read1_alignmentI < read1_extendedChains.size(); read1_alignmentI++)         /* :3408 */
            {
                for(unsigned int read2_alignmentI = 0; read2_alignmentI < read2_extendedChains.size(); read2_alignmentI++)     /* :3410 */
                {
                    double combined_log_likelihood = read1_extendedChains_log_likelihoods.at(read1_alignmentI) +
                                                     read2_extendedChains_log_likelihoods.at(read2_alignmentI);                /* :3414-3415 */
                    const verboseSeedChain& chain_read1 = read1_extendedChains.at(read1_alignmentI);                           /* :3422 */
                    const verboseSeedChain& chain_read2 = read2_extendedChains.at(read2_alignmentI);                           /* :3423 */
                    bool strandsValid = eA->alignedReadPair_strandsValid(chain_read1, chain_read2);                            /* :3425 */
                    double log_likelihood_insertSize;                                                                          /* :3430 */
                    if(strandsValid)                                                                                           /* :3431 */
                    {
                        int graphDistance = eA->alignedReadPair_pairsDistanceInGraphLevels(chain_read1, chain_read2);          /* :3433 */
                        (void)graphDistance;
                        std::set<int> underlyingSequencesDistances = eA->alignedReadPair_pairsDistancesUnderlyingSequences(chain_read1, chain_read2, graphLevel_2_underlyingSequencePositions);   /* :3434 */
                        if(underlyingSequencesDistances.size())                                                                /* :3436 */
                        {
                            std::vector<double> underlyingSequenceDistances_LLs;                                               /* :3438 */
                            for(std::set<int>::iterator distanceIt = underlyingSequencesDistances.begin(); distanceIt != underlyingSequencesDistances.end(); distanceIt++)   /* :3439 */
                            {
                                int distance = *distanceIt;                                                                    /* :3441 */
                                double distance_P = boost::math::pdf(rnd_InsertSize, distance);                                /* :3446 */
                                if(distance_P <= 0)                                                                            /* :3447 */
                                    underlyingSequenceDistances_LLs.push_back(max_insertsize_penalty_log);                     /* :3458 */
                                else
                                {
                                    if(!(distance_P <= 1)) throw std::runtime_error("distance_P > 1");                         /* :3463 */
                                    underlyingSequenceDistances_LLs.push_back(log(distance_P));                                /* :3464 */
                                }
                            }
                            std::pair<double, unsigned int> best_underlyingSequenceDistances_LLs = Utilities::findVectorMax(underlyingSequenceDistances_LLs);   /* :3467 */
                            log_likelihood_insertSize = best_underlyingSequenceDistances_LLs.first;                            /* :3468 */
                        }
                        else
                            log_likelihood_insertSize = max_insertsize_penalty_log;                                            /* :3472 */
                    }
                    else
                        log_likelihood_insertSize = max_insertsize_penalty_log;                                                /* :3494 */
                    combined_log_likelihood += log_likelihood_insertSize;                                                      /* :3497 */
                    combinations_LL.push_back(combined_log_likelihood);                                                        /* :3499 */
                    combinations_indices.push_back(std::make_pair(read1_alignmentI, read2_alignmentI));                        /* :3500 */
                    combinations_LL_insertSizeOnly.push_back(log_likelihood_insertSize);                                       /* :3502 */
                }
            }

            std::pair<double, unsigned int> combinations_max = Utilities::findVectorMax(combinations_LL);                      /* :3538 */
            unsigned int maxCombination_i1 = combinations_indices.at(combinations_max.second).first;                           /* :3539 */
            unsigned int maxCombination_i2 = combinations_indices.at(combinations_max.second).second;                          /* :3540 */
            forReturn.chains.first = read1_extendedChains.at(maxCombination_i1);                                               /* :3542 */
            forReturn.chains.second = read2_extendedChains.at(maxCombination_i2);                                              /* :3543 */
            forReturn.chains.first.fromFirstRead = true;                                                                       /* :3545 */
            forReturn.chains.second.fromFirstRead = false;                                                                     /* :3546 */
            forReturn.chains.first = read1_extendedChains.at(maxCombination_i1);                                               /* :3548 */
            mapper::processBAM::assignMappingQualities(forReturn, combinations_indices, combinations_LL, combinations_max, read1_extendedChains, read2_extendedChains);   /* :3550 */

            if(out->pair_status) out->pair_status[p] = 0;
            if(out->best_chain) { out->best_chain[2 * p] = abs_index[2 * p].at(maxCombination_i1); out->best_chain[2 * p + 1] = abs_index[2 * p + 1].at(maxCombination_i2); }
            if(out->n_combinations) out->n_combinations[p] = (int)combinations_indices.size();
            if(out->pair_ll) out->pair_ll[p] = combinations_max.first;
            if(out->pair_mapq) out->pair_mapq[p] = forReturn.mapQ;
            if(out->mate_mapq) { out->mate_mapq[2 * p] = forReturn.chains.first.mapQ; out->mate_mapq[2 * p + 1] = forReturn.chains.second.mapQ; }
            if(out->strands_valid) out->strands_valid[p] = eA->alignedReadPair_strandsValid(forReturn.chains.first, forReturn.chains.second) ? 1 : 0;
            if(best_is_penalty) best_is_penalty[p] = combinations_LL_insertSizeOnly.at(combinations_max.second) == max_insertsize_penalty_log ? 1 : 0;
            for(int m = 0; m < 2; m++) {
                const verboseSeedChain& c = m ? forReturn.chains.second : forReturn.chains.first;
                int n = store_columns(h, c, (size_t)(2 * p + m), stride, out->col_level, out->col_edge, out->col_gchar, out->col_schar, out->col_fromseed, out->col_mapq);
                if(out->n_cols) out->n_cols[2 * p + m] = n;
            }
        }
        return 0;
    });
}

/* ------------------------------------------------------------------ unpaired mapping qualities: the end of processBAM::alignOneLongRead (:3768-3777)
 *
 * `in` holds finished (extended or padded) chains of n_reads reads, chains of a read next to each other, ll[c] their log-likelihoods.  Per read:
 * Utilities::findVectorMax over its log-likelihoods (:3770), the selected chain (:3772), assignMappingQualities_unpaired (:3776, :3900-4059).
 * Outputs are per read ([n] where the paired layout has [2n]); best_chain is an index into the chains of `in`; col_fromseed is not written
 * (hlala_seeds_in does not carry it). */
int ref_mapq_unpaired(ref_handle* h, const hlala_seeds_in* in, const double* ll, int n_reads, int stride, hlala_pairs_out* out)
{
    return guarded([&]() -> int {
        using mapper::reads::verboseSeedChain;
        int c = 0;
        for(int r = 0; r < n_reads; r++) {
            std::vector<verboseSeedChain> read1_extendedChains; std::vector<double> read1_extendedChains_log_likelihoods;
            const int first = c;
            for(; c < in->n_chains && in->chain_read[c] == r; c++) { read1_extendedChains.push_back(chain_from_columns(h, in, c)); read1_extendedChains_log_likelihoods.push_back(ll[c]); }
            if(!(read1_extendedChains.size() > 0)) throw std::runtime_error("a read without chains");                            /* :3768 */
            std::pair<double, unsigned int> combinations_max = Utilities::findVectorMax(read1_extendedChains_log_likelihoods);   /* :3770 */
            verboseSeedChain forReturn = read1_extendedChains.at(combinations_max.second);                                       /* :3772 */
            forReturn.fromFirstRead = true;                                                                                      /* :3774 */
            mapper::processBAM::assignMappingQualities_unpaired(forReturn, read1_extendedChains_log_likelihoods, combinations_max, read1_extendedChains);   /* :3776 */
            if(out->pair_status) out->pair_status[r] = 0;
            if(out->best_chain) out->best_chain[r] = first + (int)combinations_max.second;
            if(out->n_combinations) out->n_combinations[r] = (int)read1_extendedChains.size();
            if(out->pair_ll) out->pair_ll[r] = combinations_max.first;
            if(out->pair_mapq) out->pair_mapq[r] = forReturn.mapQ;
            if(out->mate_mapq) out->mate_mapq[r] = forReturn.mapQ;
            if(out->strands_valid) out->strands_valid[r] = 0;
            int n = store_columns(h, forReturn, (size_t)r, stride, out->col_level, out->col_edge, out->col_gchar, out->col_schar, nullptr, out->col_mapq);
            if(out->n_cols) out->n_cols[r] = n;
        }
        if(c != in->n_chains) throw std::runtime_error("chains are not grouped by read");
        return 0;
    });
}

/* ------------------------------------------------------------------ the typer: hla::HLATyper (hla/HLATyper.cpp)
 *
 * Alignments are handed over as a hlala_seeds_in whose "chains" are the selected alignments: row 2u + m for mate m of unit u of a paired
 * batch, row u for read u of an unpaired one; chain_read[c] = c, chain_reverse[c] the strand of the selected alignment, the reads as a
 * batch carries them (the bases of the primary alignment in alignment orientation).  Beside it: mapQ_perPosition packed like the columns,
 * verboseSeedChain::mapQ per row, verboseSeedChainPair::mapQ per unit, the strand of the primary alignment per row (the raw read is
 * inverted when it is reverse, mapper/processBAM.cpp:2138-2158, :2314-2325, :2452-2475) and the read names. */
typedef struct {
    int32_t n_units, paired;
    const hlala_seeds_in* rows;
    const uint8_t* col_mapq;          /* [col_off[n_rows]] */
    const double*  row_mapq;          /* [n_rows] */
    const double*  unit_mapq;         /* [n_units], paired only */
    const uint8_t* primary_reverse;   /* [n_rows] */
    const int32_t* name_off;          /* [n_rows + 1] into names */
    const char*    names;
} ref_typer_reads;

namespace {
struct TyperAccess : hla::HLATyper {
    using hla::HLATyper::HLATyper;
    using hla::HLATyper::oneReadAlignment_2_exonPositions_paired;
    using hla::HLATyper::oneReadAlignment_2_exonPositions_unpaired;
    using hla::HLATyper::alignmentFractionOK;
    using hla::HLATyper::alignmentWeightedOKFraction;
    using hla::HLATyper::removeDoublePositionsFromRead;
};
struct TyperReads {
    std::vector<mapper::reads::oneReadPair> rawPaired; std::vector<mapper::reads::verboseSeedChainPair> alignedPaired;
    std::vector<mapper::reads::oneRead> rawUnpaired; std::vector<mapper::reads::verboseSeedChain> alignedUnpaired;
};
mapper::reads::oneRead typer_raw_read(const ref_typer_reads* in, int row)
{
    const hlala_seeds_in* s = in->rows;
    std::string name(in->names + in->name_off[row], (size_t)(in->name_off[row + 1] - in->name_off[row]));
    std::string seq((const char*)s->read_bases + s->read_off[row], (size_t)(s->read_off[row + 1] - s->read_off[row]));
    std::string qual((const char*)s->read_quals + s->read_off[row], (size_t)(s->read_off[row + 1] - s->read_off[row]));
    mapper::reads::oneRead r(name, seq, qual);
    if(in->primary_reverse[row]) r.invert();
    return r;
}
mapper::reads::verboseSeedChain typer_alignment(const ref_handle* h, const ref_typer_reads* in, int row, bool fromFirstRead)
{
    const hlala_seeds_in* s = in->rows;
    if(s->chain_read[row] != row) throw std::runtime_error("typer rows: chain_read[c] != c");
    mapper::reads::verboseSeedChain c = chain_from_columns(h, s, row);
    c.fromFirstRead = fromFirstRead;
    c.mapQ = in->row_mapq[row];
    c.mapQ_perPosition.assign((const char*)in->col_mapq + s->col_off[row], (size_t)(s->col_off[row + 1] - s->col_off[row]));
    c.readID = std::string(in->names + in->name_off[row], (size_t)(in->name_off[row + 1] - in->name_off[row]));
    return c;
}
void typer_build_reads(const ref_handle* h, const ref_typer_reads* in, TyperReads& R)
{
    const int n_rows = in->paired ? 2 * in->n_units : in->n_units;
    if(in->rows->n_chains != n_rows || in->rows->n_reads != n_rows) throw std::runtime_error("typer rows: one row per mate expected");
    for(int u = 0; u < in->n_units; u++) {
        if(in->paired) {
            mapper::reads::verboseSeedChainPair P;
            P.chains.first = typer_alignment(h, in, 2 * u, true); P.chains.second = typer_alignment(h, in, 2 * u + 1, false);     /* processBAM.cpp:3545-3546 */
            P.mapQ = in->unit_mapq[u]; P.readID = P.chains.first.readID;
            R.alignedPaired.push_back(P);
            R.rawPaired.push_back(mapper::reads::oneReadPair(typer_raw_read(in, 2 * u), typer_raw_read(in, 2 * u + 1), 0));
        } else {
            R.alignedUnpaired.push_back(typer_alignment(h, in, u, true));                                                         /* processBAM.cpp:3774 */
            R.rawUnpaired.push_back(typer_raw_read(in, u));
        }
    }
}
}  // namespace

/* HLATyper.cpp:28, :30: the thresholds of the pair test are globals of the reference */
extern double min_bothReads_weightedCharactersOK;
extern double minimumMappingQuality;

struct ref_typer { ref_handle* h = nullptr; TyperAccess* T = nullptr; };

/* HLATyper(Graph*, graphDir, ""): reads graph_dir/PRG/segments.txt and the segment files; with an empty quality-matrix name no read simulator is built */
ref_typer* ref_typer_create(ref_handle* h, const char* graph_dir)
{
    ref_typer* t = new ref_typer(); t->h = h;
    int rc = guarded([&]() -> int { t->T = new TyperAccess(h->g, std::string(graph_dir), std::string("")); return 0; });
    if(rc != 0) { delete t; return nullptr; }
    return t;
}

void ref_typer_destroy(ref_typer* t)
{
    if(!t) return;
    delete t->T; delete t;
}

/* HLATyper::intervalOverlapsWithGenes for n (first, last) level pairs: one call of the includeInHLA decision (processBAM.cpp:2114-2133, :2298-2312, :2428-2448) */
int ref_typer_include(ref_typer* t, int n, const int32_t* first, const int32_t* last, uint8_t* overlaps)
{
    return guarded([&]() -> int {
        for(int i = 0; i < n; i++) overlaps[i] = t->T->intervalOverlapsWithGenes(first[i], last[i]) ? 1 : 0;
        return 0;
    });
}

/* The two read loops at the head of the per-locus part of HLATypeInference (:1386-1464 paired, :1467-1495 unpaired) around the reference's
 * oneReadAlignment_2_exonPositions_paired / _unpaired, alignmentWeightedOKFraction, alignedReadPair_strandsValid / _pairsDistanceInGraphLevels and
 * removeDoublePositionsFromRead.  `locus` gives combined_exon_sequences_graphLevels_min / _max and graphLevel_2_exonPosition (level_to_exon), the
 * insert size and, for unpaired batches, minAlignmentLength_unpaired (a local constant of the reference, :1032); the two thresholds of the pair
 * test are the reference's globals.  Output in the layout of hlala_exon_positions: one entry per element of exonPositions_fromReads.  The
 * per-mate arrays are filled from the oneExonPosition fields of the entry's positions (thisRead_* of the position's own mate, pairedRead_* of the
 * other); a field no position of the entry witnesses stays at -1 (read_reverse: 255), and two positions of an entry that disagree about a
 * per-mate field fail the call.  pos_mapq_p (may be NULL) takes oneExonPosition::mapQ_position. */
int ref_typer_exon_positions(ref_typer* t, const ref_typer_reads* in, const hlala_locus_desc* locus, hlala_exon_positions_out* o, double* pos_mapq_p)
{
    return guarded([&]() -> int {
        using hla::oneExonPosition;
        TyperReads R; typer_build_reads(t->h, in, R);
        const std::vector<mapper::reads::verboseSeedChainPair>& alignments_paired = R.alignedPaired;
        const std::vector<mapper::reads::verboseSeedChain>& alignments_unpaired = R.alignedUnpaired;
        const std::vector<mapper::reads::oneReadPair>& alignments_originalReads_paired = R.rawPaired;
        const std::vector<mapper::reads::oneRead>& alignments_originalReads_unpaired = R.rawUnpaired;
        const double insertSize_mean = locus->insert_mean, insertSize_sd = locus->insert_sd;
        const int minAlignmentLength_unpaired = locus->min_alignment_columns;
        int combined_exon_sequences_graphLevels_min = locus->level_min, combined_exon_sequences_graphLevels_max = locus->level_max;
        std::map<int, unsigned int> graphLevel_2_exonPosition;
        for(int l = locus->level_min; l <= locus->level_max; l++) if(locus->level_to_exon[l - locus->level_min] >= 0) graphLevel_2_exonPosition[l] = (unsigned int)locus->level_to_exon[l - locus->level_min];

        std::vector<std::vector<oneExonPosition>> exonPositions_fromReads; std::vector<int> entry_unit;
        unsigned int readPairs_OK = 0, readPairs_broken = 0;
        for(unsigned int readPairI = 0; readPairI < alignments_paired.size(); readPairI++)                                     /* :1386 */
        {
            const mapper::reads::oneReadPair& originalReadPair = alignments_originalReads_paired.at(readPairI);
            const mapper::reads::verboseSeedChainPair& alignedReadPair = alignments_paired.at(readPairI);
            std::vector<oneExonPosition> read1_exonPositions, read2_exonPositions;
            t->T->oneReadAlignment_2_exonPositions_paired(alignedReadPair.chains.first, originalReadPair.reads.first, read1_exonPositions, alignedReadPair.chains.second, originalReadPair.reads.second, 1, combined_exon_sequences_graphLevels_min, combined_exon_sequences_graphLevels_max, graphLevel_2_exonPosition);   /* :1394 */
            t->T->oneReadAlignment_2_exonPositions_paired(alignedReadPair.chains.second, originalReadPair.reads.second, read2_exonPositions, alignedReadPair.chains.first, originalReadPair.reads.first, 2, combined_exon_sequences_graphLevels_min, combined_exon_sequences_graphLevels_max, graphLevel_2_exonPosition);   /* :1395 */
            if(!((alignedReadPair.chains.first.mapQ >= 0) && (alignedReadPair.chains.first.mapQ <= 1))) throw std::runtime_error("chains.first.mapQ outside [0, 1]");   /* :1403 */
            double mapQ_thisAlignment = alignedReadPair.chains.first.mapQ;                                                     /* :1404 */
            if(mapper::aligner::alignerBase::alignedReadPair_strandsValid(alignedReadPair) &&
               (abs(mapper::aligner::alignerBase::alignedReadPair_pairsDistanceInGraphLevels(alignedReadPair) - insertSize_mean) <= (5 * insertSize_sd)) &&
               (mapQ_thisAlignment >= minimumMappingQuality) &&
               ((TyperAccess::alignmentWeightedOKFraction(originalReadPair.reads.first, alignedReadPair.chains.first) >= min_bothReads_weightedCharactersOK) && (TyperAccess::alignmentWeightedOKFraction(originalReadPair.reads.second, alignedReadPair.chains.second) >= min_bothReads_weightedCharactersOK)))   /* :1405-1410 */
            {
                std::vector<oneExonPosition> thisRead_exonPositions = read1_exonPositions;                                     /* :1415 */
                thisRead_exonPositions.insert(thisRead_exonPositions.end(), read2_exonPositions.begin(), read2_exonPositions.end());   /* :1416 */
                if(thisRead_exonPositions.size() > 0)                                                                          /* :1418 */
                {
                    thisRead_exonPositions = TyperAccess::removeDoublePositionsFromRead(thisRead_exonPositions);               /* :1420 */
                    exonPositions_fromReads.push_back(thisRead_exonPositions); entry_unit.push_back((int)readPairI);           /* :1421 */
                }
                readPairs_OK++;                                                                                                /* :1424 */
            }
            else
                readPairs_broken++;                                                                                            /* :1462 */
        }
        for(unsigned int readI = 0; readI < alignments_unpaired.size(); readI++)                                               /* :1467 */
        {
            const mapper::reads::oneRead& originalRead = alignments_originalReads_unpaired.at(readI);
            const mapper::reads::verboseSeedChain& alignedRead = alignments_unpaired.at(readI);
            std::vector<oneExonPosition> read_exonPositions;
            t->T->oneReadAlignment_2_exonPositions_unpaired(alignedRead, originalRead, read_exonPositions, combined_exon_sequences_graphLevels_min, combined_exon_sequences_graphLevels_max, graphLevel_2_exonPosition);   /* :1473 */
            double mapQ_thisAlignment = alignedRead.mapQ;                                                                      /* :1475 */
            if((mapQ_thisAlignment >= minimumMappingQuality) && ((int)alignedRead.graph_aligned.size() >= minAlignmentLength_unpaired))   /* :1476 */
            {
                if(read_exonPositions.size() > 0) { exonPositions_fromReads.push_back(read_exonPositions); entry_unit.push_back((int)readI); }   /* :1481-1485 */
                readPairs_OK++;                                                                                                /* :1486 */
            }
            else
                readPairs_broken++;                                                                                            /* :1493 */
        }

        /* ---- copy out */
        o->n_pairs_ok = (int)readPairs_OK; o->n_pairs_broken = (int)readPairs_broken;
        size_t nPos = 0, nChars = 0;
        for(const auto& e : exonPositions_fromReads) { nPos += e.size(); for(const auto& p : e) nChars += p.genotype.size(); }
        o->n_reads = (int)exonPositions_fromReads.size(); o->n_pos = (int)nPos; o->n_chars = (int)nChars;
        if(o->n_reads > o->cap_reads || o->n_pos > o->cap_pos || o->n_chars > o->cap_chars) throw std::runtime_error("exon positions: output capacity too small");
        auto witness = [](double& slot, double v, const char* what) {
            if(slot == -1) slot = v;
            else if(!(slot == v)) throw std::runtime_error(std::string("positions of one entry disagree about ") + what);
        };
        int q = 0, ch = 0;
        for(size_t i = 0; i < exonPositions_fromReads.size(); i++) {
            o->read_pair[i] = entry_unit[i]; o->pos_off[i] = q;
            double wok[2] = {-1, -1}, fok[2] = {-1, -1}, mq[2] = {-1, -1}, rev[2] = {-1, -1}, cng[2] = {-1, -1}, dist = -1;
            bool have_dist = false;
            for(const oneExonPosition& p : exonPositions_fromReads[i]) {
                const int m = p.fromFirstRead ? 0 : 1;
                if(!in->paired && m != 0) throw std::runtime_error("an unpaired position that is not fromFirstRead");
                witness(wok[m], p.thisRead_WeightedCharactersOK, "thisRead_WeightedCharactersOK"); witness(fok[m], p.thisRead_fractionOK, "thisRead_fractionOK");
                if(in->paired) { witness(wok[1 - m], p.pairedRead_WeightedCharactersOK, "pairedRead_WeightedCharactersOK"); witness(fok[1 - m], p.pairedRead_fractionOK, "pairedRead_fractionOK"); }
                else if(!(p.pairedRead_WeightedCharactersOK == -1 && p.pairedRead_fractionOK == -1)) throw std::runtime_error("pairedRead_* of an unpaired position is not -1");
                if(!(p.mapQ == p.mapQ_genomic)) throw std::runtime_error("mapQ != mapQ_genomic");
                witness(mq[m], p.mapQ, "mapQ"); witness(rev[m], p.reverse ? 1 : 0, "reverse"); witness(cng[m], p.alignmentColumnsWithAtLeastOneNonGap, "alignmentColumnsWithAtLeastOneNonGap");
                if(have_dist && !(dist == p.pairs_strands_distance)) throw std::runtime_error("positions of one entry disagree about pairs_strands_distance");
                dist = p.pairs_strands_distance; have_dist = true;
                if(in->paired && !p.pairs_strands_OK) throw std::runtime_error("a position of a pair whose strands are not valid");
                o->pos_exon[q] = (int32_t)p.positionInExon; o->pos_level[q] = p.graphLevel; o->pos_mate[q] = (uint8_t)(m + 1);
                o->pos_novel_gap[q] = p.runningNovelGapEitherDirection;
                if(pos_mapq_p) pos_mapq_p[q] = p.mapQ_position;
                o->pos_mapq[q] = 0;                                /* the Phred character is an input of the caller; the reference keeps its translation (pos_mapq_p) */
                o->geno_off[q] = ch;
                if(!(p.genotype == "_" ? p.qualities.size() == 0 : p.qualities.size() == p.genotype.size())) throw std::runtime_error("genotype and qualities of unequal length");
                for(size_t k = 0; k < p.genotype.size(); k++) { o->geno_chars[ch] = (uint8_t)p.genotype[k]; o->qual_chars[ch] = k < p.qualities.size() ? (uint8_t)p.qualities[k] : 0; ch++; }
                q++;
            }
            if(dist != (double)(int32_t)dist) throw std::runtime_error("pairs_strands_distance is not an integer");
            for(int m = 0; m < 2; m++) {
                o->read_weighted_ok[2 * i + m] = wok[m]; o->read_fraction_ok[2 * i + m] = fok[m]; o->read_cols_nongap[2 * i + m] = (int32_t)cng[m];
                if(o->read_mapq) o->read_mapq[2 * i + m] = mq[m];
                if(o->read_reverse) o->read_reverse[2 * i + m] = rev[m] < 0 ? 255 : (uint8_t)rev[m];
            }
            o->read_distance[i] = (int32_t)dist;
        }
        o->pos_off[exonPositions_fromReads.size()] = q; o->geno_off[q] = ch;
        return 0;
    });
}

/* HLATyper::HLATypeInference on the alignments of `in`, writing its files into out_dir.  read_G_alleles opens "hla_nom_g.txt" in the
 * current directory: the call runs with g_dir (a directory that holds that file) as the working directory and restores the old one.
 * The all-pairs loop appends per-thread results inside a critical section, so with more than one OpenMP thread the order of
 * LLs_completeReads -- which findVectorMax, the sort on ties and findIntMapMax see -- depends on thread timing: the call runs with one. */
int ref_typer_infer(ref_typer* t, const ref_typer_reads* in, double insert_mean, double insert_sd, const char* out_dir, const char* long_reads_mode, const char* g_dir)
{
    char cwd[4096];
    if(!getcwd(cwd, sizeof(cwd))) { g_err = "getcwd failed"; return -1; }
    if(chdir(g_dir) != 0) { g_err = std::string("cannot change into ") + g_dir; return -1; }
    const int threads = omp_get_max_threads();
    omp_set_num_threads(1);
    int rc = guarded([&]() -> int {
        TyperReads R; typer_build_reads(t->h, in, R);
        t->T->HLATypeInference(R.rawPaired, R.alignedPaired, R.rawUnpaired, R.alignedUnpaired, insert_mean, insert_sd, std::string(out_dir), std::string(long_reads_mode));
        return 0;
    });
    omp_set_num_threads(threads);
    if(chdir(cwd) != 0 && rc == 0) { g_err = std::string("cannot change back into ") + cwd; rc = -1; }
    return rc;
}
}  // extern "C"

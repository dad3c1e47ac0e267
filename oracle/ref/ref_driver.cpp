/* C ABI over the reference aligner (mapper::aligner::extensionAligner of HLA*LA), linked from the reference's own
 * sources by oracle/ref/Makefile into oracle/_ref/libhlala_ref.so.  Test infrastructure: the referee of
 * oracle/hlala_oracle.cpp and, through the fixtures it writes, of the HIP kernels.  Nothing here restates the aligner;
 * this file only builds its inputs, calls it and copies its outputs.
 *
 * Order is pointer order in the reference (std::set<Node*>, std::set<Edge*>, std::map<Node*, ...>): all nodes live in
 * one array and all edges in one array, in the order of the graph description, so that pointer order is index order
 * and an Edge* turns back into an index by subtraction. */
#include "mapper/aligner/extensionAligner.h"
#include "mapper/reads/oneRead.h"
#include "mapper/reads/verboseSeedChain.h"
#include "Graph/Graph.h"
#include "Graph/Node.h"
#include "Graph/Edge.h"

#include "hlala_gpu.h"

#include <csetjmp>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <stdexcept>
#include <string>

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
        using mapper::reads::verboseSeedChain;
        mapper::aligner::extensionAligner& A = *h->A;
        for(int c = 0; c < in->n_chains; c++) {
            int r = in->chain_read[c];
            std::string seq((const char*)in->read_bases + in->read_off[r], in->read_off[r + 1] - in->read_off[r]);
            std::string qual((const char*)in->read_quals + in->read_off[r], in->read_off[r + 1] - in->read_off[r]);
            verboseSeedChain s;
            s.sequence_begin = in->chain_seq_begin[c]; s.sequence_end = in->chain_seq_end[c]; s.reverse = in->chain_reverse[c] != 0;
            for(int j = in->col_off[c]; j < in->col_off[c + 1]; j++) {
                int e = in->col_edge[j];
                if(e < -1 || e >= h->n_edges) throw std::runtime_error("seed edge out of range");
                s.graph_aligned_levels.push_back(in->col_level[j]); s.graph_aligned_edges.push_back(e < 0 ? nullptr : &h->edges[e]);
                s.graph_aligned.push_back((char)in->col_gchar[j]); s.sequence_aligned.push_back((char)in->col_schar[j]);
                s.is_from_BWAseed.push_back(true);
            }
            const unsigned seedL = rng_seed + 2u * (unsigned)c, seedR = seedL + 1u;
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
            double ll = A.scoreOneAlignment(e, rd, long_read_mode ? "longReads" : "");

            int n = (int)e.graph_aligned_levels.size();
            if(n > stride) throw std::runtime_error("more alignment columns than the output stride");
            if((int)e.graph_aligned_edges.size() != n || (int)e.graph_aligned.size() != n || (int)e.sequence_aligned.size() != n || (int)e.is_from_BWAseed.size() != n)
                throw std::runtime_error("reference chain rows of unequal length");
            if(out->status) out->status[c] = HLALA_CHAIN_OK;
            if(out->n_cols) out->n_cols[c] = n;
            if(out->seq_begin) out->seq_begin[c] = e.sequence_begin;
            if(out->seq_end) out->seq_end[c] = e.sequence_end;
            if(out->ll) out->ll[c] = ll;
            size_t base = (size_t)c * stride;
            for(int j = 0; j < n; j++) {
                int ei = h->edge_index(e.graph_aligned_edges[j]);
                if(out->col_level) out->col_level[base + j] = e.graph_aligned_levels[j];
                if(out->col_edge) out->col_edge[base + j] = ei;
                if(out->col_gchar) out->col_gchar[base + j] = (uint8_t)e.graph_aligned[j];
                if(out->col_schar) out->col_schar[base + j] = (uint8_t)e.sequence_aligned[j];
                if(out->col_fromseed) out->col_fromseed[base + j] = e.is_from_BWAseed[j] ? 1 : 0;
            }
        }
        return 0;
    });
}

}  // extern "C"

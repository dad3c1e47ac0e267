// kernel_pair_overflow.hip -- stage C for the pairs beyond the capacities of kernel_pair.hip (more than PAIR_CHAINS kept chains on a mate, more than PAIR_COMB
// combinations, several combinations and a chain of more than PAIR_COLS columns).  Opt-in (hlala_set_pair_overflow): k_pair_chains lists such a pair in the third
// list of its pass instead of refusing it, k_pair_overflow runs that list behind k_pair_multi<., true>.
// One wavefront per pair; everything whose size follows the pair lives in the wave's slab in HBM, so nothing here is bounded but by the slab.  Written for
// rare pairs: the arithmetic, its order and the tie rules are those of pair_finish / pair_positions, operation for operation -- a pair inside the capacities
// would come out of this kernel with the bytes k_pair_multi gives it --, the speed is whatever that leaves.
//
// The slab of a pair with n1 x n2 kept chains (unpaired: n2 = 1, no second list) in a batch of column stride S = max_columns, W = ceil(max(n1, n2) / 64):
//   double chainLL[nc]        log likelihood of the k-th chain of list 1, then of list 2 (nc = n1 + n2; unpaired: n1)
//   double LL[n1 * n2]        combination table, row-major (i1, i2)
//   u64    mask[S][W]         per column of the selected chain: bit k = chain k of the mate's list shares it
//   int    fact[nc][8]        first, second, last, second-last level, strand, columns, column row, chain number
//   int    ord[S]             read-base ordinal of a selected column (-1: a gap column)
//   int    baseLev[S]         compared chain, by read-base ordinal: relative level (OV_NOCOL / OV_NOLEVEL)
//   u8     baseG[S], levS[S], levG[S]     ... its graph character; by relative level: read and graph character
// = 40 nc + 8 n1 n2 + 8 S W + 11 S bytes: hlala_pair_overflow_need (include/hlala_gpu.h states the same formula).
#include "batch.h"
#include "../../include/hlala_gpu.h"

namespace hlala {

constexpr int PAIR_OVER_WAVES = HLALA_PAIR_OVERFLOW_WAVES / 2;      // blocks (of one wave) of k_pair_overflow per pass
constexpr int OV_NOCOL = -2147483647 - 1;       // no base column with this ordinal
constexpr int OV_NOLEVEL = -2147483647;         // the column carries no level (stored relative levels are >= 0)

__host__ __device__ inline long long pair_overflow_need(long long n1, long long n2, long long S, bool unpaired)
{
    if(unpaired) n2 = 1;
    const long long nc = unpaired ? n1 : n1 + n2, W = ((n1 > n2 ? n1 : n2) + 63) / 64;
    return 40 * nc + 8 * n1 * n2 + 8 * S * W + 11 * S;
}

// what one lane stored to the slab, another lane of the wave reads: stores out, wave together, loads fresh (as kernel_inflate.hip orders the bytes it reads back)
__device__ __forceinline__ void overflow_fence()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
}
__device__ __forceinline__ double overflow_lane0(double v)
{
    const long long b = __double_as_longlong(v);
    return __longlong_as_double((long long)(((u64)(u32)__builtin_amdgcn_readfirstlane((int)(b >> 32)) << 32) | (u64)(u32)__builtin_amdgcn_readfirstlane((int)b)));
}

// One pair that fits the slab: lists, combination table, first maximum, posteriors, outputs, per-position pass.  Called by the whole wave with wave-uniform arguments.
template <bool UNPAIRED, class DG, class DB>
__device__ __forceinline__ void pair_overflow_score(const DG& G, const DevTables& T, const DB& B, const PairLds& P, char* const slab, const int p, const int* cLo, const int* cHi,
                                                    const int n1, const int n2, const int lane, const int stride, const unsigned char ph1)
{
    constexpr int NM = UNPAIRED ? 1 : 2;
    const int nComb = n1 * n2, nc = UNPAIRED ? n1 : n1 + n2, W = (max(n1, n2) + 63) >> 6;
    double* const chainLL = (double*)slab;
    double* const LL = chainLL + nc;
    u64* const mask = (u64*)(LL + nComb);
    int* const fact = (int*)(mask + (size_t)stride * W);
    int* const ord = fact + 8 * (size_t)nc;
    int* const baseLev = ord + stride;
    unsigned char* const baseG = (unsigned char*)(baseLev + stride);
    unsigned char* const levS = baseG + stride;
    unsigned char* const levG = levS + stride;
    // ---- the lists, and the facts of the listed chains in list order (PairChain)
    #pragma unroll
    for(int m = 0; m < NM; m++) {
        int cnt = m ? n1 : 0;
        for(int b0 = cLo[m]; b0 < cHi[m]; b0 += 64) {
            const int c = b0 + lane; int st = 1;
            if(c < cHi[m]) st = B.ext_status[c];
            const u64 okm = __ballot(st == HLALA_CHAIN_OK);
            if(st == HLALA_CHAIN_OK) {
                const int k = cnt + __popcll(okm & ((1ull << lane) - 1ull));
                const PairChain x = pair_chain_load(B, c);
                chainLL[k] = x.ll;
                int* f = fact + 8 * (size_t)k;
                f[0] = x.fl.x; f[1] = x.fl.y; f[2] = x.fl.z; f[3] = x.fl.w; f[4] = x.rev; f[5] = x.nk; f[6] = x.row; f[7] = c;
            }
            cnt += __popcll(okm);
        }
    }
    overflow_fence();
    const int* const factB = UNPAIRED ? fact : fact + 8 * (size_t)n1;
    const double* const chainLLB = UNPAIRED ? chainLL : chainLL + n1;
    // ---- combination log likelihoods, row-major (i1, i2) (:3408-3506): ll1 + ll2, then + llIS
    if(UNPAIRED) { for(int i = lane; i < nComb; i += 64) LL[i] = chainLL[i]; }
    else {
        for(int i1 = 0; i1 < n1; i1++) {
            const int* fa = fact + 8 * (size_t)i1;
            const int fa0 = uni(fa[0]), fa1 = uni(fa[1]), fa2 = uni(fa[2]), fa3 = uni(fa[3]); const bool ra = uni(fa[4]) != 0;
            const double lA = overflow_lane0(chainLL[i1]);
            for(int i2 = 0; i2 < n2; i2++) {
                const int* fb = factB + 8 * (size_t)i2;
                const int fb0 = uni(fb[0]), fb1 = uni(fb[1]), fb2 = uni(fb[2]), fb3 = uni(fb[3]); const bool rb = uni(fb[4]) != 0;
                bool valid = false;
                if(fa0 != -1 && fb0 != -1 && ra != rb) valid = (!ra) ? (fa0 < fb0) : (fa2 > fb2);          // alignerBase.cpp:213-244
                double llIS = T.is_penalty;
                if(valid) llIS = (fa0 < fb0) ? pair_insert_ll(G, T, fa2, fa3, fb0, fb1) : pair_insert_ll(G, T, fb2, fb3, fa0, fa1);        // alignerBase.cpp:294, 312
                double combined = lA + overflow_lane0(chainLLB[i2]);
                combined += llIS;
                if(lane == 0) LL[(size_t)i1 * n2 + i2] = combined;
            }
        }
    }
    overflow_fence();
    // ---- first maximum (Utilities::findVectorMax, Utilities.cpp:309-323): the lowest index among equal values
    double mx = -1.0e300; int mi = 0x7FFFFFFF;
    for(int i = lane; i < nComb; i += 64) { const double v = LL[i]; if(v > mx) { mx = v; mi = i; } }
    for(int o = 32; o; o >>= 1) { const double ov = __shfl_xor(mx, o); const int oi = __shfl_xor(mi, o); if(ov > mx || (ov == mx && oi < mi)) { mx = ov; mi = oi; } }
    const int bestI = uni(mi), best1 = bestI / n2, best2 = bestI % n2;
    const int selA = uni(fact[8 * (size_t)best1 + 7]), selB = UNPAIRED ? selA : uni(factB[8 * (size_t)best2 + 7]);
    // ---- posterior over combinations (:4064-4085): exp(LL - max), normalised by a left-to-right sum; the marginals are left-to-right sums as well
    double mapQ = 1, q1 = 1, q2 = 1;
    if(nComb > 1) {
        for(int i = lane; i < nComb; i += 64) LL[i] = exp_cr_nonpos(LL[i] - mx);
        overflow_fence();
        double S = 0;
        if(lane == 0) { for(int i = 0; i < nComb; i++) S += LL[i]; }
        S = overflow_lane0(S);
        overflow_fence();
        for(int i = lane; i < nComb; i += 64) LL[i] = LL[i] / S;
        overflow_fence();
        double a = 0, b = 0;
        if(lane == 0) {
            int i1 = 0, i2 = 0;
            for(int i = 0; i < nComb; i++) { const double pp = LL[i]; if(i1 == best1) a += pp; if(i2 == best2) b += pp; if(++i2 == n2) { i2 = 0; i1++; } }
            if(a > 1) a = 1; if(b > 1) b = 1;
        }
        q1 = overflow_lane0(a); q2 = overflow_lane0(b);
        mapQ = overflow_lane0(LL[bestI]);
    }
    bool svalid = false;
    if(!UNPAIRED) {          // alignedReadPair_strandsValid of the selected chains (alignerBase.cpp:213-244)
        const int* fa = fact + 8 * (size_t)best1; const int* fb = factB + 8 * (size_t)best2;
        const int fa0 = uni(fa[0]), fa2 = uni(fa[2]), fb0 = uni(fb[0]), fb2 = uni(fb[2]); const bool ra = uni(fa[4]) != 0, rb = uni(fb[4]) != 0;
        if(fa0 != -1 && fb0 != -1 && ra != rb) svalid = (!ra) ? (fa0 < fb0) : (fa2 > fb2);
    }
    if(lane == 0) {
        B.pair_status[p] = 0; B.n_comb[p] = nComb; B.pair_ll[p] = mx; B.pair_mapq[p] = mapQ;
        if(UNPAIRED) { B.best_chain[p] = selA; B.mate_mapq[p] = mapQ; B.strands_valid[p] = 0; }                       // forReturn.mapQ = mapQ, :3921
        else {
            B.best_chain[2 * p] = selA; B.best_chain[2 * p + 1] = selB; B.mate_mapq[2 * p] = q1; B.mate_mapq[2 * p + 1] = q2;
            B.strands_valid[p] = svalid ? 1 : 0;
        }
    }
    // ---- per-position mapping quality of the selected chains (:4155-4311; pair_positions with its tables in the slab and 32-bit entries)
    for(int m = 0; m < NM; m++) {
        const int r = UNPAIRED ? p : 2 * p + m;
        const int nl = m ? n2 : n1, kSel = m ? best2 : best1;
        const int* const factM = m ? factB : fact;
        const int nSel = uni(factM[8 * (size_t)kSel + 5]); const size_t sb = (size_t)uni(factM[8 * (size_t)kSel + 6]) * (size_t)stride; const size_t ob = (size_t)r * stride;
        if(nComb == 1) { for(int j = lane; j < nSel; j += 64) B.sel_mapq[ob + j] = ph1; continue; }
        const int Wm = (nl + 63) >> 6;
        // read-base ordinal of each selected column (alignment orientation; strand is shared by all chains of the mate); no chain shares a column yet
        {
            int carry = 0;
            for(int j0 = 0; j0 < nSel; j0 += 64) {
                const int j = j0 + lane; const bool isBase = j < nSel && B.ext_s[sb + j] != '_';
                const u64 bm = __ballot(isBase);
                if(j < nSel) ord[j] = isBase ? carry + __popcll(bm & ((1ull << lane) - 1ull)) : -1;
                carry += __popcll(bm);
            }
            for(int j = lane; j < nSel; j += 64) for(int w = 0; w < Wm; w++) mask[(size_t)j * Wm + w] = 0;
        }
        for(int k = 0; k < nl; k++) {
            if(k == kSel) {
                // the selected chain agrees with itself in every column
                for(int j = lane; j < nSel; j += 64) mask[(size_t)j * Wm + (k >> 6)] |= (1ull << (k & 63));
                continue;
            }
            const int nk = uni(factM[8 * (size_t)k + 5]), firstK = uni(factM[8 * (size_t)k + 0]);
            const size_t kb = (size_t)uni(factM[8 * (size_t)k + 6]) * (size_t)stride;
            overflow_fence();
            for(int i = lane; i < stride; i += 64) { baseLev[i] = OV_NOCOL; levS[i] = 0; }
            overflow_fence();
            int carry = 0;
            for(int j0 = 0; j0 < nk; j0 += 64) {
                const int j = j0 + lane; const bool act = j < nk;
                unsigned char ks = 0, kg = 0; int kl = -1;
                if(act) { ks = B.ext_s[kb + j]; kg = B.ext_g[kb + j]; kl = B.ext_level[kb + j]; }
                const bool isBase = act && ks != '_';
                const u64 bm = __ballot(isBase);
                const int rel = kl == -1 ? OV_NOLEVEL : kl - firstK;          // (firstK is the first defined level: rel >= 0 for a defined level)
                if(isBase) { const int bi = carry + __popcll(bm & ((1ull << lane) - 1ull)); if(bi < stride) { baseLev[bi] = rel; baseG[bi] = kg; } }
                carry += __popcll(bm);
                if(act && kl != -1 && firstK >= 0 && rel >= 0 && rel < stride) { levS[rel] = ks; levG[rel] = kg; }
            }
            overflow_fence();
            for(int j = lane; j < nSel; j += 64) {
                const int lj = B.ext_level[sb + j]; const unsigned char gj = B.ext_g[sb + j]; const int myIdx = ord[j];
                bool hit = false;
                if(myIdx >= 0) {
                    // the other chain's column of the same read base: same level (or both none) and same graph character
                    const int bl = myIdx < stride ? baseLev[myIdx] : OV_NOCOL;
                    if(bl != OV_NOCOL) {
                        if(lj == -1) hit = bl == OV_NOLEVEL && baseG[myIdx] == gj;
                        else { const long long want = (long long)lj - firstK; hit = want >= 0 && (long long)bl == want && baseG[myIdx] == gj; }
                    }
                }
                else if(lj != -1 && firstK >= 0) { const long long li = (long long)lj - firstK; if(li >= 0 && li < stride) hit = (levS[li] == '_') && (levG[li] == gj); }
                if(hit) mask[(size_t)j * Wm + (k >> 6)] |= (1ull << (k & 63));
            }
        }
        overflow_fence();
        for(int j = lane; j < nSel; j += 64) {
            const u64* const mj = mask + (size_t)j * Wm;
            double Q = 0;                                   // alignmentPositionConfidences accumulated in combination order
            if(m == 0) { for(int i1 = 0; i1 < n1; i1++) if(mj[i1 >> 6] & (1ull << (i1 & 63))) { const double* row = LL + (size_t)i1 * n2; for(int i2 = 0; i2 < n2; i2++) Q += row[i2]; } }
            else       { for(int i1 = 0; i1 < n1; i1++) { const double* row = LL + (size_t)i1 * n2; for(int i2 = 0; i2 < n2; i2++) if(mj[i2 >> 6] & (1ull << (i2 & 63))) Q += row[i2]; } }
            if(Q > 1) Q = 1;
            B.sel_mapq[ob + j] = pair_phred(P, Q);
        }
    }
}

// ovBase: first of the four work counters of this pass's overflow list (listed, fetched, scored, refused for want of slab); ovList: [n_pairs] pair numbers
template <bool UNPAIRED>
__global__ __launch_bounds__(64) void k_pair_overflow(const DevGraph* __restrict__ Gp, const DevTables* __restrict__ Tp, const DevBatch* __restrict__ Bp,
                                                      const int* __restrict__ ovList, const int ovBase, char* __restrict__ slabs, const long long slabBytes)
{
    const DevGraph& G = *Gp;
    const DevBatch& B = *Bp;
    const DevTables& T = *Tp;
    __shared__ PairLds P;                          // (the threshold table of pair_phred; the lists and tables of this kernel are in the slab)
    const int lane = lane_id();
    const int stride = B.stride;
    constexpr int NM = UNPAIRED ? 1 : 2;
    const int nList = uni(B.work_counter[ovBase]);
    if(nList <= 0) return;
    for(int i = lane; i < 256; i += 64) P.phredThr[i] = T.phred_thr[i];
    WSYNC();
    const unsigned char ph1 = pair_phred(P, 1.0);
    char* const slab = slabs + (size_t)blockIdx.x * (size_t)slabBytes;
    for(;;) {
        int q = 0;
        if(lane == 0) q = atomicAdd(&B.work_counter[ovBase + 1], 1);
        q = __builtin_amdgcn_readfirstlane(q);
        if(q >= nList) break;
        const int p = uni(ovList[q]);
        int cLo[NM], cHi[NM], nk_[2] = {0, 1};
        #pragma unroll
        for(int m = 0; m < NM; m++) { cLo[m] = uni(B.chain_off[NM * p + m]); cHi[m] = uni(B.chain_off[NM * p + m + 1]); }
        // ---- how many chains each mate keeps (read1_extendedChains / read2_extendedChains, :3408-3420); a flagged chain or an empty list: refused, as everywhere
        int bad = 0;
        #pragma unroll
        for(int m = 0; m < NM; m++) {
            int cnt = 0;
            for(int b0 = cLo[m]; b0 < cHi[m]; b0 += 64) {
                const int c = b0 + lane; int st = 1;
                if(c < cHi[m]) st = B.ext_status[c];
                if(__ballot(st < 0)) bad = 1;
                cnt += __popcll(__ballot(st == HLALA_CHAIN_OK));
            }
            if(cnt < 1) bad = 1;
            nk_[m] = cnt;
        }
        const int n1 = nk_[0], n2 = UNPAIRED ? 1 : nk_[1];
        const long long nCombLL = (long long)n1 * n2;
        if(nCombLL > 0x7FFFFFFFll) bad = 1;
        const bool fits = !bad && pair_overflow_need(n1, n2, stride, UNPAIRED) <= slabBytes;
        // (no `continue` on the refusal: behind one, the compiler threads `if(lane == 0)` of the refusal into `if(lane == 0)` of the next draw and sends the other 63 lanes
        //  round on their own with q = 0 -- both paths meet at the fence below, as the paths of k_pair_chains meet at its WSYNC)
        if(!fits) {
            if(lane == 0) {
                B.pair_status[p] = -1; if(UNPAIRED) B.best_chain[p] = -1; else { B.best_chain[2 * p] = -1; B.best_chain[2 * p + 1] = -1; } B.n_comb[p] = 0;
                if(!bad) atomicAdd(&B.work_counter[ovBase + 3], 1);
            }
        } else {
            pair_overflow_score<UNPAIRED>(G, T, B, P, slab, p, cLo, cHi, n1, n2, lane, stride, ph1);
            if(lane == 0) atomicAdd(&B.work_counter[ovBase + 2], 1);
        }
        overflow_fence();
    }
}

}  // namespace hlala

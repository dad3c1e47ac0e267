// kernel_bamfill.hip -- the layout and the fill of a seed batch on the device (include/hlala_gpu.h: hlala_bam_fill_create / _window; the rules are bam_fill_core.h, which
// the host runs as a model).  The sample stays resident: descriptors, the bytes they point into, optionally the grouping permutation (descriptor i of the grouped order
// is recs[perm[i]]), first record and count of every unit.
//   k_fil_append   (decoder) a round's descriptors behind the sample's, their rec_off moved by where the round's compact bytes were put
//   k_fil_rank     a 16-lane group per read, one alignment of the mate per lane: the lanes find their records by two ballots over the unit's (at most 32) records, then
//                  every lane counts over 16 lane exchanges the alignments that stand before its own (fil_before: greater AS, or equal AS and later in the file) -- its
//                  rank -- and the CIGAR operations they hold; the first primary is the primary lane no other primary stands before.  Writes per read l_seq of the
//                  primary, the chain count and the CIGAR count, per unit the name length + 1.  Nothing is held in an indexed private array.
//   k_fil_host     the sizes of host units, which the host has computed, into place
//   (four hipcub::DeviceScan::ExclusiveSum: read_off, chain_off, cigar_count, name_off)
//   k_fil_src      k_fil_rank's exchanges again behind the scans: chain_src[chain] (descriptor) and chain_cig[chain] (where its CIGAR starts), read_primary[read]
// and per window of units [u0, u1), all into one cleared staging block so that the ranges of host units read as zeros:
//   k_fil_chain    a lane per chain: contig, pos, offset 0, AS, strand, and the end of its CIGAR
//   k_fil_cigar    a 16-lane group per chain, consecutive lanes on consecutive words; four byte loads per word (a CIGAR lies at any alignment in the compact buffer)
//   k_fil_names    a 16-lane group per unit, consecutive lanes on consecutive bytes, the NUL behind
//   k_fil_bases    a wavefront per read, consecutive lanes on consecutive output bytes: bases (unpacked through the 16-letter code, or the packed bytes as they lie)
//                  and qualities + 33
// and, only where hlala_bam_fill_create_wide or HLALA_SEEDS_GPU_FILL_WIDE found wide units (unit_count > 32 or a mate beyond 16; bam_fill_wide_core.h), which
// k_fil_rank and k_fil_src then leave alone (FilSample::wide, a bit per unit):
//   k_fil_wide_rank  a wavefront per wide read, drawn from the host's list of wide units: the lanes walk the unit's records in strides of 64 and keep the mate's by
//                  ballot and prefix count, score and place into LDS in file order; lane 0 runs fil_sort_wide there (the idiom of k_bgzf_inflate: the serial part on
//                  one lane, the wave places the result); the wave writes the sorted descriptor numbers and the exclusive prefix of their CIGAR counts into the
//                  read's slots of two scratch arrays, finds the first primary by a ballot in sorted order and writes the sizes where k_fil_rank writes them
//   k_fil_wide_src   behind the scans, a lane per slot: chain_src, chain_cig and read_primary from the scratch arrays (the sort is not run twice)
// No narrow kernel's serial depth depends on the sample; the loops of a lane run over 16 lanes, or over the bytes of one record's part in strides of the group.
//
// Bounds: a unit's range is checked against n before a descriptor is read and a permutation value before it indexes; every byte of the buffer is read through
// fil_byte (nothing at or beyond nBytes); chain numbers are checked against the chain count and every window offset against the window's size before a store.
// What cannot be laid out (a mate beyond 16, or beyond max_mate on the wide path, no primary, a range outside the descriptors) sets a bit in *bad and is refused by
// the host before any window runs.  The wide kernels check the list entry against the unit count, the unit's range and every place taken from LDS against the unit's
// count, the mate's count against max_mate before a slot of LDS is written, and every scratch offset against the read's slots.
#pragma once
#include <cstddef>
#include "device_common.h"
#include "bam_fill_core.h"
#include "bam_fill_wide_core.h"

namespace hlala {

struct FilSample {
    const hlala_bam_rec* recs; u32 n; const uint8_t* bytes; u64 nBytes; const u32* perm; const u32* unitFirst; const u32* unitCount; u32 nUnits; u32 nm;
    const u32* wide;      // a bit per unit: the wide kernels lay it out (null: no unit)
};
__device__ __forceinline__ bool fil_wide_unit(const FilSample& S, u64 u) { return S.wide && ((S.wide[u >> 5] >> (u & 31u)) & 1u); }
enum { FIL_BAD_RANGE = 1, FIL_BAD_MATE = 2, FIL_BAD_PRIMARY = 4, FIL_BAD_PERM = 8 };

__global__ __launch_bounds__(256) void k_fil_append(u32 n, const hlala_bam_rec* in, u64 base, hlala_bam_rec* out)
{
    static_assert(sizeof(hlala_bam_rec) == 48 && offsetof(hlala_bam_rec, rec_off) == 16, "a descriptor is six 64-bit words, rec_off the third");
    const u32 i = blockIdx.x * 256u + threadIdx.x;
    if(i >= n) return;
    const u64* src = (const u64*)(in + i); u64* dst = (u64*)(out + i);
    const u64 w0 = src[0], w1 = src[1], w2 = src[2], w3 = src[3], w4 = src[4], w5 = src[5];
    dst[0] = w0; dst[1] = w1; dst[2] = w2 + base; dst[3] = w3; dst[4] = w4; dst[5] = w5;
}

// the descriptor at place i of the grouped order
__device__ __forceinline__ u32 fil_desc(const FilSample& S, u64 i, u32& bad)
{
    if(i >= S.n) { bad |= FIL_BAD_RANGE; return 0; }
    if(!S.perm) return (u32)i;
    const u32 g = S.perm[i];
    if(g >= S.n) { bad |= FIL_BAD_PERM; return 0; }
    return g;
}

// what a lane of a read's 16-lane group knows after the exchanges
struct FilLane { bool valid, isPrimary; u32 g, rank, cnt, nCig, cigBefore, cigTotal, nameLen; int32_t lSeq; };

// All 64 lanes of the wavefront run this (ballots and exchanges inside): `live` is false for the lanes of a group beyond the last read.
__device__ __forceinline__ FilLane fil_rank(const FilSample& S, u64 r, bool live, u32& bad)
{
    using namespace hlala_bamfill;
    const u32 l = threadIdx.x & 15u, grp = (u32)lane_id() >> 4;
    u32 first = FIL_HOST, count = 0, mate = 0;
    if(live) { const u64 u = r / S.nm; mate = (u32)(r % S.nm); first = S.unitFirst[u]; count = S.unitCount[u]; }
    bool fill = live && first != FIL_HOST && !fil_wide_unit(S, r / S.nm);
    if(fill && (count == 0 || (u64)first + count > S.n)) { bad |= FIL_BAD_RANGE; fill = false; }
    if(fill && count > FIL_MAX_UNIT) { bad |= FIL_BAD_MATE; count = FIL_MAX_UNIT; }
    // records l and l + 16 of the unit: do they belong to this mate
    bool m0 = false, m1 = false;
    if(fill && l < count) m0 = S.recs[fil_desc(S, (u64)first + l, bad)].which == mate;
    if(fill && l + 16u < count) m1 = S.recs[fil_desc(S, (u64)first + l + 16u, bad)].which == mate;
    const u64 b0 = __ballot(m0), b1 = __ballot(m1);
    u32 mask = (u32)((b0 >> (16u * grp)) & 0xFFFFu) | ((u32)((b1 >> (16u * grp)) & 0xFFFFu) << 16);
    u32 cnt = (u32)__popc(mask);
    if(cnt > FIL_MAX_MATE) { bad |= FIL_BAD_MATE; cnt = FIL_MAX_MATE; }
    // lane l takes the l-th of them in file order
    for(u32 t = 0; t < l; t++) mask &= mask - 1u;
    FilLane L;
    L.valid = fill && l < cnt && mask != 0; L.cnt = cnt; L.g = 0; L.nCig = 0; L.lSeq = 0; L.nameLen = 0;
    const u32 k = L.valid ? (u32)__ffs((int)mask) - 1u : 0u;
    int32_t as = 0; u32 prim = 0;
    if(L.valid) { L.g = fil_desc(S, (u64)first + k, bad); const hlala_bam_rec& x = S.recs[L.g]; as = x.as; L.nCig = x.n_cigar; prim = (x.flags >> 1) & 1u; L.lSeq = x.l_seq; }
    if(fill && l == 0) L.nameLen = S.recs[fil_desc(S, first, bad)].nameLen;
    u32 rank = 0, cigBefore = 0, cigTotal = 0; bool primBefore = false;
    for(int j = 0; j < 16; j++) {
        const int vj = __shfl((int)L.valid, j, 16), asj = __shfl(as, j, 16); const u32 kj = (u32)__shfl((int)k, j, 16), cj = (u32)__shfl((int)L.nCig, j, 16), pj = (u32)__shfl((int)prim, j, 16);
        if(!vj) continue;
        cigTotal += cj;
        if(fil_before(asj, kj, as, k)) { rank++; cigBefore += cj; if(pj) primBefore = true; }
    }
    L.rank = rank; L.cigBefore = cigBefore; L.cigTotal = cigTotal;
    L.isPrimary = L.valid && prim && !primBefore;
    // the primary's l_seq to every lane of the group
    const u32 pm = (u32)((__ballot(L.isPrimary) >> (16u * grp)) & 0xFFFFu);
    const int src = pm ? __ffs((int)pm) - 1 : 0;
    const int32_t ls = __shfl(L.lSeq, src, 16);
    if(fill && !pm) bad |= FIL_BAD_PRIMARY;
    L.lSeq = pm ? ls : 0;
    if(!fill) L.cnt = 0;
    return L;
}

// sizes: lSeq / nChain / nCig [nReads + 1], nameSize [nUnits + 1] (cleared before; the entries of host units are k_fil_host's)
__global__ __launch_bounds__(256) void k_fil_rank(FilSample S, u64 nReads, int64_t* lSeq, int64_t* nChain, int64_t* nCig, int64_t* nameSize, u32* badOut)
{
    const u64 t = (u64)blockIdx.x * 256u + threadIdx.x, r = t >> 4;
    const bool live = r < nReads;
    u32 bad = 0;
    const FilLane L = fil_rank(S, r, live, bad);
    if(bad) atomicOr(badOut, bad);
    if(!live || (threadIdx.x & 15u) != 0 || S.unitFirst[r / S.nm] == hlala_bamfill::FIL_HOST || fil_wide_unit(S, r / S.nm)) return;
    lSeq[r] = L.lSeq > 0 ? L.lSeq : 0; nChain[r] = L.cnt; nCig[r] = L.cigTotal;
    if(r % S.nm == 0) nameSize[r / S.nm] = (int64_t)L.nameLen + 1;
}

// host unit j is unit hostUnit[j]; its sizes are hostSizes[j * (3 nm + 1) ...]
__global__ __launch_bounds__(64) void k_fil_host(u32 nHost, u32 nUnits, u32 nm, const u32* hostUnit, const int64_t* hostSizes, int64_t* lSeq, int64_t* nChain, int64_t* nCig, int64_t* nameSize)
{
    const u32 j = blockIdx.x * 64u + threadIdx.x;
    if(j >= nHost) return;
    const u32 u = hostUnit[j];
    if(u >= nUnits) return;
    const int64_t* hs = hostSizes + (u64)j * (3u * nm + 1u);
    for(u32 m = 0; m < nm; m++) { const u64 r = (u64)u * nm + m; lSeq[r] = hs[3 * m]; nChain[r] = hs[3 * m + 1]; nCig[r] = hs[3 * m + 2]; }
    nameSize[u] = hs[3 * nm];
}

// behind the scans: the chains' sources (cleared to FIL_HOST before), where their CIGARs start, the reads' primaries
__global__ __launch_bounds__(256) void k_fil_src(FilSample S, u64 nReads, const int64_t* chainOff, const int64_t* cigCount, u64 nChains, u32* chainSrc, int64_t* chainCig, int32_t* readPrimary)
{
    const u64 t = (u64)blockIdx.x * 256u + threadIdx.x, r = t >> 4;
    const bool live = r < nReads;
    u32 bad = 0;
    const FilLane L = fil_rank(S, r, live, bad);
    if(!live || !L.valid) return;
    const u64 c = (u64)chainOff[r] + L.rank;
    if(c >= nChains || c >= (u64)chainOff[r + 1]) return;
    chainSrc[c] = L.g; chainCig[c] = cigCount[r] + (int64_t)L.cigBefore;
    if(L.isPrimary) readPrimary[r] = (int32_t)c;
}

// ---- the wide units.  unit[w]: wide unit w; wide read wr = w * nm + mate owns the slots [off[wr], off[wr + 1]) of desc / cig (unit_count of them: no mate has more)
struct FilWide { const u32* unit; const u32* off; u32 nUnits, maxMate; u32 *desc, *cig, *prim; };
constexpr u32 FIL_NO_PRIMARY = 0xFFFFFFFFu;

__global__ __launch_bounds__(64) void k_fil_wide_rank(FilSample S, FilWide Wd, int64_t* lSeq, int64_t* nChain, int64_t* nCig, int64_t* nameSize, u32* badOut)
{
    using namespace hlala_bamfill;
    __shared__ int32_t sScore[FIL_WIDE_MAX];
    __shared__ uint16_t sPlace[FIL_WIDE_MAX];
    __shared__ u32 sStack[FIL_WIDE_STACK_WORDS];
    __shared__ u32 sHeaps;
    const u32 wr = blockIdx.x, lane = (u32)lane_id(), w = wr / S.nm, mate = wr % S.nm;
    if(w >= Wd.nUnits) return;
    // (every condition that ends the wavefront early is wave-uniform)
    const u32 u = Wd.unit[w];
    if(u >= S.nUnits) { if(lane == 0) atomicOr(badOut, (u32)FIL_BAD_RANGE); return; }
    const u32 first = S.unitFirst[u], count = S.unitCount[u], cap = Wd.maxMate < FIL_WIDE_MAX ? Wd.maxMate : FIL_WIDE_MAX;
    const u32 off = Wd.off[wr], offEnd = Wd.off[wr + 1];
    if(first == FIL_HOST || count == 0 || (u64)first + count > S.n || offEnd < off || offEnd - off < count) { if(lane == 0) atomicOr(badOut, (u32)FIL_BAD_RANGE); return; }
    if(count > S.nm * cap) { if(lane == 0) atomicOr(badOut, (u32)FIL_BAD_MATE); return; }                // (so a place fits 16 bits: count <= 2 * 4096)
    u32 bad = 0, n = 0;
    for(u32 base = 0; base < count; base += 64u) {
        const u32 k = base + lane;
        bool mine = false; int32_t as = 0;
        if(k < count) { const hlala_bam_rec& x = S.recs[fil_desc(S, (u64)first + k, bad)]; mine = x.which == mate; as = x.as; }
        const u64 b = __ballot(mine);
        const u32 at = n + (u32)__popcll(b & ((1ull << lane) - 1ull));
        if(mine && at < cap) { sScore[at] = as; sPlace[at] = (uint16_t)k; }
        n += (u32)__popcll(b);
    }
    if(n > cap) { if(lane == 0) atomicOr(badOut, (u32)FIL_BAD_MATE); return; }
    WSYNC();
    if(lane == 0) sHeaps = fil_sort_wide(sScore, sPlace, n, sStack);
    WSYNC();
    if(sHeaps == FIL_WIDE_OVERFLOW) { if(lane == 0) atomicOr(badOut, (u32)FIL_BAD_MATE); return; }
    u32 cigBefore = 0, primAt = FIL_NO_PRIMARY; int32_t lseq = 0;
    for(u32 base = 0; base < n; base += 64u) {
        const u32 i = base + lane;
        u32 g = 0, nc = 0; bool prim = false, ok = false; int32_t ls = 0;
        if(i < n) {
            const u32 k = sPlace[i];
            if(k < count) { g = fil_desc(S, (u64)first + k, bad); const hlala_bam_rec& x = S.recs[g]; nc = x.n_cigar; prim = ((x.flags >> 1) & 1u) != 0; ls = x.l_seq; ok = true; }
            else bad |= FIL_BAD_RANGE;
        }
        int total = 0;
        const u32 before = (u32)wave_excl_scan((int)nc, total);
        if(ok && i < offEnd - off) { Wd.desc[off + i] = g; Wd.cig[off + i] = cigBefore + before; }
        const u64 pb = __ballot(prim);
        if(primAt == FIL_NO_PRIMARY && pb) { const int src = __ffsll((unsigned long long)pb) - 1; primAt = base + (u32)src; lseq = __shfl(ls, src); }
        cigBefore += (u32)total;
    }
    if(primAt == FIL_NO_PRIMARY) bad |= FIL_BAD_PRIMARY;
    if(bad) atomicOr(badOut, bad);
    if(lane != 0) return;
    const u64 r = (u64)u * S.nm + mate;
    lSeq[r] = lseq > 0 ? lseq : 0; nChain[r] = n; nCig[r] = cigBefore; Wd.prim[wr] = primAt;
    if(mate == 0) { u32 b2 = 0; nameSize[u] = (int64_t)S.recs[fil_desc(S, first, b2)].nameLen + 1; }
}

// slot j of the scratch arrays: the wide read whose slots hold it, chain i of that read
__global__ __launch_bounds__(256) void k_fil_wide_src(FilSample S, FilWide Wd, u32 nWideReads, u32 nSlots, const int64_t* chainOff, const int64_t* cigCount, u64 nChains, u32* chainSrc, int64_t* chainCig,
                                                      int32_t* readPrimary)
{
    const u64 t = (u64)blockIdx.x * 256u + threadIdx.x;
    if(t >= nSlots || nWideReads == 0) return;
    const u32 j = (u32)t;
    u32 lo = 0, hi = nWideReads;                            // off[lo] <= j < off[hi]
    while(hi - lo > 1u) { const u32 mid = lo + (hi - lo) / 2u; if(Wd.off[mid] <= j) lo = mid; else hi = mid; }
    if(Wd.off[lo] > j || j >= Wd.off[lo + 1]) return;
    const u32 i = j - Wd.off[lo], w = lo / S.nm, mate = lo % S.nm;
    if(w >= Wd.nUnits) return;
    const u32 u = Wd.unit[w];
    if(u >= S.nUnits) return;
    const u64 r = (u64)u * S.nm + mate;
    const int64_t c0 = chainOff[r], c1 = chainOff[r + 1];
    if(c0 < 0 || c1 < c0 || (int64_t)i >= c1 - c0) return;
    const u64 c = (u64)c0 + i;
    const u32 g = Wd.desc[j];
    if(c >= nChains || g >= S.n) return;
    chainSrc[c] = g; chainCig[c] = cigCount[r] + (int64_t)Wd.cig[j];
    if(i == Wd.prim[lo]) readPrimary[r] = (int32_t)c;
}

// ---- a window: chains [c0, c0 + nc), CIGAR words [g0, g0 + ng), units [u0, u0 + nu) with name bytes [n0, n0 + nn), reads [r0, r0 + nr) with bases [b0, b0 + nb)
struct FilWindow {
    u64 c0, nc, g0, ng, u0, nu, n0, nn, r0, nr, b0, nb, p0, np;      // p0, np: the packed bytes
    int32_t *chainContig, *chainPos, *chainOffset, *chainAs; uint8_t* chainReverse; int64_t* cigarOffEnd; u32* cigar; uint8_t* names; uint8_t *bases, *packed, *quals;
};

__global__ __launch_bounds__(256) void k_fil_chain(FilSample S, FilWindow W, const u32* chainSrc, const int64_t* chainCig)
{
    const u64 k = (u64)blockIdx.x * 256u + threadIdx.x;
    if(k >= W.nc) return;
    const u32 g = chainSrc[W.c0 + k];
    if(g >= S.n) return;                                   // (FIL_HOST: a chain of a host unit)
    const hlala_bam_rec& x = S.recs[g];
    W.chainContig[k] = x.contig; W.chainPos[k] = x.pos; W.chainOffset[k] = 0; W.chainAs[k] = x.as; W.chainReverse[k] = (uint8_t)(x.flags & 1);
    W.cigarOffEnd[k] = chainCig[W.c0 + k] + x.n_cigar;
}

__global__ __launch_bounds__(256) void k_fil_cigar(FilSample S, FilWindow W, const u32* chainSrc, const int64_t* chainCig)
{
    using namespace hlala_bamfill;
    const u64 t = (u64)blockIdx.x * 256u + threadIdx.x, k = t >> 4;
    if(k >= W.nc) return;
    const u32 g = chainSrc[W.c0 + k];
    if(g >= S.n) return;
    const hlala_bam_rec& x = S.recs[g];
    const u64 at = fil_cigar_at(x), to = (u64)chainCig[W.c0 + k] - W.g0;
    for(u32 w = threadIdx.x & 15u; w < x.n_cigar; w += 16u) if(to + w < W.ng) W.cigar[to + w] = fil_word(S.bytes, S.nBytes, at + 4ull * w);
}

__global__ __launch_bounds__(256) void k_fil_names(FilSample S, FilWindow W, const int64_t* nameOff)
{
    using namespace hlala_bamfill;
    const u64 t = (u64)blockIdx.x * 256u + threadIdx.x, k = t >> 4;
    if(k >= W.nu) return;
    const u32 first = S.unitFirst[W.u0 + k];
    if(first == FIL_HOST) return;
    u32 bad = 0;
    const hlala_bam_rec& x = S.recs[fil_desc(S, first, bad)];
    const u64 to = (u64)nameOff[W.u0 + k] - W.n0;
    for(u32 i = threadIdx.x & 15u; i <= x.nameLen; i += 16u) if(to + i < W.nn) W.names[to + i] = i < x.nameLen ? fil_byte(S.bytes, S.nBytes, x.rec_off + FIL_NAME_AT + i) : 0;
}

__global__ __launch_bounds__(256) void k_fil_bases(FilSample S, FilWindow W, const int64_t* readOff, const int32_t* readPrimary, const u32* chainSrc, u64 nChains)
{
    using namespace hlala_bamfill;
    const u64 k = (u64)blockIdx.x * 4u + (threadIdx.x >> 6);
    if(k >= W.nr) return;
    const u64 r = W.r0 + k;
    if(S.unitFirst[r / S.nm] == FIL_HOST) return;
    const u64 c = (u64)(u32)readPrimary[r];
    if(c >= nChains) return;
    const u32 g = chainSrc[c];
    if(g >= S.n) return;
    const hlala_bam_rec& x = S.recs[g];
    const int64_t off = readOff[r]; const u64 ls = (u64)(readOff[r + 1] - off), to = (u64)off - W.b0;
    const u64 s4 = fil_seq_at(x), ql = fil_qual_at(x, (int32_t)ls);
    const u32 lane = (u32)lane_id();
    if(W.packed) { const u64 pt = (u64)fil_packed_at(off, (int64_t)r) - W.p0; for(u64 i = lane; i < (ls + 1) / 2; i += 64u) if(pt + i < W.np) W.packed[pt + i] = fil_byte(S.bytes, S.nBytes, s4 + i); }
    else for(u64 i = lane; i < ls; i += 64u) if(to + i < W.nb) { const uint8_t b = fil_byte(S.bytes, S.nBytes, s4 + (i >> 1)); W.bases[to + i] = fil_base((i & 1) ? (b & 15u) : (u32)(b >> 4)); }
    for(u64 i = lane; i < ls; i += 64u) if(to + i < W.nb) W.quals[to + i] = fil_qual(fil_byte(S.bytes, S.nBytes, ql + i));
}

}  // namespace hlala

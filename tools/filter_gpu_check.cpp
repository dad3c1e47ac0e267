// filter_gpu_check.cpp -- the host model of hlala_filter_positions_gpu (hla-la_amd/csrc/filter_gpu_model.h over filter_gpu_core.h) against the specification,
// hlala_filter_positions (host_filters.cpp), as a program of its own, so that it can be built with -fsanitize=address,undefined and run as a child process
// (tests/test_filter_gpu_model.py does both).  Every array is a heap buffer of exactly its size.  pos_use, read_ignored and all twelve counters must be equal on
//   * random loci with the statistics of tests/test_filters.py: synth_positions, under six parameter sets, the strand filter among them        (line "random <loci>")
//   * single-bucket loci of every size in 0..40 and 63, 64, 65, 255, 256, 257, 4095, 4096                                                   (line "single <loci>")
//   * buckets whose weights are McIlroy's adversary against the std::sort this is built with (bam_fill_model.h: fil_adversary) at n = 64, 1000 and 4096; the
//     program FAILS unless the model's counts[3] says the heap sort was entered: a fallback that never ran is not pinned           (line "adversary <n>:<heap sorts> ...")
//   * a bucket of 4097, which the model must refuse with HLALA_E_CAPACITY and a text that starts "not available:", nothing written            (line "refused 4097")
//   g++ -std=c++17 -fsanitize=address,undefined -o filter_gpu_check tools/filter_gpu_check.cpp hla-la_amd/csrc/host_filters.cpp
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../hla-la_amd/csrc/bam_fill_model.h"
#include "../hla-la_amd/csrc/filter_gpu_model.h"

namespace {

struct Locus {
    std::vector<double> wok; std::vector<int32_t> posOff{0}, exon, genoOff{0}; std::vector<uint8_t> mapq, mate, geno, rev;
    void read(double w1, double w2, bool r1, bool r2) { wok.push_back(w1); wok.push_back(w2); rev.push_back(r1); rev.push_back(r2); }
    void position(int32_t x, uint8_t q, uint8_t m, const std::string& al) { exon.push_back(x); mapq.push_back(q); mate.push_back(m); geno.insert(geno.end(), al.begin(), al.end()); genoOff.push_back((int32_t)geno.size()); }
    void end_read() { posOff.push_back((int32_t)exon.size()); }
};
template <class T> T* exact(const std::vector<T>& v) { T* p = (T*)malloc(v.size() * sizeof(T) ? v.size() * sizeof(T) : 1); if(!v.empty()) memcpy(p, v.data(), v.size() * sizeof(T)); return p; }

unsigned long long g_s = 88172645463325252ull;
unsigned long long next() { g_s ^= g_s << 13; g_s ^= g_s >> 7; g_s ^= g_s << 17; return g_s; }
double unit() { return (double)(next() >> 11) / 9007199254740992.0; }

// 0: equal (or refused alike); 1: a difference.  *heaps: counts[3] of the model
int compare(const Locus& L, const hlala_filter_params& P, const char* what, int64_t* heaps, int expect = HLALA_OK)
{
    hlala_exon_positions_out o; memset(&o, 0, sizeof(o));
    const int nr = (int)L.posOff.size() - 1, np = (int)L.exon.size();
    o.n_reads = o.cap_reads = nr; o.n_pos = o.cap_pos = np; o.n_chars = o.cap_chars = (int)L.geno.size();
    o.read_weighted_ok = exact(L.wok); o.pos_off = exact(L.posOff); o.pos_exon = exact(L.exon); o.pos_mapq = exact(L.mapq); o.pos_mate = exact(L.mate); o.geno_off = exact(L.genoOff);
    o.geno_chars = exact(L.geno); o.read_reverse = exact(L.rev);
    std::vector<uint8_t> fill((size_t)np, 7), fillR((size_t)nr, 7);
    uint8_t *useH = exact(fill), *useM = exact(fill), *ignH = exact(fillR), *ignM = exact(fillR);
    hlala_filter_stats sH, sM; memset(&sH, 0x55, sizeof(sH)); memset(&sM, 0x55, sizeof(sM));
    int64_t counts[6] = {0, 0, 0, 0, 0, 0}; std::string why;
    const int rcH = hlala_filter_positions(&o, &P, useH, ignH, &sH), rcM = hlala_filter::filter_model(&o, &P, useM, ignM, &sM, counts, 0, &why);
    int bad = 0;
    if(expect == HLALA_OK) {
        if(rcH != HLALA_OK || rcM != HLALA_OK) { fprintf(stderr, "filter_gpu_check: %s: host %d, model %d (%s)\n", what, rcH, rcM, why.c_str()); bad = 1; }
        else if(memcmp(useH, useM, (size_t)np) || memcmp(ignH, ignM, (size_t)nr) || memcmp(&sH, &sM, sizeof(sH))) {
            int j = 0; while(j < np && useH[j] == useM[j]) j++;
            fprintf(stderr, "filter_gpu_check: %s (%d reads, %d positions): the model differs from hlala_filter_positions (first pos_use difference at %d of %d)\n", what, nr, np, j, np); bad = 1;
        }
    } else {
        bool untouched = true;
        for(int j = 0; j < np; j++) untouched = untouched && useM[j] == 7;
        for(int r = 0; r < nr; r++) untouched = untouched && ignM[r] == 7;
        if(rcM != expect || !untouched || (expect == HLALA_E_CAPACITY && why.rfind("not available:", 0) != 0)) { fprintf(stderr, "filter_gpu_check: %s: model %d (%s), expected %d with nothing written\n", what, rcM, why.c_str(), expect); bad = 1; }
    }
    if(heaps) *heaps = counts[3];
    free(o.read_weighted_ok); free(o.pos_off); free(o.pos_exon); free(o.pos_mapq); free(o.pos_mate); free(o.geno_off); free(o.geno_chars); free(o.read_reverse);
    free(useH); free(useM); free(ignH); free(ignM);
    return bad;
}

hlala_filter_params defaults()
{
    hlala_filter_params P; memset(&P, 0, sizeof(P));
    P.filter_first20 = 1; P.first20_n = 20; P.first20_min_prop = 0.1; P.first20_limit_per_read = 2; P.min_per_position_mapq = 0.7;
    P.high_coverage_filter = 0; P.high_coverage_min_coverage = 100; P.high_coverage_min_freq = 0.2; P.long_read_strand_filter = 0; P.strand_min_allele_coverage = 100; P.strand_min_freq = 0.1;
    return P;
}

std::string allele(int truth)
{
    static const char* A = "ACGT";
    std::string al(1, A[truth]);
    const double u = unit();
    if(u < 0.04) al = std::string(1, A[next() % 4]);
    if(unit() < 0.02) al += unit() < 0.5 ? "T" : (unit() < 0.5 ? "TG" : std::string(1 + next() % 6, (char)(0x7E + next() % 4)));
    if(unit() < 0.005) al = "_";
    return al;
}
Locus random_locus(int nReads, int nExon)
{
    Locus L; std::vector<int> truth((size_t)nExon);
    for(int& t : truth) t = (int)(next() % 4);
    for(int r = 0; r < nReads; r++) {
        const int a = (int)(next() % (unsigned)(nExon - 30)), b = std::min(nExon, a + 20 + (int)(next() % 100));
        const bool dirty = unit() < 0.3;
        L.read(dirty ? 1.0 - (double)(1 + next() % 5) / 150.0 : 1.0, dirty ? 1.0 - (double)(next() % 4) / 150.0 : 1.0, unit() < 0.07, unit() < 0.07);
        for(int x = a; x < b; x++) {
            L.position(x, unit() < 0.05 ? '#' : 'I', (uint8_t)(1 + (x - a) * 2 / std::max(1, b - a)), allele(truth[(size_t)x]));
            if(unit() < 0.01) L.position(x, 'I', 2, allele(truth[(size_t)x]));          // a read with two entries at one exon position
        }
        L.end_read();
    }
    return L;
}
// n reads with one position each at exon position 0
Locus single_bucket(int n, const int32_t* score)
{
    Locus L;
    for(int r = 0; r < n; r++) {
        const double w = score ? (double)score[r] / 8192.0 : (unit() < 0.7 ? 1.0 : 1.0 - (double)(next() % 4) / 128.0);
        L.read(w, w, unit() < 0.5, false);
        L.position(0, 'I', 1, allele((int)(next() % 2)));
        L.end_read();
    }
    return L;
}

}  // namespace

int main()
{
    long loci = 0;
    std::vector<hlala_filter_params> sets(6, defaults());
    sets[1].high_coverage_filter = 1; sets[1].high_coverage_min_coverage = 1; sets[1].high_coverage_min_freq = 0.15;
    sets[2].first20_limit_per_read = 0;
    sets[3].min_per_position_mapq = 0.2;
    sets[4].long_read_strand_filter = 1; sets[4].strand_min_allele_coverage = 10; sets[4].strand_min_freq = 0.2;
    sets[5].long_read_strand_filter = 1; sets[5].strand_min_allele_coverage = 30; sets[5].strand_min_freq = 0.05; sets[5].first20_n = 17; sets[5].high_coverage_filter = 1;
    const int shapes[5][2] = {{60, 200}, {900, 300}, {2500, 120}, {1500, 150}, {300, 40}};
    for(const auto& sh : shapes) {
        const Locus L = random_locus(sh[0], sh[1]);
        for(const hlala_filter_params& P : sets) { if(compare(L, P, "random locus", nullptr)) return 1; loci++; }
    }
    printf("random %ld\n", loci);
    loci = 0;
    std::vector<int> sizes;
    for(int n = 0; n <= 40; n++) sizes.push_back(n);
    for(int n : {63, 64, 65, 255, 256, 257, 4095, 4096}) sizes.push_back(n);
    for(int n : sizes) {
        const Locus L = single_bucket(n, nullptr);
        for(size_t k = 0; k < (n > 1000 ? (size_t)2 : sets.size()); k++) { if(compare(L, sets[k == 1 && n > 1000 ? 4 : k], "single bucket", nullptr)) return 1; loci++; }
    }
    printf("single %ld\n", loci);
    printf("adversary");
    for(int n : {64, 1000, 4096}) {
        std::vector<int32_t> s((size_t)n);
        hlala_bamfill::fil_adversary((uint32_t)n, s.data());
        int64_t heaps = 0;
        if(compare(single_bucket(n, s.data()), sets[0], "adversary weights", &heaps)) { printf("\n"); return 1; }
        printf(" %d:%lld", n, (long long)heaps);
        if(heaps < 1) { printf("\n"); fprintf(stderr, "filter_gpu_check: the adversary bucket of %d entries did not reach the heap sort: the fallback is not pinned\n", n); return 1; }
    }
    printf("\n");
    if(compare(single_bucket(4097, nullptr), sets[0], "a bucket of 4097", nullptr, HLALA_E_CAPACITY)) return 1;
    printf("refused 4097\n");
    return 0;
}

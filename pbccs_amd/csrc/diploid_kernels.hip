// pbccs_amd/csrc/diploid_kernels.hip -- diploid site calling on the device (see diploid_kernels.hpp).
#include "diploid_kernels.hpp"

#include <cfloat>
#include <cstdlib>
#include <string>

#include "arrow_device.hpp"

namespace pbccs {

#define DHIP(expr)                                                                                     \
    do {                                                                                               \
        const hipError_t e_ = (expr);                                                                  \
        if (e_ != hipSuccess) throw DeviceError(std::string("diploid: ") + hipGetErrorString(e_));     \
    } while (0)

int site_chunk()
{
    const char* e = std::getenv("PBCCS_SITE_CHUNK");
    const int v = e ? std::atoi(e) : 0;
    return v > 0 ? v : kSiteChunk;
}

void site_mutation_codes(const std::string& tpl, int begin, int end, std::vector<int>* codes)
{
    codes->clear();
    codes->reserve((size_t)(end - begin) * 8);
    for (int p = begin; p < end; ++p) {
        const int tb = base_index(tpl[p]);
        for (int b = 0; b < 4; ++b)
            if (b != tb) codes->push_back(mut_code(p, kSub, b));
        for (int b = 0; b < 4; ++b) codes->push_back(mut_code(p, kIns, b));
        codes->push_back(mut_code(p, kDel, 0));
    }
}

namespace {

// column c of site s -> the site's mutation index j (0..7), or -1 for the template base's own column: the three
// substitution codes name every base but the template's
__device__ __forceinline__ int site_column_mutation(const int* __restrict__ codes8, int c)
{
    const int tb = 6 - (mut_base(codes8[0]) + mut_base(codes8[1]) + mut_base(codes8[2]));
    if (c == tb) return -1;
    return c - (c > tb ? 1 : 0);
}

__global__ void __launch_bounds__(256) k_site_scores(const double* __restrict__ delta, const int* __restrict__ codes,
                                                     const int* __restrict__ rActive, const int* __restrict__ rTs,
                                                     const int* __restrict__ rTe, int nReads, int nSites,
                                                     float* __restrict__ out)
{
    const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long per = (long long)nReads * kSiteAlleles;
    if (g >= per * nSites) return;
    const int s = (int)(g / per);
    const int rem = (int)(g - (long long)s * per);
    const int rr = rem / kSiteAlleles, c = rem - rr * kSiteAlleles;
    const int j = site_column_mutation(codes + 8LL * s, c);
    float v = 0.0f;
    if (j >= 0) {
        const int code = codes[8LL * s + j];
        const int type = mut_type(code), pos = mut_pos(code);
        const int me = (type == kIns) ? pos : pos + 1;
        const int ts = rTs[rr], te = rTe[rr];
        // ReadScoresMutation (MultiReadMutationScorer.cpp:70-80), the mask k_reduce applies
        const bool scores = (type == kIns) ? (ts <= me && pos <= te) : (ts < me && pos < te);
        if (rActive[rr] && scores) v = (float)delta[(long long)rr * (8LL * nSites) + 8LL * s + j];
    }
    out[g] = v;
}

__global__ void __launch_bounds__(256) k_site_scores_q(const float* __restrict__ delta, const int* __restrict__ codes,
                                                       int nReads, int nSites, float* __restrict__ out)
{
    const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long per = (long long)nReads * kSiteAlleles;
    if (g >= per * nSites) return;
    const int s = (int)(g / per);
    const int rem = (int)(g - (long long)s * per);
    const int rr = rem / kSiteAlleles, c = rem - rr * kSiteAlleles;
    const int j = site_column_mutation(codes + 8LL * s, c);
    float v = 0.0f;
    if (j >= 0) {
        v = delta[(8LL * s + j) * nReads + rr];
        if (v != v) v = 0.0f;   // NaN: the read is inactive or does not score the mutation
    }
    out[g] = v;
}

__device__ __forceinline__ float logaddexp_d(float x, float y)   // Diploid.cpp:110-118
{
    const float diff = x - y;
    if (diff > 0) return x + log1pf(expf(-diff));
    return y + log1pf(expf(diff));
}

constexpr float kLog2f = 0.693147182464599609375f;   // (float)log(2.0): `float log2 = log(2)` (Diploid.cpp:144)

// ---- k_diploid: IsSiteHeterozygous (Diploid.cpp:219-239) as a screen, 16 lanes (one DPP row) per site ---------
// Lane l < 9 loads column l of each read's row (one 36-byte row per step, coalesced) and carries that column's sum;
// lane l < 12 owns allele pair l -- in the reference's loop order (0,1) (0,2) (0,3) (1,2) (1,3) (2,3), then the same
// over the insertion columns 4..7 -- and fetches its two columns from the row's lanes.  Each lane walks the reads in
// order, so every float sum is accumulated in the reference's order; the group then folds the 9 column sums and
// the 12 pair totals from -FLT_MAX in lane order, every lane redundantly.  The row shuffles are ds_bpermute
// (`__shfl` with width 16): the source lane differs per lane (g0, g1), which CDNA's DPP row modes (shifts,
// rotates, mirrors, broadcasts of lane 15) cannot express; the kernel is bound by its expf / log1pf calls anyway.
//
// The device's expf / log1pf are OCML's and the reference's are glibc's, so the kernel only screens.  Bound on
// |logBF here - logBF on the host| for the same float tensor:
//   - a term t = log1pf(expf(-|d|)) lies in (0, ln 2].  expf within 3 ulp (OpenCL full profile) here and 1 ulp in
//     glibc moves e = expf(-|d|) <= 1 by at most 4 x 2^-24; log1p has slope <= 1, and log1pf's own 2 + 1 ulp of
//     t < 1 add 3 x 2^-24: |t_dev - t_host| <= 7 x 2^-24 < tau = 2^-21.
//   - a pair total adds fl(max + t) per read: two roundings of values that differ between the two sides, each at
//     most one ulp <= 2^-23 amax apart, with amax the largest magnitude among the partial totals and the terms.
//     After I reads the totals differ by at most I (tau + 2^-22 amax).
//   - the column sums are plain IEEE adds in the same order (contraction is off on both sides): identical.
//   - logaddexp is 1-Lipschitz in the max norm, so the 9-step fold of the column sums differs by at most
//     9 (tau + 2^-23 amax) and the 12-step fold of the pair totals by the totals' bound plus 12 (tau + 2^-23 amax);
//     the final subtraction adds one ulp of logBF <= 2^-23 amax.
//   bound = (I + 22) (tau + 2^-22 amax) covers their sum.
// A site is marked for the host (flag bit 0) unless logBF - prior <= -bound, i.e. unless the host's test
// logBF - prior > 0 is certain to fail; a NaN anywhere marks it.  Bit 1 records, for a marked site, that the best and
// second-best pair totals lie within twice the totals' bound, so the alleles could differ from the host's.  Marked
// sites are decided entirely on the host (diploid_sites), so no reported value depends on this kernel's libm.
__global__ void __launch_bounds__(256) k_diploid(const float* __restrict__ T, int nSites, int nReads, float prior,
                                                 int hostAll, int* __restrict__ flags)
{
    const long long site = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 4;
    const int l = threadIdx.x & 15;
    const bool live = site < nSites;
    const float* row = T + (live ? site : (long long)nSites - 1) * nReads * kSiteAlleles;
    const int q = l % 6, off = (l < 6) ? 0 : 4;
    const int g0 = off + (q >= 3 ? 1 : 0) + (q >= 5 ? 1 : 0);
    const int g1 = off + (q < 3 ? q + 1 : (q == 3 ? 2 : 3));
    float colSum = 0.0f;
    float total = (float)(-nReads) * kLog2f;   // `-I * log2` (:156)
    float amax = fabsf(total);
    for (int i = 0; i < nReads; ++i) {
        const float v = (l < kSiteAlleles) ? row[(long long)i * kSiteAlleles + l] : 0.0f;
        const float x = __shfl(v, g0, 16), y = __shfl(v, g1, 16);
        colSum += v;
        const float term = logaddexp_d(x, y);
        total += term;
        amax = fmaxf(amax, fmaxf(fabsf(term), fabsf(total)));
    }
    float hom = -FLT_MAX;
    for (int g = 0; g < kSiteAlleles; ++g) {
        const float s = __shfl(colSum, g, 16);
        hom = logaddexp_d(hom, s);
        amax = fmaxf(amax, fmaxf(fabsf(s), fabsf(hom)));
    }
    float het = -FLT_MAX, best = -FLT_MAX, second = -FLT_MAX, pairMax = 0.0f;
    for (int k = 0; k < kSitePairs; ++k) {
        const float t = __shfl(total, k, 16);
        pairMax = fmaxf(pairMax, __shfl(amax, k, 16));
        het = logaddexp_d(het, t);
        amax = fmaxf(amax, fabsf(het));
        if (t > best) {
            second = best;
            best = t;
        } else if (t > second) {
            second = t;
        }
    }
    amax = fmaxf(amax, pairMax);
    const float logBF = het - hom;
    const float unit = 0x1p-21f + 0x1p-22f * amax;
    const float bound = (float)(nReads + 22) * unit;
    const bool certainHom = (double)logBF - (double)prior <= -(double)bound;   // false for NaN
    int flag = (!certainHom || hostAll) ? 1 : 0;
    if (flag && !((double)best - (double)second > 2.0 * (double)nReads * (double)unit)) flag |= 2;
    if (live && l == 0) flags[site] = flag;
}

// ---- k_dgather: the marked sites' nReads x 9 slices, packed for one download ------------------------------------
__global__ void __launch_bounds__(64) k_dgather(const float* __restrict__ T, const int* __restrict__ list, int per,
                                                float* __restrict__ out)
{
    const float* src = T + (long long)list[blockIdx.x] * per;
    float* dst = out + (long long)blockIdx.x * per;
    for (int k = threadIdx.x; k < per; k += blockDim.x) dst[k] = src[k];
}

}  // namespace

void launch_site_scores_arrow(const double* delta, const int* codes, const int* rActive, const int* rTs,
                              const int* rTe, int nReads, int nSites, float* out, hipStream_t s)
{
    const long long n = (long long)nSites * nReads * kSiteAlleles;
    if (n <= 0) return;
    k_site_scores<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s>>>(delta, codes, rActive, rTs, rTe, nReads,
                                                                        nSites, out);
}

void launch_site_scores_quiver(const float* delta, const int* codes, int nReads, int nSites, float* out,
                               hipStream_t s)
{
    const long long n = (long long)nSites * nReads * kSiteAlleles;
    if (n <= 0) return;
    k_site_scores_q<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s>>>(delta, codes, nReads, nSites, out);
}

void diploid_sites(const float* tensor, int nSites, int nReads, int begin, float logPriorRatio, bool hostAll,
                   DiploidScratch& sc, hipStream_t s, std::vector<DiploidSiteH>* sites,
                   std::vector<int>* alleleForRead, DiploidStats* stats)
{
    sites->clear();
    alleleForRead->clear();
    if (nSites <= 0 || nReads <= 0) return;
    const StreamScope bound(s);
    sc.flags.reserve((size_t)nSites, false);
    const long long lanes = 16LL * nSites;
    k_diploid<<<dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, s>>>(tensor, nSites, nReads, logPriorRatio,
                                                                        hostAll ? 1 : 0, sc.flags.ptr);
    DHIP(hipGetLastError());
    std::vector<int> flags((size_t)nSites);
    DHIP(hipMemcpyAsync(flags.data(), sc.flags.ptr, (size_t)nSites * sizeof(int), hipMemcpyDeviceToHost, s));
    DHIP(hipStreamSynchronize(s));
    std::vector<int> list;
    for (int k = 0; k < nSites; ++k)
        if (flags[(size_t)k] & 1) list.push_back(k);
    stats->sitesScreened += nSites;
    stats->sitesSentToHost += (long long)list.size();
    if (list.empty()) return;
    const int per = nReads * kSiteAlleles;
    const size_t nPacked = list.size() * (size_t)per;
    sc.list.reserve(list.size(), false);
    sc.packed.reserve(nPacked, false);
    DHIP(hipMemcpyAsync(sc.list.ptr, list.data(), list.size() * sizeof(int), hipMemcpyHostToDevice, s));
    k_dgather<<<dim3((unsigned)list.size()), dim3(64), 0, s>>>(tensor, sc.list.ptr, per, sc.packed.ptr);
    DHIP(hipGetLastError());
    std::vector<float> packed(nPacked);
    DHIP(hipMemcpyAsync(packed.data(), sc.packed.ptr, nPacked * sizeof(float), hipMemcpyDeviceToHost, s));
    DHIP(hipStreamSynchronize(s));
    std::vector<int> afr((size_t)nReads);
    for (size_t a = 0; a < list.size(); ++a) {
        DiploidCall call;
        if (!is_site_heterozygous(packed.data() + a * (size_t)per, nReads, logPriorRatio, &call, afr.data())) continue;
        sites->push_back(DiploidSiteH{begin + list[a], call.allele0, call.allele1, call.logBayesFactor});
        alleleForRead->insert(alleleForRead->end(), afr.begin(), afr.end());
    }
    stats->sitesReported += (long long)sites->size();
}

}  // namespace pbccs

// pbccs_amd/csrc/strand_kernels.hip -- the strand-discordance screen's two kernels (see strand_kernels.hpp).
#include "strand_kernels.hpp"

#include "arrow_device.hpp"

namespace pbccs {

namespace {

// Per-strand sums of a round's deltas.  Lane l of a wave owns mutation m + l of the same item (but at item
// boundaries), so the loads d[rr * M] of a wave are contiguous, as k_reduce's are.
__global__ void __launch_bounds__(256) k_strand_sums(DevBatch B, ScoreWork W, StrandSums S)
{
    const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= W.mutStart[W.nWork]) return;
    int lo = 0, hi = W.nWork;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (W.mutStart[mid] <= g) lo = mid; else hi = mid;
    }
    const int k = lo;
    const int z = W.zmw[k];
    const int M = W.nMut[k];
    const int m = (int)(g - W.mutStart[k]);
    const int code = W.codes[W.mutBase[k] + m];
    const int type = mut_type(code), pos = mut_pos(code);
    const int me = (type == kIns) ? pos : pos + 1;
    const int rb = B.zReadBegin[z], nr = B.zNReads[z];
    const double* d = W.delta + W.deltaBase[k] + m;
    double sumF = 0.0, sumR = 0.0;
    int nF = 0, nR = 0;
    for (int rr = 0; rr < nr; ++rr) {
        const int r = rb + rr;
        const int ts = B.rTs[r], te = B.rTe[r];
        // ReadScoresMutation (MultiReadMutationScorer.cpp:70-80), the mask k_reduce applies
        const bool scores = (type == kIns) ? (ts <= me && pos <= te) : (ts < me && pos < te);
        if (!(B.rActive[r] && scores)) continue;
        const double v = d[(long long)rr * M];
        if (B.rStrand[r] == kFwd) {
            sumF += v;
            ++nF;
        } else {
            sumR += v;
            ++nR;
        }
    }
    const long long o = W.mutBase[k] + m;
    S.sumF[o] = sumF;
    S.sumR[o] = sumR;
    S.nF[o] = nF;
    S.nR[o] = nR;
}

__global__ void __launch_bounds__(256) k_strand_sites(ScoreWork W, const long long* __restrict__ posBase,
                                                      const int* __restrict__ posOff, StrandSums S,
                                                      const long long* __restrict__ qvBase, double minScore,
                                                      int minReads, StrandSiteOut out)
{
    const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= W.posStart[W.nWork]) return;
    int lo = 0, hi = W.nWork;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (W.posStart[mid] <= g) lo = mid; else hi = mid;
    }
    const int k = lo;
    const int p = (int)(g - W.posStart[k]);
    const int* po = posOff + posBase[k];
    const long long mb = W.mutBase[k];
    int best = -1;
    double bestV = 0.0;
    for (int m = po[p]; m < po[p + 1]; ++m) {
        const double f = S.sumF[mb + m], r = S.sumR[mb + m];
        if (S.nF[mb + m] < minReads || S.nR[mb + m] < minReads) continue;
        // (a NaN sum fails both comparisons)
        if (!((f > minScore && r < -minScore) || (r > minScore && f < -minScore))) continue;
        const double v = fmin(fabs(f), fabs(r));
        if (best < 0 || v > bestV) {
            best = m;
            bestV = v;
        }
    }
    const long long o = qvBase[k] + p;
    out.flag[o] = best >= 0 ? 1 : 0;
    out.code[o] = best >= 0 ? W.codes[mb + best] : 0;
    out.sumF[o] = best >= 0 ? S.sumF[mb + best] : 0.0;
    out.sumR[o] = best >= 0 ? S.sumR[mb + best] : 0.0;
}

}  // namespace

void launch_strand_sums(const DevBatch& B, const ScoreWork& W, long long nMut, const StrandSums& S, hipStream_t s)
{
    if (nMut <= 0) return;
    hipLaunchKernelGGL(k_strand_sums, dim3((unsigned)((nMut + 255) / 256)), dim3(256), 0, s, B, W, S);
}

void launch_strand_sites(const ScoreWork& W, long long nPos, const long long* posBase, const int* posOff,
                         const StrandSums& S, const long long* qvBase, double minScore, int minReads,
                         const StrandSiteOut& out, hipStream_t s)
{
    if (nPos <= 0) return;
    hipLaunchKernelGGL(k_strand_sites, dim3((unsigned)((nPos + 255) / 256)), dim3(256), 0, s, W, posBase, posOff, S,
                       qvBase, minScore, minReads, out);
}

}  // namespace pbccs

// pbccs_amd/csrc/arrow_wide_kernels.hip -- Arrow scoring of mutations of any width.
//
//   k_score_wide  one lane per (mutation, read) task of a list the host wrote: MutationScorer::ScoreMutation's four
//                 cases (MutationScorer.cpp:185-267) with general lengths over the wide template view, minus the
//                 read's baseline.  The reference's scorer refuses |LengthDiff| > 1 (:181-183) and its template
//                 keeps two mutant slots; the extend / link code behind the guard is already written for any
//                 length, and it is that code, instantiated for eight extension columns, that runs here.
//   k_score_wide_refill  the fourth case, the whole refill of the mutated window, in a kernel of its own: tiny
//                 windows as in the reference, and every mutation three or more bases wide.
//
// The host orients and clips each mutation for its read (OrientedMutation, MultiReadMutationScorer.cpp:93-139) and
// has checked the 8-column rule, so a task carries window coordinates.  Reads with checkpointed bands are not
// scored here (their columns are not stored): the host refuses them.
#include "arrow_device.hpp"
#include "arrow_kernels.hpp"
#include "arrow_score_device.hpp"

namespace pbccs {

constexpr int kWideExtCols = kWideExtColumns;

// the view and scoring context of a task
__device__ __forceinline__ void wide_setup(const DevBatch& B, const WideTask& w, ScoreCtxT<TplViewWide>& S)
{
    const int r = w.r;
    const int z = B.rZmw[r];
    S.B = &B;
    S.P = params_for(B, z);
    S.rd = B.seqPool + B.rSeqOff[r];
    S.I = B.rLen[r];
    S.Jorig = B.rTe[r] - B.rTs[r];
    S.a = band_alpha(B, r);
    S.b = band_beta(B, r);
    const long long cbase = B.rColBase[r];
    S.aPre = B.aPre + cbase;
    S.bSuf = B.bSuf + cbase;
    const TplView plain = window_view(B, r);
    S.tv.T = plain.T;
    S.tv.L = plain.L;
    S.tv.start = plain.start;
    S.tv.len = plain.len;
    S.tv.ms = plain.start + w.os;
    S.tv.nOld = w.oe - w.os;
    S.tv.nb = w.nb;
    S.tv.bases = w.bases;
}

__device__ __forceinline__ double wide_nan() { return __longlong_as_double(0x7ff8000000000001LL); }

__global__ void __launch_bounds__(64) k_score_wide(DevBatch B, const WideTask* __restrict__ tasks, int n,
                                                   double* __restrict__ delta)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const WideTask w = tasks[t];
    const int r = w.r;
    ScoreCtxT<TplViewWide> S;
    wide_setup(B, w, S);

    const int J = S.Jorig;
    const int os = w.os, oe = w.oe;
    const int ld = w.nb - (oe - os);   // LengthDiff
    const int Jv = S.tv.Length();
    const int extra = max(abs(ld) - 1, 0);   // neighbour columns whose row ranges an extension column adds
    const bool atBegin = os < 3;
    const bool atEnd = oe > J - 2;
    TaskStat st;
    double score = wide_nan();
    // the host's column rule, checked again: a task outside it leaves NaN and touches nothing
    const bool sane = os >= 0 && oe >= os && oe <= J && w.nb >= 0 && w.nb <= 8 && Jv >= 1;
    if (sane && wide_task_refills(os, oe, w.nb, J)) {
        // (k_score_wide_refill's: the host lists such tasks there; NaN if one arrives here)
    } else if (sane && !atBegin) {
        // middle: ExtendAlpha over 1 + |bases'| columns (2 from os - 1 for a deletion), then LinkAlphaBeta;
        // at the end: ExtendAlpha from os - 1 to the end
        int sc, nc;
        if (atEnd) {
            sc = os - 1;
            nc = Jv - sc + 1;
        } else {
            sc = (w.type == kDel) ? os - 1 : os;
            nc = (w.type == kDel) ? 2 : 1 + w.nb;
        }
        if (nc >= (atEnd ? 1 : 2) && nc <= kWideExtCols)
            score = extend_alpha_score<TplViewWide, kWideExtCols>(S, sc, nc, !atEnd, 1 + oe, 1 + oe + ld, st, extra);
    } else if (sane && !atEnd) {
        const int nExt = ld + oe + 1;
        if (nExt >= 1 && nExt <= kWideExtCols) score = extend_beta_score<TplViewWide, kWideExtCols>(S, oe, ld, st, extra);
    }
    delta[w.slot] = score - B.rBaseline[r];   // (no work counters: stats[kStatScore] is k_score's roofline)
}

// The whole refill of the mutated window, for the tasks wide_task_refills() names: the reference's last case (both
// ends within reach: tiny windows, MutationScorer.cpp:246-266) and every mutation kWideRefillWidth or more bases
// wide.  Such a mutation moves the likely path three or more rows, into cells that the fills of the unmutated
// template cut away (exp(-ScoreDiff) of each column's maximum): through the stored bands its score lay up to 5e-3
// from a refill's.  The refill bands itself around the mutated template; for the wide mutations
// it is FillAlphaBeta's first round: alpha guided by the stored alpha and beta ranges carried over to the new
// columns, then beta guided by that alpha (an unguided single alpha pass can lose the pinned last cell, which the
// reference's fills repair with their alpha / beta flip-flops).
// A kernel of its own: fill_alpha's state beside eight extension columns needs a private segment.
__global__ void __launch_bounds__(64) k_score_wide_refill(DevBatch B, const WideTask* __restrict__ tasks, int n,
                                                          double* __restrict__ delta, ScoreScratch scratch, int rowsCap)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const WideTask w = tasks[t];
    const int r = w.r;
    ScoreCtxT<TplViewWide> S;
    wide_setup(B, w, S);
    const int J = S.Jorig;
    const int os = w.os, oe = w.oe;
    const int ld = w.nb - (oe - os);
    const int Jv = S.tv.Length();
    const int width = max(w.nb, oe - os);
    double score = wide_nan();
    const bool sane = os >= 0 && oe >= os && oe <= J && w.nb >= 0 && w.nb <= 8 && Jv >= 1;
    Band m;
    int2* gr = nullptr;
    const long long ncol = (long long)Jv + 1;
    if (sane && scratch_band_take(scratch, ncol, min((long long)S.I + 1, (long long)rowsCap), &m, &gr)) {
        // The guide: new column j is old column j before the mutation and old column j - ld behind it, the columns
        // of the new bases are the old columns [os, oe]; one neighbour on either side, `width` more around the
        // mutation.  Without a guide (tiny windows, as the reference) every range is empty.
        const bool guided = width >= kWideRefillWidth;
        for (int j = 0; j <= Jv; ++j) {
            int lo = j, hi = j;
            if (j > os + w.nb) lo = hi = j - ld;
            else if (j >= os) { lo = os; hi = oe; }
            const int reach = 1 + ((j >= os - width && j <= os + w.nb + width) ? width : 0);
            lo = max(lo - reach, 0);
            hi = min(hi + reach, J);
            int b = S.I + 1, e = 0;
            for (int c = lo; guided && c <= hi; ++c) {
                const int2 ra = S.a.range[c], rb = S.b.range[c];
                if (ra.x < ra.y) { b = min(b, ra.x); e = max(e, ra.y); }
                if (rb.x < rb.y) { b = min(b, rb.x); e = max(e, rb.y); }
            }
            gr[j] = (b < e) ? make_int2(b, e) : make_int2(0, 0);
        }
        Band guide = m;
        guide.range = gr;
        const long long u = fill_alpha(S.tv, S.rd, S.I, m, &guide, false, S.P);
        if (u < 0) {
            atomicOr(scratch.overflow, 4);   // the band outgrew rowsCap values per column: the host raises it
        } else if (!guided) {
            score = log(alpha_at(m, S.I, Jv)) + sum_ls(m, Jv + 1);   // the reference's read-out of its whole fill
        } else {
            // FillAlphaBeta's second half: beta inside alpha's ranges, read out as Score() reads the baseline it is
            // compared with (log beta(0, 0) + beta's log-scales), so the two sides of the difference are cut alike
            Band bm;
            int2* unused = nullptr;
            if (scratch_band_take(scratch, ncol, min((long long)S.I + 1, (long long)rowsCap), &bm, &unused)) {
                const long long ub = fill_beta(S.tv, S.rd, S.I, bm, &m, false, S.P);
                if (ub < 0) atomicOr(scratch.overflow, 4);
                else score = log(beta_at(bm, 0, 0)) + sum_ls(bm, Jv + 1);
            }
        }
    }
    delta[w.slot] = score - B.rBaseline[r];
}

void launch_score_wide(const DevBatch& B, const WideTask* tasks, int n, double* delta, hipStream_t s)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(k_score_wide, dim3((n + 63) / 64), dim3(64), 0, s, B, tasks, n, delta);
}

void launch_score_wide_refill(const DevBatch& B, const WideTask* tasks, int n, double* delta,
                              const ScoreScratch& scratch, int rowsCap, hipStream_t s)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(k_score_wide_refill, dim3((n + 63) / 64), dim3(64), 0, s, B, tasks, n, delta, scratch, rowsCap);
}

}  // namespace pbccs

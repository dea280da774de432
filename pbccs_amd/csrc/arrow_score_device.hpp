// pbccs_amd/csrc/arrow_score_device.hpp -- the per-lane pieces of MutationScorer::ScoreMutation that the scoring
// kernels of arrow_kernels.hip (single-base, four extension columns, TplView) and arrow_wide_kernels.hip (any
// width, eight columns, TplViewWide) share: the scoring context of a (mutation, read) task, ExtendAlpha followed
// by the link or the at-end read-out, and ExtendBeta.  Templates over the template view and the column cap C.
#pragma once

#include <climits>

#include "arrow_device.hpp"
#include "arrow_kernels.hpp"

namespace pbccs {

// ------------------------------------------------------------------------------------------------
// helpers
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ Params params_for(const DevBatch& B, int z)
{
    Params P;
    P.ctx = B.zCtx + (long long)z * 9 * kCtxStride;
    P.prNot = B.prNot;
    P.prThird = B.prThird;
    P.sdn = B.sdn;
    return P;
}

__device__ __forceinline__ Band band_alpha(const DevBatch& B, int r)
{
    const long long cb = B.rColBase[r];
    Band m;
    m.range = B.aRange + cb;
    m.off = B.aOff + cb;
    m.ls = B.aLs + cb;
    m.val = B.valPool + B.rValA[r];
    m.cap = B.rValCap[r];
    return m;
}

__device__ __forceinline__ Band band_beta(const DevBatch& B, int r)
{
    const long long cb = B.rColBase[r];
    Band m;
    m.range = B.bRange + cb;
    m.off = B.bOff + cb;
    m.ls = B.bLs + cb;
    m.val = B.valPool + B.rValB[r];
    m.cap = B.rValCap[r];
    return m;
}

// ------------------------------------------------------------------------------------------------
// Mutation scoring
// ------------------------------------------------------------------------------------------------
template <class View>
struct ScoreCtxT {
    const DevBatch* B;
    Params P;
    const char* rd;
    int I;
    int Jorig;   // unmutated window length (alpha/beta have Jorig + 1 columns)
    View tv;
    Band a, b;
    const double* aPre;
    const double* bSuf;
};
using ScoreCtx = ScoreCtxT<TplView>;

// ExtendAlpha (SimpleRecursor.cpp:373-487) over n <= C columns starting at `sc`, followed either by
// LinkAlphaBeta (:306-357, middle case) or by the at-end read-out (MutationScorer.cpp:219-231).
// ext columns are never stored: sweep t recomputes columns 0..t-1 (scales known) and column t (its
// max = the FinishEditingColumn constant); a final sweep produces the link sum.  Every recomputation
// performs the same operations in the same order, so the values are bit-identical to a stored matrix.
// C == kMaxExtCols is the single-base instantiation: it links after n == 2 columns only, and no column lies
// past the stored alpha.  The wide instantiation (C == 8) links after any n (LinkAlphaBeta reads ext columns
// n - 2 and n - 1).  There a column j > Jorig has no stored alpha range (the reference's ExtendAlpha would read
// UsedRowRange out of bounds): below the mutated template's last column it runs from the last interior alpha
// column's first row to the read's end, and the last column keeps the reference's pinned row.
// `extra` (wide only): a mutation of length difference ld moves the columns behind it by |ld|, so an extension
// column takes the union of the stored ranges of |ld| - 1 more neighbours on either side than the reference's one;
// 0 for |ld| <= 1, which keeps width 1 on the reference's rows.
template <class View, int C>
__device__ double extend_alpha_score(const ScoreCtxT<View>& S, int sc, int n, bool link, int bc, int absc, TaskStat& st,
                                     int extra = 0)
{
    const int I = S.I;
    const int Jv = S.tv.Length();
    const int Jr = (C == kMaxExtCols) ? Jv : min(Jv, S.Jorig + 1);   // columns below Jr have a stored alpha range
    int cb[C], ce[C], jj[C];
    char cur[C], nxt[C];
    double pM[C], pD[C], cB[C], cS3[C];
#pragma unroll
    for (int c = 0; c < C; ++c) {
        cb[c] = 0; ce[c] = 0; jj[c] = 0; cur[c] = 0; nxt[c] = 0;
        pM[c] = 0.0; pD[c] = 0.0; cB[c] = 0.0; cS3[c] = 0.0;
        if (c < n) {
            const int j = sc + c;
            jj[c] = j;
            int b, e;
            if (j < Jr) {
                const int2 r0 = S.a.range[j];
                b = r0.x; e = r0.y;
                if (j - 1 >= 0) { const int2 r1 = S.a.range[j - 1]; b = min(b, r1.x); e = max(e, r1.y); }
                if (j + 1 < Jr) { const int2 r2 = S.a.range[j + 1]; b = min(b, r2.x); e = max(e, r2.y); }
                if (C != kMaxExtCols)
                    for (int q = 2; q <= 1 + extra; ++q) {
                        if (j - q >= 0) { const int2 r = S.a.range[j - q]; b = min(b, r.x); e = max(e, r.y); }
                        if (j + q < Jr) { const int2 r = S.a.range[j + q]; b = min(b, r.x); e = max(e, r.y); }
                    }
            } else {
                b = S.a.range[(C != kMaxExtCols && j < Jv) ? max(S.Jorig - 1, 0) : S.Jorig].x;
                e = I + 1;
            }
            cb[c] = b; ce[c] = e;
            char cbase; int cctx;
            S.tv.At(j - 1, cbase, cctx);
            cur[c] = cbase;
            const double* cp = S.P.P(cctx);
            cB[c] = cp[kB]; cS3[c] = cp[kS3];
            const int pctx = (j > 1) ? S.tv.Ctx(j - 2) : kCtxZero;
            pM[c] = S.P.P(pctx)[kM];
            pD[c] = S.P.P(pctx)[kD];
            if (j != Jv) nxt[c] = S.tv.Base(j);
        }
    }
    // alpha column sc-1 feeds ext column 0
    const int2 ar = S.a.range[sc - 1];
    const double* av = S.a.val + S.a.off[sc - 1] - ar.x;

    // link setup
    int lb = 0, le = 0;
    char linkBase = 0;
    double lM = 0.0, lD = 0.0;
    int2 br = make_int2(0, 0);
    const double* bv = nullptr;
    if (link) {
        if (C == kMaxExtCols) {
            lb = min(cb[0], cb[1]); le = max(ce[0], ce[1]);
        } else {
            lb = INT_MAX; le = INT_MIN;
#pragma unroll
            for (int c = 0; c < C; ++c)
                if (c == n - 2 || c == n - 1) { lb = min(lb, cb[c]); le = max(le, ce[c]); }
        }
        const int2 b0 = S.b.range[bc], b1 = S.b.range[bc + 1];
        lb = min(lb, min(b0.x, b1.x));
        le = max(le, max(b0.y, b1.y));
        linkBase = S.tv.Base(absc - 1);
        const int lctx = S.tv.Ctx(absc - 2);
        lM = S.P.P(lctx)[kM];
        lD = S.P.P(lctx)[kD];
        br = b0;
        bv = S.b.val + S.b.off[bc] + (b0.y - 1);   // bv[-i] = beta(i, bc)
    }

    double Cs[C], ls[C];
    bool scl[C];
#pragma unroll
    for (int c = 0; c < C; ++c) { Cs[c] = 0.0; ls[c] = 0.0; scl[c] = false; }
    double rawAtI = 0.0;
    double v = 0.0;
    const int nSweeps = link ? n + 1 : n;
    for (int t = 0; t < nSweeps; ++t) {
        const int top = min(t, n - 1);   // highest column computed in this sweep
        int lo, hi;
        if (t == n) { lo = lb; hi = le; }
        else {
            lo = cb[0]; hi = ce[0];
#pragma unroll
            for (int c = 1; c < C; ++c)
                if (c <= top) { lo = min(lo, cb[c]); hi = max(hi, ce[c]); }
        }
        double rawPrev[C], scPrev[C];
#pragma unroll
        for (int c = 0; c < C; ++c) { rawPrev[c] = 0.0; scPrev[c] = 0.0; }
        double Ct = 0.0;
        for (int i = lo; i < hi; ++i) {
            const double aD = (i - 1 >= ar.x && i - 1 < ar.y) ? av[i - 1] : 0.0;
            const double aL = (i >= ar.x && i < ar.y) ? av[i] : 0.0;
            const char rb = (i >= 1 && i - 1 < I) ? S.rd[i - 1] : (char)0;
            double rawCur[C], scCur[C];
#pragma unroll
            for (int c = 0; c < C; ++c) {
                rawCur[c] = 0.0;
                scCur[c] = 0.0;
                if (c <= top) {
                    const int j = jj[c];
                    const double pd = (c == 0) ? aD : scPrev[c > 0 ? c - 1 : 0];
                    const double pl = (c == 0) ? aL : scCur[c > 0 ? c - 1 : 0];
                    double raw = 0.0;
                    const bool in = (i >= cb[c] && i < ce[c]);
                    if (in) {
                        double s;
                        if (i > 0 && j > 0) {
                            const double em = (rb == cur[c]) ? S.P.prNot : S.P.prThird;
                            double mv = 0.0;
                            if (i == 1 && j == 1) mv = em;
                            else if (i < I && j < Jv) mv = pd * pM[c] * em;
                            else if (i == I && j == Jv) mv = pd * em;
                            s = mv;
                        } else {
                            s = rawPrev[c];   // the reference's `score` carries over (never taken: i >= 1)
                        }
                        if (i > 1 && i < I && j != Jv) s = s + rawPrev[c] * (nxt[c] == rb ? cB[c] : cS3[c]);
                        if (j > 1 && j < Jv && i != I) s = s + pl * pD[c];
                        raw = s;
                    }
                    rawCur[c] = raw;
                    if (c < t) {
                        scCur[c] = in ? (scl[c] ? raw / Cs[c] : raw) : 0.0;
                    } else if (in) {   // c == t < n: the column whose scale this sweep determines
                        if (Ct < raw) Ct = raw;
                        if (i == I) rawAtI = raw;
                    }
                }
            }
            if (t == n) {
                double s1;
                if (C == kMaxExtCols) {
                    s1 = scCur[1];
                } else {
                    s1 = 0.0;
#pragma unroll
                    for (int c = 0; c < C; ++c)
                        if (c == n - 1) s1 = scCur[c];
                }
                if (i < I) {
                    const double mprob = lM * (S.rd[i] == linkBase ? S.P.prNot : S.P.prThird);
                    const double bn = (i + 1 >= br.x && i + 1 < br.y) ? bv[-(i + 1)] : 0.0;
                    v = v + s1 * mprob * bn;
                }
                const double bh = (i >= br.x && i < br.y) ? bv[-i] : 0.0;
                v = v + s1 * lD * bh;
            }
#pragma unroll
            for (int c = 0; c < C; ++c) { rawPrev[c] = rawCur[c]; scPrev[c] = scCur[c]; }
        }
        if (t < n) {
#pragma unroll
            for (int c = 0; c < C; ++c)
                if (c == t) {
                    Cs[c] = Ct;
                    scl[c] = (Ct != 0.0 && Ct != 1.0);
                    ls[c] = scl[c] ? log(Ct) : 0.0;
                }
        }
    }
    double E = 0.0;
#pragma unroll
    for (int c = 0; c < C; ++c)
        if (c < n) {
            E = E + ls[c];
            st.cells += (unsigned long long)max(0, ce[c] - cb[c]);
        }
    st.bytes += 8ull * (unsigned long long)max(0, ar.y - ar.x) + 16ull * (unsigned long long)(n + 2);
    if (link) {
        st.cells += (unsigned long long)max(0, le - lb);
        st.bytes += 8ull * (unsigned long long)max(0, br.y - br.x) + 32ull;
        return ((log(v) + E) + S.bSuf[bc]) + S.aPre[sc];
    }
    // at-end read-out: ext(I, n-1)
    double lastC = 0.0, lastRange = 0.0;
    bool lastScl = false;
    int lastB = 0, lastE = 0;
#pragma unroll
    for (int c = 0; c < C; ++c)
        if (c == n - 1) { lastC = Cs[c]; lastScl = scl[c]; lastB = cb[c]; lastE = ce[c]; }
    (void)lastRange;
    double extI = 0.0;
    if (I >= lastB && I < lastE) extI = lastScl ? rawAtI / lastC : rawAtI;
    return (log(extI) + S.aPre[sc]) + E;
}

// ExtendBeta (SimpleRecursor.cpp:509-628) back to column 0 for mutations near the template start,
// read out as in MutationScorer.cpp:233-245.  Columns are filled high to low, rows bottom-up.
template <class View, int C>
__device__ double extend_beta_score(const ScoreCtxT<View>& S, int lastCol, int ld, TaskStat& st, int extra = 0)
{
    const int I = S.I;
    const int Jv = S.tv.Length();
    const int nExt = ld + lastCol + 1;
    const int firstCol = -ld;
    const int lastExt = nExt - 1;
    int cb[C], ce[C], jj[C], jpv[C];
    char nxt[C];
    double cM[C], cD[C], cB[C], cS3[C];
#pragma unroll
    for (int c = 0; c < C; ++c) {
        cb[c] = 0; ce[c] = 0; jj[c] = 0; jpv[c] = 0; nxt[c] = 0;
        cM[c] = 0.0; cD[c] = 0.0; cB[c] = 0.0; cS3[c] = 0.0;
        if (c < nExt) {
            const int j = c + firstCol;
            const int jp = j + ld;
            jj[c] = j; jpv[c] = jp;
            int b, e;
            if (j < 0) {
                // (wide only: a column between the first one and beta's column 0 has no stored range either; it
                // runs from the read's start to the first interior beta column's last row)
                b = 0;
                e = S.b.range[(C != kMaxExtCols && j > firstCol) ? min(1, S.Jorig) : 0].y;
            } else {
                const int2 r0 = S.b.range[j];
                b = r0.x; e = r0.y;
                if (j - 1 >= 0) { const int2 r1 = S.b.range[j - 1]; b = min(b, r1.x); e = max(e, r1.y); }
                if (j + 1 < Jv) { const int2 r2 = S.b.range[j + 1]; b = min(b, r2.x); e = max(e, r2.y); }
                if (C != kMaxExtCols)   // (as extend_alpha_score's `extra`)
                    for (int q = 2; q <= 1 + extra; ++q) {
                        if (j - q >= 0) { const int2 r = S.b.range[j - q]; b = min(b, r.x); e = max(e, r.y); }
                        if (j + q <= S.Jorig) { const int2 r = S.b.range[j + q]; b = min(b, r.x); e = max(e, r.y); }
                    }
            }
            cb[c] = b; ce[c] = e;
            nxt[c] = S.tv.Base(jp);
            const int cctx = (jp > 0) ? S.tv.Ctx(jp - 1) : kCtxZero;
            const double* cp = S.P.P(cctx);
            cM[c] = cp[kM]; cD[c] = cp[kD]; cB[c] = cp[kB]; cS3[c] = cp[kS3];
        }
    }
    // beta column lastCol + 1 feeds ext column lastExt
    const int2 br = S.b.range[lastCol + 1];
    const double* bv = S.b.val + S.b.off[lastCol + 1] + (br.y - 1);   // bv[-i] = beta(i, lastCol+1)

    double Cs[C], ls[C];
    bool scl[C];
#pragma unroll
    for (int c = 0; c < C; ++c) { Cs[c] = 0.0; ls[c] = 0.0; scl[c] = false; }
    double rawAt0 = 0.0;
    for (int t = lastExt; t >= 0; --t) {
        int lo = cb[lastExt], hi = ce[lastExt];
#pragma unroll
        for (int c = 0; c < C; ++c)
            if (c >= t && c < nExt) { lo = min(lo, cb[c]); hi = max(hi, ce[c]); }
        double rawPrev[C], scPrev[C];   // values at row i+1
#pragma unroll
        for (int c = 0; c < C; ++c) { rawPrev[c] = 0.0; scPrev[c] = 0.0; }
        double Ct = 0.0;
        for (int i = hi - 1; i >= lo; --i) {
            const double bN = (i + 1 >= br.x && i + 1 < br.y) ? bv[-(i + 1)] : 0.0;   // beta(i+1, lastCol+1)
            const double bH = (i >= br.x && i < br.y) ? bv[-i] : 0.0;                 // beta(i, lastCol+1)
            const char nb = (i < I) ? S.rd[i] : 'N';
            double rawCur[C], scCur[C];
#pragma unroll
            for (int c = 0; c < C; ++c) { rawCur[c] = 0.0; scCur[c] = 0.0; }
#pragma unroll
            for (int cc = C - 1; cc >= 0; --cc) {
                if (cc >= t && cc < nExt) {
                    const int j = jj[cc], jp = jpv[cc];
                    const double nxD = (cc == lastExt) ? bN : scPrev[cc + 1 < C ? cc + 1 : cc];
                    const double nxH = (cc == lastExt) ? bH : scCur[cc + 1 < C ? cc + 1 : cc];
                    const bool in = (i >= cb[cc] && i < ce[cc]);
                    double raw = 0.0;
                    if (in) {
                        const bool same = nb == nxt[cc];
                        double s = 0.0;
                        if (i < I && j < Jv) {
                            const double em = same ? S.P.prNot : S.P.prThird;
                            double mv = 0.0;
                            if ((i == I - 1 && jp == Jv - 1) || (i == 0 && j == firstCol)) mv = nxD * em;
                            else if (j > firstCol && i > 0) mv = nxD * cM[cc] * em;
                            s = 0.0 + mv;
                        }
                        if (i < I - 1 && i > 0 && j > firstCol) s = s + rawPrev[cc] * (same ? cB[cc] : cS3[cc]);
                        if (j < Jv - 1 && j > firstCol && i > 0) s = s + nxH * cD[cc];
                        raw = s;
                    }
                    rawCur[cc] = raw;
                    if (cc > t) {
                        scCur[cc] = in ? (scl[cc] ? raw / Cs[cc] : raw) : 0.0;
                    } else if (in) {
                        if (Ct < raw) Ct = raw;
                        if (i == 0) rawAt0 = raw;
                    }
                }
            }
#pragma unroll
            for (int c = 0; c < C; ++c) { rawPrev[c] = rawCur[c]; scPrev[c] = scCur[c]; }
        }
#pragma unroll
        for (int c = 0; c < C; ++c)
            if (c == t) {
                Cs[c] = Ct;
                scl[c] = (Ct != 0.0 && Ct != 1.0);
                ls[c] = scl[c] ? log(Ct) : 0.0;
            }
    }
    double E = 0.0;
#pragma unroll
    for (int c = 0; c < C; ++c)
        if (c < nExt) {
            E = E + ls[c];
            st.cells += (unsigned long long)max(0, ce[c] - cb[c]);
        }
    st.bytes += 8ull * (unsigned long long)max(0, br.y - br.x) + 16ull * (unsigned long long)(nExt + 2);
    const double ext00 = (0 >= cb[0] && 0 < ce[0]) ? (scl[0] ? rawAt0 / Cs[0] : rawAt0) : 0.0;
    return (log(ext00) + S.bSuf[lastCol + 1]) + E;
}

// The bump scratch of the whole-window refill (MutationScorer.cpp:246-266): a band of ncol columns with room for
// `rows` values per column on average, and beside it ncol row ranges for a fill guide (*guide).  Returns false (and
// flags the overflow for the host's grow-and-rerun) when the pool is full.
__device__ __forceinline__ bool scratch_band_take(const ScoreScratch& scratch, long long ncol, long long rows, Band* m,
                                                  int2** guide)
{
    const long long need = ncol * rows + 4 * ncol + 16;
    const unsigned long long at = atomicAdd(scratch.top, (unsigned long long)need);
    if (at + need > scratch.cap) {
        atomicOr(scratch.overflow, 1);
        return false;
    }
    double* base0 = scratch.pool + at;
    m->ls = base0;
    m->range = reinterpret_cast<int2*>(base0 + ncol);
    m->off = reinterpret_cast<int*>(base0 + 2 * ncol);    // ncol ints: half of [2 ncol, 3 ncol)
    *guide = reinterpret_cast<int2*>(base0 + 3 * ncol);
    m->val = base0 + 4 * ncol;
    m->cap = ncol * rows;
    return true;
}

}  // namespace pbccs

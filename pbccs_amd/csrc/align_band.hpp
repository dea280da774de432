// pbccs_amd/csrc/align_band.hpp -- the certified band of the pairwise aligners: its geometry, the bound U(w) on
// every path that leaves it, the rounding margin E and the widening schedule.  Host code, no device needed
// (DESIGN.md §3.19).
//
// The query is on rows i, the target on columns j; a cell's diagonal is d = j - i and delta = J - I.  A band of
// half-width w holds the diagonals lo <= d <= hi, lo = min(0, delta) - w, hi = max(0, delta) + w, so it always holds
// (0, 0) and (I, J).  A path that leaves it reaches diagonal hi + 1 (side 1) or lo - 1 (side 2):
//   side 1: at least D1 = hi + 1 deletes (left moves) and N1 = hi + 1 - delta inserts (up moves),
//   side 2: at least N2 = 1 - lo inserts and D2 = 1 - lo + delta deletes,
// and J - D diagonal moves.  With s+ the largest diagonal score:
//   NW:     U_k = s+ (J - D_k) + D_k Delete + N_k Insert,      valid when Insert + Delete <= s+,
//   affine: U_k = s+ (J - D_k) + (D_k + N_k) g+, g+ = max(GapOpen, GapExtend), valid when 2 g+ <= s+
// (every further delete comes with a further insert and takes a diagonal move away; the conditions say that this
// never pays).  A side whose diagonal lies outside the matrix (D_k > J or N_k > I) has no path: U_k = -inf.
// A banded fill with final score S is certified iff S > U(w) + E, strictly: then no path outside the band reaches S.
#pragma once

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <limits>

#include "align_kernels.hpp"

namespace pbccs {
namespace align {

constexpr int kBandAutoMargin = 32;       // auto w0: |delta| is in every band; 32 more diagonals either side.  The 32
                                          // affects only speed (how often a second attempt is needed), never a result
constexpr int kNwDead = -(1 << 30);       // NW dead-cell value: below every real score, and one add cannot wrap it
constexpr double kAffineMaxParamSum = 0x1p100;   // (I + J + 1) max|param| below this: -FLT_MAX absorbs every sum

// fallback reasons (PBCCS_BAND_*)
constexpr int kBandNone = 0, kBandNotCertifiable = 1, kBandCoversMatrix = 2, kBandStoreNotSmaller = 3,
              kBandTraceFlagged = 4, kBandUncertified = 5, kBandDegenerate = 6, kBandOverBudget = 7;

struct BandGeom {
    long long lo, hi;
};

inline BandGeom band_geom(int I, int J, long long w)
{
    const long long delta = (long long)J - I;
    const long long cap = (long long)std::max(I, J) + 1;   // wider changes nothing
    const long long ww = std::min(std::max(w, 0LL), cap);
    return BandGeom{std::min(0LL, delta) - ww, std::max(0LL, delta) + ww};
}

// both edge diagonals lie outside the matrix: the band is the whole matrix
inline bool band_covers(int I, int J, const BandGeom& g) { return g.hi + 1 > J && 1 - g.lo > I; }

// cells (i, j), 1 <= i <= I, 1 <= j <= J, inside the band
inline long long band_cells(int I, int J, const BandGeom& g)
{
    long long c = 0;
    for (int i = 1; i <= I; ++i) {
        const long long a = std::max(1LL, (long long)i + g.lo), b = std::min((long long)J, (long long)i + g.hi);
        if (b >= a) c += b - a + 1;
    }
    return c;
}

// steps of one strip's store: its column window (at most 64 R + hi - lo columns, never more than J) plus the skew of
// the lanes that own rows (all 64 unless the pair is a single short strip)
inline long long band_steps(int I, int J, int R, const BandGeom& g)
{
    const long long lanes = std::min(64LL, ((long long)I + R - 1) / R);
    return std::min((long long)J, 64LL * R + g.hi - g.lo) + lanes - 1;
}

inline long long band_store_bytes(int I, int J, int R, const BandGeom& g)
{
    const long long strips = (I + 64LL * R - 1) / (64LL * R);
    return strips * band_steps(I, J, R, g) * 64LL * R;
}

struct BandBound {
    double U = 0.0, E = 0.0;
    bool certifiable = false;
};

namespace band_detail {

// exponent of the lowest set bit of a finite non-zero float: x is an odd multiple of 2^that
inline int low_bit_exp(float x)
{
    int e;
    double m = std::frexp((double)std::fabs(x), &e);   // x = m 2^e, 0.5 <= m < 1
    while (m != std::floor(m)) {
        m *= 2.0;
        --e;
    }
    return e;
}

}  // namespace band_detail

// U(w), E and whether the pair can be certified at all with these parameters.
inline BandBound band_bound(const AlignScoring& p, int I, int J, long long w)
{
    BandBound r;
    const BandGeom g = band_geom(I, J, w);
    const double delta = (double)J - I;
    const double D[2] = {(double)g.hi + 1, 1.0 - g.lo + delta};
    const double N[2] = {(double)g.hi + 1 - delta, 1.0 - g.lo};
    const double n = (double)I + J;
    const double inf = std::numeric_limits<double>::infinity();
    double U = -inf;
    if (p.kind == kNw) {
        const double sp = std::max(p.match, p.mismatch);
        const double mx = std::max(std::max(std::fabs((double)p.match), std::fabs((double)p.mismatch)),
                                   std::max(std::fabs((double)p.insert), std::fabs((double)p.delete_)));
        r.certifiable = (double)p.insert + (double)p.delete_ <= sp && (n + 1) * mx <= (double)(1 << 30);
        for (int k = 0; k < 2; ++k)
            if (D[k] <= J && N[k] <= I) U = std::max(U, sp * (J - D[k]) + D[k] * p.delete_ + N[k] * p.insert);
        r.E = 0.0;
    } else {
        float v[5] = {p.matchScore, p.mismatchScore, p.gapOpen, p.gapExtend, p.partial};
        const int nv = p.kind == kAffineIupac ? 5 : 4;
        double sp = std::max((double)p.matchScore, (double)p.mismatchScore);
        if (p.kind == kAffineIupac) sp = std::max(sp, (double)p.partial);
        const double gp = std::max((double)p.gapOpen, (double)p.gapExtend);
        double mx = 0.0;
        bool finite = true;
        for (int k = 0; k < nv; ++k) {
            finite = finite && std::isfinite(v[k]);
            mx = std::max(mx, std::fabs((double)v[k]));
        }
        const double B = (n + 1) * mx;
        r.certifiable = finite && 2.0 * gp <= sp && B < kAffineMaxParamSum;
        for (int k = 0; k < 2; ++k)
            if (D[k] <= J && N[k] <= I) U = std::max(U, sp * (J - D[k]) + (D[k] + N[k]) * gp);
        // E = 0 when every parameter is a multiple of one power of two q and (I + J + 1) max|param| / q <= 2^24:
        // every partial sum is then a multiple of q below 2^24 q, and every float32 add is exact
        bool exact = finite;
        if (finite && mx > 0.0) {
            int q = INT32_MAX;
            for (int k = 0; k < nv; ++k)
                if (v[k] != 0.f) q = std::min(q, band_detail::low_bit_exp(v[k]));
            exact = std::ldexp(B, -q) <= 16777216.0;
        }
        if (exact) {
            r.E = 0.0;
        } else {
            // n float32 adds, partial sums within B: each rounds by at most u B', so n u B / (1 - n u), u = 2^-24;
            // the last term covers the double arithmetic of U itself
            const double u = 0x1p-24;
            r.E = n * u >= 0.5 ? inf : n * u * B / (1.0 - n * u) + 0x1p-48 * B;
            if (!(r.E < inf)) r.certifiable = false;
        }
    }
    r.U = U;
    return r;
}

inline bool band_certified(const BandBound& b, double score) { return b.certifiable && score > b.U + b.E; }

// the smallest w whose band certifies a banded score `score` (a lower bound of the full score), -1 when the pair
// cannot be certified.  U(w) does not grow with w, so the answer is found by bisection; at w = max(I, J) no path
// leaves the band and U = -inf.
inline long long band_widen(const AlignScoring& p, int I, int J, double score)
{
    if (!band_bound(p, I, J, 0).certifiable || !std::isfinite(score)) return -1;
    long long a = 0, b = std::max(I, J);
    if (!band_certified(band_bound(p, I, J, b), score)) return -1;
    while (a < b) {
        const long long m = a + (b - a) / 2;
        if (band_certified(band_bound(p, I, J, m), score)) b = m;
        else a = m + 1;
    }
    return a;
}

inline long long band_auto_width(int /*I*/, int /*J*/) { return kBandAutoMargin; }

// Rows per lane of a banded fill.  A lane sweeps the whole strip window, 64 R + W - 1 columns for W band diagonals,
// so a small R wastes the fewest cells on a narrow band; a wide band amortises the per-step shuffle, loads and
// store over more rows with a large R.  forced: PBCCS_ALIGN_ROWS_PER_LANE (0 none).
inline int band_rows_per_lane(int I, long long W, int forced)
{
    for (int R : kRowsPerLane)
        if (forced == R) return R;
    int R = W <= 128 ? 2 : (W <= 512 ? 4 : 8);
    for (int small : kRowsPerLane)
        if (I <= 64 * small) return std::min(R, small);
    return R;
}

}  // namespace align
}  // namespace pbccs

// pbccs_amd/csrc/align_band_kernels.hip -- k_align_fill_band / k_align_trace_band and AlignRunner's banded route
// (align_band.hpp).  The cell arithmetic restates k_align_fill's (align_kernels.hip) operation
// for operation; that file is not touched.
#include <algorithm>
#include <cfloat>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <type_traits>

#include "../../include/pbccs_amd.h"
#include "align_band.hpp"

namespace pbccs {
namespace align {

namespace {

void check(hipError_t e, const char* what)
{
    if (e == hipSuccess) return;
    (void)hipGetLastError();
    throw DeviceError(std::string("align band: ") + what + ": " + hipGetErrorString(e));
}

// as in align_kernels.hip
__host__ __device__ __forceinline__ float smax(float a, float b) { return (a < b) ? b : a; }
__host__ __device__ __forceinline__ float edge_m(int k) { return k == 0 ? 0.f : -FLT_MAX; }
__host__ __device__ __forceinline__ float edge_gap(int k, float open, float ext)
{
    return k == 0 ? -FLT_MAX : open + (float)(k - 1) * ext;
}

__device__ __forceinline__ int iupac_bits(int c)
{
    switch (c) {
        case 'A': return 1;
        case 'C': return 2;
        case 'G': return 4;
        case 'T': return 8;
        case 'R': return 16 | 5;
        case 'Y': return 16 | 10;
        case 'S': return 16 | 6;
        case 'W': return 16 | 9;
        case 'K': return 16 | 12;
        case 'M': return 16 | 3;
        default: return 0;
    }
}

template <class S>
__device__ __forceinline__ uint32_t bits_of(S v)
{
    if constexpr (std::is_same<S, float>::value) return __float_as_uint(v);
    else return (uint32_t)v;
}
template <class S>
__device__ __forceinline__ S from_bits(uint32_t v)
{
    if constexpr (std::is_same<S, float>::value) return __uint_as_float(v);
    else return (S)v;
}

__device__ __forceinline__ void carry_store(uint32_t* p, uint32_t v)
{
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ uint32_t carry_load(uint32_t* p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the value of a dead cell (a diagonal outside [lo, hi]): forced, never accumulated
template <class S>
__device__ __forceinline__ S dead_value()
{
    if constexpr (std::is_same<S, float>::value) return -FLT_MAX;
    else return (S)kNwDead;
}

// first column of strip s's window: the band's first column on the strip's first row, clipped to the matrix
__host__ __device__ __forceinline__ int band_ws(int s, int R, int lo) { return max(1, s * 64 * R + 1 + lo); }
// last column: the band's last column on the strip's last row
__host__ __device__ __forceinline__ int band_we(int s, int R, int hi, int J)
{
    const long long e = (long long)(s + 1) * 64 * R + hi;
    return (int)(e < (long long)J ? e : (long long)J);
}

// k_align_fill with a column window per strip.  Strip s (first matrix row b + 1, b = 64 R s) sweeps the columns
// [ws, we] = [b + 1 + lo, b + 64 R + hi] clipped to [1, J]; lane l computes column ws + t - l at step t, so the
// skew is still one column per lane and the shift, the one-step-ahead loads and the strip carry work as in the
// full fill.  Cells of the window outside the band are dead: computed like any other and then forced to the dead
// value.  Row 0, column 0 and the carried row read as dead where they are outside the band (for the carried row:
// outside the previous strip's window).  A cell's move byte lands at ((s T + t) 64 + lane) R + r, T = jb.T.
template <int KIND, int R>
__global__ __launch_bounds__(64) void k_align_fill_band(const AlignBandJob* __restrict__ jobs,
                                                        const int* __restrict__ list,
                                                        const uint8_t* __restrict__ seq, uint8_t* __restrict__ store,
                                                        uint32_t* carry, uint32_t* __restrict__ scores, AlignScoring p)
{
    constexpr bool NW = KIND == kNw;
    constexpr bool IUPAC = KIND == kAffineIupac;
    using S = typename std::conditional<NW, int, float>::type;
    const S DEAD = dead_value<S>();
    const int lane = threadIdx.x;
    const int jobIdx = list[blockIdx.x];
    const AlignBandJob jb = jobs[jobIdx];
    const int I = jb.I, J = jb.J, T = jb.T, lo = jb.lo, hi = jb.hi;
    const uint8_t* tg = seq + jb.seqOff;
    const uint8_t* qr = tg + J;
    uint32_t* cr = carry + (jb.carryOff >= 0 ? jb.carryOff : 0);
    uint8_t* st = store + jb.storeOff;
    const float open = p.gapOpen, ext = p.gapExtend;

    for (int s = 0; s < jb.nStrips; ++s) {
        const int ws = band_ws(s, R, lo), we = band_we(s, R, hi, J);
        // the window plus the skew of the strip's last lane that owns a row: <= T
        const int steps = we - ws + 1 + min(63, (I - s * 64 * R - 1) / R);
        const int pws = s > 0 ? band_ws(s - 1, R, lo) : 0, pwe = s > 0 ? band_we(s - 1, R, hi, J) : 0;
        const int row0 = (s * 64 + lane) * R;   // matrix row above the lane's first row
        const bool rows = row0 < I;
        const bool carryOut = lane == 63 && s + 1 < jb.nStrips;
        // column ws - 1: column 0 where the window starts at column 1, dead otherwise
        S leftA[R], leftB[R];
        int qc[R], qb[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int i = row0 + r + 1;
            qc[r] = i <= I ? (int)qr[i - 1] : 0;
            qb[r] = IUPAC ? iupac_bits(qc[r]) : 0;
            const bool live = ws == 1 && -i >= lo;
            if constexpr (NW) {
                leftA[r] = live ? i * p.insert : DEAD;
                leftB[r] = 0;
            } else {
                leftA[r] = live ? edge_m(i) : DEAD;
                leftB[r] = live ? edge_gap(i, open, ext) : DEAD;
            }
        }
        // (row0, ws - 1): column 0 as above; for lane 0 of a later strip whose window starts past column 1, the
        // carried row at ws - 1, which is on diagonal lo and inside the previous strip's window
        S diagA = DEAD, diagB = NW ? (S)0 : DEAD;
        if (ws == 1) {
            if (-row0 >= lo) {
                if constexpr (NW) diagA = row0 * p.insert;
                else {
                    diagA = edge_m(row0);
                    diagB = edge_gap(row0, open, ext);
                }
            }
        } else if (lane == 0 && s > 0 && ws - 1 >= pws && ws - 1 <= pwe) {
            diagA = from_bits<S>(carry_load(cr + 2 * (ws - 1)));
            if constexpr (!NW) diagB = from_bits<S>(carry_load(cr + 2 * (ws - 1) + 1));
        }
        S botA = leftA[R - 1], botB = leftB[R - 1];
        // the row above the strip at column c, for lane 0: row 0 or the carried row, dead outside the band
        auto above = [&](int c, S& a, S& b) {
            a = DEAD;
            b = NW ? (S)0 : DEAD;
            if (s == 0) {
                if (c <= hi) {
                    if constexpr (NW) a = c * p.delete_;
                    else {
                        a = edge_m(c);
                        b = edge_gap(c, open, ext);
                    }
                }
            } else if (c >= pws && c <= pwe) {
                a = from_bits<S>(carry_load(cr + 2 * c));
                if constexpr (!NW) b = from_bits<S>(carry_load(cr + 2 * c + 1));
            }
        };
        int tcN = 0;
        S cinA = 0, cinB = 0;
        {
            const int j1 = ws - lane;
            if (j1 >= ws && j1 <= we) tcN = tg[j1 - 1];
            if (lane == 0) above(ws, cinA, cinB);
        }
        for (int t = 0; t < steps; ++t) {
            const int j = ws + t - lane;
            const int tc = tcN;
            S upA = __shfl_up(botA, 1, 64);
            S upB = 0;
            if constexpr (!NW) upB = __shfl_up(botB, 1, 64);
            if (lane == 0) {
                upA = cinA;
                upB = cinB;
            }
            {
                const int j2 = j + 1;
                tcN = (j2 >= ws && j2 <= we) ? (int)tg[j2 - 1] : 0;
                if (lane == 0 && j2 <= we) above(j2, cinA, cinB);
            }
            if (rows && j >= ws && j <= we) {
                S dA = diagA, dB = diagB, uA = upA, uB = upB;
                const int tb = IUPAC ? iupac_bits(tc) : 0;
                const int d0 = j - row0 - 1;   // the diagonal of the lane's first row; row r is on d0 - r
                uint32_t pack[(R + 3) / 4] = {};
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    S nA, nB;
                    uint32_t mv;
                    if constexpr (NW) {
                        const int a = dA + (qc[r] == tc ? p.match : p.mismatch);
                        const int b = uA + p.insert;
                        const int c = leftA[r] + p.delete_;
                        nA = max(a, max(b, c));
                        nB = 0;
                        mv = (a >= b && a >= c) ? 0u : (b >= c ? 1u : 2u);
                    } else {
                        float sc = p.mismatchScore;
                        if constexpr (IUPAC) {
                            if ((qb[r] & tb & 15) != 0 && ((qb[r] ^ tb) & 16) != 0) sc = p.partial;
                        }
                        if (qc[r] == tc) sc = p.matchScore;
                        const float m = smax(dA, dB) + sc;
                        const float c0 = leftA[r] + open;
                        const float c1 = leftB[r] + ext;
                        const float c2 = uA + open;
                        const float c3 = uB + ext;
                        const float g = smax(smax(c0, c1), smax(c2, c3));
                        float best = c0;   // std::max_element: the first maximum
                        uint32_t arg = 0;
                        if (best < c1) {
                            best = c1;
                            arg = 1;
                        }
                        if (best < c2) {
                            best = c2;
                            arg = 2;
                        }
                        if (best < c3) {
                            best = c3;
                            arg = 3;
                        }
                        nA = m;
                        nB = g;
                        mv = (m >= g ? 1u : 0u) | (arg << 1);
                    }
                    const int d = d0 - r;
                    if (d < lo || d > hi) {
                        nA = DEAD;
                        nB = NW ? (S)0 : DEAD;
                    }
                    dA = leftA[r];
                    dB = leftB[r];
                    uA = nA;
                    uB = nB;
                    leftA[r] = nA;
                    leftB[r] = nB;
                    pack[r / 4] |= mv << (8 * (r % 4));
                    if (row0 + r + 1 == I && j == J) {
                        scores[2 * (long long)jobIdx] = bits_of<S>(nA);
                        scores[2 * (long long)jobIdx + 1] = bits_of<S>(nB);
                    }
                }
                botA = leftA[R - 1];
                botB = leftB[R - 1];
                diagA = upA;
                diagB = upB;
                uint8_t* dst = st + (((long long)s * T + t) * 64 + lane) * R;
                if constexpr (R == 2) *reinterpret_cast<uint16_t*>(dst) = (uint16_t)pack[0];
                else if constexpr (R == 4) *reinterpret_cast<uint32_t*>(dst) = pack[0];
                else *reinterpret_cast<uint2*>(dst) = make_uint2(pack[0], pack[1]);
                if (carryOut) {
                    carry_store(cr + 2 * j, bits_of<S>(botA));
                    if constexpr (!NW) carry_store(cr + 2 * j + 1, bits_of<S>(botB));
                }
            }
        }
        // the next strip's lane 0 reads what this strip's lane 63 stored
        if (s + 1 < jb.nStrips) __threadfence();
    }
}

// The move byte of cell (i, j), 1 <= i <= I, 1 <= j <= J, or -1 where the cell is outside the band or its strip's
// window (the store holds nothing there).
__device__ __forceinline__ int band_move_byte(const uint8_t* st, int i, int j, int R, int T, int lo, int hi, int J)
{
    const int d = j - i;
    if (d < lo || d > hi) return -1;
    const int row = i - 1;
    const int strip = row / (64 * R);
    const int rem = row - strip * 64 * R;
    const int l = rem / R, r = rem - l * R;
    const int ws = band_ws(strip, R, lo), we = band_we(strip, R, hi, J);
    if (j < ws || j > we) return -1;
    const int t = (j - ws) + l;
    return st[(((long long)strip * T + t) * 64 + l) * R + r];
}

// k_align_trace over the banded store, for certified pairs only.  A walk that would read a cell outside the band
// stops and flags the pair (it then takes the full fill); a certified walk never does.
__global__ __launch_bounds__(64) void k_align_trace_band(const AlignBandJob* __restrict__ jobs,
                                                         const int* __restrict__ list, int n,
                                                         const uint8_t* __restrict__ seq,
                                                         const uint8_t* __restrict__ store, uint8_t* __restrict__ out,
                                                         int* __restrict__ lens, int* __restrict__ status,
                                                         AlignScoring p)
{
    const int idx = blockIdx.x * 64 + threadIdx.x;
    if (idx >= n) return;
    const int jobIdx = list[idx];
    const AlignBandJob jb = jobs[jobIdx];
    const int I = jb.I, J = jb.J, R = jb.R, T = jb.T, lo = jb.lo, hi = jb.hi;
    const uint8_t* tg = seq + jb.seqOff;
    const uint8_t* qr = tg + J;
    const uint8_t* st = store + jb.storeOff;
    uint8_t* o = out + jb.outOff;
    const float open = p.gapOpen, ext = p.gapExtend;
    int i = I, j = J, len = 0, flag = 0;
    const int cap = I + J;
    if (p.kind == kNw) {
        while ((i > 0 || j > 0) && len < cap) {
            int mv;
            if (i == 0 || j == 0) {
                if (j - i < lo || j - i > hi) flag = kTraceLeftBand;
                mv = i == 0 ? 2 : 1;
            } else {
                mv = band_move_byte(st, i, j, R, T, lo, hi, J);
                if (mv < 0) flag = kTraceLeftBand;
            }
            if (flag) break;
            if (mv == 0) {
                o[len++] = qr[i - 1] == tg[j - 1] ? 'M' : 'R';
                --i;
                --j;
            } else if (mv == 1) {
                o[len++] = 'I';
                --i;
            } else {
                o[len++] = 'D';
                --j;
            }
        }
    } else {
        int mb = band_move_byte(st, i, j, R, T, lo, hi, J);
        bool inM = (mb & 1) != 0;
        if (mb < 0) flag = kTraceLeftBand;
        while (!flag && (i > 0 || j > 0) && len < cap) {
            if (j - i < lo || j - i > hi) {
                flag = kTraceLeftBand;
                break;
            }
            if (inM) {
                if (i == 0 || j == 0) {
                    flag = kTraceFlagged;
                    break;
                }
                o[len++] = qr[i - 1] == tg[j - 1] ? 'M' : 'R';
                --i;
                --j;
                if (i > 0 && j > 0) {
                    mb = band_move_byte(st, i, j, R, T, lo, hi, J);
                    if (mb < 0) {
                        flag = kTraceLeftBand;
                        break;
                    }
                    inM = (mb & 1) != 0;
                } else if (i == 0 && j == 0) inM = true;   // M(0, 0) = 0 >= GAP(0, 0) = -FLT_MAX
                else inM = -FLT_MAX >= edge_gap(i + j, open, ext);
            } else {
                int arg;
                if (i > 0 && j > 0) {
                    mb = band_move_byte(st, i, j, R, T, lo, hi, J);
                    if (mb < 0) {
                        flag = kTraceLeftBand;
                        break;
                    }
                    arg = mb >> 1;
                } else {
                    const int k = i + j;   // the one that is not 0
                    const float c0 = edge_m(k - 1) + open;
                    const float c1 = edge_gap(k - 1, open, ext) + ext;
                    float s4[4];
                    s4[0] = j > 0 ? c0 : -FLT_MAX;
                    s4[1] = j > 0 ? c1 : -FLT_MAX;
                    s4[2] = i > 0 ? c0 : -FLT_MAX;
                    s4[3] = i > 0 ? c1 : -FLT_MAX;
                    float best = s4[0];
                    arg = 0;
                    if (best < s4[1]) {
                        best = s4[1];
                        arg = 1;
                    }
                    if (best < s4[2]) {
                        best = s4[2];
                        arg = 2;
                    }
                    if (best < s4[3]) {
                        best = s4[3];
                        arg = 3;
                    }
                }
                if (arg < 2) {
                    if (j == 0) {
                        flag = kTraceFlagged;
                        break;
                    }
                    o[len++] = 'D';
                    --j;
                } else {
                    if (i == 0) {
                        flag = kTraceFlagged;
                        break;
                    }
                    o[len++] = 'I';
                    --i;
                }
                inM = (arg & 1) == 0;
            }
        }
    }
    if (!flag && (i > 0 || j > 0)) flag = kTraceFlagged;
    lens[jobIdx] = len;
    status[jobIdx] = flag;
}

template <int KIND>
void launch_fill_band(int R, int grid, hipStream_t st, const AlignBandJob* jobs, const int* list, const uint8_t* seq,
                      uint8_t* store, uint32_t* carry, uint32_t* scores, const AlignScoring& p)
{
    switch (R) {
        case 2:
            hipLaunchKernelGGL((k_align_fill_band<KIND, 2>), dim3(grid), dim3(64), 0, st, jobs, list, seq, store,
                               carry, scores, p);
            break;
        case 4:
            hipLaunchKernelGGL((k_align_fill_band<KIND, 4>), dim3(grid), dim3(64), 0, st, jobs, list, seq, store,
                               carry, scores, p);
            break;
        default:
            hipLaunchKernelGGL((k_align_fill_band<KIND, 8>), dim3(grid), dim3(64), 0, st, jobs, list, seq, store,
                               carry, scores, p);
            break;
    }
}

long long env_ll(const char* name, long long dflt)
{
    const char* v = std::getenv(name);
    if (!v || !*v) return dflt;
    return std::atoll(v);
}

double final_score(const AlignScoring& p, const uint32_t* sc)
{
    if (p.kind == kNw) return (double)(int)sc[0];
    float m, g;
    std::memcpy(&m, &sc[0], 4);
    std::memcpy(&g, &sc[1], 4);
    return (double)(m >= g ? m : g);
}

}  // namespace

// One banded attempt for the pairs idx (indices into pairs) at the half-widths ws.  Per launch group: the fills,
// the scores to the host, the certificate, then the trace of the certified pairs while their stores are still
// there.  Certified pairs get their result; the others get their banded score in scoreOut and stay unanswered.
void AlignRunner::BandAttempt(const AlignScoring& p, const PairView* pairs, const std::vector<int>& idx,
                              const std::vector<long long>& ws, PairResult* out, std::vector<double>* scoreOut,
                              std::vector<int>* verdict)
{
    const long long budget = std::max(1LL, env_ll("PBCCS_ALIGN_WORKSPACE_MB", 2048)) << 20;
    const int forced = (int)env_ll("PBCCS_ALIGN_ROWS_PER_LANE", 0);
    const int nj = (int)idx.size();
    scoreOut->assign((size_t)nj, 0.0);
    verdict->assign((size_t)nj, kBandUncertified);
    if (nj == 0) return;
    std::vector<AlignBandJob> jobs((size_t)nj);
    std::vector<BandGeom> geom((size_t)nj);
    long long seqBytes = 0, outBytes = 0, carryWords = 0;
    for (int k = 0; k < nj; ++k) {
        const PairView& pv = pairs[idx[k]];
        AlignBandJob& jb = jobs[k];
        geom[k] = band_geom(pv.I, pv.J, ws[k]);
        jb.I = pv.I;
        jb.J = pv.J;
        jb.lo = (int)geom[k].lo;   // |lo|, hi <= 2 max(I, J) + 1, and a pair that is filled fits the workspace
        jb.hi = (int)geom[k].hi;
        jb.R = band_rows_per_lane(pv.I, (long long)jb.hi - jb.lo + 1, forced);
        jb.nStrips = (pv.I + 64 * jb.R - 1) / (64 * jb.R);
        jb.T = (int)band_steps(pv.I, pv.J, jb.R, geom[k]);
        jb.storeOff = 0;
        jb.seqOff = seqBytes;
        seqBytes += (long long)pv.I + pv.J;
        jb.outOff = outBytes;
        outBytes += (long long)pv.I + pv.J;
        jb.carryOff = -1;
        if (jb.nStrips > 1) {
            jb.carryOff = carryWords;
            carryWords += 2LL * (pv.J + 1);
        }
    }
    std::vector<int> order(nj);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) {
        return band_store_bytes(jobs[a].I, jobs[a].J, jobs[a].R, geom[a]) >
               band_store_bytes(jobs[b].I, jobs[b].J, jobs[b].R, geom[b]);
    });
    struct Group {
        int begin, end;
        long long bytes;
    };
    std::vector<Group> groups;
    {
        Group g{0, 0, 0};
        for (int k = 0; k < nj; ++k) {
            AlignBandJob& jb = jobs[order[k]];
            const long long b = (band_store_bytes(jb.I, jb.J, jb.R, geom[order[k]]) + 15) & ~15LL;
            if (g.end > g.begin && g.bytes + b > budget) {
                groups.push_back(g);
                g = Group{k, k, 0};
            }
            jb.storeOff = g.bytes;
            g.bytes += b;
            g.end = k + 1;
        }
        groups.push_back(g);
    }
    long long maxStore = 0;
    for (const Group& g : groups) maxStore = std::max(maxStore, g.bytes);
    // per group: one fill list per R, then room for the group's trace list (written once its scores are known)
    std::vector<int> lists;
    struct GroupLists {
        int traceOff, fillOff[3], fillN[3];
    };
    std::vector<GroupLists> gl(groups.size());
    for (size_t q = 0; q < groups.size(); ++q) {
        for (int v = 0; v < 3; ++v) {
            gl[q].fillOff[v] = (int)lists.size();
            for (int k = groups[q].begin; k < groups[q].end; ++k)
                if (jobs[order[k]].R == kRowsPerLane[v]) lists.push_back(order[k]);
            gl[q].fillN[v] = (int)lists.size() - gl[q].fillOff[v];
        }
        gl[q].traceOff = (int)lists.size();
        lists.resize(lists.size() + (size_t)(groups[q].end - groups[q].begin), 0);
    }
    std::vector<uint8_t> seq((size_t)seqBytes);
    for (int k = 0; k < nj; ++k) {
        const PairView& pv = pairs[idx[k]];
        std::memcpy(seq.data() + jobs[k].seqOff, pv.target, (size_t)pv.J);
        std::memcpy(seq.data() + jobs[k].seqOff + pv.J, pv.query, (size_t)pv.I);
    }
    std::vector<uint8_t> hOut((size_t)outBytes);
    std::vector<int> hLens(nj, 0), hStatus(nj, -1);
    std::vector<uint32_t> hScores(2 * (size_t)nj, 0);

    check(hipSetDevice(device_), "hipSetDevice");
    StreamScope scope(stream_);
    struct StreamIdle {
        hipStream_t s;
        ~StreamIdle() { (void)hipStreamSynchronize(s); }
    } idle{stream_};
    dSeq_.reserve((size_t)seqBytes, false);
    dBandJobs_.reserve((size_t)nj, false);
    dList_.reserve(lists.size(), false);
    dOut_.reserve((size_t)outBytes, false);
    dLens_.reserve((size_t)nj, false);
    dStatus_.reserve((size_t)nj, false);
    dScores_.reserve(2 * (size_t)nj, false);
    dCarry_.reserve((size_t)std::max(1LL, carryWords), false);
    dStore_.reserve((size_t)maxStore, false);
    check(hipMemcpyAsync(dSeq_.ptr, seq.data(), (size_t)seqBytes, hipMemcpyHostToDevice, stream_), "upload");
    check(hipMemcpyAsync(dBandJobs_.ptr, jobs.data(), sizeof(AlignBandJob) * nj, hipMemcpyHostToDevice, stream_),
          "upload");
    check(hipMemcpyAsync(dList_.ptr, lists.data(), sizeof(int) * lists.size(), hipMemcpyHostToDevice, stream_),
          "upload");
    check(hipMemsetAsync(dLens_.ptr, 0, sizeof(int) * nj, stream_), "memset");
    check(hipMemsetAsync(dStatus_.ptr, 0xff, sizeof(int) * nj, stream_), "memset");   // -1: never traced
    check(hipMemsetAsync(dScores_.ptr, 0, sizeof(uint32_t) * 2 * nj, stream_), "memset");

    std::vector<char> certified((size_t)nj, 0);
    for (size_t q = 0; q < groups.size(); ++q) {
        if (profiling) check(hipEventRecord(ev_[0], stream_), "event");
        for (int v = 0; v < 3; ++v) {
            if (gl[q].fillN[v] == 0) continue;
            const int* list = dList_.ptr + gl[q].fillOff[v];
            if (p.kind == kNw)
                launch_fill_band<kNw>(kRowsPerLane[v], gl[q].fillN[v], stream_, dBandJobs_.ptr, list, dSeq_.ptr,
                                      dStore_.ptr, dCarry_.ptr, dScores_.ptr, p);
            else if (p.kind == kAffine)
                launch_fill_band<kAffine>(kRowsPerLane[v], gl[q].fillN[v], stream_, dBandJobs_.ptr, list, dSeq_.ptr,
                                          dStore_.ptr, dCarry_.ptr, dScores_.ptr, p);
            else
                launch_fill_band<kAffineIupac>(kRowsPerLane[v], gl[q].fillN[v], stream_, dBandJobs_.ptr, list,
                                               dSeq_.ptr, dStore_.ptr, dCarry_.ptr, dScores_.ptr, p);
            check(hipGetLastError(), "k_align_fill_band launch");
            bandStats.launches++;
        }
        if (profiling) check(hipEventRecord(ev_[1], stream_), "event");
        // the group's scores decide which of its pairs are walked
        check(hipMemcpyAsync(hScores.data(), dScores_.ptr, sizeof(uint32_t) * 2 * nj, hipMemcpyDeviceToHost, stream_),
              "download");
        check(hipStreamSynchronize(stream_), "sync");
        int nt = 0;
        for (int k = groups[q].begin; k < groups[q].end; ++k) {
            const int j = order[k];
            const double sc = final_score(p, &hScores[2 * (size_t)j]);
            (*scoreOut)[j] = sc;
            if (band_certified(band_bound(p, jobs[j].I, jobs[j].J, ws[j]), sc)) {
                certified[j] = 1;
                lists[(size_t)gl[q].traceOff + nt++] = j;
            }
        }
        bandStats.storeBytes += (double)groups[q].bytes;
        bandStats.groups++;
        if (nt > 0) {
            check(hipMemcpyAsync(dList_.ptr + gl[q].traceOff, lists.data() + gl[q].traceOff, sizeof(int) * nt,
                                 hipMemcpyHostToDevice, stream_),
                  "upload");
            if (profiling) check(hipEventRecord(ev_[2], stream_), "event");
            hipLaunchKernelGGL(k_align_trace_band, dim3((nt + 63) / 64), dim3(64), 0, stream_, dBandJobs_.ptr,
                               dList_.ptr + gl[q].traceOff, nt, dSeq_.ptr, dStore_.ptr, dOut_.ptr, dLens_.ptr,
                               dStatus_.ptr, p);
            check(hipGetLastError(), "k_align_trace_band launch");
            if (profiling) check(hipEventRecord(ev_[3], stream_), "event");
        }
        if (profiling) {
            check(hipStreamSynchronize(stream_), "sync");
            float ms = 0.f;
            check(hipEventElapsedTime(&ms, ev_[0], ev_[1]), "event");
            bandStats.fillMs += ms;
            if (nt > 0) {
                check(hipEventElapsedTime(&ms, ev_[2], ev_[3]), "event");
                bandStats.traceMs += ms;
            }
        }
    }
    check(hipMemcpyAsync(hOut.data(), dOut_.ptr, (size_t)outBytes, hipMemcpyDeviceToHost, stream_), "download");
    check(hipMemcpyAsync(hLens.data(), dLens_.ptr, sizeof(int) * nj, hipMemcpyDeviceToHost, stream_), "download");
    check(hipMemcpyAsync(hStatus.data(), dStatus_.ptr, sizeof(int) * nj, hipMemcpyDeviceToHost, stream_), "download");
    check(hipStreamSynchronize(stream_), "sync");
    dSeq_.trim();
    dBandJobs_.trim();
    dList_.trim();
    dOut_.trim();
    dLens_.trim();
    dStatus_.trim();
    dScores_.trim();
    dCarry_.trim();
    dStore_.trim();

    for (int k = 0; k < nj; ++k) {
        const AlignBandJob& jb = jobs[k];
        bandStats.bandCells += band_cells(jb.I, jb.J, geom[k]);
        if (!certified[k]) continue;
        if (hStatus[k] != 0 || hLens[k] < 0 || hLens[k] > jb.I + jb.J) {
            (*verdict)[k] = kBandTraceFlagged;
            continue;
        }
        (*verdict)[k] = kBandNone;
        PairResult& o = out[idx[k]];
        o = PairResult();
        const uint8_t* r = hOut.data() + jb.outOff;
        o.transcript.assign(reinterpret_cast<const char*>(r), (size_t)hLens[k]);
        std::reverse(o.transcript.begin(), o.transcript.end());
        bandStats.traceSteps += hLens[k];
        if (p.kind == kNw) {
            o.scoreI = (int)hScores[2 * (size_t)k];
        } else {
            float m, g;
            std::memcpy(&m, &hScores[2 * (size_t)k], 4);
            std::memcpy(&g, &hScores[2 * (size_t)k + 1], 4);
            o.scoreF = m >= g ? m : g;
        }
    }
}

void AlignRunner::RunBanded(const AlignScoring& p, const PairView* pairs, int n, PairResult* out,
                            const BandOptions& band, BandInfo* info)
{
    if (!band.on) {
        Run(p, pairs, n, out);
        if (info)
            for (int k = 0; k < n; ++k) info[k] = BandInfo();
        return;
    }
    const int forced = (int)env_ll("PBCCS_ALIGN_ROWS_PER_LANE", 0);
    const long long budget = std::max(1LL, env_ll("PBCCS_ALIGN_WORKSPACE_MB", 2048)) << 20;
    std::vector<BandInfo> inf((size_t)std::max(0, n));
    std::vector<int> fullIdx, cand;
    std::vector<long long> w;
    auto to_full = [&](int k, int reason) {
        inf[k].banded = 0;
        inf[k].reason = reason;
        fullIdx.push_back(k);
        bandStats.fallbacks[reason]++;
    };
    // whether the band of half-width ww is worth a fill: 0, or the reason why not
    auto refuse = [&](int k, long long ww) {
        const int I = pairs[k].I, J = pairs[k].J;
        const BandGeom g = band_geom(I, J, ww);
        if (band_covers(I, J, g)) return kBandCoversMatrix;
        int Rf = 0;
        for (int R : kRowsPerLane)
            if (forced == R) Rf = R;
        if (!Rf) {
            Rf = kRowsPerLane[2];
            for (int R : {kRowsPerLane[1], kRowsPerLane[0]})
                if (I <= 64 * R) Rf = R;
        }
        const int Rb = band_rows_per_lane(I, (long long)g.hi - g.lo + 1, forced);
        if (band_store_bytes(I, J, Rb, g) >= store_bytes(I, J, Rf)) return kBandStoreNotSmaller;
        if (band_store_bytes(I, J, Rb, g) > budget) return kBandOverBudget;   // so is the full store: PBCCS_EOOM
        return kBandNone;
    };
    for (int k = 0; k < n; ++k) {
        const int I = pairs[k].I, J = pairs[k].J;
        if (I == 0 || J == 0) {
            to_full(k, kBandDegenerate);
            continue;
        }
        if (!band_bound(p, I, J, 0).certifiable) {
            to_full(k, kBandNotCertifiable);
            continue;
        }
        const long long w0 = band.w >= 0 ? band.w : band_auto_width(I, J);
        inf[k].w = (int)std::min(w0, (long long)std::max(I, J) + 1);
        const int why = refuse(k, w0);
        if (why) {
            to_full(k, why);
            continue;
        }
        cand.push_back(k);
        w.push_back(w0);
    }
    for (int attempt = 1; attempt <= 2 && !cand.empty(); ++attempt) {
        std::vector<double> sc;
        std::vector<int> verdict;
        BandAttempt(p, pairs, cand, w, out, &sc, &verdict);
        std::vector<int> next;
        std::vector<long long> nextW;
        for (size_t c = 0; c < cand.size(); ++c) {
            const int k = cand[c];
            inf[k].attempts = attempt;
            inf[k].w = (int)std::min(w[c], (long long)std::max(pairs[k].I, pairs[k].J) + 1);
            if (attempt == 1) bandStats.fullCells += (long long)pairs[k].I * pairs[k].J;
            if (verdict[c] == kBandNone) {
                inf[k].banded = 1;
                inf[k].reason = kBandNone;
                bandStats.bandedPairs++;
                continue;
            }
            if (verdict[c] == kBandTraceFlagged || attempt == 2) {
                to_full(k, verdict[c]);
                continue;
            }
            const long long w2 = band_widen(p, pairs[k].I, pairs[k].J, sc[c]);
            if (w2 < 0) {
                to_full(k, kBandNotCertifiable);
                continue;
            }
            const int why = refuse(k, w2);
            if (why) {
                inf[k].w = (int)w2;
                to_full(k, why);
                continue;
            }
            next.push_back(k);
            nextW.push_back(w2);
            bandStats.secondAttempts++;
        }
        cand.swap(next);
        w.swap(nextW);
    }
    // the rest takes today's fill, in one call
    if (!fullIdx.empty()) {
        std::vector<PairView> pv;
        for (int k : fullIdx) pv.push_back(pairs[k]);
        std::vector<PairResult> res(pv.size());
        Run(p, pv.data(), (int)pv.size(), res.data());
        for (size_t c = 0; c < fullIdx.size(); ++c) out[fullIdx[c]] = std::move(res[c]);
    }
    bandStats.pairs += n;
    if (info)
        for (int k = 0; k < n; ++k) info[k] = inf[k];
}

}  // namespace align
}  // namespace pbccs

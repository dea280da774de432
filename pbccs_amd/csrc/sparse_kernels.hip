// pbccs_amd/csrc/sparse_kernels.hip -- SparseAlign<K> on the device (sparse_kernels.hpp)
#include "sparse_kernels.hpp"

#include <algorithm>
#include <climits>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../../include/pbccs_amd.h"

namespace pbccs {
namespace sparse {

namespace {

constexpr int kBlock = 256;

inline void check(hipError_t e, const char* what)
{
    if (e != hipSuccess) throw DeviceError(std::string(what) + ": " + hipGetErrorString(e));
}

// A 0, C 1, T 2, G 3: any bijection serves a K-mer's identity, and the complement is code ^ 2
__device__ inline int base_code(uint8_t c) { return (c >> 1) & 3; }

__device__ inline int query_base(const uint8_t* q, int len2, int rc, int j)
{
    return rc ? (base_code(q[len2 - 1 - j]) ^ 2) : base_code(q[j]);
}

__device__ inline bool homopolymer(int code, int k)
{
    const int mask = (1 << (2 * k)) - 1;
    return code == (code & 3) * (0x5555 & mask);
}

// In-place exclusive scan of a[0, n) by the whole block (sum, or running maximum with identity -1); sh holds kBlock
// ints.  Chunks of kBlock elements with a carry.
template <bool kMax>
__device__ void block_scan_exclusive(int* a, int n, int* sh)
{
    const int tid = threadIdx.x;
    const int ident = kMax ? -1 : 0;
    int carry = ident;
    for (int b = 0; b < n; b += kBlock) {
        const int i = b + tid;
        sh[tid] = i < n ? a[i] : ident;
        __syncthreads();
        for (int off = 1; off < kBlock; off <<= 1) {
            const int u = tid >= off ? sh[tid - off] : ident;
            __syncthreads();
            sh[tid] = kMax ? max(sh[tid], u) : sh[tid] + u;
            __syncthreads();
        }
        const int excl = tid ? sh[tid - 1] : ident;
        const int tot = sh[kBlock - 1];
        if (i < n) a[i] = kMax ? max(carry, excl) : carry + excl;
        carry = kMax ? max(carry, tot) : carry + tot;
        __syncthreads();
    }
}

// index of the last element <= x in the ascending a[0, n), -1 when there is none
__device__ inline int last_not_above(const int* a, int n, int x)
{
    int lo = 0, hi = n;   // first element > x
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (a[mid] <= x) lo = mid + 1;
        else hi = mid;
    }
    return lo - 1;
}

// ---- k_sparse_count ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_sparse_count(const SparseJob* jobs, const uint8_t* seq, int* work, int k,
                                                         long long* nSeeds)
{
    __shared__ long long red[kBlock];
    const SparseJob jb = jobs[blockIdx.x];
    const Layout L(jb.len1, jb.len2, k);
    int* w = work + jb.posOff;
    const int tid = threadIdx.x;
    const int T = 1 << (2 * k);
    const int n1 = max(0, jb.len1 - k + 1), n2 = max(0, jb.len2 - k + 1);
    for (int c = tid; c <= T; c += kBlock) {
        w[L.tstart + c] = 0;
        w[L.qstart + c] = 0;
        if (c < T) {
            w[L.tcur + c] = 0;
            w[L.qcur + c] = 0;
        }
    }
    __syncthreads();
    const uint8_t* t = seq + jb.tOff;
    const uint8_t* q = seq + jb.qOff;
    for (int i = tid; i < jb.len1; i += kBlock) {
        int code = -1;
        if (i < n1) {
            code = 0;
            for (int b = 0; b < k; ++b) code = (code << 2) | base_code(t[i + b]);
            if (homopolymer(code, k)) code = -1;
        }
        w[L.tcode + i] = code;
        if (code >= 0) atomicAdd(&w[L.tstart + code], 1);
    }
    for (int j = tid; j < jb.len2; j += kBlock) {
        int code = -1;
        if (j < n2) {
            code = 0;
            for (int b = 0; b < k; ++b) code = (code << 2) | query_base(q, jb.len2, jb.rc, j + b);
            if (homopolymer(code, k)) code = -1;
        }
        w[L.qcode + j] = code;
        if (code >= 0) atomicAdd(&w[L.qstart + code], 1);
    }
    __syncthreads();
    long long sum = 0;
    for (int j = tid; j < n2; j += kBlock) {
        const int code = w[L.qcode + j];
        if (code >= 0) sum += w[L.tstart + code];
    }
    red[tid] = sum;
    __syncthreads();
    for (int off = kBlock / 2; off > 0; off >>= 1) {
        if (tid < off) red[tid] += red[tid + off];
        __syncthreads();
    }
    if (tid == 0) nSeeds[blockIdx.x] = red[0];
}

// One wave lists the positions of every K-mer in ascending order: 64 positions at a time, a lane's place inside its
// K-mer's bucket is the bucket's cursor plus the number of lower lanes holding the same K-mer.
__device__ void list_positions(const int* code, int n, const int* start, int* cur, int* pos, int* rank)
{
    const int lane = threadIdx.x & 63;
    for (int b = 0; b < n; b += 64) {
        const int i = b + lane;
        const int c = i < n ? code[i] : -1;
        int below = 0, total = 0, leader = lane;
        for (int l = 63; l >= 0; --l) {
            const int cl = __shfl(c, l);
            if (c >= 0 && cl == c) {
                ++total;
                if (l < lane) ++below;
                leader = l;
            }
        }
        int base = 0;
        if (c >= 0 && leader == lane) base = atomicAdd(&cur[c], total);
        base = __shfl(base, leader);
        if (c >= 0) {
            pos[start[c] + base + below] = i;
            if (rank) rank[i] = base + below;
        }
    }
}

// ---- k_sparse_index ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_sparse_index(const SparseJob* jobs, int* work, int* seeds, int k)
{
    __shared__ int sh[kBlock];
    const SparseJob jb = jobs[blockIdx.x];
    const Layout L(jb.len1, jb.len2, k);
    int* w = work + jb.posOff;
    const int tid = threadIdx.x;
    const int T = 1 << (2 * k);
    const int n1 = max(0, jb.len1 - k + 1), n2 = max(0, jb.len2 - k + 1);
    block_scan_exclusive<false>(w + L.tstart, T + 1, sh);
    block_scan_exclusive<false>(w + L.qstart, T + 1, sh);
    // seeds per query row, and whether a column / row holds a seed at all
    for (int j = tid; j <= jb.len2; j += kBlock) {
        const int code = j < n2 ? w[L.qcode + j] : -1;
        const int cnt = code >= 0 ? w[L.tstart + code + 1] - w[L.tstart + code] : 0;
        w[L.rowstart + j] = cnt;
        if (j < jb.len2) w[L.prow + j] = cnt > 0 ? j : -1;
    }
    for (int i = tid; i < jb.len1; i += kBlock) {
        const int code = i < n1 ? w[L.tcode + i] : -1;
        const int cnt = code >= 0 ? w[L.qstart + code + 1] - w[L.qstart + code] : 0;
        w[L.pcol + i] = cnt > 0 ? i : -1;
    }
    __syncthreads();
    block_scan_exclusive<false>(w + L.rowstart, jb.len2 + 1, sh);
    block_scan_exclusive<true>(w + L.prow, jb.len2, sh);    // the greatest seed row below each row
    block_scan_exclusive<true>(w + L.pcol, jb.len1, sh);    // the greatest seed column below each column
    if (tid < 64) list_positions(w + L.tcode, n1, w + L.tstart, w + L.tcur, w + L.tpos, w + L.trank);
    else if (tid < 128) list_positions(w + L.qcode, n2, w + L.qstart, w + L.qcur, w + L.qpos, nullptr);
    __syncthreads();
    // the seeds in (v, h) order: row after row, the K-mer's target positions ascending
    int* sH = seeds + jb.seedOff;
    int* sV = sH + jb.nSeeds;
    for (int j = tid; j < n2; j += kBlock) {
        const int code = w[L.qcode + j];
        if (code < 0) continue;
        const int t0 = w[L.tstart + code], cnt = w[L.tstart + code + 1] - t0;
        const int at = w[L.rowstart + j];
        for (int r = 0; r < cnt && at + r < jb.nSeeds; ++r) {
            sH[at + r] = w[L.tpos + t0 + r];
            sV[at + r] = j;
        }
    }
}

// ---- k_sparse_visible -------------------------------------------------------------------------------------------
// visible-left of seed s: among the seeds t with h_t < h_s and h_t + K >= c_prev (c_prev the greatest seed column
// below h_s) the smallest (d, h) above (d_s, h_s).  Column c's seeds are the query positions of its K-mer,
// ascending in v, so descending in d: the candidate of a column is the largest v_t < c - d_s.
// visible-above: among the seeds t with v_t < v_s and v_t + K >= r_prev the largest (d, h) below (d_s, h_s); row w's
// candidate is the largest h_t <= d_s + w.
__global__ __launch_bounds__(kBlock) void k_sparse_visible(const SparseJob* jobs, const int* work, int* seeds, int k)
{
    const SparseJob jb = jobs[blockIdx.y];
    const Layout L(jb.len1, jb.len2, k);
    const int* w = work + jb.posOff;
    const int n = jb.nSeeds;
    const int* sH = seeds + jb.seedOff;
    const int* sV = sH + n;
    int* visL = seeds + jb.seedOff + 4LL * n;
    int* visA = visL + n;
    for (int id = blockIdx.x * kBlock + threadIdx.x; id < n; id += gridDim.x * kBlock) {
        const int h = sH[id], v = sV[id], d = h - v;
        int best = -1, bestD = 0;
        const int cp = w[L.pcol + h];
        if (cp >= 0) {
            for (int c = max(0, cp - k); c <= cp; ++c) {
                const int code = w[L.tcode + c];
                if (code < 0) continue;
                const int q0 = w[L.qstart + code], cnt = w[L.qstart + code + 1] - q0;
                if (cnt == 0 || c - d <= 0) continue;
                const int at = last_not_above(w + L.qpos + q0, cnt, c - d - 1);
                if (at < 0) continue;
                const int vt = w[L.qpos + q0 + at], dt = c - vt;
                if (best < 0 || dt < bestD) {
                    bestD = dt;
                    best = w[L.rowstart + vt] + w[L.trank + c];
                }
            }
        }
        visL[id] = best;
        best = -1;
        const int rp = w[L.prow + v];
        if (rp >= 0) {
            for (int r = max(0, rp - k); r <= rp; ++r) {
                const int code = w[L.qcode + r];
                if (code < 0) continue;
                const int t0 = w[L.tstart + code], cnt = w[L.tstart + code + 1] - t0;
                if (cnt == 0 || d + r < 0) continue;
                const int at = last_not_above(w + L.tpos + t0, cnt, d + r);
                if (at < 0) continue;
                const int dt = w[L.tpos + t0 + at] - r;
                if (best < 0 || dt >= bestD) {
                    bestD = dt;
                    best = w[L.rowstart + r] + at;
                }
            }
        }
        visA[id] = best;
    }
}

// ---- k_sparse_sweep ---------------------------------------------------------------------------------------------
__device__ inline long long link_score(int ah, int av, int bh, int bv, int k)
{
    const long long fwd = min(ah - bh, av - bv);
    const long long indels = abs((ah - av) - (bh - bv));
    const long long matches = k - max(0LL, k - fwd);
    const long long mismatches = fwd - matches;
    return kMatchReward * matches - indels - mismatches;
}

// the greatest set bit below position x, -1 when there is none (a linear scan over words)
__device__ inline int prev_set(const unsigned* bits, int x)
{
    if (x <= 0) return -1;
    int wd = (x - 1) >> 5;
    unsigned m = bits[wd] & (0xffffffffu >> (31 - ((x - 1) & 31)));
    while (true) {
        if (m) return wd * 32 + 31 - __clz(m);
        if (--wd < 0) return -1;
        m = bits[wd];
    }
}

// the smallest set bit above position x, -1 when there is none (a linear scan over words)
__device__ inline int next_set(const unsigned* bits, int nWords, int x)
{
    int wd = (x + 1) >> 5;
    if (wd >= nWords) return -1;
    unsigned m = bits[wd] & (0xffffffffu << ((x + 1) & 31));
    while (true) {
        if (m) return wd * 32 + __ffs(m) - 1;
        if (++wd >= nWords) return -1;
        m = bits[wd];
    }
}

// The column set's occupancy: one bit per column, and over it a summary with one bit per non-zero word.  Seeds far
// ahead of the chain's front find no entry for thousands of columns (a good chain's entry erases the weaker ones
// ahead of it), so a search looks at its own word and then scans the summary only.
struct Occupancy {
    unsigned* bits;   // nWords
    unsigned* sum;    // nSum, in LDS
    int nWords, nSum;
    __device__ bool test(int x) const { return (bits[x >> 5] >> (x & 31)) & 1u; }
    __device__ void set(int x)
    {
        bits[x >> 5] |= 1u << (x & 31);
        sum[x >> 10] |= 1u << ((x >> 5) & 31);
    }
    __device__ void clear(int x)
    {
        const unsigned m = bits[x >> 5] & ~(1u << (x & 31));
        bits[x >> 5] = m;
        if (!m) sum[x >> 10] &= ~(1u << ((x >> 5) & 31));
    }
    __device__ int prev(int x) const   // the greatest set column below x
    {
        if (x <= 0) return -1;
        const int wd = (x - 1) >> 5;
        const unsigned m = bits[wd] & (0xffffffffu >> (31 - ((x - 1) & 31)));
        if (m) return wd * 32 + 31 - __clz(m);
        const int w2 = prev_set(sum, wd);
        return w2 < 0 ? -1 : w2 * 32 + 31 - __clz(bits[w2]);
    }
    __device__ int next(int x) const   // the smallest set column above x
    {
        const int wd = (x + 1) >> 5;
        if (wd >= nWords) return -1;
        const unsigned m = bits[wd] & (0xffffffffu << ((x + 1) & 31));
        if (m) return wd * 32 + __ffs(m) - 1;
        const int w2 = next_set(sum, nSum, wd);
        return w2 < 0 ? -1 : w2 * 32 + __ffs(bits[w2]) - 1;
    }
};

__global__ __launch_bounds__(64) void k_sparse_sweep(const SparseJob* jobs, int* work, int* seeds, int* anchors, int k,
                                                     int ldsCols, int sumWords, SparseOut* outs)
{
    extern __shared__ int lds[];   // summary [sumWords], then column seeds, z and bits of ldsCols columns
    const SparseJob jb = jobs[blockIdx.x];
    const Layout L(jb.len1, jb.len2, k);
    int* w = work + jb.posOff;
    const int lane = threadIdx.x;
    const int n = jb.nSeeds;
    const int cols = jb.len1 + k + 1, nWords = (cols + 31) / 32;
    const bool inLds = cols <= ldsCols;
    int* colSeed = inLds ? lds + sumWords : w + L.colSeed;
    int* colZ = inLds ? lds + sumWords + ldsCols : w + L.colZ;
    Occupancy occ;
    occ.bits = reinterpret_cast<unsigned*>(inLds ? lds + sumWords + 2 * ldsCols : w + L.bitmap);
    occ.sum = reinterpret_cast<unsigned*>(lds);
    occ.nWords = nWords;
    occ.nSum = (nWords + 31) / 32;
    const int* sH = seeds + jb.seedOff;
    const int* sV = sH + n;
    int* score = seeds + jb.seedOff + 2LL * n;
    int* pred = score + n;
    const int* visL = pred + n;
    const int* visA = visL + n;
    const int* rowstart = w + L.rowstart;
    for (int c = lane; c < nWords; c += 64) occ.bits[c] = 0;
    for (int c = lane; c < occ.nSum; c += 64) occ.sum[c] = 0;
    __syncthreads();

    const int n2 = max(0, jb.len2 - k + 1);
    long long bestScore = 0;
    int bestEnd = INT_MAX;
    int leave = 0;   // the next row whose seeds leave for the column set
    for (int r = 0; r < n2; ++r) {
        const int base = rowstart[r], m = rowstart[r + 1] - base;
        if (m == 0) continue;
        for (int s = lane; s < m; s += 64) {
            const int id = base + s, h = sH[id];
            int cand = -1;
            long long cs = 0;
            const int c = occ.prev(min(h, cols));
            if (c >= 0) {
                cand = colSeed[c];
                cs = score[cand] + link_score(h, r, sH[cand], sV[cand], k);
            }
            int t = visA[id];
            if (t >= 0) {
                const long long sc = score[t] + link_score(h, r, sH[t], sV[t], k);
                if (cand < 0 || sc > cs) cand = t, cs = sc;
            }
            t = visL[id];
            if (t >= 0) {
                const long long sc = score[t] + link_score(h, r, sH[t], sV[t], k);
                if (cand < 0 || sc > cs) cand = t, cs = sc;
            }
            if (cand >= 0 && cs > 0) {
                score[id] = (int)cs;
                pred[id] = cand;
                if (cs > bestScore || (cs == bestScore && id < bestEnd)) bestScore = cs, bestEnd = id;
            } else {
                score[id] = k;
                pred[id] = -1;
            }
        }
        __syncthreads();
        // every seed t with v_t + K < r leaves, in (v, h) order
        if (lane == 0) {
            for (; leave + k < r; ++leave) {
                const int e = rowstart[leave + 1];
                for (int t = rowstart[leave]; t < e; ++t) {
                    const int col = sH[t] + k;
                    if (col >= cols) continue;   // cannot happen: h <= len1 - K
                    const int zt = score[t] + sH[t] + leave;
                    const bool there = occ.test(col);
                    if (there && colZ[col] >= zt) continue;
                    if (!there) {   // an entry already at this column keeps its seed (std::set::insert)
                        occ.set(col);
                        colSeed[col] = t;
                        colZ[col] = zt;
                    }
                    for (int nx = occ.next(col); nx >= 0 && colZ[nx] < zt; nx = occ.next(nx)) occ.clear(nx);
                }
            }
        }
        __syncthreads();
    }
    // the best end: the highest score, the first in (v, h) order among equals
    for (int off = 32; off > 0; off >>= 1) {
        const long long os = __shfl_xor(bestScore, off);
        const int oe = __shfl_xor(bestEnd, off);
        if (os > bestScore || (os == bestScore && oe < bestEnd)) bestScore = os, bestEnd = oe;
    }
    if (lane == 0) {
        const int room = max(0, min(jb.len1, jb.len2) - k + 1);
        int* a = anchors + 2 * jb.anchorOff;
        int at = room;
        if (bestEnd != INT_MAX)
            for (int t = bestEnd, steps = 0; t >= 0 && at > 0 && steps < n; t = pred[t], ++steps) {
                --at;
                a[2 * at] = sH[t];
                a[2 * at + 1] = sV[t];
            }
        SparseOut o;
        o.score = at < room ? bestScore : 0;
        o.rangeCells = 0;
        o.nAnchors = room - at;
        o.anchorStart = at;
        outs[blockIdx.x] = o;
    }
}

// ---- k_sparse_ranges --------------------------------------------------------------------------------------------
// SdpRangeFinder::InitRangeFinder on ^ -> d_0 .. d_{J-1} -> $: an anchored position takes its anchor's row +- WIDTH;
// any other the hull of the previous anchor's range stepped forward (clamped to I) and the next anchor's stepped
// back (clamped to 0), the recursions starting from RangeUnion({}) = (INT_MAX / 2, -INT_MAX / 2) at ^ and $.
__global__ __launch_bounds__(kBlock) void k_sparse_ranges(const SparseJob* jobs, const int* anchors, int* ranges,
                                                          SparseOut* outs)
{
    const SparseJob jb = jobs[blockIdx.x];
    if (jb.rangeOff < 0) return;
    const int nA = outs[blockIdx.x].nAnchors;
    const int* a = anchors + 2 * (jb.anchorOff + outs[blockIdx.x].anchorStart);
    int* out = ranges + jb.rangeOff;
    const int I = jb.len2, J = jb.len1, big = INT_MAX / 2;
    unsigned long long cells = 0;
    for (int p = threadIdx.x; p < J; p += kBlock) {
        int lo = 0, hi = nA;   // the first anchor with h > p
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (a[2 * mid] <= p) lo = mid + 1;
            else hi = mid;
        }
        int b, e;
        if (lo > 0 && a[2 * (lo - 1)] == p) {
            const int v = a[2 * (lo - 1) + 1];
            b = max(v - kWidth, 0), e = min(v + kWidth, I);
        } else {
            int fb, fe, rb, re;
            if (lo > 0) {
                const int h = a[2 * (lo - 1)], v = a[2 * (lo - 1) + 1];
                fb = min(max(v - kWidth, 0) + (p - h), I), fe = min(min(v + kWidth, I) + (p - h), I);
            } else {
                fb = min(big + p + 1, I), fe = min(-big + p + 1, I);
            }
            if (lo < nA) {
                const int h = a[2 * lo], v = a[2 * lo + 1];
                rb = max(max(v - kWidth, 0) - (h - p), 0), re = max(min(v + kWidth, I) - (h - p), 0);
            } else {
                rb = max(big - (J - p), 0), re = max(-big - (J - p), 0);
            }
            b = min(fb, rb), e = max(fe, re);
        }
        out[2 * p] = b;
        out[2 * p + 1] = e;
        if (e > b) cells += (unsigned long long)(e - b);
    }
    if (cells) atomicAdd(&outs[blockIdx.x].rangeCells, cells);
}

long long env_ll(const char* name, long long dflt)
{
    const char* s = std::getenv(name);
    if (!s || !*s) return dflt;
    char* end = nullptr;
    const long long v = std::strtoll(s, &end, 10);
    return (end && *end == 0) ? v : dflt;
}

}  // namespace

SparseRunner::SparseRunner(int device, hipStream_t stream) : device_(device), stream_(stream), ownStream_(!stream)
{
    check(hipSetDevice(device_), "hipSetDevice");
    if (ownStream_) check(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking), "hipStreamCreate");
    for (auto& e : ev_) check(hipEventCreate(&e), "hipEventCreate");
}

SparseRunner::~SparseRunner()
{
    if (stream_) {
        (void)hipStreamSynchronize(stream_);
        if (ownStream_) (void)hipStreamDestroy(stream_);
    }
    for (auto& e : ev_)
        if (e) (void)hipEventDestroy(e);
}

void SparseRunner::Run(int k, const SparseInput* in, int n, std::vector<SparseResult>* out)
{
    RunImpl(k, in, n, out, nullptr);
}

void SparseRunner::RunKeep(int k, const SparseInput* in, int n, std::vector<KeptChain>* out)
{
    std::vector<SparseResult> res;
    out->assign((size_t)std::max(0, n), KeptChain());
    RunImpl(k, in, n, &res, out);
    for (int g = 0; g < n; ++g) {
        (*out)[g].status = res[g].status;
        (*out)[g].nSeeds = res[g].nSeeds;
        (*out)[g].nAnchors = res[g].status == PBCCS_OK ? res[g].nAnchors : 0;
    }
}

// keep: the chains stay on the device; each chunk's anchor room then follows the previous chunk's in dAnchors_,
// which is sized for the whole call up front
void SparseRunner::RunImpl(int k, const SparseInput* in, int n, std::vector<SparseResult>* out,
                           std::vector<KeptChain>* keep)
{
    out->assign((size_t)std::max(0, n), SparseResult());
    if (n <= 0) return;
    const long long budgetInts = std::max(1LL, env_ll("PBCCS_SPARSE_WORKSPACE_KB", 1048576)) * 1024 / 4;
    const long long halfInts = std::max(1LL, budgetInts / 2);
    const long long maxSeeds =
        std::min(std::max(0LL, env_ll("PBCCS_SPARSE_MAX_SEEDS", kDefaultMaxSeeds)), (long long)INT_MAX / 2);
    const int ldsLimit = (int)std::min<long long>(std::max(0LL, env_ll("PBCCS_SPARSE_LDS_COLS", kSweepLdsCols)), kSweepLdsCols);

    // host part: which jobs reach the device at all
    std::vector<int> live;
    for (int g = 0; g < n; ++g) {
        const SparseInput& s = in[g];
        SparseResult& r = (*out)[g];
        stats.jobs++;
        if (s.len1 > kMaxLen || s.len2 > kMaxLen) {
            r.status = PBCCS_EINVAL;
            continue;
        }
        bool ok = true;
        for (int i = 0; i < s.len1 && ok; ++i) ok = std::memchr("ACGT", s.target[i], 4) != nullptr;
        for (int i = 0; i < s.len2 && ok; ++i) ok = std::memchr("ACGT", s.query[i], 4) != nullptr;
        if (!ok) {
            r.status = PBCCS_EINVAL;
            continue;
        }
        if (Layout(s.len1, s.len2, k).total + (s.ranges ? 2LL * s.len1 : 0) > halfInts) {
            r.status = PBCCS_EOOM;
            continue;
        }
        live.push_back(g);
    }

    check(hipSetDevice(device_), "hipSetDevice");
    StreamScope scope(stream_);
    // leaves (also by exception) only once the stream is idle: queued copies read and write the vectors below
    struct StreamIdle {
        hipStream_t s;
        ~StreamIdle() { (void)hipStreamSynchronize(s); }
    } idle{stream_};

    long long keptPairs = 0;   // keep: the anchor room of the chunks before this one
    if (keep) {
        long long all = 0;
        for (int g : live) all += std::max(0, std::min(in[g].len1, in[g].len2) - k + 1);
        dAnchors_.reserve((size_t)std::max(1LL, 2 * all), false);
    }
    size_t at = 0;
    while (at < live.size()) {
        // one chunk: as many jobs as keep the position arrays within half the budget
        std::vector<SparseJob> jobs;
        std::vector<int> owner;
        long long posInts = 0, seqBytes = 0, anchorPairs = keptPairs, rangeInts = 0;
        while (at < live.size()) {
            SparseInput s = in[live[at]];
            if (keep) s.ranges = nullptr;
            const long long need = Layout(s.len1, s.len2, k).total + (s.ranges ? 2LL * s.len1 : 0);
            if (!jobs.empty() && posInts + rangeInts + need > halfInts) break;
            SparseJob jb;
            jb.tOff = seqBytes;
            jb.qOff = seqBytes + s.len1;
            jb.posOff = posInts;
            jb.seedOff = 0;
            jb.anchorOff = anchorPairs;
            jb.rangeOff = s.ranges ? rangeInts : -1;
            jb.len1 = s.len1;
            jb.len2 = s.len2;
            jb.rc = s.rc ? 1 : 0;
            jb.nSeeds = 0;
            jobs.push_back(jb);
            owner.push_back(live[at]);
            seqBytes += (long long)s.len1 + s.len2;
            posInts += Layout(s.len1, s.len2, k).total;
            anchorPairs += std::max(0, std::min(s.len1, s.len2) - k + 1);
            if (s.ranges) rangeInts += 2LL * s.len1;
            ++at;
        }
        const int nj = (int)jobs.size();
        std::vector<uint8_t> seq((size_t)std::max(1LL, seqBytes));
        for (int j = 0; j < nj; ++j) {
            const SparseInput& s = in[owner[j]];
            if (s.len1) std::memcpy(seq.data() + jobs[j].tOff, s.target, (size_t)s.len1);
            if (s.len2) std::memcpy(seq.data() + jobs[j].qOff, s.query, (size_t)s.len2);
        }
        dSeq_.reserve(seq.size(), false);
        dJobs_.reserve((size_t)nj, false);
        dCount_.reserve((size_t)nj, false);
        dPos_.reserve((size_t)std::max(1LL, posInts), false);
        check(hipMemcpyAsync(dSeq_.ptr, seq.data(), seq.size(), hipMemcpyHostToDevice, stream_), "upload");
        check(hipMemcpyAsync(dJobs_.ptr, jobs.data(), sizeof(SparseJob) * nj, hipMemcpyHostToDevice, stream_), "upload");
        if (profiling) check(hipEventRecord(ev_[0], stream_), "event");
        hipLaunchKernelGGL(k_sparse_count, dim3(nj), dim3(kBlock), 0, stream_, dJobs_.ptr, dSeq_.ptr, dPos_.ptr, k,
                           dCount_.ptr);
        check(hipGetLastError(), "k_sparse_count launch");
        stats.launches++;
        if (profiling) check(hipEventRecord(ev_[1], stream_), "event");
        std::vector<long long> counts((size_t)nj);
        check(hipMemcpyAsync(counts.data(), dCount_.ptr, sizeof(long long) * nj, hipMemcpyDeviceToHost, stream_),
              "download");
        check(hipStreamSynchronize(stream_), "sync");
        if (profiling) {
            float ms = 0.f;
            check(hipEventElapsedTime(&ms, ev_[0], ev_[1]), "event");
            stats.deviceMs += ms;
        }

        // the jobs within the seed cap, in launch groups whose seed arrays fit the other half of the budget
        std::vector<SparseJob> active;
        std::vector<int> activeOwner;
        struct Group {
            int begin, end;
            long long seedInts;
            int maxSeeds, maxCols, ldsCols;
        };
        std::vector<Group> groups;
        for (int j = 0; j < nj; ++j) {
            SparseResult& r = (*out)[owner[j]];
            r.nSeeds = counts[j];
            stats.seeds += counts[j];
            if (counts[j] > maxSeeds || counts[j] * kSeedInts > halfInts) {
                r.status = PBCCS_EOOM;
                continue;
            }
            const long long ints = counts[j] * kSeedInts;
            if (groups.empty() || groups.back().seedInts + ints > halfInts)
                groups.push_back(Group{(int)active.size(), (int)active.size(), 0, 0, 0, 0});
            Group& G = groups.back();
            SparseJob jb = jobs[j];
            jb.nSeeds = (int)counts[j];
            jb.seedOff = G.seedInts;
            G.seedInts += ints;
            G.maxSeeds = std::max(G.maxSeeds, jb.nSeeds);
            G.maxCols = std::max(G.maxCols, jb.len1 + k + 1);
            if (jb.len1 + k + 1 <= ldsLimit) G.ldsCols = std::max(G.ldsCols, jb.len1 + k + 1);
            G.end++;
            active.push_back(jb);
            activeOwner.push_back(owner[j]);
        }
        const int na = (int)active.size();
        if (na == 0) continue;
        long long maxSeedInts = 1;
        for (const Group& G : groups) maxSeedInts = std::max(maxSeedInts, G.seedInts);
        dActive_.reserve((size_t)na, false);
        dSeeds_.reserve((size_t)maxSeedInts, false);
        dAnchors_.reserve((size_t)std::max(1LL, 2 * anchorPairs), false);
        dRanges_.reserve((size_t)std::max(1LL, rangeInts), false);
        dOut_.reserve((size_t)na, false);
        check(hipMemcpyAsync(dActive_.ptr, active.data(), sizeof(SparseJob) * na, hipMemcpyHostToDevice, stream_),
              "upload");
        if (profiling) check(hipEventRecord(ev_[2], stream_), "event");
        for (const Group& G : groups) {
            const int ng = G.end - G.begin;
            const SparseJob* dj = dActive_.ptr + G.begin;
            hipLaunchKernelGGL(k_sparse_index, dim3(ng), dim3(kBlock), 0, stream_, dj, dPos_.ptr, dSeeds_.ptr, k);
            check(hipGetLastError(), "k_sparse_index launch");
            const int gx = std::max(1, std::min(64, (G.maxSeeds + kBlock - 1) / kBlock));
            hipLaunchKernelGGL(k_sparse_visible, dim3(gx, ng), dim3(kBlock), 0, stream_, dj, dPos_.ptr, dSeeds_.ptr, k);
            check(hipGetLastError(), "k_sparse_visible launch");
            const int ldsCols = G.ldsCols;   // the widest column set of the group that fits the LDS limit
            const int sumWords = ((G.maxCols + 31) / 32 + 31) / 32;
            const size_t ldsBytes = sizeof(int) * (sumWords + 2 * (size_t)ldsCols + (ldsCols + 31) / 32);
            hipLaunchKernelGGL(k_sparse_sweep, dim3(ng), dim3(64), ldsBytes, stream_, dj, dPos_.ptr, dSeeds_.ptr,
                               dAnchors_.ptr, k, ldsCols, sumWords, dOut_.ptr + G.begin);
            check(hipGetLastError(), "k_sparse_sweep launch");
            stats.launches += 3;
            if (rangeInts) {
                hipLaunchKernelGGL(k_sparse_ranges, dim3(ng), dim3(kBlock), 0, stream_, dj, dAnchors_.ptr, dRanges_.ptr,
                                   dOut_.ptr + G.begin);
                check(hipGetLastError(), "k_sparse_ranges launch");
                stats.launches++;
            }
        }
        if (profiling) check(hipEventRecord(ev_[3], stream_), "event");
        std::vector<SparseOut> hOut((size_t)na);
        std::vector<int> hAnchors((size_t)std::max(1LL, keep ? 1 : 2 * anchorPairs)),
            hRanges((size_t)std::max(1LL, rangeInts));
        check(hipMemcpyAsync(hOut.data(), dOut_.ptr, sizeof(SparseOut) * na, hipMemcpyDeviceToHost, stream_), "download");
        if (anchorPairs && !keep)
            check(hipMemcpyAsync(hAnchors.data(), dAnchors_.ptr, sizeof(int) * 2 * anchorPairs, hipMemcpyDeviceToHost,
                                 stream_),
                  "download");
        if (rangeInts)
            check(hipMemcpyAsync(hRanges.data(), dRanges_.ptr, sizeof(int) * rangeInts, hipMemcpyDeviceToHost, stream_),
                  "download");
        check(hipStreamSynchronize(stream_), "sync");
        if (profiling) {
            float ms = 0.f;
            check(hipEventElapsedTime(&ms, ev_[2], ev_[3]), "event");
            stats.deviceMs += ms;
        }
        if (keep) keptPairs = anchorPairs;
        for (int j = 0; j < na; ++j) {
            const SparseInput& s = in[activeOwner[j]];
            SparseResult& r = (*out)[activeOwner[j]];
            const SparseJob& jb = active[j];
            const SparseOut& o = hOut[j];
            r.nAnchors = o.nAnchors;
            r.score = o.score;
            stats.anchors += o.nAnchors;
            if (keep) {
                (*keep)[activeOwner[j]].anchorOff = jb.anchorOff + o.anchorStart;
                continue;
            }
            if (o.nAnchors > s.anchorCap || (o.nAnchors > 0 && !s.anchors)) r.status = PBCCS_ERANGE;
            else if (o.nAnchors > 0)
                std::memcpy(s.anchors, hAnchors.data() + 2 * (jb.anchorOff + o.anchorStart), sizeof(int) * 2 * o.nAnchors);
            if (s.ranges) {
                if (s.len1) std::memcpy(s.ranges, hRanges.data() + jb.rangeOff, sizeof(int) * 2 * (size_t)s.len1);
                stats.rangeCells += (long long)o.rangeCells;
                stats.fullCells += (long long)s.len1 * (s.len2 + 1LL);
            }
        }
    }
    // the stream is idle: buffers that growth retired can go
    dSeq_.trim();
    dJobs_.trim();
    dActive_.trim();
    dCount_.trim();
    dPos_.trim();
    dSeeds_.trim();
    dAnchors_.trim();
    dRanges_.trim();
    dOut_.trim();
}

}  // namespace sparse
}  // namespace pbccs

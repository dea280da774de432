// pbccs_amd/csrc/demux_kernels.hip -- k_demux_score, k_demux_call, k_demux_extent and the engine's
// demultiplexing workspace (demux_kernels.hpp).
#include "demux_kernels.hpp"

#include <algorithm>
#include <climits>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../../include/pbccs_amd.h"

namespace pbccs {
namespace demux {

namespace {

void check(hipError_t e, const char* what)
{
    if (e == hipSuccess) return;
    (void)hipGetLastError();
    throw DeviceError(std::string("demux: ") + what + ": " + hipGetErrorString(e));
}

// A read byte as a barcode base: 0..3 for exactly A C G T, 4 (matches nothing) for every other byte
__host__ __device__ __forceinline__ int base_code(int c)
{
    return c == 'A' ? 0 : c == 'C' ? 1 : c == 'G' ? 2 : c == 'T' ? 3 : 4;
}

constexpr unsigned long long kEvenBits = 0x5555555555555555ull;

// Bit 2 k of the result: base k of the packed word equals wc (wc == 4: no base does)
__device__ __forceinline__ unsigned long long match_bits(unsigned long long word, int wc)
{
    const unsigned long long y = word ^ ((unsigned long long)(wc & 3) * kEvenBits);
    return wc < 4 ? ~(y | (y >> 1)) & kEvenBits : 0ull;
}

// Scores of 64 barcodes per pass inside one window.  One wavefront per (read, end); four per block.
template <int LMAX>
__global__ __launch_bounds__(256) void k_demux_score(const DemuxJob* __restrict__ jobs, int nJobs,
                                                     const uint8_t* __restrict__ win,
                                                     const unsigned long long* __restrict__ codes,
                                                     const int* __restrict__ lens, int B, int match, int mismatch,
                                                     int ins, int del, int* __restrict__ scores,
                                                     DemuxEnd* __restrict__ ends)
{
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
    if (wave >= 2 * nJobs) return;
    const int r = wave >> 1, e = wave & 1;
    const int wlen = jobs[r].wlen;
    const uint8_t* w = win + jobs[r].winOff + (e ? wlen : 0);

    const int bonus = match - mismatch;
    int b1 = INT_MIN, i1 = INT_MAX, b2 = INT_MIN;   // this lane's best, its index, and the best of its others
    for (int p = 0; p * 64 < B; ++p) {
        const int b = p * 64 + lane;
        const bool valid = b < B;
        const int bb = valid ? b : B - 1;
        const unsigned long long c0 = codes[((size_t)e * B + bb) * kWordsPerBarcode];
        const unsigned long long c1 = LMAX > 32 ? codes[((size_t)e * B + bb) * kWordsPerBarcode + 1] : 0ull;
        const int len = lens[bb];
        int S[LMAX + 1];
#pragma unroll
        for (int i = 0; i <= LMAX; ++i) S[i] = i * ins;
        int best = len * ins;   // column 0 of row len
        for (int j = 0; j < wlen; ++j) {
            const int wc = base_code(w[j]);   // the same for every lane
            const unsigned long long m0 = match_bits(c0, wc);
            const unsigned long long m1 = LMAX > 32 ? match_bits(c1, wc) : 0ull;
            const unsigned mw[4] = {(unsigned)m0, (unsigned)(m0 >> 32), (unsigned)m1, (unsigned)(m1 >> 32)};
            int lenj = len;
            asm volatile("" : "+v"(lenj));   // opaque per column: 64 hoisted row compares would not fit the SGPRs
            int diag = 0, up = 0, cur = 0;
#pragma unroll
            for (int i = 1; i <= LMAX; ++i) {
                // 0 or -1 from the row's match bit (a signed 1-bit field): arithmetic, not a select on a lane mask
                const int eq = (int)(mw[(i - 1) / 16] << (31 - 2 * ((i - 1) & 15))) >> 31;
                const int old = S[i];
                const int v = max(diag + mismatch + (bonus & eq), max(old + del, up + ins));
                diag = old;
                S[i] = v;
                up = v;
                cur = i == lenj ? v : cur;
            }
            best = max(best, cur);
        }
        if (valid) {
            if (scores) scores[((size_t)r * 2 + e) * B + b] = best;
            if (best > b1) {   // indices rise with the passes: a later one only when strictly greater
                b2 = b1;
                b1 = best;
                i1 = b;
            } else {
                b2 = max(b2, best);
            }
        }
    }
    // butterfly over the lanes: both partners of a step keep the same merged triple
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const int ob1 = __shfl_xor(b1, m, 64), oi1 = __shfl_xor(i1, m, 64), ob2 = __shfl_xor(b2, m, 64);
        if (b1 > ob1 || (b1 == ob1 && i1 < oi1)) {
            b2 = max(b2, ob1);
        } else {
            b2 = max(ob2, b1);
            b1 = ob1;
            i1 = oi1;
        }
    }
    if (lane == 0) ends[(size_t)r * 2 + e] = DemuxEnd{b1, i1, b2};
}

__host__ __device__ inline int score_lead(long long best, long long second)
{
    if (second == INT_MIN) return INT_MAX;   // no other barcode
    const long long d = best - second;
    return d > INT_MAX ? INT_MAX : (int)d;
}

// The call rules for one read.  rowL / rowT: its two score rows, read by the symmetric design only.
__host__ __device__ inline void call_rules(const DemuxEnd& L, const DemuxEnd& T, const int* rowL, const int* rowT,
                                           const int* lens, int B, const DemuxOptions& o, DemuxCall* c)
{
    long long score;
    int i, j, sl;
    if (!o.symmetric) {
        i = L.index;
        j = T.index;
        score = (long long)L.best + T.best;
        const int a = score_lead(L.best, L.second), b = score_lead(T.best, T.second);
        sl = a < b ? a : b;
    } else {
        long long t1 = LLONG_MIN, t2 = LLONG_MIN;
        i = 0;
        for (int b = 0; b < B; ++b) {
            const long long t = (long long)rowL[b] + rowT[b];
            if (b == 0 || t > t1) {
                t2 = t1;
                t1 = t;
                i = b;
            } else if (t > t2) {
                t2 = t;
            }
        }
        j = i;
        score = t1;
        sl = B > 1 ? score_lead(t1, t2) : INT_MAX;
    }
    const long long num = 100 * score, den = (long long)o.match * (lens[i] + lens[j]);   // den > 0
    long long q = num / den;
    if (num % den != 0 && num < 0) --q;   // floor
    q = q < 0 ? 0 : q > 100 ? 100 : q;
    c->lead = i;
    c->trail = j;
    c->score = (int)score;
    c->scoreLead = sl;
    c->quality = (int)q;
    c->called = (q >= o.minQuality && sl >= o.minScoreLead) ? 1 : 0;
}

__global__ __launch_bounds__(64) void k_demux_call(int nJobs, const DemuxEnd* __restrict__ ends,
                                                   const int* __restrict__ scores, const int* __restrict__ lens,
                                                   int B, DemuxOptions o, DemuxCall* __restrict__ calls)
{
    const int r = blockIdx.x * 64 + threadIdx.x;
    if (r >= nJobs) return;
    DemuxCall c;
    const int* row = o.symmetric ? scores + (size_t)r * 2 * B : nullptr;
    call_rules(ends[(size_t)r * 2], ends[(size_t)r * 2 + 1], row, row ? row + B : nullptr, lens, B, o, &c);
    DemuxCall* dst = &calls[r];
    dst->lead = c.lead;
    dst->trail = c.trail;
    dst->called = c.called;
    dst->score = c.score;
    dst->scoreLead = c.scoreLead;
    dst->quality = c.quality;
}

// The extents of a read's two called barcodes.  One lane per (read, end); the lane's column holds, beside each
// score, the window column where the cell's path left row 0.
template <int LMAX>
__global__ __launch_bounds__(64) void k_demux_extent(const DemuxJob* __restrict__ jobs, int nJobs,
                                                     const uint8_t* __restrict__ win,
                                                     const unsigned long long* __restrict__ codes,
                                                     const int* __restrict__ lens, int B, int match, int mismatch,
                                                     int ins, int del, DemuxCall* __restrict__ calls)
{
    const int t = blockIdx.x * 64 + threadIdx.x;
    if (t >= 2 * nJobs) return;
    const int r = t >> 1, e = t & 1;
    const int wlen = jobs[r].wlen;
    const uint8_t* w = win + jobs[r].winOff + (e ? wlen : 0);
    const int b = e ? calls[r].trail : calls[r].lead;
    const unsigned long long c0 = codes[((size_t)e * B + b) * kWordsPerBarcode];
    const unsigned long long c1 = LMAX > 32 ? codes[((size_t)e * B + b) * kWordsPerBarcode + 1] : 0ull;
    const int len = lens[b];
    int S[LMAX + 1], st[LMAX + 1];
#pragma unroll
    for (int i = 0; i <= LMAX; ++i) {
        S[i] = i * ins;
        st[i] = 0;
    }
    int best = len * ins, bj = 0, bst = 0;
    for (int j = 1; j <= wlen; ++j) {
        const int wc = base_code(w[j - 1]);
        int diagS = 0, diagSt = st[0], upS = 0, upSt = j, cur = 0, curSt = 0;
        st[0] = j;
        int lenj = len;
        asm volatile("" : "+v"(lenj));   // opaque per column, as in k_demux_score
#pragma unroll
        for (int i = 1; i <= LMAX; ++i) {
            const unsigned long long cw = (i - 1) < 32 ? c0 : c1;
            const int qc = (int)((cw >> (2 * ((i - 1) & 31))) & 3ull);
            const int oldS = S[i], oldSt = st[i];
            int v = diagS + (qc == wc ? match : mismatch), s = diagSt;   // diagonal, Delete, Extra: a later one
            if (oldS + del > v) {                                        // only when strictly greater
                v = oldS + del;
                s = oldSt;
            }
            if (upS + ins > v) {
                v = upS + ins;
                s = upSt;
            }
            diagS = oldS;
            diagSt = oldSt;
            S[i] = v;
            st[i] = s;
            upS = v;
            upSt = s;
            cur = i == lenj ? v : cur;
            curSt = i == lenj ? s : curSt;
        }
        if (cur > best) {   // the smallest column holding the row's maximum
            best = cur;
            bj = j;
            bst = curSt;
        }
    }
    if (e == 0) {
        calls[r].leadBegin = bst;
        calls[r].leadEnd = bj;
    } else {
        calls[r].trailBegin = jobs[r].off + bst;
        calls[r].trailEnd = jobs[r].off + bj;
    }
}

long long env_ll(const char* name, long long dflt)
{
    const char* s = std::getenv(name);
    return s && *s ? std::atoll(s) : dflt;
}

template <int LMAX>
void launch(int nj, hipStream_t st, const DemuxJob* jobs, const uint8_t* win, const unsigned long long* codes,
            const int* lens, int B, const DemuxOptions& o, int* scores, DemuxEnd* ends, DemuxCall* calls)
{
    hipLaunchKernelGGL(k_demux_score<LMAX>, dim3((2 * nj + 3) / 4), dim3(256), 0, st, jobs, nj, win, codes, lens, B,
                       o.match, o.mismatch, o.insert, o.delete_, scores, ends);
    check(hipGetLastError(), "k_demux_score launch");
    hipLaunchKernelGGL(k_demux_call, dim3((nj + 63) / 64), dim3(64), 0, st, nj, ends, scores, lens, B, o, calls);
    check(hipGetLastError(), "k_demux_call launch");
    hipLaunchKernelGGL(k_demux_extent<LMAX>, dim3((2 * nj + 63) / 64), dim3(64), 0, st, jobs, nj, win, codes, lens, B,
                       o.match, o.mismatch, o.insert, o.delete_, calls);
    check(hipGetLastError(), "k_demux_extent launch");
}

int complement_code(int c) { return 3 - c; }   // A <-> T, C <-> G

}  // namespace

DemuxRunner::DemuxRunner(int device) : device_(device)
{
    check(hipSetDevice(device_), "hipSetDevice");
    check(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking), "hipStreamCreate");
    for (auto& e : ev_) check(hipEventCreate(&e), "hipEventCreate");
}

DemuxRunner::~DemuxRunner()
{
    if (stream_) {
        (void)hipStreamSynchronize(stream_);
        (void)hipStreamDestroy(stream_);
    }
    for (auto& e : ev_)
        if (e) (void)hipEventDestroy(e);
}

void DemuxRunner::Run(const char* const* seqs, const int* lens, int B, const DemuxOptions& o,
                      const char* const* reads, const int* rlens, int n, DemuxEnd* ends, DemuxCall* calls, int* scores)
{
    const long long budget = std::max(1LL, env_ll("PBCCS_DEMUX_WORKSPACE_KB", 262144)) * 1024;
    const bool matrix = scores != nullptr || o.symmetric;   // the symmetric design reads its rows
    const int W = o.window;
    // the barcodes, 2 bits per base: forward for the leading end, reverse complement for the trailing end
    int lmaxLen = 0;
    long long sumLen = 0;
    std::vector<unsigned long long> codes((size_t)2 * B * kWordsPerBarcode, 0ull);
    for (int b = 0; b < B; ++b) {
        lmaxLen = std::max(lmaxLen, lens[b]);
        sumLen += lens[b];
        for (int k = 0; k < lens[b]; ++k) {
            const unsigned long long f = (unsigned long long)base_code(seqs[b][k]);
            const unsigned long long rc = (unsigned long long)complement_code(base_code(seqs[b][lens[b] - 1 - k]));
            codes[((size_t)b) * kWordsPerBarcode + k / 32] |= f << (2 * (k % 32));
            codes[((size_t)B + b) * kWordsPerBarcode + k / 32] |= rc << (2 * (k % 32));
        }
    }
    const int LMAX = lmaxLen <= 16 ? 16 : lmaxLen <= 32 ? 32 : 64;

    // the reads that reach the device; an empty read scores len(b) * Insert on both ends and launches nothing
    std::vector<int> readOf;
    std::vector<DemuxJob> jobs;
    for (int r = 0; r < n; ++r) {
        stats.reads++;
        const int len = reads[r] ? std::max(0, rlens[r]) : 0;
        if (len == 0) {
            DemuxEnd e{INT_MIN, 0, INT_MIN};
            for (int b = 0; b < B; ++b) {
                const int s = lens[b] * o.insert;
                if (scores) scores[(size_t)r * 2 * B + b] = scores[((size_t)r * 2 + 1) * B + b] = s;
                if (b == 0 || s > e.best) {
                    e.second = b == 0 ? INT_MIN : e.best;
                    e.best = s;
                    e.index = b;
                } else {
                    e.second = std::max(e.second, s);
                }
            }
            std::vector<int> row;
            if (o.symmetric) {
                row.resize(B);
                for (int b = 0; b < B; ++b) row[b] = lens[b] * o.insert;
            }
            DemuxCall c{};
            call_rules(e, e, row.data(), row.data(), lens, B, o, &c);
            if (ends) ends[(size_t)r * 2] = ends[(size_t)r * 2 + 1] = e;
            if (calls) calls[r] = c;
            continue;
        }
        const int wlen = std::min(W, len);
        stats.cells += 2LL * wlen * sumLen;
        jobs.push_back(DemuxJob{0, wlen, std::max(0, len - W)});
        readOf.push_back(r);
    }
    const int nj = (int)jobs.size();
    if (nj == 0) return;

    // launch groups of consecutive jobs whose windows and score rows fit the budget
    struct Group {
        int begin, end;
        long long winBytes;
    };
    std::vector<Group> lg;
    {
        const long long fixed = (matrix ? 8LL * B : 0) + (long long)(sizeof(DemuxJob) + 2 * sizeof(DemuxEnd) + sizeof(DemuxCall));
        Group g{0, 0, 0};
        long long bytes = 0;
        for (int k = 0; k < nj; ++k) {
            const long long mine = fixed + 2LL * jobs[k].wlen;
            if (g.end > g.begin && bytes + mine > budget) {
                lg.push_back(g);
                g = Group{k, k, 0};
                bytes = 0;
            }
            jobs[k].winOff = g.winBytes;
            g.winBytes += 2LL * jobs[k].wlen;
            bytes += mine;
            g.end = k + 1;
        }
        lg.push_back(g);
    }
    int maxJobs = 1;
    long long maxWin = 1;
    for (const Group& g : lg) {
        maxJobs = std::max(maxJobs, g.end - g.begin);
        maxWin = std::max(maxWin, g.winBytes);
    }

    std::vector<uint8_t> win((size_t)maxWin);
    std::vector<DemuxEnd> hEnds((size_t)2 * maxJobs);
    std::vector<DemuxCall> hCalls((size_t)maxJobs);
    std::vector<int> hScores(scores ? (size_t)2 * B * maxJobs : 0);
    check(hipSetDevice(device_), "hipSetDevice");
    StreamScope scope(stream_);
    // leaves (also by exception) only once the stream is idle: queued copies read and write the vectors above
    struct StreamIdle {
        hipStream_t s;
        ~StreamIdle() { (void)hipStreamSynchronize(s); }
    } idle{stream_};
    dWin_.reserve((size_t)maxWin, false);
    dJobs_.reserve((size_t)maxJobs, false);
    dCodes_.reserve(codes.size(), false);
    dLens_.reserve((size_t)B, false);
    dEnds_.reserve((size_t)2 * maxJobs, false);
    dCalls_.reserve((size_t)maxJobs, false);
    if (matrix) dScores_.reserve((size_t)2 * B * maxJobs, false);
    check(hipMemcpyAsync(dCodes_.ptr, codes.data(), sizeof(unsigned long long) * codes.size(), hipMemcpyHostToDevice,
                         stream_), "upload");
    check(hipMemcpyAsync(dLens_.ptr, lens, sizeof(int) * B, hipMemcpyHostToDevice, stream_), "upload");
    for (const Group& g : lg) {
        const int m = g.end - g.begin;
        for (int k = g.begin; k < g.end; ++k) {
            const int r = readOf[k], wlen = jobs[k].wlen;
            std::memcpy(win.data() + jobs[k].winOff, reads[r], (size_t)wlen);
            std::memcpy(win.data() + jobs[k].winOff + wlen, reads[r] + jobs[k].off, (size_t)wlen);
        }
        check(hipMemcpyAsync(dWin_.ptr, win.data(), (size_t)g.winBytes, hipMemcpyHostToDevice, stream_), "upload");
        check(hipMemcpyAsync(dJobs_.ptr, jobs.data() + g.begin, sizeof(DemuxJob) * m, hipMemcpyHostToDevice, stream_),
              "upload");
        if (profiling) check(hipEventRecord(ev_[0], stream_), "event");
        int* ds = matrix ? dScores_.ptr : nullptr;
        if (LMAX == 16)
            launch<16>(m, stream_, dJobs_.ptr, dWin_.ptr, dCodes_.ptr, dLens_.ptr, B, o, ds, dEnds_.ptr, dCalls_.ptr);
        else if (LMAX == 32)
            launch<32>(m, stream_, dJobs_.ptr, dWin_.ptr, dCodes_.ptr, dLens_.ptr, B, o, ds, dEnds_.ptr, dCalls_.ptr);
        else
            launch<64>(m, stream_, dJobs_.ptr, dWin_.ptr, dCodes_.ptr, dLens_.ptr, B, o, ds, dEnds_.ptr, dCalls_.ptr);
        stats.launches += 3;
        if (profiling) check(hipEventRecord(ev_[1], stream_), "event");
        check(hipMemcpyAsync(hEnds.data(), dEnds_.ptr, sizeof(DemuxEnd) * 2 * m, hipMemcpyDeviceToHost, stream_),
              "download");
        check(hipMemcpyAsync(hCalls.data(), dCalls_.ptr, sizeof(DemuxCall) * m, hipMemcpyDeviceToHost, stream_),
              "download");
        if (scores)
            check(hipMemcpyAsync(hScores.data(), dScores_.ptr, sizeof(int) * 2 * B * m, hipMemcpyDeviceToHost, stream_),
                  "download");
        check(hipStreamSynchronize(stream_), "sync");
        if (profiling) {
            float ms = 0.f;
            check(hipEventElapsedTime(&ms, ev_[0], ev_[1]), "event");
            stats.deviceMs += ms;
        }
        for (int k = 0; k < m; ++k) {
            const int r = readOf[g.begin + k];
            if (ends) {
                ends[(size_t)r * 2] = hEnds[(size_t)k * 2];
                ends[(size_t)r * 2 + 1] = hEnds[(size_t)k * 2 + 1];
            }
            if (calls) calls[r] = hCalls[k];
            if (scores)
                std::memcpy(scores + (size_t)r * 2 * B, hScores.data() + (size_t)k * 2 * B, sizeof(int) * 2 * B);
        }
    }
    // the stream is idle: buffers that growth retired can go
    dWin_.trim();
    dJobs_.trim();
    dCodes_.trim();
    dLens_.trim();
    dScores_.trim();
    dEnds_.trim();
    dCalls_.trim();
}

}  // namespace demux
}  // namespace pbccs

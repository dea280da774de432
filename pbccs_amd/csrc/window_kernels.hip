// pbccs_amd/csrc/window_kernels.hip -- k_window_cuts / k_window_join and the engine's window workspace
// (window_kernels.hpp).
#include "window_kernels.hpp"

#include <algorithm>
#include <string>

namespace pbccs {
namespace window {

namespace {

constexpr int kBlock = 256;

void check(hipError_t e, const char* what)
{
    if (e == hipSuccess) return;
    (void)hipGetLastError();
    throw DeviceError(std::string("window: ") + what + ": " + hipGetErrorString(e));
}

// Rule 2 of §3.18.  a = the last anchor with h <= b: v_a + (b - h_a), lowered to the next anchor's v; with no anchor
// at or before b, the first anchor (h', v') stepped back: max(0, v' - (h' - b)).  Never past the read's end.
__global__ __launch_bounds__(kBlock) void k_window_cuts(const CutTask* __restrict__ tasks, int n,
                                                        const int* __restrict__ anchors, int* __restrict__ cuts)
{
    const int idx = blockIdx.x * kBlock + threadIdx.x;
    if (idx >= n) return;
    const CutTask t = tasks[idx];
    const int* a = anchors + 2 * t.anchorOff;
    int lo = 0, hi = t.nAnchors;   // the first anchor with h > b
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (a[2 * mid] <= t.b) lo = mid + 1;
        else hi = mid;
    }
    int c = 0;
    if (lo > 0) {
        c = a[2 * (lo - 1) + 1] + (t.b - a[2 * (lo - 1)]);
        if (lo < t.nAnchors) c = min(c, a[2 * lo + 1]);
    } else if (t.nAnchors > 0) {
        c = max(0, a[1] - (a[0] - t.b));
    }
    cuts[idx] = min(c, t.flen);
}

__device__ __forceinline__ int wave_scan_add(int v, int lane)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(v, d);
        if (lane >= d) v += o;
    }
    return v;
}

__device__ __forceinline__ int wave_scan_max(int v, int lane)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(v, d);
        if (lane >= d) v = max(v, o);
    }
    return v;
}

// One transcript (stored reversed: forward character x is tr[len - 1 - x]).  For every candidate p of [lo, hi] whose
// draft columns p - g .. p + g - 1 are taken by 2g neighbouring M, w[p - lo] = TargetToQueryPositions[p - s].
__device__ void note_candidates(const uint8_t* __restrict__ tr, int len, int s, int lo, int hi, int g, int* w,
                                int lane)
{
    int tBase = 0, qBase = 0, runBase = 0;   // target / query consumed, and the run of M that ends, before the chunk
    for (int x0 = 0; x0 < len; x0 += 64) {
        const int x = x0 + lane;
        const int c = x < len ? (int)tr[len - 1 - x] : 0;
        const int isM = c == 'M';
        const int isT = isM | (c == 'R') | (c == 'D');
        const int isQ = isM | (c == 'R') | (c == 'I');
        const int incT = wave_scan_add(isT, lane), incQ = wave_scan_add(isQ, lane);
        const int lastOther = wave_scan_max(isM ? -1 : lane, lane);
        const int run = lastOther < 0 ? runBase + lane + 1 : lane - lastOther;
        if (isM && run >= 2 * g) {
            const int col = tBase + incT - 1;     // the draft column of this M, relative to s
            const int p = s + col - g + 1;
            if (p >= lo && p <= hi) w[p - lo] = qBase + incQ - 1 - (g - 1);
        }
        tBase += __shfl(incT, 63);
        qBase += __shfl(incQ, 63);
        runBase = __shfl(run, 63);
        if (s + tBase - g > hi) break;   // every later column lies past the last candidate's run
    }
}

__global__ __launch_bounds__(64) void k_window_join(const JoinTask* __restrict__ tasks,
                                                    const uint8_t* __restrict__ transcripts, int* __restrict__ work,
                                                    JoinOut* __restrict__ outs)
{
    const JoinTask t = tasks[blockIdx.x];
    const int lane = threadIdx.x;
    const int nc = t.hi - t.lo + 1;
    JoinOut o;
    o.p = -1, o.cutA = 0, o.cutB = 0;
    if (nc <= 0) {
        if (lane == 0) outs[blockIdx.x] = o;
        return;
    }
    int* wa = work + t.workOff;
    int* wb = wa + nc;
    for (int c = lane; c < 2 * nc; c += 64) wa[c] = -1;
    __syncthreads();
    note_candidates(transcripts + t.offA, t.lenA, t.sA, t.lo, t.hi, t.guard, wa, lane);
    note_candidates(transcripts + t.offB, t.lenB, t.sB, t.lo, t.hi, t.guard, wb, lane);
    __syncthreads();
    // candidate number i: mid for 0, mid + d for 2d - 1, mid - d for 2d
    const int reach = max(t.hi - t.mid, t.mid - t.lo);
    bool found = false;
    for (int i0 = 0; i0 <= 2 * reach && !found; i0 += 64) {
        const int i = i0 + lane;
        const int d = (i + 1) >> 1;
        const int p = (i & 1) ? t.mid + d : t.mid - d;
        bool ok = i <= 2 * reach && p >= t.lo && p <= t.hi;
        int ca = 0, cb = 0;
        if (ok) {
            ca = wa[p - t.lo];
            cb = wb[p - t.lo];
            ok = ca >= 0 && cb >= 0;
        }
        const unsigned long long m = __ballot(ok);
        if (m) {
            found = true;
            if (lane == __ffsll((long long)m) - 1) {
                o.p = p, o.cutA = ca, o.cutB = cb;
                outs[blockIdx.x] = o;
            }
        }
    }
    if (!found && lane == 0) outs[blockIdx.x] = o;
}

}  // namespace

WindowRunner::WindowRunner(int device) : device_(device)
{
    check(hipSetDevice(device_), "hipSetDevice");
    check(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking), "hipStreamCreate");
}

WindowRunner::~WindowRunner()
{
    if (stream_) {
        (void)hipStreamSynchronize(stream_);
        (void)hipStreamDestroy(stream_);
    }
}

void WindowRunner::Cuts(const int* anchors, const std::vector<CutTask>& tasks, std::vector<int>* cuts)
{
    const int n = (int)tasks.size();
    cuts->assign((size_t)n, 0);
    if (n == 0) return;
    check(hipSetDevice(device_), "hipSetDevice");
    StreamScope scope(stream_);
    struct StreamIdle {
        hipStream_t s;
        ~StreamIdle() { (void)hipStreamSynchronize(s); }
    } idle{stream_};
    dCutTasks_.reserve((size_t)n, false);
    dCuts_.reserve((size_t)n, false);
    check(hipMemcpyAsync(dCutTasks_.ptr, tasks.data(), sizeof(CutTask) * n, hipMemcpyHostToDevice, stream_), "upload");
    hipLaunchKernelGGL(k_window_cuts, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, stream_, dCutTasks_.ptr, n,
                       anchors, dCuts_.ptr);
    check(hipGetLastError(), "k_window_cuts launch");
    cutLaunches++;
    check(hipMemcpyAsync(cuts->data(), dCuts_.ptr, sizeof(int) * n, hipMemcpyDeviceToHost, stream_), "download");
    check(hipStreamSynchronize(stream_), "sync");
    dCutTasks_.trim();
    dCuts_.trim();
}

void WindowRunner::Joins(const uint8_t* transcripts, std::vector<JoinTask>& tasks, std::vector<JoinOut>* out)
{
    const int n = (int)tasks.size();
    out->assign((size_t)n, JoinOut{-1, 0, 0});
    if (n == 0) return;
    long long workInts = 0;
    for (JoinTask& t : tasks) {
        t.workOff = workInts;
        workInts += 2LL * std::max(0, t.hi - t.lo + 1);
    }
    check(hipSetDevice(device_), "hipSetDevice");
    StreamScope scope(stream_);
    struct StreamIdle {
        hipStream_t s;
        ~StreamIdle() { (void)hipStreamSynchronize(s); }
    } idle{stream_};
    dJoinTasks_.reserve((size_t)n, false);
    dJoinOut_.reserve((size_t)n, false);
    dWork_.reserve((size_t)std::max(1LL, workInts), false);
    check(hipMemcpyAsync(dJoinTasks_.ptr, tasks.data(), sizeof(JoinTask) * n, hipMemcpyHostToDevice, stream_), "upload");
    hipLaunchKernelGGL(k_window_join, dim3(n), dim3(64), 0, stream_, dJoinTasks_.ptr, transcripts, dWork_.ptr,
                       dJoinOut_.ptr);
    check(hipGetLastError(), "k_window_join launch");
    joinLaunches++;
    check(hipMemcpyAsync(out->data(), dJoinOut_.ptr, sizeof(JoinOut) * n, hipMemcpyDeviceToHost, stream_), "download");
    check(hipStreamSynchronize(stream_), "sync");
    dJoinTasks_.trim();
    dJoinOut_.trim();
    dWork_.trim();
}

}  // namespace window
}  // namespace pbccs

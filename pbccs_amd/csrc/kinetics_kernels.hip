// pbccs_amd/csrc/kinetics_kernels.hip -- k_kin_columns, k_kin_reduce and the engine's kinetics workspace
// (kinetics_kernels.hpp).
#include "kinetics_kernels.hpp"

#include <algorithm>
#include <cstring>
#include <stdexcept>
#include <string>

namespace pbccs {
namespace kinetics {

namespace {

void check(hipError_t e, const char* what)
{
    if (e == hipSuccess) return;
    (void)hipGetLastError();
    throw DeviceError(std::string("kinetics: ") + what + ": " + hipGetErrorString(e));
}

// One wavefront per read.  Lane l of chunk c holds transcript character 64 c + l; its target and query positions
// are the carries plus the target- / query-advancing lanes below it.
__global__ __launch_bounds__(64) void k_kin_columns(const KinRead* __restrict__ reads,
                                                    const uint8_t* __restrict__ tr, int* __restrict__ qidx,
                                                    int* __restrict__ contributed)
{
    const KinRead r = reads[blockIdx.x];
    const int lane = threadIdx.x;
    const unsigned long long below = (1ull << lane) - 1ull;
    const int nT = r.te - r.tb;
    int t = 0, q = r.rb;   // the chunk's first target position (from tb) and oriented query position
    bool any = false;
    for (int base = 0; base < r.trLen; base += 64) {
        const int k = base + lane;
        const int ch = k < r.trLen ? tr[r.trOff + k] : 0;
        const bool both = ch == 'M' || ch == 'R';
        const bool advT = both || ch == 'D';
        const bool advQ = both || ch == 'I';
        const unsigned long long mT = __ballot(advT), mQ = __ballot(advQ);
        const int tp = t + __popcll(mT & below);
        const int qp = q + __popcll(mQ & below);
        // the host checked the transcript against [tb, te) and I; the guards keep a store inside the extent anyway
        if (advT && tp < nT) qidx[r.qidxOff + tp] = both && qp < r.I ? (r.rc ? r.I - 1 - qp : qp) : -1;
        any = any || (mT & mQ) != 0;
        t += __popcll(mT);
        q += __popcll(mQ);
    }
    if (lane == 0) contributed[blockIdx.x] = any ? 1 : 0;
}

__device__ __forceinline__ unsigned rounded_mean(unsigned long long s, int n)
{
    if (n == 0) return 0u;
    const unsigned long long m = (2ull * s + (unsigned long long)n) / (2ull * (unsigned long long)n);
    return m < 65535ull ? (unsigned)m : 65535u;
}

// One thread per (ZMW, strand, position).  The block's ZMW, strand and the read records are the same for every
// thread of the block; adjacent threads read adjacent qidx entries.
__global__ __launch_bounds__(kReduceThreads) void k_kin_reduce(
    const KinBlock* __restrict__ blocks, const KinZmw* __restrict__ zmws, const KinRead* __restrict__ reads,
    const int* __restrict__ qidx, const int* __restrict__ contributed, const uint16_t* __restrict__ frames,
    uint16_t* __restrict__ mean, uint8_t* __restrict__ code, int* __restrict__ cov, int* __restrict__ counts)
{
    const KinBlock b = blocks[blockIdx.x];
    const KinZmw z = zmws[b.zmw];
    const int p = b.p0 + (int)threadIdx.x;
    if (p >= z.L) return;
    unsigned long long sIp = 0, sPw = 0;
    int nIp = 0, nPw = 0, nc = 0;
    for (int k = z.readBegin; k < z.readEnd; ++k) {
        const KinRead& r = reads[k];
        if (r.rc != b.strand) continue;
        const bool hasIp = r.ipOff >= 0, hasPw = r.pwOff >= 0;
        nc += (contributed[k] != 0 && (hasIp || hasPw)) ? 1 : 0;
        if (p < r.tb || p >= r.te) continue;
        const int qi = qidx[r.qidxOff + (p - r.tb)];
        if (qi < 0) continue;
        if (hasIp) {
            sIp += frames[r.ipOff + qi];
            ++nIp;
        }
        if (hasPw) {
            sPw += frames[r.pwOff + qi];
            ++nPw;
        }
    }
    const unsigned mIp = rounded_mean(sIp, nIp), mPw = rounded_mean(sPw, nPw);
    const long long at = z.outOff + 2LL * b.strand * z.L + (b.strand ? z.L - 1 - p : p);
    mean[at] = (uint16_t)mIp;
    mean[at + z.L] = (uint16_t)mPw;
    code[at] = (uint8_t)codec_v1_encode(mIp);
    code[at + z.L] = (uint8_t)codec_v1_encode(mPw);
    cov[at] = nIp;
    cov[at + z.L] = nPw;
    if (p == 0) counts[2 * b.zmw + b.strand] = nc;
}

// kUsed, kEmptyExtent, or throws: the checks that keep every device index inside its buffer
int vet(const ReadView& r, int L)
{
    if (r.trLen < 0 || (r.trLen > 0 && !r.tr)) throw std::invalid_argument("kinetics: bad transcript");
    if (r.I < 0 || r.rb < 0 || r.tb < 0 || r.te < r.tb || r.te > L)
        throw std::invalid_argument("kinetics: a read's extents leave the consensus or the read");
    long long nT = 0, nQ = 0, nB = 0;
    for (int k = 0; k < r.trLen; ++k) {
        const char c = r.tr[k];
        if (c == 'M' || c == 'R') {
            ++nT, ++nQ, ++nB;
        } else if (c == 'D') {
            ++nT;
        } else if (c == 'I') {
            ++nQ;
        } else {
            throw std::invalid_argument("kinetics: not a transcript character");
        }
    }
    if (nT != r.te - r.tb) throw std::invalid_argument("kinetics: the transcript does not span [tb, te)");
    if (r.rb + nQ > r.I) throw std::invalid_argument("kinetics: the transcript runs past the read's end");
    (void)nB;
    return (nT == 0 || nQ == 0) ? kEmptyExtent : kUsed;
}

}  // namespace

KineticsRunner::KineticsRunner(int device) : device_(device)
{
    check(hipSetDevice(device_), "hipSetDevice");
    check(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking), "hipStreamCreate");
    for (auto& e : ev_) check(hipEventCreate(&e), "hipEventCreate");
}

KineticsRunner::~KineticsRunner()
{
    if (stream_) {
        (void)hipStreamSynchronize(stream_);
        (void)hipStreamDestroy(stream_);
    }
    for (auto& e : ev_)
        if (e) (void)hipEventDestroy(e);
}

void KineticsRunner::Run(const ZmwView* zmws, int nz, ZmwOut* out)
{
    // host part: statuses, the device reads (grouped by ZMW, input order) and the pools' sizes
    std::vector<KinRead> reads;
    std::vector<KinZmw> zs((size_t)std::max(0, nz));
    std::vector<KinBlock> blocks;
    std::vector<const ReadView*> src;
    std::vector<std::vector<int>> status((size_t)std::max(0, nz));
    long long trBytes = 0, nQidx = 0, nFrames = 0, sumL = 0, columns = 0;
    for (int z = 0; z < nz; ++z) {
        const ZmwView& Z = zmws[z];
        if (Z.L < 0 || Z.n < 0 || (Z.n > 0 && !Z.reads)) throw std::invalid_argument("kinetics: bad ZMW");
        status[z].assign((size_t)Z.n, kUsed);
        zs[z].outOff = 4 * sumL;
        zs[z].L = Z.L;
        zs[z].readBegin = (int)reads.size();
        for (int k = 0; k < Z.n; ++k) {
            const ReadView& r = Z.reads[k];
            const int st = r.skip != kUsed ? r.skip : vet(r, Z.L);
            status[z][k] = st;
            if (st != kUsed) continue;
            KinRead d;
            d.trOff = trBytes;
            d.qidxOff = nQidx;
            d.ipOff = r.ip ? nFrames : -1;
            if (r.ip) nFrames += r.I;
            d.pwOff = r.pw ? nFrames : -1;
            if (r.pw) nFrames += r.I;
            d.trLen = r.trLen;
            d.I = r.I;
            d.rc = r.rc ? 1 : 0;
            d.rb = r.rb;
            d.tb = r.tb;
            d.te = r.te;
            trBytes += r.trLen;
            nQidx += r.te - r.tb;
            columns += r.trLen;
            reads.push_back(d);
            src.push_back(&r);
        }
        zs[z].readEnd = (int)reads.size();
        for (int s = 0; s < 2; ++s)
            for (int p0 = 0; p0 < Z.L; p0 += kReduceThreads) blocks.push_back(KinBlock{z, s, p0});
        sumL += Z.L;
    }
    for (int z = 0; z < nz; ++z) {
        stats.reads += zmws[z].n;
        for (int st : status[z]) {
            stats.unmapped += st == kUnmapped;
            stats.emptyExtent += st == kEmptyExtent;
            stats.alignFailed += st == kAlignFailed;
        }
        if (out[z].readStatus)
            for (int k = 0; k < zmws[z].n; ++k) out[z].readStatus[k] = status[z][k];
        out[z].contributed[0] = out[z].contributed[1] = 0;
    }
    if (sumL == 0) return;   // nothing to write

    const size_t nr = reads.size();
    std::vector<uint8_t> tr((size_t)trBytes);
    std::vector<uint16_t> frames((size_t)nFrames);
    for (size_t k = 0; k < nr; ++k) {
        const ReadView& r = *src[k];
        if (r.trLen) std::memcpy(tr.data() + reads[k].trOff, r.tr, (size_t)r.trLen);
        if (r.ip && r.I) std::memcpy(frames.data() + reads[k].ipOff, r.ip, sizeof(uint16_t) * (size_t)r.I);
        if (r.pw && r.I) std::memcpy(frames.data() + reads[k].pwOff, r.pw, sizeof(uint16_t) * (size_t)r.I);
    }
    const size_t nOut = (size_t)(4 * sumL);
    std::vector<uint16_t> hMean(nOut);
    std::vector<uint8_t> hCode(nOut);
    std::vector<int> hCov(nOut), hCounts((size_t)(2 * nz));

    check(hipSetDevice(device_), "hipSetDevice");
    StreamScope scope(stream_);
    // leaves (also by exception) only once the stream is idle: queued copies read and write the vectors above
    struct StreamIdle {
        hipStream_t s;
        ~StreamIdle() { (void)hipStreamSynchronize(s); }
    } idle{stream_};
    dTr_.reserve(std::max<size_t>(1, tr.size()), false);
    dFrames_.reserve(std::max<size_t>(1, frames.size()), false);
    dQidx_.reserve(std::max<size_t>(1, (size_t)nQidx), false);
    dContrib_.reserve(std::max<size_t>(1, nr), false);
    dReads_.reserve(std::max<size_t>(1, nr), false);
    dZmws_.reserve((size_t)nz, false);
    dBlocks_.reserve(blocks.size(), false);
    dMean_.reserve(nOut, false);
    dCode_.reserve(nOut, false);
    dCov_.reserve(nOut, false);
    dCounts_.reserve((size_t)(2 * nz), false);
    if (!tr.empty()) check(hipMemcpyAsync(dTr_.ptr, tr.data(), tr.size(), hipMemcpyHostToDevice, stream_), "upload");
    if (!frames.empty())
        check(hipMemcpyAsync(dFrames_.ptr, frames.data(), sizeof(uint16_t) * frames.size(), hipMemcpyHostToDevice,
                             stream_),
              "upload");
    if (nr) check(hipMemcpyAsync(dReads_.ptr, reads.data(), sizeof(KinRead) * nr, hipMemcpyHostToDevice, stream_), "upload");
    check(hipMemcpyAsync(dZmws_.ptr, zs.data(), sizeof(KinZmw) * (size_t)nz, hipMemcpyHostToDevice, stream_), "upload");
    check(hipMemcpyAsync(dBlocks_.ptr, blocks.data(), sizeof(KinBlock) * blocks.size(), hipMemcpyHostToDevice, stream_),
          "upload");
    check(hipMemsetAsync(dCounts_.ptr, 0, sizeof(int) * (size_t)(2 * nz), stream_), "memset");
    if (profiling) check(hipEventRecord(ev_[0], stream_), "event");
    if (nr) {
        hipLaunchKernelGGL(k_kin_columns, dim3((unsigned)nr), dim3(64), 0, stream_, dReads_.ptr, dTr_.ptr, dQidx_.ptr,
                           dContrib_.ptr);
        check(hipGetLastError(), "k_kin_columns launch");
        stats.launches++;
    }
    if (profiling) check(hipEventRecord(ev_[1], stream_), "event");
    hipLaunchKernelGGL(k_kin_reduce, dim3((unsigned)blocks.size()), dim3(kReduceThreads), 0, stream_, dBlocks_.ptr,
                       dZmws_.ptr, dReads_.ptr, dQidx_.ptr, dContrib_.ptr, dFrames_.ptr, dMean_.ptr, dCode_.ptr,
                       dCov_.ptr, dCounts_.ptr);
    check(hipGetLastError(), "k_kin_reduce launch");
    stats.launches++;
    if (profiling) check(hipEventRecord(ev_[2], stream_), "event");
    check(hipMemcpyAsync(hMean.data(), dMean_.ptr, sizeof(uint16_t) * nOut, hipMemcpyDeviceToHost, stream_), "download");
    check(hipMemcpyAsync(hCode.data(), dCode_.ptr, nOut, hipMemcpyDeviceToHost, stream_), "download");
    check(hipMemcpyAsync(hCov.data(), dCov_.ptr, sizeof(int) * nOut, hipMemcpyDeviceToHost, stream_), "download");
    check(hipMemcpyAsync(hCounts.data(), dCounts_.ptr, sizeof(int) * (size_t)(2 * nz), hipMemcpyDeviceToHost, stream_),
          "download");
    check(hipStreamSynchronize(stream_), "sync");
    if (profiling) {
        float a = 0.f, b = 0.f;
        check(hipEventElapsedTime(&a, ev_[0], ev_[1]), "event");
        check(hipEventElapsedTime(&b, ev_[1], ev_[2]), "event");
        stats.columnsMs += a;
        stats.reduceMs += b;
    }
    // the stream is idle: buffers that growth retired can go
    dTr_.trim();
    dFrames_.trim();
    dQidx_.trim();
    dContrib_.trim();
    dReads_.trim();
    dZmws_.trim();
    dBlocks_.trim();
    dMean_.trim();
    dCode_.trim();
    dCov_.trim();
    dCounts_.trim();
    stats.columns += columns;
    stats.positions += 2 * sumL;

    for (int z = 0; z < nz; ++z) {
        const size_t L = (size_t)zs[z].L;
        for (int v = 0; v < 4; ++v) {
            const size_t at = (size_t)zs[z].outOff + (size_t)v * L;
            if (!L) break;
            if (out[z].mean[v]) std::memcpy(out[z].mean[v], hMean.data() + at, sizeof(uint16_t) * L);
            if (out[z].code[v]) std::memcpy(out[z].code[v], hCode.data() + at, L);
            if (out[z].coverage[v]) std::memcpy(out[z].coverage[v], hCov.data() + at, sizeof(int) * L);
        }
        out[z].contributed[0] = hCounts[2 * (size_t)z];
        out[z].contributed[1] = hCounts[2 * (size_t)z + 1];
    }
}

}  // namespace kinetics
}  // namespace pbccs

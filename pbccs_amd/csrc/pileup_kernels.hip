// pbccs_amd/csrc/pileup_kernels.hip -- k_pile_columns, k_pile_reduce, k_pile_scan, k_pile_rows and the engine's
// pileup workspace (pileup_kernels.hpp).
#include "pileup_kernels.hpp"

#include <algorithm>
#include <cstring>
#include <stdexcept>
#include <string>

namespace pbccs {
namespace pileup {

namespace {

void check(hipError_t e, const char* what)
{
    if (e == hipSuccess) return;
    (void)hipGetLastError();
    throw DeviceError(std::string("pileup: ") + what + ": " + hipGetErrorString(e));
}

// A C G T -> 0..3, anything else 5; the complement of a base code c < 4 is 3 - c
__device__ __forceinline__ int base_code(int ch, int rc)
{
    const int k = ch == 'A' ? 0 : ch == 'C' ? 1 : ch == 'G' ? 2 : ch == 'T' ? 3 : 5;
    return (rc && k < 4) ? 3 - k : k;
}

// the character of oriented position q of a read
__device__ __forceinline__ int oriented_char(const PileRead& r, const uint8_t* __restrict__ seq, int q)
{
    if (q < 0 || q >= r.I) return 'N';   // never, for a vetted read: keeps the load inside the text
    const int ch = seq[r.seqOff + (r.rc ? r.I - 1 - q : q)];
    if (!r.rc) return ch;
    return ch == 'A' ? 'T' : ch == 'C' ? 'G' : ch == 'G' ? 'C' : ch == 'T' ? 'A' : 'N';
}

// One wavefront per read.  Lane l of chunk c holds transcript character 64 c + l.
__global__ __launch_bounds__(64) void k_pile_columns(const PileRead* __restrict__ reads,
                                                     const uint8_t* __restrict__ tr, const uint8_t* __restrict__ seq,
                                                     uint8_t* __restrict__ code, int* __restrict__ insLen,
                                                     int* __restrict__ qAt, int* __restrict__ colCounts)
{
    const PileRead r = reads[blockIdx.x];
    const int lane = threadIdx.x;
    const unsigned long long below = (1ull << lane) - 1ull;
    const int nT = r.te - r.tb;
    int t = 0, q = r.rb;   // the chunk's first target position (from tb) and oriented query position
    int open = 0;          // the length of the I run that reaches the chunk's start
    int nM = 0, nR = 0, nI = 0, nD = 0;
    for (int base = 0; base < r.trLen; base += 64) {
        const int k = base + lane;
        const int ch = k < r.trLen ? tr[r.trOff + k] : 0;
        const bool isM = ch == 'M', isR = ch == 'R', isI = ch == 'I', isD = ch == 'D';
        const bool both = isM || isR;
        const bool advT = both || isD;
        const unsigned long long mM = __ballot(isM), mR = __ballot(isR), mI = __ballot(isI), mD = __ballot(isD);
        const unsigned long long mT = mM | mR | mD, mQ = mM | mR | mI;
        const int tp = t + __popcll(mT & below);
        const int qp = q + __popcll(mQ & below);
        // the I run that ends right below this lane: back to the highest lane below that holds no I, or through
        // the chunk's start into the open run
        const unsigned long long stopBelow = ~mI & below;
        const int run = stopBelow ? lane - 64 + __clzll((long long)stopBelow) : lane + open;
        // the host checked the transcript against [tb, te) and I; the guards keep a store inside the extent anyway
        if (advT && tp < nT) {
            int c = 4;
            if (both) c = qp < r.I ? base_code(seq[r.seqOff + (r.rc ? r.I - 1 - qp : qp)], r.rc) : 5;
            code[r.colOff + tp] = (uint8_t)c;
            insLen[r.slotOff + tp] = run;
            qAt[r.slotOff + tp] = qp - run;
        }
        const int nv = min(64, r.trLen - base);
        const unsigned long long valid = nv == 64 ? ~0ull : (1ull << nv) - 1ull;
        const unsigned long long stop = ~mI & valid;
        open = stop ? nv - 64 + __clzll((long long)stop) : open + nv;
        t += __popcll(mT);
        q += __popcll(mQ);
        nM += __popcll(mM);
        nR += __popcll(mR);
        nI += __popcll(mI);
        nD += __popcll(mD);
    }
    if (lane == 0) {
        insLen[r.slotOff + nT] = open;   // the slot after the read's last consensus position
        qAt[r.slotOff + nT] = q - open;
        colCounts[4 * blockIdx.x + 0] = nM;
        colCounts[4 * blockIdx.x + 1] = nR;
        colCounts[4 * blockIdx.x + 2] = nI;
        colCounts[4 * blockIdx.x + 3] = nD;
    }
}

// One thread per (ZMW, slot); slot s < L is also position s.  The block's ZMW and the read records are the same
// for every thread of the block; adjacent threads read adjacent code bytes and slots.
__global__ __launch_bounds__(kReduceThreads) void k_pile_reduce(
    const PileBlock* __restrict__ blocks, const PileZmw* __restrict__ zmws, const PileRead* __restrict__ reads,
    const uint8_t* __restrict__ cons, const uint8_t* __restrict__ code, const int* __restrict__ insLen,
    int* __restrict__ counts, int* __restrict__ insReads, int* __restrict__ insBases, int* __restrict__ slotCov,
    int* __restrict__ cov, int* __restrict__ maxIns, uint8_t* __restrict__ plurality,
    uint8_t* __restrict__ insPlurality, unsigned long long* __restrict__ covSum)
{
    __shared__ int waveSum[kReduceThreads / 64];
    const PileBlock b = blocks[blockIdx.x];
    const PileZmw z = zmws[b.zmw];
    const int s = b.s0 + (int)threadIdx.x;
    const bool isSlot = s <= z.L, isPos = s < z.L;
    int f0 = 0, f1 = 0, f2 = 0, f3 = 0, f4 = 0, f5 = 0, r0 = 0, r1 = 0, r2 = 0, r3 = 0, r4 = 0, r5 = 0;
    int ir0 = 0, ir1 = 0, ib0 = 0, ib1 = 0, sc = 0, mx = 0;
    if (isSlot) {
        for (int k = z.readBegin; k < z.readEnd; ++k) {
            const PileRead& r = reads[k];
            if (s < r.tb || s > r.te) continue;
            ++sc;
            const int il = insLen[r.slotOff + (s - r.tb)];
            const int has = il > 0 ? 1 : 0;
            ir0 += r.rc ? 0 : has;
            ir1 += r.rc ? has : 0;
            ib0 += r.rc ? 0 : il;
            ib1 += r.rc ? il : 0;
            mx = max(mx, il);
            if (s >= r.te) continue;
            // strand and code in one number: twelve compares and adds, no indexed registers
            const int c = (r.rc ? 6 : 0) + (int)code[r.colOff + (s - r.tb)];
            f0 += c == 0; f1 += c == 1; f2 += c == 2; f3 += c == 3; f4 += c == 4; f5 += c == 5;
            r0 += c == 6; r1 += c == 7; r2 += c == 8; r3 += c == 9; r4 += c == 10; r5 += c == 11;
        }
        const long long so = 2 * z.slotOff;
        insReads[so + s] = ir0;
        insReads[so + (z.L + 1) + s] = ir1;
        insBases[so + s] = ib0;
        insBases[so + (z.L + 1) + s] = ib1;
        slotCov[z.slotOff + s] = sc;
        maxIns[z.slotOff + s] = mx;
        insPlurality[z.slotOff + s] = (uint8_t)(2 * (ir0 + ir1) > sc ? 1 : 0);
    }
    int total = 0;
    if (isPos) {
        int* cf = counts + 12 * z.posOff + 6LL * s;
        int* cr = cf + 6LL * z.L;
        cf[0] = f0; cf[1] = f1; cf[2] = f2; cf[3] = f3; cf[4] = f4; cf[5] = f5;
        cr[0] = r0; cr[1] = r1; cr[2] = r2; cr[3] = r3; cr[4] = r4; cr[5] = r5;
        total = f0 + f1 + f2 + f3 + f4 + f5 + r0 + r1 + r2 + r3 + r4 + r5;
        cov[z.posOff + s] = total;
        const int j0 = f0 + r0, j1 = f1 + r1, j2 = f2 + r2, j3 = f3 + r3, j4 = f4 + r4;
        const int best = max(max(max(j0, j1), max(j2, j3)), j4);
        const int low = j0 == best ? 0 : j1 == best ? 1 : j2 == best ? 2 : j3 == best ? 3 : 4;
        const int ch = cons[z.posOff + s];
        const int own = ch == 'A' ? 0 : ch == 'C' ? 1 : ch == 'G' ? 2 : ch == 'T' ? 3 : 5;
        const int jOwn = own == 0 ? j0 : own == 1 ? j1 : own == 2 ? j2 : own == 3 ? j3 : -1;
        plurality[z.posOff + s] = (uint8_t)(best == 0 ? 255 : jOwn == best ? own : low);
    }
    // cov_sum: the wave's sum by shuffles, the block's through LDS, one integer atomic per block
    for (int d = 32; d > 0; d >>= 1) total += __shfl_down(total, d, 64);
    if ((threadIdx.x & 63) == 0) waveSum[threadIdx.x >> 6] = total;
    __syncthreads();
    if (threadIdx.x == 0) {
        int t = 0;
        for (int w = 0; w < kReduceThreads / 64; ++w) t += waveSum[w];
        if (t) atomicAdd(&covSum[b.zmw], (unsigned long long)t);
    }
}

// One block per ZMW: first[s] = s + the exclusive sum of maxins, in tiles of a block with a carry; col and width
// follow.
__global__ __launch_bounds__(kScanThreads) void k_pile_scan(const PileZmw* __restrict__ zmws,
                                                            const int* __restrict__ maxIns, int* __restrict__ first,
                                                            int* __restrict__ col, int* __restrict__ width)
{
    __shared__ int waveSum[kScanThreads / 64];
    const PileZmw z = zmws[blockIdx.x];
    const int n = z.L + 1;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int carry = 0;   // the same in every thread
    for (int base = 0; base < n; base += kScanThreads) {
        const int s = base + (int)threadIdx.x;
        const int v = s < n ? maxIns[z.slotOff + s] : 0;
        int x = v;   // the wave's inclusive scan
        for (int d = 1; d < 64; d <<= 1) {
            const int y = __shfl_up(x, d, 64);
            if (lane >= d) x += y;
        }
        if (lane == 63) waveSum[wave] = x;
        __syncthreads();
        int before = 0, tile = 0;
        for (int w = 0; w < kScanThreads / 64; ++w) {
            const int ws = waveSum[w];
            before += w < wave ? ws : 0;
            tile += ws;
        }
        const int excl = carry + before + x - v;
        if (s < n) first[z.slotOff + s] = s + excl;
        if (s < z.L) col[z.posOff + s] = s + excl + v;
        carry += tile;
        __syncthreads();   // waveSum is written again in the next tile
    }
    if (threadIdx.x == 0) width[blockIdx.x] = z.L + carry;
}

// One thread per (read, slot j of the read's extent): the slot's inserted bases and padding, then the position's
// cell.
__global__ __launch_bounds__(kRowThreads) void k_pile_rows(
    const PileRowBlock* __restrict__ blocks, const PileZmw* __restrict__ zmws, const PileRead* __restrict__ reads,
    const uint8_t* __restrict__ seq, const uint8_t* __restrict__ code, const int* __restrict__ insLen,
    const int* __restrict__ qAt, const int* __restrict__ maxIns, const int* __restrict__ first,
    const int* __restrict__ width, const long long* __restrict__ rowBase, uint8_t* __restrict__ rows)
{
    const PileRowBlock b = blocks[blockIdx.x];
    const PileRead r = reads[b.read];
    const PileZmw z = zmws[r.zmw];
    const int nT = r.te - r.tb;
    const int j = b.j0 + (int)threadIdx.x;
    if (j > nT) return;
    const int W = width[r.zmw];
    uint8_t* row = rows + rowBase[r.zmw] + (long long)r.row * W;
    const int s = r.tb + j;
    const int f = first[z.slotOff + s], mx = maxIns[z.slotOff + s];
    const int k = min(insLen[r.slotOff + j], mx), q0 = qAt[r.slotOff + j];
    const int at = j == 0 ? f + mx - k : f;
    if (f < 0 || f + mx + (j < nT ? 1 : 0) > W) return;   // never: first and maxins come from these very reads
    for (int i = 0; i < k; ++i) row[at + i] = (uint8_t)oriented_char(r, seq, q0 + i);
    if (j > 0 && j < nT)
        for (int i = k; i < mx; ++i) row[f + i] = '-';
    if (j < nT) {
        const int c = code[r.colOff + j];
        row[f + mx] = (uint8_t)(c == 4 ? '-' : oriented_char(r, seq, q0 + k));
    }
}

// kUsed, kEmptyExtent, or throws: the checks that keep every device index inside its buffer (KineticsRunner's)
int vet(const ReadView& r, int L)
{
    if (r.trLen < 0 || (r.trLen > 0 && !r.tr)) throw std::invalid_argument("pileup: bad transcript");
    if (r.I < 0 || r.rb < 0 || r.tb < 0 || r.te < r.tb || r.te > L)
        throw std::invalid_argument("pileup: a read's extents leave the consensus or the read");
    if (r.I > 0 && !r.seq) throw std::invalid_argument("pileup: a read without its text");
    long long nT = 0, nQ = 0;
    for (int k = 0; k < r.trLen; ++k) {
        const char c = r.tr[k];
        if (c == 'M' || c == 'R') {
            ++nT, ++nQ;
        } else if (c == 'D') {
            ++nT;
        } else if (c == 'I') {
            ++nQ;
        } else {
            throw std::invalid_argument("pileup: not a transcript character");
        }
    }
    if (nT != r.te - r.tb) throw std::invalid_argument("pileup: the transcript does not span [tb, te)");
    if (r.rb + nQ > r.I) throw std::invalid_argument("pileup: the transcript runs past the read's end");
    return (nT == 0 || nQ == 0) ? kEmptyExtent : kUsed;
}

template <class T>
void up(DevVec<T>& d, const std::vector<T>& h, hipStream_t st)
{
    d.reserve(std::max<size_t>(1, h.size()), false);
    if (!h.empty()) check(hipMemcpyAsync(d.ptr, h.data(), sizeof(T) * h.size(), hipMemcpyHostToDevice, st), "upload");
}

template <class T>
void down(std::vector<T>& h, const DevVec<T>& d, hipStream_t st)
{
    if (!h.empty()) check(hipMemcpyAsync(h.data(), d.ptr, sizeof(T) * h.size(), hipMemcpyDeviceToHost, st), "download");
}

}  // namespace

PileupRunner::PileupRunner(int device) : device_(device)
{
    check(hipSetDevice(device_), "hipSetDevice");
    check(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking), "hipStreamCreate");
    for (auto& e : ev_) check(hipEventCreate(&e), "hipEventCreate");
}

PileupRunner::~PileupRunner()
{
    if (stream_) {
        (void)hipStreamSynchronize(stream_);
        (void)hipStreamDestroy(stream_);
    }
    for (auto& e : ev_)
        if (e) (void)hipEventDestroy(e);
}

void PileupRunner::Run(const ZmwView* zmws, int nz, ZmwOut* out, MsaOut* msa)
{
    // host part: statuses, the device reads (grouped by ZMW, input order) and the pools' sizes
    std::vector<PileRead> reads;
    std::vector<PileZmw> zs((size_t)std::max(0, nz));
    std::vector<PileBlock> blocks;
    std::vector<PileRowBlock> rowBlocks;
    std::vector<const ReadView*> src;
    std::vector<std::pair<int, int>> where;   // (ZMW, read) of each device read
    std::vector<std::vector<int>> status((size_t)std::max(0, nz));
    long long trBytes = 0, seqBytes = 0, nCols = 0, nSlots = 0, sumL = 0, columns = 0;
    bool wantRows = false;
    for (int z = 0; z < nz; ++z) {
        const ZmwView& Z = zmws[z];
        if (Z.L < 0 || Z.n < 0 || (Z.n > 0 && !Z.reads) || (Z.L > 0 && !Z.cons))
            throw std::invalid_argument("pileup: bad ZMW");
        status[z].assign((size_t)Z.n, kUsed);
        zs[z].posOff = sumL;
        zs[z].slotOff = sumL + z;
        zs[z].L = Z.L;
        zs[z].readBegin = (int)reads.size();
        const bool rowsHere = msa && msa[z].rows;
        wantRows = wantRows || rowsHere;
        for (int k = 0; k < Z.n; ++k) {
            const ReadView& r = Z.reads[k];
            const int st = r.skip != kUsed ? r.skip : vet(r, Z.L);
            status[z][k] = st;
            if (st != kUsed) continue;
            PileRead d;
            d.trOff = trBytes;
            d.seqOff = seqBytes;
            d.colOff = nCols;
            d.slotOff = nSlots;
            d.trLen = r.trLen;
            d.I = r.I;
            d.rc = r.rc ? 1 : 0;
            d.rb = r.rb;
            d.tb = r.tb;
            d.te = r.te;
            d.zmw = z;
            d.row = k;
            trBytes += r.trLen;
            seqBytes += r.I;
            nCols += r.te - r.tb;
            nSlots += r.te - r.tb + 1;
            columns += r.trLen;
            if (rowsHere)
                for (int j0 = 0; j0 <= r.te - r.tb; j0 += kRowThreads)
                    rowBlocks.push_back(PileRowBlock{(int)reads.size(), j0});
            reads.push_back(d);
            src.push_back(&r);
            where.emplace_back(z, k);
        }
        zs[z].readEnd = (int)reads.size();
        for (int s0 = 0; s0 <= Z.L; s0 += kReduceThreads) blocks.push_back(PileBlock{z, s0});
        sumL += Z.L;
    }
    for (int z = 0; z < nz; ++z) {
        stats.reads += zmws[z].n;
        int used[2] = {0, 0};
        for (int k = 0; k < zmws[z].n; ++k) {
            const int st = status[z][k];
            stats.unmapped += st == kUnmapped;
            stats.emptyExtent += st == kEmptyExtent;
            stats.alignFailed += st == kAlignFailed;
            if (st == kUsed) used[zmws[z].reads[k].rc ? 1 : 0]++;
        }
        if (!out) continue;
        ZmwOut& o = out[z];
        o.covSum = 0;
        o.nUsed[0] = used[0];
        o.nUsed[1] = used[1];
        for (int k = 0; k < zmws[z].n; ++k) {
            if (o.readStatus) o.readStatus[k] = status[z][k];
            if (o.nMatch) o.nMatch[k] = 0;
            if (o.nMismatch) o.nMismatch[k] = 0;
            if (o.nIns) o.nIns[k] = 0;
            if (o.nDel) o.nDel[k] = 0;
        }
    }
    if (nz <= 0) return;

    const size_t nr = reads.size();
    const size_t totSlots = (size_t)(sumL + nz);
    std::vector<uint8_t> tr((size_t)trBytes), seq((size_t)seqBytes), cons((size_t)sumL);
    for (size_t k = 0; k < nr; ++k) {
        const ReadView& r = *src[k];
        if (r.trLen) std::memcpy(tr.data() + reads[k].trOff, r.tr, (size_t)r.trLen);
        if (r.I) std::memcpy(seq.data() + reads[k].seqOff, r.seq, (size_t)r.I);
    }
    for (int z = 0; z < nz; ++z)
        if (zs[z].L) std::memcpy(cons.data() + zs[z].posOff, zmws[z].cons, (size_t)zs[z].L);
    std::vector<int> hColCounts(4 * nr), hCounts((size_t)(12 * sumL)), hInsReads(2 * totSlots), hInsBases(2 * totSlots),
        hSlotCov(totSlots), hCov((size_t)sumL), hMaxIns(totSlots), hCol(msa ? (size_t)sumL : 0), hWidth(msa ? (size_t)nz : 0);
    std::vector<uint8_t> hPlur((size_t)sumL), hInsPlur(totSlots), hRows;
    std::vector<unsigned long long> hCovSum((size_t)nz);
    std::vector<long long> rowBase((size_t)nz, 0);

    check(hipSetDevice(device_), "hipSetDevice");
    StreamScope scope(stream_);
    // leaves (also by exception) only once the stream is idle: queued copies read and write the vectors above
    struct StreamIdle {
        hipStream_t s;
        ~StreamIdle() { (void)hipStreamSynchronize(s); }
    } idle{stream_};
    up(dTr_, tr, stream_);
    up(dSeq_, seq, stream_);
    up(dCons_, cons, stream_);
    up(dReads_, reads, stream_);
    up(dZmws_, zs, stream_);
    up(dBlocks_, blocks, stream_);
    dCode_.reserve(std::max<size_t>(1, (size_t)nCols), false);
    dInsLen_.reserve(std::max<size_t>(1, (size_t)nSlots), false);
    dQAt_.reserve(std::max<size_t>(1, (size_t)nSlots), false);
    dColCounts_.reserve(std::max<size_t>(1, 4 * nr), false);
    dCounts_.reserve(std::max<size_t>(1, (size_t)(12 * sumL)), false);
    dInsReads_.reserve(2 * totSlots, false);
    dInsBases_.reserve(2 * totSlots, false);
    dSlotCov_.reserve(totSlots, false);
    dCov_.reserve(std::max<size_t>(1, (size_t)sumL), false);
    dMaxIns_.reserve(totSlots, false);
    dPlur_.reserve(std::max<size_t>(1, (size_t)sumL), false);
    dInsPlur_.reserve(totSlots, false);
    dCovSum_.reserve((size_t)nz, false);
    check(hipMemsetAsync(dCovSum_.ptr, 0, sizeof(unsigned long long) * (size_t)nz, stream_), "memset");
    if (profiling) check(hipEventRecord(ev_[0], stream_), "event");
    if (nr) {
        hipLaunchKernelGGL(k_pile_columns, dim3((unsigned)nr), dim3(64), 0, stream_, dReads_.ptr, dTr_.ptr, dSeq_.ptr,
                           dCode_.ptr, dInsLen_.ptr, dQAt_.ptr, dColCounts_.ptr);
        check(hipGetLastError(), "k_pile_columns launch");
        stats.launches++;
    }
    if (profiling) check(hipEventRecord(ev_[1], stream_), "event");
    hipLaunchKernelGGL(k_pile_reduce, dim3((unsigned)blocks.size()), dim3(kReduceThreads), 0, stream_, dBlocks_.ptr,
                       dZmws_.ptr, dReads_.ptr, dCons_.ptr, dCode_.ptr, dInsLen_.ptr, dCounts_.ptr, dInsReads_.ptr,
                       dInsBases_.ptr, dSlotCov_.ptr, dCov_.ptr, dMaxIns_.ptr, dPlur_.ptr, dInsPlur_.ptr, dCovSum_.ptr);
    check(hipGetLastError(), "k_pile_reduce launch");
    stats.launches++;
    if (profiling) check(hipEventRecord(ev_[2], stream_), "event");
    bool ranRows = false;
    if (msa) {
        dFirst_.reserve(totSlots, false);
        dCol_.reserve(std::max<size_t>(1, (size_t)sumL), false);
        dWidth_.reserve((size_t)nz, false);
        hipLaunchKernelGGL(k_pile_scan, dim3((unsigned)nz), dim3(kScanThreads), 0, stream_, dZmws_.ptr, dMaxIns_.ptr,
                           dFirst_.ptr, dCol_.ptr, dWidth_.ptr);
        check(hipGetLastError(), "k_pile_scan launch");
        stats.launches++;
        if (profiling) check(hipEventRecord(ev_[3], stream_), "event");
        down(hWidth, dWidth_, stream_);
        down(hCol, dCol_, stream_);
        check(hipStreamSynchronize(stream_), "sync");   // the rows' layout needs the widths
        long long rowBytes = 0;
        for (int z = 0; z < nz; ++z) {
            msa[z].width = hWidth[z];
            if (!msa[z].rows) continue;
            if (msa[z].rowWidth != hWidth[z])
                throw std::invalid_argument("pileup: the rows were sized for another width");
            rowBase[z] = rowBytes;
            rowBytes += (long long)zmws[z].n * hWidth[z];
        }
        if (wantRows && rowBytes > 0) {
            hRows.resize((size_t)rowBytes);
            dRows_.reserve((size_t)rowBytes, false);
            check(hipMemsetAsync(dRows_.ptr, ' ', (size_t)rowBytes, stream_), "memset");
            if (!rowBlocks.empty()) {
                up(dRowBase_, rowBase, stream_);
                up(dRowBlocks_, rowBlocks, stream_);
                hipLaunchKernelGGL(k_pile_rows, dim3((unsigned)rowBlocks.size()), dim3(kRowThreads), 0, stream_,
                                   dRowBlocks_.ptr, dZmws_.ptr, dReads_.ptr, dSeq_.ptr, dCode_.ptr, dInsLen_.ptr,
                                   dQAt_.ptr, dMaxIns_.ptr, dFirst_.ptr, dWidth_.ptr, dRowBase_.ptr, dRows_.ptr);
                check(hipGetLastError(), "k_pile_rows launch");
                stats.launches++;
                ranRows = true;
            }
            if (profiling) check(hipEventRecord(ev_[4], stream_), "event");
            down(hRows, dRows_, stream_);
        }
    }
    if (out) {
        down(hColCounts, dColCounts_, stream_);
        down(hCounts, dCounts_, stream_);
        down(hInsReads, dInsReads_, stream_);
        down(hInsBases, dInsBases_, stream_);
        down(hSlotCov, dSlotCov_, stream_);
        down(hCov, dCov_, stream_);
        down(hMaxIns, dMaxIns_, stream_);
        down(hPlur, dPlur_, stream_);
        down(hInsPlur, dInsPlur_, stream_);
        down(hCovSum, dCovSum_, stream_);
    }
    check(hipStreamSynchronize(stream_), "sync");
    if (profiling) {
        float a = 0.f;
        check(hipEventElapsedTime(&a, ev_[0], ev_[1]), "event");
        stats.columnsMs += a;
        check(hipEventElapsedTime(&a, ev_[1], ev_[2]), "event");
        stats.reduceMs += a;
        if (msa) {
            check(hipEventElapsedTime(&a, ev_[2], ev_[3]), "event");
            stats.scanMs += a;
        }
        if (ranRows) {
            check(hipEventElapsedTime(&a, ev_[3], ev_[4]), "event");
            stats.rowsMs += a;
        }
    }
    // the stream is idle: buffers that growth retired can go
    dTr_.trim(), dSeq_.trim(), dCons_.trim(), dCode_.trim(), dPlur_.trim(), dInsPlur_.trim(), dRows_.trim();
    dInsLen_.trim(), dQAt_.trim(), dColCounts_.trim(), dCounts_.trim(), dInsReads_.trim(), dInsBases_.trim();
    dSlotCov_.trim(), dCov_.trim(), dMaxIns_.trim(), dFirst_.trim(), dCol_.trim(), dWidth_.trim(), dCovSum_.trim();
    dRowBase_.trim(), dReads_.trim(), dZmws_.trim(), dBlocks_.trim(), dRowBlocks_.trim();
    stats.columns += columns;
    stats.slots += (long long)totSlots;

    for (int z = 0; z < nz; ++z) {
        const size_t L = (size_t)zs[z].L, po = (size_t)zs[z].posOff, so = (size_t)zs[z].slotOff;
        if (msa) {
            if (msa[z].col && L) std::memcpy(msa[z].col, hCol.data() + po, sizeof(int) * L);
            if (msa[z].rows && zmws[z].n && hWidth[z])
                std::memcpy(msa[z].rows, hRows.data() + rowBase[z], (size_t)zmws[z].n * (size_t)hWidth[z]);
        }
        if (!out) continue;
        ZmwOut& o = out[z];
        if (o.counts && L) std::memcpy(o.counts, hCounts.data() + 12 * po, sizeof(int) * 12 * L);
        if (o.insReads) std::memcpy(o.insReads, hInsReads.data() + 2 * so, sizeof(int) * 2 * (L + 1));
        if (o.insBases) std::memcpy(o.insBases, hInsBases.data() + 2 * so, sizeof(int) * 2 * (L + 1));
        if (o.slotCov) std::memcpy(o.slotCov, hSlotCov.data() + so, sizeof(int) * (L + 1));
        if (o.maxIns) std::memcpy(o.maxIns, hMaxIns.data() + so, sizeof(int) * (L + 1));
        if (o.insPlurality) std::memcpy(o.insPlurality, hInsPlur.data() + so, L + 1);
        if (o.cov && L) std::memcpy(o.cov, hCov.data() + po, sizeof(int) * L);
        if (o.plurality && L) std::memcpy(o.plurality, hPlur.data() + po, L);
        o.covSum = (long long)hCovSum[(size_t)z];
    }
    if (out)
        for (size_t k = 0; k < nr; ++k) {
            ZmwOut& o = out[where[k].first];
            const int at = where[k].second;
            if (o.nMatch) o.nMatch[at] = hColCounts[4 * k];
            if (o.nMismatch) o.nMismatch[at] = hColCounts[4 * k + 1];
            if (o.nIns) o.nIns[at] = hColCounts[4 * k + 2];
            if (o.nDel) o.nDel[at] = hColCounts[4 * k + 3];
        }
}

}  // namespace pileup
}  // namespace pbccs

// pbccs_amd/csrc/split_map_kernels.hip -- k_split_fill, k_split_chain and the engine's split-mapping workspace
// (split_map_kernels.hpp).
#include "split_map_kernels.hpp"

#include <algorithm>
#include <climits>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <string>

#include "../../include/pbccs_amd.h"

namespace pbccs {
namespace map {

namespace {

void check(hipError_t e, const char* what)
{
    if (e == hipSuccess) return;
    (void)hipGetLastError();
    throw DeviceError(std::string("split map: ") + what + ": " + hipGetErrorString(e));
}

// ConsensusCore Sequence.cpp:44-105 (ComplementArray; note N <-> M), as k_map_fill's complement()
__device__ __forceinline__ int complement(int c)
{
    switch (c) {
        case 'A': return 'T'; case 'C': return 'G'; case 'G': return 'C'; case 'T': return 'A';
        case 'a': return 't'; case 'c': return 'g'; case 'g': return 'c'; case 't': return 'a';
        case 'N': return 'M'; case 'M': return 'N'; case 'n': return 'm'; case 'm': return 'n';
        case '-': return '-';
        case 0: return 3; case 1: return 2; case 2: return 1; case 3: return 0;
    }
    return 127;
}

template <int CTRL, int ROWMASK>
__device__ __forceinline__ int dpp_i(int old, int x)
{
    return __builtin_amdgcn_update_dpp(old, x, CTRL, ROWMASK, 0xF, false);
}

// wave_shr:1 -- lane l receives lane l - 1's x; lane 0 (no source lane) keeps `first`
__device__ __forceinline__ int shr1(int first, int x) { return dpp_i<0x138, 0xF>(first, x); }

// A scan element is a cell's value before the Delete candidate, V(i, j), as a source of the Delete chain: the key
// is ((score + 4 j) << 1) | cls, so that keys of different columns compare as their scores would at any column to
// the right of both.  cls 1: V came from Start or the diagonal, which win a tie against Delete; cls 0: it came from
// Extra, which loses one.  Of two sources with equal keys the right one wins when cls is 1 (at its own cell it
// beat the chain from the left) and the left one when cls is 0.  -1 is the identity.
__device__ __forceinline__ bool right_wins(int kl, int kr) { return kr + (kr & 1) > kl; }

template <int CTRL, int ROWMASK>
__device__ __forceinline__ void scan_step(int& k, uint32_t& s)
{
    const int ik = dpp_i<CTRL, ROWMASK>(-1, k);
    const uint32_t is = (uint32_t)dpp_i<CTRL, ROWMASK>(0, (int)s);
    if (!right_wins(ik, k)) {
        k = ik;
        s = is;
    }
}

// inclusive scan over the 64 lanes, lane order = column order
__device__ __forceinline__ void wave_scan(int& k, uint32_t& s)
{
    scan_step<0x111, 0xF>(k, s);   // row_shr:1
    scan_step<0x112, 0xF>(k, s);   // row_shr:2
    scan_step<0x114, 0xF>(k, s);   // row_shr:4
    scan_step<0x118, 0xF>(k, s);   // row_shr:8
    scan_step<0x142, 0xA>(k, s);   // row_bcast:15 (rows 1, 3)
    scan_step<0x143, 0xC>(k, s);   // row_bcast:31 (rows 2, 3)
}

__device__ __forceinline__ int wave_max(int x)
{
    x = max(x, dpp_i<0x111, 0xF>(INT_MIN, x));
    x = max(x, dpp_i<0x112, 0xF>(INT_MIN, x));
    x = max(x, dpp_i<0x114, 0xF>(INT_MIN, x));
    x = max(x, dpp_i<0x118, 0xF>(INT_MIN, x));
    x = max(x, dpp_i<0x142, 0xA>(INT_MIN, x));
    x = max(x, dpp_i<0x143, 0xC>(INT_MIN, x));
    return __builtin_amdgcn_readlane(x, 63);
}

// One wavefront per read.  Cell (i, j) of orientation o, 1 <= i <= I, 1 <= j <= J, has consumed i read bases and j
// bases of the column sequence (the draft for o = 0, its reverse complement for o = 1); lane l owns columns
// (tile * 64 + l) * C + 1 .. + C of every tile.  Candidates in order, a later one winning only when strictly
// greater: Start (G(i - 1), the cell itself becomes the start cell), diagonal, Delete (left), Extra (up).
template <int C, bool TILED>
__global__ __launch_bounds__(64) void k_split_fill(const SplitJob* __restrict__ jobs, const int* __restrict__ list,
                                                   const uint8_t* __restrict__ seq, int P, unsigned long long* rowbuf,
                                                   SplitRow* __restrict__ rows, SplitHead* __restrict__ heads)
{
    const int lane = threadIdx.x;
    const int jobIdx = list[blockIdx.x];
    const SplitJob jb = jobs[jobIdx];
    const int I = jb.I, J = jb.J;
    const int nTiles = TILED ? jb.nTiles : 1;
    const uint8_t* tg = seq + jb.draftOff;
    const uint8_t* rd = seq + jb.readOff;
    SplitRow* rec = rows + jb.rowOff;
    // the lane's columns of the previous row, parked per tile and orientation: word ((o * nTiles + tile) * C + c) *
    // 64 + lane holds the score in the low half and the start cell in the high half; a lane reads only its own words
    unsigned long long* buf = rowbuf + (TILED ? jb.bufOff : 0) + lane;

    int ph[2][C];        // H(i - 1, j)
    uint32_t ps[2][C];   // its start cell (i0 << 16) | j0
    int tb[C];           // the column's base, forward in bits 0-7 and reverse complement in bits 8-15

    // row 0: H = 0, start cell (0, j)
    for (int tile = 0; tile < nTiles; ++tile) {
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const int j = (tile * 64 + lane) * C + c + 1;
            ph[0][c] = ph[1][c] = 0;
            ps[0][c] = ps[1][c] = (uint32_t)j;
            if (TILED) {
                buf[(size_t)((0 * nTiles + tile) * C + c) * 64] = (unsigned long long)(uint32_t)j << 32;
                buf[(size_t)((1 * nTiles + tile) * C + c) * 64] = (unsigned long long)(uint32_t)j << 32;
            } else {
                tb[c] = j <= J ? (int)tg[j - 1] | (complement((int)tg[J - j]) << 8) : 0;
            }
        }
    }
    if (lane == 0) rec[0] = SplitRow{0, 0, 0, 0u, 0u};

    int G1 = 0, G2 = 0, gRow = 0;   // G(i - 1), G(i - 2), the row where G last rose
    int endScore = 0, endRow = 0;
    for (int i = 1; i <= I; ++i) {
        const int rb = (int)rd[i - 1];
        int lbKey = -1, lbJ = 0;   // the lane's best cell of the row: key (score << 1) | (1 - o)
        uint32_t lbS = 0;
        int cK[2] = {-1, -1};      // the Delete chain's carry into the tile; column 0 never feeds it (Start is larger)
        uint32_t cS[2] = {0, 0};
        int dH[2];                 // H(i - 1, j) of the column left of the tile: column 0 holds G(i - 2), start (i - 1, 0)
        uint32_t dS[2];
        dH[0] = dH[1] = i == 1 ? 0 : G2;
        dS[0] = dS[1] = (uint32_t)(i - 1) << 16;
        for (int tile = 0; tile < nTiles; ++tile) {
            const int j0 = (tile * 64 + lane) * C;
            if (TILED) {
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    const int j = j0 + c + 1;
                    const unsigned long long w0 = buf[(size_t)((0 * nTiles + tile) * C + c) * 64];
                    const unsigned long long w1 = buf[(size_t)((1 * nTiles + tile) * C + c) * 64];
                    ph[0][c] = (int)(uint32_t)w0;
                    ps[0][c] = (uint32_t)(w0 >> 32);
                    ph[1][c] = (int)(uint32_t)w1;
                    ps[1][c] = (uint32_t)(w1 >> 32);
                    tb[c] = j <= J ? (int)tg[j - 1] | (complement((int)tg[J - j]) << 8) : 0;
                }
            }
#pragma unroll
            for (int o = 0; o < 2; ++o) {
                // the diagonal's source for the lane's first column is the left lane's last column
                int dh = shr1(dH[o], ph[o][C - 1]);
                uint32_t ds = (uint32_t)shr1((int)dS[o], (int)ps[o][C - 1]);
                dH[o] = __builtin_amdgcn_readlane(ph[o][C - 1], 63);
                dS[o] = (uint32_t)__builtin_amdgcn_readlane((int)ps[o][C - 1], 63);
                int vk[C];
                uint32_t vs[C];
                int aK = -1;   // the lane's block as one scan element
                uint32_t aS = 0;
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    const int j = j0 + c + 1;
                    const int base = (tb[c] >> (8 * o)) & 0xff;
                    int sc = G1;
                    uint32_t st = ((uint32_t)i << 16) | (uint32_t)j;
                    const int a = dh + (rb == base ? kMatch : kMismatch);
                    if (a > sc) {
                        sc = a;
                        st = ds;
                    }
                    dh = ph[o][c];
                    ds = ps[o][c];
                    int cls = 1;
                    const int u = dh + kInsert;
                    if (u > sc) {
                        sc = u;
                        st = ds;
                        cls = 0;
                    }
                    const int k = j <= J ? ((sc - kDelete * j) << 1) | cls : -1;
                    vk[c] = k;
                    vs[c] = st;
                    if (right_wins(aK, k)) {
                        aK = k;
                        aS = st;
                    }
                }
                wave_scan(aK, aS);
                int run = shr1(cK[o], aK);
                uint32_t runS = (uint32_t)shr1((int)cS[o], (int)aS);
                cK[o] = __builtin_amdgcn_readlane(aK, 63);
                cS[o] = (uint32_t)__builtin_amdgcn_readlane((int)aS, 63);
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    const int j = j0 + c + 1;
                    if (right_wins(run, vk[c])) {
                        run = vk[c];
                        runS = vs[c];
                    }
                    const int h = (run >> 1) + kDelete * j;
                    ph[o][c] = h;
                    ps[o][c] = runS;
                    const int key = (h << 1) | (1 - o);
                    if (j <= J && key > lbKey) {
                        lbKey = key;
                        lbJ = j;
                        lbS = runS;
                    }
                }
            }
            if (TILED) {
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    buf[(size_t)((0 * nTiles + tile) * C + c) * 64] =
                        ((unsigned long long)ps[0][c] << 32) | (uint32_t)ph[0][c];
                    buf[(size_t)((1 * nTiles + tile) * C + c) * 64] =
                        ((unsigned long long)ps[1][c] << 32) | (uint32_t)ph[1][c];
                }
            }
        }
        // R(i): the larger score, then o = 0, then the smaller column
        const int m = wave_max(lbKey);
        const int jm = -wave_max(lbKey == m ? -lbJ : INT_MIN);
        const unsigned long long who = __ballot(lbKey == m && lbJ == jm);
        const uint32_t start = (uint32_t)__shfl((int)lbS, __ffsll((long long)who) - 1, 64);
        const int score = m >> 1;
        int G = G1;
        if (score - P > G1) {
            G = score - P;
            gRow = i;
        }
        if (score > endScore) {
            endScore = score;
            endRow = i;
        }
        if (lane == 0) rec[i] = SplitRow{G, gRow, score, ((uint32_t)(1 - (m & 1)) << 31) | (uint32_t)jm, start};
        G2 = G1;
        G1 = G;
    }
    if (lane == 0) heads[jobIdx] = SplitHead{endRow, endScore};
}

// One lane per read: from the chain's end row back through the row records.  A segment that ends at R(r) with start
// cell (i0, j0) owns H - g, g = G(i0 - 1); g = 0 starts the chain, otherwise the predecessor ends at R(r') for the
// first row r' with G(r') = g.  The first maxSeg segments met (the chain's last ones) are kept, last one first.
__global__ __launch_bounds__(64) void k_split_chain(const SplitJob* __restrict__ jobs, const int* __restrict__ list,
                                                    int n, const SplitRow* __restrict__ rows,
                                                    const SplitHead* __restrict__ heads, int maxSeg,
                                                    SplitSeg* __restrict__ segs, SplitTail* __restrict__ tails)
{
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const int jobIdx = list[t];
    const SplitJob jb = jobs[jobIdx];
    const SplitRow* rec = rows + jb.rowOff;
    const SplitHead hd = heads[jobIdx];
    SplitSeg* out = segs + (size_t)jobIdx * maxSeg;
    int count = 0;
    int r = hd.endRow;
    while (hd.score > 0 && r >= 1) {
        const SplitRow e = rec[r];
        const int o = (int)(e.oj >> 31), j1 = (int)(e.oj & 0xffffu);
        const int i0 = (int)(e.start >> 16), j0 = (int)(e.start & 0xffffu);
        if (i0 > r) break;   // never: a start cell lies at or above its end row
        const int g = i0 > 0 ? rec[i0 - 1].G : 0;
        if (count < maxSeg) out[count] = SplitSeg{o, i0, r, o ? jb.J - j1 : j0, o ? jb.J - j0 : j1, e.score - g};
        ++count;
        if (g == 0) break;
        r = rec[i0 - 1].gRow;
    }
    tails[jobIdx] = SplitTail{count, hd.score};
}

template <int C>
void launch_fill_c(bool tiled, int grid, hipStream_t st, const SplitJob* jobs, const int* list, const uint8_t* seq, int P,
                   unsigned long long* buf, SplitRow* rows, SplitHead* heads)
{
    if (tiled)
        hipLaunchKernelGGL((k_split_fill<C, true>), dim3(grid), dim3(64), 0, st, jobs, list, seq, P, buf, rows, heads);
    else
        hipLaunchKernelGGL((k_split_fill<C, false>), dim3(grid), dim3(64), 0, st, jobs, list, seq, P, buf, rows, heads);
}

void launch_fill(int C, bool tiled, int grid, hipStream_t st, const SplitJob* jobs, const int* list, const uint8_t* seq,
                 int P, unsigned long long* buf, SplitRow* rows, SplitHead* heads)
{
    switch (C) {
        case 2: launch_fill_c<2>(tiled, grid, st, jobs, list, seq, P, buf, rows, heads); break;
        case 4: launch_fill_c<4>(tiled, grid, st, jobs, list, seq, P, buf, rows, heads); break;
        default: launch_fill_c<8>(tiled, grid, st, jobs, list, seq, P, buf, rows, heads); break;
    }
}

long long env_ll(const char* name, long long dflt)
{
    const char* v = std::getenv(name);
    if (!v || !*v) return dflt;
    return std::atoll(v);
}

// the variant of a draft of J columns: index into kSplitColsPerLane and whether the row-buffer path runs
void variant_of(int J, int* v, bool* tiled)
{
    const int forced = (int)env_ll("PBCCS_SPLIT_COLS_PER_LANE", 0);   // tests: every path with every C
    *v = -1;
    for (int k = 0; k < 3; ++k)
        if (forced == kSplitColsPerLane[k]) *v = k;
    if (*v < 0) {
        *v = 2;
        for (int k = 2; k >= 0; --k)
            if (J <= 64 * kSplitColsPerLane[k]) *v = k;
    }
    *tiled = env_ll("PBCCS_SPLIT_TILED", 0) != 0 || J > 64 * kSplitColsPerLane[*v];
}

}  // namespace

SplitMapRunner::SplitMapRunner(int device, hipStream_t stream) : device_(device), stream_(stream)
{
    check(hipSetDevice(device_), "hipSetDevice");
    for (auto& e : ev_) check(hipEventCreate(&e), "hipEventCreate");
}

SplitMapRunner::~SplitMapRunner()
{
    if (stream_) (void)hipStreamSynchronize(stream_);
    for (auto& e : ev_)
        if (e) (void)hipEventDestroy(e);
}

void SplitMapRunner::Run(const MapGroup* groups, int ng, int jumpPenalty, int maxSegments,
                         std::vector<SplitMapResult>* out)
{
    const long long budget = std::max(1LL, env_ll("PBCCS_SPLIT_WORKSPACE_KB", 262144)) * 1024;
    size_t total = 0;
    for (int g = 0; g < ng; ++g) total += (size_t)std::max(0, groups[g].n);
    out->assign(total, SplitMapResult());
    // host part: one job per read that reaches the device and the sequence pool (each draft and each read once)
    std::vector<SplitJob> jobs;
    std::vector<int> readOf, varOf;
    std::vector<long long> bytesOf, wordsOf;
    std::vector<const char*> readPtr, draftPtr;
    long long seqBytes = 0;
    size_t idx = 0;
    for (int g = 0; g < ng; ++g) {
        const MapGroup& G = groups[g];
        const long long draftOff = seqBytes;
        bool draftUsed = false;
        for (int r = 0; r < G.n; ++r, ++idx) {
            stats.jobs++;
            const int I = G.seqs[r] ? G.lens[r] : 0;
            if (I <= 0) continue;   // never mapped
            int v;
            bool tiled;
            variant_of(G.J, &v, &tiled);
            const int C = kSplitColsPerLane[v];
            const int nTiles = tiled ? (G.J + 64 * C - 1) / (64 * C) : 1;
            const long long words = tiled ? 2LL * nTiles * C * 64 : 0;
            const long long bytes = words * 8 + (I + 1LL) * (long long)sizeof(SplitRow);
            if (bytes > budget) {
                (*out)[idx].status = PBCCS_EOOM;
                continue;
            }
            if (!draftUsed) {
                seqBytes += G.J;
                draftUsed = true;
            }
            SplitJob jb;
            jb.readOff = seqBytes;
            jb.draftOff = draftOff;
            jb.rowOff = 0;
            jb.bufOff = -1;
            jb.I = I;
            jb.J = G.J;
            jb.nTiles = nTiles;
            jb.pad = 0;
            jobs.push_back(jb);
            readOf.push_back((int)idx);
            varOf.push_back(2 * v + (tiled ? 1 : 0));
            bytesOf.push_back(bytes);
            wordsOf.push_back(words);
            readPtr.push_back(G.seqs[r]);
            draftPtr.push_back(G.draft);
            seqBytes += I;
        }
    }
    const int nj = (int)jobs.size();
    if (nj == 0) return;

    std::vector<uint8_t> seq((size_t)seqBytes);
    for (int k = 0; k < nj; ++k) {
        std::memcpy(seq.data() + jobs[k].draftOff, draftPtr[k], (size_t)jobs[k].J);
        std::memcpy(seq.data() + jobs[k].readOff, readPtr[k], (size_t)jobs[k].I);
    }

    std::vector<int> order(nj);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) {
        return (long long)jobs[a].I * jobs[a].J > (long long)jobs[b].I * jobs[b].J;
    });
    // launch groups over the sorted list: each group's row records and row buffers fit the budget
    struct Group {
        int begin, end;
        long long bytes, rows, words;
    };
    std::vector<Group> lg;
    {
        Group g{0, 0, 0, 0, 0};
        for (int k = 0; k < nj; ++k) {
            SplitJob& jb = jobs[order[k]];
            if (g.end > g.begin && g.bytes + bytesOf[order[k]] > budget) {
                lg.push_back(g);
                g = Group{k, k, 0, 0, 0};
            }
            jb.rowOff = g.rows;
            if (wordsOf[order[k]]) jb.bufOff = g.words;
            g.rows += jb.I + 1LL;
            g.words += wordsOf[order[k]];
            g.bytes += bytesOf[order[k]];
            g.end = k + 1;
        }
        lg.push_back(g);
    }
    long long maxRows = 1, maxWords = 1;
    for (const Group& g : lg) {
        maxRows = std::max(maxRows, g.rows);
        maxWords = std::max(maxWords, g.words);
    }
    // per launch group: the whole group's list (k_split_chain), then one list per variant
    std::vector<int> lists;
    struct GroupLists {
        int all, off[6], n[6];
    };
    std::vector<GroupLists> gl(lg.size());
    for (size_t q = 0; q < lg.size(); ++q) {
        gl[q].all = (int)lists.size();
        for (int k = lg[q].begin; k < lg[q].end; ++k) lists.push_back(order[k]);
        for (int v = 0; v < 6; ++v) {
            gl[q].off[v] = (int)lists.size();
            for (int k = lg[q].begin; k < lg[q].end; ++k)
                if (varOf[order[k]] == v) lists.push_back(order[k]);
            gl[q].n[v] = (int)lists.size() - gl[q].off[v];
        }
    }

    std::vector<SplitSeg> hSegs((size_t)nj * maxSegments);
    std::vector<SplitTail> hTails((size_t)nj);
    check(hipSetDevice(device_), "hipSetDevice");
    StreamScope scope(stream_);
    // leaves (also by exception) only once the stream is idle: queued copies read and write the vectors above
    struct StreamIdle {
        hipStream_t s;
        ~StreamIdle() { (void)hipStreamSynchronize(s); }
    } idle{stream_};
    dSeq_.reserve((size_t)seqBytes, false);
    dJobs_.reserve((size_t)nj, false);
    dList_.reserve(lists.size(), false);
    dBuf_.reserve((size_t)maxWords, false);
    dRows_.reserve((size_t)maxRows, false);
    dHeads_.reserve((size_t)nj, false);
    dSegs_.reserve(hSegs.size(), false);
    dTails_.reserve((size_t)nj, false);
    check(hipMemcpyAsync(dSeq_.ptr, seq.data(), (size_t)seqBytes, hipMemcpyHostToDevice, stream_), "upload");
    check(hipMemcpyAsync(dJobs_.ptr, jobs.data(), sizeof(SplitJob) * nj, hipMemcpyHostToDevice, stream_), "upload");
    check(hipMemcpyAsync(dList_.ptr, lists.data(), sizeof(int) * lists.size(), hipMemcpyHostToDevice, stream_),
          "upload");
    if (profiling) check(hipEventRecord(ev_[0], stream_), "event");
    for (size_t q = 0; q < lg.size(); ++q) {
        for (int v = 0; v < 6; ++v) {
            if (gl[q].n[v] == 0) continue;
            launch_fill(kSplitColsPerLane[v / 2], (v & 1) != 0, gl[q].n[v], stream_, dJobs_.ptr,
                        dList_.ptr + gl[q].off[v], dSeq_.ptr, jumpPenalty, dBuf_.ptr, dRows_.ptr, dHeads_.ptr);
            check(hipGetLastError(), "k_split_fill launch");
            stats.launches++;
        }
        const int n = lg[q].end - lg[q].begin;
        hipLaunchKernelGGL(k_split_chain, dim3((n + 63) / 64), dim3(64), 0, stream_, dJobs_.ptr, dList_.ptr + gl[q].all,
                           n, dRows_.ptr, dHeads_.ptr, maxSegments, dSegs_.ptr, dTails_.ptr);
        check(hipGetLastError(), "k_split_chain launch");
        stats.launches++;
    }
    if (profiling) check(hipEventRecord(ev_[1], stream_), "event");
    check(hipMemcpyAsync(hSegs.data(), dSegs_.ptr, sizeof(SplitSeg) * hSegs.size(), hipMemcpyDeviceToHost, stream_),
          "download");
    check(hipMemcpyAsync(hTails.data(), dTails_.ptr, sizeof(SplitTail) * nj, hipMemcpyDeviceToHost, stream_),
          "download");
    check(hipStreamSynchronize(stream_), "sync");
    if (profiling) {
        float ms = 0.f;
        check(hipEventElapsedTime(&ms, ev_[0], ev_[1]), "event");
        stats.deviceMs += ms;
    }
    // the stream is idle: buffers that growth retired can go
    dSeq_.trim();
    dJobs_.trim();
    dList_.trim();
    dBuf_.trim();
    dRows_.trim();
    dHeads_.trim();
    dSegs_.trim();
    dTails_.trim();

    for (int k = 0; k < nj; ++k) {
        SplitMapResult& o = (*out)[readOf[k]];
        stats.cells += 2LL * jobs[k].I * jobs[k].J;
        stats.tiled += varOf[k] & 1;
        o.count = hTails[k].count;
        o.score = hTails[k].score;
        o.truncated = o.count > maxSegments;
        const int kept = std::min(o.count, maxSegments);
        o.segs.assign(hSegs.begin() + (size_t)k * maxSegments, hSegs.begin() + (size_t)k * maxSegments + kept);
        std::reverse(o.segs.begin(), o.segs.end());
    }
}

}  // namespace map
}  // namespace pbccs

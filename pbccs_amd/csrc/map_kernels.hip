// pbccs_amd/csrc/map_kernels.hip -- k_map_fill and the engine's mapping workspace (map_kernels.hpp,
// DESIGN.md §3.15).
#include "map_kernels.hpp"

#include <algorithm>
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
    throw DeviceError(std::string("map: ") + what + ": " + hipGetErrorString(e));
}

// ConsensusCore Sequence.cpp:44-105 (ComplementArray; note N <-> M), as poa_engine.hip's complement()
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

// wave_shr:1 -- lane l receives lane l - 1's x; lane 0 (no source lane) keeps `first`
__device__ __forceinline__ int shr1(int first, int x)
{
    return __builtin_amdgcn_update_dpp(first, x, 0x138, 0xF, 0xF, false);
}

// The strip boundary is written by lane 63 of one strip and read by the lanes of the next strip of the same
// wavefront: agent-scope relaxed accesses keep both off the CU's L1, whose lines may still hold the previous
// strip's values (as k_align_fill's carry).  One word per column: score in the low half, start cell in the high.
__device__ __forceinline__ void carry_store(unsigned long long* p, int score, uint32_t start)
{
    __hip_atomic_store(p, ((unsigned long long)start << 32) | (uint32_t)score, __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ unsigned long long carry_load(unsigned long long* p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// (score, j, i) a is a better end cell than b: the larger score, then the smaller column, then the smaller row
// (makeAlignmentColumnForExit: columns in order, strict '>', ArgMax = first maximal row)
__device__ __forceinline__ bool better(int sa, int ja, int ia, int sb, int jb, int ib)
{
    return sa > sb || (sa == sb && (ja < jb || (ja == jb && ia < ib)));
}

// One wavefront per job.  Cell (i, j), 1 <= i <= I, 1 <= j <= J, has consumed i read bases and j draft bases: row
// i - 1 = (strip * 64 + lane) * R + r, computed at step t = (j - 1) + lane of its strip.  Candidates in the
// reference's order, a later one winning only when strictly greater: Start (0, the cell itself becomes the start
// cell), diagonal, Delete (left), Extra (up).  Row 0 and column 0 are Start cells of score 0.
template <int R>
__global__ __launch_bounds__(64) void k_map_fill(const MapJob* __restrict__ jobs, const int* __restrict__ list,
                                                 const uint8_t* __restrict__ seq, unsigned long long* carry,
                                                 MapCell* __restrict__ out)
{
    const int lane = threadIdx.x;
    const int jobIdx = list[blockIdx.x];
    const MapJob jb = jobs[jobIdx];
    const int I = jb.I, J = jb.J, T = J + 63;
    const uint8_t* tg = seq + jb.draftOff;
    const uint8_t* rd = seq + jb.readOff;
    unsigned long long* cr = carry + (jb.carryOff >= 0 ? jb.carryOff : 0);
    int best = 0, bestI = 0, bestJ = 0;
    uint32_t bestS = 0;

    for (int s = 0; s < jb.nStrips; ++s) {
        const int row0 = (s * 64 + lane) * R;   // matrix row above the lane's first row
        const bool rows = row0 < I;
        const bool carryOut = lane == 63 && s + 1 < jb.nStrips;
        int left[R], qc[R];
        uint32_t lst[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int i = row0 + r + 1;
            int c = -1;   // a row past the read matches nothing, so it never beats the cell it descends from
            if (i <= I) c = jb.rc ? complement((int)rd[I - i]) : (int)rd[i - 1];
            qc[r] = c;
            left[r] = 0;
            lst[r] = (uint32_t)i << 16;
        }
        int diag = 0, bot = 0, tc = 0;
        uint32_t dgs = (uint32_t)row0 << 16, bts = lst[R - 1];
        int lb = 0, lbJ = 0, lbR = 0;   // the strip's best cell of this lane: first in (j, i) order by strict '>'
        uint32_t lbS = 0;
        // 64 steps' inputs of lane 0 are loaded one block ahead, one per lane: the draft bases, and for a later strip
        // the row above it
        int tgN = lane < J ? (int)tg[lane] : 0;
        unsigned long long cN = 0;
        if (s > 0 && lane + 1 <= J) cN = carry_load(cr + lane + 1);
        for (int t0 = 0; t0 < T; t0 += 64) {
            const int tgC = tgN;
            const int cLo = (int)(uint32_t)cN, cHi = (int)(uint32_t)(cN >> 32);
            {
                const int n0 = t0 + 64 + lane;
                tgN = n0 < J ? (int)tg[n0] : 0;
                cN = 0;
                if (s > 0 && n0 + 1 <= J) cN = carry_load(cr + n0 + 1);
            }
            const int kEnd = min(64, T - t0);
#pragma nounroll
            for (int k = 0; k < kEnd; ++k) {
                const int t = t0 + k;
                const int j = t - lane + 1;
                // lane 0: draft base t and the cell above the strip in column t + 1
                int cinS = 0, cinP = t + 1;   // row 0: a Start cell (0, j)
                if (s > 0) {
                    cinS = __builtin_amdgcn_readlane(cLo, k);
                    cinP = __builtin_amdgcn_readlane(cHi, k);
                }
                tc = shr1(__builtin_amdgcn_readlane(tgC, k), tc);
                const int up = shr1(cinS, bot);
                const uint32_t ups = (uint32_t)shr1(cinP, (int)bts);
                if (rows && j >= 1 && j <= J) {
                    int d = diag, u = up;
                    uint32_t ds = dgs, us = ups;
                    const uint32_t here = ((uint32_t)(row0 + 1) << 16) | (uint32_t)j;
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        int sc = 0;
                        uint32_t st = here + ((uint32_t)r << 16);
                        const int a = d + (qc[r] == tc ? kMatch : kMismatch);
                        if (a > sc) {
                            sc = a;
                            st = ds;
                        }
                        const int c = left[r] + kDelete;
                        if (c > sc) {
                            sc = c;
                            st = lst[r];
                        }
                        const int b = u + kInsert;
                        if (b > sc) {
                            sc = b;
                            st = us;
                        }
                        d = left[r];
                        ds = lst[r];
                        u = sc;
                        us = st;
                        left[r] = sc;
                        lst[r] = st;
                        if (sc > lb) {
                            lb = sc;
                            lbJ = j;
                            lbR = r;
                            lbS = st;
                        }
                    }
                    bot = left[R - 1];
                    bts = lst[R - 1];
                    diag = up;
                    dgs = ups;
                    if (carryOut) carry_store(cr + j, bot, bts);
                }
            }
        }
        const int lbI = row0 + lbR + 1;
        if (better(lb, lbJ, lbI, best, bestJ, bestI)) {
            best = lb;
            bestJ = lbJ;
            bestI = lbI;
            bestS = lbS;
        }
        // the next strip's lanes read what this strip's lane 63 stored
        if (s + 1 < jb.nStrips) __threadfence();
    }
    // nothing positive anywhere: every lane still holds (0, 0, 0), the ^ column's row 0
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const int os = __shfl_xor(best, off, 64), oj = __shfl_xor(bestJ, off, 64), oi = __shfl_xor(bestI, off, 64);
        const uint32_t ost = (uint32_t)__shfl_xor((int)bestS, off, 64);
        if (better(os, oj, oi, best, bestJ, bestI)) {
            best = os;
            bestJ = oj;
            bestI = oi;
            bestS = ost;
        }
    }
    if (lane == 0) out[jobIdx] = MapCell{best, bestI, bestJ, bestS};
}

void launch_fill(int R, int grid, hipStream_t st, const MapJob* jobs, const int* list, const uint8_t* seq,
                 unsigned long long* carry, MapCell* out)
{
    switch (R) {
        case 4:
            hipLaunchKernelGGL((k_map_fill<4>), dim3(grid), dim3(64), 0, st, jobs, list, seq, carry, out);
            break;
        case 8:
            hipLaunchKernelGGL((k_map_fill<8>), dim3(grid), dim3(64), 0, st, jobs, list, seq, carry, out);
            break;
        default:
            hipLaunchKernelGGL((k_map_fill<16>), dim3(grid), dim3(64), 0, st, jobs, list, seq, carry, out);
            break;
    }
}

long long env_ll(const char* name, long long dflt)
{
    const char* v = std::getenv(name);
    if (!v || !*v) return dflt;
    return std::atoll(v);
}

int rows_per_lane(int I)
{
    const int forced = (int)env_ll("PBCCS_MAP_ROWS_PER_LANE", 0);   // tests: every strip path with every R
    for (int R : kRowsPerLane)
        if (forced == R) return R;
    for (int R : kRowsPerLane)
        if (I <= 64 * R) return R;
    return kRowsPerLane[2];
}

}  // namespace

MapRunner::MapRunner(int device) : device_(device)
{
    check(hipSetDevice(device_), "hipSetDevice");
    check(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking), "hipStreamCreate");
    for (auto& e : ev_) check(hipEventCreate(&e), "hipEventCreate");
}

MapRunner::~MapRunner()
{
    if (stream_) {
        (void)hipStreamSynchronize(stream_);
        (void)hipStreamDestroy(stream_);
    }
    for (auto& e : ev_)
        if (e) (void)hipEventDestroy(e);
}

void MapRunner::Run(const MapGroup* groups, int ng, float minScoreToAdd, std::vector<MapResult>* out)
{
    const long long budgetWords = std::max(1LL, env_ll("PBCCS_MAP_WORKSPACE_KB", 262144)) * 1024 / 8;
    size_t total = 0;
    for (int g = 0; g < ng; ++g) total += (size_t)std::max(0, groups[g].n);
    out->assign(total, MapResult());
    // host part: the work list (two jobs per read that reaches the device) and the sequence pool (each draft and
    // each read once)
    std::vector<MapJob> jobs;
    std::vector<int> readOf, Rof;
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
            const int R = rows_per_lane(I);
            const int nStrips = (I + 64 * R - 1) / (64 * R);
            if (nStrips > 1 && 2 * (G.J + 1LL) > budgetWords) {
                (*out)[idx].status = PBCCS_EOOM;
                continue;
            }
            if (!draftUsed) {
                seqBytes += G.J;
                draftUsed = true;
            }
            for (int o = 0; o < 2; ++o) {
                MapJob jb;
                jb.readOff = seqBytes;
                jb.draftOff = draftOff;
                jb.carryOff = -1;
                jb.I = I;
                jb.J = G.J;
                jb.rc = o;
                jb.nStrips = nStrips;
                jobs.push_back(jb);
                readOf.push_back((int)idx);
                Rof.push_back(R);
            }
            seqBytes += I;
        }
    }
    const int nj = (int)jobs.size();
    if (nj == 0) return;

    std::vector<uint8_t> seq((size_t)seqBytes);
    {
        size_t k = 0, ri = 0;
        for (int g = 0; g < ng; ++g) {
            const MapGroup& G = groups[g];
            bool draftDone = false;
            for (int r = 0; r < G.n; ++r, ++ri) {
                if (k >= (size_t)nj || readOf[k] != (int)ri) continue;
                if (!draftDone) {
                    std::memcpy(seq.data() + jobs[k].draftOff, G.draft, (size_t)G.J);
                    draftDone = true;
                }
                std::memcpy(seq.data() + jobs[k].readOff, G.seqs[r], (size_t)jobs[k].I);
                k += 2;
            }
        }
    }

    std::vector<int> order(nj);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) {
        return (long long)jobs[a].I * jobs[a].J > (long long)jobs[b].I * jobs[b].J;
    });
    // launch groups over the sorted list: each group's boundary buffers fit the budget
    struct Group {
        int begin, end;
        long long words;
    };
    std::vector<Group> lg;
    {
        Group g{0, 0, 0};
        for (int k = 0; k < nj; ++k) {
            MapJob& jb = jobs[order[k]];
            const long long w = jb.nStrips > 1 ? jb.J + 1LL : 0;
            if (g.end > g.begin && g.words + w > budgetWords) {
                lg.push_back(g);
                g = Group{k, k, 0};
            }
            if (w) jb.carryOff = g.words;
            g.words += w;
            g.end = k + 1;
        }
        lg.push_back(g);
    }
    long long maxWords = 1;
    for (const Group& g : lg) maxWords = std::max(maxWords, g.words);
    // per launch group: one list per R
    std::vector<int> lists;
    struct GroupLists {
        int off[3], n[3];
    };
    std::vector<GroupLists> gl(lg.size());
    for (size_t q = 0; q < lg.size(); ++q)
        for (int v = 0; v < 3; ++v) {
            gl[q].off[v] = (int)lists.size();
            for (int k = lg[q].begin; k < lg[q].end; ++k)
                if (Rof[order[k]] == kRowsPerLane[v]) lists.push_back(order[k]);
            gl[q].n[v] = (int)lists.size() - gl[q].off[v];
        }

    std::vector<MapCell> hOut((size_t)nj);
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
    dCarry_.reserve((size_t)maxWords, false);
    dOut_.reserve((size_t)nj, false);
    check(hipMemcpyAsync(dSeq_.ptr, seq.data(), (size_t)seqBytes, hipMemcpyHostToDevice, stream_), "upload");
    check(hipMemcpyAsync(dJobs_.ptr, jobs.data(), sizeof(MapJob) * nj, hipMemcpyHostToDevice, stream_), "upload");
    check(hipMemcpyAsync(dList_.ptr, lists.data(), sizeof(int) * lists.size(), hipMemcpyHostToDevice, stream_),
          "upload");
    if (profiling) check(hipEventRecord(ev_[0], stream_), "event");
    for (size_t q = 0; q < lg.size(); ++q)
        for (int v = 0; v < 3; ++v) {
            if (gl[q].n[v] == 0) continue;
            launch_fill(kRowsPerLane[v], gl[q].n[v], stream_, dJobs_.ptr, dList_.ptr + gl[q].off[v], dSeq_.ptr,
                        dCarry_.ptr, dOut_.ptr);
            check(hipGetLastError(), "k_map_fill launch");
            stats.launches++;
        }
    if (profiling) check(hipEventRecord(ev_[1], stream_), "event");
    check(hipMemcpyAsync(hOut.data(), dOut_.ptr, sizeof(MapCell) * nj, hipMemcpyDeviceToHost, stream_), "download");
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
    dCarry_.trim();
    dOut_.trim();

    // SparsePoa's choice (src/SparsePoa.cpp:112-132), scores compared as floats like the reference's
    for (int k = 0; k < nj; k += 2) {
        MapResult& o = (*out)[readOf[k]];
        const MapJob& jb = jobs[k];
        stats.cells += 2LL * (jb.I + 1) * jb.J;
        stats.strips += 2LL * jb.nStrips;
        const float c1 = (float)hOut[k].score, c2 = (float)hOut[k + 1].score;
        int chosen = -1;
        if (c1 >= c2 && c1 >= minScoreToAdd) chosen = 0;
        else if (c2 >= c1 && c2 >= minScoreToAdd) chosen = 1;
        o.score = std::max(hOut[k].score, hOut[k + 1].score);
        if (chosen < 0) continue;
        const MapCell& c = hOut[k + chosen];
        o.mapped = 1;
        o.rc = chosen;
        o.ext[0] = (int)(c.start >> 16);
        o.ext[1] = c.endI;
        o.ext[2] = (int)(c.start & 0xffffu);
        o.ext[3] = c.endJ;
    }
}

}  // namespace map
}  // namespace pbccs

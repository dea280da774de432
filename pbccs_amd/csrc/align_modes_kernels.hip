// pbccs_amd/csrc/align_modes_kernels.hip -- k_align_fill_ends / k_align_trace_ends and AlignRunner::RunEnds: the
// ends-free modes (SEMIGLOBAL, LOCAL) of the int32 pairwise aligner (align_kernels.hpp).
// The geometry, the move store and the strip carry are k_align_fill's (§3.14); the cell rule, the tie order and
// the end cell are the reference POA's on a graph that holds the target as one unbranched path (§3.15).
#include "align_kernels.hpp"

#include <algorithm>
#include <climits>
#include <cstdlib>
#include <cstring>
#include <numeric>

#include "../../include/pbccs_amd.h"

namespace pbccs {
namespace align {

namespace {

void check(hipError_t e, const char* what)
{
    if (e == hipSuccess) return;
    (void)hipGetLastError();
    throw DeviceError(std::string("align: ") + what + ": " + hipGetErrorString(e));
}

// the strip carry, as k_align_fill's: agent-scope relaxed accesses keep it off the CU's L1
__device__ __forceinline__ void carry_store(uint32_t* p, uint32_t v)
{
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ uint32_t carry_load(uint32_t* p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// (score, j, i) a is a better end cell than b: the larger score, then the smaller column, then the smaller row
// (makeAlignmentColumnForExit: columns in order, strict '>', ArgMax = first maximal row), as k_map_fill's
__device__ __forceinline__ bool better(int sa, int ja, int ia, int sb, int jb, int ib)
{
    return sa > sb || (sa == sb && (ja < jb || (ja == jb && ia < ib)));
}

// One wavefront per job, k_align_fill's layout: cell (i, j), 1 <= i <= I, 1 <= j <= J, is row
// i - 1 = (strip * 64 + lane) * R + r, computed at step t = (j - 1) + lane of its strip; its move byte lands at
// ((strip * (J + 63) + t) * 64 + lane) * R + r.  Candidates in the POA's order, a later one winning only when
// strictly greater: (LOCAL) Start 0, diagonal, Delete (left), Extra (up).  Row 0 is Start cells of score 0; column
// 0 is i * Insert reached by Extra (SEMIGLOBAL) or Start cells of score 0 (LOCAL).  The carry holds one word per
// column.  ends[8 * job + 0..2] receives the end cell: score, i, j.
template <int MODE, int R>
__global__ __launch_bounds__(64) void k_align_fill_ends(const AlignJob* __restrict__ jobs,
                                                        const int* __restrict__ list,
                                                        const uint8_t* __restrict__ seq, uint8_t* __restrict__ store,
                                                        uint32_t* carry, int* __restrict__ ends, AlignScoring p)
{
    constexpr bool LOCAL = MODE == kEndsLocal;
    const int lane = threadIdx.x;
    const int jobIdx = list[blockIdx.x];
    const AlignJob jb = jobs[jobIdx];
    const int I = jb.I, J = jb.J, T = J + 63;
    const uint8_t* tg = seq + jb.seqOff;
    const uint8_t* qr = tg + J;
    uint32_t* cr = carry + (jb.carryOff >= 0 ? jb.carryOff : 0);
    uint8_t* st = store + jb.storeOff;
    const int edge = LOCAL ? 0 : p.insert;   // column 0: S(i, 0) = i * edge

    // LOCAL: every lane starts at the (0, 0) Start cell.  SEMIGLOBAL: only the lane that owns row I holds a
    // candidate, starting at (I, 0).
    int best = 0, bestI = 0, bestJ = 0;
    if constexpr (!LOCAL) {
        const int rowI = (I - 1) - (jb.nStrips - 1) * 64 * R;
        const bool own = rowI / R == lane;
        best = own ? I * p.insert : INT_MIN;
        bestI = I;
    }

    for (int s = 0; s < jb.nStrips; ++s) {
        const int row0 = (s * 64 + lane) * R;   // matrix row above the lane's first row
        const bool rows = row0 < I;
        const bool carryOut = lane == 63 && s + 1 < jb.nStrips;
        // the rows of this lane that may hold the end cell: LOCAL every real row, SEMIGLOBAL row I alone.  A
        // padded row past I never does.
        const int trkLo = LOCAL ? 0 : I - 1 - row0;
        const int trkHi = I - row0;   // r in [trkLo, trkHi)
        int left[R], qc[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int i = row0 + r + 1;
            qc[r] = i <= I ? (int)qr[i - 1] : -1;   // a padded row matches nothing
            left[r] = min(i, I) * edge;
        }
        int diag = min(row0, I) * edge;
        int bot = left[R - 1];
        int lb = LOCAL ? 0 : INT_MIN, lbJ = 0, lbR = 0;   // the strip's best cell of this lane, first in (j, i) order
        // the next step's inputs are loaded one step ahead: the target byte, and for lane 0 the row above the strip
        int tcN = 0, cin = 0;
        {
            const int j1 = 1 - lane;
            if (j1 >= 1 && j1 <= J) tcN = tg[j1 - 1];
            if (lane == 0 && s > 0) cin = (int)carry_load(cr + 1);
        }
        for (int t = 0; t < T; ++t) {
            const int j = t - lane + 1;
            const int tc = tcN;
            int up = __shfl_up(bot, 1, 64);
            if (lane == 0) up = cin;
            {
                const int j2 = j + 1;
                tcN = (j2 >= 1 && j2 <= J) ? (int)tg[j2 - 1] : 0;
                if (lane == 0 && j2 <= J && s > 0) cin = (int)carry_load(cr + j2);
            }
            if (rows && j >= 1 && j <= J) {
                int d = diag, u = up;
                uint32_t pack[(R + 3) / 4] = {};
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    int sc;
                    uint32_t mv;
                    const int a = d + (qc[r] == tc ? p.match : p.mismatch);
                    if constexpr (LOCAL) {
                        sc = 0;
                        mv = kMoveStart;
                        if (a > sc) {
                            sc = a;
                            mv = kMoveDiag;
                        }
                    } else {
                        sc = a;
                        mv = kMoveDiag;
                    }
                    const int c = left[r] + p.delete_;
                    if (c > sc) {
                        sc = c;
                        mv = kMoveDelete;
                    }
                    const int b = u + p.insert;
                    if (b > sc) {
                        sc = b;
                        mv = kMoveExtra;
                    }
                    d = left[r];
                    u = sc;
                    left[r] = sc;
                    pack[r / 4] |= mv << (8 * (r % 4));
                    if (r >= trkLo && r < trkHi && sc > lb) {
                        lb = sc;
                        lbJ = j;
                        lbR = r;
                    }
                }
                bot = left[R - 1];
                diag = up;
                uint8_t* dst = st + (((long long)s * T + t) * 64 + lane) * R;
                if constexpr (R == 2) *reinterpret_cast<uint16_t*>(dst) = (uint16_t)pack[0];
                else if constexpr (R == 4) *reinterpret_cast<uint32_t*>(dst) = pack[0];
                else *reinterpret_cast<uint2*>(dst) = make_uint2(pack[0], pack[1]);
                if (carryOut) carry_store(cr + j, (uint32_t)bot);
            }
        }
        const int lbI = row0 + lbR + 1;
        if (better(lb, lbJ, lbI, best, bestJ, bestI)) {
            best = lb;
            bestJ = lbJ;
            bestI = lbI;
        }
        // the next strip's lane 0 reads what this strip's lane 63 stored
        if (s + 1 < jb.nStrips) __threadfence();
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const int os = __shfl_xor(best, off, 64), oj = __shfl_xor(bestJ, off, 64), oi = __shfl_xor(bestI, off, 64);
        if (better(os, oj, oi, best, bestJ, bestI)) {
            best = os;
            bestJ = oj;
            bestI = oi;
        }
    }
    if (lane == 0) {
        int* e = ends + 8 * (long long)jobIdx;
        e[0] = best;
        e[1] = bestI;
        e[2] = bestJ;
    }
}

__device__ __forceinline__ int move_byte(const uint8_t* st, int i, int j, int R, int T)
{
    const int row = i - 1;
    const int strip = row / (64 * R);
    const int rem = row - strip * 64 * R;
    const int l = rem / R, r = rem - l * R;
    const int t = (j - 1) + l;
    return st[(((long long)strip * T + t) * 64 + l) * R + r];
}

// One thread per job: the walk from the end cell back to the first Start cell, one dependent byte load per step.
// Border cells have no byte: row 0 is Start; column 0 is Extra (SEMIGLOBAL) or Start (LOCAL).  Writes the
// transcript reversed (M R I D) and ends[8 * job + 3..5]: the Start cell (i0, j0) and the length.
__global__ __launch_bounds__(64) void k_align_trace_ends(const AlignJob* __restrict__ jobs,
                                                         const int* __restrict__ list, int n,
                                                         const uint8_t* __restrict__ seq,
                                                         const uint8_t* __restrict__ store, uint8_t* __restrict__ out,
                                                         int* __restrict__ ends, int mode)
{
    const int idx = blockIdx.x * 64 + threadIdx.x;
    if (idx >= n) return;
    const int jobIdx = list[idx];
    const AlignJob jb = jobs[jobIdx];
    const int I = jb.I, J = jb.J, R = jb.R, T = J + 63;
    const uint8_t* tg = seq + jb.seqOff;
    const uint8_t* qr = tg + J;
    const uint8_t* st = store + jb.storeOff;
    uint8_t* o = out + jb.outOff;
    int* e = ends + 8 * (long long)jobIdx;
    int i = min(max(e[1], 0), I), j = min(max(e[2], 0), J), len = 0;
    const int cap = I + J;
    while (i > 0 && len < cap) {
        int mv;
        if (j == 0) {
            if (mode == kEndsLocal) break;
            mv = kMoveExtra;
        } else {
            mv = move_byte(st, i, j, R, T);
        }
        if (mv == kMoveStart) break;
        if (mv == kMoveDiag) {
            o[len++] = qr[i - 1] == tg[j - 1] ? 'M' : 'R';
            --i;
            --j;
        } else if (mv == kMoveDelete) {
            o[len++] = 'D';
            --j;
        } else {
            o[len++] = 'I';
            --i;
        }
    }
    e[3] = i;
    e[4] = j;
    e[5] = len;
}

template <int MODE>
void launch_fill_ends(int R, int grid, hipStream_t st, const AlignJob* jobs, const int* list, const uint8_t* seq,
                      uint8_t* store, uint32_t* carry, int* ends, const AlignScoring& p)
{
    switch (R) {
        case 2:
            hipLaunchKernelGGL((k_align_fill_ends<MODE, 2>), dim3(grid), dim3(64), 0, st, jobs, list, seq, store,
                               carry, ends, p);
            break;
        case 4:
            hipLaunchKernelGGL((k_align_fill_ends<MODE, 4>), dim3(grid), dim3(64), 0, st, jobs, list, seq, store,
                               carry, ends, p);
            break;
        default:
            hipLaunchKernelGGL((k_align_fill_ends<MODE, 8>), dim3(grid), dim3(64), 0, st, jobs, list, seq, store,
                               carry, ends, p);
            break;
    }
}

long long env_ll(const char* name, long long dflt)
{
    const char* v = std::getenv(name);
    if (!v || !*v) return dflt;
    return std::atoll(v);
}

int rows_per_lane(int I)   // Run's choice
{
    const int forced = (int)env_ll("PBCCS_ALIGN_ROWS_PER_LANE", 0);
    for (int R : kRowsPerLane)
        if (forced == R) return R;
    for (int R : kRowsPerLane)
        if (I <= 64 * R) return R;
    return kRowsPerLane[2];
}

// ConsensusCore Sequence.cpp:44-105 (ComplementArray; note N <-> M), as map_kernels.hip's complement()
int complement(int c)
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

}  // namespace

// Run's host part (the sort by cells, the R choice, the launch groups under the budget) around the two kernels
// above.  With bothStrands every pair that reaches the device is two jobs: the query as given and its reverse
// complement (formed here, on the host); forward wins iff its score >= the other's (SparsePoa.cpp:112-132).
void AlignRunner::RunEnds(const AlignScoring& p, int mode, bool bothStrands, const PairView* pairs, int n,
                          PairResult* out, EndsExtent* ext)
{
    const long long budget = std::max(1LL, env_ll("PBCCS_ALIGN_WORKSPACE_MB", 2048)) << 20;
    const int per = bothStrands ? 2 : 1;
    std::vector<AlignJob> jobs;
    std::vector<int> pairOf;
    std::vector<std::string> rcq;   // by job: the reverse complement of an odd job's query
    long long seqBytes = 0, outBytes = 0, carryWords = 0;
    for (int k = 0; k < n; ++k) {
        const int I = pairs[k].I, J = pairs[k].J;
        PairResult& o = out[k];
        o = PairResult();
        ext[k] = EndsExtent();
        if (I == 0) continue;   // score 0, empty transcript, all extents 0
        if (J == 0) {           // SEMIGLOBAL: all I; LOCAL: empty
            if (mode == kEndsSemiglobal) {
                o.transcript.assign((size_t)I, 'I');
                o.scoreI = I * p.insert;
                ext[k].queryEnd = I;
            }
            continue;
        }
        const long long mx = std::max(std::max(std::llabs((long long)p.match), std::llabs((long long)p.mismatch)),
                                      std::max(std::llabs((long long)p.insert), std::llabs((long long)p.delete_)));
        if (((long long)I + J) * mx > 0x7fffffffLL) {
            o.status = PBCCS_EINVAL;
            continue;
        }
        const int R = rows_per_lane(I);
        if (store_bytes(I, J, R) > budget) {
            o.status = PBCCS_EOOM;
            continue;
        }
        for (int v = 0; v < per; ++v) {
            AlignJob jb;
            jb.I = I;
            jb.J = J;
            jb.R = R;
            jb.nStrips = (I + 64 * R - 1) / (64 * R);
            jb.storeOff = 0;
            jb.seqOff = seqBytes;
            seqBytes += (long long)I + J;
            jb.outOff = outBytes;
            outBytes += (long long)I + J;
            jb.carryOff = -1;
            if (jb.nStrips > 1) {
                jb.carryOff = carryWords;
                carryWords += J + 1LL;
            }
            jobs.push_back(jb);
            pairOf.push_back(k);
            rcq.emplace_back();
            if (v == 1) {
                std::string& s = rcq.back();
                s.resize((size_t)I);
                for (int x = 0; x < I; ++x) s[(size_t)x] = (char)complement((unsigned char)pairs[k].query[I - 1 - x]);
            }
        }
    }
    const int nj = (int)jobs.size();
    stats.pairs += n;
    if (nj == 0) return;

    std::vector<int> order(nj);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) {
        return (long long)jobs[a].I * jobs[a].J > (long long)jobs[b].I * jobs[b].J;
    });
    struct Group {
        int begin, end;
        long long bytes;
    };
    std::vector<Group> groups;
    {
        Group g{0, 0, 0};
        for (int k = 0; k < nj; ++k) {
            AlignJob& jb = jobs[order[k]];
            const long long b = (store_bytes(jb.I, jb.J, jb.R) + 15) & ~15LL;
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
    std::vector<int> lists;
    struct GroupLists {
        int traceOff, fillOff[3], fillN[3];
    };
    std::vector<GroupLists> gl(groups.size());
    for (size_t q = 0; q < groups.size(); ++q) {
        gl[q].traceOff = (int)lists.size();
        for (int k = groups[q].begin; k < groups[q].end; ++k) lists.push_back(order[k]);
        for (int v = 0; v < 3; ++v) {
            gl[q].fillOff[v] = (int)lists.size();
            for (int k = groups[q].begin; k < groups[q].end; ++k)
                if (jobs[order[k]].R == kRowsPerLane[v]) lists.push_back(order[k]);
            gl[q].fillN[v] = (int)lists.size() - gl[q].fillOff[v];
        }
    }
    std::vector<uint8_t> seq((size_t)seqBytes);
    for (int k = 0; k < nj; ++k) {
        const PairView& pv = pairs[pairOf[k]];
        std::memcpy(seq.data() + jobs[k].seqOff, pv.target, (size_t)pv.J);
        std::memcpy(seq.data() + jobs[k].seqOff + pv.J, rcq[k].empty() ? pv.query : rcq[k].data(), (size_t)pv.I);
    }

    std::vector<uint8_t> hOut((size_t)outBytes);
    std::vector<int> hEnds(8 * (size_t)nj);

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
    dOut_.reserve((size_t)outBytes, false);
    dEnds_.reserve(8 * (size_t)nj, false);
    dCarry_.reserve((size_t)std::max(1LL, carryWords), false);
    dStore_.reserve((size_t)maxStore, false);
    check(hipMemcpyAsync(dSeq_.ptr, seq.data(), (size_t)seqBytes, hipMemcpyHostToDevice, stream_), "upload");
    check(hipMemcpyAsync(dJobs_.ptr, jobs.data(), sizeof(AlignJob) * nj, hipMemcpyHostToDevice, stream_), "upload");
    check(hipMemcpyAsync(dList_.ptr, lists.data(), sizeof(int) * lists.size(), hipMemcpyHostToDevice, stream_),
          "upload");
    check(hipMemsetAsync(dEnds_.ptr, 0xff, sizeof(int) * 8 * nj, stream_), "memset");   // -1: never traced

    for (size_t q = 0; q < groups.size(); ++q) {
        if (profiling) check(hipEventRecord(ev_[0], stream_), "event");
        for (int v = 0; v < 3; ++v) {
            if (gl[q].fillN[v] == 0) continue;
            const int* list = dList_.ptr + gl[q].fillOff[v];
            if (mode == kEndsLocal)
                launch_fill_ends<kEndsLocal>(kRowsPerLane[v], gl[q].fillN[v], stream_, dJobs_.ptr, list, dSeq_.ptr,
                                             dStore_.ptr, dCarry_.ptr, dEnds_.ptr, p);
            else
                launch_fill_ends<kEndsSemiglobal>(kRowsPerLane[v], gl[q].fillN[v], stream_, dJobs_.ptr, list,
                                                  dSeq_.ptr, dStore_.ptr, dCarry_.ptr, dEnds_.ptr, p);
            check(hipGetLastError(), "k_align_fill_ends launch");
            stats.launches++;
        }
        if (profiling) {
            check(hipEventRecord(ev_[1], stream_), "event");
            check(hipEventRecord(ev_[2], stream_), "event");
        }
        const int gn = groups[q].end - groups[q].begin;
        hipLaunchKernelGGL(k_align_trace_ends, dim3((gn + 63) / 64), dim3(64), 0, stream_, dJobs_.ptr,
                           dList_.ptr + gl[q].traceOff, gn, dSeq_.ptr, dStore_.ptr, dOut_.ptr, dEnds_.ptr, mode);
        check(hipGetLastError(), "k_align_trace_ends launch");
        if (profiling) {
            check(hipEventRecord(ev_[3], stream_), "event");
            check(hipStreamSynchronize(stream_), "sync");
            float ms = 0.f;
            check(hipEventElapsedTime(&ms, ev_[0], ev_[1]), "event");
            stats.fillMs += ms;
            check(hipEventElapsedTime(&ms, ev_[2], ev_[3]), "event");
            stats.traceMs += ms;
        }
        stats.groups++;
        stats.bytes += (double)groups[q].bytes;
    }

    check(hipMemcpyAsync(hOut.data(), dOut_.ptr, (size_t)outBytes, hipMemcpyDeviceToHost, stream_), "download");
    check(hipMemcpyAsync(hEnds.data(), dEnds_.ptr, sizeof(int) * 8 * nj, hipMemcpyDeviceToHost, stream_), "download");
    check(hipStreamSynchronize(stream_), "sync");
    dSeq_.trim();
    dJobs_.trim();
    dList_.trim();
    dOut_.trim();
    dEnds_.trim();
    dCarry_.trim();
    dStore_.trim();

    for (int k = 0; k < nj; k += per) {
        int use = k;
        if (bothStrands && hEnds[8 * (size_t)k] < hEnds[8 * (size_t)(k + 1)]) use = k + 1;
        stats.cells += (long long)per * jobs[k].I * jobs[k].J;
        PairResult& o = out[pairOf[k]];
        const AlignJob& jb = jobs[use];
        const int* e = &hEnds[8 * (size_t)use];
        const int i1 = e[1], j1 = e[2], i0 = e[3], j0 = e[4], len = e[5];
        if (i0 < 0 || j0 < 0 || i0 > i1 || j0 > j1 || i1 > jb.I || j1 > jb.J || len < 0 || len > jb.I + jb.J) {
            o.status = PBCCS_EINVAL;   // never traced, or a walk that left the matrix
            continue;
        }
        stats.traceSteps += len;
        const uint8_t* r = hOut.data() + jb.outOff;
        o.transcript.assign(reinterpret_cast<const char*>(r), (size_t)len);
        std::reverse(o.transcript.begin(), o.transcript.end());
        o.scoreI = e[0];
        ext[pairOf[k]] = EndsExtent{j0, j1, i0, i1, use != k ? 1 : 0};
    }
}

}  // namespace align
}  // namespace pbccs

// pbccs_amd/csrc/align_kernels.hip -- k_align_fill / k_align_trace and the engine's align workspace
// (align_kernels.hpp).
#include "align_kernels.hpp"

#include <algorithm>
#include <cfloat>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <type_traits>

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

// std::max(a, b): a unless a < b (the reference's choice between equal values, -0.0f and 0.0f included)
__host__ __device__ __forceinline__ float smax(float a, float b) { return (a < b) ? b : a; }

// Column-0 / row-0 values of the reference's initialisation.  k is the row (or column) index.
// NW: Score(k, 0) = k * Insert, Score(0, k) = k * Delete (step = that parameter).
// Affine: M(0, 0) = 0, M = -FLT_MAX elsewhere; GAP(0, 0) = -FLT_MAX, GAP(k) = GapOpen + (k - 1) * GapExtend.
__host__ __device__ __forceinline__ float edge_m(int k) { return k == 0 ? 0.f : -FLT_MAX; }
__host__ __device__ __forceinline__ float edge_gap(int k, float open, float ext)
{
    return k == 0 ? -FLT_MAX : open + (float)(k - 1) * ext;
}

// Bits 0-3: the bases a byte stands for (A 1, C 2, G 4, T 8); bit 4: one of the six two-base codes
// IsIupacPartialMatch knows (AffineAlignment.cpp:65-78).  Every other byte is 0.  For unequal bytes t, q:
// IsIupacPartialMatch(t, q) || IsIupacPartialMatch(q, t) == the sets meet and exactly one byte is a code.
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

// The strip carry is written by lane 63 of one strip and read by lane 0 of the next strip of the same wavefront:
// agent-scope relaxed accesses keep both off the CU's L1, whose lines may still hold the previous strip's values.
__device__ __forceinline__ void carry_store(uint32_t* p, uint32_t v)
{
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ uint32_t carry_load(uint32_t* p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// One wavefront per pair.  Cell (i, j), 1 <= i <= I, 1 <= j <= J: row i - 1 = (strip * 64 + lane) * R + r, computed
// at step t = (j - 1) + lane of its strip; its move byte lands at ((strip * (J + 63) + t) * 64 + lane) * R + r.
// NW byte: ArgMax3 (0 diagonal, 1 up / insert, 2 left / delete).  Affine byte: bit 0 = M(i, j) >= GAP(i, j),
// bits 1-2 = first maximum of {M(i, j-1) + open, GAP(i, j-1) + ext, M(i-1, j) + open, GAP(i-1, j) + ext}.
template <int KIND, int R>
__global__ __launch_bounds__(64) void k_align_fill(const AlignJob* __restrict__ jobs, const int* __restrict__ list,
                                                   const uint8_t* __restrict__ seq, uint8_t* __restrict__ store,
                                                   uint32_t* carry, uint32_t* __restrict__ scores, AlignScoring p)
{
    constexpr bool NW = KIND == kNw;
    constexpr bool IUPAC = KIND == kAffineIupac;
    using S = typename std::conditional<NW, int, float>::type;
    const int lane = threadIdx.x;
    const int jobIdx = list[blockIdx.x];
    const AlignJob jb = jobs[jobIdx];
    const int I = jb.I, J = jb.J, T = J + 63;
    const uint8_t* tg = seq + jb.seqOff;
    const uint8_t* qr = tg + J;
    uint32_t* cr = carry + (jb.carryOff >= 0 ? jb.carryOff : 0);
    uint8_t* st = store + jb.storeOff;
    const float open = p.gapOpen, ext = p.gapExtend;

    for (int s = 0; s < jb.nStrips; ++s) {
        const int row0 = (s * 64 + lane) * R;   // matrix row above the lane's first row
        const bool rows = row0 < I;
        const bool carryOut = lane == 63 && s + 1 < jb.nStrips;
        S leftA[R], leftB[R];
        int qc[R], qb[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int i = row0 + r + 1;
            qc[r] = i <= I ? (int)qr[i - 1] : 0;
            qb[r] = IUPAC ? iupac_bits(qc[r]) : 0;
            if constexpr (NW) {
                leftA[r] = i * p.insert;
                leftB[r] = 0;
            } else {
                leftA[r] = edge_m(i);
                leftB[r] = edge_gap(i, open, ext);
            }
        }
        S diagA, diagB;
        if constexpr (NW) {
            diagA = row0 * p.insert;
            diagB = 0;
        } else {
            diagA = edge_m(row0);
            diagB = edge_gap(row0, open, ext);
        }
        S botA = leftA[R - 1], botB = leftB[R - 1];
        // the next step's inputs are loaded one step ahead: the target byte, and for lane 0 the row above the strip
        int tcN = 0;
        S cinA = 0, cinB = 0;
        {
            const int j1 = 1 - lane;
            if (j1 >= 1 && j1 <= J) tcN = tg[j1 - 1];
            if (lane == 0) {
                if (s == 0) {
                    if constexpr (NW) cinA = p.delete_;
                    else {
                        cinA = edge_m(1);
                        cinB = edge_gap(1, open, ext);
                    }
                } else {
                    cinA = from_bits<S>(carry_load(cr + 2));
                    if constexpr (!NW) cinB = from_bits<S>(carry_load(cr + 3));
                }
            }
        }
        for (int t = 0; t < T; ++t) {
            const int j = t - lane + 1;
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
                tcN = (j2 >= 1 && j2 <= J) ? (int)tg[j2 - 1] : 0;
                if (lane == 0 && j2 <= J) {
                    if (s == 0) {
                        if constexpr (NW) cinA = j2 * p.delete_;
                        else {
                            cinA = edge_m(j2);
                            cinB = edge_gap(j2, open, ext);
                        }
                    } else {
                        cinA = from_bits<S>(carry_load(cr + 2 * j2));
                        if constexpr (!NW) cinB = from_bits<S>(carry_load(cr + 2 * j2 + 1));
                    }
                }
            }
            if (rows && j >= 1 && j <= J) {
                S dA = diagA, dB = diagB, uA = upA, uB = upB;
                const int tb = IUPAC ? iupac_bits(tc) : 0;
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

__device__ __forceinline__ int move_byte(const uint8_t* st, int i, int j, int R, int T)
{
    const int row = i - 1;
    const int strip = row / (64 * R);
    const int rem = row - strip * 64 * R;
    const int l = rem / R, r = rem - l * R;
    const int t = (j - 1) + l;
    return st[(((long long)strip * T + t) * 64 + l) * R + r];
}

// One thread per pair: the serial walk from (I, J) to (0, 0), one dependent byte load per step.  Writes the
// transcript reversed (M R I D) and its length.  Boundary cells (row 0, column 0) take their moves from the
// reference's guarded candidates over the initialisation values.  An affine walk that is in M on row 0 or column 0
// (the reference reads outside its matrices there), or a GAP move that would leave the matrix, stops the walk
// and flags the pair.
__global__ __launch_bounds__(64) void k_align_trace(const AlignJob* __restrict__ jobs, const int* __restrict__ list,
                                                    int n, const uint8_t* __restrict__ seq,
                                                    const uint8_t* __restrict__ store, uint8_t* __restrict__ out,
                                                    int* __restrict__ lens, int* __restrict__ status, AlignScoring p)
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
    const float open = p.gapOpen, ext = p.gapExtend;
    int i = I, j = J, len = 0, flag = 0;
    const int cap = I + J;
    if (p.kind == kNw) {
        while ((i > 0 || j > 0) && len < cap) {
            const int mv = i == 0 ? 2 : (j == 0 ? 1 : move_byte(st, i, j, R, T));
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
        bool inM = (move_byte(st, i, j, R, T) & 1) != 0;
        while ((i > 0 || j > 0) && len < cap) {
            if (inM) {
                if (i == 0 || j == 0) {
                    flag = kTraceFlagged;
                    break;
                }
                o[len++] = qr[i - 1] == tg[j - 1] ? 'M' : 'R';
                --i;
                --j;
                if (i > 0 && j > 0) inM = (move_byte(st, i, j, R, T) & 1) != 0;
                else if (i == 0 && j == 0) inM = true;   // M(0, 0) = 0 >= GAP(0, 0) = -FLT_MAX
                else inM = -FLT_MAX >= edge_gap(i + j, open, ext);
            } else {
                int arg;
                if (i > 0 && j > 0) {
                    arg = move_byte(st, i, j, R, T) >> 1;
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
    if (i > 0 || j > 0) flag = kTraceFlagged;
    lens[jobIdx] = len;
    status[jobIdx] = flag;
}

template <int KIND>
void launch_fill(int R, int grid, hipStream_t st, const AlignJob* jobs, const int* list, const uint8_t* seq,
                 uint8_t* store, uint32_t* carry, uint32_t* scores, const AlignScoring& p)
{
    switch (R) {
        case 2:
            hipLaunchKernelGGL((k_align_fill<KIND, 2>), dim3(grid), dim3(64), 0, st, jobs, list, seq, store, carry,
                               scores, p);
            break;
        case 4:
            hipLaunchKernelGGL((k_align_fill<KIND, 4>), dim3(grid), dim3(64), 0, st, jobs, list, seq, store, carry,
                               scores, p);
            break;
        default:
            hipLaunchKernelGGL((k_align_fill<KIND, 8>), dim3(grid), dim3(64), 0, st, jobs, list, seq, store, carry,
                               scores, p);
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
    const int forced = (int)env_ll("PBCCS_ALIGN_ROWS_PER_LANE", 0);   // tests: every strip path with every R
    for (int R : kRowsPerLane)
        if (forced == R) return R;
    for (int R : kRowsPerLane)
        if (I <= 64 * R) return R;
    return kRowsPerLane[2];
}

}  // namespace

AlignRunner::AlignRunner(int device) : device_(device)
{
    check(hipSetDevice(device_), "hipSetDevice");
    check(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking), "hipStreamCreate");
    for (auto& e : ev_) check(hipEventCreate(&e), "hipEventCreate");
}

AlignRunner::~AlignRunner()
{
    if (stream_) {
        (void)hipStreamSynchronize(stream_);
        (void)hipStreamDestroy(stream_);
    }
    for (auto& e : ev_)
        if (e) (void)hipEventDestroy(e);
}

void AlignRunner::Run(const AlignScoring& p, const PairView* pairs, int n, PairResult* out)
{
    RunImpl(p, pairs, n, out, nullptr);
}

void AlignRunner::RunKeep(const AlignScoring& p, const PairView* pairs, int n, std::vector<KeptTranscript>* out)
{
    std::vector<PairResult> res((size_t)std::max(0, n));
    out->assign((size_t)std::max(0, n), KeptTranscript());
    RunImpl(p, pairs, n, res.data(), out);
    for (int k = 0; k < n; ++k) (*out)[k].status = res[k].status;
}

// keep: the reversed transcripts stay in dOut_ and are not downloaded
void AlignRunner::RunImpl(const AlignScoring& p, const PairView* pairs, int n, PairResult* out,
                          std::vector<KeptTranscript>* keep)
{
    const long long budget = std::max(1LL, env_ll("PBCCS_ALIGN_WORKSPACE_MB", 2048)) << 20;
    // host part: degenerate pairs, the work list
    std::vector<AlignJob> jobs;
    std::vector<int> pairOf;
    long long seqBytes = 0, outBytes = 0, carryWords = 0;
    for (int k = 0; k < n; ++k) {
        const int I = pairs[k].I, J = pairs[k].J;
        PairResult& o = out[k];
        o = PairResult();
        if (I == 0 || J == 0) {   // all D, all I, or empty: no launch
            o.transcript.assign((size_t)(I + J), I == 0 ? 'D' : 'I');
            if (p.kind == kNw) {
                o.scoreI = I == 0 ? J * p.delete_ : I * p.insert;
            } else {
                const float m = edge_m(I + J), g = edge_gap(I + J, p.gapOpen, p.gapExtend);
                o.scoreF = m >= g ? m : g;
            }
            continue;
        }
        if (p.kind == kNw) {
            const long long mx = std::max(std::max(std::llabs((long long)p.match), std::llabs((long long)p.mismatch)),
                                          std::max(std::llabs((long long)p.insert), std::llabs((long long)p.delete_)));
            if (((long long)I + J) * mx > 0x7fffffffLL) {
                o.status = PBCCS_EINVAL;
                continue;
            }
        }
        AlignJob jb;
        jb.I = I;
        jb.J = J;
        jb.R = rows_per_lane(I);
        jb.nStrips = (I + 64 * jb.R - 1) / (64 * jb.R);
        if (store_bytes(I, J, jb.R) > budget) {
            o.status = PBCCS_EOOM;
            continue;
        }
        jb.storeOff = 0;
        jb.seqOff = seqBytes;
        seqBytes += (long long)I + J;
        jb.outOff = outBytes;
        outBytes += (long long)I + J;
        jb.carryOff = -1;
        if (jb.nStrips > 1) {
            jb.carryOff = carryWords;
            carryWords += 2LL * (J + 1);
        }
        jobs.push_back(jb);
        pairOf.push_back(k);
    }
    const int nj = (int)jobs.size();
    stats.pairs += n;
    if (nj == 0) return;

    std::vector<int> order(nj);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) {
        return (long long)jobs[a].I * jobs[a].J > (long long)jobs[b].I * jobs[b].J;
    });
    // launch groups over the sorted list: each group's move stores fit the budget
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
    // per group: the trace list (the group's slice of `order`), then one fill list per R
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
        std::memcpy(seq.data() + jobs[k].seqOff + pv.J, pv.query, (size_t)pv.I);
    }

    std::vector<uint8_t> hOut((size_t)(keep ? 0 : outBytes));
    std::vector<int> hLens(nj), hStatus(nj);
    std::vector<uint32_t> hScores(2 * (size_t)nj);

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
    dLens_.reserve((size_t)nj, false);
    dStatus_.reserve((size_t)nj, false);
    dScores_.reserve(2 * (size_t)nj, false);
    dCarry_.reserve((size_t)std::max(1LL, carryWords), false);
    dStore_.reserve((size_t)maxStore, false);
    check(hipMemcpyAsync(dSeq_.ptr, seq.data(), (size_t)seqBytes, hipMemcpyHostToDevice, stream_), "upload");
    check(hipMemcpyAsync(dJobs_.ptr, jobs.data(), sizeof(AlignJob) * nj, hipMemcpyHostToDevice, stream_), "upload");
    check(hipMemcpyAsync(dList_.ptr, lists.data(), sizeof(int) * lists.size(), hipMemcpyHostToDevice, stream_),
          "upload");
    check(hipMemsetAsync(dLens_.ptr, 0, sizeof(int) * nj, stream_), "memset");
    check(hipMemsetAsync(dStatus_.ptr, 0xff, sizeof(int) * nj, stream_), "memset");   // -1: never traced

    for (size_t q = 0; q < groups.size(); ++q) {
        if (profiling) check(hipEventRecord(ev_[0], stream_), "event");
        for (int v = 0; v < 3; ++v) {
            if (gl[q].fillN[v] == 0) continue;
            const int* list = dList_.ptr + gl[q].fillOff[v];
            if (p.kind == kNw)
                launch_fill<kNw>(kRowsPerLane[v], gl[q].fillN[v], stream_, dJobs_.ptr, list, dSeq_.ptr, dStore_.ptr,
                                 dCarry_.ptr, dScores_.ptr, p);
            else if (p.kind == kAffine)
                launch_fill<kAffine>(kRowsPerLane[v], gl[q].fillN[v], stream_, dJobs_.ptr, list, dSeq_.ptr,
                                     dStore_.ptr, dCarry_.ptr, dScores_.ptr, p);
            else
                launch_fill<kAffineIupac>(kRowsPerLane[v], gl[q].fillN[v], stream_, dJobs_.ptr, list, dSeq_.ptr,
                                          dStore_.ptr, dCarry_.ptr, dScores_.ptr, p);
            check(hipGetLastError(), "k_align_fill launch");
            stats.launches++;
        }
        if (profiling) {
            check(hipEventRecord(ev_[1], stream_), "event");
            check(hipEventRecord(ev_[2], stream_), "event");
        }
        const int gn = groups[q].end - groups[q].begin;
        hipLaunchKernelGGL(k_align_trace, dim3((gn + 63) / 64), dim3(64), 0, stream_, dJobs_.ptr,
                           dList_.ptr + gl[q].traceOff, gn, dSeq_.ptr, dStore_.ptr, dOut_.ptr, dLens_.ptr,
                           dStatus_.ptr, p);
        check(hipGetLastError(), "k_align_trace launch");
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

    if (!keep)
        check(hipMemcpyAsync(hOut.data(), dOut_.ptr, (size_t)outBytes, hipMemcpyDeviceToHost, stream_), "download");
    check(hipMemcpyAsync(hLens.data(), dLens_.ptr, sizeof(int) * nj, hipMemcpyDeviceToHost, stream_), "download");
    check(hipMemcpyAsync(hStatus.data(), dStatus_.ptr, sizeof(int) * nj, hipMemcpyDeviceToHost, stream_), "download");
    check(hipMemcpyAsync(hScores.data(), dScores_.ptr, sizeof(uint32_t) * 2 * nj, hipMemcpyDeviceToHost, stream_),
          "download");
    check(hipStreamSynchronize(stream_), "sync");
    // the stream is idle: buffers that growth retired can go
    dSeq_.trim();
    dJobs_.trim();
    dList_.trim();
    dOut_.trim();
    dLens_.trim();
    dStatus_.trim();
    dScores_.trim();
    dCarry_.trim();
    dStore_.trim();

    for (int k = 0; k < nj; ++k) {
        PairResult& o = out[pairOf[k]];
        const AlignJob& jb = jobs[k];
        stats.cells += (long long)jb.I * jb.J;
        if (hStatus[k] != 0 || hLens[k] < 0 || hLens[k] > jb.I + jb.J) {
            o.status = PBCCS_EINVAL;   // the walk left the matrix (pathological parameters)
            continue;
        }
        stats.traceSteps += hLens[k];
        if (keep) {
            KeptTranscript& kt = (*keep)[pairOf[k]];
            kt.onDevice = true;
            kt.off = jb.outOff;
            kt.len = hLens[k];
            continue;
        }
        const uint8_t* r = hOut.data() + jb.outOff;
        o.transcript.assign(reinterpret_cast<const char*>(r), (size_t)hLens[k]);
        std::reverse(o.transcript.begin(), o.transcript.end());
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

}  // namespace align
}  // namespace pbccs

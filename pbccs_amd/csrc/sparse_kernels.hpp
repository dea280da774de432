// pbccs_amd/csrc/sparse_kernels.hpp -- SparseAlign<K> on the device: the K-mer seeds of a (target, query) pair and
// their sparse-dynamic-programming chain (include/pacbio/ccs/SparseAlignment.h FindSeeds / SparseAlign,
// src/ChainSeeds.cpp with matchReward 3), plus the rows SdpRangeFinder::InitRangeFinder would allow each position
// of a linear draft.  DESIGN.md §3.16.
//
// Five kernels per launch group, one job per block:
//   k_sparse_count    2-bit K-mer codes of both sequences (the query's reverse complement formed here), the two
//                     direct-address K-mer count tables, the job's seed total
//   k_sparse_index    tables -> bucket starts, position lists in ascending order per K-mer, row starts, the previous
//                     seed column / row of every position, and the seeds themselves in (v, h) order
//   k_sparse_visible  one lane per seed: its visible-left and visible-above candidates (both depend on positions
//                     only, never on scores: a window of at most K + 1 columns / rows, one binary search each)
//   k_sparse_sweep    one wavefront per job: the row sweep.  Lanes score a row group's seeds; the column set is a
//                     direct array column -> (seed, z) with an occupancy bitmap, in LDS when it fits; the bitmap's
//                     summary level (one bit per non-zero word) is always in LDS
//   k_sparse_ranges   the alignable read rows per draft position from the nearest anchor on each side
// No block waits for another, and every loop is bounded by a length, a seed count or a word count of the job.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "engine.hpp"

namespace pbccs {
namespace sparse {

constexpr int kMinK = 4, kMaxK = 8;          // a direct-address table of 4^K <= 65536 counters
constexpr int kMaxLen = 1 << 20;             // per sequence: scores and z stay far inside int32
constexpr int kWidth = 30;                   // SdpRangeFinder's WIDTH
constexpr int kMatchReward = 3;
constexpr int kSweepLdsCols = 6144;          // column sets of up to this many columns (len1 + K + 1) live in LDS
constexpr long long kDefaultMaxSeeds = 1LL << 22;   // per job (PBCCS_SPARSE_MAX_SEEDS)
constexpr int kSeedInts = 6;                 // h, v, score, pred, visible-left, visible-above per seed

// Where a job's per-position arrays sit in its slice of the workspace (ints).
struct Layout {
    long long tcode, qcode, tstart, qstart, tcur, qcur, tpos, trank, qpos, rowstart, pcol, prow, colSeed, colZ,
        bitmap, total;
    __host__ __device__ Layout(int len1, int len2, int k)
    {
        const long long T = 1LL << (2 * k), cols = (long long)len1 + k + 1;
        long long at = 0;
        tcode = at, at += len1;
        qcode = at, at += len2;
        tstart = at, at += T + 1;
        qstart = at, at += T + 1;
        tcur = at, at += T;
        qcur = at, at += T;
        tpos = at, at += len1;
        trank = at, at += len1;
        qpos = at, at += len2;
        rowstart = at, at += len2 + 1;
        pcol = at, at += len1;
        prow = at, at += len2;
        colSeed = at, at += cols;
        colZ = at, at += cols;
        bitmap = at, at += (cols + 31) / 32;
        total = at;
    }
};

struct SparseJob {
    long long tOff, qOff;    // the sequences in the uploaded pool; the query as given
    long long posOff;        // this job's Layout in the position workspace (ints)
    long long seedOff;       // kSeedInts arrays of nSeeds ints in the seed pool; set after the count
    long long anchorOff;     // anchor pairs (h, v); room for max(0, min(len1, len2) - K + 1)
    long long rangeOff;      // 2 * len1 ints, -1 when not asked for
    int len1, len2, rc, nSeeds;
};

struct SparseOut {
    long long score;                   // best chain score, 0 without a chain
    unsigned long long rangeCells;     // sum of the ranges' lengths
    int nAnchors, anchorStart;         // the chain occupies [anchorStart, anchorStart + nAnchors) of the job's room
};

// One pair as the C ABI hands it over; results go straight to the caller's buffers.
struct SparseInput {
    const char* target;
    int len1;
    const char* query;
    int len2;
    int rc;
    int* anchors;
    int anchorCap;
    int* ranges;   // may be NULL
};

struct SparseResult {
    int status = 0;
    int nAnchors = 0;
    long long nSeeds = 0, score = 0;
};

struct SparseStats {
    long long jobs = 0, seeds = 0, anchors = 0, launches = 0;
    long long rangeCells = 0, fullCells = 0;   // over the jobs that asked for ranges: inside them / len1 (len2 + 1)
    double deviceMs = 0.0;                      // all five kernels, profiling on
};

// One pair whose chain stays on the device (RunKeep): what the host may know of it.
struct KeptChain {
    int status = 0;
    int nAnchors = 0;
    long long nSeeds = 0;
    long long anchorOff = 0;   // the chain's first (h, v) pair in AnchorsDevice(), in pairs
};

class SparseRunner {
public:
    // stream: the caller's stream to run on (the POA runner's); nullptr creates one
    explicit SparseRunner(int device, hipStream_t stream = nullptr);
    ~SparseRunner();
    SparseRunner(const SparseRunner&) = delete;
    SparseRunner& operator=(const SparseRunner&) = delete;

    // Every pair of the batch.  Per job: PBCCS_EINVAL for a letter outside ACGT or a sequence longer than kMaxLen,
    // PBCCS_EOOM when its seeds exceed the cap (PBCCS_SPARSE_MAX_SEEDS, default 4194304) or its own arrays half the
    // workspace budget (PBCCS_SPARSE_WORKSPACE_KB, default 1048576) -- known after the counting pass, the job gets
    // no further device work -- and PBCCS_ERANGE when the chain does not fit anchorCap.  The batch is split into
    // launch groups whose arrays fit the budget.
    void Run(int k, const SparseInput* in, int n, std::vector<SparseResult>* out);

    // The same for a consumer on the device: no anchor or range leaves it (the inputs' anchors / ranges are not
    // read), every chain of the call stays in AnchorsDevice() until the next call, and the host learns each
    // pair's status, seed count, chain length and the chain's place.
    void RunKeep(int k, const SparseInput* in, int n, std::vector<KeptChain>* out);
    const int* AnchorsDevice() const { return dAnchors_.ptr; }

    SparseStats stats;
    bool profiling = false;

private:
    void RunImpl(int k, const SparseInput* in, int n, std::vector<SparseResult>* out, std::vector<KeptChain>* keep);
    int device_;
    hipStream_t stream_ = nullptr;
    bool ownStream_ = true;
    hipEvent_t ev_[4] = {nullptr, nullptr, nullptr, nullptr};
    DevVec<uint8_t> dSeq_;
    DevVec<SparseJob> dJobs_, dActive_;
    DevVec<long long> dCount_;
    DevVec<int> dPos_, dSeeds_, dAnchors_, dRanges_;
    DevVec<SparseOut> dOut_;
};

}  // namespace sparse
}  // namespace pbccs

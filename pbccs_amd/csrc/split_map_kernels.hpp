// pbccs_amd/csrc/split_map_kernels.hpp -- split mapping on the device: a read that holds several passes fused
// across a missed adapter is placed on the draft as a chain of LOCAL segments, on either strand, at a jump
// penalty (the reference has no such step, the rule is this project's own).
//
// The DP is row-synchronous: G(i), the best chain that ends at or before read row i (less the jump penalty), is
// the Start value of every cell of row i + 1 in both orientations, so both orientations of a read advance
// together, one read row at a time.  k_split_fill runs one wavefront per read.  Lanes own blocks of C consecutive
// draft columns; within a row the Delete chain H(i, j) = max(V(i, j), H(i, j - 1) - 4) is a max-plus scan that
// carries the start cell: serial inside a lane's block, a log-step DPP scan across the lanes, the carry handed
// from tile to tile when the draft is wider than 64 C columns.  The previous row of H and its start cells stay
// in registers when the draft fits one tile; otherwise each lane parks its own columns in a per-read row buffer
// that only it reads back.  Per row one record reaches memory; k_split_chain walks the records back into
// segments.  No matrix is stored.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "engine.hpp"
#include "map_kernels.hpp"

namespace pbccs {
namespace map {

constexpr int kSplitColsPerLane[3] = {2, 4, 8};   // the compiled C values: tiles of 128, 256, 512 columns
constexpr int kSplitMaxSegments = 64;             // the most segments a call may ask back per read

// One read (both orientations) on the device.
struct SplitJob {
    long long readOff;    // the read as given at seq[readOff, +I)
    long long draftOff;   // the draft at seq[draftOff, +J)
    long long rowOff;     // the read's I + 1 row records in the record buffer
    long long bufOff;     // the read's row buffer (2 * nTiles * C * 64 words of 64 bits), -1 on the register path
    int I, J;
    int nTiles;           // ceil(J / (64 C)); 1 on the register path
    int pad;
};

// Row i of a read: G(i), the row where G last rose, and R(i): score, (o << 31) | j, packed start cell
struct SplitRow {
    int G, gRow, score;
    uint32_t oj, start;
};

// Per read: the chain's end row and score
struct SplitHead {
    int endRow, score;
};

// One segment as the device reports it: extents on the read as given and on the draft (forward coordinates)
struct SplitSeg {
    int rc, rb, re, tb, te, score;
};

struct SplitTail {
    int count, score;   // the chain's true segment count and score
};

struct SplitMapStats {
    long long jobs = 0;       // reads given
    long long cells = 0;      // 2 I J per read that reached the device
    long long launches = 0;
    long long tiled = 0;      // reads that ran on the row-buffer path
    double deviceMs = 0.0;    // k_split_fill + k_split_chain, profiling on
};

struct SplitMapResult {
    int count = 0;       // the chain's segment count (may exceed segs.size())
    int truncated = 0;
    int score = 0;       // the chain score; 0: not mapped
    int status = 0;      // PBCCS_OK / PBCCS_EOOM
    std::vector<SplitSeg> segs;   // the last min(count, maxSegments) segments, in read order
};

// The engine's split-mapping workspace.  It runs on the stream of the engine's MapRunner; calls on one engine
// take turns (the engine's mapping mutex).
class SplitMapRunner {
public:
    SplitMapRunner(int device, hipStream_t stream);
    ~SplitMapRunner();
    SplitMapRunner(const SplitMapRunner&) = delete;
    SplitMapRunner& operator=(const SplitMapRunner&) = delete;

    // Split-maps every read of every group; out holds one result per read, group after group.  A NULL or empty
    // read is never mapped.  Reads are sorted by cell count, largest first, one launch per (C, path); the batch is
    // split into launch groups whose row records and row buffers fit the budget (PBCCS_SPLIT_WORKSPACE_KB,
    // default 262144); a read whose own buffers exceed it gets status PBCCS_EOOM and no device work.
    // PBCCS_SPLIT_COLS_PER_LANE forces a compiled C (a draft wider than 64 C then runs tiled),
    // PBCCS_SPLIT_TILED=1 forces the row-buffer path.
    void Run(const MapGroup* groups, int ng, int jumpPenalty, int maxSegments, std::vector<SplitMapResult>* out);

    SplitMapStats stats;
    bool profiling = false;

private:
    int device_;
    hipStream_t stream_;
    hipEvent_t ev_[2] = {nullptr, nullptr};
    DevVec<uint8_t> dSeq_;
    DevVec<SplitJob> dJobs_;
    DevVec<int> dList_;
    DevVec<unsigned long long> dBuf_;
    DevVec<SplitRow> dRows_;
    DevVec<SplitHead> dHeads_;
    DevVec<SplitSeg> dSegs_;
    DevVec<SplitTail> dTails_;
};

}  // namespace map
}  // namespace pbccs

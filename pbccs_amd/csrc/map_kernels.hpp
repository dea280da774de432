// pbccs_amd/csrc/map_kernels.hpp -- MapToDraft on the device: what SparsePoa::OrientAndAddRead + FindConsensus
// report for a read on a graph that holds only the draft as one unbranched path, i.e. a LOCAL alignment of the
// read (both orientations) against the linear draft with DefaultPoaConfig's integer scores, reduced to the three
// things the polish needs: orientation, extent on the read, extent on the draft.
//
// k_map_fill runs one wavefront per (read, orientation) job as a skewed anti-diagonal wavefront: lane l owns R
// consecutive read rows and at step t computes draft column t - l + 1 for them; lane l - 1's bottom cell (score and
// packed start cell) and the draft base arrive by one wave_shr:1 DPP each.  Every cell carries the Start cell its
// path left from, so no score, move or path reaches memory and nothing is walked back; the wave keeps a running
// best end cell under the reference's tie rule.  A read taller than 64 R rows runs in row strips; lane 63's bottom
// row goes to the next strip's lane 0 through a per-job boundary buffer (one 64-bit word per column).
// DESIGN.md §3.15.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "engine.hpp"

namespace pbccs {
namespace map {

constexpr int kRowsPerLane[3] = {4, 8, 16};   // the compiled R values: strips of 256, 512, 1024 rows
constexpr int kMaxLen = 65535;                // a start cell packs (i0 << 16) | j0
// DefaultPoaConfig(LOCAL), ConsensusCore PoaConfig / AlignConfig: integers
constexpr int kMatch = 3, kMismatch = -5, kInsert = -4, kDelete = -4;

// One (read, orientation) on the device.  The read is on rows (I), the draft on columns (J); both >= 1.
struct MapJob {
    long long readOff;    // the read as given at seq[readOff, +I); the reverse complement is formed in the kernel
    long long draftOff;   // the draft at seq[draftOff, +J)
    long long carryOff;   // into the boundary buffer (J + 1 words of 64 bits), -1 for a single-strip job
    int I, J;
    int rc;               // 1: map the reverse complement
    int nStrips;          // ceil(I / (64 R))
};

// Per job: best score, its end cell (i1, j1) and the packed start cell (i0 << 16) | j0 of the path that ends there.
struct MapCell {
    int score, endI, endJ;
    uint32_t start;
};

struct MapStats {
    long long jobs = 0;       // reads given (each is two device jobs)
    long long cells = 0;      // 2 (I + 1) J per mapped-or-not read that reached the device
    long long launches = 0, strips = 0;
    double deviceMs = 0.0;    // k_map_fill, profiling on
};

// One draft and the reads to place on it (pbccs_map_input)
struct MapGroup {
    const char* draft;
    int J;
    const char* const* seqs;
    const int* lens;
    int n;
};

struct MapResult {
    int mapped = 0, rc = 0;
    int ext[4] = {0, 0, 0, 0};   // ExtentOnRead begin/end, ExtentOnConsensus begin/end
    int score = 0;               // the chosen orientation's score (the larger one when not mapped)
    int status = 0;              // PBCCS_OK / PBCCS_EOOM
};

// The engine's mapping workspace: its own stream and the small per-call buffers.
class MapRunner {
public:
    explicit MapRunner(int device);
    ~MapRunner();
    MapRunner(const MapRunner&) = delete;
    MapRunner& operator=(const MapRunner&) = delete;

    // Maps every read of every group; out holds one result per read, group after group.  A NULL or empty read is
    // never mapped.  Jobs are sorted by cell count, largest first, one launch per R; multi-strip jobs are split
    // into launch groups whose boundary buffers fit the budget (PBCCS_MAP_WORKSPACE_KB, default 262144); a read
    // whose own buffers exceed it gets status PBCCS_EOOM and no device work.
    void Run(const MapGroup* groups, int ng, float minScoreToAdd, std::vector<MapResult>* out);

    // the engine's mapping stream (SplitMapRunner queues its work on it too)
    hipStream_t stream() const { return stream_; }

    MapStats stats;
    bool profiling = false;

private:
    int device_;
    hipStream_t stream_ = nullptr;
    hipEvent_t ev_[2] = {nullptr, nullptr};
    DevVec<uint8_t> dSeq_;
    DevVec<MapJob> dJobs_;
    DevVec<int> dList_;
    DevVec<unsigned long long> dCarry_;
    DevVec<MapCell> dOut_;
};

}  // namespace map
}  // namespace pbccs

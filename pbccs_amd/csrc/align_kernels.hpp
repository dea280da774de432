// pbccs_amd/csrc/align_kernels.hpp -- batched pairwise alignment on the device (ConsensusCore Align/):
// Align (Needleman-Wunsch, int32; PairwiseAlignment.cpp:125-212) and AlignAffine / AlignAffineIupac (two-state
// affine, float32; AffineAlignment.cpp:110-252), bit-exact.
//
// k_align_fill runs one wavefront per pair as a skewed anti-diagonal wavefront: lane l owns R consecutive query
// rows and at step t computes target column t - l + 1 for them; lane l - 1's bottom row arrives through a
// one-lane shift.  A query taller than 64 R rows runs in strips; a strip's last row is carried to the next strip
// through a small per-pair buffer.  No score matrix reaches HBM: each cell leaves one move byte (the traceback's
// decision, taken from the very values the fill computed), stored by (strip, step, lane, row-in-lane) so that a
// step's store is one contiguous 64 R-byte write.  k_align_trace walks the bytes, one thread per pair.
// DESIGN.md §3.14.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <vector>

#include "engine.hpp"

namespace pbccs {
namespace align {

constexpr int kNw = 0, kAffine = 1, kAffineIupac = 2;   // PBCCS_ALIGN_*
constexpr int kRowsPerLane[3] = {2, 4, 8};              // the compiled R values: strips of 128, 256, 512 rows
constexpr int kTraceFlagged = 1;                        // trace status: the walk in M reached row 0 or column 0

struct AlignScoring {
    int kind;
    int match, mismatch, insert, delete_;                          // AlignParams
    float matchScore, mismatchScore, gapOpen, gapExtend, partial;   // AffineAlignmentParams
};

// One pair on the device.  The query is on rows (I), the target on columns (J); both >= 1.
struct AlignJob {
    long long storeOff;   // byte offset of the pair's move bytes in the launch group's store (16-byte aligned)
    long long seqOff;     // target at seq[seqOff, +J), query at seq[seqOff + J, +I)
    long long carryOff;   // into the strip carry (2 (J + 1) words), -1 for a single-strip pair
    long long outOff;     // into the reversed-transcript pool (I + J bytes)
    int I, J;
    int R;                // rows per lane of the pair's fill
    int nStrips;          // ceil(I / (64 R))
};

// Move bytes of one pair: nStrips strips x (J + 63) steps x 64 lanes x R rows.
inline long long store_bytes(int I, int J, int R)
{
    const long long strips = (I + 64LL * R - 1) / (64LL * R);
    return strips * (J + 63LL) * 64LL * R;
}

struct AlignStats {
    long long pairs = 0, cells = 0, launches = 0, traceSteps = 0, groups = 0;
    double fillMs = 0.0, traceMs = 0.0;
    double bytes = 0.0;   // move-store bytes the fills covered
};

struct PairView {
    const char* target;
    int J;
    const char* query;
    int I;
};

struct PairResult {
    std::string transcript;
    int scoreI = 0;
    float scoreF = 0.f;
    int status = 0;   // PBCCS_OK / PBCCS_EINVAL / PBCCS_EOOM
};

// One pair whose transcript stays on the device (RunKeep): what the host may know of it.
struct KeptTranscript {
    int status = 0;        // PBCCS_OK / PBCCS_EINVAL / PBCCS_EOOM
    bool onDevice = false; // false: a degenerate or refused pair, nothing of it is in TranscriptsDevice()
    long long off = 0;     // the transcript, reversed (its last character first), in TranscriptsDevice()
    int len = 0;
};

// The engine's align workspace: its own stream, the move store and the small per-call buffers.
class AlignRunner {
public:
    explicit AlignRunner(int device);
    ~AlignRunner();
    AlignRunner(const AlignRunner&) = delete;
    AlignRunner& operator=(const AlignRunner&) = delete;

    // Aligns every pair (degenerate ones on the host).  The pairs are sorted by cell count, largest first, and
    // split into launch groups whose move stores fit the budget (PBCCS_ALIGN_WORKSPACE_MB, default 2048); a pair
    // whose own store exceeds it gets status PBCCS_EOOM and no device work.
    void Run(const AlignScoring& p, const PairView* pairs, int n, PairResult* out);

    // The same for a consumer on the device: no transcript leaves it, every transcript of the call stays in
    // TranscriptsDevice() until the next call, and the host learns each pair's status, length and place.
    void RunKeep(const AlignScoring& p, const PairView* pairs, int n, std::vector<KeptTranscript>* out);
    const uint8_t* TranscriptsDevice() const { return dOut_.ptr; }

    AlignStats stats;
    bool profiling = false;

private:
    void RunImpl(const AlignScoring& p, const PairView* pairs, int n, PairResult* out,
                 std::vector<KeptTranscript>* keep);
    int device_;
    hipStream_t stream_ = nullptr;
    hipEvent_t ev_[4] = {nullptr, nullptr, nullptr, nullptr};
    DevVec<uint8_t> dSeq_, dStore_, dOut_;
    DevVec<AlignJob> dJobs_;
    DevVec<int> dList_, dLens_, dStatus_;
    DevVec<uint32_t> dCarry_, dScores_;
};

}  // namespace align
}  // namespace pbccs

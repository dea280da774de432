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
// DESIGN.md §3.14.  RunBanded is the opt-in certified band for long near-identical pairs (align_band.hpp,
// align_band_kernels.hip); Run and RunKeep do not use it.  RunEnds is the ends-free int32 aligner
// (SEMIGLOBAL, LOCAL: k_align_fill_ends / k_align_trace_ends in align_modes_kernels.hip) on the
// same workspace; Run, RunKeep and RunBanded stay GLOBAL.
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
constexpr int kTraceLeftBand = 2;                       // banded trace status: the walk would read outside the band
constexpr int kEndsSemiglobal = 1, kEndsLocal = 2;      // RunEnds' modes (PBCCS_POA_SEMIGLOBAL / _LOCAL)
constexpr int kMoveDiag = 0, kMoveDelete = 1, kMoveExtra = 2, kMoveStart = 3;   // k_align_fill_ends' move bytes

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

// One pair of a banded fill (align_band.hpp): the band's diagonals lo <= j - i <= hi and the
// steps T of one strip in the store, nStrips x T x 64 lanes x R rows.
struct AlignBandJob {
    long long storeOff, seqOff, carryOff, outOff;   // as AlignJob's
    int I, J;
    int R, nStrips;
    int lo, hi;
    int T, pad;
};

// The banded route is off unless asked for.  w < 0: the automatic first half-width.
struct BandOptions {
    bool on = false;
    long long w = -1;
};

// What became of one pair of a banded call.
struct BandInfo {
    int banded = 0;     // 1: the answer is a certified banded fill's; 0: the full fill's (or the host's)
    int w = 0;          // the last half-width tried
    int attempts = 0;   // banded fills of this pair: 0, 1 or 2
    int reason = 0;     // why the pair took the full fill (kBand*), 0 for a banded pair
};

struct AlignBandStats {
    long long pairs = 0, bandedPairs = 0, secondAttempts = 0;
    long long fallbacks[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // by reason
    long long bandCells = 0, fullCells = 0;              // cells inside the bands filled; I x J of the same pairs
    long long launches = 0, groups = 0, traceSteps = 0;
    double storeBytes = 0.0;                             // banded move-store bytes the fills covered
    double fillMs = 0.0, traceMs = 0.0;
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

// What an ends-free alignment covers: target[targetBegin, targetEnd) and query[queryBegin, queryEnd), the query's
// in the coordinates of the sequence that was aligned (its reverse complement when rc).
struct EndsExtent {
    int targetBegin = 0, targetEnd = 0, queryBegin = 0, queryEnd = 0, rc = 0;
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

    // Run with the certified band (align_band.hpp): at most two banded fills per pair, the second at the width the
    // first one's score calls for; a pair's banded answer is returned only when its certificate holds, every other
    // pair goes through Run.  info (optional, n entries) says what became of each pair.
    void RunBanded(const AlignScoring& p, const PairView* pairs, int n, PairResult* out, const BandOptions& band,
                   BandInfo* info);

    // The ends-free modes of the int32 aligner (mode kEndsSemiglobal / kEndsLocal; p.kind is kNw, Insert and Delete
    // <= 0): the reference POA's rules on the target as one unbranched path.  Sorting, the rows per lane, the launch
    // groups and PBCCS_EOOM are Run's.  out[k].transcript covers the extent ext[k]; out[k].scoreI is the end cell's
    // score.  bothStrands: the query is also aligned reverse complemented and forward wins iff its score >= the
    // other's.
    void RunEnds(const AlignScoring& p, int mode, bool bothStrands, const PairView* pairs, int n, PairResult* out,
                 EndsExtent* ext);

    AlignStats stats;
    AlignBandStats bandStats;
    bool profiling = false;

private:
    void RunImpl(const AlignScoring& p, const PairView* pairs, int n, PairResult* out,
                 std::vector<KeptTranscript>* keep);
    void BandAttempt(const AlignScoring& p, const PairView* pairs, const std::vector<int>& idx,
                     const std::vector<long long>& ws, PairResult* out, std::vector<double>* scoreOut,
                     std::vector<int>* verdict);
    int device_;
    hipStream_t stream_ = nullptr;
    hipEvent_t ev_[4] = {nullptr, nullptr, nullptr, nullptr};
    DevVec<uint8_t> dSeq_, dStore_, dOut_;
    DevVec<AlignJob> dJobs_;
    DevVec<AlignBandJob> dBandJobs_;
    DevVec<int> dList_, dLens_, dStatus_, dEnds_;
    DevVec<uint32_t> dCarry_, dScores_;
};

}  // namespace align
}  // namespace pbccs

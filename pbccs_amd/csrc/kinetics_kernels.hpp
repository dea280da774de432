// pbccs_amd/csrc/kinetics_kernels.hpp -- consensus kinetics on the device: the subreads' inter-pulse durations (ip)
// and pulse widths (pw), carried onto consensus coordinates through each read's Align transcript and folded into
// one value per consensus base and strand.  The reference (2015 pbccs) has no kinetics; the
// rules are this project's own:
//
//   Frames and CodecV1.  Kinetics are unsigned frame counts.  A B:S tag holds frames as they are, a B:C tag CodecV1
//   codes: code c decodes to base[g] + ((c & 63) << g) with g = c >> 6 and base = {0, 64, 192, 448}, so the
//   representable values are 0..63 step 1, 64..190 step 2, 192..444 step 4, 448..952 step 8.  Encoding: frames
//   above 952 give 255, otherwise the nearest representable value, a tie to the larger one (65 -> 66).  (pbbam's
//   published codec restated without pbbam at hand: unpinned.)
//
//   Which reads, and where.  For a consensus C of length L and a read of length I: MapToDraft(C, read, 0) gives rc,
//   the extent [rb, re) in the oriented read and [tb, te) on C (map_kernels.hpp); Align(C[tb, te), oriented[rb, re))
//   with the default AlignConfig gives the transcript (align_kernels.hpp).  A read that is not mapped, has an empty
//   extent or whose alignment fails is skipped with a per-read status.
//
//   Contribution.  A transcript column M or R aligns oriented read position q to consensus position p and
//   contributes the read's values at original index q (rc == 0) or I - 1 - q (rc == 1: the kinetics of a reverse
//   complemented read are the array reversed).  I columns contribute nothing; a D column leaves p without a
//   contribution from this read.  rc == 0 reads are the forward strand, rc == 1 reads the reverse strand.
//
//   Per strand, position and track: n(p) contributing reads, S(p) the integer sum of their frames; the mean is
//   (2 S + n) / (2 n) in integer division (halves round up), 0 where n == 0, saturating at 65535; the code is the
//   CodecV1 encoding of the mean.  All integer arithmetic: order-independent and exactly reproducible.  A read whose
//   ip or pw is absent contributes nothing to that track and is not counted in it, so the coverage is kept per
//   track.  fn / rn: the reads of the strand that contributed at least one column to a track they carry.  Forward
//   arrays are indexed by consensus position; reverse-strand arrays are stored in the reverse strand's own
//   direction, entry k belonging to consensus position L - 1 - k.
//
// k_kin_columns: one wavefront per read walks the transcript in chunks of 64 characters, one per lane; two ballots
// ("advances the target": M R D, "advances the query": M R I), a popcount of the lanes below and two running
// carries give every lane its target and query position; M / R lanes store the original read index (rc flip
// applied), D lanes -1, to qidx[read][p - tb].  Each target position of a read is written exactly once: no
// atomics, no LDS.  k_kin_reduce: one thread per (ZMW, strand, position) loops over the ZMW's reads of that strand
// in input order, sums ip[qidx] and pw[qidx], forms the rounded means and their codes (branch-free arithmetic on
// the group boundaries) and writes them at the strand's index; the thread of position 0 also counts fn / rn from
// the per-read "contributed" flags k_kin_columns left.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "engine.hpp"

namespace pbccs {
namespace kinetics {

constexpr int kReduceThreads = 256;
// per-read status (PBCCS_KIN_*)
constexpr int kUsed = 0, kUnmapped = 1, kEmptyExtent = 2, kAlignFailed = 3;

// CodecV1, host and device.  encode: g = the group of the frame count, low = (frames - base[g]) rounded half up
// to the group's step; a low of 64 carries into the next group's first code by plain addition, and the result is
// clamped to 255.
__host__ __device__ inline unsigned codec_v1_decode(unsigned c)
{
    const unsigned g = (c >> 6) & 3u;
    return 64u * ((1u << g) - 1u) + ((c & 63u) << g);
}
__host__ __device__ inline unsigned codec_v1_encode(unsigned frames)
{
    const unsigned g = (unsigned)(frames >= 64u) + (unsigned)(frames >= 192u) + (unsigned)(frames >= 448u);
    const unsigned base = 64u * ((1u << g) - 1u);
    const unsigned c = (g << 6) + ((frames - base + ((1u << g) >> 1)) >> g);
    return c < 255u ? c : 255u;
}

// One read that reaches the device.
struct KinRead {
    long long trOff;     // the transcript at tr[trOff, +trLen)
    long long qidxOff;   // the read's consensus extent at qidx[qidxOff, + te - tb)
    long long ipOff;     // the read's I frames at frames[ipOff, +I); -1: the track is absent
    long long pwOff;
    int trLen, I;
    int rc, rb;
    int tb, te;
};

struct KinZmw {
    long long outOff;         // the ZMW's 4 L outputs at [outOff, +4 L): fwd ipd, fwd pw, rev ipd, rev pw
    int L;
    int readBegin, readEnd;   // its device reads, in input order
};

// One block of k_kin_reduce: kReduceThreads positions from p0 of one strand of one ZMW
struct KinBlock {
    int zmw, strand, p0;
};

// The caller's view of one read and one ZMW (pbccs_kinetics_read / pbccs_kinetics_pileup_input)
struct ReadView {
    const char* tr;
    int trLen;
    int rc, rb, tb, te, I;
    const uint16_t* ip;
    const uint16_t* pw;
    int skip;   // kUsed, or the reason the caller already has for skipping the read
};

struct ZmwView {
    int L;
    const ReadView* reads;
    int n;
};

// Outputs of one ZMW; every pointer may be NULL.  Index 2 strand + track: fwd ipd, fwd pw, rev ipd, rev pw.
struct ZmwOut {
    uint16_t* mean[4];
    uint8_t* code[4];
    int* coverage[4];
    int contributed[2];   // fn, rn
    int* readStatus;      // n entries
};

struct KinStats {
    long long reads = 0;                                   // reads given
    long long unmapped = 0, emptyExtent = 0, alignFailed = 0;   // reads skipped, by reason
    long long columns = 0;                                 // transcript columns walked
    long long positions = 0;                               // (ZMW, strand, position) threads
    long long launches = 0;
    double columnsMs = 0.0, reduceMs = 0.0;                // profiling on
};

// The engine's kinetics workspace: its own stream and buffers.
class KineticsRunner {
public:
    explicit KineticsRunner(int device);
    ~KineticsRunner();
    KineticsRunner(const KineticsRunner&) = delete;
    KineticsRunner& operator=(const KineticsRunner&) = delete;

    // Throws std::invalid_argument, before any device work, for a read that is not skipped and whose transcript
    // holds a character other than M R I D, does not span [tb, te), runs past the read's end, or whose extents
    // leave the consensus.  A read with te == tb or without a query column is skipped as kEmptyExtent.
    void Run(const ZmwView* zmws, int nz, ZmwOut* out);

    KinStats stats;
    bool profiling = false;

private:
    int device_;
    hipStream_t stream_ = nullptr;
    hipEvent_t ev_[3] = {nullptr, nullptr, nullptr};
    DevVec<uint8_t> dTr_, dCode_;
    DevVec<uint16_t> dFrames_, dMean_;
    DevVec<int> dQidx_, dContrib_, dCov_, dCounts_;
    DevVec<KinRead> dReads_;
    DevVec<KinZmw> dZmws_;
    DevVec<KinBlock> dBlocks_;
};

}  // namespace kinetics
}  // namespace pbccs

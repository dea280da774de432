// pbccs_amd/csrc/demux_kernels.hpp -- barcode calling on the device: which barcode pair flanks a CCS read
// (the reference has no demultiplexing, the rules are this project's own, built from the
// SEMIGLOBAL rules of §3.26).
//
// Every barcode is placed inside a window at each end of every read.  k_demux_score runs one wavefront per
// (read, end): lanes are barcodes, 64 per pass; a lane keeps its barcode's whole DP column (rows 0..LMAX) in
// registers and steps through the window's columns, whose byte is the same for every lane.  Only the score of each
// barcode, the running maximum of its last row, leaves the DP; the wave reduces best, best index and second.
// k_demux_call applies the call rules, one lane per read; k_demux_extent fills the two called (window, barcode)
// pairs of a read once more, one lane per pair, and carries each cell's start column through the DP in the rules'
// candidate order, so the extents are the traceback's without a move store.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "engine.hpp"

namespace pbccs {
namespace demux {

constexpr int kMaxBarcodeLen = 64;
constexpr int kMaxBarcodes = 65535;
constexpr int kMaxWindow = 1024;
constexpr int kWordsPerBarcode = 2;   // 64 bases, 2 bits each, in two 64-bit words

// One read on the device: its two windows lie in the window pool, the trailing one after the leading one
struct DemuxJob {
    long long winOff;   // the leading window at win[winOff, +wlen), the trailing one at win[winOff + wlen, +wlen)
    int wlen;           // min(W, n)
    int off;            // max(0, n - W): the trailing window's place on the read
};

// One end of one read: the best barcode (smallest index holding the maximum) and the maximum over the others
struct DemuxEnd {
    int best, index, second;   // second INT_MIN with one barcode
};

// One read's call; the extents are in read coordinates
struct DemuxCall {
    int lead, trail;       // the called barcodes i and j (filled for an uncalled read too)
    int called;
    int score, scoreLead, quality;
    int leadBegin, leadEnd, trailBegin, trailEnd;
};

struct DemuxOptions {
    int match = 3, mismatch = -5, insert = -4, delete_ = -4;
    int symmetric = 0;
    int window = 0;
    int minQuality = 0, minScoreLead = 0;
};

struct DemuxStats {
    long long reads = 0;
    long long cells = 0;      // 2 * min(W, n) * the sum of the barcode lengths, per read
    long long launches = 0;
    double deviceMs = 0.0;    // the three kernels, profiling on
};

// The engine's demultiplexing workspace: its own stream; calls on one engine take turns on it.
class DemuxRunner {
public:
    explicit DemuxRunner(int device);
    ~DemuxRunner();
    DemuxRunner(const DemuxRunner&) = delete;
    DemuxRunner& operator=(const DemuxRunner&) = delete;

    // seqs / lens: the barcodes (validated by the caller: 1..64 bases of ACGT, 1..65535 of them).  reads / rlens:
    // n reads of any length (NULL or empty: nothing is launched for it).  ends, calls: n entries each (ends: two
    // per read); scores: NULL, or n * 2 * B ints.  The batch is split into launch groups whose windows and score
    // rows fit the budget (PBCCS_DEMUX_WORKSPACE_KB, default 262144); a group holds at least one read.
    void Run(const char* const* seqs, const int* lens, int B, const DemuxOptions& o, const char* const* reads,
             const int* rlens, int n, DemuxEnd* ends, DemuxCall* calls, int* scores);

    DemuxStats stats;
    bool profiling = false;

private:
    int device_;
    hipStream_t stream_ = nullptr;
    hipEvent_t ev_[2] = {nullptr, nullptr};
    DevVec<uint8_t> dWin_;
    DevVec<DemuxJob> dJobs_;
    DevVec<unsigned long long> dCodes_;
    DevVec<int> dLens_;
    DevVec<int> dScores_;
    DevVec<DemuxEnd> dEnds_;
    DevVec<DemuxCall> dCalls_;
};

}  // namespace demux
}  // namespace pbccs

// pbccs_amd/csrc/window_kernels.hpp -- the two device steps of the windowed polish.
//
//   k_window_cuts   one lane per (read, window boundary): where a draft position falls in the read's forward text,
//                   from the read's SparseAlign chain, which sparse_kernels.hip left on the device
//                   (SparseRunner::RunKeep).  One binary search per lane; only the cuts are downloaded.
//   k_window_join   one wavefront per pair of neighbouring windows: walks both windows' draft-to-consensus
//                   transcripts, which align_kernels.hip left on the device (AlignRunner::RunKeep), in chunks of 64
//                   characters, forms the length of the run of M each character ends with a wave scan, notes for
//                   every candidate draft position of the overlap the consensus position it maps to when 2 guard
//                   neighbouring M surround it, and takes the first candidate in the order mid, mid + 1, mid - 1, ...
//                   that both transcripts accept.  Only (p, cut, cut) per joint is downloaded.
// Every loop is bounded by a chain length, a transcript length or a candidate count.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "engine.hpp"

namespace pbccs {
namespace window {

struct CutTask {
    long long anchorOff;   // the chain's first (h, v) pair in the kept anchors, in pairs; h relative to the read's tstart
    int nAnchors;          // >= 1
    int b;                 // the boundary, relative to the read's tstart
    int flen;              // the read's length
};

struct JoinTask {
    long long offA, offB;   // the two reversed transcripts in the kept transcript pool
    long long workOff;      // 2 (hi - lo + 1) ints of the candidate workspace
    int lenA, lenB;
    int sA, sB;             // the windows' first draft positions
    int lo, hi, mid;        // candidates lo <= p <= hi, tried outwards from mid
    int guard;
};

struct JoinOut {
    int p;   // -1: no join
    int cutA, cutB;
};

// The engine's window workspace: its own stream and the small task buffers.
class WindowRunner {
public:
    explicit WindowRunner(int device);
    ~WindowRunner();
    WindowRunner(const WindowRunner&) = delete;
    WindowRunner& operator=(const WindowRunner&) = delete;

    // anchors: SparseRunner::AnchorsDevice() after a RunKeep whose stream is idle
    void Cuts(const int* anchors, const std::vector<CutTask>& tasks, std::vector<int>* cuts);
    // transcripts: AlignRunner::TranscriptsDevice() after a RunKeep; the tasks' workOff are set here
    void Joins(const uint8_t* transcripts, std::vector<JoinTask>& tasks, std::vector<JoinOut>* out);

    long long cutLaunches = 0, joinLaunches = 0;

private:
    int device_;
    hipStream_t stream_ = nullptr;
    DevVec<CutTask> dCutTasks_;
    DevVec<JoinTask> dJoinTasks_;
    DevVec<JoinOut> dJoinOut_;
    DevVec<int> dCuts_, dWork_;
};

}  // namespace window
}  // namespace pbccs

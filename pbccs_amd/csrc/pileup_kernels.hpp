// pbccs_amd/csrc/pileup_kernels.hpp -- the subread pileup on the consensus: which subread bases stand over each
// consensus position.  The reference (2015 pbccs) has no pileup; the rules are this project's
// own.  Everything is integer arithmetic and order-independent.
//
//   Inputs.  A consensus C of length L over any characters; per read its text (length I), the placement rc,
//   [rb, re) in the oriented read, [tb, te) on C, and a transcript over M R I D (M R D advance the consensus, M R I
//   the oriented read).  Validation, refusals and per-read status codes are those of kinetics_kernels.hpp.  The
//   oriented read is the text for rc == 0, its reverse complement for rc == 1; a character outside ACGT is code 5
//   ("other") in either orientation and its complement is N.
//
//   Orientation.  Every output is indexed by consensus position, or by slot, in the consensus's own direction for
//   both strands (unlike the kinetics arrays, whose reverse-strand entries run in the reverse strand's direction).
//
//   Counts, per strand (rc == 0 forward, rc == 1 reverse), over used reads: counts[strand][p][c], c in A C G T gap
//   other: an M or R column at p adds 1 at the code of the oriented read base, a D column 1 at gap.  Slot s in
//   [0, L] lies before position s (slot L after the last one): a read with k >= 1 I columns after s - tb
//   consensus-advancing columns and before the next adds 1 to ins_reads[strand][s] and k to ins_bases[strand][s].
//   slot_cov[s]: used reads of both strands with tb <= s <= te.  cov[p]: the sum of the twelve counts at p.
//
//   Plurality.  J[p][c] = counts[0][p][c] + counts[1][p][c], c in 0..4 (other does not compete): the c with the
//   largest J; on a tie the consensus's own base when it is among the tied codes, else the lowest code; 255 where
//   all five are 0.  ins_plurality[s] = 2 (ins_reads[0][s] + ins_reads[1][s]) > slot_cov[s].
//
//   Gapped rows.  maxins[s]: the longest insertion a used read has at slot s.  first[s] = s + sum_{s' < s}
//   maxins[s'], col[p] = first[p] + maxins[p], width = L + sum maxins.  One row of width bytes per read, blank
//   (' ') for a read that is not used.  A used read writes at col[p], p in [tb, te), its oriented base or '-' for a
//   D column; at slot s in [tb, te] its k inserted bases, right-aligned (cells first[s] + maxins[s] - k ...) for
//   s == tb, left-aligned otherwise; for tb < s < te the unused cells of the slot are '-'.
//
// k_pile_columns: one wavefront per read walks the transcript 64 characters at a time; ballots and a popcount of
// the lanes below give each lane its consensus and read position; a consensus-advancing lane stores its code byte
// and, for the slot before it, the length of the I run that ends right below it and the read position where that
// run began.  The run may have begun in an earlier chunk: the length of the run still open at a chunk's end is
// carried, so each slot is written once, by one lane.  The four column counts are the ballots' popcounts.
// k_pile_reduce: one thread per (ZMW, slot) loops over the ZMW's reads in input order.  k_pile_scan: one block per
// ZMW, an exclusive scan of maxins in tiles of a block with a carry.  k_pile_rows: one thread per (read, slot).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "engine.hpp"
#include "kinetics_kernels.hpp"

namespace pbccs {
namespace pileup {

constexpr int kReduceThreads = 256;
constexpr int kScanThreads = 256;
constexpr int kRowThreads = 256;
// per-read status (PBCCS_KIN_*)
using kinetics::kAlignFailed;
using kinetics::kEmptyExtent;
using kinetics::kUnmapped;
using kinetics::kUsed;

// One read that reaches the device.
struct PileRead {
    long long trOff;     // the transcript at tr[trOff, +trLen)
    long long seqOff;    // the read's text at seq[seqOff, +I)
    long long colOff;    // its code bytes at code[colOff, + te - tb)
    long long slotOff;   // its te - tb + 1 slots at insLen / qAt[slotOff, ...)
    int trLen, I;
    int rc, rb;
    int tb, te;
    int zmw, row;        // its ZMW and its index among that ZMW's reads (the row it writes)
};

struct PileZmw {
    long long posOff;    // positions before this ZMW's: the sum of the earlier L
    long long slotOff;   // slots before this ZMW's: the sum of the earlier L + 1
    int L;
    int readBegin, readEnd;   // its device reads, in input order
};

// One block of k_pile_reduce: kReduceThreads slots from s0 of one ZMW
struct PileBlock {
    int zmw, s0;
};

// One block of k_pile_rows: kRowThreads slots from j0 of one read's extent
struct PileRowBlock {
    int read, j0;
};

struct ReadView {
    const char* tr;
    int trLen;
    const char* seq;
    int I;
    int rc, rb, tb, te;
    int skip;   // kUsed, or the reason the caller already has for skipping the read
};

struct ZmwView {
    const char* cons;
    int L;
    const ReadView* reads;
    int n;
};

// Outputs of one ZMW; every pointer may be NULL.
struct ZmwOut {
    int* counts;          // [2][L][6]
    int* insReads;        // [2][L + 1]
    int* insBases;        // [2][L + 1]
    int* slotCov;         // [L + 1]
    int* cov;             // [L]
    int* maxIns;          // [L + 1]
    uint8_t* plurality;   // [L]
    uint8_t* insPlurality;   // [L + 1]
    int* readStatus;      // n entries each
    int *nMatch, *nMismatch, *nIns, *nDel;
    long long covSum;
    int nUsed[2];
};

// The gapped rows of one ZMW
struct MsaOut {
    int width;
    int* col;     // [L], may be NULL
    char* rows;   // n rows of `rowWidth` bytes, may be NULL
    int rowWidth; // the width the caller sized rows for; a mismatch with `width` throws
};

struct PileStats {
    long long reads = 0;
    long long unmapped = 0, emptyExtent = 0, alignFailed = 0;
    long long columns = 0;   // transcript columns walked
    long long slots = 0;     // (ZMW, slot) threads of the reduction
    long long launches = 0;
    long long placed = 0;    // reads sent through the placement and alignment stage (pbccs_pileup_batch)
    long long shared = 0;    // ... of which the stage's transcript also fed a kinetics output
    double columnsMs = 0.0, reduceMs = 0.0, scanMs = 0.0, rowsMs = 0.0;   // profiling on
};

// The engine's pileup workspace: its own stream and buffers.
class PileupRunner {
public:
    explicit PileupRunner(int device);
    ~PileupRunner();
    PileupRunner(const PileupRunner&) = delete;
    PileupRunner& operator=(const PileupRunner&) = delete;

    // Throws std::invalid_argument, before any device work, for what KineticsRunner::Run refuses.  out may be NULL
    // (rows only), msa may be NULL (counts only); with msa the scan runs, and k_pile_rows where a ZMW has rows.
    void Run(const ZmwView* zmws, int nz, ZmwOut* out, MsaOut* msa);

    PileStats stats;
    bool profiling = false;

private:
    int device_;
    hipStream_t stream_ = nullptr;
    hipEvent_t ev_[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    DevVec<uint8_t> dTr_, dSeq_, dCons_, dCode_, dPlur_, dInsPlur_, dRows_;
    DevVec<int> dInsLen_, dQAt_, dColCounts_, dCounts_, dInsReads_, dInsBases_, dSlotCov_, dCov_, dMaxIns_, dFirst_,
        dCol_, dWidth_;
    DevVec<unsigned long long> dCovSum_;
    DevVec<long long> dRowBase_;
    DevVec<PileRead> dReads_;
    DevVec<PileZmw> dZmws_;
    DevVec<PileBlock> dBlocks_;
    DevVec<PileRowBlock> dRowBlocks_;
};

}  // namespace pileup
}  // namespace pbccs

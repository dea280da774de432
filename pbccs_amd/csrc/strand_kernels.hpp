// pbccs_amd/csrc/strand_kernels.hpp -- the strand-discordance screen.
//
// A rule of this project's own: the reference declares ConsensusSettings::Directional and stops at a TODO
// (include/pacbio/ccs/Consensus.h:94-109).  After a scoring round without a fast-score break (ConsensusQVs' sweep,
// or an explicit list) the per-(read, mutation) deltas are on the device; the screen sums them per strand.
//
//   k_strand_sums   one thread per mutation of the round (k_reduce's indexing).  The ZMW's reads in AddRead order:
//                   a read that is active and scores the mutation (ReadScoresMutation) adds its delta to sumF when
//                   its strand is forward, else to sumR, and counts in nF / nR.  No break.  Plain sequential FP64
//                   adds: on exact bands the sums are bit-equal to a host loop over Scores(m, 0).
//   k_strand_sites  one thread per template position (k_qv's indexing).  A mutation qualifies when
//                   nF >= minReads && nR >= minReads and (sumF > T && sumR < -T) or (sumR > T && sumF < -T); a NaN
//                   sum compares false.  The position reports its qualifying mutation with the largest
//                   min(|sumF|, |sumR|), the first in enumeration order on a tie.
#pragma once

#include <hip/hip_runtime.h>

#include "arrow_kernels.hpp"

namespace pbccs {

// per mutation, indexed like the round's scores (W.mutBase[k] + m)
struct StrandSums {
    double* sumF = nullptr;
    double* sumR = nullptr;
    int* nF = nullptr;
    int* nR = nullptr;
};

// per template position, indexed like the round's qvs (qvBase[k] + p)
struct StrandSiteOut {
    int* flag = nullptr;   // 1: the position is discordant
    int* code = nullptr;   // the reported mutation's code (valid where flag is 1)
    double* sumF = nullptr;
    double* sumR = nullptr;
};

void launch_strand_sums(const DevBatch& B, const ScoreWork& W, long long nMut, const StrandSums& S, hipStream_t s);
void launch_strand_sites(const ScoreWork& W, long long nPos, const long long* posBase, const int* posOff,
                         const StrandSums& S, const long long* qvBase, double minScore, int minReads,
                         const StrandSiteOut& out, hipStream_t s);

}  // namespace pbccs

// include/pbccs_amd/Pileup.hpp -- the subread pileup on a consensus through the C ABI: per-strand base counts at
// every consensus position, insertions at every slot, the plurality call, the effective coverage and each read's
// concordance (pbccs_pileup_batch).  Beyond the reference: 2015 pbccs has no pileup.
//
//   PacBio::CCS::ConsensusPileup(consensus, reads)
//   PacBio::CCS::PileupCigar(transcript, rb, readLength)
//
// Every array is indexed by consensus position, or by slot (slot s lies before position s), in the consensus's own
// direction for both strands -- unlike the kinetics arrays of Kinetics.hpp.
#pragma once

#include <array>
#include <cmath>
#include <cstdint>
#include <limits>
#include <stdexcept>
#include <string>
#include <vector>

#include "ConsensusCore.hpp"

namespace PacBio {
namespace CCS {

struct PileupRead {
    int Status = 0;   // PBCCS_KIN_*
    int NumMatch = 0, NumMismatch = 0, NumInsertion = 0, NumDeletion = 0;
    bool ReverseComplemented = false;
    int ReadBegin = 0, ReadEnd = 0, TemplateBegin = 0, TemplateEnd = 0;
    std::string Transcript;   // M R I D; empty for a read that is not used
    // matches over columns; NaN for a read that is not used
    double Concordance() const
    {
        const int n = NumMatch + NumMismatch + NumInsertion + NumDeletion;
        return Status == PBCCS_KIN_USED && n ? (double)NumMatch / n : std::numeric_limits<double>::quiet_NaN();
    }
};

struct ConsensusPileupResult {
    // per strand (0 forward, 1 reverse): Counts[strand][6 * p + c], c in A C G T gap other
    std::array<std::vector<int>, 2> Counts, InsertingReads, InsertedBases;
    std::vector<int> SlotCoverage, MaxInsertion, Coverage;
    std::vector<uint8_t> Plurality, InsertionPlurality;   // a code 0..4 or 255; 0 / 1
    std::vector<PileupRead> Reads;
    long long CoverageSum = 0;
    double EffectiveCoverage = 0.0;   // ec
    int NumUsed[2] = {0, 0};
};

// rb S, the transcript's runs with M -> =, R -> X, I, D, then readLength - re S; no zero-length clips
inline std::string PileupCigar(const std::string& transcript, int rb, int readLength)
{
    std::string out = rb > 0 ? std::to_string(rb) + "S" : "";
    int nq = 0;
    for (size_t k = 0; k < transcript.size();) {
        const char ch = transcript[k];
        size_t e = k;
        while (e < transcript.size() && transcript[e] == ch) ++e;
        const char op = ch == 'M' ? '=' : ch == 'R' ? 'X' : ch == 'I' ? 'I' : ch == 'D' ? 'D' : 0;
        if (!op) throw std::invalid_argument("PileupCigar: not a transcript character");
        out += std::to_string(e - k) + op;
        if (ch != 'D') nq += (int)(e - k);
        k = e;
    }
    const int tail = readLength - rb - nq;
    if (rb < 0 || tail < 0) throw std::invalid_argument("PileupCigar: the transcript leaves the read");
    if (tail) out += std::to_string(tail) + "S";
    return out;
}

// Places every read on the consensus (MapToDraft), aligns the extents (Align, default AlignConfig) and piles the
// transcripts' columns up per strand; banded: the aligner's certified band (the same answers).
inline ConsensusPileupResult ConsensusPileup(const std::string& consensus, const std::vector<std::string>& reads,
                                             bool banded = false)
{
    const int n = (int)reads.size();
    const size_t L = consensus.size();
    std::vector<const char*> seqs(n + 1, nullptr);
    std::vector<int> lens(n + 1, 0);
    std::vector<std::vector<char>> trBuf((size_t)n);
    std::vector<char*> trPtr(n + 1, nullptr);
    for (int k = 0; k < n; ++k) {
        seqs[k] = reads[k].data();
        lens[k] = (int)reads[k].size();
        trBuf[k].assign(L + reads[k].size() + 1, 0);
        trPtr[k] = trBuf[k].data();
    }
    ConsensusPileupResult res;
    std::vector<int> counts(12 * L + 1), insReads(2 * (L + 1)), insBases(2 * (L + 1));
    res.SlotCoverage.assign(L + 1, 0);
    res.MaxInsertion.assign(L + 1, 0);
    res.InsertionPlurality.assign(L + 1, 0);
    res.Coverage.assign(L + 1, 0);
    res.Plurality.assign(L + 1, 0);
    std::vector<std::vector<int>> per(11, std::vector<int>(n + 1, 0));
    const pbccs_pileup_input in{consensus.data(), (int)L, n, seqs.data(), lens.data(), nullptr, nullptr, nullptr};
    pbccs_pileup_output out{};
    out.counts = counts.data();
    out.ins_reads = insReads.data();
    out.ins_bases = insBases.data();
    out.slot_cov = res.SlotCoverage.data();
    out.max_ins = res.MaxInsertion.data();
    out.cov = res.Coverage.data();
    out.plurality = res.Plurality.data();
    out.ins_plurality = res.InsertionPlurality.data();
    out.read_status = per[0].data();
    out.n_match = per[1].data();
    out.n_mismatch = per[2].data();
    out.n_ins = per[3].data();
    out.n_del = per[4].data();
    out.rc = per[5].data();
    out.rb = per[6].data();
    out.re = per[7].data();
    out.tb = per[8].data();
    out.te = per[9].data();
    out.transcripts = trPtr.data();
    out.transcript_lens = per[10].data();
    pbccs_pileup_options opts;
    pbccs_pileup_options_default(&opts);
    if (banded) opts.band.mode = PBCCS_BAND_AUTO;
    ConsensusCore::detail::Check(pbccs_pileup_batch(ConsensusCore::detail::DefaultEngine(), &in, 1, &opts, &out));
    for (int s = 0; s < 2; ++s) {
        res.Counts[s].assign(counts.begin() + 6 * L * s, counts.begin() + 6 * L * (s + 1));
        res.InsertingReads[s].assign(insReads.begin() + (L + 1) * s, insReads.begin() + (L + 1) * (s + 1));
        res.InsertedBases[s].assign(insBases.begin() + (L + 1) * s, insBases.begin() + (L + 1) * (s + 1));
    }
    res.Coverage.resize(L);
    res.Plurality.resize(L);
    res.Reads.resize((size_t)n);
    for (int k = 0; k < n; ++k) {
        PileupRead& r = res.Reads[k];
        r.Status = per[0][k];
        r.NumMatch = per[1][k];
        r.NumMismatch = per[2][k];
        r.NumInsertion = per[3][k];
        r.NumDeletion = per[4][k];
        r.ReverseComplemented = per[5][k] != 0;
        r.ReadBegin = per[6][k];
        r.ReadEnd = per[7][k];
        r.TemplateBegin = per[8][k];
        r.TemplateEnd = per[9][k];
        r.Transcript.assign(trBuf[k].data(), (size_t)per[10][k]);
    }
    res.CoverageSum = out.cov_sum;
    res.EffectiveCoverage = L ? (double)out.cov_sum / (double)L : 0.0;
    res.NumUsed[0] = out.n_used[0];
    res.NumUsed[1] = out.n_used[1];
    return res;
}

}  // namespace CCS
}  // namespace PacBio

// include/pbccs_amd/Kinetics.hpp -- consensus kinetics through the C ABI: per-strand mean inter-pulse duration and
// pulse width of a consensus, from its subreads' ip / pw frame tracks (pbccs_kinetics_batch).
// Beyond the reference: 2015 pbccs has no kinetics.  The codec is pbbam's published CodecV1, restated (unpinned).
//
//   PacBio::CCS::CodecV1Decode / CodecV1Encode   one code or frame count
//   PacBio::CCS::KineticsRead                    a subread with its tracks (an empty track: absent)
//   PacBio::CCS::ConsensusKinetics(consensus, reads)
#pragma once

#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "ConsensusCore.hpp"

namespace PacBio {
namespace CCS {

// code c -> base[g] + ((c & 63) << g), g = c >> 6, base = {0, 64, 192, 448}
inline uint16_t CodecV1Decode(uint8_t code)
{
    const unsigned g = code >> 6;
    return (uint16_t)(64u * ((1u << g) - 1u) + ((code & 63u) << g));
}

// frames above 952 -> 255; otherwise the nearest representable value, a tie to the larger one (65 -> 66)
inline uint8_t CodecV1Encode(unsigned frames)
{
    if (frames > 952u) return 255;
    const unsigned g = (frames >= 64u) + (frames >= 192u) + (frames >= 448u);
    const unsigned c = (g << 6) + ((frames - 64u * ((1u << g) - 1u) + ((1u << g) >> 1)) >> g);
    return (uint8_t)(c < 255u ? c : 255u);
}

struct KineticsRead {
    std::string Sequence;
    std::vector<uint16_t> Ipd;          // one frame count per base, or empty: the read has no such track
    std::vector<uint16_t> PulseWidth;
};

// One strand's arrays.  Forward: indexed by consensus position; reverse: in the reverse strand's own direction
// (entry k belongs to consensus position length - 1 - k).
struct StrandKinetics {
    std::vector<uint8_t> IpdCodes, PulseWidthCodes;       // CodecV1 codes of the means
    std::vector<uint16_t> IpdMean, PulseWidthMean;        // rounded mean frames
    std::vector<int> IpdCoverage, PulseWidthCoverage;     // contributing reads per position
    int NumPasses = 0;                                    // fn / rn
};

struct ConsensusKineticsResult {
    StrandKinetics Forward, Reverse;
    std::vector<int> ReadStatus;   // PBCCS_KIN_* per read
};

// Places every read on the consensus (MapToDraft), aligns the extents (Align, default AlignConfig) and folds the
// M / R columns' frames per strand and position; banded: the aligner's certified band (the same answers).
// Throws std::invalid_argument for a track whose length differs from its read's.
inline ConsensusKineticsResult ConsensusKinetics(const std::string& consensus, const std::vector<KineticsRead>& reads,
                                                 bool banded = false)
{
    const int n = (int)reads.size();
    const size_t L = consensus.size();
    std::vector<const char*> seqs(n + 1, nullptr);
    std::vector<int> lens(n + 1, 0);
    std::vector<const unsigned short*> ip(n + 1, nullptr), pw(n + 1, nullptr);
    for (int k = 0; k < n; ++k) {
        const KineticsRead& r = reads[k];
        if ((!r.Ipd.empty() && r.Ipd.size() != r.Sequence.size()) ||
            (!r.PulseWidth.empty() && r.PulseWidth.size() != r.Sequence.size()))
            throw std::invalid_argument("ConsensusKinetics: a track's length differs from its read's");
        seqs[k] = r.Sequence.data();
        lens[k] = (int)r.Sequence.size();
        ip[k] = r.Ipd.empty() ? nullptr : r.Ipd.data();
        pw[k] = r.PulseWidth.empty() ? nullptr : r.PulseWidth.data();
    }
    ConsensusKineticsResult res;
    StrandKinetics* strands[2] = {&res.Forward, &res.Reverse};
    for (StrandKinetics* s : strands) {
        s->IpdCodes.assign(L, 0);
        s->PulseWidthCodes.assign(L, 0);
        s->IpdMean.assign(L, 0);
        s->PulseWidthMean.assign(L, 0);
        s->IpdCoverage.assign(L, 0);
        s->PulseWidthCoverage.assign(L, 0);
    }
    res.ReadStatus.assign(n + 1, 0);
    const pbccs_kinetics_input in{consensus.data(), (int)L, n, seqs.data(), lens.data(), ip.data(), pw.data()};
    pbccs_kinetics_output out{};
    for (int s = 0; s < 2; ++s) {
        out.mean[2 * s] = strands[s]->IpdMean.data();
        out.mean[2 * s + 1] = strands[s]->PulseWidthMean.data();
        out.code[2 * s] = strands[s]->IpdCodes.data();
        out.code[2 * s + 1] = strands[s]->PulseWidthCodes.data();
        out.coverage[2 * s] = strands[s]->IpdCoverage.data();
        out.coverage[2 * s + 1] = strands[s]->PulseWidthCoverage.data();
    }
    out.read_status = res.ReadStatus.data();
    pbccs_kinetics_options opts;
    pbccs_kinetics_options_default(&opts);
    if (banded) opts.band.mode = PBCCS_BAND_AUTO;
    ConsensusCore::detail::Check(pbccs_kinetics_batch(ConsensusCore::detail::DefaultEngine(), &in, 1, &opts, &out));
    res.Forward.NumPasses = out.n_contributed[0];
    res.Reverse.NumPasses = out.n_contributed[1];
    res.ReadStatus.resize(n);
    return res;
}

}  // namespace CCS
}  // namespace PacBio

// include/pbccs_amd/Align.hpp -- header-only C++ facade for ConsensusCore's pairwise aligners over the C ABI
// (pbccs_align_batch).  A caller of ConsensusCore/Align/{AlignConfig,PairwiseAlignment,AffineAlignment}.hpp
// compiles against it by swapping those includes for this header.
//
// Mirrored surface (reference file:line):
//   AlignMode, AlignParams, AlignConfig                     Align/AlignConfig.hpp, AlignConfig.cpp:48-74
//   PairwiseAlignment (+ FromTranscript)                    Align/PairwiseAlignment.hpp:65-97, .cpp:51-123, 309-368
//   Align (both overloads), TargetToQueryPositions (both)   Align/PairwiseAlignment.hpp:100-113, .cpp:125-303
//   AffineAlignmentParams, Default / IupacAware params,
//   AlignAffine, AlignAffineIupac                           Align/AffineAlignment.hpp, .cpp:215-252
// PairwiseAlignment, FromTranscript and TargetToQueryPositions are host code; the aligners run on the device.
// As in the reference, the aligners return a new PairwiseAlignment the caller deletes.  AlignBatch aligns many
// pairs in one call.  AlignLinear is not provided.
//
// Not in the reference: every aligner takes a trailing BandOptions (default off).  BandOptions::Auto() or
// BandOptions::Width(w) turns on the certified banded fill: a long, near-identical pair is filled
// inside a band of diagonals, and the banded answer is returned only where its score proves it to be the full
// fill's; every other pair takes the full fill.  The results are the same either way.
#pragma once

#include <algorithm>
#include <cmath>
#include <string>
#include <utility>
#include <vector>

#include "AlignMode.hpp"
#include "ConsensusCore.hpp"

namespace ConsensusCore {

struct AlignParams {
    int Match, Mismatch, Insert, Delete;
    AlignParams(int match, int mismatch, int insert, int delete_)
        : Match(match), Mismatch(mismatch), Insert(insert), Delete(delete_)
    {
    }
    static AlignParams Default() { return AlignParams(0, -1, -1, -1); }   // edit distance
};

struct AlignConfig {
    AlignParams Params;
    AlignMode Mode;
    AlignConfig(AlignParams params, AlignMode mode) : Params(params), Mode(mode) {}
    static AlignConfig Default() { return AlignConfig(AlignParams::Default(), GLOBAL); }
};

struct AffineAlignmentParams {
    float MatchScore, MismatchScore, GapOpen, GapExtend, PartialMatchScore;
    AffineAlignmentParams(float matchScore, float mismatchScore, float gapOpen, float gapExtend,
                          float partialMatchScore = 0)
        : MatchScore(matchScore), MismatchScore(mismatchScore), GapOpen(gapOpen), GapExtend(gapExtend),
          PartialMatchScore(partialMatchScore)
    {
    }
};

inline AffineAlignmentParams DefaultAffineAlignmentParams() { return AffineAlignmentParams(0, -1.0f, -1.0f, -0.5f, 0); }
inline AffineAlignmentParams IupacAwareAffineAlignmentParams()
{
    return AffineAlignmentParams(0, -1.0f, -1.0f, -0.5f, -0.25f);
}

struct BandOptions {
    int Mode;   // PBCCS_BAND_OFF / PBCCS_BAND_AUTO / PBCCS_BAND_WIDTH
    int W;      // the first half-width (PBCCS_BAND_WIDTH)
    static BandOptions Off() { return BandOptions{PBCCS_BAND_OFF, 0}; }
    static BandOptions Auto() { return BandOptions{PBCCS_BAND_AUTO, 0}; }
    static BandOptions Width(int w) { return BandOptions{PBCCS_BAND_WIDTH, w}; }
};

class PairwiseAlignment {
public:
    PairwiseAlignment(const std::string& target, const std::string& query)
        : target_(target), query_(query), transcript_(target.length(), 'Z')
    {
        if (target_.length() != query_.length()) throw InvalidInputError();
        for (size_t i = 0; i < target_.length(); i++) {
            const char t = target_[i], q = query_[i];
            if (t == '-' && q == '-') throw InvalidInputError();
            transcript_[i] = t == q ? 'M' : (t == '-' ? 'I' : (q == '-' ? 'D' : 'R'));
        }
    }
    std::string Target() const { return target_; }
    std::string Query() const { return query_; }
    std::string Transcript() const { return transcript_; }
    float Accuracy() const { return ((float)(Matches())) / Length(); }
    int Matches() const { return Count('M'); }
    int Errors() const { return Length() - Matches(); }
    int Mismatches() const { return Count('R'); }
    int Insertions() const { return Count('I'); }
    int Deletions() const { return Count('D'); }
    int Length() const { return (int)target_.length(); }

    // NULL if the transcript does not map unalnTarget onto unalnQuery; caller deletes
    static PairwiseAlignment* FromTranscript(const std::string& transcript, const std::string& unalnTarget,
                                             const std::string& unalnQuery)
    {
        std::string alnTarget, alnQuery;
        const int tLen = (int)unalnTarget.length(), qLen = (int)unalnQuery.length();
        int tPos = 0, qPos = 0;
        for (char x : transcript) {
            if (tPos > tLen || qPos > qLen) return NULL;
            const char t = (tPos < tLen ? unalnTarget[tPos] : '\0');
            const char q = (qPos < qLen ? unalnQuery[qPos] : '\0');
            switch (x) {
                case 'M':
                case 'R':
                    if ((t == q) != (x == 'M')) return NULL;
                    alnTarget.push_back(t);
                    alnQuery.push_back(q);
                    tPos++;
                    qPos++;
                    break;
                case 'I':
                    alnTarget.push_back('-');
                    alnQuery.push_back(q);
                    qPos++;
                    break;
                case 'D':
                    alnTarget.push_back(t);
                    alnQuery.push_back('-');
                    tPos++;
                    break;
                default:
                    return NULL;
            }
        }
        if (tPos != tLen || qPos != qLen) return NULL;
        return new PairwiseAlignment(alnTarget, alnQuery);
    }

private:
    int Count(char c) const { return (int)std::count(transcript_.begin(), transcript_.end(), c); }
    std::string target_, query_, transcript_;
};

// These return an array of target length + 1 with indices into the query string
inline std::vector<int> TargetToQueryPositions(const std::string& transcript)
{
    std::vector<int> ntp;
    int queryPos = 0;
    for (char c : transcript) {
        if (c == 'M' || c == 'R') {
            ntp.push_back(queryPos);
            queryPos++;
        } else if (c == 'D') {
            ntp.push_back(queryPos);
        } else if (c == 'I') {
            queryPos++;
        } else {
            throw InvalidInputError("not a transcript character");
        }
    }
    ntp.push_back(queryPos);
    return ntp;
}

inline std::vector<int> TargetToQueryPositions(const PairwiseAlignment& aln)
{
    return TargetToQueryPositions(aln.Transcript());
}

namespace detail {

struct AlignOutput {
    std::vector<PairwiseAlignment*> alignments;   // caller deletes
    std::vector<int> intScores;                   // Align: Score(I, J)
    std::vector<float> floatScores;               // affine: max(M, GAP)(I, J)
    std::vector<pbccs_align_band_info> bandInfo;  // with a band: what became of each pair
};

// (target, query) pairs through pbccs_align_batch.  The refusals the reference makes (and the ones it should)
// are thrown before the engine is touched.
inline AlignOutput RunAlign(pbccs_align_params p, const std::vector<std::pair<std::string, std::string>>& pairs,
                            BandOptions band = BandOptions::Off())
{
    if (band.Mode == PBCCS_BAND_WIDTH && band.W < 0) throw InvalidInputError("band half-width must be >= 0");
    if (p.kind == PBCCS_ALIGN_NW && p.mode != PBCCS_POA_GLOBAL)
        throw UnsupportedFeatureError("Only GLOBAL alignment supported at present");
    if (p.kind != PBCCS_ALIGN_NW &&
        !(std::isfinite(p.match_score) && std::isfinite(p.mismatch_score) && std::isfinite(p.gap_open) &&
          std::isfinite(p.gap_extend) && std::isfinite(p.partial_match_score)))
        throw InvalidInputError("affine alignment parameters must be finite");
    const int n = (int)pairs.size();
    std::vector<pbccs_align_pair> in(n);
    std::vector<pbccs_align_result> out(n);
    std::vector<std::string> buf(n);
    for (int k = 0; k < n; ++k) {
        in[k] = pbccs_align_pair{pairs[k].first.data(), (int)pairs[k].first.size(), pairs[k].second.data(),
                                 (int)pairs[k].second.size()};
        buf[k].resize(pairs[k].first.size() + pairs[k].second.size() + 1);
        out[k] = pbccs_align_result{&buf[k][0], (int)buf[k].size() - 1, 0, 0, 0.f, 0};
    }
    AlignOutput r;
    if (n == 0) return r;
    if (band.Mode == PBCCS_BAND_OFF) {
        Check(pbccs_align_batch(DefaultEngine(), &p, in.data(), n, out.data()));
    } else {
        const pbccs_align_band b{band.Mode, band.W};
        r.bandInfo.resize(n);
        Check(pbccs_align_batch_ex(DefaultEngine(), &p, in.data(), n, out.data(), &b, r.bandInfo.data()));
    }
    for (int k = 0; k < n; ++k) {
        PairwiseAlignment* a =
            PairwiseAlignment::FromTranscript(buf[k].substr(0, out[k].len), pairs[k].first, pairs[k].second);
        if (!a) {
            for (PairwiseAlignment* x : r.alignments) delete x;
            throw DeviceError("the device returned a transcript that does not map the target onto the query");
        }
        r.alignments.push_back(a);
        r.intScores.push_back(out[k].score_i);
        r.floatScores.push_back(out[k].score_f);
    }
    return r;
}

inline pbccs_align_params NwParams(const AlignConfig& c)
{
    return pbccs_align_params{PBCCS_ALIGN_NW, (int)c.Mode,      c.Params.Match, c.Params.Mismatch,
                              c.Params.Insert, c.Params.Delete, 0.f,            0.f,
                              0.f,             0.f,             0.f};
}

inline pbccs_align_params AffineParams(int kind, const AffineAlignmentParams& a)
{
    return pbccs_align_params{kind, PBCCS_POA_GLOBAL, 0, 0, 0, 0, a.MatchScore, a.MismatchScore, a.GapOpen, a.GapExtend,
                              a.PartialMatchScore};
}

}  // namespace detail

inline PairwiseAlignment* Align(const std::string& target, const std::string& query, int* score,
                                AlignConfig config = AlignConfig::Default(), BandOptions band = BandOptions::Off())
{
    detail::AlignOutput r = detail::RunAlign(detail::NwParams(config), {{target, query}}, band);
    if (score != NULL) *score = r.intScores[0];
    return r.alignments[0];
}

inline PairwiseAlignment* Align(const std::string& target, const std::string& query,
                                AlignConfig config = AlignConfig::Default(), BandOptions band = BandOptions::Off())
{
    return Align(target, query, NULL, config, band);
}

inline PairwiseAlignment* AlignAffine(const std::string& target, const std::string& query,
                                      AffineAlignmentParams params = DefaultAffineAlignmentParams(),
                                      BandOptions band = BandOptions::Off())
{
    return detail::RunAlign(detail::AffineParams(PBCCS_ALIGN_AFFINE, params), {{target, query}}, band).alignments[0];
}

inline PairwiseAlignment* AlignAffineIupac(const std::string& target, const std::string& query,
                                           AffineAlignmentParams params = IupacAwareAffineAlignmentParams(),
                                           BandOptions band = BandOptions::Off())
{
    return detail::RunAlign(detail::AffineParams(PBCCS_ALIGN_AFFINE_IUPAC, params), {{target, query}}, band)
        .alignments[0];
}

// The vector forms: every (target, query) pair in one device call, results in input order; caller deletes.
// scores (optional) receives Score(I, J) per pair; with a band, info (optional) receives what became of each pair.
inline std::vector<PairwiseAlignment*> AlignBatch(const std::vector<std::pair<std::string, std::string>>& pairs,
                                                  AlignConfig config = AlignConfig::Default(),
                                                  std::vector<int>* scores = NULL,
                                                  BandOptions band = BandOptions::Off(),
                                                  std::vector<pbccs_align_band_info>* info = NULL)
{
    detail::AlignOutput r = detail::RunAlign(detail::NwParams(config), pairs, band);
    if (scores) *scores = r.intScores;
    if (info) *info = r.bandInfo;
    return r.alignments;
}

inline std::vector<PairwiseAlignment*> AlignAffineBatch(const std::vector<std::pair<std::string, std::string>>& pairs,
                                                        AffineAlignmentParams params = DefaultAffineAlignmentParams(),
                                                        BandOptions band = BandOptions::Off())
{
    return detail::RunAlign(detail::AffineParams(PBCCS_ALIGN_AFFINE, params), pairs, band).alignments;
}

inline std::vector<PairwiseAlignment*> AlignAffineIupacBatch(
    const std::vector<std::pair<std::string, std::string>>& pairs,
    AffineAlignmentParams params = IupacAwareAffineAlignmentParams(), BandOptions band = BandOptions::Off())
{
    return detail::RunAlign(detail::AffineParams(PBCCS_ALIGN_AFFINE_IUPAC, params), pairs, band).alignments;
}

}  // namespace ConsensusCore

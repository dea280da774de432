// tests/cpp/align_driver.cpp -- a ConsensusCore Align/ caller written against include/pbccs_amd/Align.hpp only.
//
// Without arguments: the host-only known answers (PairwiseAlignment, FromTranscript, TargetToQueryPositions, the
// refusals that come before the engine is touched); prints "known answers ok".  No device is needed.
// With a case file: aligns its pairs on the device and prints one "aln <transcript>. <score>" line per pair
// (the dot keeps an empty transcript a word; score: the int for Align; affine kinds print no score, as the reference
// returns none), first through the vector form, then "one <transcript>." for the first pair through the single-pair
// call.
// Case file: line 1 "<kind> <params...>" (kind 0: Match Mismatch Insert Delete; kinds 1, 2: MatchScore MismatchScore
// GapOpen GapExtend PartialMatchScore as hex floats), line 2 n, then n lines "<target> <query>" ("." = empty).
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iostream>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include <pbccs_amd/Align.hpp>

using namespace ConsensusCore;  // NOLINT

#define REQUIRE(c)                                                        \
    do {                                                                  \
        if (!(c)) {                                                       \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);    \
            return 1;                                                     \
        }                                                                 \
    } while (0)

static int KnownAnswers()
{
    {
        PairwiseAlignment a("GATC", "GA-C");
        REQUIRE(a.Target() == "GATC" && a.Query() == "GA-C" && a.Length() == 4 && a.Matches() == 3);
        REQUIRE(a.Deletions() == 1 && a.Mismatches() == 0 && a.Insertions() == 0 && a.Errors() == 1);
        REQUIRE(a.Accuracy() == 0.75f && a.Transcript() == "MMDM");
        PairwiseAlignment a2("GATTA-CA", "CA-TAACA");
        REQUIRE(a2.Transcript() == "RMDMMIMM" && a2.Accuracy() == 5.f / 8);
        REQUIRE(a2.Mismatches() == 1 && a2.Deletions() == 1 && a2.Insertions() == 1 && a2.Matches() == 5);
        REQUIRE((TargetToQueryPositions(a2) == std::vector<int>{0, 1, 2, 2, 3, 5, 6, 7}));
    }
    {
        bool threw = false;
        try {
            PairwiseAlignment bad("GATC", "GAC");
        } catch (const InvalidInputError&) {
            threw = true;
        }
        REQUIRE(threw);
        threw = false;
        try {
            PairwiseAlignment bad("GA-C", "GA-C");
        } catch (const InvalidInputError&) {
            threw = true;
        }
        REQUIRE(threw);
    }
    REQUIRE((TargetToQueryPositions("MMM") == std::vector<int>{0, 1, 2, 3}));
    REQUIRE((TargetToQueryPositions("DMM") == std::vector<int>{0, 0, 1, 2}));
    REQUIRE((TargetToQueryPositions("MDM") == std::vector<int>{0, 1, 1, 2}));
    REQUIRE((TargetToQueryPositions("MMD") == std::vector<int>{0, 1, 2, 2}));
    REQUIRE((TargetToQueryPositions("IMM") == std::vector<int>{1, 2, 3}));
    REQUIRE((TargetToQueryPositions("MIM") == std::vector<int>{0, 2, 3}));
    REQUIRE((TargetToQueryPositions("MMI") == std::vector<int>{0, 1, 3}));
    REQUIRE((TargetToQueryPositions("MRM") == std::vector<int>{0, 1, 2, 3}));
    REQUIRE((TargetToQueryPositions("MDIM") == std::vector<int>{0, 1, 2, 3}));
    REQUIRE((TargetToQueryPositions("MIDM") == std::vector<int>{0, 2, 2, 3}));
    {
        std::unique_ptr<PairwiseAlignment> a(PairwiseAlignment::FromTranscript("RMDMMIMM", "GATTACA", "CATAACA"));
        REQUIRE(a && a->Target() == "GATTA-CA" && a->Query() == "CA-TAACA");
        REQUIRE(PairwiseAlignment::FromTranscript("MMMM", "GATT", "GAT") == NULL);
        REQUIRE(PairwiseAlignment::FromTranscript("MMM", "GATT", "GAT") == NULL);
        REQUIRE(PairwiseAlignment::FromTranscript("MMRM", "GATT", "GATT") == NULL);
        REQUIRE(PairwiseAlignment::FromTranscript("MMMM", "GATT", "GACT") == NULL);
        REQUIRE(PairwiseAlignment::FromTranscript("MMXM", "GATT", "GATT") == NULL);
    }
    {
        const AlignConfig c = AlignConfig::Default();
        REQUIRE(c.Mode == GLOBAL && c.Params.Match == 0 && c.Params.Mismatch == -1 && c.Params.Insert == -1 &&
                c.Params.Delete == -1);
        const AffineAlignmentParams d = DefaultAffineAlignmentParams(), u = IupacAwareAffineAlignmentParams();
        REQUIRE(d.MatchScore == 0 && d.MismatchScore == -1 && d.GapOpen == -1 && d.GapExtend == -0.5f &&
                d.PartialMatchScore == 0);
        REQUIRE(u.PartialMatchScore == -0.25f && u.GapExtend == -0.5f);
    }
    // refused before any engine exists: these throw the reference's errors even without a device
    {
        bool threw = false;
        try {
            Align("GATT", "GAT", AlignConfig(AlignParams::Default(), SEMIGLOBAL));
        } catch (const UnsupportedFeatureError&) {
            threw = true;
        }
        REQUIRE(threw);
        threw = false;
        try {
            AlignAffine("GATT", "GAT", AffineAlignmentParams(0, -1, -1, std::numeric_limits<float>::infinity(), 0));
        } catch (const InvalidInputError&) {
            threw = true;
        }
        REQUIRE(threw);
    }
    std::printf("known answers ok\n");
    return 0;
}

static std::string Field(const std::string& s) { return s == "." ? std::string() : s; }

int main(int argc, char** argv)
{
    if (argc < 2) return KnownAnswers();
    std::ifstream in(argv[1]);
    int kind = 0, n = 0;
    in >> kind;
    int ip[4] = {0, -1, -1, -1};
    float fp[5] = {0, 0, 0, 0, 0};
    if (kind == 0) {
        for (int& v : ip) in >> v;
    } else {
        for (float& v : fp) {
            std::string w;
            in >> w;
            v = std::strtof(w.c_str(), NULL);
        }
    }
    in >> n;
    std::vector<std::pair<std::string, std::string>> pairs(n);
    for (auto& p : pairs) {
        std::string t, q;
        in >> t >> q;
        p = {Field(t), Field(q)};
    }
    if (!in) {
        std::fprintf(stderr, "bad case file\n");
        return 2;
    }
    try {
        std::vector<PairwiseAlignment*> alns;
        std::vector<int> scores;
        std::unique_ptr<PairwiseAlignment> one;
        const AffineAlignmentParams ap(fp[0], fp[1], fp[2], fp[3], fp[4]);
        if (kind == 0) {
            const AlignConfig cfg(AlignParams(ip[0], ip[1], ip[2], ip[3]), GLOBAL);
            alns = AlignBatch(pairs, cfg, &scores);
            if (n) one.reset(Align(pairs[0].first, pairs[0].second, cfg));
        } else if (kind == 1) {
            alns = AlignAffineBatch(pairs, ap);
            if (n) one.reset(AlignAffine(pairs[0].first, pairs[0].second, ap));
        } else {
            alns = AlignAffineIupacBatch(pairs, ap);
            if (n) one.reset(AlignAffineIupac(pairs[0].first, pairs[0].second, ap));
        }
        for (int k = 0; k < n; ++k) {
            if (kind == 0) std::printf("aln %s. %d\n", alns[k]->Transcript().c_str(), scores[k]);
            else std::printf("aln %s.\n", alns[k]->Transcript().c_str());
            delete alns[k];
        }
        if (one) std::printf("one %s.\n", one->Transcript().c_str());
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}

// pbccs_amd/csrc/arrow_model.hpp -- host-side Arrow model and mutation bookkeeping.
//
// Cheap per-ZMW work that stays on the host CPU next to the GPU engine: the SNR -> transition
// parameter model, z-score expectations, mutation ordering/enumeration for the neighbourhood
// rounds, and real template edits with coordinate remapping.  The DP work runs on the GPU.
#pragma once

#include <cstdint>
#include <string>
#include <utility>
#include <vector>

namespace pbccs {

constexpr double kMismatchProbability = 0.00505052456472967;   // ArrowConfig.hpp:54 (MISMATCH_PROBABILITY)
constexpr double kMinFavorableScoreDiff = 0.04;                // MultiReadMutationScorer.cpp:56

struct TransParams {
    double match = 0.0, stick = 0.0, branch = 0.0, deletion = 0.0;
};

// ContextParameterProvider::GetTransitionParameters (ContextParameterProvider.cpp:66-110) for the
// 8 contexts; slot order AA CC GG TT NA NC NG NT.
void transition_table(const double snr[4], TransParams out[8]);
// Device layout: 9 slots x {Match, Stick, Branch, Deletion, Stick / 3.0}; slot 8 = zeros.
void device_context_table(const TransParams t[8], double out[45]);

// ExpectedContextLL (Expectations.hpp:12-40)
std::pair<double, double> expected_context_ll(const TransParams& p, double eps);

// A single-base mutation (Mutation.hpp); ordered as in Mutation-inl.hpp:179-186.
struct Mutation {
    int type = 2;    // 0 insertion, 1 deletion, 2 substitution
    int start = 0;
    int end = 1;
    char base = 'A';   // '-' for deletions
    int LengthDiff() const { return type == 0 ? 1 : (type == 1 ? -1 : 0); }
    bool operator<(const Mutation& o) const
    {
        if (start != o.start) return start < o.start;
        if (end != o.end) return end < o.end;
        if (type != o.type) return type < o.type;
        const std::string a = type == 1 ? std::string() : std::string(1, base);
        const std::string b = o.type == 1 ? std::string() : std::string(1, o.base);
        return a < b;
    }
    bool operator==(const Mutation& o) const
    {
        return type == o.type && start == o.start && end == o.end && (type == 1 || base == o.base);
    }
    static Mutation Make(int type, int pos, char base)
    {
        Mutation m;
        m.type = type;
        m.start = pos;
        m.end = type == 0 ? pos : pos + 1;
        m.base = type == 1 ? '-' : base;
        return m;
    }
};

int mutation_code(const Mutation& m);
Mutation mutation_from_code(int code);

bool is_acgt(const std::string& s);
std::string reverse_complement(const std::string& s);

// Count of UniqueSingleBaseMutationEnumerator::Mutations() for an ACGT template.
long long unique_mutation_count(const std::string& tpl);
// UniqueSingleBaseMutationEnumerator::Mutations(b, e) (MutationEnumerator.cpp:114-145), as codes.
void unique_mutations(const std::string& tpl, int b, int e, std::vector<int>* codes);
// Per-base rich QVs of one template, by mutation type: the QVs of the partial sums of
// ConsensusQVs' sum over a position's substitutions, insertions and deletion, and the base of its best-scoring
// substitution / insertion.  (File formats name by error type: ins* is PacBio's DeletionQV / DeletionTag, del its
// InsertionQV.)
struct RichQVs {
    std::vector<int> subQv, insQv, delQv;
    std::string subTag, insTag;
};
// UniqueNearbyMutations (MutationEnumerator-inl.hpp:50-68): std::set<Mutation> order, as codes.
void nearby_mutations(const std::string& tpl, const std::vector<int>& centerStarts, int nbhd,
                      std::vector<int>* codes);

// ApplyMutations (Mutation.cpp:115-128) and TargetToQueryPositions (Mutation.cpp:193-197).
// Returns false when an edit is out of range (the reference would throw).
bool apply_mutations(const std::string& tpl, std::vector<Mutation> muts, std::string* out, std::vector<int>* mtp);

// A mutation of any width (Mutation.hpp): type, [start, end) and the new bases.  Invariants as in
// Mutation-inl.hpp:102-115, order as in Mutation-inl.hpp:179-186 (start, end, type, new bases).
struct MutationEx {
    int type = 2;    // 0 insertion, 1 deletion, 2 substitution
    int start = 0;
    int end = 1;
    std::string bases;   // empty for deletions
    bool Valid() const
    {
        if (type == 0) return start == end && !bases.empty();
        if (type == 1) return start < end && bases.empty();
        if (type == 2) return start < end && (int)bases.size() == end - start;
        return false;
    }
    int LengthDiff() const { return type == 0 ? (int)bases.size() : (type == 1 ? start - end : 0); }
    bool operator<(const MutationEx& o) const
    {
        if (start != o.start) return start < o.start;
        if (end != o.end) return end < o.end;
        if (type != o.type) return type < o.type;
        return bases < o.bases;
    }
    bool operator==(const MutationEx& o) const
    {
        return type == o.type && start == o.start && end == o.end && bases == o.bases;
    }
};

// ApplyMutations (Mutation.cpp:115-128), MutationsToTranscript (:130-171) and TargetToQueryPositions
// (:193-197) for any width.  Returns false for an invalid mutation or an edit outside the template.
bool apply_mutations_ex(const std::string& tpl, std::vector<MutationEx> muts, std::string* out, std::vector<int>* mtp);

// RepeatMutationEnumerator::Mutations(begin, end) (MutationEnumerator.cpp:161-218): an insertion and a
// deletion of one repeat element at the start of every run of >= minRepeatElements elements.
void repeat_mutations(const std::string& tpl, int repeatLength, int minRepeatElements, int begin, int end,
                      std::vector<MutationEx>* out);
// UniqueNearbyMutations (MutationEnumerator-inl.hpp:50-68) over the repeat enumerator: the union of
// Mutations(c - nbhd, c + nbhd) over the centres, in std::set<Mutation> order.
void nearby_repeat_mutations(const std::string& tpl, int repeatLength, int minRepeatElements,
                             const std::vector<int>& centerStarts, int nbhd, std::vector<MutationEx>* out);

// Arrow's view of a mutation of any width from one read: ReadScoresMutation
// (Arrow/MultiReadMutationScorer.cpp:70-80), then OrientedMutation (:93-139) -- the clip to the read's window for
// mutations wider than one template base, then the strand -- in the coordinates of the window [ts, te).
struct OrientedEx {
    bool scores = false;   // the read scores the mutation
    int type = 2;
    int os = 0, oe = 0;    // the window columns [os, oe) replaced, on the read's strand
    std::string bases;     // the new bases on the read's strand (clipped for a substitution)
    int LengthDiff() const { return type == 0 ? (int)bases.size() : (type == 1 ? os - oe : 0); }
};
OrientedEx orient_mutation_ex(const MutationEx& m, int strand, int ts, int te);
// Extension columns ScoreMutation (Arrow/MutationScorer.cpp:185-267) needs for an oriented mutation in a window of J
// columns: 1 + |bases| in the middle (2 for a deletion), to the window's end or its start in the edge cases, 0 for
// the whole-window refill (it takes a band from scratch, not the extension buffer), -1 when the mutated window
// would be empty.
int wide_columns_needed(const OrientedEx& o, int J);

// ProbabilityToQV (Consensus-inl.hpp:130-138)
int probability_to_qv(double p);

// ---- diploid site calling (Arrow/Diploid.cpp:94-241; Quiver/Diploid.cpp differs only in casts) ------------
// A site's scores: nReads x 9 floats, row-major, columns Substitution(p, ACGT), Insertion(p, ACGT), Deletion(p)
// -- the order LENGTH_DIFFS (Diploid.cpp:99) assumes.
constexpr int kSiteAlleles = 9;
constexpr int kSitePairs = 12;   // allele pairs g0 < g1 of equal length difference: 6 substitution + 6 insertion
struct DiploidCall {
    int allele0 = -1, allele1 = -1;
    float logBayesFactor = 0.0f;
};
// IsSiteHeterozygous (Diploid.cpp:219-239) in float with the reference's operation order and the host libm.
// Returns logBF - logPriorRatio > 0; alleleForRead (nReads entries, may be NULL) receives AssignReadsToAlleles
// (:204-213).  The call is filled either way.
bool is_site_heterozygous(const float* siteScores, int nReads, float logPriorRatio, DiploidCall* call,
                          int* alleleForRead);
struct DiploidSiteH {   // a reported DiploidSite (Diploid.hpp), AlleleForRead kept beside it
    int position, allele0, allele1;
    float logBayesFactor;
};
struct DiploidStats {   // the device screen's work (pbccs_diploid_stats)
    long long sitesScreened = 0, sitesSentToHost = 0, sitesReported = 0;
};

}  // namespace pbccs

// include/pbccs_amd/ConsensusCore.hpp -- header-only C++ facade with ConsensusCore's class names over
// the C ABI in include/pbccs_amd.h, so that pbccs' per-ZMW driver (include/pacbio/ccs/Consensus.h:436-512)
// compiles against the MI355X engine by swapping its ConsensusCore includes for this header.
//
// Mirrored surface (reference file:line):
//   Arrow::SNR, ContextParameters            Arrow/ContextParameterProvider.hpp, ContextParameters.hpp
//   Arrow::BandingOptions, Arrow::ArrowConfig Arrow/ArrowConfig.hpp:63-128
//   ArrowSequenceFeatures, ArrowRead, MappedArrowRead, StrandEnum   Features.hpp, Read.hpp:47-97
//   Mutation, MutationType                    Mutation.hpp:50-129
//   Arrow::AddReadResult, ArrowMultiReadMutationScorer   Arrow/MultiReadMutationScorer.hpp:60-284
//   RefineOptions, RefineConsensus, ConsensusQVs          Consensus.hpp:48-79
// The Quiver family's classes are in pbccs_amd/Quiver.hpp (as ConsensusCore keeps them under Quiver/).
// Errors surface as ConsensusCore-style exceptions on the C++ side (the ABI itself never throws).
#pragma once

#include <cfloat>
#include <limits>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "../pbccs_amd.h"

namespace ConsensusCore {

class InvalidInputError : public std::runtime_error {
public:
    explicit InvalidInputError(const std::string& m = "invalid input") : std::runtime_error(m) {}
};

class UnsupportedFeatureError : public std::runtime_error {
public:
    explicit UnsupportedFeatureError(const std::string& m = "unsupported feature") : std::runtime_error(m) {}
};

class DeviceError : public std::runtime_error {
public:
    explicit DeviceError(const std::string& m) : std::runtime_error(m) {}
};

namespace detail {
inline void Check(int rc)
{
    if (rc == PBCCS_OK) return;
    const std::string msg = pbccs_last_error();
    if (rc == PBCCS_EINVAL || rc == PBCCS_ERANGE) throw InvalidInputError(msg);
    throw DeviceError(msg);
}

// One engine per process and device (ccs: one device per worker process).
inline pbccs_engine* DefaultEngine(int device = 0)
{
    static pbccs_engine* eng = nullptr;
    if (!eng) Check(pbccs_engine_create(device, &eng));
    return eng;
}
}  // namespace detail

enum MutationType { INSERTION = PBCCS_INSERTION, DELETION = PBCCS_DELETION, SUBSTITUTION = PBCCS_SUBSTITUTION };
enum StrandEnum { FORWARD_STRAND = PBCCS_FORWARD_STRAND, REVERSE_STRAND = PBCCS_REVERSE_STRAND };

class Mutation {
public:
    Mutation(MutationType type, int position, char base)
        : type_(type), start_(position), end_(type == INSERTION ? position : position + 1),
          newBases_(type == DELETION ? std::string() : std::string(1, base))
    {}
    Mutation(MutationType type, int start, int end, const std::string& newBases)
        : type_(type), start_(start), end_(end), newBases_(newBases)
    {
        if (!CheckInvariants()) throw InvalidInputError();
    }
    // Mutation-inl.hpp:66-77: end from the new bases' length (an insertion's is its start), a deletion's bases dropped
    Mutation(MutationType type, int position, const std::string& newBases)
        : type_(type), start_(position),
          end_(type == INSERTION ? position : position + (int)newBases.size()),
          newBases_(type == DELETION ? std::string() : newBases)
    {
        if (!CheckInvariants()) throw InvalidInputError();
    }
    // Mutation-inl.hpp:103-115
    bool CheckInvariants() const
    {
        return (type_ == INSERTION && start_ == end_ && !newBases_.empty()) ||
               (type_ == DELETION && start_ < end_ && newBases_.empty()) ||
               (type_ == SUBSTITUTION && start_ < end_ && (int)newBases_.size() == end_ - start_);
    }
    MutationType Type() const { return type_; }
    int Start() const { return start_; }
    int End() const { return end_; }
    std::string NewBases() const { return newBases_; }
    bool IsInsertion() const { return type_ == INSERTION; }
    bool IsDeletion() const { return type_ == DELETION; }
    bool IsSubstitution() const { return type_ == SUBSTITUTION; }
    int LengthDiff() const
    {
        return type_ == INSERTION ? (int)newBases_.size() : (type_ == DELETION ? start_ - end_ : 0);
    }
    bool operator<(const Mutation& o) const
    {
        if (start_ != o.start_) return start_ < o.start_;
        if (end_ != o.end_) return end_ < o.end_;
        if (type_ != o.type_) return type_ < o.type_;
        return newBases_ < o.newBases_;
    }
    bool operator==(const Mutation& o) const
    {
        return start_ == o.start_ && end_ == o.end_ && type_ == o.type_ && newBases_ == o.newBases_;
    }
    // one base wide: the single-base ABI (pbccs_mutation) carries it
    bool IsSingleBase() const
    {
        return newBases_.size() <= 1 && end_ - start_ == (type_ == INSERTION ? 0 : 1);
    }
    // any width (the _ex entry points of either scorer family); new_bases points into this Mutation
    pbccs_mutation_ex ToCEx() const
    {
        pbccs_mutation_ex m;
        m.type = (int)type_;
        m.start = start_;
        m.end = end_;
        m.new_bases = newBases_.data();
        m.n_bases = (int)newBases_.size();
        return m;
    }
    pbccs_mutation ToC() const
    {
        if (newBases_.size() > 1) throw InvalidInputError("Only mutations of size 1 allowed");
        pbccs_mutation m;
        m.type = (int)type_;
        m.start = start_;
        m.end = end_;
        m.new_base = newBases_.empty() ? '-' : newBases_[0];
        return m;
    }

private:
    MutationType type_;
    int start_, end_;
    std::string newBases_;
};

struct ArrowSequenceFeatures {
    std::string Sequence;
    explicit ArrowSequenceFeatures(const std::string& seq) : Sequence(seq) {}
    int Length() const { return (int)Sequence.size(); }
};

struct ArrowRead {
    ArrowSequenceFeatures Features;
    std::string Name, Chemistry;
    ArrowRead(const ArrowSequenceFeatures& f, const std::string& name, const std::string& chem)
        : Features(f), Name(name), Chemistry(chem)
    {}
    int Length() const { return Features.Length(); }
};

struct MappedArrowRead : public ArrowRead {
    StrandEnum Strand;
    int TemplateStart, TemplateEnd;
    MappedArrowRead(const ArrowRead& r, StrandEnum strand, int ts, int te)
        : ArrowRead(r), Strand(strand), TemplateStart(ts), TemplateEnd(te)
    {}
};

struct RefineOptions {
    int MaximumIterations;
    int MutationSeparation;
    int MutationNeighborhood;
};
static const RefineOptions DefaultRefineOptions = {40, 10, 20};

namespace Arrow {

enum AddReadResult { SUCCESS = 0, ALPHABETAMISMATCH = 1, MEM_FAIL = 2, POOR_ZSCORE = 3, OTHER = 4 };
static const char* AddReadResultNames[] = {"SUCCESS", "ALPHA/BETA MISMATCH", "EXCESSIVE MEMORY USAGE",
                                           "POOR Z-SCORE", "OTHER"};

struct SNR {
    double A, C, G, T;
    SNR(double a, double c, double g, double t) : A(a), C(c), G(g), T(t) {}
};

struct ContextParameters {
    SNR snr;
    explicit ContextParameters(const SNR& s) : snr(s) {}
};

struct BandingOptions {
    double ScoreDiff;
    explicit BandingOptions(double scoreDiff) : ScoreDiff(scoreDiff)
    {
        if (scoreDiff < 0) throw InvalidInputError("ScoreDiff must be positive!");
    }
};

class ArrowConfig {
public:
    ContextParameters CtxParams;
    BandingOptions Banding;
    double FastScoreThreshold;
    double AddThreshold;
    ArrowConfig(const ContextParameters& ctx, const BandingOptions& b, double fastScoreThreshold = -12.5,
                double addThreshold = std::numeric_limits<double>::quiet_NaN())
        : CtxParams(ctx), Banding(b), FastScoreThreshold(fastScoreThreshold), AddThreshold(addThreshold)
    {}
    pbccs_arrow_config ToC() const
    {
        pbccs_arrow_config c;
        c.snr[0] = CtxParams.snr.A;
        c.snr[1] = CtxParams.snr.C;
        c.snr[2] = CtxParams.snr.G;
        c.snr[3] = CtxParams.snr.T;
        c.score_diff = Banding.ScoreDiff;
        c.fast_score_threshold = FastScoreThreshold;
        c.add_threshold = AddThreshold;
        return c;
    }
};

// The strand-discordance screen (no reference twin: the reference stops at the Directional TODO,
// include/pacbio/ccs/Consensus.h:94-109).  StrandSums: the sums of Scores(m, 0) over the active forward / reverse reads
// that score m, in AddRead order, and how many reads entered each.  StrandSite: a template position with a
// single-base mutation one strand favours by more than minScore while the other opposes it by more than minScore.
struct StrandSums {
    double SumFwd, SumRev;
    int NFwd, NRev;
};
struct StrandSite {
    int Position;
    MutationType Type;
    char Base;   // '-' for a deletion
    double SumFwd, SumRev;
    Mutation ToMutation() const { return Mutation(Type, Position, Base); }
};

// DiploidSite / IsSiteHeterozygous (Arrow/Diploid.hpp:47-62, Diploid.cpp:94-241).  Position is this facade's
// addition: the template position, set by the scorers' DiploidSites (-1 from IsSiteHeterozygous).
struct DiploidSite {
    int Allele0;
    int Allele1;
    float LogBayesFactor;
    std::vector<int> AlleleForRead;
    int Position;
    DiploidSite(int allele0, int allele1, float logBayesFactor, std::vector<int> alleleForRead)
        : Allele0(allele0), Allele1(allele1), LogBayesFactor(logBayesFactor), AlleleForRead(std::move(alleleForRead)),
          Position(-1)
    {}
};

// siteScores: dim1 reads x dim2 (= 9) alleles, row-major.  NULL when the site is not heterozygous; otherwise a
// new DiploidSite the caller owns, as in the reference.
inline DiploidSite* IsSiteHeterozygous(const float* siteScores, int dim1, int dim2, float logPriorRatio)
{
    int isHet = 0;
    pbccs_diploid_site site;
    std::vector<int> alleleForRead(dim1 > 0 ? dim1 : 0);
    detail::Check(pbccs_is_site_heterozygous(siteScores, dim1, dim2, logPriorRatio, &isHet, &site, alleleForRead.data()));
    if (!isHet) return nullptr;
    return new DiploidSite(site.allele0, site.allele1, site.log_bayes_factor, alleleForRead);
}

namespace diploid {
// the scorers' SiteScores / DiploidSites over either family's C entry points
template <class H, class F>
std::vector<float> SiteScores(H* handle, F call, int nReads, int begin, int end)
{
    std::vector<float> out((size_t)(end > begin ? end - begin : 0) * (size_t)nReads * 9);
    long long n = 0;
    detail::Check(call(handle, begin, end, out.data(), (long long)out.size(), &n));
    return out;
}
template <class H, class F>
std::vector<DiploidSite> DiploidSites(H* handle, F call, int nReads, int begin, int end, float logPriorRatio,
                                      bool hostAll)
{
    const int cap = end > begin ? end - begin : 0;
    std::vector<pbccs_diploid_site> sites((size_t)cap + 1);
    std::vector<int> afr((size_t)cap * (size_t)nReads + 1);
    int n = 0;
    detail::Check(call(handle, begin, end, logPriorRatio, hostAll ? 1 : 0, sites.data(), cap, &n, afr.data()));
    std::vector<DiploidSite> out;
    for (int k = 0; k < n; ++k) {
        out.emplace_back(sites[k].allele0, sites[k].allele1, sites[k].log_bayes_factor,
                         std::vector<int>(afr.begin() + (size_t)k * nReads, afr.begin() + (size_t)(k + 1) * nReads));
        out.back().Position = sites[k].position;
    }
    return out;
}
}  // namespace diploid

class ArrowMultiReadMutationScorer {
public:
    ArrowMultiReadMutationScorer(const ArrowConfig& config, const std::string& tpl)
        : config_(config), handle_(nullptr)
    {
        const pbccs_arrow_config c = config.ToC();
        detail::Check(pbccs_scorer_create(detail::DefaultEngine(), &c, tpl.data(), (int)tpl.size(), &handle_));
    }
    ~ArrowMultiReadMutationScorer()
    {
        if (handle_) pbccs_scorer_destroy(handle_);
    }
    ArrowMultiReadMutationScorer(ArrowMultiReadMutationScorer&& o) noexcept : config_(o.config_), handle_(o.handle_)
    {
        o.handle_ = nullptr;
    }
    ArrowMultiReadMutationScorer(const ArrowMultiReadMutationScorer&) = delete;
    ArrowMultiReadMutationScorer& operator=(const ArrowMultiReadMutationScorer&) = delete;

    AddReadResult AddRead(const MappedArrowRead& mr, double threshold)
    {
        int res = 0;
        const std::string& s = mr.Features.Sequence;
        detail::Check(pbccs_scorer_add_read(handle_, s.data(), (int)s.size(), (int)mr.Strand, mr.TemplateStart,
                                            mr.TemplateEnd, threshold, &res));
        return (AddReadResult)res;
    }
    AddReadResult AddRead(const MappedArrowRead& mr) { return AddRead(mr, config_.AddThreshold); }

    // A mutation wider than one base goes to the pbccs_scorer_*_ex calls (k_score_wide); the
    // reference's scorer throws for it (Arrow/MutationScorer.cpp:181-183).  Single-base ones stay where they were.
    double Score(const Mutation& m, double fastScoreThreshold = -DBL_MAX)
    {
        double v = 0.0;
        if (!m.IsSingleBase()) {
            const pbccs_mutation_ex x = m.ToCEx();
            detail::Check(pbccs_scorer_score_many_ex(handle_, &x, 1, fastScoreThreshold, &v));
            return v;
        }
        const pbccs_mutation c = m.ToC();
        detail::Check(pbccs_scorer_score(handle_, &c, fastScoreThreshold, &v));
        return v;
    }
    double Score(MutationType t, int position, char base) { return Score(Mutation(t, position, base)); }
    double FastScore(const Mutation& m) { return Score(m, config_.FastScoreThreshold); }
    std::vector<double> Scores(const Mutation& m, double unscoredValue = 0.0)
    {
        std::vector<double> out(NumReads());
        if (!m.IsSingleBase()) {
            const pbccs_mutation_ex x = m.ToCEx();
            detail::Check(pbccs_scorer_scores_ex(handle_, &x, unscoredValue, out.data()));
            return out;
        }
        const pbccs_mutation c = m.ToC();
        detail::Check(pbccs_scorer_scores(handle_, &c, unscoredValue, out.data()));
        return out;
    }
    bool IsFavorable(const Mutation& m) { return Score(m) > 0.04; }
    bool FastIsFavorable(const Mutation& m) { return FastScore(m) > 0.04; }
    void ApplyMutations(const std::vector<Mutation>& muts)
    {
        bool wide = false;
        for (const Mutation& m : muts) wide = wide || !m.IsSingleBase();
        if (wide) {
            std::vector<pbccs_mutation_ex> x;
            for (const Mutation& m : muts) x.push_back(m.ToCEx());
            detail::Check(pbccs_scorer_apply_mutations_ex(handle_, x.data(), (int)x.size()));
            return;
        }
        std::vector<pbccs_mutation> c;
        for (const Mutation& m : muts) c.push_back(m.ToC());
        detail::Check(pbccs_scorer_apply_mutations(handle_, c.data(), (int)c.size()));
    }
    std::string Template(StrandEnum strand = FORWARD_STRAND) const
    {
        int len = 0;
        std::string out(TemplateLength() + 1, '\0');
        detail::Check(pbccs_scorer_template(handle_, (int)strand, &out[0], (int)out.size(), &len));
        out.resize(len);
        return out;
    }
    int TemplateLength() const { return pbccs_scorer_template_length(handle_); }
    int NumReads() const { return pbccs_scorer_num_reads(handle_); }
    double BaselineScore() const
    {
        double v = 0.0;
        detail::Check(pbccs_scorer_baseline_score(handle_, &v));
        return v;
    }
    std::vector<double> BaselineScores() const
    {
        std::vector<double> out(NumReads());
        int n = 0;
        detail::Check(pbccs_scorer_baseline_scores(handle_, out.data(), (int)out.size(), &n));
        out.resize(n);
        return out;
    }
    std::pair<std::pair<double, double>, std::vector<double>> ZScores() const
    {
        double zg = 0.0, za = 0.0;
        std::vector<double> zs(NumReads());
        detail::Check(pbccs_scorer_zscores(handle_, &zg, &za, zs.data()));
        return std::make_pair(std::make_pair(zg, za), zs);
    }
    std::vector<int> NumFlipFlops() const
    {
        std::vector<int> out(NumReads());
        detail::Check(pbccs_scorer_num_flipflops(handle_, out.data()));
        return out;
    }
    // The site tensor of template positions [begin, end) (end < 0: the template's end): [site][read][9] floats,
    // a site's slice being what IsSiteHeterozygous takes; and IsSiteHeterozygous at each of those positions
    // (the heterozygous sites by ascending Position).
    std::vector<float> SiteScores(int begin = 0, int end = -1)
    {
        return diploid::SiteScores(handle_, pbccs_scorer_site_scores, NumReads(), begin, end < 0 ? TemplateLength() : end);
    }
    std::vector<DiploidSite> DiploidSites(float logPriorRatio, int begin = 0, int end = -1, bool hostAll = false)
    {
        return diploid::DiploidSites(handle_, pbccs_scorer_diploid_sites, NumReads(), begin,
                                    end < 0 ? TemplateLength() : end, logPriorRatio, hostAll);
    }
    // Per-strand sums of single-base mutations (k_strand_sums): bit-equal to summing Scores(m, 0) per strand.
    std::vector<StrandSums> StrandScores(const std::vector<Mutation>& muts)
    {
        const size_t n = muts.size();
        std::vector<pbccs_mutation> c;
        for (const Mutation& m : muts) c.push_back(m.ToC());
        std::vector<double> sf(n), sr(n);
        std::vector<int> nf(n), nr(n);
        detail::Check(pbccs_scorer_strand_scores(handle_, c.data(), (int)n, sf.data(), sr.data(), nf.data(), nr.data()));
        std::vector<StrandSums> out(n);
        for (size_t i = 0; i < n; ++i) out[i] = StrandSums{sf[i], sr[i], nf[i], nr[i]};
        return out;
    }
    // The strand-discordant sites of the current template, by ascending Position (the ConsensusQVs sweep, then
    // k_strand_sums and k_strand_sites).
    std::vector<StrandSite> StrandSites(double minScore = 12.5, int minReads = 2)
    {
        pbccs_strand_options o;
        pbccs_strand_options_default(&o);
        o.min_score = minScore;
        o.min_reads = minReads;
        const int cap = TemplateLength() > 0 ? TemplateLength() : 1;
        std::vector<int> pos(cap), type(cap);
        std::vector<char> base(cap);
        std::vector<double> sf(cap), sr(cap);
        int n = 0;
        detail::Check(pbccs_scorer_strand_sites(handle_, &o, pos.data(), type.data(), base.data(), sf.data(), sr.data(),
                                                cap, &n));
        std::vector<StrandSite> out;
        for (int k = 0; k < n; ++k) out.push_back(StrandSite{pos[k], (MutationType)type[k], base[k], sf[k], sr[k]});
        return out;
    }
    pbccs_scorer* Handle() { return handle_; }

private:
    ArrowConfig config_;
    pbccs_scorer* handle_;
};

}  // namespace Arrow

// RefineConsensus / ConsensusQVs (Consensus.hpp:63-79)
inline bool RefineConsensus(Arrow::ArrowMultiReadMutationScorer& mms, size_t* nTested, size_t* nApplied,
                            const RefineOptions& opts = DefaultRefineOptions)
{
    pbccs_refine_options o;
    o.max_iterations = opts.MaximumIterations;
    o.mutation_separation = opts.MutationSeparation;
    o.mutation_neighborhood = opts.MutationNeighborhood;
    long long nt = 0, na = 0;
    int conv = 0;
    detail::Check(pbccs_refine_consensus(mms.Handle(), &o, &nt, &na, &conv));
    *nTested += (size_t)nt;
    *nApplied += (size_t)na;
    return conv != 0;
}

// RefineRepeats / RefineDinucleotideRepeats (Consensus.hpp:69-76) for the Arrow scorer (pbccs_refine_repeats).
// RefineRepeatOptions sets MaximumIterations = 1 and leaves the other two fields unset; DefaultRefineOptions' 10
// and 20 stand in, as for the Quiver scorers (Quiver.hpp).
inline bool RefineRepeats(Arrow::ArrowMultiReadMutationScorer& mms, int repeatLength, int minRepeatElements = 3,
                          size_t* nTested = nullptr, size_t* nApplied = nullptr, int maximumIterations = 1)
{
    pbccs_repeat_options o;
    o.repeat_length = repeatLength;
    o.min_repeat_elements = minRepeatElements;
    o.max_iterations = maximumIterations;
    o.mutation_separation = DefaultRefineOptions.MutationSeparation;
    o.mutation_neighborhood = DefaultRefineOptions.MutationNeighborhood;
    long long nt = 0, na = 0;
    int conv = 0;
    detail::Check(pbccs_refine_repeats(mms.Handle(), &o, &nt, &na, &conv));
    if (nTested) *nTested += (size_t)nt;
    if (nApplied) *nApplied += (size_t)na;
    return conv != 0;
}

inline bool RefineDinucleotideRepeats(Arrow::ArrowMultiReadMutationScorer& mms, int minDinucleotideRepeatElements = 3)
{
    return RefineRepeats(mms, 2, minDinucleotideRepeatElements);
}

inline std::vector<int> ConsensusQVs(Arrow::ArrowMultiReadMutationScorer& mms)
{
    std::vector<int> q(mms.TemplateLength());
    int n = 0;
    detail::Check(pbccs_consensus_qvs(mms.Handle(), q.data(), (int)q.size(), &n));
    q.resize(n);
    return q;
}

// Per-base rich QVs (no reference twin): ConsensusQVs' sum of a position taken apart by mutation
// type.  Qvs is ConsensusQVs(mms); SubQv / InsQv / DelQv are the QVs of the partial sums over the position's
// substitutions / insertions / deletion; Tags = (SubTag, InsTag), the base of its best-scoring substitution /
// insertion.  Names follow the mutation type; file formats name by error type, the inverse: PacBio's DeletionQV /
// DeletionTag (dq / dt) are InsQv / InsTag, InsertionQV (iq) is DelQv, sq / st are SubQv / SubTag.
struct RichConsensusQVs {
    std::vector<int> Qvs, SubQv, InsQv, DelQv;
    std::pair<std::string, std::string> Tags;   // (SubTag, InsTag)
    const std::string& SubTag() const { return Tags.first; }
    const std::string& InsTag() const { return Tags.second; }
};

namespace detail {
// shared by the Arrow and the Quiver overloads: call(qvs, rich, n) is the family's pbccs_*_consensus_qvs_rich
template <typename Call>
inline RichConsensusQVs RichQVs(int length, Call call)
{
    const size_t cap = (size_t)(length > 0 ? length : 1);
    RichConsensusQVs r;
    r.Qvs.resize(cap);
    r.SubQv.resize(cap);
    r.InsQv.resize(cap);
    r.DelQv.resize(cap);
    r.Tags.first.resize(cap);
    r.Tags.second.resize(cap);
    pbccs_rich_qvs c;
    c.sub_qv = r.SubQv.data();
    c.ins_qv = r.InsQv.data();
    c.del_qv = r.DelQv.data();
    c.sub_tag = &r.Tags.first[0];
    c.ins_tag = &r.Tags.second[0];
    c.cap = (int)cap;
    c.len = 0;
    int n = 0;
    Check(call(r.Qvs.data(), &c, &n));
    r.Qvs.resize(n);
    r.SubQv.resize(n);
    r.InsQv.resize(n);
    r.DelQv.resize(n);
    r.Tags.first.resize(n);
    r.Tags.second.resize(n);
    return r;
}
}  // namespace detail

inline RichConsensusQVs ConsensusRichQVs(Arrow::ArrowMultiReadMutationScorer& mms)
{
    return detail::RichQVs(mms.TemplateLength(), [&](int* qvs, pbccs_rich_qvs* rich, int* n) {
        return pbccs_consensus_qvs_rich(mms.Handle(), qvs, rich, n);
    });
}

}  // namespace ConsensusCore

// A ConsensusCore caller of the diploid surface, written against the facade headers only
// (include/pbccs_amd/ConsensusCore.hpp for ConsensusCore::Arrow, include/pbccs_amd/Quiver.hpp for ConsensusCore):
// DiploidSite, IsSiteHeterozygous and the scorers' SiteScores / DiploidSites.  Without arguments it checks the
// analytic known answers of IsSiteHeterozygous on the host (no device).  With a case file as argv[1] --
//   <18 params> / <template> / <n reads> / per read: <strand> <ts> <te> <seq> <ins> <subs> <del> <tag> <merge>
//   then one log prior ratio per line
// (the format of quiver_multibase_driver.cpp) -- it builds the Quiver scorer and answers per prior one line per
// heterozygous site: site <prior hex> <position> <allele0> <allele1> <logBF hex> <allele of each read, no spaces>
#include <pbccs_amd/Quiver.hpp>

#include <cmath>
#include <cstdio>
#include <fstream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

using namespace ConsensusCore;

namespace {

int failures = 0;
#define CHECK(x)                                                     \
    do {                                                             \
        if (!(x)) {                                                  \
            std::printf("FAIL line %d: %s\n", __LINE__, #x);         \
            ++failures;                                              \
        }                                                            \
    } while (0)

std::vector<float> track(const std::string& s)
{
    std::vector<float> v;
    std::stringstream ss(s);
    std::string x;
    while (std::getline(ss, x, ',')) v.push_back(std::stof(x));
    return v;
}

void known_answers()
{
    // all-zero scores: every pair total and every column sum is 0, so logBF = ln 12 - ln 9
    std::vector<float> zero(8 * 9, 0.0f);
    std::unique_ptr<DiploidSite> a(IsSiteHeterozygous(zero.data(), 8, 9, 0.0f));
    CHECK(a && std::fabs(a->LogBayesFactor - std::log(12.0 / 9.0)) <= 1e-5);
    CHECK(a && a->Allele0 == 0 && a->Allele1 == 1 && a->AlleleForRead == std::vector<int>(8, 1));
    CHECK(IsSiteHeterozygous(zero.data(), 8, 9, 1.0f) == nullptr);
    // two clean alleles on alternating reads, through the Arrow namespace's names
    std::vector<float> m(8 * 9, -50.0f);
    for (int i = 0; i < 8; ++i) {
        m[i * 9 + 0] = (i % 2) ? -20.0f : 0.0f;
        m[i * 9 + 1] = (i % 2) ? 0.0f : -20.0f;
    }
    std::unique_ptr<Arrow::DiploidSite> b(Arrow::IsSiteHeterozygous(m.data(), 8, 9, 0.0f));
    CHECK(b && std::fabs(b->LogBayesFactor - (80.0 - 9.0 * std::log(2.0))) <= 1e-4);
    CHECK(b && b->Allele0 == 0 && b->Allele1 == 1);
    for (int i = 0; b && i < 8; ++i) CHECK(b->AlleleForRead[i] == i % 2);
    bool threw = false;
    try {
        delete IsSiteHeterozygous(zero.data(), 9, 8, 0.0f);
    } catch (const InvalidInputError&) {
        threw = true;
    }
    CHECK(threw);
}

// the Arrow scorer's members (instantiated so that the facade compiles and links; called only with a device)
std::size_t arrow_surface(Arrow::ArrowMultiReadMutationScorer& s)
{
    return s.SiteScores().size() + s.DiploidSites(0.0f).size();
}

}  // namespace

int main(int argc, char** argv)
{
    try {
        known_answers();
        std::printf("known answers %s\n", failures ? "failed" : "ok");
        if (argc > 1) {
            std::ifstream in(argv[1]);
            float p[18];
            for (float& x : p) in >> x;
            std::string tpl;
            int n = 0;
            in >> tpl >> n;
            QuiverConfigTable table;
            table.InsertDefault(QuiverConfig(
                QvModelParams("*", "test", p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], p[8], p[9], p[10], p[11], p[12],
                              p[13], p[14], p[15], p[16], p[17]),
                ALL_MOVES, BandingOptions(4, 12.5), -12.5));
            SparseSseQvMultiReadMutationScorer s(table, tpl);
            for (int k = 0; k < n; ++k) {
                int strand, ts, te;
                std::string seq, f[5];
                in >> strand >> ts >> te >> seq;
                std::vector<float> tr[5];
                for (int t = 0; t < 5; ++t) {
                    in >> f[t];
                    tr[t] = track(f[t]);
                }
                const QvSequenceFeatures feat(seq, tr[0].data(), tr[1].data(), tr[2].data(), tr[3].data(), tr[4].data());
                s.AddRead(MappedQvRead(QvRead(feat, "read", "*"), strand ? REVERSE_STRAND : FORWARD_STRAND, ts, te));
            }
            const std::vector<float> tensor = s.SiteScores();
            CHECK(tensor.size() == tpl.size() * (std::size_t)n * 9);
            float prior = 0.0f;
            while (in >> prior) {
                for (const DiploidSite& d : s.DiploidSites(prior)) {
                    // the facade's host primitive on the same slice gives the same site
                    std::unique_ptr<DiploidSite> h(
                        IsSiteHeterozygous(tensor.data() + (std::size_t)d.Position * n * 9, n, 9, prior));
                    CHECK(h && h->Allele0 == d.Allele0 && h->Allele1 == d.Allele1 &&
                          h->LogBayesFactor == d.LogBayesFactor && h->AlleleForRead == d.AlleleForRead);
                    std::string afr;
                    for (int a : d.AlleleForRead) afr += (char)('0' + a);
                    std::printf("site %a %d %d %d %a %s\n", (double)prior, d.Position, d.Allele0, d.Allele1,
                                (double)d.LogBayesFactor, afr.c_str());
                }
            }
        }
    } catch (const std::exception& e) {
        std::printf("error %s\n", e.what());
        return 2;
    }
    (void)&arrow_surface;
    return failures ? 1 : 0;
}

// tests/cpp/align_band_driver.cpp -- the certified band through include/pbccs_amd/Align.hpp (BandOptions).
//
// Without arguments: the host-only part (the certificate's bound through the C ABI, the refusal of a negative
// half-width before the engine is touched); prints "band host ok".  No device is needed.
// With "<k> <target> <query>": aligns the pair on the device, full and banded at first half-widths k and k - 1
// (k - 1 only when k > 0), with the three aligners; every banded alignment must equal the full one.  Prints
// "nw <transcript>. <score> attempts <a at k> <a at k - 1> banded <b at k> <b at k - 1>" and "equal ok".
#include <cstdio>
#include <cstdlib>
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

static int HostOnly()
{
    const pbccs_align_params nw = detail::NwParams(AlignConfig::Default());
    double u = 0, e = 1;
    int ok = 0, w = 0;
    REQUIRE(pbccs_align_band_bound(&nw, 120, 120, 5, &u, &e, &ok) == PBCCS_OK);
    REQUIRE(u == -12.0 && e == 0.0 && ok == 1);   // 6 deletes and 6 inserts to reach the first diagonal outside
    REQUIRE(pbccs_align_band_widen(&nw, 120, 120, -10.0, &w) == PBCCS_OK && w == 5);
    const pbccs_align_params bad = detail::AffineParams(PBCCS_ALIGN_AFFINE, AffineAlignmentParams(0, -1, 0.5f, -0.5f));
    REQUIRE(pbccs_align_band_bound(&bad, 120, 120, 5, &u, &e, &ok) == PBCCS_OK && ok == 0);
    REQUIRE(pbccs_align_band_widen(&bad, 120, 120, -10.0, &w) == PBCCS_OK && w == -1);
    bool threw = false;
    try {
        Align("GATT", "GAT", AlignConfig::Default(), BandOptions::Width(-1));
    } catch (const InvalidInputError&) {
        threw = true;
    }
    REQUIRE(threw);
    REQUIRE(BandOptions::Off().Mode == PBCCS_BAND_OFF && BandOptions::Auto().Mode == PBCCS_BAND_AUTO);
    std::printf("band host ok\n");
    return 0;
}

int main(int argc, char** argv)
{
    if (argc < 4) return HostOnly();
    const int k = std::atoi(argv[1]);
    const std::string t = argv[2], q = argv[3];
    try {
        const std::vector<std::pair<std::string, std::string>> pairs{{t, q}};
        std::vector<int> s0, s1, s2;
        std::vector<pbccs_align_band_info> i1, i2;
        std::vector<PairwiseAlignment*> full = AlignBatch(pairs, AlignConfig::Default(), &s0);
        std::vector<PairwiseAlignment*> at = AlignBatch(pairs, AlignConfig::Default(), &s1, BandOptions::Width(k), &i1);
        std::unique_ptr<PairwiseAlignment> a0(full[0]), a1(at[0]);
        REQUIRE(a1->Transcript() == a0->Transcript() && s1 == s0 && i1.size() == 1);
        int attempts2 = 0, banded2 = 0;
        if (k > 0) {
            std::vector<PairwiseAlignment*> below =
                AlignBatch(pairs, AlignConfig::Default(), &s2, BandOptions::Width(k - 1), &i2);
            std::unique_ptr<PairwiseAlignment> a2(below[0]);
            REQUIRE(a2->Transcript() == a0->Transcript() && s2 == s0 && i2.size() == 1);
            attempts2 = i2[0].attempts;
            banded2 = i2[0].banded;
        }
        // the single-pair calls, every aligner, automatic width
        int score = 0;
        std::unique_ptr<PairwiseAlignment> b(Align(t, q, &score, AlignConfig::Default(), BandOptions::Auto()));
        REQUIRE(b->Transcript() == a0->Transcript() && score == s0[0]);
        std::unique_ptr<PairwiseAlignment> f1(AlignAffine(t, q)),
            g1(AlignAffine(t, q, DefaultAffineAlignmentParams(), BandOptions::Width(k)));
        REQUIRE(f1->Transcript() == g1->Transcript());
        std::unique_ptr<PairwiseAlignment> f2(AlignAffineIupac(t, q)),
            g2(AlignAffineIupac(t, q, IupacAwareAffineAlignmentParams(), BandOptions::Width(k)));
        REQUIRE(f2->Transcript() == g2->Transcript());
        std::printf("nw %s. %d attempts %d %d banded %d %d\n", a0->Transcript().c_str(), s0[0], i1[0].attempts,
                    attempts2, i1[0].banded, banded2);
        std::printf("equal ok\n");
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}

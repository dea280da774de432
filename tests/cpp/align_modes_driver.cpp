// tests/cpp/align_modes_driver.cpp -- the ends-free modes through include/pbccs_amd/Align.hpp (AlignEnds).
//
// Without arguments: the refusals, thrown before the engine is touched (no device is needed); prints
// "modes host ok".
// With "<target> <query> <match> <mismatch> <insert> <delete>": aligns the pair on the device SEMIGLOBAL and LOCAL
// and prints one line per mode: "<mode> <transcript>. <score> <target begin> <target end> <query begin> <query end>
// <rc>".  The Python side compares the lines with the restatement.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>

#include <pbccs_amd/Align.hpp>

using namespace ConsensusCore;  // NOLINT

#define REQUIRE(c)                                                        \
    do {                                                                  \
        if (!(c)) {                                                       \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);    \
            return 1;                                                     \
        }                                                                 \
    } while (0)

template <class E, class F>
static bool Throws(F f)
{
    try {
        f();
    } catch (const E&) {
        return true;
    } catch (...) {
        return false;
    }
    return false;
}

static int HostOnly()
{
    AlignExtent x{0, 0, 0, 0, false};
    REQUIRE(Throws<InvalidInputError>([&] { AlignEnds("GATT", "GAT", GLOBAL, AlignParams::Default(), &x); }));
    REQUIRE(Throws<InvalidInputError>([&] { AlignEnds("GATT", "GAT", SEMIGLOBAL, AlignParams(0, -1, 1, -1), &x); }));
    REQUIRE(Throws<InvalidInputError>([&] { AlignEnds("GATT", "GAT", LOCAL, AlignParams(0, -1, -1, 1), &x); }));
    // the reference's own entry goes on refusing the modes
    REQUIRE(Throws<UnsupportedFeatureError>(
        [&] { Align("GATT", "GAT", AlignConfig(AlignParams::Default(), SEMIGLOBAL)); }));
    REQUIRE(Throws<UnsupportedFeatureError>([&] { Align("GATT", "GAT", AlignConfig(AlignParams::Default(), LOCAL)); }));
    // the C entry: the same refusals are PBCCS_EINVAL (a null engine is refused first, so only the shape is checked)
    const pbccs_align_params p = detail::NwParams(AlignConfig::Default());
    const pbccs_align_ends e{PBCCS_POA_LOCAL, 0};
    REQUIRE(pbccs_align_batch_ends(NULL, &p, &e, NULL, 0, NULL, NULL) == PBCCS_EINVAL);
    REQUIRE(ReverseComplementOf("ACGTN") == "MACGT");
    std::printf("modes host ok\n");
    return 0;
}

int main(int argc, char** argv)
{
    if (argc < 7) return HostOnly();
    const std::string t = argv[1], q = argv[2];
    const AlignParams params(std::atoi(argv[3]), std::atoi(argv[4]), std::atoi(argv[5]), std::atoi(argv[6]));
    try {
        const AlignMode modes[2] = {SEMIGLOBAL, LOCAL};
        for (AlignMode m : modes) {
            AlignExtent x{0, 0, 0, 0, false};
            int score = 0;
            std::unique_ptr<PairwiseAlignment> a(AlignEnds(t, q, m, params, &x, &score));
            std::printf("%d %s. %d %d %d %d %d %d\n", (int)m, a->Transcript().c_str(), score, x.TargetBegin, x.TargetEnd,
                        x.QueryBegin, x.QueryEnd, x.ReverseComplemented ? 1 : 0);
        }
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}

// tests/cpp/demux_driver.cpp -- barcode demultiplexing through include/pbccs_amd/Demux.hpp (BarcodeDemux).
//
// Without arguments: the refusals, thrown before the engine is touched (no device is needed); prints
// "demux host ok".
// With "run": reads from standard input "<match> <mismatch> <insert> <delete> <design> <window> <min_quality>
// <min_score_lead>", then one line of barcodes separated by blanks, then one read per line ("-" is the empty read),
// calls them on the device and prints one line per read: lead trail called score score_lead quality, the four
// extent ends, the clip, overlap, and best / index / second of the two ends.  The Python side compares the lines
// with the restatement.
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include <pbccs_amd/Demux.hpp>

using PacBio::CCS::BarcodeCall;
using PacBio::CCS::BarcodeDemux;
using ConsensusCore::AlignParams;
using ConsensusCore::InvalidInputError;

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
    REQUIRE(Throws<InvalidInputError>([] { BarcodeDemux d({}); }));
    REQUIRE(Throws<InvalidInputError>([] { BarcodeDemux d({"ACGN"}); }));
    REQUIRE(Throws<InvalidInputError>([] { BarcodeDemux d({"acgt"}); }));
    REQUIRE(Throws<InvalidInputError>([] { BarcodeDemux d({""}); }));
    REQUIRE(Throws<InvalidInputError>([] { BarcodeDemux d({std::string(65, 'A')}); }));
    REQUIRE(Throws<InvalidInputError>([] { BarcodeDemux d({"ACGT"}, {"a", "b"}); }));
    BarcodeDemux d({"ACGT", std::string(64, 'C')}, {"first", "second"});
    REQUIRE(d.Size() == 2 && d.Name(1) == "second" && BarcodeDemux({"A"}).Name(0) == "0");
    REQUIRE(Throws<InvalidInputError>([&] { d.Params(AlignParams(0, -5, -4, -4)); }));
    REQUIRE(Throws<InvalidInputError>([&] { d.Params(AlignParams(3, -5, 1, -4)); }));
    REQUIRE(Throws<InvalidInputError>([&] { d.Params(AlignParams(3, -5, -4, 1)); }));
    REQUIRE(Throws<InvalidInputError>([&] { d.Window(0); }));
    REQUIRE(Throws<InvalidInputError>([&] { d.Window(1025); }));
    REQUIRE(Throws<InvalidInputError>([&] { d.WindowMult(17); }));
    REQUIRE(Throws<InvalidInputError>([&] { d.MinQuality(-1); }));
    // the C entry: a null engine is refused first, so only the shape is checked
    REQUIRE(pbccs_demux_batch(NULL, NULL, NULL, NULL, 0, NULL) == PBCCS_EINVAL);
    pbccs_demux_options o;
    pbccs_demux_options_default(&o);
    REQUIRE(o.match == 3 && o.mismatch == -5 && o.insert == -4 && o.delete_ == -4 && o.window_mult == 3);
    REQUIRE(o.min_quality == PBCCS_DEMUX_MIN_QUALITY && o.min_score_lead == 0 && o.design == PBCCS_DEMUX_ASYMMETRIC);
    BarcodeCall c{};
    c.Called = true;
    c.Clip = {2, 5};
    REQUIRE(BarcodeDemux::Clip("ACGTACGT", c) == "GTA");
    c.Overlap = true;
    REQUIRE(BarcodeDemux::Clip("ACGTACGT", c) == "ACGTACGT");
    std::printf("demux host ok\n");
    return 0;
}

int main(int argc, char** argv)
{
    if (argc < 2) return HostOnly();
    try {
        int m, x, i, d, design, window, minq, minlead;
        std::string line, tok;
        std::getline(std::cin, line);
        std::istringstream(line) >> m >> x >> i >> d >> design >> window >> minq >> minlead;
        std::getline(std::cin, line);
        std::vector<std::string> barcodes, reads;
        std::istringstream bs(line);
        while (bs >> tok) barcodes.push_back(tok);
        while (std::getline(std::cin, line)) reads.push_back(line == "-" ? std::string() : line);
        BarcodeDemux demux(barcodes);
        demux.Params(AlignParams(m, x, i, d)).SetDesign(design ? BarcodeDemux::SYMMETRIC : BarcodeDemux::ASYMMETRIC);
        demux.MinQuality(minq).MinScoreLead(minlead);
        if (window > 0) demux.Window(window);
        for (const BarcodeCall& c : demux.Call(reads))
            std::printf("%d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d\n", c.Lead, c.Trail, c.Called ? 1 : 0,
                        c.Score, c.ScoreLead, c.Quality, c.LeadExtent.first, c.LeadExtent.second, c.TrailExtent.first,
                        c.TrailExtent.second, c.Clip.first, c.Clip.second, c.Overlap ? 1 : 0, c.LeadBest,
                        c.LeadBestIndex, c.LeadSecond, c.TrailBest, c.TrailBestIndex, c.TrailSecond);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}

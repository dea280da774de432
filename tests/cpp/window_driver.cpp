// tests/cpp/window_driver.cpp -- a caller of the windowed polish written against include/pbccs_amd/WindowedPolish.hpp
// only.
//
// Without arguments: the host-only known answers (the plan, the join rule, the refusals that come before the engine
// is touched); prints "known answers ok".  No device is needed.
// With a case file: polishes its ZMWs on the device and prints per ZMW
//   zmw <status> <fallback> <windows> <unanchored> <tested> <applied> <passes> <consensus>.
//   qvs <q> ...
//   reads <code> ...
//   win <begin> <end> <join> <cut_begin> <cut_end> <status> <tested> <applied>      (one per window)
// Case file: line 1 "<window> <overlap> <guard> <k>", line 2 n, then per ZMW "<draft> <snr x 4> <reads>" and per read
// "<seq> <strand> <ts> <te> <full_pass>" ("." = a placeholder).
#include <cstdio>
#include <fstream>
#include <iostream>
#include <string>
#include <utility>
#include <vector>

#include <pbccs_amd/WindowedPolish.hpp>

using namespace PacBio::CCS;  // NOLINT

#define REQUIRE(c)                                                        \
    do {                                                                  \
        if (!(c)) {                                                       \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);    \
            return 1;                                                     \
        }                                                                 \
    } while (0)

typedef std::vector<std::pair<int, int>> Plan;

static int KnownAnswers()
{
    WindowOptions o;
    o.Window = 200, o.Overlap = 100, o.Guard = 8, o.K = 6;
    REQUIRE((WindowPlan(700, o) == Plan{{0, 300}, {200, 500}, {400, 700}}));
    REQUIRE((WindowPlan(701, o) == Plan{{0, 251}, {151, 402}, {302, 553}, {453, 701}}));
    REQUIRE((WindowPlan(300, o) == Plan{{0, 300}}));
    REQUIRE(WindowPlan(10000).size() == 5 && WindowPlan(2200).size() == 1);
    {
        const std::string all(300, 'M');
        WindowJoinResult j = WindowJoin(all, {0, 300}, all, {200, 500}, 8);
        REQUIRE(j.Found && j.Position == 250 && j.CutA == 250 && j.CutB == 50);
        const std::string del = std::string(250, 'M') + "D" + std::string(49, 'M');
        j = WindowJoin(del, {0, 300}, all, {200, 500}, 8);
        REQUIRE(j.Found && j.Position == 242 && j.CutA == 242 && j.CutB == 42);
        const std::string ins = std::string(50, 'M') + "I" + std::string(250, 'M');
        j = WindowJoin(all, {0, 300}, ins, {200, 500}, 8);
        REQUIRE(j.Found && j.Position == 258 && j.CutA == 258 && j.CutB == 59);
        std::string none;
        for (int i = 0; i < 300; ++i) none += i % 8 == 7 ? 'R' : 'M';
        REQUIRE(!WindowJoin(none, {0, 300}, all, {200, 500}, 8).Found);
    }
    for (const WindowOptions& bad : {WindowOptions{200, 200, 8, 8}, WindowOptions{200, 15, 8, 8}, WindowOptions{200, 100, 0, 8},
                                     WindowOptions{200, 100, 8, 3}, WindowOptions{200, 100, 8, 9}}) {
        bool threw = false;
        try {
            WindowPlan(700, bad);
        } catch (const std::exception&) {
            threw = true;
        }
        REQUIRE(threw);
    }
    std::printf("known answers ok\n");
    return 0;
}

int main(int argc, char** argv)
{
    if (argc < 2) return KnownAnswers();
    std::ifstream in(argv[1]);
    WindowOptions o;
    int n = 0;
    in >> o.Window >> o.Overlap >> o.Guard >> o.K >> n;
    std::vector<WindowedZmw> zmws((size_t)(n > 0 ? n : 0));
    for (WindowedZmw& z : zmws) {
        int nr = 0;
        in >> z.Draft >> z.Snr[0] >> z.Snr[1] >> z.Snr[2] >> z.Snr[3] >> nr;
        z.Reads.resize((size_t)(nr > 0 ? nr : 0));
        for (WindowedRead& r : z.Reads) {
            int full = 1;
            in >> r.Seq >> r.Strand >> r.TemplateStart >> r.TemplateEnd >> full;
            r.FullPass = full != 0;
            if (r.Seq == ".") r.Seq.clear(), r.Placeholder = true;
        }
    }
    if (!in) {
        std::fprintf(stderr, "bad case file\n");
        return 2;
    }
    try {
        const std::vector<WindowedResult> res = WindowedPolish(zmws, nullptr, o);
        for (const WindowedResult& r : res) {
            std::printf("zmw %d %d %zu %d %lld %lld %d %s.\n", r.Status, r.Fallback, r.Windows.size(), r.UnanchoredReads,
                        r.Tested, r.Applied, r.NumPasses, r.Consensus.c_str());
            std::printf("qvs");
            for (int q : r.Qvs) std::printf(" %d", q);
            std::printf("\nreads");
            for (int c : r.AddReadResults) std::printf(" %d", c);
            std::printf("\n");
            for (const WindowRecord& w : r.Windows)
                std::printf("win %d %d %d %d %d %d %lld %lld\n", w.Begin, w.End, w.Join, w.CutBegin, w.CutEnd, w.Status,
                            w.Tested, w.Applied);
        }
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}

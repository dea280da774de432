// PacBio::CCS::SplitMapToDraft through include/pbccs_amd/SparsePoa.hpp.  Input (stdin): line 1 = jump penalty and
// max segments, line 2 = the draft, then one read per line.  Output per read: one "count truncated score" line, then
// one "rc readBegin readEnd cssBegin cssEnd score" line per segment returned.
#include <pbccs_amd/SparsePoa.hpp>

#include <iostream>
#include <sstream>
#include <string>
#include <vector>

using namespace PacBio::CCS;

int main()
{
    std::string line, draft;
    if (!std::getline(std::cin, line)) return 2;
    int jumpPenalty = 0, maxSegments = 0;
    std::istringstream(line) >> jumpPenalty >> maxSegments;
    if (!std::getline(std::cin, draft)) return 2;
    std::vector<std::string> reads;
    while (std::getline(std::cin, line)) reads.push_back(line);

    const std::vector<SplitAlignment> chains = SplitMapToDraft(draft, reads, jumpPenalty, maxSegments);
    for (const SplitAlignment& c : chains) {
        std::cout << c.NumSegments << " " << c.Truncated << " " << c.Score << "\n";
        for (const PoaAlignmentSummary& s : c.Segments)
            std::cout << s.ReverseComplementedRead << " " << s.ExtentOnRead.Left() << " " << s.ExtentOnRead.Right() << " "
                      << s.ExtentOnConsensus.Left() << " " << s.ExtentOnConsensus.Right() << " " << (int)s.AlignmentScore
                      << "\n";
    }
    return 0;
}

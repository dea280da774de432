// PacBio::CCS::ConsensusPileup and PileupCigar through include/pbccs_amd/Pileup.hpp.
// "pileup_driver cigar": stdin holds lines "transcript rb read_length"; prints one CIGAR per line (host code only).
// Without an argument (or with "band"), stdin: line 1 = the consensus, then one read per line.  Output, one line of
// integers each: "cov_sum n_used_fwd n_used_rev", forward counts, reverse counts, forward / reverse inserting reads,
// forward / reverse inserted bases, slot coverage, longest insertion, coverage, plurality, insertion plurality, then
// per read "status n_match n_mismatch n_ins n_del rc rb re tb te" followed by a line with its transcript.
#include <pbccs_amd/Pileup.hpp>

#include <iostream>
#include <sstream>
#include <string>
#include <vector>

using namespace PacBio::CCS;

template <class V>
static void line_of(const V& v)
{
    for (size_t k = 0; k < v.size(); ++k) std::cout << (k ? " " : "") << (long long)v[k];
    std::cout << "\n";
}

int main(int argc, char** argv)
{
    if (argc > 1 && std::string(argv[1]) == "cigar") {
        std::string tr;
        int rb, len;
        while (std::cin >> tr >> rb >> len) std::cout << PileupCigar(tr, rb, len) << "\n";
        return 0;
    }
    std::string consensus, seq;
    if (!std::getline(std::cin, consensus)) return 2;
    std::vector<std::string> reads;
    while (std::getline(std::cin, seq)) reads.push_back(seq);
    const ConsensusPileupResult r = ConsensusPileup(consensus, reads, argc > 1 && std::string(argv[1]) == "band");
    std::cout << r.CoverageSum << " " << r.NumUsed[0] << " " << r.NumUsed[1] << "\n";
    line_of(r.Counts[0]);
    line_of(r.Counts[1]);
    line_of(r.InsertingReads[0]);
    line_of(r.InsertingReads[1]);
    line_of(r.InsertedBases[0]);
    line_of(r.InsertedBases[1]);
    line_of(r.SlotCoverage);
    line_of(r.MaxInsertion);
    line_of(r.Coverage);
    line_of(r.Plurality);
    line_of(r.InsertionPlurality);
    for (const PileupRead& p : r.Reads) {
        std::cout << p.Status << " " << p.NumMatch << " " << p.NumMismatch << " " << p.NumInsertion << " "
                  << p.NumDeletion << " " << (p.ReverseComplemented ? 1 : 0) << " " << p.ReadBegin << " " << p.ReadEnd
                  << " " << p.TemplateBegin << " " << p.TemplateEnd << "\n"
                  << p.Transcript << "\n";
    }
    return 0;
}

// A ConsensusCore caller written against include/pbccs_amd/ConsensusCore.hpp only: the Arrow scorer with mutations
// of any width and RefineRepeats.  Input (stdin):
//   line 1: <draft> <snrA> <snrC> <snrG> <snrT> <repeatLength>
//   line 2: <type 0|1|2> <start> <end> <new bases, or - for a deletion>     the wide mutation to score on the draft
//   then  : <strand 0|1> <tstart> <tend> <read bases>
// Output: the wide mutation's Score, FastScore and Scores as hex floats, then RefineConsensus, RefineRepeats (twice)
// with the templates they end on, and the template after ApplyMutations of the wide mutation.
#include <pbccs_amd/ConsensusCore.hpp>

#include <cstdio>
#include <iostream>
#include <string>
#include <vector>

using namespace ConsensusCore;
using namespace ConsensusCore::Arrow;

static std::string hex(double v)
{
    char b[64];
    std::snprintf(b, sizeof(b), "%a", v);
    return b;
}

int main()
{
    std::string draft, bases;
    double a, c, g, t;
    int repeatLength, mtype, mstart, mend;
    if (!(std::cin >> draft >> a >> c >> g >> t >> repeatLength)) return 2;
    if (!(std::cin >> mtype >> mstart >> mend >> bases)) return 2;
    ArrowConfig config(ContextParameters(SNR(a, c, g, t)), BandingOptions(12.5));
    ArrowMultiReadMutationScorer scorer(config, draft);
    int strand, ts, te;
    std::string seq;
    while (std::cin >> strand >> ts >> te >> seq)
        scorer.AddRead(MappedArrowRead(ArrowRead(ArrowSequenceFeatures(seq), "read", "N/A"),
                                       strand ? REVERSE_STRAND : FORWARD_STRAND, ts, te));
    const Mutation wide((MutationType)mtype, mstart, mend, mtype == DELETION ? std::string() : bases);
    std::cout << "score " << hex(scorer.Score(wide)) << " " << hex(scorer.FastScore(wide));
    for (double v : scorer.Scores(wide)) std::cout << " " << hex(v);
    std::cout << "\n";
    size_t nTested = 0, nApplied = 0;
    const bool converged = RefineConsensus(scorer, &nTested, &nApplied);
    std::cout << "refine " << converged << " " << nTested << " " << nApplied << " " << scorer.Template() << "\n";
    for (int pass = 0; pass < 2; ++pass) {
        size_t rt = 0, ra = 0;
        const bool rc = RefineRepeats(scorer, repeatLength, 3, &rt, &ra);
        std::cout << "repeats " << rc << " " << rt << " " << ra << " " << scorer.Template() << "\n";
    }
    // ApplyMutations takes the same Mutation
    scorer.ApplyMutations(std::vector<Mutation>{wide});
    std::cout << "applied " << scorer.Template() << "\n";
    return 0;
}

// pbccs_amd/csrc/refine_repeats.hpp -- the host loop of RefineRepeats, shared by the Quiver and the Arrow batch.
//
// AbstractRefineConsensus (Consensus-inl.hpp:159-251) over RepeatMutationEnumerator for any number of scorers in
// lock-step rounds: per round every scorer's candidates (all of them in its first round, UniqueNearbyMutations of
// the last round's favourable ones after), one scoring call and one refill for all scorers, BestSubset on the host
// (a scorer has a handful of repeat candidates).  What differs between the families sits behind Ops:
//   const std::string& Template(int z)
//   int Refuse(int z, const std::vector<MutationEx>& cand)
//       0, or the status that ends the scorer's loop before any of its candidates is scored (the 8-column rule, ...)
//   void Score(const std::vector<int>& zs, const std::vector<std::vector<MutationEx>>& cand,
//              std::vector<std::vector<float>>* score, std::vector<std::vector<char>>* favourable)
//       per scorer and candidate the float-cast Score and the family's FastIsFavorable
//   void Edit(int z, const std::string& next, const std::vector<int>& mtp, std::vector<int>* refill)
//       the template becomes `next`, the reads' windows go through mtp, the reads to refill are appended
//   void Refill(const std::vector<int>& reads)
// status[k]: 0, 1 when an edit could not be applied, or what Refuse returned.
#pragma once

#include <set>
#include <string>
#include <vector>

#include "arrow_model.hpp"
#include "engine.hpp"

namespace pbccs {

struct ScoredEx {
    int idx, pos;
    float score;
};

inline std::vector<ScoredEx> best_subset_ex(std::vector<ScoredEx> in, int sep)   // Consensus-inl.hpp:98-118
{
    if (sep == 0) return in;
    std::vector<ScoredEx> out;
    while (!in.empty()) {
        size_t best = 0;
        for (size_t k = 1; k < in.size(); ++k)
            if (in[best].score < in[k].score) best = k;
        const ScoredEx b = in[best];
        out.push_back(b);
        std::vector<ScoredEx> keep;
        for (const ScoredEx& s : in)
            if (!(b.pos - sep <= s.pos && s.pos <= b.pos + sep)) keep.push_back(s);
        in.swap(keep);
    }
    return out;
}

template <class Ops>
void refine_repeats_lockstep(Ops& ops, const std::vector<int>& zs, int repeatLength, int minRepeatElements,
                             const RefineOptions& ro, std::vector<long long>* nTested,
                             std::vector<long long>* nApplied, std::vector<char>* converged, std::vector<int>* status)
{
    const int n = (int)zs.size();
    nTested->assign(n, 0);
    nApplied->assign(n, 0);
    converged->assign(n, 0);
    status->assign(n, 0);
    std::vector<char> done(n, 0);
    std::vector<int> iter(n, 0);
    std::vector<std::set<std::string>> history(n);
    std::vector<std::vector<int>> centers(n);
    if (ro.maxIterations <= 0) return;
    for (;;) {
        std::vector<int> act, idx;
        std::vector<std::vector<MutationEx>> cand;
        for (int k = 0; k < n; ++k) {
            if (done[k]) continue;
            const std::string& tpl = ops.Template(zs[k]);
            std::vector<MutationEx> c;
            if (iter[k] == 0) repeat_mutations(tpl, repeatLength, minRepeatElements, 0, (int)tpl.size(), &c);
            else nearby_repeat_mutations(tpl, repeatLength, minRepeatElements, centers[k], ro.mutationNeighborhood, &c);
            if (const int why = ops.Refuse(zs[k], c)) {   // nothing of this scorer is scored
                (*status)[k] = why;
                done[k] = 1;
                continue;
            }
            (*nTested)[k] += (long long)c.size();
            act.push_back(zs[k]);
            idx.push_back(k);
            cand.push_back(std::move(c));
        }
        if (act.empty()) break;
        std::vector<std::vector<float>> score;
        std::vector<std::vector<char>> favourable;
        ops.Score(act, cand, &score, &favourable);
        std::vector<int> refill;
        for (size_t a = 0; a < act.size(); ++a) {
            const int k = idx[a];
            const std::string tpl = ops.Template(act[a]);
            std::vector<ScoredEx> fav;
            for (int m = 0; m < (int)cand[a].size(); ++m)
                if (favourable[a][m]) fav.push_back({m, cand[a][m].start, score[a][m]});
            if (fav.empty()) {
                (*converged)[k] = 1;
                done[k] = 1;
                continue;
            }
            std::vector<ScoredEx> best = best_subset_ex(fav, ro.mutationSeparation);
            std::vector<MutationEx> muts;
            for (const ScoredEx& s : best) muts.push_back(cand[a][s.idx]);
            if (best.size() > 1) {   // a template seen before: the single best mutation only (:215-223)
                std::string nx;
                std::vector<int> mtp;
                if (apply_mutations_ex(tpl, muts, &nx, &mtp) && history[k].count(nx)) {
                    best.resize(1);
                    muts.resize(1);
                }
            }
            (*nApplied)[k] += (long long)best.size();
            history[k].insert(tpl);
            centers[k].clear();
            for (const ScoredEx& s : fav) centers[k].push_back(s.pos);
            std::string next;
            std::vector<int> mtp;
            if (!apply_mutations_ex(tpl, muts, &next, &mtp) || next.empty()) {
                (*status)[k] = 1;
                done[k] = 1;
                continue;
            }
            ops.Edit(act[a], next, mtp, &refill);
            if (++iter[k] >= ro.maxIterations) done[k] = 1;
        }
        if (!refill.empty()) ops.Refill(refill);   // a refill that mismatches marks the read inactive
    }
}

}  // namespace pbccs

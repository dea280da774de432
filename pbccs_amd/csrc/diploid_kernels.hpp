// pbccs_amd/csrc/diploid_kernels.hpp -- diploid site calling shared by the Arrow and Quiver engines
// (ConsensusCore Arrow/Diploid.cpp:94-241, Quiver/Diploid.cpp): the site tensor, the per-site screen and the
// host decision of the sites the screen marks.
#pragma once

#include <hip/hip_runtime.h>

#include <vector>

#include "arrow_model.hpp"
#include "engine.hpp"

namespace pbccs {

// Sites per scoring round of SiteScores: 8 mutations per site, so a round holds 32768 mutations per read -- what
// a ConsensusQVs round of a 4 kb template already puts through the scoring launches, their scratch pools and the
// edge-case lists (all of which regrow on overflow; the chunk keeps a long template from sizing them in one step).
constexpr int kSiteChunk = 4096;
int site_chunk();   // kSiteChunk, or PBCCS_SITE_CHUNK (test hook: several rounds on a short template)

// The 8 scored mutation codes of every site of [begin, end), site-major, in column order with the template
// base's own substitution left out (the unique-mutation enumeration would also drop homopolymer duplicates).
void site_mutation_codes(const std::string& tpl, int begin, int end, std::vector<int>* codes);

// k_site_scores: out[(site0 + s) * nReads * 9 ...] for the nSites sites of one scoring round over `codes`
// (8 per site).  Arrow: delta[read * M + m] doubles, masked by rActive / ReadScoresMutation as k_reduce masks
// them, rounded to float.  Quiver: delta[m * nReads + read] floats, NaN (inactive / not scored) -> 0.
void launch_site_scores_arrow(const double* delta, const int* codes, const int* rActive, const int* rTs,
                              const int* rTe, int nReads, int nSites, float* out, hipStream_t s);
void launch_site_scores_quiver(const float* delta, const int* codes, int nReads, int nSites, float* out,
                               hipStream_t s);

// The screen (k_diploid) over a device tensor [nSites][nReads][9], the marked sites' slices packed into one
// download (k_dgather) and decided by is_site_heterozygous.  Reported sites in ascending position (begin + site);
// alleleForRead holds nReads entries per reported site.
void diploid_sites(const float* tensor, int nSites, int nReads, int begin, float logPriorRatio, bool hostAll,
                   DiploidScratch& scratch, hipStream_t s, std::vector<DiploidSiteH>* sites,
                   std::vector<int>* alleleForRead, DiploidStats* stats);

}  // namespace pbccs

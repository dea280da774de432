// include/pbccs_amd/SparseAlignment.hpp -- header-only C++ facade for SparseAlign, with pbccs's and ConsensusCore's
// names, over pbccs_sparse_align_batch (include/pbccs_amd.h).
//
// Mirrored surface (reference file:line):
//   PacBio::CCS::SparseAlign<TSize>(const std::string&, const std::string&)  include/pacbio/ccs/SparseAlignment.h:292-310
//   PacBio::CCS::SdpRangeFinder::FindAnchors                                 src/SparsePoa.cpp:56-64
//   ConsensusCore::detail::SdpAnchor / SdpAnchorVector                       ConsensusCore/Poa/RangeFinder.hpp:20-21
// Beyond the reference: SdpRangeFinder::FindAlignableRanges, the rows InitRangeFinder would report for a graph that
// holds only the consensus as one unbranched path; InitRangeFinder / FindAlignableRange (RangeFinder.cpp:71-171) take
// a SparsePoa (SparsePoa.hpp) in place of the graph, consensus path and consensus sequence, which stay in the engine.
#pragma once

#include <algorithm>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "ConsensusCore.hpp"

namespace ConsensusCore {
namespace detail {
typedef std::pair<size_t, size_t> SdpAnchor;
typedef std::vector<SdpAnchor> SdpAnchorVector;
}  // namespace detail
}  // namespace ConsensusCore

namespace PacBio {
namespace CCS {

namespace detail {
// one pair through pbccs_sparse_align_batch; ranges (optional) receives 2 * seq1.size() ints
inline std::vector<std::pair<size_t, size_t>> SparseAlignK(int k, const std::string& seq1, const std::string& seq2,
                                                           std::vector<int>* ranges = nullptr)
{
    const int cap = std::max(0, (int)std::min(seq1.size(), seq2.size()) - k + 1);
    std::vector<int> anchors(2 * (size_t)cap + 2);
    if (ranges) ranges->assign(2 * seq1.size() + 2, 0);
    const pbccs_sparse_align_input in{seq1.data(), (int)seq1.size(), seq2.data(), (int)seq2.size(), 0,
                                      anchors.data(), cap, ranges ? ranges->data() : nullptr};
    pbccs_sparse_align_output out{};
    ConsensusCore::detail::Check(pbccs_sparse_align_batch(ConsensusCore::detail::DefaultEngine(), k, &in, 1, &out));
    if (ranges) ranges->resize(2 * seq1.size());
    std::vector<std::pair<size_t, size_t>> chain;
    for (int a = 0; a < out.n_anchors; ++a) chain.emplace_back((size_t)anchors[2 * a], (size_t)anchors[2 * a + 1]);
    return chain;
}
}  // namespace detail

// SparseAlign<TSize>(seq1, seq2): the chained K-mer anchors (position in seq1, position in seq2).  4 <= TSize <= 8.
template <size_t TSize>
std::vector<std::pair<size_t, size_t>> SparseAlign(const std::string& seq1, const std::string& seq2)
{
    return detail::SparseAlignK((int)TSize, seq1, seq2);
}

// src/SparsePoa.cpp:52-65.  The reference's class derives from ConsensusCore's SdpRangeFinder and is handed to the
// POA, which then ignores the rows it reports (PoaGraphImpl.cpp:235-352); here it stands alone.
class SdpRangeFinder {
public:
    ConsensusCore::detail::SdpAnchorVector FindAnchors(const std::string& consensusSequence,
                                                       const std::string& readSequence) const
    {
        return SparseAlign<6>(consensusSequence, readSequence);
    }

    // [begin, end) of the read rows alignable to each consensus position (WIDTH 30 around an anchor)
    std::vector<std::pair<int, int>> FindAlignableRanges(const std::string& consensusSequence,
                                                         const std::string& readSequence) const
    {
        std::vector<int> flat;
        detail::SparseAlignK(6, consensusSequence, readSequence, &flat);
        std::vector<std::pair<int, int>> ranges;
        for (size_t p = 0; p < consensusSequence.size(); ++p) ranges.emplace_back(flat[2 * p], flat[2 * p + 1]);
        return ranges;
    }

    // InitRangeFinder over a SparsePoa's current graph (which must hold a read) for one read; false when the
    // alignment would take the full fill, and FindAlignableRange then has nothing to report.
    template <class TSparsePoa>
    bool InitRangeFinder(const TSparsePoa& poa, const std::string& readSequence, bool reverseComplement = false)
    {
        return poa.AlignableRanges(readSequence, reverseComplement, &consensusPath_, &anchors_, &rangeByVertex_);
    }
    // [begin, end) of the read rows alignable to a vertex of that graph
    std::pair<int, int> FindAlignableRange(size_t vertex) const
    {
        if (vertex >= rangeByVertex_.size()) throw std::out_of_range("FindAlignableRange: no such vertex");
        return rangeByVertex_[vertex];
    }
    const std::vector<int>& ConsensusPath() const { return consensusPath_; }
    const ConsensusCore::detail::SdpAnchorVector& Anchors() const { return anchors_; }

private:
    std::vector<int> consensusPath_;
    ConsensusCore::detail::SdpAnchorVector anchors_;
    std::vector<std::pair<int, int>> rangeByVertex_;
};

}  // namespace CCS
}  // namespace PacBio

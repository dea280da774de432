// include/pbccs_amd/Demux.hpp -- barcode demultiplexing of CCS reads over the C ABI (pbccs_demux_batch).
//
// Header-only.  The reference has no demultiplexing; the rules are this project's own (stated in
// full in tests/demux_restatement.py): every barcode is placed SEMIGLOBAL inside a window at each read end, the
// leading end forward and the trailing end reverse-complemented, and the best pair is called when its quality and
// its lead over the second best pass two thresholds.
#pragma once

#include <algorithm>
#include <string>
#include <utility>
#include <vector>

#include <pbccs_amd.h>
#include <pbccs_amd/Align.hpp>

namespace PacBio {
namespace CCS {

struct BarcodeCall {
    int Lead, Trail;                 // the called barcodes i and j (filled for an uncalled read too)
    bool Called;
    std::pair<int, int> Pair;        // (min, max), or (-1, -1) for an uncalled read
    int Score, ScoreLead, Quality;
    std::pair<int, int> LeadExtent, TrailExtent;   // in read coordinates
    std::pair<int, int> Clip;        // the insert is read.substr(Clip.first, Clip.second - Clip.first); (-1, -1): overlap
    bool Overlap;
    int LeadBest, LeadBestIndex, LeadSecond, TrailBest, TrailBestIndex, TrailSecond;   // second INT_MIN: none
};

class BarcodeDemux {
public:
    enum Design { ASYMMETRIC = PBCCS_DEMUX_ASYMMETRIC, SYMMETRIC = PBCCS_DEMUX_SYMMETRIC };

    // Thrown here, before any engine exists (ConsensusCore::InvalidInputError): no barcode or more than 65535, a
    // barcode of 0 or more than 64 bases or with a character other than uppercase A C G T.
    explicit BarcodeDemux(std::vector<std::string> barcodes, std::vector<std::string> names = {})
        : barcodes_(std::move(barcodes)), names_(std::move(names))
    {
        using ConsensusCore::InvalidInputError;
        if (barcodes_.empty() || barcodes_.size() > PBCCS_DEMUX_MAX_BARCODES)
            throw InvalidInputError("a barcode set holds 1 to 65535 barcodes");
        if (!names_.empty() && names_.size() != barcodes_.size()) throw InvalidInputError("one name per barcode");
        for (const std::string& b : barcodes_) {
            if (b.empty() || b.size() > PBCCS_DEMUX_MAX_BARCODE_LEN)
                throw InvalidInputError("a barcode has 1 to 64 bases");
            if (b.find_first_not_of("ACGT") != std::string::npos)
                throw InvalidInputError("a barcode holds uppercase A, C, G and T only");
            longest_ = std::max(longest_, (int)b.size());
        }
        pbccs_demux_options_default(&opts_);
    }

    // The options; every setter returns *this.  Params: Match > 0, Insert <= 0, Delete <= 0.
    BarcodeDemux& Params(const ConsensusCore::AlignParams& p)
    {
        if (p.Match <= 0 || p.Insert > 0 || p.Delete > 0)
            throw ConsensusCore::InvalidInputError("demux needs Match > 0, Insert <= 0 and Delete <= 0");
        opts_.match = p.Match;
        opts_.mismatch = p.Mismatch;
        opts_.insert = p.Insert;
        opts_.delete_ = p.Delete;
        return *this;
    }
    BarcodeDemux& SetDesign(Design d)
    {
        opts_.design = (int)d;
        return *this;
    }
    BarcodeDemux& Window(int w)   // 1..1024; without it three times the longest barcode (WindowMult)
    {
        if (w < 1 || w > PBCCS_DEMUX_MAX_WINDOW)
            throw ConsensusCore::InvalidInputError("the demux window is 1 to 1024 bases");
        opts_.window = w;
        return *this;
    }
    BarcodeDemux& WindowMult(int m)
    {
        if (m < 1 || (long long)m * longest_ > PBCCS_DEMUX_MAX_WINDOW)
            throw ConsensusCore::InvalidInputError("the demux window is 1 to 1024 bases");
        opts_.window = 0;
        opts_.window_mult = m;
        return *this;
    }
    BarcodeDemux& MinQuality(int q)
    {
        if (q < 0) throw ConsensusCore::InvalidInputError("min_quality >= 0");
        opts_.min_quality = q;
        return *this;
    }
    BarcodeDemux& MinScoreLead(int s)
    {
        opts_.min_score_lead = s;
        return *this;
    }

    size_t Size() const { return barcodes_.size(); }
    const std::string& Barcode(size_t k) const { return barcodes_[k]; }
    std::string Name(size_t k) const { return names_.empty() ? std::to_string(k) : names_[k]; }

    // Every read in one device call; scores (optional) receives the full matrix [read][end][barcode].
    std::vector<BarcodeCall> Call(const std::vector<std::string>& reads, std::vector<int>* scores = NULL) const
    {
        const int n = (int)reads.size(), B = (int)barcodes_.size();
        std::vector<const char*> seqs(B);
        std::vector<int> lens(B);
        for (int b = 0; b < B; ++b) {
            seqs[b] = barcodes_[b].data();
            lens[b] = (int)barcodes_[b].size();
        }
        const pbccs_demux_barcodes bc{seqs.data(), lens.data(), B};
        std::vector<pbccs_demux_read> in(n);
        for (int r = 0; r < n; ++r) in[r] = pbccs_demux_read{reads[r].data(), (int)reads[r].size()};
        std::vector<int> lead(n), trail(n), called(n), score(n), sl(n), q(n), ext(4 * (size_t)n), clip(2 * (size_t)n),
            over(n), best(6 * (size_t)n);
        if (scores) scores->assign((size_t)n * 2 * B, 0);
        pbccs_demux_output out{lead.data(), trail.data(), called.data(), score.data(), sl.data(), q.data(),
                               ext.data(), clip.data(), over.data(), best.data(), scores ? scores->data() : NULL};
        ConsensusCore::detail::Check(
            pbccs_demux_batch(ConsensusCore::detail::DefaultEngine(), &bc, &opts_, in.data(), n, &out));
        std::vector<BarcodeCall> res(n);
        for (int r = 0; r < n; ++r) {
            BarcodeCall& c = res[r];
            c.Lead = lead[r];
            c.Trail = trail[r];
            c.Called = called[r] != 0;
            c.Pair = c.Called ? std::make_pair(std::min(c.Lead, c.Trail), std::max(c.Lead, c.Trail))
                              : std::make_pair(-1, -1);
            c.Score = score[r];
            c.ScoreLead = sl[r];
            c.Quality = q[r];
            c.LeadExtent = std::make_pair(ext[4 * r], ext[4 * r + 1]);
            c.TrailExtent = std::make_pair(ext[4 * r + 2], ext[4 * r + 3]);
            c.Clip = std::make_pair(clip[2 * r], clip[2 * r + 1]);
            c.Overlap = over[r] != 0;
            c.LeadBest = best[6 * r];
            c.LeadBestIndex = best[6 * r + 1];
            c.LeadSecond = best[6 * r + 2];
            c.TrailBest = best[6 * r + 3];
            c.TrailBestIndex = best[6 * r + 4];
            c.TrailSecond = best[6 * r + 5];
        }
        return res;
    }

    BarcodeCall Call(const std::string& read) const { return Call(std::vector<std::string>(1, read))[0]; }

    // The insert of a read: the read without its two barcodes; whole when uncalled or when the barcodes overlap
    static std::string Clip(const std::string& read, const BarcodeCall& c)
    {
        if (!c.Called || c.Overlap) return read;
        return read.substr(c.Clip.first, c.Clip.second - c.Clip.first);
    }

private:
    std::vector<std::string> barcodes_, names_;
    int longest_ = 0;
    pbccs_demux_options opts_;
};

}  // namespace CCS
}  // namespace PacBio

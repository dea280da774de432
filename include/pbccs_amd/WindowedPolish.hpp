// include/pbccs_amd/WindowedPolish.hpp -- header-only C++ facade for the windowed polish over the C ABI
// (pbccs_polish_windowed).  The reference has no counterpart: a caller of Consensus.h's polish
// that wants long drafts polished in overlapping windows hands its mapped reads to PacBio::CCS::WindowedPolish.
//
//   WindowOptions                       pbccs_window_options (window 2000, overlap 200, guard 8, k 6)
//   WindowPlan(L, opts)                 the windows of a draft (host only)
//   WindowJoin(ta, wa, tb, wb, guard)   the join of two windows' transcripts (host only)
//   WindowedPolish(zmws, settings, opts) one record per ZMW, stitched or from the whole-template route
#pragma once

#include <cmath>
#include <string>
#include <utility>
#include <vector>

#include "ConsensusCore.hpp"

namespace PacBio {
namespace CCS {

struct WindowOptions {
    int Window = 2000, Overlap = 200, Guard = 8, K = 6;
    pbccs_window_options C() const { return pbccs_window_options{Window, Overlap, Guard, K}; }
};

struct WindowedRead {
    std::string Seq;   // as sequenced; empty with Placeholder: a read the driver did not add
    bool Placeholder = false;
    int Strand = 0, TemplateStart = 0, TemplateEnd = 0;
    bool FullPass = true;
};

struct WindowedZmw {
    std::string Draft;
    double Snr[4] = {0, 0, 0, 0};
    std::vector<WindowedRead> Reads;
};

struct WindowRecord {
    int Begin, End, Join, CutBegin, CutEnd, Status;
    long long Tested, Applied;
};

struct WindowedResult {
    int Status = PBCCS_ZMW_OTHER;
    std::string Consensus;
    std::vector<int> Qvs, AddReadResults, StatusCounts;
    std::vector<double> ZScores;
    double GlobalZScore = 0, AvgZScore = 0, PredictedAccuracy = 0;
    long long Tested = 0, Applied = 0;
    int NumPasses = 0;
    bool Windowed = false;
    int Fallback = PBCCS_WINDOW_FALLBACK_NONE, UnanchoredReads = 0;
    std::vector<WindowRecord> Windows;
};

inline std::vector<std::pair<int, int>> WindowPlan(int draftLength, const WindowOptions& opts = WindowOptions())
{
    const pbccs_window_options w = opts.C();
    int n = 0;
    const int rc = pbccs_window_plan(draftLength, &w, nullptr, 0, &n);
    if (rc != PBCCS_OK && rc != PBCCS_ERANGE) ConsensusCore::detail::Check(rc);
    std::vector<int> b(2 * (size_t)(n > 0 ? n : 1));
    ConsensusCore::detail::Check(pbccs_window_plan(draftLength, &w, b.data(), n, &n));
    std::vector<std::pair<int, int>> out;
    for (int i = 0; i < n; ++i) out.emplace_back(b[2 * i], b[2 * i + 1]);
    return out;
}

// found: (true, p, cutA, cutB)
struct WindowJoinResult {
    bool Found;
    int Position, CutA, CutB;
};

inline WindowJoinResult WindowJoin(const std::string& transcriptA, std::pair<int, int> windowA,
                                   const std::string& transcriptB, std::pair<int, int> windowB, int guard = 8)
{
    int found = 0, p = -1, ca = 0, cb = 0;
    ConsensusCore::detail::Check(pbccs_window_join(transcriptA.data(), (int)transcriptA.size(), windowA.first,
                                                   windowA.second, transcriptB.data(), (int)transcriptB.size(),
                                                   windowB.first, windowB.second, guard, &found, &p, &ca, &cb));
    return WindowJoinResult{found != 0, p, ca, cb};
}

// settings NULL: pbccs_polish_options_default
inline std::vector<WindowedResult> WindowedPolish(const std::vector<WindowedZmw>& zmws,
                                                  const pbccs_polish_options* settings = nullptr,
                                                  const WindowOptions& opts = WindowOptions())
{
    const int n = (int)zmws.size();
    const pbccs_window_options w = opts.C();
    struct Arrays {
        std::vector<const char*> seqs;
        std::vector<int> lens, strands, ts, te, arr, qvs;
        std::vector<unsigned char> full;
        std::vector<double> zs;
        std::string cons;
        std::vector<pbccs_window_record> recs;
    };
    std::vector<Arrays> A((size_t)n);
    std::vector<pbccs_zmw_input> in((size_t)n);
    std::vector<pbccs_zmw_output> out((size_t)n);
    std::vector<pbccs_window_info> info((size_t)n);
    for (int z = 0; z < n; ++z) {
        const WindowedZmw& Z = zmws[z];
        Arrays& a = A[z];
        for (const WindowedRead& r : Z.Reads) {
            a.seqs.push_back(r.Placeholder ? nullptr : r.Seq.data());
            a.lens.push_back(r.Placeholder ? 0 : (int)r.Seq.size());
            a.strands.push_back(r.Strand);
            a.ts.push_back(r.TemplateStart);
            a.te.push_back(r.TemplateEnd);
            a.full.push_back(r.FullPass ? 1 : 0);
        }
        const size_t nr = Z.Reads.size();
        a.arr.assign(nr + 1, -1);
        a.zs.assign(nr + 1, 0.0);
        a.cons.assign(2 * Z.Draft.size() + 64, '\0');
        a.qvs.assign(a.cons.size(), 0);
        a.recs.resize(WindowPlan((int)Z.Draft.size(), opts).size());
        in[z].draft = Z.Draft.data();
        in[z].draft_len = (int)Z.Draft.size();
        for (int k = 0; k < 4; ++k) in[z].snr[k] = Z.Snr[k];
        in[z].n_reads = (int)nr;
        a.seqs.push_back(nullptr);   // never an empty array behind the pointers
        a.lens.push_back(0), a.strands.push_back(0), a.ts.push_back(0), a.te.push_back(0), a.full.push_back(0);
        in[z].seqs = a.seqs.data();
        in[z].lens = a.lens.data();
        in[z].strands = a.strands.data();
        in[z].tstarts = a.ts.data();
        in[z].tends = a.te.data();
        in[z].full_pass = a.full.data();
        out[z] = pbccs_zmw_output();
        out[z].consensus = &a.cons[0];
        out[z].consensus_cap = (int)a.cons.size();
        out[z].qvs = a.qvs.data();
        out[z].add_read_results = a.arr.data();
        out[z].zscores = a.zs.data();
        info[z] = pbccs_window_info();
        info[z].windows = a.recs.data();
        info[z].windows_cap = (int)a.recs.size();
    }
    ConsensusCore::detail::Check(pbccs_polish_windowed(ConsensusCore::detail::DefaultEngine(), in.data(), n, settings, &w,
                                                       out.data(), info.data()));
    std::vector<WindowedResult> res((size_t)n);
    for (int z = 0; z < n; ++z) {
        WindowedResult& r = res[z];
        const pbccs_zmw_output& o = out[z];
        const size_t nr = zmws[z].Reads.size();
        r.Status = o.status;
        if ((o.status == PBCCS_ZMW_SUCCESS || o.status == PBCCS_ZMW_POOR_QUALITY) && o.consensus_len > 0) {
            r.Consensus.assign(A[z].cons.data(), (size_t)o.consensus_len);
            r.Qvs.assign(A[z].qvs.begin(), A[z].qvs.begin() + o.consensus_len);
        }
        r.AddReadResults.assign(A[z].arr.begin(), A[z].arr.begin() + nr);
        r.ZScores.assign(A[z].zs.begin(), A[z].zs.begin() + nr);
        r.StatusCounts.assign(o.status_counts, o.status_counts + 5);
        r.GlobalZScore = o.zg;
        r.AvgZScore = o.za;
        r.PredictedAccuracy = o.predicted_accuracy;
        r.Tested = o.n_tested;
        r.Applied = o.n_applied;
        r.NumPasses = o.n_passes;
        r.Windowed = info[z].n_windows > 1;
        r.Fallback = info[z].fallback;
        r.UnanchoredReads = info[z].unanchored_reads;
        for (int x = 0; x < info[z].n_windows && x < info[z].windows_cap; ++x) {
            const pbccs_window_record& q = A[z].recs[x];
            r.Windows.push_back(WindowRecord{q.begin, q.end, q.join, q.cut_begin, q.cut_end, q.status, q.n_tested, q.n_applied});
        }
    }
    return res;
}

}  // namespace CCS
}  // namespace PacBio

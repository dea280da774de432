// pbccs_amd/csrc/capi.hip -- the C ABI (include/pbccs_amd.h) over ArrowBatch.
#include "../../include/pbccs_amd.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <atomic>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <limits>
#include <memory>
#include <mutex>
#include <new>
#include <stdexcept>
#include <string>
#include <thread>
#include <vector>

#include "align_band.hpp"
#include "align_kernels.hpp"
#include "engine.hpp"
#include "driver.hpp"
#include "kinetics_kernels.hpp"
#include "pileup_kernels.hpp"
#include "map_kernels.hpp"
#include "demux_kernels.hpp"
#include "split_map_kernels.hpp"
#include "poa_engine.hpp"
#include "quiver_engine.hpp"
#include "sparse_kernels.hpp"
#include "window_kernels.hpp"

using namespace pbccs;

// ZMW work queue (pbccs_polish_batch): device memory left free beside the batches' band pools (score
// buffers, selection scratch, in-kernel growth headroom), and the largest batch (the best 2 kb batch
// shape measured).
constexpr double kQueueMargin = 24.0 * (1ull << 30);
constexpr int kCcsTailPiece = 250;   // smallest piece of the last ccs chunk's polish (pbccs_ccs_batch)
constexpr int kQueueMaxZmws = 2000;
// readOf entry of a read the caller did not add (NULL sequence): counted in the drop fraction's
// denominator only, as the reads Consensus.h:441-471 skips (POA rejected it, or ExtractMappedRead did)
constexpr int kSkippedRead = -2;

struct pbccs_engine {
    int device = 0;
    Counters counters;
    bool profiling = false;
    KernelStat stats[kKernelKinds];
    // Resident pools.  Batches are dealt round-robin onto `concurrency` workspace slots; batches that
    // share a slot never polish at the same time (pbccs_batch_polish_many runs one slot per thread).
    int concurrency = 4;
    int nextSlot = 0;
    std::mutex statsMu;        // counters / stats are merged from the slots' worker threads
    long long oomRetries = 0;   // device batches rerun after PBCCS_EOOM
    long long repeatSkippedCkpt = 0;   // pbccs_polish_batch_ex: ZMWs whose repeat round a checkpointed read skipped
    DiploidStats diploid;       // the diploid screen's work (pbccs_diploid_stats_get)
    long long strandScreened = 0, strandSites = 0, strandSplit = 0;   // pbccs_strand_stats_get
    long long createHostNs = 0, createUploadNs = 0;   // pbccs_batch_create: host setup / reservations + upload
    std::vector<std::unique_ptr<Workspace>> slots;
    // the POA draft step's device state (made on first use): kPoaSlices runners, one per concurrent slice
    // PBCCS_POA_SLICES overrides the slice count (A/B): more slices overlap one slice's host graph work with
    // the others' device rounds, with fewer host threads each
    static constexpr int kPoaSlicesDefault = 3;   // 1 / 2 / 3 / 4 slices: 1400 / 1527 / 1575 / 1571 ccs ZMWs/s (profiles/r3y_ccs_slices_ab.txt)
    static int PoaSlices()
    {
        static const int n = std::max(1, std::min(8, std::getenv("PBCCS_POA_SLICES") ? std::atoi(std::getenv("PBCCS_POA_SLICES"))
                                                                                      : kPoaSlicesDefault));
        return n;
    }
    std::vector<std::unique_ptr<poa::PoaRunner>> poa;
    std::mutex poaMu;
    poa::PoaRunner& Poa(int k = 0)
    {
        if (poa.empty()) {
            const int hw = std::max(2, std::min(16, (int)std::thread::hardware_concurrency()));
            for (int i = 0; i < PoaSlices(); ++i)
                poa.emplace_back(new poa::PoaRunner(device, std::max(1, hw / PoaSlices())));
        }
        poa[k]->profiling = profiling;
        return *poa[k];
    }
    std::vector<poa::PoaRunner*> PoaRunners()
    {
        std::vector<poa::PoaRunner*> v;
        for (int k = 0; k < PoaSlices(); ++k) v.push_back(&Poa(k));
        return v;
    }
    // pbccs_quiver_polish_batch's scorer batch, kept between calls (Reset per call) so its device buffers and host
    // pools are allocated once; calls on one engine take turns on it
    std::unique_ptr<quiver::QuiverBatch> quiverBatch;
    std::mutex quiverMu;
    // the pairwise aligner's workspace (made on first use): its own stream and move store, apart from the polish
    // slots and the POA pools; calls on one engine take turns on it
    std::unique_ptr<align::AlignRunner> align;
    std::mutex alignMu;
    align::AlignRunner& Align()
    {
        if (!align) align.reset(new align::AlignRunner(device));
        align->profiling = profiling;
        return *align;
    }
    // the draft mapper's workspace (made on first use): its own stream; calls on one engine take turns on it
    std::unique_ptr<map::MapRunner> mapper;
    std::mutex mapMu;
    map::MapRunner& Map()
    {
        if (!mapper) mapper.reset(new map::MapRunner(device));
        mapper->profiling = profiling;
        return *mapper;
    }
    // the split mapper's workspace (made on first use), on the mapper's stream and under mapMu as well
    std::unique_ptr<map::SplitMapRunner> splitMapper;
    map::SplitMapRunner& SplitMap()
    {
        if (!splitMapper) splitMapper.reset(new map::SplitMapRunner(device, Map().stream()));
        splitMapper->profiling = profiling;
        return *splitMapper;
    }
    // SparseAlign's workspace (made on first use): its own stream; calls on one engine take turns on it
    std::unique_ptr<sparse::SparseRunner> sparseRunner;
    std::mutex sparseMu;
    sparse::SparseRunner& Sparse()
    {
        if (!sparseRunner) sparseRunner.reset(new sparse::SparseRunner(device));
        sparseRunner->profiling = profiling;
        return *sparseRunner;
    }
    // the windowed polish's workspace (made on first use): its own stream; calls on one engine take turns on it
    std::unique_ptr<window::WindowRunner> windowRunner;
    std::mutex windowMu;
    pbccs_window_stats windowStats{};
    window::WindowRunner& Window()
    {
        if (!windowRunner) windowRunner.reset(new window::WindowRunner(device));
        return *windowRunner;
    }
    // the kinetics pileup's workspace (made on first use): its own stream; calls on one engine take turns on it
    std::unique_ptr<kinetics::KineticsRunner> kineticsRunner;
    std::mutex kineticsMu;
    kinetics::KineticsRunner& Kinetics()
    {
        if (!kineticsRunner) kineticsRunner.reset(new kinetics::KineticsRunner(device));
        kineticsRunner->profiling = profiling;
        return *kineticsRunner;
    }
    // the base pileup's workspace (made on first use): its own stream; calls on one engine take turns on it
    std::unique_ptr<pileup::PileupRunner> pileupRunner;
    std::mutex pileupMu;
    pileup::PileupRunner& Pileup()
    {
        if (!pileupRunner) pileupRunner.reset(new pileup::PileupRunner(device));
        pileupRunner->profiling = profiling;
        return *pileupRunner;
    }
    // the demultiplexer's workspace (made on first use): its own stream; calls on one engine take turns on it
    std::unique_ptr<demux::DemuxRunner> demuxRunner;
    std::mutex demuxMu;
    demux::DemuxRunner& Demux()
    {
        if (!demuxRunner) demuxRunner.reset(new demux::DemuxRunner(device));
        demuxRunner->profiling = profiling;
        return *demuxRunner;
    }
    Workspace* Slot(int s)
    {
        while ((int)slots.size() <= s) slots.emplace_back(new Workspace(true));
        return slots[s].get();
    }
};

// Owned host copy of a batch's inputs: a batch that ran the device out of memory is rebuilt from it.
struct HostInputs {
    struct Zmw {
        std::string draft;
        std::vector<std::string> seqs;
        std::vector<const char*> seqPtr;
        std::vector<int> lens, strands, ts, te;
        std::vector<unsigned char> full;
    };
    std::vector<Zmw> z;
    std::vector<pbccs_zmw_input> in;   // views into z
    void assign(const pbccs_zmw_input* src, int n)
    {
        z.assign(n, Zmw());
        in.assign(n, pbccs_zmw_input());
        for (int i = 0; i < n; ++i) {
            const pbccs_zmw_input& s = src[i];
            Zmw& d = z[i];
            const int nr = std::max(0, s.n_reads);
            d.draft.assign(s.draft ? s.draft : "", s.draft ? std::max(0, s.draft_len) : 0);
            d.seqs.resize(nr);
            d.lens.assign(nr, 0);
            d.strands.assign(nr, 0);
            d.ts.assign(nr, 0);
            d.te.assign(nr, 0);
            d.full.assign(nr, 1);
            for (int k = 0; k < nr; ++k) {
                d.lens[k] = s.lens[k];
                if (s.seqs[k]) d.seqs[k].assign(s.seqs[k], std::max(0, s.lens[k]));
                d.strands[k] = s.strands[k];
                d.ts[k] = s.tstarts[k];
                d.te[k] = s.tends[k];
                if (s.full_pass) d.full[k] = s.full_pass[k];
            }
            d.seqPtr.resize(nr);
            for (int k = 0; k < nr; ++k) d.seqPtr[k] = s.seqs[k] ? d.seqs[k].c_str() : nullptr;
            pbccs_zmw_input& v = in[i];
            v = s;
            v.draft = d.draft.c_str();
            v.seqs = d.seqPtr.data();
            v.lens = d.lens.data();
            v.strands = d.strands.data();
            v.tstarts = d.ts.data();
            v.tends = d.te.data();
            v.full_pass = d.full.data();
        }
    }
};

struct pbccs_batch {
    HostInputs inputs;
    pbccs_engine* eng = nullptr;
    int slot = 0;
    std::unique_ptr<ArrowBatch> B;
    pbccs_polish_options o;
    int n = 0;
    std::vector<int> zOf;                       // -1: rejected before the device (status in preStatus)
    std::vector<int> preStatus;
    std::vector<int> nReads;
    std::vector<std::vector<int>> readOf;       // -1: read not added (invalid window)
    std::vector<std::vector<unsigned char>> fullPass;
    std::vector<int> allReads;
    bool polished = false;
    // pbccs_polish_batch_ex: RefineRepeats between RefineConsensus and ConsensusQVs
    bool hasRepeats = false;
    pbccs_repeat_options repeats{};
};

struct pbccs_scorer {
    pbccs_engine* eng = nullptr;
    std::unique_ptr<ArrowBatch> batch;
    pbccs_arrow_config cfg;
    int z = 0;
};

namespace {

thread_local std::string g_lastError;

int fail(int code, const char* msg)
{
    g_lastError = msg ? msg : "";
    return code;
}

template <class F>
int guarded(F&& f)
{
    try {
        return f();
    } catch (const DeviceOom& e) {
        return fail(PBCCS_EOOM, e.what());
    } catch (const DeviceError& e) {
        return fail(PBCCS_EDEVICE, e.what());
    } catch (const std::bad_alloc&) {
        return fail(PBCCS_EOOM, "out of memory");
    } catch (const std::invalid_argument& e) {
        return fail(PBCCS_EINVAL, e.what());
    } catch (const std::out_of_range& e) {
        return fail(PBCCS_EINVAL, e.what());
    } catch (const std::exception& e) {
        return fail(PBCCS_EDEVICE, e.what());
    } catch (...) {
        return fail(PBCCS_EDEVICE, "unknown failure");
    }
}

ArrowOptions options_from(const pbccs_arrow_config* c)
{
    ArrowOptions o;
    if (c) {
        o.scoreDiff = c->score_diff;
        o.fastScoreThreshold = c->fast_score_threshold;
        o.addThreshold = c->add_threshold;
    }
    return o;
}

bool to_mutation(const pbccs_mutation& in, int L, Mutation* out)
{
    if (in.type < 0 || in.type > 2) return false;
    const int width = in.end - in.start;
    if (in.type == PBCCS_INSERTION ? width != 0 : width != 1) return false;   // single-base only
    if (in.start < 0) return false;
    if (in.type == PBCCS_INSERTION ? in.start > L : in.start >= L) return false;
    if (in.type != PBCCS_DELETION && !(in.new_base == 'A' || in.new_base == 'C' || in.new_base == 'G' || in.new_base == 'T'))
        return false;
    *out = Mutation::Make(in.type, in.start, in.new_base);
    return true;
}

bool read_scores(int ts, int te, const Mutation& m)   // MultiReadMutationScorer.cpp:70-80
{
    if (m.type == PBCCS_INSERTION) return ts <= m.end && m.start <= te;
    return ts < m.end && m.start < te;
}

}  // namespace

extern "C" {

const char* pbccs_last_error(void) { return g_lastError.c_str(); }

int pbccs_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int pbccs_engine_create(int device, pbccs_engine** out)
{
    if (!out) return fail(PBCCS_EINVAL, "null out");
    return guarded([&] {
        int n = 0;
        if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n)
            return fail(PBCCS_EDEVICE, "no such HIP device");
        if (hipSetDevice(device) != hipSuccess) return fail(PBCCS_EDEVICE, "hipSetDevice failed");
        pbccs_engine* e = new pbccs_engine();
        e->device = device;
        *out = e;
        return PBCCS_OK;
    });
}

void pbccs_engine_destroy(pbccs_engine* eng) { delete eng; }

int pbccs_engine_counters(pbccs_engine* eng, pbccs_counters* out, int reset)
{
    if (!eng || !out) return fail(PBCCS_EINVAL, "null argument");
    out->fill_launches = eng->counters.fillLaunches;
    out->score_launches = eng->counters.scoreLaunches;
    out->score_tasks = eng->counters.scoreTasks;
    out->mutations = eng->counters.mutations;
    out->band_top_bytes = eng->counters.bandTopBytes;
    out->band_region_bytes = eng->counters.bandRegionBytes;
    out->band_used_bytes = eng->counters.bandUsedBytes;
    long long mapped = 0;
    for (const auto& s : eng->slots) mapped += (long long)s->val.mapped_bytes();
    out->pool_mapped_bytes = mapped;
    out->oom_retries = eng->oomRetries;
    out->create_host_ns = eng->createHostNs;
    out->create_upload_ns = eng->createUploadNs;
    out->derive_ns = eng->counters.deriveNs;
    for (int k = 0; k < 16; ++k) out->fill_work[k] = eng->counters.fillWork[k];
    out->scan_reads = eng->counters.scanReads;
    out->uncertain_reads = eng->counters.uncertainReads;
    out->exact_rounds = eng->counters.exactRounds;
    for (int k = 0; k < 4; ++k) out->uncertain_why[k] = eng->counters.uncertainWhy[k];
    out->repeat_skipped_ckpt = eng->repeatSkippedCkpt;
    if (reset) {
        eng->counters = Counters();
        eng->oomRetries = 0;
        eng->repeatSkippedCkpt = 0;
        eng->createHostNs = eng->createUploadNs = 0;
    }
    return PBCCS_OK;
}

// ---- scorer ---------------------------------------------------------------------------------------
int pbccs_scorer_create(pbccs_engine* eng, const pbccs_arrow_config* cfg, const char* tpl, int tpl_len,
                        pbccs_scorer** out)
{
    if (!eng || !cfg || !tpl || tpl_len <= 0 || !out) return fail(PBCCS_EINVAL, "bad argument");
    return guarded([&] {
        std::unique_ptr<pbccs_scorer> s(new pbccs_scorer());
        s->eng = eng;
        s->cfg = *cfg;
        s->batch.reset(new ArrowBatch(eng->device));
        s->z = s->batch->AddZmw(std::string(tpl, tpl_len), cfg->snr, options_from(cfg));
        *out = s.release();
        return PBCCS_OK;
    });
}

void pbccs_scorer_destroy(pbccs_scorer* s) { delete s; }

int pbccs_scorer_add_read(pbccs_scorer* s, const char* seq, int len, int strand, int tstart, int tend,
                          double threshold, int* result)
{
    if (!s || !seq || len < 0 || !result || (strand != 0 && strand != 1)) return fail(PBCCS_EINVAL, "bad argument");
    return guarded([&] {
        ArrowBatch& B = *s->batch;
        const int r = B.AppendRead(s->z, std::string(seq, len), strand, tstart, tend);
        B.FillReads({r});
        *result = B.FinishAddRead(r, threshold);
        return PBCCS_OK;
    });
}

int pbccs_scorer_score_many(pbccs_scorer* s, const pbccs_mutation* m, int n, double fast_threshold, double* scores)
{
    if (!s || (n > 0 && (!m || !scores)) || n < 0) return fail(PBCCS_EINVAL, "bad argument");
    return guarded([&] {
        ArrowBatch& B = *s->batch;
        const int L = (int)B.Template(s->z).size();
        std::vector<std::vector<int>> codes(1);
        for (int i = 0; i < n; ++i) {
            Mutation mu;
            if (!to_mutation(m[i], L, &mu)) return fail(PBCCS_EINVAL, "invalid single-base mutation");
            codes[0].push_back(mutation_code(mu));
        }
        if (n == 0) return PBCCS_OK;
        std::vector<std::vector<double>> sc;
        B.ScoreLists({s->z}, codes, fast_threshold, &sc);
        for (int i = 0; i < n; ++i) scores[i] = sc[0][i];
        return PBCCS_OK;
    });
}

int pbccs_scorer_score(pbccs_scorer* s, const pbccs_mutation* m, double fast_threshold, double* score)
{
    return pbccs_scorer_score_many(s, m, 1, fast_threshold, score);
}

int pbccs_scorer_scores(pbccs_scorer* s, const pbccs_mutation* m, double unscored, double* per_read)
{
    if (!s || !m || !per_read) return fail(PBCCS_EINVAL, "bad argument");
    return guarded([&] {
        ArrowBatch& B = *s->batch;
        Mutation mu;
        if (!to_mutation(*m, (int)B.Template(s->z).size(), &mu)) return fail(PBCCS_EINVAL, "invalid mutation");
        std::vector<std::vector<double>> sc, pr;
        B.ScoreLists({s->z}, {{mutation_code(mu)}}, -std::numeric_limits<double>::max(), &sc, &pr);
        const int nr = B.NumReads(s->z);
        for (int k = 0; k < nr; ++k) {
            const int r = B.ReadIndex(s->z, k);
            const bool scored = B.ReadActive(r) && read_scores(B.ReadTs(r), B.ReadTe(r), mu);
            per_read[k] = scored ? pr[0][k] : unscored;
        }
        return PBCCS_OK;
    });
}

int pbccs_scorer_is_favorable(pbccs_scorer* s, const pbccs_mutation* m, int fast, int* favorable)
{
    if (!s || !favorable) return fail(PBCCS_EINVAL, "bad argument");
    double v = 0.0;
    const double thr = fast ? s->cfg.fast_score_threshold : -std::numeric_limits<double>::max();
    const int rc = pbccs_scorer_score(s, m, thr, &v);
    if (rc != PBCCS_OK) return rc;
    *favorable = v > kMinFavorableScoreDiff ? 1 : 0;
    return PBCCS_OK;
}

int pbccs_scorer_apply_mutations(pbccs_scorer* s, const pbccs_mutation* m, int n)
{
    if (!s || n < 0 || (n > 0 && !m)) return fail(PBCCS_EINVAL, "bad argument");
    return guarded([&] {
        ArrowBatch& B = *s->batch;
        const int L = (int)B.Template(s->z).size();
        std::vector<Mutation> muts;
        for (int i = 0; i < n; ++i) {
            Mutation mu;
            if (!to_mutation(m[i], L, &mu)) return fail(PBCCS_EINVAL, "invalid mutation");
            muts.push_back(mu);
        }
        if (!B.ApplyMutations(s->z, muts)) return fail(PBCCS_EINVAL, "mutation outside the template");
        return PBCCS_OK;
    });
}

int pbccs_scorer_template(pbccs_scorer* s, int strand, char* out, int cap, int* len)
{
    if (!s || !len) return fail(PBCCS_EINVAL, "bad argument");
    const std::string t = strand == PBCCS_FORWARD_STRAND ? s->batch->Template(s->z) : s->batch->TemplateRev(s->z);
    *len = (int)t.size();
    if (!out || cap < (int)t.size() + 1) return fail(PBCCS_ERANGE, "buffer too small");
    std::memcpy(out, t.c_str(), t.size() + 1);
    return PBCCS_OK;
}

int pbccs_scorer_template_length(pbccs_scorer* s) { return s ? (int)s->batch->Template(s->z).size() : -1; }

int pbccs_scorer_num_reads(pbccs_scorer* s) { return s ? s->batch->NumReads(s->z) : -1; }

int pbccs_scorer_read_info(pbccs_scorer* s, int i, int* active, int* strand, int* tstart, int* tend)
{
    if (!s || i < 0 || i >= s->batch->NumReads(s->z)) return fail(PBCCS_EINVAL, "bad read index");
    const int r = s->batch->ReadIndex(s->z, i);
    if (active) *active = s->batch->ReadActive(r) ? 1 : 0;
    if (strand) *strand = s->batch->ReadStrand(r);
    if (tstart) *tstart = s->batch->ReadTs(r);
    if (tend) *tend = s->batch->ReadTe(r);
    return PBCCS_OK;
}

int pbccs_scorer_baseline_score(pbccs_scorer* s, double* score)
{
    if (!s || !score) return fail(PBCCS_EINVAL, "bad argument");
    *score = s->batch->BaselineScore(s->z);
    return PBCCS_OK;
}

int pbccs_scorer_baseline_scores(pbccs_scorer* s, double* out, int cap, int* n)
{
    if (!s || !n) return fail(PBCCS_EINVAL, "bad argument");
    std::vector<double> v;
    for (int k = 0; k < s->batch->NumReads(s->z); ++k) {
        const int r = s->batch->ReadIndex(s->z, k);
        if (s->batch->ReadActive(r)) v.push_back(s->batch->ReadScore(r));
    }
    *n = (int)v.size();
    if (!out || cap < (int)v.size()) return fail(PBCCS_ERANGE, "buffer too small");
    std::copy(v.begin(), v.end(), out);
    return PBCCS_OK;
}

int pbccs_scorer_zscores(pbccs_scorer* s, double* zg, double* za, double* per_read)
{
    if (!s || !zg || !za) return fail(PBCCS_EINVAL, "bad argument");
    std::vector<double> zs;
    s->batch->ZScores(s->z, zg, za, &zs);
    if (per_read) std::copy(zs.begin(), zs.end(), per_read);
    return PBCCS_OK;
}

int pbccs_scorer_num_flipflops(pbccs_scorer* s, int* out)
{
    if (!s || !out) return fail(PBCCS_EINVAL, "bad argument");
    for (int k = 0; k < s->batch->NumReads(s->z); ++k) out[k] = s->batch->ReadFlips(s->batch->ReadIndex(s->z, k));
    return PBCCS_OK;
}

int pbccs_refine_consensus(pbccs_scorer* s, const pbccs_refine_options* opts, long long* n_tested,
                           long long* n_applied, int* converged)
{
    if (!s || !n_tested || !n_applied || !converged) return fail(PBCCS_EINVAL, "bad argument");
    return guarded([&] {
        RefineOptions ro;
        if (opts) {
            ro.maxIterations = opts->max_iterations;
            ro.mutationSeparation = opts->mutation_separation;
            ro.mutationNeighborhood = opts->mutation_neighborhood;
        }
        std::vector<int> conv;
        std::vector<long long> nt, na;
        s->batch->Refine({s->z}, ro, &conv, &nt, &na);
        *n_tested += nt[0];
        *n_applied += na[0];
        if (conv[0] < 0) return fail(PBCCS_EINVAL, "mutation could not be applied");
        *converged = conv[0];
        return PBCCS_OK;
    });
}

int pbccs_consensus_qvs(pbccs_scorer* s, int* qvs, int cap, int* n)
{
    if (!s || !n) return fail(PBCCS_EINVAL, "bad argument");
    return guarded([&] {
        std::vector<std::vector<int>> q;
        s->batch->QVs({s->z}, &q);
        *n = (int)q[0].size();
        if (!qvs || cap < *n) return fail(PBCCS_ERANGE, "buffer too small");
        std::copy(q[0].begin(), q[0].end(), qvs);
        return PBCCS_OK;
    });
}

// ---- per-base rich QVs ------------------------------------------------------------------
// One ZMW's rich arrays into the caller's buffers; false (len = -required) when they are too small.
static bool write_rich(pbccs_rich_qvs* r, const RichQVs& v)
{
    const int L = (int)v.subQv.size();
    if (r->cap < L || (L > 0 && (!r->sub_qv || !r->ins_qv || !r->del_qv || !r->sub_tag || !r->ins_tag))) {
        r->len = -L;
        return false;
    }
    std::copy(v.subQv.begin(), v.subQv.end(), r->sub_qv);
    std::copy(v.insQv.begin(), v.insQv.end(), r->ins_qv);
    std::copy(v.delQv.begin(), v.delQv.end(), r->del_qv);
    std::copy(v.subTag.begin(), v.subTag.end(), r->sub_tag);
    std::copy(v.insTag.begin(), v.insTag.end(), r->ins_tag);
    r->len = L;
    return true;
}

int pbccs_consensus_qvs_rich(pbccs_scorer* s, int* qvs, pbccs_rich_qvs* rich, int* n)
{
    if (!s || !n || !rich) return fail(PBCCS_EINVAL, "bad argument");
    return guarded([&] {
        std::vector<std::vector<int>> q;
        std::vector<RichQVs> r;
        s->batch->QVs({s->z}, &q, &r);
        *n = (int)q[0].size();
        if (!qvs || !write_rich(rich, r[0])) {
            rich->len = -*n;
            return fail(PBCCS_ERANGE, "buffer too small");
        }
        std::copy(q[0].begin(), q[0].end(), qvs);
        return PBCCS_OK;
    });
}

// ---- batched polish -------------------------------------------------------------------------------
void pbccs_polish_options_default(pbccs_polish_options* o)
{
    if (!o) return;
    o->min_passes = 3;
    o->min_length = 10;
    o->min_zscore = -5.0;
    o->max_drop_fraction = 0.34;
    o->min_predicted_accuracy = 0.90;
    o->score_diff = 12.5;
    o->refine.max_iterations = 40;
    o->refine.mutation_separation = 10;
    o->refine.mutation_neighborhood = 20;
    o->zmws_per_batch = 0;
}

// Merge a batch's counters and profile into its engine.  Never throws: it runs in worker threads and on
// the way out of the C ABI (a device error while resolving events only loses that batch's timings).
static void merge_engine_stats(pbccs_engine* eng, ArrowBatch& B)
{
    std::lock_guard<std::mutex> lk(eng->statsMu);
    try {
        const Counters& c = B.counters();
        eng->counters.fillLaunches += c.fillLaunches;
        eng->counters.scoreLaunches += c.scoreLaunches;
        eng->counters.scoreTasks += c.scoreTasks;
        eng->counters.mutations += c.mutations;
        eng->counters.deriveNs += c.deriveNs;
        eng->counters.scanReads += c.scanReads;
        eng->counters.uncertainReads += c.uncertainReads;
        eng->counters.exactRounds += c.exactRounds;
        for (int k = 0; k < 4; ++k) eng->counters.uncertainWhy[k] += c.uncertainWhy[k];
        for (int k = 0; k < 16; ++k) eng->counters.fillWork[k] += c.fillWork[k];
        eng->counters.bandTopBytes = std::max(eng->counters.bandTopBytes, c.bandTopBytes);
        eng->counters.bandRegionBytes = std::max(eng->counters.bandRegionBytes, c.bandRegionBytes);
        eng->counters.bandUsedBytes = std::max(eng->counters.bandUsedBytes, c.bandUsedBytes);
        B.ResetCounters();
        B.CollectProfile(eng->stats);
    } catch (...) {
        (void)hipGetLastError();
    }
}

// A batch on an explicit workspace slot (slot < 0: the next slot round-robin).
static int create_batch(pbccs_engine* eng, const pbccs_zmw_input* in, int n, const pbccs_polish_options* opts,
                        int slot, pbccs_batch** out, const pbccs_repeat_options* repeats = nullptr)
{
    if (!eng || n < 0 || (n > 0 && !in) || !out) return fail(PBCCS_EINVAL, "bad argument");
    return guarded([&] {
        if (hipSetDevice(eng->device) != hipSuccess) return fail(PBCCS_EDEVICE, "hipSetDevice failed");
        const auto t0 = std::chrono::steady_clock::now();
        std::unique_ptr<pbccs_batch> b(new pbccs_batch());
        b->eng = eng;
        pbccs_polish_options_default(&b->o);
        if (opts) b->o = *opts;
        b->n = n;
        if (repeats) {
            b->hasRepeats = true;
            b->repeats = *repeats;
        }
        b->slot = slot >= 0 ? slot : eng->nextSlot++ % std::max(1, eng->concurrency);
        b->inputs.assign(in, n);
        // every batch gets its own streams (ArrowBatch's ownStreams); a batch made and polished on its slot's thread
        // (slot >= 0: the queue, the ccs chunks, reruns) uses the slot's descriptor arena and read pool
        // PBCCS_SLOT_STREAMS=1 (debug / A/B): the slot workspace's persistent streams instead
        // (read per batch: a test switches it at run time)
        const bool slotStreams = std::getenv("PBCCS_SLOT_STREAMS") && std::getenv("PBCCS_SLOT_STREAMS")[0] == '1';
        b->B.reset(new ArrowBatch(eng->device, eng->Slot(b->slot), !slotStreams, slot >= 0));
        b->B->SetProfiling(eng->profiling);
        ArrowOptions ao;
        ao.scoreDiff = b->o.score_diff;
        b->zOf.assign(n, -1);
        b->preStatus.assign(n, PBCCS_ZMW_OTHER);
        b->nReads.assign(n, 0);
        b->readOf.assign(n, {});
        b->fullPass.assign(n, {});
        for (int i = 0; i < n; ++i) {
            const pbccs_zmw_input& z = in[i];
            b->nReads[i] = z.n_reads;
            if (z.n_reads <= 0) { b->preStatus[i] = PBCCS_ZMW_NO_SUBREADS; continue; }
            if (z.draft_len < b->o.min_length) { b->preStatus[i] = PBCCS_ZMW_TOO_SHORT; continue; }
            const std::string draft(z.draft, z.draft_len);
            if (!is_acgt(draft)) { b->preStatus[i] = PBCCS_ZMW_OTHER; continue; }
            b->zOf[i] = b->B->AddZmw(draft, z.snr, ao);
            for (int k = 0; k < z.n_reads; ++k) {
                int r = -1;
                if (!z.seqs[k]) r = kSkippedRead;   // not added (Consensus.h:448-451): denominator only
                else if (z.tstarts[k] >= 0 && z.tends[k] <= z.draft_len && z.tstarts[k] < z.tends[k] && z.lens[k] > 0)
                    r = b->B->AppendRead(b->zOf[i], std::string(z.seqs[k], z.lens[k]), z.strands[k] ? 1 : 0,
                                         z.tstarts[k], z.tends[k]);
                b->readOf[i].push_back(r);
                b->fullPass[i].push_back(z.full_pass ? z.full_pass[k] : 1);
                if (r >= 0) b->allReads.push_back(r);
            }
        }
        const auto t1 = std::chrono::steady_clock::now();
        b->B->Prepare();
        const auto t2 = std::chrono::steady_clock::now();
        {
            std::lock_guard<std::mutex> lk(eng->statsMu);
            eng->createHostNs += std::chrono::duration_cast<std::chrono::nanoseconds>(t1 - t0).count();
            eng->createUploadNs += std::chrono::duration_cast<std::chrono::nanoseconds>(t2 - t1).count();
        }
        *out = b.release();
        return PBCCS_OK;
    });
}

int pbccs_batch_create(pbccs_engine* eng, const pbccs_zmw_input* in, int n, const pbccs_polish_options* opts,
                       pbccs_batch** out)
{
    return create_batch(eng, in, n, opts, -1, out);
}

void pbccs_batch_destroy(pbccs_batch* b) { delete b; }

// repTested / repApplied (b->n entries each, may be NULL): RefineRepeats' counts of a batch made with repeats
// rich (b->n entries, may be NULL): the rich QVs of each ZMW beside its qvs (k_qv_rich instead of k_qv)
// The strand screen of a span: its thresholds and, per ZMW, where its sites go.
struct StrandScreen {
    StrandOptions opt;
    std::vector<StrandSiteH>* const* sites = nullptr;   // one vector per ZMW of the span (left empty without QVs)
};

static int polish_one(pbccs_batch* b, pbccs_zmw_output* out, long long* repTested = nullptr,
                      long long* repApplied = nullptr, pbccs_rich_qvs* rich = nullptr,
                      const StrandScreen* strand = nullptr)
{
    if (!b || (b->n > 0 && !out)) return fail(PBCCS_EINVAL, "bad argument");
    if (b->polished) return fail(PBCCS_ESTATE, "a batch polishes once");
    if (!b->B) return fail(PBCCS_ESTATE, "the batch's device state was released");
    return guarded([&] {
        if (hipSetDevice(b->eng->device) != hipSuccess) return fail(PBCCS_EDEVICE, "hipSetDevice failed");
        b->polished = true;
        ArrowBatch& B = *b->B;
        const pbccs_polish_options& o = b->o;
        const int n = b->n;
        for (int i = 0; i < n; ++i) {
            pbccs_zmw_output& q = out[i];
            q.status = b->preStatus[i];
            q.consensus_len = 0;
            q.zg = q.za = std::numeric_limits<double>::quiet_NaN();
            q.predicted_accuracy = 0.0;
            q.n_tested = q.n_applied = 0;
            q.n_passes = 0;
            for (int k = 0; k < 5; ++k) q.status_counts[k] = 0;
            for (int k = 0; k < b->nReads[i]; ++k) {
                if (q.add_read_results) q.add_read_results[k] = -1;
                if (q.zscores) q.zscores[k] = std::numeric_limits<double>::quiet_NaN();
            }
        }
        // PBCCS_RECLAIM=1: bands of ZMWs the batch is done with are dropped as it goes and every refill relays
        // the value pool out (ArrowBatch::Relayout), with ConsensusQVs run in the round a ZMW
        // converges.  Opt-in: it cuts the refine rounds' band top (42.5 -> 39.9 GB per 2000-ZMW batch; the
        // initial fill sets the high-water) but the per-round QVs cost 5.5% (profiles/r2h5_reclaim_ab)
        const char* reclaimEnv = std::getenv("PBCCS_RECLAIM");
        // (the repeat round reads the converged ZMWs' bands after the refine loop: no reclaim with it)
        const bool reclaim = reclaimEnv && std::strcmp(reclaimEnv, "1") == 0 && !b->hasRepeats;
        B.SetReclaim(reclaim);
        // the certified fast path for the batch's tall reads; PBCCS_CERTIFIED_SCAN=0: exact fills only
        const char* ce = std::getenv("PBCCS_CERTIFIED_SCAN");   // read per batch: tests switch it at run time
        // (k_score_wide's scores carry no deviation bound: a batch with a repeat round fills exactly)
        const bool certified = (!ce || ce[0] != '0') && !b->hasRepeats;
        B.SetCertifiedScan(certified);
        B.FillReads(b->allReads);
        B.CertifyAddReads(b->allReads, o.min_zscore);
        std::vector<int> refineZ, refineIdx, dropZ;
        for (int i = 0; i < n; ++i) {
            if (b->zOf[i] < 0) continue;
            pbccs_zmw_output& q = out[i];
            int nPasses = 0, nDropped = 0;
            for (int k = 0; k < b->nReads[i]; ++k) {
                const int r = b->readOf[i][k];
                if (r == kSkippedRead) continue;
                const int st = (r >= 0) ? B.FinishAddRead(r, o.min_zscore) : PBCCS_ADD_OTHER;
                if (q.add_read_results) q.add_read_results[k] = st;
                q.status_counts[st] += 1;
                if (st == PBCCS_ADD_SUCCESS && b->fullPass[i][k]) ++nPasses;
                else if (st != PBCCS_ADD_SUCCESS) ++nDropped;
            }
            q.n_passes = nPasses;
            if (nPasses < o.min_passes) {
                q.status = PBCCS_ZMW_TOO_FEW_PASSES;
                dropZ.push_back(b->zOf[i]);
                continue;
            }
            const double frac = (double)nDropped / b->nReads[i];
            if (frac > o.max_drop_fraction) {
                q.status = PBCCS_ZMW_TOO_MANY_UNUSABLE;
                dropZ.push_back(b->zOf[i]);
                continue;
            }
            std::vector<double> zs;
            B.ZScores(b->zOf[i], &q.zg, &q.za, &zs);
            if (q.zscores) {
                int j = 0;
                for (int k = 0; k < b->nReads[i]; ++k)
                    if (b->readOf[i][k] >= 0) q.zscores[k] = zs[j++];
            }
            refineZ.push_back(b->zOf[i]);
            refineIdx.push_back(i);
        }
        RefineOptions ro;
        ro.maxIterations = o.refine.max_iterations;
        ro.mutationSeparation = o.refine.mutation_separation;
        ro.mutationNeighborhood = o.refine.mutation_neighborhood;
        B.Retire(dropZ);
        std::vector<int> conv;
        std::vector<long long> nt, na;
        // ConsensusQVs (Consensus.h:496-512) run inside the refine loop, in the round each ZMW converges
        std::vector<std::vector<int>> qvAll;
        std::vector<RichQVs> richAll, richQ;
        std::vector<std::vector<StrandSiteH>> strandAll, strandQ;
        B.Refine(refineZ, ro, &conv, &nt, &na, false, reclaim ? &qvAll : nullptr, reclaim && rich ? &richAll : nullptr,
                 strand ? &strand->opt : nullptr, reclaim && strand ? &strandAll : nullptr);
        if (strand)
            for (int i = 0; i < n; ++i) strand->sites[i]->clear();
        std::vector<int> qvZ, qvIdx;
        std::vector<std::vector<int>> qvs;
        if (rich)
            for (int i = 0; i < n; ++i) rich[i].len = 0;
        for (size_t k = 0; k < refineZ.size(); ++k) {
            pbccs_zmw_output& q = out[refineIdx[k]];
            q.n_tested = nt[k];
            q.n_applied = na[k];
            if (conv[k] == 1) {
                qvZ.push_back(refineZ[k]);
                qvIdx.push_back(refineIdx[k]);
                if (reclaim) qvs.push_back(std::move(qvAll[k]));
                if (reclaim && rich) richQ.push_back(std::move(richAll[k]));
                if (reclaim && strand) strandQ.push_back(std::move(strandAll[k]));
            } else q.status = conv[k] < 0 ? PBCCS_ZMW_OTHER : PBCCS_ZMW_NON_CONVERGENT;
        }
        for (int i = 0; i < n; ++i) {
            if (repTested) repTested[i] = 0;
            if (repApplied) repApplied[i] = 0;
        }
        if (b->hasRepeats && !qvZ.empty()) {
            // RefineRepeats on the ZMWs RefineConsensus converged on, in lock-step rounds; a ZMW with a read on
            // checkpointed bands skips it (status 3) and finishes as it would without the repeat round
            RefineOptions rr;
            rr.maxIterations = b->repeats.max_iterations;
            rr.mutationSeparation = b->repeats.mutation_separation;
            rr.mutationNeighborhood = b->repeats.mutation_neighborhood;
            std::vector<long long> rt, ra;
            std::vector<char> rconv;
            std::vector<int> rst;
            B.RefineRepeats(qvZ, b->repeats.repeat_length, b->repeats.min_repeat_elements, rr, &rt, &ra, &rconv, &rst);
            std::vector<int> keepZ, keepIdx;
            std::vector<std::vector<StrandSiteH>> keepStrand;
            long long skipped = 0;
            for (size_t k = 0; k < qvZ.size(); ++k) {
                if (repTested) repTested[qvIdx[k]] = rt[k];
                if (repApplied) repApplied[qvIdx[k]] = ra[k];
                if (rst[k] == 3) ++skipped;
                if (rst[k] == 1 || rst[k] == 2) {
                    out[qvIdx[k]].status = PBCCS_ZMW_OTHER;
                    continue;
                }
                keepZ.push_back(qvZ[k]);
                keepIdx.push_back(qvIdx[k]);
                if (reclaim && strand) keepStrand.push_back(std::move(strandQ[k]));
            }
            qvZ.swap(keepZ);
            qvIdx.swap(keepIdx);
            if (reclaim && strand) strandQ.swap(keepStrand);
            if (skipped) {
                std::lock_guard<std::mutex> lk(b->eng->statsMu);
                b->eng->repeatSkippedCkpt += skipped;
            }
        }
        if (!reclaim) B.QVs(qvZ, &qvs, rich ? &richQ : nullptr, strand ? &strand->opt : nullptr, strand ? &strandQ : nullptr);
        for (size_t k = 0; k < qvZ.size(); ++k) {
            pbccs_zmw_output& q = out[qvIdx[k]];
            const std::string& t = B.Template(qvZ[k]);
            double acc = 0.0;   // Consensus.h:506-512
            for (int v : qvs[k]) acc += std::pow(10.0, static_cast<double>(v) / -10.0);
            acc = 1.0 - acc / qvs[k].size();
            q.predicted_accuracy = acc;
            if ((int)t.size() + 1 > q.consensus_cap || !q.consensus) {
                q.consensus_len = -(int)t.size();
                q.status = PBCCS_ZMW_OTHER;
                continue;
            }
            std::memcpy(q.consensus, t.c_str(), t.size() + 1);
            q.consensus_len = (int)t.size();
            if (rich && !write_rich(&rich[qvIdx[k]], richQ[k])) {   // as a consensus buffer that is too small
                q.status = PBCCS_ZMW_OTHER;
                continue;
            }
            if (q.qvs) std::copy(qvs[k].begin(), qvs[k].end(), q.qvs);
            q.status = (acc < o.min_predicted_accuracy) ? PBCCS_ZMW_POOR_QUALITY : PBCCS_ZMW_SUCCESS;
            if (strand) *strand->sites[qvIdx[k]] = std::move(strandQ[k]);
        }
        return PBCCS_OK;
    });
}

// Create, polish, account and destroy one device batch of m ZMWs on `slot`.
static int polish_span(pbccs_engine* eng, int slot, const pbccs_zmw_input* in, int m, const pbccs_polish_options* o,
                       pbccs_zmw_output* out, const pbccs_repeat_options* repeats = nullptr,
                       long long* repTested = nullptr, long long* repApplied = nullptr, pbccs_rich_qvs* rich = nullptr,
                       const StrandScreen* strand = nullptr)
{
    pbccs_batch* h = nullptr;
    int r = create_batch(eng, in, m, o, slot, &h, repeats);
    if (r == PBCCS_OK) r = polish_one(h, out, repTested, repApplied, rich, strand);
    if (h) {
        if (h->B) merge_engine_stats(eng, *h->B);
        pbccs_batch_destroy(h);
    }
    return r;
}

// Rerun ZMWs whose batch ran the device out of memory, alone on `slot` once the other slots have drained
// and every slot's band pool is unmapped; a span that still does not fit is halved.  A ZMW's result does
// not depend on the batch it polishes in (the engine's only cross-ZMW state is the launch grouping), so
// the retry changes the schedule and nothing else.  Outputs land in out[0..n) in input order.
static int polish_retry(pbccs_engine* eng, int slot, const pbccs_zmw_input* in, int n, const pbccs_polish_options* o,
                        pbccs_zmw_output* out, const pbccs_repeat_options* repeats = nullptr,
                        long long* repTested = nullptr, long long* repApplied = nullptr, pbccs_rich_qvs* rich = nullptr,
                        const StrandScreen* strand = nullptr)
{
    std::vector<std::pair<int, int>> todo{{0, n}};
    // the slot's outgrown buffers go back to the device before the rerun (nothing of the slot is queued: its batches
    // were destroyed, and the pools were unmapped with the device synchronised)
    eng->Slot(slot)->TrimRetired();
    while (!todo.empty()) {
        const std::pair<int, int> span = todo.back();
        todo.pop_back();
        {
            std::lock_guard<std::mutex> lk(eng->statsMu);
            eng->oomRetries += 1;
        }
        StrandScreen sub;
        if (strand) {
            sub.opt = strand->opt;
            sub.sites = strand->sites + span.first;
        }
        const int r = polish_span(eng, slot, in + span.first, span.second - span.first, o, out + span.first, repeats,
                                  repTested ? repTested + span.first : nullptr,
                                  repApplied ? repApplied + span.first : nullptr,
                                  rich ? rich + span.first : nullptr, strand ? &sub : nullptr);
        if (r == PBCCS_OK) continue;
        if (r != PBCCS_EOOM || span.second - span.first < 2) return r;
        eng->Slot(slot)->val.unmap_all();
        const int mid = span.first + (span.second - span.first) / 2;
        todo.emplace_back(mid, span.second);
        todo.emplace_back(span.first, mid);
    }
    return PBCCS_OK;
}

int pbccs_batch_polish(pbccs_batch* b, pbccs_zmw_output* out)
{
    int rc = polish_one(b, out);
    if (b && b->B) merge_engine_stats(b->eng, *b->B);
    if (rc == PBCCS_EOOM && b) {   // alone on the device already: free this slot's pool and rerun, halving
        b->B.reset();
        b->eng->Slot(b->slot)->val.unmap_all();
        rc = polish_retry(b->eng, b->slot, b->inputs.in.data(), b->n, &b->o, out);
    }
    return rc;
}

int pbccs_batch_polish_many(pbccs_batch* const* batches, int n, pbccs_zmw_output* const* outs)
{
    if (n < 0 || (n > 0 && (!batches || !outs))) return fail(PBCCS_EINVAL, "bad argument");
    if (n == 0) return PBCCS_OK;
    pbccs_engine* eng = batches[0] ? batches[0]->eng : nullptr;
    for (int i = 0; i < n; ++i)
        if (!batches[i] || batches[i]->eng != eng || (batches[i]->n > 0 && !outs[i]))
            return fail(PBCCS_EINVAL, "batches must be non-null and belong to one engine");
    // one host thread (and HIP stream: each ArrowBatch owns one) per workspace slot
    std::vector<std::vector<int>> bySlot;
    for (int i = 0; i < n; ++i) {
        const int s = batches[i]->slot;
        if ((int)bySlot.size() <= s) bySlot.resize(s + 1);
        bySlot[s].push_back(i);
    }
    std::vector<int> rc(n, PBCCS_OK);
    std::vector<std::string> err(n);
    std::vector<std::thread> pool;
    for (const std::vector<int>& list : bySlot) {
        if (list.empty()) continue;
        pool.emplace_back([&, list] {
            for (int i : list) {   // polish_one and merge_engine_stats never throw
                rc[i] = polish_one(batches[i], outs[i]);
                if (rc[i] != PBCCS_OK) err[i] = g_lastError;
                if (batches[i]->B) merge_engine_stats(eng, *batches[i]->B);
            }
        });
    }
    for (std::thread& t : pool) t.join();
    // Batches that ran the device out of memory while the other slots held their pools are rebuilt from
    // their inputs and rerun one at a time, after every slot's pool is unmapped (halved while they still do
    // not fit).
    std::vector<int> deferred;
    for (int i = 0; i < n; ++i)
        if (rc[i] == PBCCS_EOOM) deferred.push_back(i);
    if (!deferred.empty()) {
        for (int i : deferred) batches[i]->B.reset();
        for (size_t s = 0; s < eng->slots.size(); ++s) eng->slots[s]->val.unmap_all();
        for (int i : deferred) {
            pbccs_batch* b = batches[i];
            rc[i] = polish_retry(eng, b->slot, b->inputs.in.data(), b->n, &b->o, outs[i]);
            if (rc[i] != PBCCS_OK) err[i] = g_lastError;
        }
    }
    for (int i = 0; i < n; ++i)
        if (rc[i] != PBCCS_OK) return fail(rc[i], err[i].c_str());
    return PBCCS_OK;
}

int pbccs_engine_set_concurrency(pbccs_engine* eng, int batches_in_flight)
{
    if (!eng || batches_in_flight < 1 || batches_in_flight > 64) return fail(PBCCS_EINVAL, "bad argument");
    eng->concurrency = batches_in_flight;
    return PBCCS_OK;
}

int pbccs_engine_reserve_pool(pbccs_engine* eng, size_t bytes_per_slot)
{
    if (!eng) return fail(PBCCS_EINVAL, "bad argument");
    return guarded([&] {
        if (hipSetDevice(eng->device) != hipSuccess) return fail(PBCCS_EDEVICE, "hipSetDevice failed");
        for (int s = 0; s < std::max(1, eng->concurrency); ++s) {
            VmPool& v = eng->Slot(s)->val;
            v.reserve(std::max<size_t>(bytes_per_slot / sizeof(double), 1), true);
            // touch the mapped memory once here, so first-use costs of fresh device pages are not paid by
            // the first fills that land on them
            if (hipMemsetAsync(v.ptr, 0, v.cap * sizeof(double), nullptr) != hipSuccess)
                return fail(PBCCS_EDEVICE, "hipMemset of the band pool failed");
        }
        if (hipDeviceSynchronize() != hipSuccess) return fail(PBCCS_EDEVICE, "device synchronisation failed");
        return PBCCS_OK;
    });
}

// ---- ZMW work queue ------------------------------------------------------------------------------
// Estimated FP64 band footprint of one ZMW at its high-water mark (zmw_est_bytes below).  Per read: two band
// regions of ~32 rows x window plus column metadata (the typical band), plus the expected share of bands that
// explode on the reband, whose fraction of the (I+1)(J+1) matrix grows with the window (oracle band statistics,
// DESIGN.md §6).  Checks: 2 kb / 10 passes ~19 MB (measured 13.5 MB, profiles/r2h6_regrow_slots), 10 kb / 8 passes
// ~150 MB with checkpointed bands (measured 142 MB: 68 GB for 480 ZMWs, profiles/r3b_bench_10kb_ckpt8.json),
// 20 kb ~120 MB per read (the round-4 estimate, 63 MB, let 8 slots run the device out of memory 27 times on the
// configs[3] mix).
// Band-pool bytes the workspace slots hold mapped.
static size_t slot_pool_bytes(pbccs_engine* eng)
{
    size_t b = 0;
    for (const auto& s : eng->slots) b += s->val.mapped_bytes();
    return b;
}

static double zmw_est_bytes(const pbccs_zmw_input& z)
{
    int K = 0, minLen = 0;
    ckpt_policy(&K, &minLen);
    double b = 0.0;
    for (int k = 0; k < z.n_reads; ++k) {
        const double J = std::max(1, z.tends ? z.tends[k] - (z.tstarts ? z.tstarts[k] : 0) : z.draft_len);
        const double I = z.lens ? std::max(0, z.lens[k]) : J;
        const double cells = (I + 1) * (J + 1);
        // the typical band: the first regions ((J + 66) x 16 values per matrix) and the column metadata
        const double typical = J * 0.5 * (2 * 32 * 8 * 1.25 + 80 + 8 * 8);
        // bands that explode on the 4%-of-matrix reband: the oracle's AddRead stores, per matrix, a mean fraction
        // of the (I+1)(J+1) matrix over all reads that grows with the window -- 0.023 / 0.044 / 0.074 / 0.098 at
        // 5 / 10 / 15 / 20 kb (6 reads each; 1 / 2 / 4 / 4 of them exploded to 0.05-0.21) -- held in exact regions
        // (+1/16 slack, regrow_bands), plus the tall reads' abandoned first regions (4% of the matrix, pt of the
        // reads: ~1 in 10 at 2 kb, 2 in 3 at 15-20 kb)
        const double frac = std::min(0.12, 0.005 * J / 1000.0);
        const double pt = std::min(0.7, 0.08 + J / 30000.0);
        double tall = 2.0 * 8.0 * frac * cells * (1.0 + 1.0 / 16) + pt * 2.0 * 8.0 * cells / 25.0;
        // checkpointed tall bands: every K-th column plus the kept tails of both matrices
        if (K > 0 && J >= minLen) tall = tall / K + pt * 2.0 * 8.0 * (kCkptTail + 1) * (I + 1);
        b += typical + tall;
    }
    // the refine rounds' per-ZMW buffers beside the bands: ~9 unique single-base mutations per template base
    // (Prepare's unique_mutation_count + 64), each with a code, a score, a flag and one delta per read (dDelta_:
    // 43 MB for a 20 kb template with 30 reads, which the band-only estimate missed: 5 OOM retries in the 2000-ZMW
    // configs[3] run, profiles/r5_mixed_2000_s8.json)
    const double L = std::max(1, z.draft_len);
    b += (9.0 * L + 64.0) * (8.0 * std::max(1, z.n_reads) + 13.0);
    return std::max(b, 4096.0);
}

int pbccs_plan_batches(const pbccs_zmw_input* in, int n, double budget_bytes, int max_per_batch,
                       double max_len_ratio, int* order, int* batch_start, double* est_bytes, int* n_batches)
{
    if (n < 0 || (n > 0 && (!in || !order || !batch_start)) || !n_batches || max_per_batch < 1 ||
        !(budget_bytes > 0) || !(max_len_ratio >= 1.0))
        return fail(PBCCS_EINVAL, "bad argument");
    std::vector<double> est(n);
    std::vector<int> idx(n);
    for (int i = 0; i < n; ++i) {
        est[i] = zmw_est_bytes(in[i]);
        idx[i] = i;
        if (est_bytes) est_bytes[i] = est[i];
    }
    // length buckets (then pass count): similar windows share launches, whose LDS and band heights are
    // sized by their longest read; the input index breaks ties so the plan is deterministic
    std::stable_sort(idx.begin(), idx.end(), [&](int a, int b) {
        if (in[a].draft_len != in[b].draft_len) return in[a].draft_len < in[b].draft_len;
        return in[a].n_reads < in[b].n_reads;
    });
    struct Span { int b, e; double bytes; };
    std::vector<Span> spans;
    for (int k = 0; k < n;) {
        Span s{k, k, 0.0};
        const double first = std::max(1, in[idx[k]].draft_len);
        while (s.e < n) {
            const int z = idx[s.e];
            const bool room = s.e - s.b < max_per_batch && s.bytes + est[z] <= budget_bytes &&
                              in[z].draft_len <= max_len_ratio * first;
            if (!room && s.e > s.b) break;   // a ZMW over budget on its own still gets a batch
            s.bytes += est[z];
            ++s.e;
        }
        spans.push_back(s);
        k = s.e;
    }
    // longest templates first, then largest: a batch's time is its rounds' latency, which grows with the template
    // (the tall reads' column sweeps), not with its bytes -- most batches of a mixed input are capped at the same
    // budget, and ordered by bytes the 15-20 kb batches started last and left four of eight slots idle for the last
    // third of a configs[3] run (profiles/r9ze_mixed_slot_gaps.json); the queue's tail is then made of short batches
    std::vector<int> spanLen(spans.size());
    for (size_t k = 0; k < spans.size(); ++k) spanLen[k] = in[idx[spans[k].e - 1]].draft_len;   // ascending inside
    std::vector<size_t> so(spans.size());
    for (size_t k = 0; k < so.size(); ++k) so[k] = k;
    std::stable_sort(so.begin(), so.end(), [&](size_t a, size_t b) {
        if (spanLen[a] != spanLen[b]) return spanLen[a] > spanLen[b];
        return spans[a].bytes > spans[b].bytes;
    });
    std::vector<Span> sorted;
    for (size_t k : so) sorted.push_back(spans[k]);
    spans.swap(sorted);
    int o = 0;
    for (size_t b = 0; b < spans.size(); ++b) {
        batch_start[b] = o;
        for (int k = spans[b].b; k < spans[b].e; ++k) order[o++] = idx[k];
    }
    batch_start[spans.size()] = o;
    *n_batches = (int)spans.size();
    return PBCCS_OK;
}

// pbccs_polish_batch (repeats == NULL) and pbccs_polish_batch_ex: the ZMW work queue
static int polish_batch_impl(pbccs_engine* eng, const pbccs_zmw_input* in, int n, const pbccs_polish_options* opts,
                             const pbccs_repeat_options* repeats, long long* repTested, long long* repApplied,
                             pbccs_zmw_output* out, pbccs_rich_qvs* rich = nullptr,
                             const StrandOptions* strandOpt = nullptr,
                             std::vector<std::vector<StrandSiteH>>* strandSites = nullptr)
{
    if (!eng || n < 0 || (n > 0 && (!in || !out))) return fail(PBCCS_EINVAL, "bad argument");
    if (n == 0) return PBCCS_OK;
    if (!(strandOpt && strandSites)) strandOpt = nullptr;
    if (strandOpt) strandSites->assign(n, {});
    pbccs_polish_options o;
    pbccs_polish_options_default(&o);
    if (opts) o = *opts;
    const int slots = std::max(1, eng->concurrency);
    std::vector<int> order(n), start(n + 1);
    int nb = 0;
    if (o.zmws_per_batch > 0) {   // caller-sized consecutive chunks
        for (int i = 0; i < n; ++i) order[i] = i;
        for (int b0 = 0; b0 < n; b0 += o.zmws_per_batch) start[nb++] = b0;
        start[nb] = n;
    } else {
        size_t freeB = 0, totalB = 0;
        if (hipSetDevice(eng->device) != hipSuccess || hipMemGetInfo(&freeB, &totalB) != hipSuccess)
            return fail(PBCCS_EDEVICE, "hipMemGetInfo failed");
        // every slot polishes at once: split what is free beyond the growth margin between them (the slots'
        // mapped band pools count as free: a batch on the slot reuses them)
        const double spare = std::max(0.0, (double)freeB + (double)slot_pool_bytes(eng) - (double)kQueueMargin);
        // PBCCS_QUEUE_BUDGET_SCALE (A/B): the per-slot budget against the planner's per-ZMW estimates
        const char* bs = std::getenv("PBCCS_QUEUE_BUDGET_SCALE");
        const double budget = std::max(1.0 * (1 << 30), 0.9 * spare / slots) * (bs ? std::max(0.1, std::atof(bs)) : 1.0);
        int rc = pbccs_plan_batches(in, n, budget, kQueueMaxZmws, 1.5, order.data(), start.data(), nullptr, &nb);
        if (rc != PBCCS_OK) return rc;
        // a last wave with fewer batches than slots leaves slots idle through its whole polish: cap the batch
        // size so the batches come in whole waves (smaller batches stay within the per-slot budget); small
        // inputs keep their plan, since batches of under ~256 ZMWs pay the per-round latency for too few
        if (nb % slots != 0 && n >= 256 * slots) {
            const int waves = (nb + slots - 1) / slots;
            const int per = std::max(1, (n + waves * slots - 1) / (waves * slots));
            rc = pbccs_plan_batches(in, n, budget, std::min(per, kQueueMaxZmws), 1.5, order.data(), start.data(),
                                    nullptr, &nb);
            if (rc != PBCCS_OK) return rc;
        }
    }
    // the workspace slots exist before the workers start (Slot() grows a shared vector)
    for (int s = 0; s < slots; ++s) eng->Slot(s);
    std::atomic<int> next{0};
    std::atomic<bool> stop{false};
    std::vector<int> rc(slots, PBCCS_OK);
    std::vector<std::string> err(slots);
    // a span [b, e) of `order`: inputs gathered, outputs scattered back to input order (also on failure:
    // the output structs only point at the caller's buffers)
    auto gather = [&](int b, int e, std::vector<pbccs_zmw_input>* bin, std::vector<pbccs_zmw_output>* bout) {
        bin->resize(e - b);
        bout->resize(e - b);
        for (int k = 0; k < e - b; ++k) {
            (*bin)[k] = in[order[b + k]];
            (*bout)[k] = out[order[b + k]];
        }
    };
    auto scatter = [&](int b, int e, const std::vector<pbccs_zmw_output>& bout) {
        for (int k = 0; k < e - b; ++k) out[order[b + k]] = bout[k];
    };
    // the rich-QV structs of a span (they point at the caller's buffers, as the outputs do)
    auto gather_rich = [&](int b, int e, std::vector<pbccs_rich_qvs>* br) {
        br->resize(rich ? e - b : 0);
        for (int k = 0; rich && k < e - b; ++k) (*br)[k] = rich[order[b + k]];
    };
    // the strand screen of a span: the sites land in the caller's per-ZMW vectors directly
    auto gather_strand = [&](int b, int e, std::vector<std::vector<StrandSiteH>*>* bs, StrandScreen* sc) {
        bs->resize(strandOpt ? e - b : 0);
        for (int k = 0; strandOpt && k < e - b; ++k) (*bs)[k] = &(*strandSites)[order[b + k]];
        if (strandOpt) sc->opt = *strandOpt;
        sc->sites = bs->data();
    };
    auto scatter_rich = [&](int b, int e, const std::vector<pbccs_rich_qvs>& br) {
        for (int k = 0; rich && k < e - b; ++k) rich[order[b + k]] = br[k];
    };
    // RefineRepeats' counts of a span, back to input order
    auto scatter_counts = [&](int b, int e, const std::vector<long long>& rt, const std::vector<long long>& ra) {
        for (int k = 0; k < e - b; ++k) {
            if (repTested) repTested[order[b + k]] = rt[k];
            if (repApplied) repApplied[order[b + k]] = ra[k];
        }
    };
    // Batches that ran the device out of memory while the other slots held theirs are deferred and rerun
    // one at a time once every slot's pool is unmapped (polish_retry).
    std::mutex deferMu;
    std::vector<std::pair<int, int>> deferred;
    auto worker = [&](int slot) {
        std::vector<pbccs_zmw_input> bin;
        std::vector<pbccs_zmw_output> bout;
        std::vector<long long> brt, bra;
        std::vector<pbccs_rich_qvs> brich;
        std::vector<std::vector<StrandSiteH>*> bstrand;
        StrandScreen screen;
        for (;;) {
            const int b = next.fetch_add(1);
            if (b >= nb || stop.load()) return;
            int r = PBCCS_OK;
            try {
                gather(start[b], start[b + 1], &bin, &bout);
                gather_rich(start[b], start[b + 1], &brich);
                gather_strand(start[b], start[b + 1], &bstrand, &screen);
                if (repeats) {
                    brt.assign(start[b + 1] - start[b], 0);
                    bra.assign(start[b + 1] - start[b], 0);
                }
            } catch (...) {
                r = fail(PBCCS_EOOM, "out of host memory");
            }
            if (r == PBCCS_OK)
                r = polish_span(eng, slot, bin.data(), start[b + 1] - start[b], &o, bout.data(), repeats,
                                repeats ? brt.data() : nullptr, repeats ? bra.data() : nullptr,
                                rich ? brich.data() : nullptr, strandOpt ? &screen : nullptr);
            if (r == PBCCS_OK) {
                scatter(start[b], start[b + 1], bout);
                scatter_rich(start[b], start[b + 1], brich);
                if (repeats) scatter_counts(start[b], start[b + 1], brt, bra);
            } else if (r == PBCCS_EOOM) {
                std::lock_guard<std::mutex> lk(deferMu);
                deferred.emplace_back(start[b], start[b + 1]);
                double est = 0.0;   // one line per deferred batch: what the plan expected, what ran out
                for (const pbccs_zmw_input& z : bin) est += zmw_est_bytes(z);
                std::fprintf(stderr, "[queue] batch %d (%d ZMWs, estimated %.1f GB) deferred on slot %d: %s\n", b,
                             start[b + 1] - start[b], est / 1e9, slot, g_lastError.c_str());
            } else {
                rc[slot] = r;
                err[slot] = g_lastError;
                stop.store(true);
                return;
            }
        }
    };
    std::vector<std::thread> pool;
    for (int s = 0; s < std::min(slots, nb); ++s) pool.emplace_back(worker, s);
    for (std::thread& t : pool) t.join();
    // every batch of the call is destroyed (its streams synchronised): the slots' outgrown buffers can go
    for (int s = 0; s < slots; ++s) eng->Slot(s)->TrimRetired();
    for (int s = 0; s < slots; ++s)
        if (rc[s] != PBCCS_OK) return fail(rc[s], err[s].c_str());
    if (!deferred.empty()) {
        for (int s = 0; s < slots; ++s) eng->Slot(s)->val.unmap_all();
        std::sort(deferred.begin(), deferred.end());
        return guarded([&] {
            std::vector<pbccs_zmw_input> bin;
            std::vector<pbccs_zmw_output> bout;
            std::vector<pbccs_rich_qvs> brich;
            std::vector<std::vector<StrandSiteH>*> bstrand;
            StrandScreen screen;
            for (const std::pair<int, int>& span : deferred) {
                gather(span.first, span.second, &bin, &bout);
                gather_rich(span.first, span.second, &brich);
                gather_strand(span.first, span.second, &bstrand, &screen);
                std::vector<long long> brt(span.second - span.first, 0), bra(span.second - span.first, 0);
                const int r = polish_retry(eng, 0, bin.data(), span.second - span.first, &o, bout.data(), repeats,
                                           repeats ? brt.data() : nullptr, repeats ? bra.data() : nullptr,
                                           rich ? brich.data() : nullptr, strandOpt ? &screen : nullptr);
                if (r != PBCCS_OK) return r;
                scatter(span.first, span.second, bout);
                scatter_rich(span.first, span.second, brich);
                if (repeats) scatter_counts(span.first, span.second, brt, bra);
            }
            return PBCCS_OK;
        });
    }
    return PBCCS_OK;
}

int pbccs_polish_batch(pbccs_engine* eng, const pbccs_zmw_input* in, int n, const pbccs_polish_options* opts,
                       pbccs_zmw_output* out)
{
    return polish_batch_impl(eng, in, n, opts, nullptr, nullptr, nullptr, out);
}

int pbccs_polish_batch_ex(pbccs_engine* eng, const pbccs_zmw_input* in, int n, const pbccs_polish_options* opts,
                          const pbccs_repeat_options* repeats, long long* repeat_tested, long long* repeat_applied,
                          pbccs_zmw_output* out)
{
    if (repeats && (repeats->repeat_length < 1 || repeats->repeat_length > PBCCS_MAX_MUTATION_BASES))
        return fail(PBCCS_EINVAL, "repeat_length must be 1..7");
    return polish_batch_impl(eng, in, n, opts, repeats, repeats ? repeat_tested : nullptr,
                             repeats ? repeat_applied : nullptr, out);
}

int pbccs_polish_batch_ex2(pbccs_engine* eng, const pbccs_zmw_input* in, int n, const pbccs_polish_options* opts,
                           const pbccs_polish_extras* extras, pbccs_zmw_output* out)
{
    const pbccs_polish_extras none{};
    const pbccs_polish_extras& x = extras ? *extras : none;
    if (x.repeats && (x.repeats->repeat_length < 1 || x.repeats->repeat_length > PBCCS_MAX_MUTATION_BASES))
        return fail(PBCCS_EINVAL, "repeat_length must be 1..7");
    return polish_batch_impl(eng, in, n, opts, x.repeats, x.repeats ? x.repeat_tested : nullptr,
                             x.repeats ? x.repeat_applied : nullptr, out, x.rich);
}

// ---- directional consensus ----------------------------------------------------------------
void pbccs_strand_options_default(pbccs_strand_options* o)
{
    if (!o) return;
    o->min_score = 12.5;
    o->min_reads = 2;
    o->min_sites = 1;
    o->directional = 0;
}

static bool strand_options_ok(const pbccs_strand_options& o)
{
    return o.min_score >= 0.0 && o.min_reads >= 0 && o.min_sites >= 0 && o.directional >= 0 && o.directional <= 2;
}

static StrandOptions strand_engine_options(const pbccs_strand_options& o)
{
    StrandOptions e;
    e.minScore = o.min_score;
    e.minReads = o.min_reads;
    return e;
}

// After a joint polish that ran the screen (sites[i]: ZMW i's sites): the sites into sres[i]'s buffers, the split
// decision, and the split ZMWs' single-strand inputs, forward then reverse per ZMW, through the same batch path
// together.  sres[i].fwd / rev take per-read entries by position in in[i]'s reads.  PBCCS_ERANGE (after every output
// is written) when a ZMW's site buffers are too small.
static int strand_finish(pbccs_engine* eng, const pbccs_zmw_input* in, int n, const pbccs_polish_options* opts,
                         const pbccs_repeat_options* repeats, const pbccs_strand_options& so,
                         const std::vector<std::vector<StrandSiteH>>& sites, const pbccs_zmw_output* out,
                         pbccs_strand_result* sres)
{
    return guarded([&] {
        bool range = false;
        long long screened = 0, nSites = 0;
        std::vector<int> split;
        for (int i = 0; i < n; ++i) {
            pbccs_strand_result& r = sres[i];
            const bool hasQvs = out[i].status == PBCCS_ZMW_SUCCESS || out[i].status == PBCCS_ZMW_POOR_QUALITY;
            if (!hasQvs) continue;
            ++screened;
            const std::vector<StrandSiteH>& v = sites[i];
            const int m = (int)v.size();
            nSites += m;
            if (m > r.cap || (m > 0 && (!r.position || !r.type || !r.base || !r.sum_fwd || !r.sum_rev))) {
                r.n_sites = -m;
                range = true;
            } else {
                for (int k = 0; k < m; ++k) {
                    r.position[k] = v[k].pos;
                    r.type[k] = v[k].type;
                    r.base[k] = v[k].base;
                    r.sum_fwd[k] = v[k].sumF;
                    r.sum_rev[k] = v[k].sumR;
                }
                r.n_sites = m;
            }
            if (so.directional == 2 || (so.directional == 1 && m >= so.min_sites)) split.push_back(i);
        }
        const int ns = (int)split.size();
        struct Sub {
            std::vector<const char*> seqs;
            std::vector<int> lens, strands, ts, te, idx, arr;
            std::vector<unsigned char> fp;
            std::vector<double> zs;
        };
        std::vector<Sub> subs(2 * ns);
        std::vector<pbccs_zmw_input> sin(2 * ns);
        std::vector<pbccs_zmw_output> sout(2 * ns);
        for (int q = 0; q < 2 * ns; ++q) {
            const int i = split[q / 2], want = q & 1;
            const pbccs_zmw_input& z = in[i];
            Sub& u = subs[q];
            for (int k = 0; k < z.n_reads; ++k) {
                if ((z.strands[k] ? 1 : 0) != want) continue;
                u.seqs.push_back(z.seqs[k]);
                u.lens.push_back(z.lens[k]);
                u.strands.push_back(z.strands[k]);
                u.ts.push_back(z.tstarts[k]);
                u.te.push_back(z.tends[k]);
                u.fp.push_back(z.full_pass ? z.full_pass[k] : 1);
                u.idx.push_back(k);
            }
            u.arr.assign(u.idx.size() + 1, -1);
            u.zs.assign(u.idx.size() + 1, std::numeric_limits<double>::quiet_NaN());
            pbccs_zmw_input& s = sin[q];
            s = z;
            s.n_reads = (int)u.idx.size();
            s.seqs = u.seqs.data();
            s.lens = u.lens.data();
            s.strands = u.strands.data();
            s.tstarts = u.ts.data();
            s.tends = u.te.data();
            s.full_pass = u.fp.data();
            pbccs_zmw_output& o = sout[q];
            o = want ? sres[i].rev : sres[i].fwd;
            o.add_read_results = u.arr.data();
            o.zscores = u.zs.data();
        }
        if (ns > 0) {
            std::vector<long long> rt(2 * ns, 0), ra(2 * ns, 0);
            const int r2 = polish_batch_impl(eng, sin.data(), 2 * ns, opts, repeats, repeats ? rt.data() : nullptr,
                                             repeats ? ra.data() : nullptr, sout.data());
            if (r2 != PBCCS_OK) return r2;
        }
        for (int q = 0; q < 2 * ns; ++q) {
            const int i = split[q / 2];
            pbccs_zmw_output& dst = (q & 1) ? sres[i].rev : sres[i].fwd;
            int* const arr = dst.add_read_results;
            double* const zs = dst.zscores;
            dst = sout[q];
            dst.add_read_results = arr;
            dst.zscores = zs;
            // per-read entries indexed like the joint record's: -1 / NaN for the other strand's reads
            for (int k = 0; k < in[i].n_reads; ++k) {
                if (arr) arr[k] = -1;
                if (zs) zs[k] = std::numeric_limits<double>::quiet_NaN();
            }
            const Sub& u = subs[q];
            for (size_t j = 0; j < u.idx.size(); ++j) {
                if (arr) arr[u.idx[j]] = u.arr[j];
                if (zs) zs[u.idx[j]] = u.zs[j];
            }
            sres[i].split = 1;
        }
        {
            std::lock_guard<std::mutex> lk(eng->statsMu);
            eng->strandScreened += screened;
            eng->strandSites += nSites;
            eng->strandSplit += ns;
        }
        return range ? fail(PBCCS_ERANGE, "strand site buffers too small") : PBCCS_OK;
    });
}

int pbccs_polish_batch_strand(pbccs_engine* eng, const pbccs_zmw_input* in, int n, const pbccs_polish_options* opts,
                              const pbccs_polish_extras* extras, const pbccs_strand_options* strand,
                              pbccs_strand_result* strand_out, pbccs_zmw_output* out)
{
    if (!eng || n < 0 || (n > 0 && (!in || !out || !strand_out))) return fail(PBCCS_EINVAL, "bad argument");
    const pbccs_polish_extras none{};
    const pbccs_polish_extras& x = extras ? *extras : none;
    if (x.repeats && (x.repeats->repeat_length < 1 || x.repeats->repeat_length > PBCCS_MAX_MUTATION_BASES))
        return fail(PBCCS_EINVAL, "repeat_length must be 1..7");
    pbccs_strand_options so;
    pbccs_strand_options_default(&so);
    if (strand) so = *strand;
    if (!strand_options_ok(so))
        return fail(PBCCS_EINVAL, "strand options: min_score, min_reads, min_sites >= 0, directional 0..2");
    for (int i = 0; i < n; ++i) {
        if (in[i].n_reads > 0 && !in[i].strands) return fail(PBCCS_EINVAL, "bad pbccs_zmw_input");
        strand_out[i].n_sites = 0;
        strand_out[i].split = 0;
    }
    const StrandOptions eo = strand_engine_options(so);
    std::vector<std::vector<StrandSiteH>> sites;
    const int rc = polish_batch_impl(eng, in, n, opts, x.repeats, x.repeats ? x.repeat_tested : nullptr,
                                     x.repeats ? x.repeat_applied : nullptr, out, x.rich, &eo, &sites);
    if (rc != PBCCS_OK) return rc;
    return strand_finish(eng, in, n, opts, x.repeats, so, sites, out, strand_out);
}

int pbccs_scorer_strand_scores(pbccs_scorer* s, const pbccs_mutation* m, int n, double* sum_fwd, double* sum_rev,
                               int* n_fwd, int* n_rev)
{
    if (!s || n < 0 || (n > 0 && (!m || !sum_fwd || !sum_rev || !n_fwd || !n_rev))) return fail(PBCCS_EINVAL, "bad argument");
    return guarded([&] {
        ArrowBatch& B = *s->batch;
        const int L = (int)B.Template(s->z).size();
        std::vector<int> codes;
        for (int i = 0; i < n; ++i) {
            Mutation mu;
            if (!to_mutation(m[i], L, &mu)) return fail(PBCCS_EINVAL, "invalid single-base mutation");
            codes.push_back(mutation_code(mu));
        }
        StrandSumsH h;
        B.StrandScores(s->z, codes, &h);
        for (int i = 0; i < n; ++i) {
            sum_fwd[i] = h.sumF[i];
            sum_rev[i] = h.sumR[i];
            n_fwd[i] = h.nF[i];
            n_rev[i] = h.nR[i];
        }
        return PBCCS_OK;
    });
}

int pbccs_scorer_strand_sites(pbccs_scorer* s, const pbccs_strand_options* opts, int* position, int* type, char* base,
                              double* sum_fwd, double* sum_rev, int cap, int* n)
{
    if (!s || !n || cap < 0) return fail(PBCCS_EINVAL, "bad argument");
    pbccs_strand_options so;
    pbccs_strand_options_default(&so);
    if (opts) so = *opts;
    if (!strand_options_ok(so)) return fail(PBCCS_EINVAL, "strand options: min_score, min_reads >= 0");
    return guarded([&] {
        StrandOptions eo;
        eo.minScore = so.min_score;
        eo.minReads = so.min_reads;
        std::vector<std::vector<int>> q;
        std::vector<std::vector<StrandSiteH>> v;
        s->batch->QVs({s->z}, &q, nullptr, &eo, &v);
        *n = (int)v[0].size();
        if (*n > cap || (*n > 0 && (!position || !type || !base || !sum_fwd || !sum_rev)))
            return fail(PBCCS_ERANGE, "buffer too small");
        for (int k = 0; k < *n; ++k) {
            position[k] = v[0][k].pos;
            type[k] = v[0][k].type;
            base[k] = v[0][k].base;
            sum_fwd[k] = v[0][k].sumF;
            sum_rev[k] = v[0][k].sumR;
        }
        return PBCCS_OK;
    });
}

int pbccs_strand_stats_get(pbccs_engine* eng, pbccs_strand_stats* out, int reset)
{
    if (!eng || !out) return fail(PBCCS_EINVAL, "null argument");
    std::lock_guard<std::mutex> lock(eng->statsMu);
    out->strand_screened = eng->strandScreened;
    out->strand_sites = eng->strandSites;
    out->strand_split = eng->strandSplit;
    if (reset) eng->strandScreened = eng->strandSites = eng->strandSplit = 0;
    return PBCCS_OK;
}

int pbccs_engine_set_profiling(pbccs_engine* eng, int on)
{
    if (!eng) return fail(PBCCS_EINVAL, "null engine");
    eng->profiling = on != 0;
    return PBCCS_OK;
}

int pbccs_engine_kernel_stats(pbccs_engine* eng, pbccs_kernel_stat* out, int cap, int* n, int reset)
{
    if (!eng || !n) return fail(PBCCS_EINVAL, "bad argument");
    *n = kKernelKinds;
    if (!out || cap < kKernelKinds) return fail(PBCCS_ERANGE, "buffer too small");
    for (int k = 0; k < kKernelKinds; ++k) {
        std::memset(out[k].name, 0, sizeof(out[k].name));
        std::strncpy(out[k].name, kKernelNames[k], sizeof(out[k].name) - 1);
        out[k].launches = eng->stats[k].launches;
        out[k].device_ms = eng->stats[k].ms;
        out[k].cells = eng->stats[k].cells;
        out[k].bytes = eng->stats[k].bytes;
        out[k].wave_s = eng->stats[k].waveTicks / 1e8;   // s_memrealtime runs at 100 MHz
        if (reset) eng->stats[k] = KernelStat();
    }
    return PBCCS_OK;
}

}  // extern "C"

// ================================================================ Quiver family
#include "quiver_engine.hpp"

struct pbccs_quiver_scorer {
    pbccs_engine* eng = nullptr;
    std::unique_ptr<quiver::QuiverBatch> batch;
    std::vector<std::pair<std::string, int>> table;   // QuiverConfigTable: chemistry -> config index
    std::vector<pbccs_quiver_config> cfgs;
    int z = 0;
};

namespace {

quiver::QParams qparams(const pbccs_quiver_config& c)
{
    quiver::QParams p;
    const pbccs_qv_model_params& m = c.params;
    p.Match = m.match;
    p.Mismatch = m.mismatch;
    p.MismatchS = m.mismatch_s;
    p.Branch = m.branch;
    p.BranchS = m.branch_s;
    p.DeletionN = m.deletion_n;
    p.DeletionWithTag = m.deletion_with_tag;
    p.DeletionWithTagS = m.deletion_with_tag_s;
    p.Nce = m.nce;
    p.NceS = m.nce_s;
    for (int k = 0; k < 4; ++k) {
        p.Merge[k] = m.merge[k];
        p.MergeS[k] = m.merge_s[k];
    }
    p.scoreDiff = c.score_diff;
    p.fastThreshold = c.fast_score_threshold;
    p.addThreshold = c.add_threshold;
    p.moves = c.moves_available;
    p.sumProduct = c.sum_product ? 1 : 0;
    p.simple = (c.recursor == PBCCS_QV_RECURSOR_SPARSE_SIMPLE || c.recursor == PBCCS_QV_RECURSOR_DENSE_SIMPLE) ? 1 : 0;
    p.dense = (c.recursor == PBCCS_QV_RECURSOR_DENSE_SSE || c.recursor == PBCCS_QV_RECURSOR_DENSE_SIMPLE) ? 1 : 0;
    return p;
}

// Quiver mutations may lie past the template end: no read scores them (ReadScoresMutation, :60-71)
bool to_quiver_mutation(const pbccs_mutation& in, Mutation* out)
{
    if (in.type < 0 || in.type > 2 || in.start < 0) return false;
    const int width = in.end - in.start;
    if (in.type == PBCCS_INSERTION ? width != 0 : width != 1) return false;   // single-base only
    if (in.type != PBCCS_DELETION && !(in.new_base == 'A' || in.new_base == 'C' || in.new_base == 'G' || in.new_base == 'T'))
        return false;
    *out = Mutation::Make(in.type, in.start, in.new_base);
    return true;
}

int quiver_codes(const pbccs_mutation* m, int n, std::vector<int>* codes)
{
    for (int i = 0; i < n; ++i) {
        Mutation mu;
        if (!to_quiver_mutation(m[i], &mu)) return fail(PBCCS_EINVAL, "invalid single-base mutation");
        codes->push_back(mutation_code(mu));
    }
    return PBCCS_OK;
}

// pbccs_mutation_ex -> MutationEx; acgtOnly: the template-editing calls
bool to_mutation_ex(const pbccs_mutation_ex& in, bool acgtOnly, bool anyBase, MutationEx* out)
{
    if (in.type < 0 || in.type > 2 || in.start < 0 || in.n_bases < 0) return false;
    out->type = in.type;
    out->start = in.start;
    out->end = in.end;
    out->bases.clear();
    if (in.type != PBCCS_DELETION) {
        if (in.n_bases > 0 && !in.new_bases) return false;
        out->bases.assign(in.new_bases ? in.new_bases : "", (size_t)in.n_bases);
    }
    if (!out->Valid()) return false;
    if (anyBase) return true;
    if ((int)out->bases.size() > PBCCS_MAX_MUTATION_BASES) return false;
    for (char c : out->bases) {
        const bool acgt = c == 'A' || c == 'C' || c == 'G' || c == 'T';
        if (!acgt && (acgtOnly || !(c == 'M' || c == 'N'))) return false;
    }
    return true;
}

int quiver_mutations_ex(const pbccs_mutation_ex* m, int n, bool acgtOnly, std::vector<MutationEx>* out)
{
    for (int i = 0; i < n; ++i) {
        MutationEx mu;
        if (!to_mutation_ex(m[i], acgtOnly, false, &mu)) return fail(PBCCS_EINVAL, "invalid multi-base mutation");
        out->push_back(mu);
    }
    return PBCCS_OK;
}

// the scoring calls' common front: parse, then the 8-column rule, before any launch
int quiver_scorable_ex(pbccs_quiver_scorer* s, const pbccs_mutation_ex* m, int n, std::vector<MutationEx>* out)
{
    if (quiver_mutations_ex(m, n, false, out) != PBCCS_OK) return PBCCS_EINVAL;
    if (!s->batch->ColumnsFit(s->z, *out))
        return fail(PBCCS_EINVAL, "mutation needs more than 8 extend-buffer columns on some read");
    return PBCCS_OK;
}

}  // namespace

extern "C" {

int pbccs_quiver_scorer_create(pbccs_engine* eng, const pbccs_quiver_config* configs, const char* const* chemistries,
                               int n_configs, const char* tpl, int tpl_len, pbccs_quiver_scorer** out)
{
    if (!eng || !configs || n_configs < 1 || !tpl || tpl_len <= 0 || !out) return fail(PBCCS_EINVAL, "bad argument");
    for (int k = 0; k < n_configs; ++k)
        if (configs[k].recursor < PBCCS_QV_RECURSOR_SPARSE_SSE || configs[k].recursor > PBCCS_QV_RECURSOR_DENSE_SIMPLE)
            return fail(PBCCS_EINVAL, "unknown recursor type");
    return guarded([&] {
        std::unique_ptr<pbccs_quiver_scorer> s(new pbccs_quiver_scorer());
        s->eng = eng;
        s->batch.reset(new quiver::QuiverBatch(eng->device));
        float fast = 0.0f;   // min over the table, starting at 0 (:129-135)
        for (int k = 0; k < n_configs; ++k) {
            const std::string name = (chemistries && chemistries[k]) ? chemistries[k] : "*";
            bool dup = false;
            for (auto& kv : s->table) dup = dup || kv.first == name;
            if (dup) continue;   // InsertAs_ keeps the first entry of a name (QuiverConfig.cpp:67-78)
            s->table.emplace_back(name, s->batch->AddConfig(qparams(configs[k])));
            s->cfgs.push_back(configs[k]);
            fast = std::min(fast, configs[k].fast_score_threshold);
        }
        s->z = s->batch->AddZmw(std::string(tpl, tpl_len), fast);
        *out = s.release();
        return PBCCS_OK;
    });
}

void pbccs_quiver_scorer_destroy(pbccs_quiver_scorer* s) { delete s; }

int pbccs_quiver_scorer_add_read(pbccs_quiver_scorer* s, const char* seq, int len, const float* ins_qv,
                                 const float* subs_qv, const float* del_qv, const float* del_tag,
                                 const float* merge_qv, const char* chemistry, int strand, int tstart, int tend,
                                 float threshold, int* active)
{
    if (!s || !seq || len <= 0 || !active || (strand != 0 && strand != 1)) return fail(PBCCS_EINVAL, "bad argument");
    return guarded([&] {
        // QuiverConfigTable::At: exact chemistry, else "*" (QuiverConfig.cpp:112-127)
        const std::string chem = chemistry ? chemistry : "*";
        int cfg = -1;
        size_t pos = 0;
        for (size_t k = 0; k < s->table.size(); ++k)
            if (s->table[k].first == chem) { cfg = s->table[k].second; pos = k; }
        if (cfg < 0)
            for (size_t k = 0; k < s->table.size(); ++k)
                if (s->table[k].first == "*") { cfg = s->table[k].second; pos = k; }
        if (cfg < 0) return fail(PBCCS_EINVAL, "Chemistry not found in QuiverConfigTable");
        quiver::QReadFeatures f;
        f.seq.assign(seq, len);
        auto track = [&](std::vector<float>& v, const float* src) {
            v.assign(len, 0.0f);
            if (src) std::copy(src, src + len, v.begin());
        };
        track(f.ins, ins_qv);
        track(f.subs, subs_qv);
        track(f.del, del_qv);
        track(f.tag, del_tag);
        track(f.merge, merge_qv);
        const float thr = std::isnan(threshold) ? s->cfgs[pos].add_threshold : threshold;
        *active = s->batch->AddRead(s->z, f, strand, tstart, tend, cfg, thr) ? 1 : 0;
        return PBCCS_OK;
    });
}

int pbccs_quiver_scorer_score_many(pbccs_quiver_scorer* s, const pbccs_mutation* m, int n, int fast, float* scores)
{
    if (!s || n < 0 || (n > 0 && (!m || !scores))) return fail(PBCCS_EINVAL, "bad argument");
    return guarded([&] {
        std::vector<int> codes;
        if (quiver_codes(m, n, &codes) != PBCCS_OK) return PBCCS_EINVAL;
        std::vector<float> d;
        s->batch->Deltas(s->z, codes, &d);
        for (int i = 0; i < n; ++i) scores[i] = s->batch->Score(s->z, d, i, fast != 0);
        return PBCCS_OK;
    });
}

int pbccs_quiver_scorer_read_score_mutation(pbccs_quiver_scorer* s, int i, const pbccs_mutation* m, float* score)
{
    if (!s || !m || !score || i < 0 || i >= s->batch->NumReads(s->z)) return fail(PBCCS_EINVAL, "bad argument");
    return guarded([&] {
        std::vector<int> codes;
        if (quiver_codes(m, 1, &codes) != PBCCS_OK) return PBCCS_EINVAL;
        *score = s->batch->ReadScoreMutation(s->batch->ReadIndex(s->z, i), codes[0]);
        return PBCCS_OK;
    });
}

int pbccs_quiver_scorer_scores(pbccs_quiver_scorer* s, const pbccs_mutation* m, float unscored, float* per_read)
{
    if (!s || !m || !per_read) return fail(PBCCS_EINVAL, "bad argument");
    return guarded([&] {
        std::vector<int> codes;
        if (quiver_codes(m, 1, &codes) != PBCCS_OK) return PBCCS_EINVAL;
        std::vector<float> d;
        s->batch->Deltas(s->z, codes, &d);
        const int nr = s->batch->NumReads(s->z);
        for (int k = 0; k < nr; ++k) per_read[k] = std::isnan(d[k]) ? unscored : d[k];
        return PBCCS_OK;
    });
}

int pbccs_quiver_scorer_is_favorable(pbccs_quiver_scorer* s, const pbccs_mutation* m, int fast, int* favorable)
{
    if (!s || !m || !favorable) return fail(PBCCS_EINVAL, "bad argument");
    return guarded([&] {
        std::vector<int> codes;
        if (quiver_codes(m, 1, &codes) != PBCCS_OK) return PBCCS_EINVAL;
        std::vector<float> d;
        s->batch->Deltas(s->z, codes, &d);
        *favorable = fast ? (s->batch->FastIsFavorable(s->z, d, 0) ? 1 : 0)
                          : ((double)s->batch->Score(s->z, d, 0, false) > 0.04 ? 1 : 0);
        return PBCCS_OK;
    });
}

int pbccs_quiver_scorer_apply_mutations(pbccs_quiver_scorer* s, const pbccs_mutation* m, int n)
{
    if (!s || n < 0 || (n > 0 && !m)) return fail(PBCCS_EINVAL, "bad argument");
    return guarded([&] {
        std::vector<Mutation> muts;
        for (int i = 0; i < n; ++i) {
            Mutation mu;
            if (!to_quiver_mutation(m[i], &mu)) return fail(PBCCS_EINVAL, "invalid mutation");
            muts.push_back(mu);
        }
        if (!s->batch->ApplyMutations(s->z, muts)) return fail(PBCCS_EINVAL, "mutation outside the template");
        return PBCCS_OK;
    });
}

int pbccs_quiver_scorer_score_many_ex(pbccs_quiver_scorer* s, const pbccs_mutation_ex* m, int n, int fast,
                                      float* scores)
{
    if (!s || n < 0 || (n > 0 && (!m || !scores))) return fail(PBCCS_EINVAL, "bad argument");
    return guarded([&] {
        std::vector<MutationEx> muts;
        if (quiver_scorable_ex(s, m, n, &muts) != PBCCS_OK) return PBCCS_EINVAL;
        std::vector<float> d;
        s->batch->DeltasEx(s->z, muts, &d);
        for (int i = 0; i < n; ++i) scores[i] = s->batch->Score(s->z, d, i, fast != 0);
        return PBCCS_OK;
    });
}

int pbccs_quiver_scorer_scores_ex(pbccs_quiver_scorer* s, const pbccs_mutation_ex* m, float unscored,
                                  float* per_read)
{
    if (!s || !m || !per_read) return fail(PBCCS_EINVAL, "bad argument");
    return guarded([&] {
        std::vector<MutationEx> muts;
        if (quiver_scorable_ex(s, m, 1, &muts) != PBCCS_OK) return PBCCS_EINVAL;
        std::vector<float> d;
        s->batch->DeltasEx(s->z, muts, &d);
        const int nr = s->batch->NumReads(s->z);
        for (int k = 0; k < nr; ++k) per_read[k] = std::isnan(d[k]) ? unscored : d[k];
        return PBCCS_OK;
    });
}

int pbccs_quiver_scorer_is_favorable_ex(pbccs_quiver_scorer* s, const pbccs_mutation_ex* m, int fast,
                                        int* favorable)
{
    if (!s || !m || !favorable) return fail(PBCCS_EINVAL, "bad argument");
    return guarded([&] {
        std::vector<MutationEx> muts;
        if (quiver_scorable_ex(s, m, 1, &muts) != PBCCS_OK) return PBCCS_EINVAL;
        std::vector<float> d;
        s->batch->DeltasEx(s->z, muts, &d);
        *favorable = fast ? (s->batch->FastIsFavorable(s->z, d, 0) ? 1 : 0)
                          : ((double)s->batch->Score(s->z, d, 0, false) > 0.04 ? 1 : 0);
        return PBCCS_OK;
    });
}

int pbccs_quiver_scorer_read_score_mutation_ex(pbccs_quiver_scorer* s, int i, const pbccs_mutation_ex* m,
                                               float* score)
{
    if (!s || !m || !score || i < 0 || i >= s->batch->NumReads(s->z)) return fail(PBCCS_EINVAL, "bad argument");
    return guarded([&] {
        std::vector<MutationEx> muts;
        if (quiver_mutations_ex(m, 1, false, &muts) != PBCCS_OK) return PBCCS_EINVAL;
        if (!s->batch->ReadScoreMutationEx(s->batch->ReadIndex(s->z, i), muts[0], score))
            return fail(PBCCS_EINVAL, "mutation outside the read's window or needing more than 8 columns");
        return PBCCS_OK;
    });
}

int pbccs_quiver_scorer_apply_mutations_ex(pbccs_quiver_scorer* s, const pbccs_mutation_ex* m, int n)
{
    if (!s || n < 0 || (n > 0 && !m)) return fail(PBCCS_EINVAL, "bad argument");
    return guarded([&] {
        std::vector<MutationEx> muts;
        if (quiver_mutations_ex(m, n, true, &muts) != PBCCS_OK) return PBCCS_EINVAL;
        if (!s->batch->ApplyMutationsEx(s->z, muts)) return fail(PBCCS_EINVAL, "mutation outside the template");
        return PBCCS_OK;
    });
}

int pbccs_quiver_refine_repeats(pbccs_quiver_scorer* s, const pbccs_repeat_options* opts, long long* n_tested,
                                long long* n_applied, int* converged)
{
    if (!s || !n_tested || !n_applied || !converged) return fail(PBCCS_EINVAL, "bad argument");
    pbccs_repeat_options o = {2, 3, 1, 10, 20};
    if (opts) o = *opts;
    if (o.repeat_length < 1 || o.repeat_length > PBCCS_MAX_MUTATION_BASES)
        return fail(PBCCS_EINVAL, "repeat_length must be 1..7");
    return guarded([&] {
        RefineOptions ro;
        ro.maxIterations = o.max_iterations;
        ro.mutationSeparation = o.mutation_separation;
        ro.mutationNeighborhood = o.mutation_neighborhood;
        bool conv = false;
        const int rc = s->batch->RefineRepeats(s->z, o.repeat_length, o.min_repeat_elements, ro, n_tested, n_applied,
                                               &conv);
        if (rc == 1) return fail(PBCCS_EINVAL, "invalid edit");
        if (rc == 2) return fail(PBCCS_EINVAL, "repeat mutation needs more than 8 extend-buffer columns on some read");
        *converged = conv ? 1 : 0;
        return PBCCS_OK;
    });
}

int pbccs_repeat_mutations(const char* tpl, int tpl_len, int repeat_length, int min_repeat_elements, int begin,
                           int end, pbccs_mutation_ex* out, int cap, int* n)
{
    if (!tpl || tpl_len < 0 || !n || cap < 0 || (cap > 0 && !out) || repeat_length < 1)
        return fail(PBCCS_EINVAL, "bad argument");
    std::vector<MutationEx> muts;
    repeat_mutations(std::string(tpl, (size_t)tpl_len), repeat_length, min_repeat_elements, begin, end, &muts);
    *n = (int)muts.size();
    if ((int)muts.size() > cap) return fail(PBCCS_ERANGE, "buffer too small");
    for (size_t k = 0; k < muts.size(); ++k) {
        out[k].type = muts[k].type;
        out[k].start = muts[k].start;
        out[k].end = muts[k].end;
        out[k].n_bases = (int)muts[k].bases.size();
        out[k].new_bases = muts[k].type == PBCCS_INSERTION ? tpl + muts[k].start : nullptr;
    }
    return PBCCS_OK;
}

int pbccs_apply_mutations(const char* tpl, int tpl_len, const pbccs_mutation_ex* muts, int n, char* out, int cap,
                          int* len, int* mtp)
{
    if (!tpl || tpl_len < 0 || n < 0 || (n > 0 && !muts) || !out || !len) return fail(PBCCS_EINVAL, "bad argument");
    std::vector<MutationEx> ms;
    for (int i = 0; i < n; ++i) {
        MutationEx mu;
        if (!to_mutation_ex(muts[i], false, true, &mu)) return fail(PBCCS_EINVAL, "invalid mutation");
        ms.push_back(mu);
    }
    std::string next;
    std::vector<int> map;
    if (!apply_mutations_ex(std::string(tpl, (size_t)tpl_len), ms, &next, &map))
        return fail(PBCCS_EINVAL, "mutation outside the template");
    *len = (int)next.size();
    if ((int)next.size() + 1 > cap) return fail(PBCCS_ERANGE, "buffer too small");
    std::memcpy(out, next.c_str(), next.size() + 1);
    if (mtp) std::copy(map.begin(), map.end(), mtp);
    return PBCCS_OK;
}

// ---- Arrow: mutations of any width ---------------------------------------------------
// the scoring calls' common front: parse (ACGT only), the checkpoint refusal, then the 8-column rule -- all on
// the host, before any launch
static int arrow_scorable_ex(pbccs_scorer* s, const pbccs_mutation_ex* m, int n, std::vector<MutationEx>* out)
{
    for (int i = 0; i < n; ++i) {
        MutationEx mu;
        if (!to_mutation_ex(m[i], true, false, &mu)) return fail(PBCCS_EINVAL, "invalid multi-base mutation");
        out->push_back(mu);
    }
    if (s->batch->HasCheckpointedReads(s->z))
        return fail(PBCCS_EINVAL, "a read keeps checkpointed bands: wide mutations are not scored on this scorer");
    std::string why;
    if (!s->batch->WideColumnsFit(s->z, *out, &why)) return fail(PBCCS_EINVAL, why.c_str());
    return PBCCS_OK;
}

int pbccs_scorer_score_many_ex(pbccs_scorer* s, const pbccs_mutation_ex* m, int n, double fast_threshold,
                               double* scores)
{
    if (!s || n < 0 || (n > 0 && (!m || !scores))) return fail(PBCCS_EINVAL, "bad argument");
    return guarded([&] {
        std::vector<std::vector<MutationEx>> muts(1);
        if (arrow_scorable_ex(s, m, n, &muts[0]) != PBCCS_OK) return PBCCS_EINVAL;
        if (n == 0) return PBCCS_OK;
        std::vector<std::vector<double>> sc;
        s->batch->ScoreWide({s->z}, muts, fast_threshold, &sc);
        for (int i = 0; i < n; ++i) scores[i] = sc[0][i];
        return PBCCS_OK;
    });
}

int pbccs_scorer_scores_ex(pbccs_scorer* s, const pbccs_mutation_ex* m, double unscored, double* per_read)
{
    if (!s || !m || !per_read) return fail(PBCCS_EINVAL, "bad argument");
    return guarded([&] {
        std::vector<std::vector<MutationEx>> muts(1);
        if (arrow_scorable_ex(s, m, 1, &muts[0]) != PBCCS_OK) return PBCCS_EINVAL;
        std::vector<std::vector<double>> sc, pr;
        s->batch->ScoreWide({s->z}, muts, -std::numeric_limits<double>::max(), &sc, &pr);
        const int nr = s->batch->NumReads(s->z);
        for (int k = 0; k < nr; ++k) per_read[k] = std::isnan(pr[0][k]) ? unscored : pr[0][k];
        return PBCCS_OK;
    });
}

int pbccs_scorer_is_favorable_ex(pbccs_scorer* s, const pbccs_mutation_ex* m, int fast, int* favorable)
{
    if (!s || !m || !favorable) return fail(PBCCS_EINVAL, "bad argument");
    double v = 0.0;
    const double thr = fast ? s->cfg.fast_score_threshold : -std::numeric_limits<double>::max();
    const int rc = pbccs_scorer_score_many_ex(s, m, 1, thr, &v);
    if (rc != PBCCS_OK) return rc;
    *favorable = v > kMinFavorableScoreDiff ? 1 : 0;
    return PBCCS_OK;
}

int pbccs_scorer_apply_mutations_ex(pbccs_scorer* s, const pbccs_mutation_ex* m, int n)
{
    if (!s || n < 0 || (n > 0 && !m)) return fail(PBCCS_EINVAL, "bad argument");
    return guarded([&] {
        std::vector<MutationEx> muts;
        for (int i = 0; i < n; ++i) {
            MutationEx mu;
            if (!to_mutation_ex(m[i], true, false, &mu)) return fail(PBCCS_EINVAL, "invalid multi-base mutation");
            muts.push_back(mu);
        }
        if (!s->batch->ApplyMutationsEx(s->z, muts))
            return fail(PBCCS_EINVAL, "mutation outside the template, or overlapping edits");
        return PBCCS_OK;
    });
}

int pbccs_refine_repeats(pbccs_scorer* s, const pbccs_repeat_options* opts, long long* n_tested, long long* n_applied,
                         int* converged)
{
    if (!s || !n_tested || !n_applied || !converged) return fail(PBCCS_EINVAL, "bad argument");
    pbccs_repeat_options o = {2, 3, 1, 10, 20};
    if (opts) o = *opts;
    if (o.repeat_length < 1 || o.repeat_length > PBCCS_MAX_MUTATION_BASES)
        return fail(PBCCS_EINVAL, "repeat_length must be 1..7");
    return guarded([&] {
        RefineOptions ro;
        ro.maxIterations = o.max_iterations;
        ro.mutationSeparation = o.mutation_separation;
        ro.mutationNeighborhood = o.mutation_neighborhood;
        std::vector<long long> nt, na;
        std::vector<char> conv;
        std::vector<int> st;
        s->batch->RefineRepeats({s->z}, o.repeat_length, o.min_repeat_elements, ro, &nt, &na, &conv, &st);
        *n_tested = nt[0];
        *n_applied = na[0];
        if (st[0] == 1) return fail(PBCCS_EINVAL, "invalid edit");
        if (st[0] == 2) return fail(PBCCS_EINVAL, "repeat mutation needs more than 8 extension columns on some read");
        if (st[0] == 3)
            return fail(PBCCS_EINVAL, "a read keeps checkpointed bands: wide mutations are not scored on this scorer");
        *converged = conv[0] ? 1 : 0;
        return PBCCS_OK;
    });
}

int pbccs_wide_columns_needed(const pbccs_mutation_ex* m, int strand, int tstart, int tend, int* columns)
{
    if (!m || !columns || (strand != 0 && strand != 1) || tstart < 0 || tend < tstart)
        return fail(PBCCS_EINVAL, "bad argument");
    MutationEx mu;
    if (!to_mutation_ex(*m, true, false, &mu)) return fail(PBCCS_EINVAL, "invalid multi-base mutation");
    const OrientedEx o = orient_mutation_ex(mu, strand, tstart, tend);
    const int c = o.scores ? wide_columns_needed(o, tend - tstart) : 0;
    *columns = !o.scores ? -1 : (c < 0 ? -2 : c);
    return PBCCS_OK;
}

int pbccs_quiver_scorer_template(pbccs_quiver_scorer* s, int strand, char* out, int cap, int* len)
{
    if (!s || !out || !len) return fail(PBCCS_EINVAL, "bad argument");
    const std::string t = strand ? reverse_complement(s->batch->Template(s->z)) : s->batch->Template(s->z);
    *len = (int)t.size();
    if ((int)t.size() + 1 > cap) return fail(PBCCS_ERANGE, "buffer too small");
    std::memcpy(out, t.c_str(), t.size() + 1);
    return PBCCS_OK;
}

int pbccs_quiver_scorer_num_reads(pbccs_quiver_scorer* s) { return s ? s->batch->NumReads(s->z) : -1; }

int pbccs_quiver_scorer_read_info(pbccs_quiver_scorer* s, int i, int* active, int* strand, int* tstart, int* tend)
{
    if (!s || i < 0 || i >= s->batch->NumReads(s->z)) return fail(PBCCS_EINVAL, "bad argument");
    const int r = s->batch->ReadIndex(s->z, i);
    if (active) *active = s->batch->Active(r) ? 1 : 0;
    if (strand) *strand = s->batch->Strand(r);
    if (tstart) *tstart = s->batch->Ts(r);
    if (tend) *tend = s->batch->Te(r);
    return PBCCS_OK;
}

int pbccs_quiver_scorer_baseline_score(pbccs_quiver_scorer* s, float* score)
{
    if (!s || !score) return fail(PBCCS_EINVAL, "bad argument");
    *score = s->batch->BaselineScore(s->z);
    return PBCCS_OK;
}

int pbccs_quiver_scorer_baseline_scores(pbccs_quiver_scorer* s, float* out, int cap, int* n)
{
    if (!s || !n) return fail(PBCCS_EINVAL, "bad argument");
    std::vector<float> v;
    for (int k = 0; k < s->batch->NumReads(s->z); ++k) {
        const int r = s->batch->ReadIndex(s->z, k);
        if (s->batch->Active(r)) v.push_back(s->batch->ReadScore(r));
    }
    *n = (int)v.size();
    if ((int)v.size() > cap || (!out && !v.empty())) return fail(PBCCS_ERANGE, "buffer too small");
    std::copy(v.begin(), v.end(), out);
    return PBCCS_OK;
}

int pbccs_quiver_scorer_num_flipflops(pbccs_quiver_scorer* s, int* out)
{
    if (!s || !out) return fail(PBCCS_EINVAL, "bad argument");
    for (int k = 0; k < s->batch->NumReads(s->z); ++k) out[k] = s->batch->Flips(s->batch->ReadIndex(s->z, k));
    return PBCCS_OK;
}

int pbccs_quiver_scorer_allocated_entries(pbccs_quiver_scorer* s, int i, long long* alpha, long long* beta)
{
    if (!s || i < 0 || i >= s->batch->NumReads(s->z) || !alpha || !beta) return fail(PBCCS_EINVAL, "bad argument");
    const int r = s->batch->ReadIndex(s->z, i);
    *alpha = s->batch->Allocated(r, 0);
    *beta = s->batch->Allocated(r, 1);
    return PBCCS_OK;
}

int pbccs_quiver_scorer_alignment(pbccs_quiver_scorer* s, int i, char* target, char* query, int cap, int* len)
{
    if (!s || i < 0 || i >= s->batch->NumReads(s->z) || !len) return fail(PBCCS_EINVAL, "bad argument");
    return guarded([&] {
        std::string t, q;
        if (!s->batch->Alignment(s->batch->ReadIndex(s->z, i), &t, &q))
            return fail(PBCCS_ESTATE, "Alignment needs a Viterbi scorer and a read with a scorer");
        *len = (int)t.size();
        if ((int)t.size() > cap || !target || !query) return fail(PBCCS_ERANGE, "buffer too small");
        memcpy(target, t.data(), t.size());
        memcpy(query, q.data(), q.size());
        return PBCCS_OK;
    });
}

int pbccs_quiver_refine_consensus(pbccs_quiver_scorer* s, const pbccs_refine_options* opts, long long* n_tested,
                                  long long* n_applied, int* converged)
{
    if (!s || !n_tested || !n_applied || !converged) return fail(PBCCS_EINVAL, "bad argument");
    return guarded([&] {
        RefineOptions ro;
        if (opts) {
            ro.maxIterations = opts->max_iterations;
            ro.mutationSeparation = opts->mutation_separation;
            ro.mutationNeighborhood = opts->mutation_neighborhood;
        }
        bool conv = false;
        if (!s->batch->Refine(s->z, ro, n_tested, n_applied, &conv)) return fail(PBCCS_EINVAL, "invalid edit");
        *converged = conv ? 1 : 0;
        return PBCCS_OK;
    });
}

int pbccs_quiver_consensus_qvs(pbccs_quiver_scorer* s, int* qvs, int cap, int* n)
{
    if (!s || !n) return fail(PBCCS_EINVAL, "bad argument");
    return guarded([&] {
        const std::vector<int> q = s->batch->QVs(s->z);
        *n = (int)q.size();
        if ((int)q.size() > cap || !qvs) return fail(PBCCS_ERANGE, "buffer too small");
        std::copy(q.begin(), q.end(), qvs);
        return PBCCS_OK;
    });
}

int pbccs_quiver_consensus_qvs_rich(pbccs_quiver_scorer* s, int* qvs, pbccs_rich_qvs* rich, int* n)
{
    if (!s || !n || !rich) return fail(PBCCS_EINVAL, "bad argument");
    return guarded([&] {
        std::vector<RichQVs> r;
        const std::vector<std::vector<int>> q = s->batch->QVsMany({s->z}, &r);
        *n = (int)q[0].size();
        if (!qvs || !write_rich(rich, r[0])) {
            rich->len = -*n;
            return fail(PBCCS_ERANGE, "buffer too small");
        }
        std::copy(q[0].begin(), q[0].end(), qvs);
        return PBCCS_OK;
    });
}

int pbccs_qv_evaluator_moves(pbccs_engine* eng, const pbccs_qv_features* read, const char* tpl, int tpl_len,
                             const pbccs_qv_model_params* params, int pin_start, int pin_end, const int* i,
                             const int* j, int n, float* inc, float* del, float* extra, float* merge)
{
    if (!eng || !read || !read->seq || read->len < 0 || !tpl || tpl_len < 0 || !params || n < 0 ||
        (n > 0 && (!i || !j)))
        return fail(PBCCS_EINVAL, "bad argument");
    if (n == 0) return PBCCS_OK;
    return guarded([&] {
        if (hipSetDevice(eng->device) != hipSuccess) return fail(PBCCS_EDEVICE, "hipSetDevice failed");
        const int I = read->len;
        // one device block: QParams | 5 feature tracks | cells i, j | outputs | read bases | template
        pbccs_quiver_config c{};
        c.params = *params;
        c.moves_available = 15;
        const quiver::QParams qp = qparams(c);
        std::vector<float> feat((size_t)5 * std::max(I, 1), 0.0f);
        const float* tr[5] = {read->ins_qv, read->subs_qv, read->del_qv, read->del_tag, read->merge_qv};
        for (int k = 0; k < 5; ++k)
            if (tr[k]) std::copy(tr[k], tr[k] + I, feat.begin() + (size_t)k * std::max(I, 1));
        auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
        const size_t oP = 0, oF = up(sizeof(qp)), oI = oF + up(feat.size() * 4), oJ = oI + up((size_t)n * 4),
                     oO = oJ + up((size_t)n * 4), oS = oO + up((size_t)16 * n), oT = oS + up((size_t)I + 1),
                     top = oT + up((size_t)tpl_len + 1);
        std::vector<char> h(top, 0);
        std::memcpy(h.data() + oP, &qp, sizeof(qp));
        std::memcpy(h.data() + oF, feat.data(), feat.size() * 4);
        std::memcpy(h.data() + oI, i, (size_t)n * 4);
        std::memcpy(h.data() + oJ, j, (size_t)n * 4);
        std::memcpy(h.data() + oS, read->seq, I);
        std::memcpy(h.data() + oT, tpl, tpl_len);
        DevVec<char> d;
        d.reserve(top, false);
        hipStream_t st = nullptr;
        if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) return fail(PBCCS_EDEVICE, "stream");
        struct StreamGuard {
            hipStream_t s;
            ~StreamGuard() { (void)hipStreamSynchronize(s); (void)hipStreamDestroy(s); }
        } guard{st};
        if (hipMemcpyAsync(d.ptr, h.data(), top, hipMemcpyHostToDevice, st) != hipSuccess)
            return fail(PBCCS_EDEVICE, "upload failed");
        const float* df = reinterpret_cast<const float*>(d.ptr + oF);
        const size_t F = std::max(I, 1);
        quiver::QRead r{d.ptr + oS, df, df + F, df + 2 * F, df + 3 * F, df + 4 * F, I};
        quiver::launch_qv_moves(r, reinterpret_cast<const quiver::QParams*>(d.ptr + oP), d.ptr + oT, tpl_len,
                                pin_start ? 1 : 0, pin_end ? 1 : 0, reinterpret_cast<const int*>(d.ptr + oI),
                                reinterpret_cast<const int*>(d.ptr + oJ), n, reinterpret_cast<float*>(d.ptr + oO), st);
        if (hipGetLastError() != hipSuccess) return fail(PBCCS_EDEVICE, "k_qv_moves launch failed");
        std::vector<float> out((size_t)4 * n);
        if (hipMemcpyAsync(out.data(), d.ptr + oO, out.size() * 4, hipMemcpyDeviceToHost, st) != hipSuccess ||
            hipStreamSynchronize(st) != hipSuccess)
            return fail(PBCCS_EDEVICE, "download failed");
        float* dst[4] = {inc, del, extra, merge};
        for (int k = 0; k < 4; ++k)
            if (dst[k]) std::copy(out.begin() + (size_t)k * n, out.begin() + (size_t)(k + 1) * n, dst[k]);
        return PBCCS_OK;
    });
}

// pbccs_quiver_polish_batch and its _ex form: rep == nullptr is the plain call
static int quiver_polish_batch_impl(pbccs_engine* eng, const pbccs_quiver_config* configs,
                                    const char* const* chemistries, int n_configs, const pbccs_quiver_zmw* zmws, int n,
                                    const pbccs_refine_options* opts, const pbccs_repeat_options* rep,
                                    long long* repeat_tested, long long* repeat_applied, pbccs_quiver_result* out,
                                    pbccs_rich_qvs* rich = nullptr)
{
    if (!eng || !configs || n_configs < 1 || n < 0 || (n > 0 && (!zmws || !out))) return fail(PBCCS_EINVAL, "bad argument");
    for (int k = 0; k < n_configs; ++k)
        if (configs[k].recursor < PBCCS_QV_RECURSOR_SPARSE_SSE || configs[k].recursor > PBCCS_QV_RECURSOR_DENSE_SIMPLE)
            return fail(PBCCS_EINVAL, "unknown recursor type");
    for (int z = 0; z < n; ++z) {
        if (!zmws[z].tpl || zmws[z].tpl_len <= 0 || zmws[z].n_reads < 0 || (zmws[z].n_reads > 0 && !zmws[z].reads))
            return fail(PBCCS_EINVAL, "bad pbccs_quiver_zmw");
        for (int r = 0; r < zmws[z].n_reads; ++r) {
            const pbccs_quiver_read& q = zmws[z].reads[r];
            if (!q.seq || q.len <= 0 || (q.strand != 0 && q.strand != 1)) return fail(PBCCS_EINVAL, "bad pbccs_quiver_read");
        }
    }
    if (n == 0) return PBCCS_OK;
    return guarded([&] {
        std::lock_guard<std::mutex> lock(eng->quiverMu);
        if (!eng->quiverBatch) {
            eng->quiverBatch.reset(new quiver::QuiverBatch(eng->device));
            eng->quiverBatch->PinHostPools();
        }
        quiver::QuiverBatch& qb = *eng->quiverBatch;
        qb.Reset();
        qb.SetProfiling(eng->profiling);
        // the QuiverConfigTable, as pbccs_quiver_scorer_create builds it
        std::vector<std::pair<std::string, int>> table;
        std::vector<const pbccs_quiver_config*> cfgs;
        float fast = 0.0f;
        for (int k = 0; k < n_configs; ++k) {
            const std::string name = (chemistries && chemistries[k]) ? chemistries[k] : "*";
            bool dup = false;
            for (auto& kv : table) dup = dup || kv.first == name;
            if (dup) continue;
            table.emplace_back(name, qb.AddConfig(qparams(configs[k])));
            cfgs.push_back(&configs[k]);
            fast = std::min(fast, configs[k].fast_score_threshold);
        }
        std::vector<int> zs(n);
        std::vector<quiver::QuiverBatch::ReadSpec> specs;
        std::vector<int> specZmw;
        for (int z = 0; z < n; ++z) {
            zs[z] = qb.AddZmw(std::string(zmws[z].tpl, zmws[z].tpl_len), fast);
            for (int r = 0; r < zmws[z].n_reads; ++r) {
                const pbccs_quiver_read& q = zmws[z].reads[r];
                const std::string chem = q.chemistry ? q.chemistry : "*";
                int cfg = -1;
                size_t pos = 0;
                for (size_t k = 0; k < table.size(); ++k)
                    if (table[k].first == chem) { cfg = table[k].second; pos = k; }
                if (cfg < 0)
                    for (size_t k = 0; k < table.size(); ++k)
                        if (table[k].first == "*") { cfg = table[k].second; pos = k; }
                if (cfg < 0) return fail(PBCCS_EINVAL, "Chemistry not found in QuiverConfigTable");
                quiver::QuiverBatch::ReadSpec sp;
                sp.z = zs[z];
                sp.strand = q.strand;
                sp.ts = q.tstart;
                sp.te = q.tend < 0 ? zmws[z].tpl_len : q.tend;
                sp.config = cfg;
                sp.threshold = std::isnan(q.threshold) ? cfgs[pos]->add_threshold : q.threshold;
                sp.seq = q.seq;
                sp.len = q.len;
                sp.track[0] = q.ins_qv;
                sp.track[1] = q.subs_qv;
                sp.track[2] = q.del_qv;
                sp.track[3] = q.del_tag;
                sp.track[4] = q.merge_qv;
                specs.push_back(sp);
                specZmw.push_back(z);
            }
        }
        // PBCCS_QUIVER_TRACE=1: one stderr line with the wall time of each phase (prepare, AddRead, refine, QVs)
        static const bool qtrace = std::getenv("PBCCS_QUIVER_TRACE") != nullptr;
        auto qt0 = std::chrono::steady_clock::now();
        auto lap = [&]() {
            const auto t = std::chrono::steady_clock::now();
            const double ms = std::chrono::duration<double, std::milli>(t - qt0).count();
            qt0 = t;
            return ms;
        };
        const double msPrep = lap();
        const std::vector<char> act = qb.AddReads(&specs);
        const double msAdd = lap();
        for (int z = 0; z < n; ++z) out[z].n_active = 0;
        for (size_t k = 0; k < act.size(); ++k) out[specZmw[k]].n_active += act[k];
        RefineOptions ro;
        if (opts) {
            ro.maxIterations = opts->max_iterations;
            ro.mutationSeparation = opts->mutation_separation;
            ro.mutationNeighborhood = opts->mutation_neighborhood;
        }
        std::vector<long long> nt, na;
        std::vector<char> conv, ok;
        qb.RefineMany(zs, ro, &nt, &na, &conv, &ok);
        if (rep) {   // RefineRepeats on the scorers RefineConsensus left usable, in lock-step rounds
            std::vector<int> rk, rz;
            for (int z = 0; z < n; ++z) {
                if (repeat_tested) repeat_tested[z] = 0;
                if (repeat_applied) repeat_applied[z] = 0;
                if (ok[z]) { rk.push_back(z); rz.push_back(zs[z]); }
            }
            RefineOptions rr;
            rr.maxIterations = rep->max_iterations;
            rr.mutationSeparation = rep->mutation_separation;
            rr.mutationNeighborhood = rep->mutation_neighborhood;
            std::vector<long long> rt, ra;
            std::vector<char> rconv;
            std::vector<int> rst;
            qb.RefineRepeatsMany(rz, rep->repeat_length, rep->min_repeat_elements, rr, &rt, &ra, &rconv, &rst);
            for (size_t k = 0; k < rk.size(); ++k) {
                if (repeat_tested) repeat_tested[rk[k]] = rt[k];
                if (repeat_applied) repeat_applied[rk[k]] = ra[k];
                if (rst[k] != 0) ok[rk[k]] = 0;
            }
        }
        const double msRefine = lap();
        std::vector<int> wantQv;
        for (int z = 0; z < n; ++z)
            if ((out[z].qvs || rich) && ok[z]) wantQv.push_back(z);
        std::vector<int> qz;
        for (int z : wantQv) qz.push_back(zs[z]);
        std::vector<RichQVs> richQ;
        const std::vector<std::vector<int>> qv =
            qz.empty() ? std::vector<std::vector<int>>() : qb.QVsMany(qz, rich ? &richQ : nullptr);
        for (int z = 0; rich && z < n; ++z) rich[z].len = 0;
        if (qtrace)
            std::fprintf(stderr, "[quiver] scorers %d prepare %.1f ms addread %.1f ms refine %.1f ms qvs %.1f ms\n", n,
                         msPrep, msAdd, msRefine, lap());
        for (int z = 0; z < n; ++z) {
            pbccs_quiver_result& o = out[z];
            o.n_tested = nt[z];
            o.n_applied = na[z];
            o.converged = conv[z];
            o.ok = ok[z];
            const std::string& t = qb.Template(zs[z]);
            o.consensus_len = (int)t.size();
            if (o.consensus && o.consensus_cap >= (int)t.size()) memcpy(o.consensus, t.data(), t.size());
        }
        for (size_t k = 0; k < wantQv.size(); ++k) {
            pbccs_quiver_result& o = out[wantQv[k]];
            if (o.qvs && o.consensus_cap >= (int)qv[k].size()) std::copy(qv[k].begin(), qv[k].end(), o.qvs);
            if (rich) write_rich(&rich[wantQv[k]], richQ[k]);
        }
        {
            std::lock_guard<std::mutex> lk(eng->statsMu);
            qb.CollectProfile(eng->stats);
        }
        return PBCCS_OK;
    });
}

int pbccs_quiver_polish_batch(pbccs_engine* eng, const pbccs_quiver_config* configs, const char* const* chemistries,
                              int n_configs, const pbccs_quiver_zmw* zmws, int n, const pbccs_refine_options* opts,
                              pbccs_quiver_result* out)
{
    return quiver_polish_batch_impl(eng, configs, chemistries, n_configs, zmws, n, opts, nullptr, nullptr, nullptr, out);
}

int pbccs_quiver_polish_batch_ex(pbccs_engine* eng, const pbccs_quiver_config* configs, const char* const* chemistries,
                                 int n_configs, const pbccs_quiver_zmw* zmws, int n, const pbccs_refine_options* opts,
                                 const pbccs_repeat_options* repeats, long long* repeat_tested,
                                 long long* repeat_applied, pbccs_quiver_result* out)
{
    if (repeats && (repeats->repeat_length < 1 || repeats->repeat_length > PBCCS_MAX_MUTATION_BASES))
        return fail(PBCCS_EINVAL, "repeat_length must be 1..7");
    return quiver_polish_batch_impl(eng, configs, chemistries, n_configs, zmws, n, opts, repeats, repeat_tested,
                                    repeat_applied, out);
}

int pbccs_quiver_polish_batch_ex2(pbccs_engine* eng, const pbccs_quiver_config* configs,
                                  const char* const* chemistries, int n_configs, const pbccs_quiver_zmw* zmws, int n,
                                  const pbccs_refine_options* opts, const pbccs_polish_extras* extras,
                                  pbccs_quiver_result* out)
{
    const pbccs_polish_extras none{};
    const pbccs_polish_extras& x = extras ? *extras : none;
    if (x.repeats && (x.repeats->repeat_length < 1 || x.repeats->repeat_length > PBCCS_MAX_MUTATION_BASES))
        return fail(PBCCS_EINVAL, "repeat_length must be 1..7");
    return quiver_polish_batch_impl(eng, configs, chemistries, n_configs, zmws, n, opts, x.repeats, x.repeat_tested,
                                    x.repeat_applied, out, x.rich);
}

// ---------------------------------------------------------------- Diploid site calling
// IsSiteHeterozygous / DiploidSite (Arrow/Diploid.cpp:94-241, Quiver/Diploid.cpp); DESIGN.md §3.13

int pbccs_is_site_heterozygous(const float* site_scores, int n_reads, int n_alleles, float log_prior_ratio,
                               int* is_het, pbccs_diploid_site* site, int* allele_for_read)
{
    // the reference asserts dim2 == MUTATIONS_PER_SITE (Diploid.cpp:140)
    if (!site_scores || !is_het || !site || !allele_for_read || n_alleles != kSiteAlleles || n_reads <= 0)
        return fail(PBCCS_EINVAL, "bad argument");
    DiploidCall call;
    *is_het = is_site_heterozygous(site_scores, n_reads, log_prior_ratio, &call, allele_for_read) ? 1 : 0;
    site->allele0 = call.allele0;
    site->allele1 = call.allele1;
    site->log_bayes_factor = call.logBayesFactor;
    return PBCCS_OK;
}

// the two families' common back: range and capacity checks before any launch, then the batch's call
static int site_scores_impl(int tplLen, int nReads, int begin, int end, float* out, long long cap, long long* n,
                            const std::function<void(std::vector<float>*)>& run)
{
    if (!n) return fail(PBCCS_EINVAL, "bad argument");
    if (begin < 0 || end > tplLen || begin >= end) return fail(PBCCS_EINVAL, "site range outside the template");
    *n = (long long)(end - begin) * nReads * kSiteAlleles;
    if (cap < *n || (!out && *n > 0)) return fail(PBCCS_ERANGE, "buffer too small");
    if (*n == 0) return PBCCS_OK;
    return guarded([&] {
        std::vector<float> t;
        run(&t);
        std::copy(t.begin(), t.end(), out);
        return PBCCS_OK;
    });
}

static int diploid_sites_impl(pbccs_engine* eng, int tplLen, int nReads, int begin, int end,
                              pbccs_diploid_site* sites, int cap, int* n, int* allele_for_read,
                              const std::function<void(std::vector<DiploidSiteH>*, std::vector<int>*, DiploidStats*)>& run)
{
    if (!n || cap < 0 || (cap > 0 && !sites)) return fail(PBCCS_EINVAL, "bad argument");
    if (begin < 0 || end > tplLen || begin >= end) return fail(PBCCS_EINVAL, "site range outside the template");
    *n = 0;
    if (nReads == 0) return PBCCS_OK;
    return guarded([&] {
        std::vector<DiploidSiteH> found;
        std::vector<int> afr;
        DiploidStats st;
        run(&found, &afr, &st);
        {
            std::lock_guard<std::mutex> lock(eng->statsMu);
            eng->diploid.sitesScreened += st.sitesScreened;
            eng->diploid.sitesSentToHost += st.sitesSentToHost;
            eng->diploid.sitesReported += st.sitesReported;
        }
        *n = (int)found.size();
        if (*n > cap) return fail(PBCCS_ERANGE, "buffer too small");
        for (int k = 0; k < *n; ++k) {
            sites[k].position = found[k].position;
            sites[k].allele0 = found[k].allele0;
            sites[k].allele1 = found[k].allele1;
            sites[k].log_bayes_factor = found[k].logBayesFactor;
        }
        if (allele_for_read) std::copy(afr.begin(), afr.end(), allele_for_read);
        return PBCCS_OK;
    });
}

int pbccs_scorer_site_scores(pbccs_scorer* s, int begin, int end, float* out, long long cap, long long* n)
{
    if (!s) return fail(PBCCS_EINVAL, "bad argument");
    return site_scores_impl((int)s->batch->Template(s->z).size(), s->batch->NumReads(s->z), begin, end, out, cap, n,
                            [&](std::vector<float>* t) { s->batch->SiteScores(s->z, begin, end, t); });
}

int pbccs_quiver_scorer_site_scores(pbccs_quiver_scorer* s, int begin, int end, float* out, long long cap,
                                    long long* n)
{
    if (!s) return fail(PBCCS_EINVAL, "bad argument");
    return site_scores_impl((int)s->batch->Template(s->z).size(), s->batch->NumReads(s->z), begin, end, out, cap, n,
                            [&](std::vector<float>* t) { s->batch->SiteScores(s->z, begin, end, t); });
}

int pbccs_scorer_diploid_sites(pbccs_scorer* s, int begin, int end, float log_prior_ratio, int host_all,
                               pbccs_diploid_site* sites, int cap, int* n, int* allele_for_read)
{
    if (!s) return fail(PBCCS_EINVAL, "bad argument");
    return diploid_sites_impl(s->eng, (int)s->batch->Template(s->z).size(), s->batch->NumReads(s->z), begin, end, sites,
                              cap, n, allele_for_read,
                              [&](std::vector<DiploidSiteH>* f, std::vector<int>* a, DiploidStats* st) {
                                  s->batch->DiploidSites(s->z, begin, end, log_prior_ratio, host_all != 0, f, a, st);
                              });
}

int pbccs_quiver_scorer_diploid_sites(pbccs_quiver_scorer* s, int begin, int end, float log_prior_ratio,
                                      int host_all, pbccs_diploid_site* sites, int cap, int* n, int* allele_for_read)
{
    if (!s) return fail(PBCCS_EINVAL, "bad argument");
    return diploid_sites_impl(s->eng, (int)s->batch->Template(s->z).size(), s->batch->NumReads(s->z), begin, end, sites,
                              cap, n, allele_for_read,
                              [&](std::vector<DiploidSiteH>* f, std::vector<int>* a, DiploidStats* st) {
                                  s->batch->DiploidSites(s->z, begin, end, log_prior_ratio, host_all != 0, f, a, st);
                              });
}

int pbccs_diploid_stats_get(pbccs_engine* eng, pbccs_diploid_stats* out, int reset)
{
    if (!eng || !out) return fail(PBCCS_EINVAL, "null argument");
    std::lock_guard<std::mutex> lock(eng->statsMu);
    out->sites_screened = eng->diploid.sitesScreened;
    out->sites_sent_to_host = eng->diploid.sitesSentToHost;
    out->sites_reported = eng->diploid.sitesReported;
    if (reset) eng->diploid = DiploidStats();
    return PBCCS_OK;
}

// ---------------------------------------------------------------- POA draft

struct pbccs_sparse_poa {
    pbccs_engine* eng;
    poa::ZmwPoa z;
    bool banded = false;   // pbccs_sparse_poa_set_banded
};

namespace {

int put_text(const std::string& s, char* out, int cap, int* len)
{
    if (len) *len = (int)s.size();
    if ((int)s.size() > cap || (!out && !s.empty())) return fail(PBCCS_ERANGE, "buffer too small");
    if (!s.empty()) memcpy(out, s.data(), s.size());
    return PBCCS_OK;
}

}  // namespace

static int poa_batch_impl(pbccs_engine* eng, const pbccs_poa_input* in, int n, long long max_coverage,
                          int min_coverage, bool banded, pbccs_poa_output* out)
{
    if (!eng || n < 0 || (n > 0 && (!in || !out)) || max_coverage < 1) return fail(PBCCS_EINVAL, "bad argument");
    return guarded([&] {
        std::vector<std::vector<std::string>> own(n);
        std::vector<std::vector<const std::string*>> reads(n);
        for (int z = 0; z < n; ++z) {
            if (in[z].n_reads < 0 || (in[z].n_reads > 0 && (!in[z].seqs || !in[z].lens)))
                return fail(PBCCS_EINVAL, "bad pbccs_poa_input");
            own[z].resize(in[z].n_reads);
            for (int r = 0; r < in[z].n_reads; ++r) {
                if (in[z].seqs[r] && in[z].lens[r] < 0) return fail(PBCCS_EINVAL, "negative read length");
                if (in[z].seqs[r]) own[z][r].assign(in[z].seqs[r], in[z].lens[r]);   // empty: key -1
            }
            for (int r = 0; r < in[z].n_reads; ++r) reads[z].push_back(in[z].seqs[r] ? &own[z][r] : nullptr);
        }
        std::vector<std::string> css;
        std::vector<std::vector<int>> keys, ext;
        std::vector<std::vector<char>> rc;
        {
            std::lock_guard<std::mutex> lk(eng->poaMu);
            poa::PoaBatch(eng->PoaRunners(), reads, max_coverage, min_coverage, &css, &keys, &rc, &ext, nullptr,
                          banded);
        }
        bool range = false;
        for (int z = 0; z < n; ++z) {
            pbccs_poa_output& o = out[z];
            o.len = (int)css[z].size();
            o.n_keys = (int)rc[z].size();
            if (o.consensus && o.len <= o.cap) memcpy(o.consensus, css[z].data(), css[z].size());
            else range = true;
            for (int r = 0; r < in[z].n_reads; ++r)
                if (o.keys) o.keys[r] = keys[z][r];
            for (int k = 0; k < o.n_keys; ++k) {
                if (o.rc) o.rc[k] = rc[z][k];
                if (o.extents)
                    for (int e = 0; e < 4; ++e) o.extents[4 * k + e] = ext[z][4 * k + e];
            }
        }
        return range ? fail(PBCCS_ERANGE, "consensus buffer too small") : PBCCS_OK;
    });
}

int pbccs_poa_batch(pbccs_engine* eng, const pbccs_poa_input* in, int n, long long max_coverage, int min_coverage,
                    pbccs_poa_output* out)
{
    return poa_batch_impl(eng, in, n, max_coverage, min_coverage, false, out);
}

void pbccs_poa_options_default(pbccs_poa_options* o)
{
    if (!o) return;
    o->max_coverage = std::numeric_limits<long long>::max();
    o->min_coverage = -1;
    o->banded = 0;
}

int pbccs_poa_batch_ex(pbccs_engine* eng, const pbccs_poa_input* in, int n, const pbccs_poa_options* opts,
                       pbccs_poa_output* out)
{
    pbccs_poa_options o;
    if (opts) o = *opts;
    else pbccs_poa_options_default(&o);
    return poa_batch_impl(eng, in, n, o.max_coverage, o.min_coverage, o.banded != 0, out);
}

int pbccs_sparse_poa_create(pbccs_engine* eng, pbccs_sparse_poa** out)
{
    if (!eng || !out) return fail(PBCCS_EINVAL, "bad argument");
    return guarded([&] {
        *out = new pbccs_sparse_poa{eng, poa::ZmwPoa()};
        return PBCCS_OK;
    });
}

int pbccs_sparse_poa_set_banded(pbccs_sparse_poa* p, int on)
{
    if (!p) return fail(PBCCS_EINVAL, "bad argument");
    p->banded = on != 0;
    return PBCCS_OK;
}

int pbccs_sparse_poa_alignable_ranges(pbccs_sparse_poa* p, const char* seq, int len, int rc, int* css_path,
                                      int css_cap, int* css_len, int* anchors, int anchor_cap, int* n_anchors,
                                      int* ranges, int range_cap, int* n_vertices, int* fallback)
{
    if (!p || (!seq && len > 0) || len < 0 || !css_len || !n_anchors || !n_vertices || !fallback)
        return fail(PBCCS_EINVAL, "bad argument");
    return guarded([&] {
        if (p->z.graph.NumReads() == 0) return fail(PBCCS_ESTATE, "the graph holds no read");
        poa::RangeReport rep;
        {
            std::lock_guard<std::mutex> lk(p->eng->poaMu);
            p->eng->Poa().Ranges(&p->z.graph, std::string(seq ? seq : "", len), rc != 0, &rep);
        }
        *css_len = (int)rep.cssPath.size();
        *n_anchors = (int)rep.anchors.size() / 2;
        *n_vertices = (int)rep.ranges.size() / 2;
        *fallback = rep.ranges.empty() ? 1 : 0;
        if (*css_len > css_cap || *n_anchors > anchor_cap || *n_vertices > range_cap ||
            (!css_path && *css_len) || (!anchors && *n_anchors) || (!ranges && *n_vertices))
            return fail(PBCCS_ERANGE, "buffer too small");
        if (*css_len) memcpy(css_path, rep.cssPath.data(), rep.cssPath.size() * sizeof(int));
        if (*n_anchors) memcpy(anchors, rep.anchors.data(), rep.anchors.size() * sizeof(int));
        if (*n_vertices) memcpy(ranges, rep.ranges.data(), rep.ranges.size() * sizeof(int));
        return PBCCS_OK;
    });
}

int pbccs_sparse_poa_try_add_read(pbccs_sparse_poa* p, const char* seq, int len, int rc, int banded, float* score,
                                  int* steps, int cap, int* n_steps)
{
    if (!p || !seq || len <= 0 || !score || !n_steps || cap < 0) return fail(PBCCS_EINVAL, "bad argument");
    return guarded([&] {
        if (p->z.graph.NumReads() == 0) return fail(PBCCS_ESTATE, "the graph holds no read");
        poa::AlignRequest rq{&p->z.graph, std::string(seq, len), poa::kLocal, true, 0.f, banded != 0, rc ? 1 : 0};
        std::vector<poa::AlignRequest> req{rq};
        std::vector<poa::AlignResult> res;
        {
            std::lock_guard<std::mutex> lk(p->eng->poaMu);
            p->eng->Poa().Align(req, &res);
        }
        const poa::AlignResult& R = res[0];
        *score = R.score[rc ? 1 : 0];
        *n_steps = (int)R.steps.size();
        if (*n_steps > cap || (!steps && *n_steps)) return fail(PBCCS_ERANGE, "buffer too small");
        int row = len;   // the cell each step stands on: $'s row, the End move's source row, then as the moves go
        for (int k = 0; k < *n_steps; ++k) {
            const int mv = (int)(R.steps[k] >> 28);
            steps[3 * k] = (int)(R.steps[k] & poa::kStepVertexMask);
            steps[3 * k + 1] = mv;
            steps[3 * k + 2] = row;
            if (mv == poa::kEnd) row = R.head.endRow;
            else if (mv == poa::kStart) row = 0;
            else if (mv != poa::kDelete) row--;
        }
        return PBCCS_OK;
    });
}

void pbccs_sparse_poa_destroy(pbccs_sparse_poa* p) { delete p; }

int pbccs_sparse_poa_orient_and_add_read(pbccs_sparse_poa* p, const char* seq, int len, float min_score_to_add,
                                         int* key)
{
    if (!p || (!seq && len > 0) || len < 0 || !key) return fail(PBCCS_EINVAL, "bad argument");
    return guarded([&] {
        if (len == 0) {   // an empty read is never added (the rule of pbccs_poa_batch / pbccs_ccs_batch)
            *key = -1;
            return PBCCS_OK;
        }
        const std::string s(seq, len);
        if (p->z.graph.NumReads() == 0) {
            std::vector<int> path;
            p->z.graph.AddFirstRead(s, &path);
            p->z.readPaths.push_back(std::move(path));
            p->z.rc.push_back(0);
            *key = 0;
            return PBCCS_OK;
        }
        std::vector<poa::AlignRequest> req{
            poa::AlignRequest{&p->z.graph, s, poa::kLocal, true, min_score_to_add, p->banded}};
        std::vector<poa::AlignResult> res;
        {
            std::lock_guard<std::mutex> lk(p->eng->poaMu);
            p->eng->Poa().Align(req, &res);
        }
        if (res[0].chosen < 0) {
            *key = -1;
            return PBCCS_OK;
        }
        p->z.readPaths.push_back(std::move(res[0].path));
        p->z.rc.push_back((char)res[0].chosen);
        *key = (int)p->z.readPaths.size() - 1;
        return PBCCS_OK;
    });
}

int pbccs_sparse_poa_find_consensus(pbccs_sparse_poa* p, int min_coverage, char* out, int cap, int* len, int* rc,
                                    int* extents, int* n_keys)
{
    if (!p || !len) return fail(PBCCS_EINVAL, "bad argument");
    return guarded([&] {
        std::vector<int> ext;
        const std::string css = p->z.readPaths.empty() ? std::string() : p->z.FindConsensus(min_coverage, &ext);
        const int nk = (int)p->z.rc.size();
        if (n_keys) *n_keys = nk;
        for (int k = 0; k < nk; ++k) {
            if (rc) rc[k] = p->z.rc[k];
            if (extents)
                for (int e = 0; e < 4; ++e) extents[4 * k + e] = ext[4 * k + e];
        }
        return put_text(css, out, cap, len);
    });
}

int pbccs_sparse_poa_graphviz(pbccs_sparse_poa* p, int flags, int min_coverage, char* out, int cap, int* len)
{
    if (!p || !len) return fail(PBCCS_EINVAL, "bad argument");
    return guarded([&] {
        std::vector<int> path;
        if (!p->z.readPaths.empty()) p->z.FindConsensus(min_coverage, nullptr, &path);
        return put_text(p->z.graph.GraphViz(flags & 1, flags & 2, &path), out, cap, len);
    });
}

int pbccs_poa_consensus(pbccs_engine* eng, const char* const* reads, const int* lens, int n, int mode,
                        int min_coverage, char* out, int cap, int* len, int flags, char* dot, int dot_cap,
                        int* dot_len)
{
    if (!eng || n < 0 || (n > 0 && (!reads || !lens)) || !len || mode < 0 || mode > 2)
        return fail(PBCCS_EINVAL, "bad argument");
    return guarded([&] {
        poa::PoaGraph g;
        for (int r = 0; r < n; ++r) {
            if (!reads[r] || lens[r] <= 0) return fail(PBCCS_EINVAL, "Input sequences must have nonzero length.");
            const std::string s(reads[r], lens[r]);
            if (g.NumReads() == 0) {
                g.AddFirstRead(s, nullptr);
                continue;
            }
            std::vector<poa::AlignRequest> req{poa::AlignRequest{&g, s, (poa::AlignMode)mode, false, 0.f}};
            std::vector<poa::AlignResult> res;
            std::lock_guard<std::mutex> lk(eng->poaMu);
            eng->Poa().Align(req, &res);
        }
        const std::vector<int> path = g.ConsensusPath((poa::AlignMode)mode, min_coverage);
        if (dot) {
            const int rc = put_text(g.GraphViz(flags & 1, flags & 2, &path), dot, dot_cap, dot_len);
            if (rc != PBCCS_OK) return rc;
        }
        return put_text(g.Sequence(path), out, cap, len);
    });
}

int pbccs_poa_band_stats_get(pbccs_engine* eng, pbccs_poa_band_stats* out, int reset)
{
    if (!eng || !out) return fail(PBCCS_EINVAL, "bad argument");
    return guarded([&] {
        std::lock_guard<std::mutex> lk(eng->poaMu);
        poa::BandStats s;
        for (poa::PoaRunner* r : eng->PoaRunners()) {   // everything adds up over the slices
            const poa::BandStats& x = r->band;
            s.bandedAlignments += x.bandedAlignments;
            s.fallbacks += x.fallbacks;
            s.bandCells += x.bandCells;
            s.fullCells += x.fullCells;
            s.seeds += x.seeds;
            s.anchors += x.anchors;
            s.seedMs += x.seedMs;
            s.rangesMs += x.rangesMs;
            s.fillMs += x.fillMs;
            s.traceMs += x.traceMs;
            s.scoreBytes += x.scoreBytes;
            if (reset) r->band = poa::BandStats();
        }
        *out = pbccs_poa_band_stats{s.bandedAlignments, s.fallbacks, s.bandCells, s.fullCells, s.seeds,     s.anchors,
                                    s.seedMs,           s.rangesMs,  s.fillMs,    s.traceMs,   s.scoreBytes};
        return PBCCS_OK;
    });
}

int pbccs_poa_stats_get(pbccs_engine* eng, pbccs_poa_stats* out, int reset)
{
    if (!eng || !out) return fail(PBCCS_EINVAL, "bad argument");
    return guarded([&] {
        std::lock_guard<std::mutex> lk(eng->poaMu);
        poa::PoaStats s;
        for (poa::PoaRunner* r : eng->PoaRunners()) {   // counts add up; wall times are the slices' maxima
            const poa::PoaStats& x = r->stats;
            s.alignments += x.alignments;
            s.cells += x.cells;
            s.launches += x.launches;
            s.traceSteps += x.traceSteps;
            s.fillMs += x.fillMs;
            s.traceMs += x.traceMs;
            s.bytes += x.bytes;
            s.progMs = std::max(s.progMs, x.progMs);
            s.deviceMs = std::max(s.deviceMs, x.deviceMs);
            s.threadMs = std::max(s.threadMs, x.threadMs);
            s.consensusMs = std::max(s.consensusMs, x.consensusMs);
            s.totalMs = std::max(s.totalMs, x.totalMs);
            if (reset) r->stats = poa::PoaStats();
        }
        *out = pbccs_poa_stats{s.alignments, s.cells,  s.launches, s.traceSteps, s.fillMs,     s.traceMs,
                               s.bytes,      s.progMs, s.deviceMs, s.threadMs,  s.consensusMs, s.totalMs};
        return PBCCS_OK;
    });
}

// ---- pairwise alignment (align_kernels.hpp) --------------------------------------------------------------
int pbccs_align_batch(pbccs_engine* eng, const pbccs_align_params* params, const pbccs_align_pair* pairs, int n,
                      pbccs_align_result* out)
{
    return pbccs_align_batch_ex(eng, params, pairs, n, out, nullptr, nullptr);
}

int pbccs_align_batch_ex(pbccs_engine* eng, const pbccs_align_params* params, const pbccs_align_pair* pairs, int n,
                         pbccs_align_result* out, const pbccs_align_band* band, pbccs_align_band_info* info)
{
    if (!eng || !params || n < 0 || (n > 0 && (!pairs || !out))) return fail(PBCCS_EINVAL, "bad argument");
    const pbccs_align_params& a = *params;
    if (a.kind != PBCCS_ALIGN_NW && a.kind != PBCCS_ALIGN_AFFINE && a.kind != PBCCS_ALIGN_AFFINE_IUPAC)
        return fail(PBCCS_EINVAL, "unknown alignment kind");
    if (a.kind == PBCCS_ALIGN_NW && a.mode != PBCCS_POA_GLOBAL)
        return fail(PBCCS_EINVAL, "Only GLOBAL alignment supported at present");
    if (a.kind != PBCCS_ALIGN_NW &&
        !(std::isfinite(a.match_score) && std::isfinite(a.mismatch_score) && std::isfinite(a.gap_open) &&
          std::isfinite(a.gap_extend) && std::isfinite(a.partial_match_score)))
        return fail(PBCCS_EINVAL, "affine alignment parameters must be finite");
    if (band && band->mode != PBCCS_BAND_OFF && band->mode != PBCCS_BAND_AUTO && band->mode != PBCCS_BAND_WIDTH)
        return fail(PBCCS_EINVAL, "unknown band mode");
    if (band && band->mode == PBCCS_BAND_WIDTH && band->w < 0) return fail(PBCCS_EINVAL, "negative band half-width");
    for (int k = 0; k < n; ++k) {
        const pbccs_align_pair& p = pairs[k];
        if (p.target_len < 0 || p.query_len < 0 || (p.target_len > 0 && !p.target) || (p.query_len > 0 && !p.query))
            return fail(PBCCS_EINVAL, "bad pbccs_align_pair");
        if (out[k].cap < 0 || (out[k].cap > 0 && !out[k].transcript)) return fail(PBCCS_EINVAL, "bad pbccs_align_result");
    }
    return guarded([&] {
        const align::AlignScoring sc{a.kind,        a.match,          a.mismatch, a.insert,     a.delete_,
                                     a.match_score, a.mismatch_score, a.gap_open, a.gap_extend, a.partial_match_score};
        std::vector<align::PairView> pv(n);
        for (int k = 0; k < n; ++k) pv[k] = align::PairView{pairs[k].target, pairs[k].target_len, pairs[k].query, pairs[k].query_len};
        std::vector<align::PairResult> res(n);
        {
            std::lock_guard<std::mutex> lk(eng->alignMu);
            if (band && band->mode != PBCCS_BAND_OFF) {
                align::BandOptions bo;
                bo.on = true;
                bo.w = band->mode == PBCCS_BAND_WIDTH ? band->w : -1;
                std::vector<align::BandInfo> bi((size_t)n);
                eng->Align().RunBanded(sc, pv.data(), n, res.data(), bo, bi.data());
                if (info)
                    for (int k = 0; k < n; ++k)
                        info[k] = pbccs_align_band_info{bi[k].banded, bi[k].w, bi[k].attempts, bi[k].reason};
            } else {
                eng->Align().Run(sc, pv.data(), n, res.data());
                if (info)
                    for (int k = 0; k < n; ++k) info[k] = pbccs_align_band_info{0, 0, 0, 0};
            }
        }
        int rc = PBCCS_OK;
        bool small = false;
        for (int k = 0; k < n; ++k) {
            pbccs_align_result& o = out[k];
            const align::PairResult& r = res[k];
            o.len = (int)r.transcript.size();
            o.score_i = r.scoreI;
            o.score_f = r.scoreF;
            o.status = r.status;
            if (r.status != PBCCS_OK) {
                if (rc == PBCCS_OK) rc = r.status;
                continue;
            }
            if (o.len > o.cap) {
                o.status = PBCCS_ERANGE;
                small = true;
                continue;
            }
            if (o.len > 0) std::memcpy(o.transcript, r.transcript.data(), (size_t)o.len);
        }
        if (rc == PBCCS_EINVAL) return fail(rc, "a pair cannot be aligned (int32 overflow, or a traceback that leaves the matrix)");
        if (rc == PBCCS_EOOM) return fail(rc, "a pair's move store exceeds the align workspace (PBCCS_ALIGN_WORKSPACE_MB)");
        if (rc != PBCCS_OK) return fail(rc, "alignment failed");
        if (small) return fail(PBCCS_ERANGE, "transcript buffer too small");
        return PBCCS_OK;
    });
}

// the ends-free modes (align_modes_kernels.hip)
int pbccs_align_batch_ends(pbccs_engine* eng, const pbccs_align_params* params, const pbccs_align_ends* ends,
                           const pbccs_align_pair* pairs, int n, pbccs_align_result* out, pbccs_align_extent* ext)
{
    if (!eng || !params || !ends || n < 0 || (n > 0 && (!pairs || !out || !ext)))
        return fail(PBCCS_EINVAL, "bad argument");
    const pbccs_align_params& a = *params;
    if (a.kind != PBCCS_ALIGN_NW)
        return fail(PBCCS_EINVAL, "SEMIGLOBAL and LOCAL alignment are defined for the linear (NW) scores only");
    if (ends->mode == PBCCS_POA_GLOBAL) return fail(PBCCS_EINVAL, "GLOBAL alignment is pbccs_align_batch's");
    if (ends->mode != PBCCS_POA_SEMIGLOBAL && ends->mode != PBCCS_POA_LOCAL)
        return fail(PBCCS_EINVAL, "unknown alignment mode");
    if (a.insert > 0 || a.delete_ > 0)
        return fail(PBCCS_EINVAL, "SEMIGLOBAL and LOCAL alignment need Insert <= 0 and Delete <= 0");
    for (int k = 0; k < n; ++k) {
        const pbccs_align_pair& p = pairs[k];
        if (p.target_len < 0 || p.query_len < 0 || (p.target_len > 0 && !p.target) || (p.query_len > 0 && !p.query))
            return fail(PBCCS_EINVAL, "bad pbccs_align_pair");
        if (out[k].cap < 0 || (out[k].cap > 0 && !out[k].transcript)) return fail(PBCCS_EINVAL, "bad pbccs_align_result");
    }
    return guarded([&] {
        const align::AlignScoring sc{align::kNw, a.match, a.mismatch, a.insert, a.delete_, 0.f, 0.f, 0.f, 0.f, 0.f};
        std::vector<align::PairView> pv(n);
        for (int k = 0; k < n; ++k) pv[k] = align::PairView{pairs[k].target, pairs[k].target_len, pairs[k].query, pairs[k].query_len};
        std::vector<align::PairResult> res(n);
        std::vector<align::EndsExtent> ex(n);
        {
            std::lock_guard<std::mutex> lk(eng->alignMu);
            eng->Align().RunEnds(sc, ends->mode, ends->both_strands != 0, pv.data(), n, res.data(), ex.data());
        }
        int rc = PBCCS_OK;
        bool small = false;
        for (int k = 0; k < n; ++k) {
            pbccs_align_result& o = out[k];
            const align::PairResult& r = res[k];
            o.len = (int)r.transcript.size();
            o.score_i = r.scoreI;
            o.score_f = 0.f;
            o.status = r.status;
            ext[k] = pbccs_align_extent{ex[k].targetBegin, ex[k].targetEnd, ex[k].queryBegin, ex[k].queryEnd, ex[k].rc};
            if (r.status != PBCCS_OK) {
                if (rc == PBCCS_OK) rc = r.status;
                continue;
            }
            if (o.len > o.cap) {
                o.status = PBCCS_ERANGE;
                small = true;
                continue;
            }
            if (o.len > 0) std::memcpy(o.transcript, r.transcript.data(), (size_t)o.len);
        }
        if (rc == PBCCS_EINVAL) return fail(rc, "a pair cannot be aligned (int32 overflow)");
        if (rc == PBCCS_EOOM) return fail(rc, "a pair's move store exceeds the align workspace (PBCCS_ALIGN_WORKSPACE_MB)");
        if (rc != PBCCS_OK) return fail(rc, "alignment failed");
        if (small) return fail(PBCCS_ERANGE, "transcript buffer too small");
        return PBCCS_OK;
    });
}

int pbccs_align_stats_get(pbccs_engine* eng, pbccs_align_stats* out, int reset)
{
    if (!eng || !out) return fail(PBCCS_EINVAL, "bad argument");
    return guarded([&] {
        std::lock_guard<std::mutex> lk(eng->alignMu);
        const align::AlignStats s = eng->align ? eng->align->stats : align::AlignStats();
        *out = pbccs_align_stats{s.pairs, s.cells, s.launches, s.traceSteps, s.fillMs, s.traceMs, s.bytes, s.groups};
        if (reset && eng->align) eng->align->stats = align::AlignStats();
        return PBCCS_OK;
    });
}

namespace {
align::AlignScoring band_scoring(const pbccs_align_params& a)
{
    return align::AlignScoring{a.kind,        a.match,          a.mismatch, a.insert,     a.delete_,
                               a.match_score, a.mismatch_score, a.gap_open, a.gap_extend, a.partial_match_score};
}
bool band_args_ok(const pbccs_align_params* a, int I, int J)
{
    return a && I >= 0 && J >= 0 &&
           (a->kind == PBCCS_ALIGN_NW || a->kind == PBCCS_ALIGN_AFFINE || a->kind == PBCCS_ALIGN_AFFINE_IUPAC);
}
}  // namespace

int pbccs_align_band_bound(const pbccs_align_params* params, int query_len, int target_len, int w, double* u,
                           double* e, int* certifiable)
{
    if (!band_args_ok(params, query_len, target_len) || w < 0 || !u || !e || !certifiable)
        return fail(PBCCS_EINVAL, "bad argument");
    const align::BandBound b = align::band_bound(band_scoring(*params), query_len, target_len, w);
    *u = b.U;
    *e = b.E;
    *certifiable = b.certifiable ? 1 : 0;
    return PBCCS_OK;
}

int pbccs_align_band_widen(const pbccs_align_params* params, int query_len, int target_len, double score, int* w)
{
    if (!band_args_ok(params, query_len, target_len) || !w) return fail(PBCCS_EINVAL, "bad argument");
    *w = (int)align::band_widen(band_scoring(*params), query_len, target_len, score);
    return PBCCS_OK;
}

int pbccs_align_band_stats_get(pbccs_engine* eng, pbccs_align_band_stats* out, int reset)
{
    if (!eng || !out) return fail(PBCCS_EINVAL, "bad argument");
    return guarded([&] {
        std::lock_guard<std::mutex> lk(eng->alignMu);
        const align::AlignBandStats s = eng->align ? eng->align->bandStats : align::AlignBandStats();
        pbccs_align_band_stats o{};
        o.pairs = s.pairs;
        o.banded_pairs = s.bandedPairs;
        o.second_attempts = s.secondAttempts;
        for (int k = 0; k < 8; ++k) o.fallbacks[k] = s.fallbacks[k];
        o.band_cells = s.bandCells;
        o.full_cells = s.fullCells;
        o.launches = s.launches;
        o.groups = s.groups;
        o.trace_steps = s.traceSteps;
        o.store_bytes = s.storeBytes;
        o.fill_ms = s.fillMs;
        o.trace_ms = s.traceMs;
        *out = o;
        if (reset && eng->align) eng->align->bandStats = align::AlignBandStats();
        return PBCCS_OK;
    });
}

// ---- MapToDraft (map_kernels.hpp) ---------------------------------------------------------------------------
int pbccs_map_batch(pbccs_engine* eng, const pbccs_map_input* in, int n, float min_score_to_add,
                    pbccs_map_output* out)
{
    if (!eng || n < 0 || (n > 0 && (!in || !out))) return fail(PBCCS_EINVAL, "bad argument");
    for (int g = 0; g < n; ++g) {
        const pbccs_map_input& m = in[g];
        if (!m.draft || m.draft_len <= 0) return fail(PBCCS_EINVAL, "empty draft");
        if (m.n_reads < 0 || (m.n_reads > 0 && (!m.seqs || !m.lens))) return fail(PBCCS_EINVAL, "bad pbccs_map_input");
        if (m.draft_len > map::kMaxLen) return fail(PBCCS_EINVAL, "draft longer than 65535");
        for (int r = 0; r < m.n_reads; ++r) {
            if (m.lens[r] < 0 || (m.lens[r] > 0 && !m.seqs[r]))
                return fail(PBCCS_EINVAL, "bad read (NULL sequence or negative length)");
            if (m.lens[r] > map::kMaxLen) return fail(PBCCS_EINVAL, "read longer than 65535");
        }
    }
    return guarded([&] {
        std::vector<map::MapGroup> groups(n);
        for (int g = 0; g < n; ++g)
            groups[g] = map::MapGroup{in[g].draft, in[g].draft_len, in[g].seqs, in[g].lens, in[g].n_reads};
        std::vector<map::MapResult> res;
        {
            std::lock_guard<std::mutex> lk(eng->mapMu);
            eng->Map().Run(groups.data(), n, min_score_to_add, &res);
        }
        bool oom = false;
        size_t k = 0;
        for (int g = 0; g < n; ++g)
            for (int r = 0; r < in[g].n_reads; ++r, ++k) {
                const map::MapResult& m = res[k];
                oom = oom || m.status == PBCCS_EOOM;
                if (out[g].mapped) out[g].mapped[r] = m.mapped;
                if (out[g].rc) out[g].rc[r] = m.rc;
                if (out[g].score) out[g].score[r] = m.score;
                if (out[g].extents)
                    for (int e = 0; e < 4; ++e) out[g].extents[4 * r + e] = m.ext[e];
            }
        if (oom) return fail(PBCCS_EOOM, "a read's boundary buffers exceed the map workspace (PBCCS_MAP_WORKSPACE_KB)");
        return PBCCS_OK;
    });
}

int pbccs_map_stats_get(pbccs_engine* eng, pbccs_map_stats* out, int reset)
{
    if (!eng || !out) return fail(PBCCS_EINVAL, "bad argument");
    return guarded([&] {
        std::lock_guard<std::mutex> lk(eng->mapMu);
        const map::MapStats s = eng->mapper ? eng->mapper->stats : map::MapStats();
        *out = pbccs_map_stats{s.jobs, s.cells, s.launches, s.strips, s.deviceMs};
        if (reset && eng->mapper) eng->mapper->stats = map::MapStats();
        return PBCCS_OK;
    });
}

// ---- split mapping (split_map_kernels.hpp) ------------------------------------------------------------------
int pbccs_split_map_batch(pbccs_engine* eng, const pbccs_map_input* in, int n, int jump_penalty, int max_segments,
                          pbccs_split_map_output* out)
{
    if (!eng || n < 0 || (n > 0 && (!in || !out))) return fail(PBCCS_EINVAL, "bad argument");
    if (jump_penalty < 0) jump_penalty = PBCCS_SPLIT_JUMP_PENALTY;
    if (max_segments <= 0) max_segments = PBCCS_SPLIT_MAX_SEGMENTS;
    if (max_segments > map::kSplitMaxSegments) return fail(PBCCS_EINVAL, "max_segments above 64");
    for (int g = 0; g < n; ++g) {
        const pbccs_map_input& m = in[g];
        if (!m.draft || m.draft_len <= 0) return fail(PBCCS_EINVAL, "empty draft");
        if (m.n_reads < 0 || (m.n_reads > 0 && (!m.seqs || !m.lens))) return fail(PBCCS_EINVAL, "bad pbccs_map_input");
        if (m.draft_len > map::kMaxLen) return fail(PBCCS_EINVAL, "draft longer than 65535");
        for (int r = 0; r < m.n_reads; ++r) {
            if (m.lens[r] < 0 || (m.lens[r] > 0 && !m.seqs[r]))
                return fail(PBCCS_EINVAL, "bad read (NULL sequence or negative length)");
            if (m.lens[r] > map::kMaxLen) return fail(PBCCS_EINVAL, "read longer than 65535");
        }
    }
    return guarded([&] {
        std::vector<map::MapGroup> groups(n);
        for (int g = 0; g < n; ++g)
            groups[g] = map::MapGroup{in[g].draft, in[g].draft_len, in[g].seqs, in[g].lens, in[g].n_reads};
        std::vector<map::SplitMapResult> res;
        {
            std::lock_guard<std::mutex> lk(eng->mapMu);
            eng->SplitMap().Run(groups.data(), n, jump_penalty, max_segments, &res);
        }
        bool oom = false;
        size_t k = 0;
        for (int g = 0; g < n; ++g)
            for (int r = 0; r < in[g].n_reads; ++r, ++k) {
                const map::SplitMapResult& m = res[k];
                oom = oom || m.status == PBCCS_EOOM;
                if (out[g].n_segments) out[g].n_segments[r] = m.count;
                if (out[g].truncated) out[g].truncated[r] = m.truncated;
                if (out[g].score) out[g].score[r] = m.score;
                if (out[g].segments) {
                    int* sg = out[g].segments + (size_t)r * max_segments * 6;
                    std::fill(sg, sg + (size_t)max_segments * 6, 0);
                    for (const map::SplitSeg& s : m.segs) {
                        const int v[6] = {s.rc, s.rb, s.re, s.tb, s.te, s.score};
                        sg = std::copy(v, v + 6, sg);
                    }
                }
            }
        if (oom) return fail(PBCCS_EOOM, "a read's buffers exceed the split-map workspace (PBCCS_SPLIT_WORKSPACE_KB)");
        return PBCCS_OK;
    });
}

int pbccs_split_map_stats_get(pbccs_engine* eng, pbccs_split_map_stats* out, int reset)
{
    if (!eng || !out) return fail(PBCCS_EINVAL, "bad argument");
    return guarded([&] {
        std::lock_guard<std::mutex> lk(eng->mapMu);
        const map::SplitMapStats s = eng->splitMapper ? eng->splitMapper->stats : map::SplitMapStats();
        *out = pbccs_split_map_stats{s.jobs, s.cells, s.launches, s.tiled, s.deviceMs};
        if (reset && eng->splitMapper) eng->splitMapper->stats = map::SplitMapStats();
        return PBCCS_OK;
    });
}

// ---- consensus kinetics (kinetics_kernels.hpp) -------------------------------------------------------------
namespace {
// ConsensusCore Sequence.cpp:44-105 (ComplementArray; note N <-> M), as k_map_fill's complement()
char kin_complement(char c)
{
    switch (c) {
        case 'A': return 'T'; case 'C': return 'G'; case 'G': return 'C'; case 'T': return 'A';
        case 'a': return 't'; case 'c': return 'g'; case 'g': return 'c'; case 't': return 'a';
        case 'N': return 'M'; case 'M': return 'N'; case 'n': return 'm'; case 'm': return 'n';
        case '-': return '-';
    }
    return 127;
}

void kin_outputs(const std::vector<kinetics::ZmwOut>& zo, int n, pbccs_kinetics_output* out)
{
    for (int z = 0; z < n; ++z) {
        out[z].n_contributed[0] = zo[z].contributed[0];
        out[z].n_contributed[1] = zo[z].contributed[1];
    }
}

kinetics::ZmwOut kin_out_view(const pbccs_kinetics_output& o)
{
    kinetics::ZmwOut v;
    for (int k = 0; k < 4; ++k) {
        v.mean[k] = o.mean[k];
        v.code[k] = o.code[k];
        v.coverage[k] = o.coverage[k];
    }
    v.contributed[0] = v.contributed[1] = 0;
    v.readStatus = o.read_status;
    return v;
}
}  // namespace

void pbccs_kinetics_options_default(pbccs_kinetics_options* o)
{
    if (!o) return;
    o->band.mode = PBCCS_BAND_OFF;
    o->band.w = 0;
}

int pbccs_kinetics_pileup(pbccs_engine* eng, const pbccs_kinetics_pileup_input* in, int n, pbccs_kinetics_output* out)
{
    if (!eng || n < 0 || (n > 0 && (!in || !out))) return fail(PBCCS_EINVAL, "bad argument");
    for (int z = 0; z < n; ++z)
        if (in[z].consensus_len < 0 || in[z].n_reads < 0 || (in[z].n_reads > 0 && !in[z].reads))
            return fail(PBCCS_EINVAL, "bad pbccs_kinetics_pileup_input");
    return guarded([&] {
        std::vector<std::vector<kinetics::ReadView>> rv((size_t)n);
        std::vector<kinetics::ZmwView> zv((size_t)n);
        std::vector<kinetics::ZmwOut> zo((size_t)n);
        for (int z = 0; z < n; ++z) {
            rv[z].resize((size_t)in[z].n_reads);
            for (int k = 0; k < in[z].n_reads; ++k) {
                const pbccs_kinetics_read& r = in[z].reads[k];
                rv[z][k] = kinetics::ReadView{r.transcript, r.transcript_len, r.rc, r.rb, r.tb, r.te,
                                              r.len,        r.ip,             r.pw, kinetics::kUsed};
            }
            zv[z] = kinetics::ZmwView{in[z].consensus_len, rv[z].data(), in[z].n_reads};
            zo[z] = kin_out_view(out[z]);
        }
        {
            std::lock_guard<std::mutex> lk(eng->kineticsMu);
            eng->Kinetics().Run(zv.data(), n, zo.data());   // vets every read before any device work
        }
        kin_outputs(zo, n, out);
        return PBCCS_OK;
    });
}

namespace {
extern "C++" {   // templates inside the ABI's extern "C" block
// The placement and alignment stage pbccs_kinetics_batch and pbccs_pileup_batch share, for the ZMWs [z0, z1) of an
// input with consensus, consensus_len, n_reads, seqs and lens: pbccs_map_batch's placement, then Align (NW, default
// parameters) of consensus[tb, te) against the oriented read's [rb, re).
struct PlacedRead {
    int rc, rb, re, tb, te;
    int skip;         // kinetics::kUsed, or why the read is skipped
    const char* tr;   // the transcript (owned by the stage), NULL for a skipped read
    int trLen;
};
struct PlaceStage {
    std::vector<std::vector<PlacedRead>> reads;   // per ZMW of the slice
    std::vector<std::string> oriented;            // the reverse-complemented extents (the forward ones are views)
    std::vector<align::PairResult> res;
};

template <class In>
void place_and_align(pbccs_engine* eng, const In* in, int z0, int z1, const pbccs_align_band& band, PlaceStage& st)
{
    const int n = z1 - z0;
    std::vector<map::MapGroup> groups((size_t)n);
    for (int g = 0; g < n; ++g) {
        const In& m = in[z0 + g];
        groups[g] = map::MapGroup{m.consensus, m.consensus_len, m.seqs, m.lens, m.n_reads};
    }
    std::vector<map::MapResult> placed;
    {
        std::lock_guard<std::mutex> lk(eng->mapMu);
        eng->Map().Run(groups.data(), n, 0.0f, &placed);
    }
    // the pairs: consensus[tb, te) against the oriented read's [rb, re)
    st.reads.assign((size_t)n, {});
    std::vector<align::PairView> pairs;
    std::vector<std::pair<int, int>> pairOf;   // (ZMW of the slice, read)
    size_t idx = 0, nRev = 0;
    for (int g = 0; g < n; ++g)
        for (int r = 0; r < in[z0 + g].n_reads; ++r, ++idx)
            if (placed[idx].mapped && placed[idx].rc) ++nRev;
    st.oriented.clear();
    st.oriented.reserve(nRev);   // the pairs keep pointers into the strings
    idx = 0;
    for (int g = 0; g < n; ++g) {
        const In& m = in[z0 + g];
        st.reads[g].resize((size_t)m.n_reads);
        for (int r = 0; r < m.n_reads; ++r, ++idx) {
            const map::MapResult& p = placed[idx];
            PlacedRead& v = st.reads[g][r];
            const int rb = p.ext[0], re = p.ext[1], tb = p.ext[2], te = p.ext[3];
            v = PlacedRead{p.rc, rb, re, tb, te, kinetics::kUsed, nullptr, 0};
            if (!p.mapped) {
                v.skip = kinetics::kUnmapped;
                continue;
            }
            if (re <= rb || te <= tb) {
                v.skip = kinetics::kEmptyExtent;
                continue;
            }
            const char* q = m.seqs[r] + rb;
            if (p.rc) {
                std::string s((size_t)(re - rb), ' ');
                const int I = m.lens[r];
                for (int k = rb; k < re; ++k) s[(size_t)(k - rb)] = kin_complement(m.seqs[r][I - 1 - k]);
                st.oriented.push_back(std::move(s));
                q = st.oriented.back().data();
            }
            pairs.push_back(align::PairView{m.consensus + tb, te - tb, q, re - rb});
            pairOf.emplace_back(g, r);
        }
    }
    const int np = (int)pairs.size();
    st.res.assign((size_t)np, align::PairResult());
    if (np) {
        const align::AlignScoring sc{PBCCS_ALIGN_NW, 0, -1, -1, -1, 0.f, 0.f, 0.f, 0.f, 0.f};   // AlignConfig::Default()
        std::lock_guard<std::mutex> lk(eng->alignMu);
        if (band.mode != PBCCS_BAND_OFF) {
            align::BandOptions bo;
            bo.on = true;
            bo.w = band.mode == PBCCS_BAND_WIDTH ? band.w : -1;
            eng->Align().RunBanded(sc, pairs.data(), np, st.res.data(), bo, nullptr);
        } else {
            eng->Align().Run(sc, pairs.data(), np, st.res.data());
        }
    }
    for (int k = 0; k < np; ++k) {
        PlacedRead& v = st.reads[pairOf[k].first][pairOf[k].second];
        if (st.res[k].status != PBCCS_OK) {
            v.skip = kinetics::kAlignFailed;
            continue;
        }
        v.tr = st.res[k].transcript.data();
        v.trLen = (int)st.res[k].transcript.size();
    }
}

// The kinetics pileup of the stage's reads: ZMW g of the stage goes to outs[g] where that is not NULL
template <class In>
void kinetics_of_stage(pbccs_engine* eng, const In* in, int z0, const PlaceStage& st,
                       const std::vector<pbccs_kinetics_output*>& outs)
{
    const int n = (int)st.reads.size();
    std::vector<std::vector<kinetics::ReadView>> rv;
    std::vector<kinetics::ZmwView> zv;
    std::vector<kinetics::ZmwOut> zo;
    std::vector<pbccs_kinetics_output*> dst;
    rv.reserve((size_t)n);
    for (int g = 0; g < n; ++g) {
        if (!outs[g]) continue;
        const In& m = in[z0 + g];
        rv.emplace_back((size_t)m.n_reads);
        for (int r = 0; r < m.n_reads; ++r) {
            const PlacedRead& p = st.reads[g][r];
            rv.back()[r] = kinetics::ReadView{p.tr, p.trLen, p.rc, p.rb, p.tb, p.te, m.lens[r],
                                              m.ip ? m.ip[r] : nullptr, m.pw ? m.pw[r] : nullptr, p.skip};
        }
        zv.push_back(kinetics::ZmwView{m.consensus_len, rv.back().data(), m.n_reads});
        zo.push_back(kin_out_view(*outs[g]));
        dst.push_back(outs[g]);
    }
    if (zv.empty()) return;
    {
        std::lock_guard<std::mutex> lk(eng->kineticsMu);
        eng->Kinetics().Run(zv.data(), (int)zv.size(), zo.data());
    }
    for (size_t k = 0; k < dst.size(); ++k) kin_outputs({zo[k]}, 1, dst[k]);
}

}  // extern "C++"

// One slice of pbccs_kinetics_batch: ZMWs [z0, z1)
void kinetics_slice(pbccs_engine* eng, const pbccs_kinetics_input* in, int z0, int z1,
                    const pbccs_kinetics_options& opts, pbccs_kinetics_output* out)
{
    PlaceStage st;
    place_and_align(eng, in, z0, z1, opts.band, st);
    std::vector<pbccs_kinetics_output*> outs((size_t)(z1 - z0));
    for (int g = 0; g < z1 - z0; ++g) outs[g] = out + z0 + g;
    kinetics_of_stage(eng, in, z0, st, outs);
}
}  // namespace

int pbccs_kinetics_batch(pbccs_engine* eng, const pbccs_kinetics_input* in, int n, const pbccs_kinetics_options* opts,
                         pbccs_kinetics_output* out)
{
    if (!eng || n < 0 || (n > 0 && (!in || !out))) return fail(PBCCS_EINVAL, "bad argument");
    pbccs_kinetics_options o;
    pbccs_kinetics_options_default(&o);
    if (opts) o = *opts;
    if (o.band.mode != PBCCS_BAND_OFF && o.band.mode != PBCCS_BAND_AUTO && o.band.mode != PBCCS_BAND_WIDTH)
        return fail(PBCCS_EINVAL, "unknown band mode");
    if (o.band.mode == PBCCS_BAND_WIDTH && o.band.w < 0) return fail(PBCCS_EINVAL, "negative band half-width");
    for (int g = 0; g < n; ++g) {
        const pbccs_kinetics_input& m = in[g];
        if (!m.consensus || m.consensus_len <= 0) return fail(PBCCS_EINVAL, "empty consensus");
        if (m.n_reads < 0 || (m.n_reads > 0 && (!m.seqs || !m.lens)))
            return fail(PBCCS_EINVAL, "bad pbccs_kinetics_input");
        if (m.consensus_len > map::kMaxLen) return fail(PBCCS_EINVAL, "consensus longer than 65535");
        for (int r = 0; r < m.n_reads; ++r) {
            if (m.lens[r] < 0 || (m.lens[r] > 0 && !m.seqs[r]))
                return fail(PBCCS_EINVAL, "bad read (NULL sequence or negative length)");
            if (m.lens[r] > map::kMaxLen) return fail(PBCCS_EINVAL, "read longer than 65535");
        }
    }
    return guarded([&] {
        // slices of at most kSliceBases read bases bound the host copies and the device pools of one pass
        constexpr long long kSliceBases = 32LL << 20;
        int z0 = 0;
        while (z0 < n) {
            long long bases = 0;
            int z1 = z0;
            while (z1 < n) {
                long long b = 0;
                for (int r = 0; r < in[z1].n_reads; ++r) b += in[z1].lens[r];
                if (z1 > z0 && bases + b > kSliceBases) break;
                bases += b;
                ++z1;
            }
            kinetics_slice(eng, in, z0, z1, o, out);
            z0 = z1;
        }
        return PBCCS_OK;
    });
}

int pbccs_kinetics_stats_get(pbccs_engine* eng, pbccs_kinetics_stats* out, int reset)
{
    if (!eng || !out) return fail(PBCCS_EINVAL, "bad argument");
    return guarded([&] {
        std::lock_guard<std::mutex> lk(eng->kineticsMu);
        const kinetics::KinStats s = eng->kineticsRunner ? eng->kineticsRunner->stats : kinetics::KinStats();
        *out = pbccs_kinetics_stats{s.reads,     s.unmapped, s.emptyExtent, s.alignFailed, s.columns,
                                    s.positions, s.launches, s.columnsMs,   s.reduceMs};
        if (reset && eng->kineticsRunner) eng->kineticsRunner->stats = kinetics::KinStats();
        return PBCCS_OK;
    });
}

// ---- subread pileup (pileup_kernels.hpp) ---------------------------------------------------------------------
namespace {
pileup::ZmwOut pile_out_view(const pbccs_pileup_output& o)
{
    pileup::ZmwOut v;
    v.counts = o.counts;
    v.insReads = o.ins_reads;
    v.insBases = o.ins_bases;
    v.slotCov = o.slot_cov;
    v.cov = o.cov;
    v.maxIns = o.max_ins;
    v.plurality = o.plurality;
    v.insPlurality = o.ins_plurality;
    v.readStatus = o.read_status;
    v.nMatch = o.n_match;
    v.nMismatch = o.n_mismatch;
    v.nIns = o.n_ins;
    v.nDel = o.n_del;
    v.covSum = 0;
    v.nUsed[0] = v.nUsed[1] = 0;
    return v;
}

// the per-ZMW figures and the placement of n reads
void pile_outputs(const pileup::ZmwOut& zo, const pileup::ZmwView& zv, pbccs_pileup_output& o)
{
    o.cov_sum = zo.covSum;
    o.n_used[0] = zo.nUsed[0];
    o.n_used[1] = zo.nUsed[1];
    for (int k = 0; k < zv.n; ++k) {
        const pileup::ReadView& r = zv.reads[k];
        if (o.rc) o.rc[k] = r.rc ? 1 : 0;
        if (o.rb) o.rb[k] = r.rb;
        if (o.tb) o.tb[k] = r.tb;
        if (o.te) o.te[k] = r.te;
    }
}

bool bad_columns_input(const pbccs_pileup_columns_input* in, int n)
{
    for (int z = 0; z < n; ++z)
        if (in[z].consensus_len < 0 || in[z].n_reads < 0 || (in[z].n_reads > 0 && !in[z].reads) ||
            (in[z].consensus_len > 0 && !in[z].consensus))
            return true;
    return false;
}

void columns_views(const pbccs_pileup_columns_input* in, int n, std::vector<std::vector<pileup::ReadView>>& rv,
                   std::vector<pileup::ZmwView>& zv)
{
    rv.assign((size_t)n, {});
    zv.assign((size_t)n, pileup::ZmwView());
    for (int z = 0; z < n; ++z) {
        rv[z].resize((size_t)in[z].n_reads);
        for (int k = 0; k < in[z].n_reads; ++k) {
            const pbccs_pileup_read& r = in[z].reads[k];
            rv[z][k] = pileup::ReadView{r.transcript, r.transcript_len, r.seq, r.len, r.rc, r.rb, r.tb, r.te,
                                        pileup::kUsed};
        }
        zv[z] = pileup::ZmwView{in[z].consensus, in[z].consensus_len, rv[z].data(), in[z].n_reads};
    }
}

// re of a read from its transcript's read columns (pbccs_pileup_columns, where the caller gives no re)
int read_end(const pileup::ReadView& r)
{
    int nq = 0;
    for (int k = 0; k < r.trLen; ++k) nq += r.tr[k] != 'D';
    return r.rb + nq;
}
}  // namespace

void pbccs_pileup_options_default(pbccs_pileup_options* o)
{
    if (!o) return;
    o->band.mode = PBCCS_BAND_OFF;
    o->band.w = 0;
}

int pbccs_pileup_columns(pbccs_engine* eng, const pbccs_pileup_columns_input* in, int n, pbccs_pileup_output* out)
{
    if (!eng || n < 0 || (n > 0 && (!in || !out))) return fail(PBCCS_EINVAL, "bad argument");
    if (bad_columns_input(in, n)) return fail(PBCCS_EINVAL, "bad pbccs_pileup_columns_input");
    return guarded([&] {
        std::vector<std::vector<pileup::ReadView>> rv;
        std::vector<pileup::ZmwView> zv;
        columns_views(in, n, rv, zv);
        std::vector<pileup::ZmwOut> zo((size_t)n);
        for (int z = 0; z < n; ++z) zo[z] = pile_out_view(out[z]);
        {
            std::lock_guard<std::mutex> lk(eng->pileupMu);
            eng->Pileup().Run(zv.data(), n, zo.data(), nullptr);   // vets every read before any device work
        }
        for (int z = 0; z < n; ++z) {
            pile_outputs(zo[z], zv[z], out[z]);
            for (int k = 0; k < zv[z].n; ++k) {
                const bool used = !out[z].read_status || out[z].read_status[k] == PBCCS_KIN_USED;
                if (out[z].re) out[z].re[k] = used ? read_end(rv[z][k]) : rv[z][k].rb;
                if (out[z].transcript_lens) out[z].transcript_lens[k] = 0;
            }
        }
        return PBCCS_OK;
    });
}

int pbccs_pileup_msa(pbccs_engine* eng, const pbccs_pileup_columns_input* in, int n, int* widths, int* const* cols,
                     char* const* rows)
{
    if (!eng || n < 0 || (n > 0 && (!in || !widths))) return fail(PBCCS_EINVAL, "bad argument");
    if (bad_columns_input(in, n)) return fail(PBCCS_EINVAL, "bad pbccs_pileup_columns_input");
    return guarded([&] {
        std::vector<std::vector<pileup::ReadView>> rv;
        std::vector<pileup::ZmwView> zv;
        columns_views(in, n, rv, zv);
        std::vector<pileup::MsaOut> mo((size_t)n);
        for (int z = 0; z < n; ++z)
            mo[z] = pileup::MsaOut{0, cols ? cols[z] : nullptr, rows ? rows[z] : nullptr, widths[z]};
        {
            std::lock_guard<std::mutex> lk(eng->pileupMu);
            eng->Pileup().Run(zv.data(), n, nullptr, mo.data());
        }
        for (int z = 0; z < n; ++z) widths[z] = mo[z].width;
        return PBCCS_OK;
    });
}

namespace {
// One slice of pbccs_pileup_batch: ZMWs [z0, z1)
void pileup_slice(pbccs_engine* eng, const pbccs_pileup_input* in, int z0, int z1, const pbccs_pileup_options& opts,
                  pbccs_pileup_output* out)
{
    const int n = z1 - z0;
    PlaceStage st;
    place_and_align(eng, in, z0, z1, opts.band, st);
    std::vector<pbccs_kinetics_output*> kout((size_t)n);
    long long placed = 0, shared = 0;
    for (int g = 0; g < n; ++g) {
        kout[g] = in[z0 + g].kinetics;
        placed += in[z0 + g].n_reads;
        if (kout[g]) shared += in[z0 + g].n_reads;
    }
    kinetics_of_stage(eng, in, z0, st, kout);
    std::vector<std::vector<pileup::ReadView>> rv((size_t)n);
    std::vector<pileup::ZmwView> zv((size_t)n);
    std::vector<pileup::ZmwOut> zo((size_t)n);
    for (int g = 0; g < n; ++g) {
        const pbccs_pileup_input& m = in[z0 + g];
        rv[g].resize((size_t)m.n_reads);
        for (int r = 0; r < m.n_reads; ++r) {
            const PlacedRead& p = st.reads[g][r];
            rv[g][r] = pileup::ReadView{p.tr, p.trLen, m.seqs[r], m.lens[r], p.rc, p.rb, p.tb, p.te, p.skip};
        }
        zv[g] = pileup::ZmwView{m.consensus, m.consensus_len, rv[g].data(), m.n_reads};
        zo[g] = pile_out_view(out[z0 + g]);
    }
    {
        std::lock_guard<std::mutex> lk(eng->pileupMu);
        pileup::PileupRunner& run = eng->Pileup();
        run.Run(zv.data(), n, zo.data(), nullptr);
        run.stats.placed += placed;
        run.stats.shared += shared;
    }
    for (int g = 0; g < n; ++g) {
        pbccs_pileup_output& o = out[z0 + g];
        pile_outputs(zo[g], zv[g], o);
        for (int r = 0; r < zv[g].n; ++r) {
            const PlacedRead& p = st.reads[g][r];
            if (o.re) o.re[r] = p.re;
            const bool used = p.skip == pileup::kUsed && p.tr;
            if (o.transcript_lens) o.transcript_lens[r] = used ? p.trLen : 0;
            if (used && o.transcripts && o.transcripts[r] && p.trLen > 0 &&
                p.trLen <= in[z0 + g].consensus_len + in[z0 + g].lens[r])
                std::memcpy(o.transcripts[r], p.tr, (size_t)p.trLen);
        }
    }
}
}  // namespace

int pbccs_pileup_batch(pbccs_engine* eng, const pbccs_pileup_input* in, int n, const pbccs_pileup_options* opts,
                       pbccs_pileup_output* out)
{
    if (!eng || n < 0 || (n > 0 && (!in || !out))) return fail(PBCCS_EINVAL, "bad argument");
    pbccs_pileup_options o;
    pbccs_pileup_options_default(&o);
    if (opts) o = *opts;
    if (o.band.mode != PBCCS_BAND_OFF && o.band.mode != PBCCS_BAND_AUTO && o.band.mode != PBCCS_BAND_WIDTH)
        return fail(PBCCS_EINVAL, "unknown band mode");
    if (o.band.mode == PBCCS_BAND_WIDTH && o.band.w < 0) return fail(PBCCS_EINVAL, "negative band half-width");
    for (int g = 0; g < n; ++g) {
        const pbccs_pileup_input& m = in[g];
        if (!m.consensus || m.consensus_len <= 0) return fail(PBCCS_EINVAL, "empty consensus");
        if (m.n_reads < 0 || (m.n_reads > 0 && (!m.seqs || !m.lens)))
            return fail(PBCCS_EINVAL, "bad pbccs_pileup_input");
        if (m.consensus_len > map::kMaxLen) return fail(PBCCS_EINVAL, "consensus longer than 65535");
        for (int r = 0; r < m.n_reads; ++r) {
            if (m.lens[r] < 0 || (m.lens[r] > 0 && !m.seqs[r]))
                return fail(PBCCS_EINVAL, "bad read (NULL sequence or negative length)");
            if (m.lens[r] > map::kMaxLen) return fail(PBCCS_EINVAL, "read longer than 65535");
        }
    }
    return guarded([&] {
        // slices as pbccs_kinetics_batch's
        constexpr long long kSliceBases = 32LL << 20;
        int z0 = 0;
        while (z0 < n) {
            long long bases = 0;
            int z1 = z0;
            while (z1 < n) {
                long long b = 0;
                for (int r = 0; r < in[z1].n_reads; ++r) b += in[z1].lens[r];
                if (z1 > z0 && bases + b > kSliceBases) break;
                bases += b;
                ++z1;
            }
            pileup_slice(eng, in, z0, z1, o, out);
            z0 = z1;
        }
        return PBCCS_OK;
    });
}

int pbccs_pileup_stats_get(pbccs_engine* eng, pbccs_pileup_stats* out, int reset)
{
    if (!eng || !out) return fail(PBCCS_EINVAL, "bad argument");
    return guarded([&] {
        std::lock_guard<std::mutex> lk(eng->pileupMu);
        const pileup::PileStats s = eng->pileupRunner ? eng->pileupRunner->stats : pileup::PileStats();
        *out = pbccs_pileup_stats{s.reads,    s.unmapped, s.emptyExtent, s.alignFailed, s.columns, s.slots, s.launches,
                                  s.placed,   s.shared,   s.columnsMs,   s.reduceMs,    s.scanMs,  s.rowsMs};
        if (reset && eng->pileupRunner) eng->pileupRunner->stats = pileup::PileStats();
        return PBCCS_OK;
    });
}

// ---- SparseAlign (sparse_kernels.hpp) -----------------------------------------------------------------------
int pbccs_sparse_align_batch(pbccs_engine* eng, int k, const pbccs_sparse_align_input* in, int n,
                             pbccs_sparse_align_output* out)
{
    if (!eng || n < 0 || (n > 0 && (!in || !out))) return fail(PBCCS_EINVAL, "bad argument");
    if (k < sparse::kMinK || k > sparse::kMaxK) return fail(PBCCS_EINVAL, "SparseAlign: k must be 4..8");
    for (int g = 0; g < n; ++g) {
        const pbccs_sparse_align_input& s = in[g];
        if (s.target_len < 0 || s.query_len < 0 || (s.target_len > 0 && !s.target) || (s.query_len > 0 && !s.query) ||
            s.anchor_cap < 0 || (s.anchor_cap > 0 && !s.anchors))
            return fail(PBCCS_EINVAL, "bad pbccs_sparse_align_input (NULL buffer or negative length)");
    }
    return guarded([&] {
        std::vector<sparse::SparseInput> jobs(n);
        for (int g = 0; g < n; ++g)
            jobs[g] = sparse::SparseInput{in[g].target, in[g].target_len, in[g].query, in[g].query_len,
                                          in[g].reverse_complement, in[g].anchors, in[g].anchor_cap, in[g].ranges};
        std::vector<sparse::SparseResult> res;
        {
            std::lock_guard<std::mutex> lk(eng->sparseMu);
            eng->Sparse().Run(k, jobs.data(), n, &res);
        }
        int first = PBCCS_OK;
        for (int g = 0; g < n; ++g) {
            out[g] = pbccs_sparse_align_output{res[g].status, res[g].nAnchors, res[g].nSeeds, res[g].score};
            if (first == PBCCS_OK) first = res[g].status;
        }
        if (first == PBCCS_EINVAL) return fail(first, "SparseAlign: a letter outside ACGT, or a sequence longer than 1048576");
        if (first == PBCCS_EOOM)
            return fail(first, "SparseAlign: a pair exceeds the seed cap (PBCCS_SPARSE_MAX_SEEDS) or the workspace "
                               "(PBCCS_SPARSE_WORKSPACE_KB)");
        if (first == PBCCS_ERANGE) return fail(first, "SparseAlign: a chain is longer than its anchor buffer");
        return first;
    });
}

int pbccs_sparse_align_stats_get(pbccs_engine* eng, pbccs_sparse_align_stats* out, int reset)
{
    if (!eng || !out) return fail(PBCCS_EINVAL, "bad argument");
    return guarded([&] {
        std::lock_guard<std::mutex> lk(eng->sparseMu);
        const sparse::SparseStats s = eng->sparseRunner ? eng->sparseRunner->stats : sparse::SparseStats();
        *out = pbccs_sparse_align_stats{s.jobs, s.seeds, s.anchors, s.launches, s.deviceMs, s.rangeCells, s.fullCells};
        if (reset && eng->sparseRunner) eng->sparseRunner->stats = sparse::SparseStats();
        return PBCCS_OK;
    });
}

// ---- Windowed polish (window_kernels.hpp) ------------------------------------------------------
void pbccs_window_options_default(pbccs_window_options* o)
{
    if (!o) return;
    o->window = 2000;
    o->overlap = 200;
    o->guard = 8;
    o->k = 6;
}

static bool window_options_ok(const pbccs_window_options* w)
{
    return w && w->window > w->overlap && w->guard >= 1 && (long long)w->overlap >= 2LL * w->guard &&
           w->k >= sparse::kMinK && w->k <= sparse::kMaxK;
}

// Rule 1
static std::vector<std::pair<int, int>> window_bounds(int L, const pbccs_window_options& w)
{
    std::vector<std::pair<int, int>> v;
    if (L <= (long long)w.window + w.overlap) {
        v.emplace_back(0, std::max(0, L));
        return v;
    }
    const long long span = (long long)L - w.overlap;
    const long long n = (span + w.window - 1) / w.window;
    const long long S = (span + n - 1) / n;
    for (long long i = 0; i < n; ++i)
        v.emplace_back((int)(i * S), (int)std::min<long long>(L, i * S + S + w.overlap));
    return v;
}

int pbccs_window_plan(int draft_len, const pbccs_window_options* w, int* bounds, int cap, int* n_windows)
{
    if (!window_options_ok(w)) return fail(PBCCS_EINVAL, "window options: need window > overlap >= 2 guard, guard >= 1, 4 <= k <= 8");
    if (draft_len < 0 || !n_windows || cap < 0 || (cap > 0 && !bounds)) return fail(PBCCS_EINVAL, "bad argument");
    return guarded([&] {
        const std::vector<std::pair<int, int>> v = window_bounds(draft_len, *w);
        *n_windows = (int)v.size();
        if ((int)v.size() > cap) return fail(PBCCS_ERANGE, "bounds buffer too small");
        for (size_t i = 0; i < v.size(); ++i) bounds[2 * i] = v[i].first, bounds[2 * i + 1] = v[i].second;
        return PBCCS_OK;
    });
}

// Rule 4 on one transcript: per draft column the index of its character, and TargetToQueryPositions.
static bool window_columns(const char* t, int len, int width, std::vector<int>* col, std::vector<int>* ttq)
{
    col->clear();
    ttq->clear();
    int q = 0;
    for (int x = 0; x < len; ++x) {
        const char c = t[x];
        if (c == 'M' || c == 'R') col->push_back(x), ttq->push_back(q++);
        else if (c == 'D') col->push_back(x), ttq->push_back(q);
        else if (c == 'I') ++q;
        else return false;
    }
    ttq->push_back(q);
    return (int)col->size() == width;
}

static bool window_good_at(const char* t, int len, const std::vector<int>& col, int rel, int g)
{
    if (rel - g < 0 || rel + g > (int)col.size()) return false;
    const int x0 = col[rel - g];
    if (x0 + 2 * g > len) return false;
    for (int x = x0; x < x0 + 2 * g; ++x)
        if (t[x] != 'M') return false;
    return true;
}

int pbccs_window_join(const char* transcript_a, int len_a, int begin_a, int end_a, const char* transcript_b,
                      int len_b, int begin_b, int end_b, int guard, int* found, int* p, int* cut_a, int* cut_b)
{
    if (len_a < 0 || len_b < 0 || (len_a > 0 && !transcript_a) || (len_b > 0 && !transcript_b) || guard < 1 || !found ||
        !p || !cut_a || !cut_b || begin_a < 0 || begin_a > end_a || begin_b > end_b || begin_a >= begin_b)
        return fail(PBCCS_EINVAL, "bad argument");
    return guarded([&] {
        std::vector<int> colA, colB, ttqA, ttqB;
        if (!window_columns(transcript_a, len_a, end_a - begin_a, &colA, &ttqA) ||
            !window_columns(transcript_b, len_b, end_b - begin_b, &colB, &ttqB))
            return fail(PBCCS_EINVAL, "a transcript does not span its window or holds a character other than M R I D");
        *found = 0;
        *p = -1;
        *cut_a = *cut_b = 0;
        const long long lo = (long long)begin_b + guard, hi = (long long)end_a - guard;
        if (lo > hi) return PBCCS_OK;
        const long long mid = ((long long)begin_b + end_a) / 2;
        for (long long d = 0; mid - d >= lo || mid + d <= hi; ++d) {
            for (int side = 0; side < (d == 0 ? 1 : 2); ++side) {
                const long long c = side == 0 ? mid + d : mid - d;
                if (c < lo || c > hi || c - begin_b > end_b - begin_b) continue;
                const int ra = (int)(c - begin_a), rb = (int)(c - begin_b);
                if (!window_good_at(transcript_a, len_a, colA, ra, guard) ||
                    !window_good_at(transcript_b, len_b, colB, rb, guard))
                    continue;
                *found = 1;
                *p = (int)c;
                *cut_a = ttqA[ra];
                *cut_b = ttqB[rb];
                return PBCCS_OK;
            }
        }
        return PBCCS_OK;
    });
}

struct WinSlice {
    int cb, ce, ts, te;   // cb < 0: a placeholder
};
struct WinZmw {
    std::vector<std::pair<int, int>> wins;
    std::vector<WinSlice> sl;   // [window * n_reads + read]
    int unanchored = 0;
};

static int window_check_inputs(const pbccs_zmw_input* in, int n)
{
    for (int z = 0; z < n; ++z) {
        const pbccs_zmw_input& s = in[z];
        if (s.draft_len < 0 || (s.draft_len > 0 && !s.draft) ||
            (s.n_reads > 0 && (!s.seqs || !s.lens || !s.strands || !s.tstarts || !s.tends)))
            return fail(PBCCS_EINVAL, "bad pbccs_zmw_input");
    }
    return PBCCS_OK;
}

// Rules 1 and 2 for every ZMW: the plan, the chains (kept on the device) and the cuts (k_window_cuts).
static void window_slices_impl(pbccs_engine* eng, const pbccs_zmw_input* in, int n, const pbccs_window_options& w,
                               int minLength, std::vector<WinZmw>* out)
{
    out->assign((size_t)n, WinZmw());
    struct JobRef {
        int z, r;
    };
    std::vector<sparse::SparseInput> jobs;
    std::vector<JobRef> refs;
    for (int z = 0; z < n; ++z) {
        const pbccs_zmw_input& s = in[z];
        WinZmw& Z = (*out)[z];
        Z.wins = window_bounds(s.draft_len, w);
        const int nr = std::max(0, s.n_reads), nw = (int)Z.wins.size();
        Z.sl.assign((size_t)nw * nr, WinSlice{-1, -1, -1, -1});
        for (int r = 0; r < nr; ++r) {
            if (!s.seqs[r]) continue;
            const bool mapped = s.tstarts[r] >= 0 && s.tends[r] <= s.draft_len && s.tstarts[r] < s.tends[r] && s.lens[r] > 0;
            if (nw == 1 || !mapped) {   // as it is; a read the driver would refuse stays refused in window 0
                Z.sl[r] = WinSlice{0, std::max(0, s.lens[r]), s.tstarts[r], s.tends[r]};
                continue;
            }
            jobs.push_back(sparse::SparseInput{s.draft + s.tstarts[r], s.tends[r] - s.tstarts[r], s.seqs[r], s.lens[r],
                                               s.strands[r] ? 1 : 0, nullptr, 0, nullptr});
            refs.push_back(JobRef{z, r});
        }
    }
    if (jobs.empty()) return;
    std::lock_guard<std::mutex> lk(eng->sparseMu);   // the chains stay the runner's until the cuts are taken
    std::vector<sparse::KeptChain> kept;
    eng->Sparse().RunKeep(w.k, jobs.data(), (int)jobs.size(), &kept);
    struct Pending {
        int z, w, r, iLo, iHi, lo, hi;   // iLo / iHi: a cut task, -1 the read's start, -2 its end
    };
    std::vector<window::CutTask> tasks;
    std::vector<Pending> pend;
    for (size_t g = 0; g < jobs.size(); ++g) {
        const int z = refs[g].z, r = refs[g].r;
        WinZmw& Z = (*out)[z];
        if (kept[g].status != PBCCS_OK || kept[g].nAnchors <= 0) {
            Z.unanchored++;
            continue;
        }
        const int ts = in[z].tstarts[r], te = in[z].tends[r], flen = in[z].lens[r];
        auto boundary = [&](int b) {
            if (b == ts) return -1;
            if (b == te) return -2;
            tasks.push_back(window::CutTask{kept[g].anchorOff, kept[g].nAnchors, b - ts, flen});
            return (int)tasks.size() - 1;
        };
        for (int x = 0; x < (int)Z.wins.size(); ++x) {
            const int lo = std::max(ts, Z.wins[x].first), hi = std::min(te, Z.wins[x].second);
            if (hi - lo < minLength || hi <= lo) continue;
            const int iLo = boundary(lo), iHi = boundary(hi);
            pend.push_back(Pending{z, x, r, iLo, iHi, lo, hi});
        }
    }
    std::vector<int> cuts;
    {
        std::lock_guard<std::mutex> wl(eng->windowMu);
        eng->Window().Cuts(eng->Sparse().AnchorsDevice(), tasks, &cuts);
        eng->windowStats.cut_tasks += (long long)tasks.size();
        eng->windowStats.launches += tasks.empty() ? 0 : 1;
    }
    for (const Pending& p : pend) {
        const int flen = in[p.z].lens[p.r];
        const int cb = p.iLo == -1 ? 0 : (p.iLo == -2 ? flen : cuts[p.iLo]);
        const int ce = p.iHi == -1 ? 0 : (p.iHi == -2 ? flen : cuts[p.iHi]);
        if (ce - cb < minLength || ce <= cb) continue;
        WinZmw& Z = (*out)[p.z];
        Z.sl[(size_t)p.w * in[p.z].n_reads + p.r] = WinSlice{cb, ce, p.lo - Z.wins[p.w].first, p.hi - Z.wins[p.w].first};
    }
}

int pbccs_window_slices(pbccs_engine* eng, const pbccs_zmw_input* in, int n, const pbccs_window_options* w,
                        int min_length, int* n_windows, int* slices, long long cap, long long* n_ints,
                        int* unanchored)
{
    if (!window_options_ok(w)) return fail(PBCCS_EINVAL, "window options: need window > overlap >= 2 guard, guard >= 1, 4 <= k <= 8");
    if (!eng || n < 0 || (n > 0 && (!in || !n_windows)) || !n_ints || cap < 0 || (cap > 0 && !slices))
        return fail(PBCCS_EINVAL, "bad argument");
    if (window_check_inputs(in, n) != PBCCS_OK) return PBCCS_EINVAL;
    return guarded([&] {
        long long need = 0;
        for (int z = 0; z < n; ++z) {
            n_windows[z] = (int)window_bounds(in[z].draft_len, *w).size();
            need += 4LL * n_windows[z] * std::max(0, in[z].n_reads);
        }
        *n_ints = need;
        if (need > cap) return fail(PBCCS_ERANGE, "slices buffer too small");
        if (hipSetDevice(eng->device) != hipSuccess) return fail(PBCCS_EDEVICE, "hipSetDevice failed");
        std::vector<WinZmw> Z;
        window_slices_impl(eng, in, n, *w, min_length, &Z);
        long long at = 0;
        for (int z = 0; z < n; ++z) {
            for (const WinSlice& s : Z[z].sl) {
                slices[at++] = s.cb, slices[at++] = s.ce;
                slices[at++] = s.cb < 0 ? -1 : s.ts, slices[at++] = s.cb < 0 ? -1 : s.te;
            }
            if (unanchored) unanchored[z] = Z[z].unanchored;
        }
        return PBCCS_OK;
    });
}

// One window (or one single-window ZMW) of the first pbccs_polish_batch call: what its input and output point into.
struct WinBuf {
    std::vector<const char*> seqs;
    std::vector<int> lens, ts, te, arr, qvs;
    std::vector<double> zsc;
    std::vector<char> cons;
    std::vector<int> richQv;     // a rich call: the window's sub / ins / del QVs, cons.size() entries each
    std::vector<char> richTag;   // and its sub / ins tags
};

static int polish_windowed_impl(pbccs_engine* eng, const pbccs_zmw_input* in, int n, const pbccs_polish_options& o,
                                const pbccs_window_options& w, pbccs_zmw_output* out, pbccs_window_info* info,
                                pbccs_rich_qvs* rich = nullptr)
{
    using Clock = std::chrono::steady_clock;
    auto ms = [](Clock::time_point a, Clock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
    if (hipSetDevice(eng->device) != hipSuccess) return fail(PBCCS_EDEVICE, "hipSetDevice failed");
    const double nan = std::numeric_limits<double>::quiet_NaN();
    const auto t0 = Clock::now();
    std::vector<WinZmw> Z;
    window_slices_impl(eng, in, n, w, o.min_length, &Z);
    const auto t1 = Clock::now();

    // rule 3: every window of every multi-window ZMW, and every one-window ZMW as it is, in one call
    std::vector<int> first((size_t)n + 1, 0);
    for (int z = 0; z < n; ++z) first[z + 1] = first[z] + (int)Z[z].wins.size();
    const int np = first[n];
    std::vector<pbccs_zmw_input> pin((size_t)np);
    std::vector<pbccs_zmw_output> pout((size_t)np);
    std::vector<WinBuf> buf((size_t)np);
    std::vector<pbccs_rich_qvs> prich(rich ? (size_t)np : 0);   // the windows' rich QVs
    long long multi = 0, windows = 0, unanchored = 0;
    for (int z = 0; z < n; ++z) {
        const int nw = (int)Z[z].wins.size(), nr = std::max(0, in[z].n_reads);
        if (nw == 1) {
            pin[first[z]] = in[z];
            pout[first[z]] = out[z];
            if (rich) prich[first[z]] = rich[z];
            continue;
        }
        ++multi;
        windows += nw;
        unanchored += Z[z].unanchored;
        for (int x = 0; x < nw; ++x) {
            WinBuf& B = buf[first[z] + x];
            const int s = Z[z].wins[x].first, e = Z[z].wins[x].second;
            B.seqs.assign((size_t)nr, nullptr);
            B.lens.assign((size_t)nr, 0);
            B.ts.assign((size_t)nr, 0);
            B.te.assign((size_t)nr, e - s);
            B.arr.assign((size_t)nr, -1);
            B.zsc.assign((size_t)nr, nan);
            B.cons.assign(2 * (size_t)(e - s) + 64, 0);
            B.qvs.assign(B.cons.size(), 0);
            for (int r = 0; r < nr; ++r) {
                const WinSlice& sl = Z[z].sl[(size_t)x * nr + r];
                if (sl.cb < 0) continue;
                // as sequenced: the reverse strand's slice is seq[|f| - end, |f| - begin)
                B.seqs[r] = in[z].seqs[r] + (in[z].strands[r] ? in[z].lens[r] - sl.ce : sl.cb);
                B.lens[r] = sl.ce - sl.cb;
                B.ts[r] = sl.ts;
                B.te[r] = sl.te;
            }
            pbccs_zmw_input& pi = pin[first[z] + x];
            pi = in[z];
            pi.draft = in[z].draft + s;
            pi.draft_len = e - s;
            pi.seqs = B.seqs.data();
            pi.lens = B.lens.data();
            pi.tstarts = B.ts.data();
            pi.tends = B.te.data();
            pbccs_zmw_output& po = pout[first[z] + x];
            std::memset(&po, 0, sizeof(po));
            po.consensus = B.cons.data();
            po.consensus_cap = (int)B.cons.size();
            po.qvs = B.qvs.data();
            po.add_read_results = B.arr.data();
            po.zscores = B.zsc.data();
            if (rich) {
                const size_t cap = B.cons.size();
                B.richQv.assign(3 * cap, 0);
                B.richTag.assign(2 * cap, 0);
                prich[first[z] + x] = pbccs_rich_qvs{B.richQv.data(), B.richQv.data() + cap, B.richQv.data() + 2 * cap,
                                                     B.richTag.data(), B.richTag.data() + cap, (int)cap, 0};
            }
        }
    }
    int rc = polish_batch_impl(eng, pin.data(), np, &o, nullptr, nullptr, nullptr, pout.data(),
                               rich ? prich.data() : nullptr);
    if (rc != PBCCS_OK) return rc;
    const auto t2 = Clock::now();

    // rule 4: the joins of the ZMWs whose windows all succeeded
    std::vector<char> whole((size_t)n, 0);   // the fallback reason per ZMW
    std::vector<align::PairView> pairs;
    std::vector<int> pairOf((size_t)np, -1);
    for (int z = 0; z < n; ++z) {
        const int nw = (int)Z[z].wins.size();
        if (nw == 1) continue;
        for (int x = 0; x < nw; ++x)
            if (pout[first[z] + x].status != PBCCS_ZMW_SUCCESS) whole[z] = PBCCS_WINDOW_FALLBACK_WINDOW;
        if (whole[z]) continue;
        for (int x = 0; x < nw; ++x) {
            pairOf[first[z] + x] = (int)pairs.size();
            pairs.push_back(align::PairView{pin[first[z] + x].draft, pin[first[z] + x].draft_len, pout[first[z] + x].consensus,
                                            pout[first[z] + x].consensus_len});
        }
    }
    struct JointRef {
        int z, x;
    };
    std::vector<JointRef> jref;
    std::vector<window::JoinOut> joins;
    if (!pairs.empty()) {
        const align::AlignScoring sc{align::kNw, 0, -1, -1, -1, 0.f, 0.f, 0.f, 0.f, 0.f};
        const char* hj = std::getenv("PBCCS_WINDOW_HOST_JOIN");   // tests: the host rule on downloaded transcripts
        const bool hostJoin = hj && hj[0] == '1';
        std::lock_guard<std::mutex> lk(eng->alignMu);   // the transcripts stay the runner's until the joins are taken
        std::vector<align::KeptTranscript> kept;
        std::vector<align::PairResult> full;
        if (hostJoin) {
            full.resize(pairs.size());
            eng->Align().Run(sc, pairs.data(), (int)pairs.size(), full.data());
        } else {
            eng->Align().RunKeep(sc, pairs.data(), (int)pairs.size(), &kept);
        }
        std::vector<window::JoinTask> tasks;
        std::vector<int> taskOf;
        for (int z = 0; z < n; ++z) {
            const int nw = (int)Z[z].wins.size();
            if (nw == 1 || whole[z]) continue;
            for (int x = 0; x + 1 < nw; ++x) {
                jref.push_back(JointRef{z, x});
                joins.push_back(window::JoinOut{-1, 0, 0});
                const int a = pairOf[first[z] + x], b = pairOf[first[z] + x + 1];
                const std::pair<int, int> wa = Z[z].wins[x], wb = Z[z].wins[x + 1];
                if (hostJoin) {
                    int found = 0, p = -1, ca = 0, cb = 0;
                    if (full[a].status == PBCCS_OK && full[b].status == PBCCS_OK && wa.first < wb.first &&
                        pbccs_window_join(full[a].transcript.data(), (int)full[a].transcript.size(), wa.first, wa.second,
                                          full[b].transcript.data(), (int)full[b].transcript.size(), wb.first, wb.second,
                                          w.guard, &found, &p, &ca, &cb) == PBCCS_OK &&
                        found)
                        joins.back() = window::JoinOut{p, ca, cb};
                    continue;
                }
                if (!kept[a].onDevice || !kept[b].onDevice || kept[a].status != PBCCS_OK || kept[b].status != PBCCS_OK)
                    continue;
                window::JoinTask t;
                t.offA = kept[a].off, t.offB = kept[b].off, t.workOff = 0;
                t.lenA = kept[a].len, t.lenB = kept[b].len;
                t.sA = wa.first, t.sB = wb.first;
                t.lo = wb.first + w.guard, t.hi = wa.second - w.guard, t.mid = (wb.first + wa.second) / 2;
                t.guard = w.guard;
                if (t.lo > t.hi) continue;
                taskOf.push_back((int)joins.size() - 1);
                tasks.push_back(t);
            }
        }
        if (!tasks.empty()) {
            std::vector<window::JoinOut> got;
            std::lock_guard<std::mutex> wl(eng->windowMu);
            eng->Window().Joins(eng->Align().TranscriptsDevice(), tasks, &got);
            for (size_t q = 0; q < tasks.size(); ++q) joins[taskOf[q]] = got[q];
            eng->windowStats.launches += 1;
        }
    }
    const auto t3 = Clock::now();

    // rules 5 and 6: stitch, or send the ZMW to the whole-template route
    std::vector<std::vector<pbccs_window_record>> recs((size_t)n);
    for (int z = 0; z < n; ++z) {
        const int nw = (int)Z[z].wins.size();
        recs[z].resize((size_t)nw);
        for (int x = 0; x < nw; ++x) {
            const pbccs_zmw_output& po = pout[first[z] + x];
            recs[z][x] = pbccs_window_record{Z[z].wins[x].first, Z[z].wins[x].second, -1, 0, 0, po.status, po.n_tested, po.n_applied};
        }
        if (nw == 1) {
            out[z] = pout[first[z]];
            if (rich) rich[z] = prich[first[z]];
            recs[z][0].cut_end = std::max(0, out[z].consensus_len);
        } else if (rich) {
            rich[z].len = 0;
        }
    }
    for (size_t q = 0; q < jref.size();) {
        const int z = jref[q].z, nw = (int)Z[z].wins.size();
        int begin = 0;
        for (int x = 0; x + 1 < nw; ++x, ++q) {
            if (whole[z]) continue;
            const window::JoinOut& j = joins[q];
            if (j.p < 0 || j.cutA < begin || j.cutA > pout[first[z] + x].consensus_len ||
                j.cutB > pout[first[z] + x + 1].consensus_len) {
                whole[z] = PBCCS_WINDOW_FALLBACK_NO_JOIN;
                continue;
            }
            recs[z][x].join = j.p;
            recs[z][x].cut_begin = begin;
            recs[z][x].cut_end = j.cutA;
            begin = j.cutB;
        }
        if (!whole[z]) {
            recs[z][nw - 1].cut_begin = begin;
            recs[z][nw - 1].cut_end = pout[first[z] + nw - 1].consensus_len;
        }
    }
    for (int z = 0; z < n; ++z) {
        const int nw = (int)Z[z].wins.size(), nr = std::max(0, in[z].n_reads);
        if (nw == 1 || whole[z]) continue;
        long long len = 0;
        double err = 0.0;
        for (int x = 0; x < nw; ++x) {
            const pbccs_window_record& R = recs[z][x];
            len += R.cut_end - R.cut_begin;
            for (int c = R.cut_begin; c < R.cut_end; ++c)
                err += std::pow(10.0, static_cast<double>(pout[first[z] + x].qvs[c]) / -10.0);
        }
        const double acc = len > 0 ? 1.0 - err / (double)len : 0.0;
        if (len <= 0 || acc < o.min_predicted_accuracy) {
            whole[z] = PBCCS_WINDOW_FALLBACK_ACCURACY;
            continue;
        }
        pbccs_zmw_output& q = out[z];
        q.predicted_accuracy = acc;
        q.n_tested = q.n_applied = 0;
        q.n_passes = 0;
        q.zg = nan;
        for (int c = 0; c < 5; ++c) q.status_counts[c] = 0;
        for (int x = 0; x < nw; ++x) {
            const pbccs_zmw_output& po = pout[first[z] + x];
            q.n_tested += po.n_tested;
            q.n_applied += po.n_applied;
            if (!(po.zg >= q.zg)) q.zg = po.zg;   // the minimum; a NaN zg stays
        }
        double zsum = 0.0;
        int zn = 0;
        for (int r = 0; r < nr; ++r) {
            int code = -1;
            double zmin = nan;
            for (int x = 0; x < nw; ++x) {
                const int c = buf[first[z] + x].arr[r];
                if (c >= 0 && (code < 0 || code == PBCCS_ADD_SUCCESS)) code = c;
                const double v = buf[first[z] + x].zsc[r];
                if (!std::isnan(v) && !(v >= zmin)) zmin = v;
            }
            if (q.add_read_results) q.add_read_results[r] = code;
            if (q.zscores) q.zscores[r] = zmin;
            if (code >= 0) q.status_counts[code] += 1;
            if (code == PBCCS_ADD_SUCCESS) {
                if (!in[z].full_pass || in[z].full_pass[r]) q.n_passes += 1;
                if (!std::isnan(zmin)) zsum += zmin, ++zn;
            }
        }
        q.za = zn ? zsum / zn : nan;
        if (len + 1 > q.consensus_cap || !q.consensus) {
            q.consensus_len = -(int)len;
            q.status = PBCCS_ZMW_OTHER;
            continue;
        }
        if (rich) {   // the same pieces of the windows' rich arrays
            pbccs_rich_qvs& rq = rich[z];
            if (rq.cap < len || !rq.sub_qv || !rq.ins_qv || !rq.del_qv || !rq.sub_tag || !rq.ins_tag) {
                rq.len = -(int)len;
                q.consensus_len = 0;
                q.status = PBCCS_ZMW_OTHER;
                continue;
            }
            long long ra = 0;
            for (int x = 0; x < nw; ++x) {
                const pbccs_window_record& R = recs[z][x];
                const pbccs_rich_qvs& pr = prich[first[z] + x];
                std::copy(pr.sub_qv + R.cut_begin, pr.sub_qv + R.cut_end, rq.sub_qv + ra);
                std::copy(pr.ins_qv + R.cut_begin, pr.ins_qv + R.cut_end, rq.ins_qv + ra);
                std::copy(pr.del_qv + R.cut_begin, pr.del_qv + R.cut_end, rq.del_qv + ra);
                std::copy(pr.sub_tag + R.cut_begin, pr.sub_tag + R.cut_end, rq.sub_tag + ra);
                std::copy(pr.ins_tag + R.cut_begin, pr.ins_tag + R.cut_end, rq.ins_tag + ra);
                ra += R.cut_end - R.cut_begin;
            }
            rq.len = (int)len;
        }
        long long at = 0;
        for (int x = 0; x < nw; ++x) {
            const pbccs_window_record& R = recs[z][x];
            const int m = R.cut_end - R.cut_begin;
            std::memcpy(q.consensus + at, pout[first[z] + x].consensus + R.cut_begin, (size_t)m);
            if (q.qvs) std::copy(pout[first[z] + x].qvs + R.cut_begin, pout[first[z] + x].qvs + R.cut_end, q.qvs + at);
            at += m;
        }
        q.consensus[at] = 0;
        q.consensus_len = (int)len;
        q.status = PBCCS_ZMW_SUCCESS;
    }

    // the fallbacks of the call, whole, in a second call
    std::vector<int> fz;
    for (int z = 0; z < n; ++z)
        if (whole[z]) fz.push_back(z);
    if (!fz.empty()) {
        std::vector<pbccs_zmw_input> fin;
        std::vector<pbccs_zmw_output> fout;
        std::vector<pbccs_rich_qvs> frich;
        for (int z : fz) fin.push_back(in[z]), fout.push_back(out[z]);
        for (int z : fz)
            if (rich) frich.push_back(rich[z]);
        rc = polish_batch_impl(eng, fin.data(), (int)fz.size(), &o, nullptr, nullptr, nullptr, fout.data(),
                               rich ? frich.data() : nullptr);
        if (rc != PBCCS_OK) return rc;
        for (size_t q = 0; q < fz.size(); ++q) out[fz[q]] = fout[q];
        for (size_t q = 0; rich && q < fz.size(); ++q) rich[fz[q]] = frich[q];
    }
    const auto t4 = Clock::now();
    if (info)
        for (int z = 0; z < n; ++z) {
            info[z].n_windows = (int)Z[z].wins.size();
            info[z].fallback = whole[z];
            info[z].unanchored_reads = Z[z].unanchored;
            if (info[z].windows)
                for (int x = 0; x < std::min(info[z].n_windows, info[z].windows_cap); ++x) info[z].windows[x] = recs[z][x];
        }
    {
        std::lock_guard<std::mutex> wl(eng->windowMu);
        pbccs_window_stats& S = eng->windowStats;
        S.zmws += multi;
        S.windows += windows;
        S.unanchored_reads += unanchored;
        S.joints += (long long)jref.size();
        for (int z : fz) S.fallbacks[(int)whole[z]] += 1;
        S.slices_ms += ms(t0, t1);
        S.polish_ms += ms(t1, t2);
        S.join_ms += ms(t2, t3);
        S.fallback_ms += ms(t3, t4);
    }
    return PBCCS_OK;
}

int pbccs_polish_windowed(pbccs_engine* eng, const pbccs_zmw_input* in, int n, const pbccs_polish_options* opts,
                          const pbccs_window_options* w, pbccs_zmw_output* out, pbccs_window_info* info)
{
    if (!window_options_ok(w)) return fail(PBCCS_EINVAL, "window options: need window > overlap >= 2 guard, guard >= 1, 4 <= k <= 8");
    if (!eng || n < 0 || (n > 0 && (!in || !out))) return fail(PBCCS_EINVAL, "bad argument");
    if (window_check_inputs(in, n) != PBCCS_OK) return PBCCS_EINVAL;
    pbccs_polish_options o;
    if (opts) o = *opts;
    else pbccs_polish_options_default(&o);
    return guarded([&] { return polish_windowed_impl(eng, in, n, o, *w, out, info); });
}

int pbccs_polish_windowed_ex(pbccs_engine* eng, const pbccs_zmw_input* in, int n, const pbccs_polish_options* opts,
                             const pbccs_window_options* w, const pbccs_polish_extras* extras, pbccs_zmw_output* out,
                             pbccs_window_info* info)
{
    if (!extras || !extras->rich) return pbccs_polish_windowed(eng, in, n, opts, w, out, info);
    if (!window_options_ok(w)) return fail(PBCCS_EINVAL, "window options: need window > overlap >= 2 guard, guard >= 1, 4 <= k <= 8");
    if (!eng || n < 0 || (n > 0 && (!in || !out))) return fail(PBCCS_EINVAL, "bad argument");
    if (window_check_inputs(in, n) != PBCCS_OK) return PBCCS_EINVAL;
    pbccs_polish_options o;
    if (opts) o = *opts;
    else pbccs_polish_options_default(&o);
    return guarded([&] { return polish_windowed_impl(eng, in, n, o, *w, out, info, extras->rich); });
}

int pbccs_window_stats_get(pbccs_engine* eng, pbccs_window_stats* out, int reset)
{
    if (!eng || !out) return fail(PBCCS_EINVAL, "bad argument");
    std::lock_guard<std::mutex> lk(eng->windowMu);
    *out = eng->windowStats;
    if (reset) eng->windowStats = pbccs_window_stats{};
    return PBCCS_OK;
}

// One POA chunk of the pipelined ccs batch: its live ZMWs and everything their polish inputs point into.
struct CcsChunk {
    std::vector<int> zs;   // caller indices of the chunk's ZMWs
    std::vector<std::string> css;
    std::vector<std::vector<driver::MappedRead>> mapped;
    std::vector<std::vector<const char*>> seqPtr;
    std::vector<std::vector<int>> lens, strands, ts, te;
    std::vector<std::vector<unsigned char>> full;
    std::vector<pbccs_zmw_input> pin;   // the ZMWs that reach the polish
    std::vector<int> pinZ;
    std::vector<pbccs_zmw_output> pout;
    std::vector<pbccs_rich_qvs> prich;   // a rich call: the caller's rich-QV structs of the ZMWs in pin
    // a strand call: the screen's sites of the ZMWs in pin, and the pointers polish_span takes
    std::vector<std::vector<StrandSiteH>> psites;
    std::vector<std::vector<StrandSiteH>*> psitePtr;
    // per-read polish outputs by position in the polish input (FilterReads order up to the maxPoaCov stop);
    // scattered back to the caller's subread order once the chunk's polish is final
    std::vector<std::vector<int>> arr;
    std::vector<std::vector<double>> zsc;
    bool draftRange = false;   // a draft longer than its caller buffer
    // per polish position: the caller's subread (-1: a placeholder of a read FilterReads dropped) and, for a
    // segment of a split read (pbccs_ccs_batch_split), its index in segs
    std::vector<std::vector<int>> posSub, posSeg;
    struct SplitSegment {
        int subread;
        map::SplitSeg seg;
        unsigned char full;
    };
    std::vector<std::vector<SplitSegment>> segs;
    std::vector<int> nSplit, nMissed;
};

// A read FilterReads dropped and its split mapping: accepted as a missed-adapter read when the chain is whole, has at
// least two segments on alternating strands, and at least two of them reach minLength read bases.  Those segments
// become polish reads cut from the read as given (its own coordinates: no Appendix A.15 quirk); interior segments
// are full passes, the first needs the read's ADAPTER_BEFORE, the last its ADAPTER_AFTER.
static bool split_read(const driver::Subread& read, int subread, const map::SplitMapResult& chain, size_t minLength,
                       std::vector<driver::MappedRead>* reads, std::vector<CcsChunk::SplitSegment>* segs)
{
    reads->clear();
    segs->clear();
    if (chain.truncated || chain.segs.size() < 2) return false;
    for (size_t k = 1; k < chain.segs.size(); ++k)
        if (chain.segs[k].rc == chain.segs[k - 1].rc) return false;
    for (size_t k = 0; k < chain.segs.size(); ++k) {
        const map::SplitSeg& sg = chain.segs[k];
        if ((size_t)(sg.re - sg.rb) < minLength) continue;
        driver::MappedRead mr;
        mr.seq = read.seq.substr(sg.rb, sg.re - sg.rb);
        mr.strand = sg.rc ? 1 : 0;
        mr.ts = sg.tb;
        mr.te = sg.te;
        reads->push_back(std::move(mr));
        const bool full = (k > 0 || (read.flags & driver::kAdapterBefore)) &&
                          (k + 1 < chain.segs.size() || (read.flags & driver::kAdapterAfter));
        segs->push_back(CcsChunk::SplitSegment{subread, sg, (unsigned char)(full ? 1 : 0)});
    }
    return reads->size() >= 2;
}

// The chunk's polish outputs: the caller's pbccs_zmw_output fields, but per-read arrays owned by the chunk.
static void bind_polish_outputs(CcsChunk* C, const pbccs_ccs_output* out)
{
    for (size_t q = 0; q < C->pinZ.size(); ++q) {
        C->pout[q] = out[C->pinZ[q]].polish;
        C->pout[q].add_read_results = C->arr[q].data();
        C->pout[q].zscores = C->zsc[q].data();
    }
}

// The POA draft of one chunk (Consensus.h:422-425, 352-390), then TooShort and ExtractMappedRead
// (Consensus.h:427-471) into the chunk's polish inputs.  mapPastCap: the reads the maxPoaCov stop never reached
// (key -2) are placed on the finished drafts and treated like POA reads: one MapRunner call per POA slice, on the
// slice's thread once its drafts are final, while the other slices' POA rounds go on.
static void ccs_draft_chunk(pbccs_engine* eng, const pbccs_ccs_input* in, const pbccs_polish_options& o,
                            long long max_poa_coverage, bool mapPastCap, bool bandedPoa,
                            const std::vector<std::vector<driver::Subread>>& sub,
                            const std::vector<std::vector<int>>& order, pbccs_ccs_output* out, CcsChunk* C,
                            const pbccs_split_options* split = nullptr)
{
    const size_t m = C->zs.size();
    std::vector<std::vector<const std::string*>> poaReads(m);
    for (size_t q = 0; q < m; ++q)
        for (int k : order[C->zs[q]]) poaReads[q].push_back(k >= 0 ? &sub[C->zs[q]][k].seq : nullptr);
    std::vector<std::vector<int>> keys, ext;
    std::vector<std::vector<char>> rc;
    // past the cap: mapRes[q] holds one result per read of ZMW q past the stop, in FilterReads order
    std::vector<std::vector<map::MapResult>> mapRes(m);
    const std::function<void(int, int)> mapSlice = [&](int q0, int q1) {
        std::vector<map::MapGroup> groups;
        std::vector<size_t> groupQ;
        std::vector<std::vector<const char*>> ptrs(q1 - q0);
        std::vector<std::vector<int>> lens(q1 - q0);
        for (int q = q0; q < q1; ++q) {
            std::vector<const char*>& pq = ptrs[q - q0];
            std::vector<int>& lq = lens[q - q0];
            const int z = C->zs[q];
            if ((int)C->css[q].size() < o.min_length || C->css[q].empty()) continue;
            for (size_t i = 0; i < keys[q].size(); ++i) {
                if (keys[q][i] != -2) continue;
                const int k = order[z][i];
                pq.push_back(k >= 0 ? sub[z][k].seq.data() : nullptr);
                lq.push_back(k >= 0 ? (int)sub[z][k].seq.size() : 0);
            }
            if (pq.empty()) continue;
            if ((int)C->css[q].size() > map::kMaxLen) throw std::invalid_argument("map_past_cap: draft longer than 65535");
            groups.push_back(map::MapGroup{C->css[q].data(), (int)C->css[q].size(), pq.data(), lq.data(), (int)pq.size()});
            groupQ.push_back((size_t)q);
        }
        if (groups.empty()) return;
        std::vector<map::MapResult> res;
        {
            std::lock_guard<std::mutex> lk(eng->mapMu);   // the slices take turns on the engine's mapper
            eng->Map().Run(groups.data(), (int)groups.size(), 0.f, &res);
        }
        size_t at = 0;
        for (size_t g = 0; g < groups.size(); ++g) {
            mapRes[groupQ[g]].assign(res.begin() + at, res.begin() + at + groups[g].n);
            at += (size_t)groups[g].n;
        }
        for (const map::MapResult& r : res)
            if (r.status != PBCCS_OK) throw DeviceOom("a read's boundary buffers exceed the map workspace");
    };
    poa::PoaBatch(eng->PoaRunners(), poaReads, max_poa_coverage, -1, &C->css, &keys, &rc, &ext,
                  mapPastCap ? &mapSlice : nullptr, bandedPoa);
    // split: the reads FilterReads dropped, ZMW by ZMW in input order, split-mapped onto the finished drafts in one
    // call; splitRes[q] holds one chain per dropped read of ZMW q (empty: nothing to place, or no draft to place on)
    std::vector<std::vector<int>> droppedOf(m);
    std::vector<std::vector<map::SplitMapResult>> splitRes(m);
    if (split) {
        std::vector<map::MapGroup> groups;
        std::vector<size_t> groupQ;
        std::vector<std::vector<const char*>> ptrs(m);
        std::vector<std::vector<int>> lens(m);
        for (size_t q = 0; q < m; ++q) {
            const int z = C->zs[q];
            const std::string& css = C->css[q];
            if ((int)css.size() < o.min_length || css.empty() || (int)css.size() > map::kMaxLen) continue;
            bool slot = false;   // a placeholder the polish input will hold
            for (size_t i = 0; i < keys[q].size() && (keys[q][i] != -2 || mapPastCap); ++i)
                slot = slot || order[z][i] < 0;
            if (!slot) continue;
            std::vector<char> kept(sub[z].size(), 0);
            for (int k : order[z])
                if (k >= 0) kept[k] = 1;
            for (size_t k = 0; k < sub[z].size(); ++k) {
                if (kept[k]) continue;
                const bool fits = !sub[z][k].seq.empty() && (int)sub[z][k].seq.size() <= map::kMaxLen;
                droppedOf[q].push_back((int)k);
                ptrs[q].push_back(fits ? sub[z][k].seq.data() : nullptr);   // too long for the mapper: stays dropped
                lens[q].push_back(fits ? (int)sub[z][k].seq.size() : 0);
            }
            groups.push_back(map::MapGroup{css.data(), (int)css.size(), ptrs[q].data(), lens[q].data(), (int)ptrs[q].size()});
            groupQ.push_back(q);
        }
        if (!groups.empty()) {
            std::vector<map::SplitMapResult> res;
            {
                std::lock_guard<std::mutex> lk(eng->mapMu);
                eng->SplitMap().Run(groups.data(), (int)groups.size(), split->jump_penalty, split->max_segments, &res);
            }
            size_t at = 0;
            for (size_t g = 0; g < groups.size(); ++g) {
                splitRes[groupQ[g]].assign(res.begin() + at, res.begin() + at + groups[g].n);
                at += (size_t)groups[g].n;
            }
            for (const map::SplitMapResult& r : res)
                if (r.status != PBCCS_OK) throw DeviceOom("a read's buffers exceed the split-map workspace");
        }
    }
    C->mapped.resize(m);
    C->posSub.resize(m);
    C->posSeg.resize(m);
    C->segs.resize(m);
    C->nSplit.assign(m, 0);
    C->nMissed.assign(m, 0);
    C->seqPtr.resize(m);
    C->lens.resize(m);
    C->strands.resize(m);
    C->ts.resize(m);
    C->te.resize(m);
    C->full.resize(m);
    for (size_t q = 0; q < m; ++q) {
        const int z = C->zs[q];
        const std::string& css = C->css[q];
        if (out[z].draft) {
            if (out[z].draft_cap >= (int)css.size()) memcpy(out[z].draft, css.data(), css.size());
            else C->draftRange = true;
        }
        out[z].draft_len = (int)css.size();
        if ((int)css.size() < o.min_length) {
            out[z].polish.status = PBCCS_ZMW_TOO_SHORT;
            continue;
        }
        std::vector<unsigned char> added;
        const std::vector<int>& kk = keys[q];
        size_t past = 0, nextDropped = 0;
        std::vector<driver::MappedRead> segReads;
        std::vector<CcsChunk::SplitSegment> segRecs;
        for (size_t i = 0; i < kk.size() && (kk[i] != -2 || mapPastCap); ++i) {
            driver::MappedRead mr;
            const int key = kk[i];
            bool ok;
            if (order[z][i] < 0 && nextDropped < splitRes[q].size()) {
                // the k-th placeholder stands for the k-th dropped read: replaced in place by its segments
                const size_t d = nextDropped++;
                const int k = droppedOf[q][d];
                if (split_read(sub[z][k], k, splitRes[q][d], (size_t)o.min_length, &segReads, &segRecs)) {
                    for (size_t g = 0; g < segReads.size(); ++g) {
                        C->mapped[q].push_back(segReads[g]);
                        added.push_back(1);
                        C->full[q].push_back(segRecs[g].full);
                        C->posSub[q].push_back(k);
                        C->posSeg[q].push_back((int)C->segs[q].size());
                        C->segs[q].push_back(segRecs[g]);
                    }
                    C->nSplit[q]++;
                    C->nMissed[q] += splitRes[q][d].count - 1;
                    if (key == -2) ++past;   // its mapRes entry (a read never mapped) is passed over
                    continue;
                }
            }
            C->posSub[q].push_back(order[z][i]);
            C->posSeg[q].push_back(-1);
            if (key == -2) {
                const map::MapResult& r = mapRes[q][past++];
                ok = r.mapped && driver::ExtractMappedRead(sub[z][order[z][i]], r.rc != 0, r.ext[0], r.ext[1], r.ext[2],
                                                           r.ext[3], (size_t)o.min_length, &mr);
            } else {
                ok = key >= 0 &&
                     driver::ExtractMappedRead(sub[z][order[z][i]], rc[q][key] != 0, ext[q][4 * key],
                                               ext[q][4 * key + 1], ext[q][4 * key + 2], ext[q][4 * key + 3],
                                               (size_t)o.min_length, &mr);
            }
            C->mapped[q].push_back(ok ? mr : driver::MappedRead());
            added.push_back(ok ? 1 : 0);
            C->full[q].push_back(ok && sub[z][order[z][i]].FullPass() ? 1 : 0);
        }
        for (size_t i = 0; i < C->mapped[q].size(); ++i) {
            const driver::MappedRead& mr = C->mapped[q][i];
            C->seqPtr[q].push_back(added[i] ? mr.seq.data() : nullptr);
            C->lens[q].push_back((int)mr.seq.size());
            C->strands[q].push_back(mr.strand);
            C->ts[q].push_back(mr.ts);
            C->te[q].push_back(mr.te);
        }
        pbccs_zmw_input zi;
        zi.draft = css.data();
        zi.draft_len = (int)css.size();
        for (int b = 0; b < 4; ++b) zi.snr[b] = in[z].snr[b];
        zi.n_reads = (int)C->mapped[q].size();
        zi.seqs = C->seqPtr[q].data();
        zi.lens = C->lens[q].data();
        zi.strands = C->strands[q].data();
        zi.tstarts = C->ts[q].data();
        zi.tends = C->te[q].data();
        zi.full_pass = C->full[q].data();
        C->pin.push_back(zi);
        C->pinZ.push_back(z);
        C->pout.push_back(out[z].polish);
        C->arr.emplace_back(std::max<size_t>(1, C->mapped[q].size()), -1);
        C->zsc.emplace_back(std::max<size_t>(1, C->mapped[q].size()), std::numeric_limits<double>::quiet_NaN());
    }
    bind_polish_outputs(C, out);
}

static int ccs_batch_impl(pbccs_engine* eng, const pbccs_ccs_input* in, int n, long long max_poa_coverage,
                          bool mapPastCap, bool bandedPoa, const pbccs_polish_options* opts, pbccs_ccs_output* out,
                          const pbccs_window_options* win = nullptr, pbccs_window_info* info = nullptr,
                          pbccs_rich_qvs* rich = nullptr, const pbccs_strand_options* strand = nullptr,
                          pbccs_strand_result* sres = nullptr, const pbccs_split_options* split = nullptr,
                          pbccs_ccs_split_output* splitOut = nullptr)
{
    if (!eng || n < 0 || (n > 0 && (!in || !out)) || max_poa_coverage < 1) return fail(PBCCS_EINVAL, "bad argument");
    if (split && (win || strand || (n > 0 && !splitOut)))
        return fail(PBCCS_EINVAL, "split reads take no windows and no strand screen, and need their outputs");
    for (int z = 0; split && z < n; ++z) {
        splitOut[z].n_reads = splitOut[z].n_segments = splitOut[z].n_missed_adapters = splitOut[z].n_added = 0;
        if (splitOut[z].cap < 0) return fail(PBCCS_EINVAL, "bad pbccs_ccs_split_output");
    }
    if (strand && (win || !sres || !strand_options_ok(*strand)))
        return fail(PBCCS_EINVAL, "the strand screen takes no windows, needs its outputs and valid options");
    for (int z = 0; rich && z < n; ++z) rich[z].len = 0;   // ZMWs that never reach the polish
    for (int z = 0; strand && z < n; ++z) sres[z].n_sites = sres[z].split = 0;
    StrandOptions strandEng;
    if (strand) strandEng = strand_engine_options(*strand);
    // the screen of the chunk's polish inputs [lo, lo + ...)
    auto chunk_screen = [&](CcsChunk& C, int lo) {
        StrandScreen sc;
        sc.opt = strandEng;
        sc.sites = strand ? C.psitePtr.data() + lo : nullptr;
        return sc;
    };
    if (win && !window_options_ok(win))
        return fail(PBCCS_EINVAL, "window options: need window > overlap >= 2 guard, guard >= 1, 4 <= k <= 8");
    if (win && info)
        for (int z = 0; z < n; ++z) info[z].n_windows = info[z].fallback = info[z].unanchored_reads = 0;
    pbccs_polish_options o;
    if (opts) o = *opts;
    else pbccs_polish_options_default(&o);
    return guarded([&] {
        // FilterReads per ZMW (Consensus.h:411-420)
        std::vector<std::vector<driver::Subread>> sub(n);
        std::vector<std::vector<int>> order(n);
        std::vector<int> live;
        for (int z = 0; z < n; ++z) {
            if (in[z].n_subreads < 0 || (in[z].n_subreads > 0 && (!in[z].seqs || !in[z].lens)))
                return fail(PBCCS_EINVAL, "bad pbccs_ccs_input");
            for (int r = 0; r < in[z].n_subreads; ++r)
                if (in[z].lens[r] < 0 || (in[z].lens[r] > 0 && !in[z].seqs[r]))
                    return fail(PBCCS_EINVAL, "bad subread (NULL sequence or negative length)");
                else if (mapPastCap && in[z].lens[r] > map::kMaxLen)
                    return fail(PBCCS_EINVAL, "map_past_cap: subread longer than 65535");
        }
        for (int z = 0; z < n; ++z) {   // every per-read slot starts as "not added"
            for (int r = 0; r < in[z].n_subreads; ++r) {
                if (out[z].add_order) out[z].add_order[r] = -1;
                if (out[z].polish.add_read_results) out[z].polish.add_read_results[r] = -1;
                if (out[z].polish.zscores) out[z].polish.zscores[r] = std::numeric_limits<double>::quiet_NaN();
            }
        }
        for (int z = 0; z < n; ++z) {
            for (int r = 0; r < in[z].n_subreads; ++r) {
                driver::Subread s;
                if (in[z].lens[r] > 0) s.seq.assign(in[z].seqs[r], in[z].lens[r]);
                if (in[z].flags) s.flags = in[z].flags[r];
                sub[z].push_back(std::move(s));
            }
            order[z] = driver::FilterReads(sub[z], (size_t)o.min_length);
            bool any = false;
            for (int k : order[z]) any = any || k >= 0;
            if (any) live.push_back(z);
            else {
                out[z].polish.status = PBCCS_ZMW_NO_SUBREADS;
                out[z].draft_len = 0;
            }
        }
        if (live.empty()) return PBCCS_OK;
        std::lock_guard<std::mutex> poaLock(eng->poaMu);
        // Chunks: one POA batch each, polished as one device batch on a workspace slot while the next chunk's
        // POA runs.  They are planned like pbccs_polish_batch's batches, from each ZMW's filtered subreads
        // (the median length standing in for the draft): length buckets and the per-slot share of the HBM
        // left beside the POA's score pools.  No whole-wave split: the chunks reach the slots one POA apart,
        // and larger chunks keep both stages busier (2000-ZMW chunks measured 1544 ZMWs/s end to end against
        // 1384 for 1000 and 1066 for 500).
        const int slots = std::max(1, eng->concurrency);
        // 40 GB over the slices (kPoaSlicesDefault = 3: 13.3 GB each).  One read round of a 2 kb slice costs
        // ~17.7 MB per ZMW (17.7 GB for 1000 ZMWs), so a 2000-ZMW chunk's ~667-ZMW slices need ~11.8 GB
        const size_t kPoaPoolPerSlice = (40ull << 30) / (size_t)pbccs_engine::PoaSlices();
        for (poa::PoaRunner* r : eng->PoaRunners()) r->SetPoolBudget(kPoaPoolPerSlice);
        std::vector<std::vector<int>> liveLens(live.size());
        std::vector<pbccs_zmw_input> est(live.size());
        for (size_t q = 0; q < live.size(); ++q) {
            const int z = live[q];
            std::vector<int> kept;
            for (int k : order[z])
                if (k >= 0) liveLens[q].push_back(in[z].lens[k]);
            kept = liveLens[q];
            std::sort(kept.begin(), kept.end());
            std::memset(&est[q], 0, sizeof(est[q]));
            est[q].draft_len = kept[kept.size() / 2];
            est[q].n_reads = (int)liveLens[q].size();
            est[q].lens = liveLens[q].data();
        }
        size_t freeB = 0, totalB = 0;
        if (hipSetDevice(eng->device) != hipSuccess || hipMemGetInfo(&freeB, &totalB) != hipSuccess)
            return fail(PBCCS_EDEVICE, "hipMemGetInfo failed");
        size_t poaMapped = 0;
        for (poa::PoaRunner* r : eng->PoaRunners()) poaMapped += r->PoolMappedBytes();
        const double spare = std::max(0.0, (double)freeB + (double)poaMapped + (double)slot_pool_bytes(eng) - kQueueMargin -
                                               (double)(kPoaPoolPerSlice * eng->PoaRunners().size()));
        const double budget = std::max(1.0 * (1 << 30), 0.9 * spare / slots);
        const int nl = (int)live.size();
        std::vector<int> perm(nl), start(nl + 1);
        int nb = 0;
        int rcp = PBCCS_OK;
        if (o.zmws_per_batch > 0) {   // caller-sized consecutive chunks
            for (int i = 0; i < nl; ++i) perm[i] = i;
            for (int b0 = 0; b0 < nl; b0 += o.zmws_per_batch) start[nb++] = b0;
            start[nb] = nl;
        } else {
            // about ten chunks per call, 1000-2000 ZMWs each: the POA of chunk k + 1 runs beside the polish of chunk
            // k, so the first draft and the last polish are the pipeline's fill and drain -- at 10,000 ZMWs 1000-ZMW
            // chunks ran 1943 / 1917 ZMWs/s against 1717 / 1850 for 2000, at 20,000 2000-ZMW chunks won (1986 / 1987
            // vs 1874 / 1852; profiles/r9zt_ccs_chunk_ab.txt)
            const int cap = std::max(std::min(nl / 10, kQueueMaxZmws), std::min(1000, kQueueMaxZmws));
            rcp = pbccs_plan_batches(est.data(), nl, budget, cap, 1.5, perm.data(), start.data(), nullptr, &nb);
        }
        if (rcp != PBCCS_OK) return rcp;
        std::vector<CcsChunk> chunks(nb);
        for (int c = 0; c < nb; ++c)
            for (int k = start[c]; k < start[c + 1]; ++k) chunks[c].zs.push_back(live[perm[k]]);
        // consumers: the polish slots pull drafted chunks as the producer (this thread) finishes them
        for (int s = 0; s < slots; ++s) eng->Slot(s);
        std::mutex qmu;
        std::condition_variable qcv;
        // work items (chunk, first, end) over each chunk's polish inputs: a chunk is one item, except the last
        // one, whose polish is the run's tail with the other slots idle: it is cut into one piece per slot (a
        // polish batch's time is its refine rounds' latency, ~1.1 s for a few hundred ZMWs against ~1.8 s for
        // 2000, so parallel pieces shorten the tail; earlier chunks stay whole, their pieces would only queue)
        std::vector<std::array<int, 3>> work;
        int drafted = 0, next = 0;
        bool stop = false;
        std::vector<int> prc(nb, PBCCS_OK);
        std::vector<std::string> perr(nb);
        // PBCCS_CCS_TRACE=1: one stderr line per chunk stage (ms since the call began)
        static const bool trace = std::getenv("PBCCS_CCS_TRACE") != nullptr;
        const auto tBegin = std::chrono::steady_clock::now();
        auto since = [&] {
            return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tBegin).count();
        };
        auto worker = [&](int slot) {
            for (;;) {
                std::array<int, 3> w;
                {
                    std::unique_lock<std::mutex> lk(qmu);
                    qcv.wait(lk, [&] { return stop || next < drafted; });
                    if (next >= drafted) return;   // stopped with nothing left
                    w = work[next++];
                }
                const int c = w[0], lo = w[1], hi = w[2];
                CcsChunk& C = chunks[c];
                if (hi <= lo) continue;
                const double p0 = since();
                const StrandScreen sc = chunk_screen(C, lo);
                const int rc = polish_span(eng, slot, C.pin.data() + lo, hi - lo, &o, C.pout.data() + lo, nullptr, nullptr,
                                           nullptr, rich ? C.prich.data() + lo : nullptr, strand ? &sc : nullptr);
                if (trace)
                    std::fprintf(stderr, "[ccs] chunk %d polish slot %d zmws %d %.1f-%.1f ms\n", c, slot, hi - lo, p0,
                                 since());
                if (rc != PBCCS_OK) {
                    std::lock_guard<std::mutex> lk(qmu);
                    if (prc[c] == PBCCS_OK || rc != PBCCS_EOOM) prc[c] = rc;   // EOOM: the chunk reruns whole below
                    if (rc != PBCCS_EOOM) {
                        perr[c] = g_lastError;
                        stop = true;
                        qcv.notify_all();
                        return;
                    }
                }
            }
        };
        // PBCCS_CCS_SERIAL=1: every chunk drafted before the first polishes (the A/B reference schedule)
        const char* serialEnv = std::getenv("PBCCS_CCS_SERIAL");
        // windows: the windowed polish runs pbccs_polish_batch on every slot itself, so the chunks polish one after
        // another once all are drafted
        const bool serial = win || (serialEnv && serialEnv[0] == '1');
        std::vector<std::thread> pool;
        if (!serial)
            for (int s = 0; s < std::min(slots, nb); ++s) pool.emplace_back(worker, s);
        int rcDraft = PBCCS_OK;
        std::string errDraft;
        for (int c = 0; c < nb; ++c) {
            {
                std::lock_guard<std::mutex> lk(qmu);
                if (stop) break;
            }
            const double d0 = since();
            try {
                ccs_draft_chunk(eng, in, o, max_poa_coverage, mapPastCap, bandedPoa, sub, order, out, &chunks[c], split);
                if (rich)
                    for (int z : chunks[c].pinZ) chunks[c].prich.push_back(rich[z]);
                if (strand) {
                    chunks[c].psites.assign(chunks[c].pinZ.size(), {});
                    for (std::vector<StrandSiteH>& v : chunks[c].psites) chunks[c].psitePtr.push_back(&v);
                }
                if (trace)
                    std::fprintf(stderr, "[ccs] chunk %d draft zmws %zu %.1f-%.1f ms\n", c, chunks[c].zs.size(), d0,
                                 since());
            } catch (const std::bad_alloc&) {
                rcDraft = PBCCS_EOOM;
                errDraft = "out of memory in the POA draft";
            } catch (const std::exception& e) {
                rcDraft = PBCCS_EDEVICE;
                errDraft = e.what();
            }
            std::lock_guard<std::mutex> lk(qmu);
            if (rcDraft != PBCCS_OK) {
                stop = true;
            } else {
                const int m = (int)chunks[c].pin.size();
                const char* pe = std::getenv("PBCCS_CCS_TAIL_PIECE");   // test hook: smaller pieces
                const int piece = pe ? std::max(1, std::atoi(pe)) : kCcsTailPiece;
                const int pieces = c + 1 < nb ? 1 : std::max(1, std::min(slots, m / piece));
                for (int k = 0; k < pieces; ++k)
                    work.push_back({c, (int)((long long)m * k / pieces), (int)((long long)m * (k + 1) / pieces)});
                drafted = (int)work.size();
            }
            qcv.notify_all();
            if (rcDraft != PBCCS_OK) break;
        }
        {
            std::lock_guard<std::mutex> lk(qmu);
            stop = true;   // every drafted chunk is still taken: workers leave once next == drafted
            qcv.notify_all();
        }
        if (serial) {
            for (poa::PoaRunner* r : eng->PoaRunners()) r->ReleasePool();
            if (!win)
                for (int s = 0; s < std::min(slots, nb); ++s) pool.emplace_back(worker, s);
        }
        if (win && rcDraft == PBCCS_OK) {
            for (int c = 0; c < nb && rcDraft == PBCCS_OK; ++c) {
                CcsChunk& C = chunks[c];
                const int m = (int)C.pin.size();
                if (m == 0) continue;
                std::vector<pbccs_window_info> cinfo;
                if (info)
                    for (int q = 0; q < m; ++q) cinfo.push_back(info[C.pinZ[q]]);
                rcDraft = polish_windowed_impl(eng, C.pin.data(), m, o, *win, C.pout.data(), info ? cinfo.data() : nullptr,
                                               rich ? C.prich.data() : nullptr);
                if (rcDraft != PBCCS_OK) errDraft = g_lastError;
                else if (info)
                    for (int q = 0; q < m; ++q) info[C.pinZ[q]] = cinfo[q];
            }
        }
        for (std::thread& t : pool) t.join();
        for (int s = 0; s < slots; ++s) eng->Slot(s)->TrimRetired();   // every chunk's batch is destroyed
        for (poa::PoaRunner* r : eng->PoaRunners()) {
            r->ReleasePool();
            r->SetPoolBudget(0);
        }
        if (rcDraft != PBCCS_OK) return fail(rcDraft, errDraft.c_str());
        for (int c = 0; c < nb; ++c)
            if (prc[c] != PBCCS_OK && prc[c] != PBCCS_EOOM) return fail(prc[c], perr[c].c_str());
        // chunks that ran the device out of memory beside the others: rerun alone once every pool is unmapped
        bool unmapped = false;
        for (int c = 0; c < nb; ++c) {
            if (prc[c] != PBCCS_EOOM) continue;
            if (!unmapped) {
                for (int s = 0; s < slots; ++s) eng->Slot(s)->val.unmap_all();
                unmapped = true;
            }
            CcsChunk& C = chunks[c];
            bind_polish_outputs(&C, out);
            const StrandScreen sc = chunk_screen(C, 0);
            const int r = polish_retry(eng, 0, C.pin.data(), (int)C.pin.size(), &o, C.pout.data(), nullptr, nullptr,
                                       nullptr, rich ? C.prich.data() : nullptr, strand ? &sc : nullptr);
            if (r != PBCCS_OK) return r;
        }
        bool draftRange = false, splitRange = false;
        for (const CcsChunk& C : chunks) {
            draftRange = draftRange || C.draftRange;
            for (size_t q = 0; q < C.pinZ.size(); ++q) {
                const int z = C.pinZ[q];
                pbccs_zmw_output& po = out[z].polish;
                if (rich) rich[z] = C.prich[q];
                int* const arrOut = po.add_read_results;
                double* const zsOut = po.zscores;
                po = C.pout[q];
                po.add_read_results = arrOut;
                po.zscores = zsOut;
                // polish position i is FilterReads' i-th read, i.e. caller subread order[z][i]; the scorer's reads
                // (AddRead calls) are the positions with a result, in position order
                int added = 0;
                pbccs_ccs_split_output* so = split ? &splitOut[z] : nullptr;
                if (so) {
                    so->n_reads = C.nSplit[q];
                    so->n_missed_adapters = C.nMissed[q];
                    so->n_segments = (int)C.segs[q].size();
                    if (so->n_segments > so->cap) splitRange = true;
                }
                for (size_t i = 0; i < C.mapped[q].size(); ++i) {
                    const int k = C.posSub[q][i];
                    if (k < 0) continue;
                    const int g = C.posSeg[q][i];
                    if (g >= 0) {   // a segment of a split read: the subread's own entries stay -1 / NaN
                        if (g >= so->cap) continue;
                        const CcsChunk::SplitSegment& sg = C.segs[q][g];
                        const int v[6] = {sg.seg.rc, sg.seg.rb, sg.seg.re, sg.seg.tb, sg.seg.te, sg.seg.score};
                        if (so->subread) so->subread[g] = sg.subread;
                        if (so->segments) std::copy(v, v + 6, so->segments + 6 * (size_t)g);
                        if (so->full_pass) so->full_pass[g] = sg.full;
                        if (so->add_read_results) so->add_read_results[g] = C.arr[q][i];
                        if (so->zscores) so->zscores[g] = C.zsc[q][i];
                    } else {
                        if (arrOut) arrOut[k] = C.arr[q][i];
                        if (zsOut) zsOut[k] = C.zsc[q][i];
                    }
                    if (C.arr[q][i] < 0) continue;
                    // with split reads there can be more AddRead calls than subreads: the whole order goes to the
                    // split output, the caller's add_order holds as much of it as it has room for
                    if (so && so->add_order && added < in[z].n_subreads + so->cap) so->add_order[added] = k;
                    if (out[z].add_order && added < in[z].n_subreads) out[z].add_order[added] = k;
                    ++added;
                }
                if (so) so->n_added = added;
            }
        }
        // the strand screen's second half over the polish inputs of every chunk: sites, split
        // decision, the per-strand polish; per-read entries go from polish positions back to the caller's subreads
        int strandRc = PBCCS_OK;
        if (strand) {
            std::vector<pbccs_zmw_input> pin;
            std::vector<pbccs_zmw_output> pout;
            std::vector<std::vector<StrandSiteH>> sites;
            std::vector<pbccs_strand_result> pres;
            std::vector<int> pz;
            for (CcsChunk& C : chunks)
                for (size_t q = 0; q < C.pinZ.size(); ++q) {
                    pin.push_back(C.pin[q]);
                    pout.push_back(out[C.pinZ[q]].polish);
                    sites.push_back(std::move(C.psites[q]));
                    pres.push_back(sres[C.pinZ[q]]);
                    pz.push_back(C.pinZ[q]);
                }
            const size_t np = pin.size();
            std::vector<std::vector<int>> arrF(np), arrR(np);
            std::vector<std::vector<double>> zsF(np), zsR(np);
            for (size_t q = 0; q < np; ++q) {
                const size_t m = (size_t)std::max(1, pin[q].n_reads);
                arrF[q].assign(m, -1);
                arrR[q].assign(m, -1);
                zsF[q].assign(m, std::numeric_limits<double>::quiet_NaN());
                zsR[q].assign(m, std::numeric_limits<double>::quiet_NaN());
                pres[q].fwd.add_read_results = arrF[q].data();
                pres[q].rev.add_read_results = arrR[q].data();
                pres[q].fwd.zscores = zsF[q].data();
                pres[q].rev.zscores = zsR[q].data();
            }
            strandRc = strand_finish(eng, pin.data(), (int)np, &o, nullptr, *strand, sites, pout.data(), pres.data());
            if (strandRc != PBCCS_OK && strandRc != PBCCS_ERANGE) return strandRc;
            for (size_t q = 0; q < np; ++q) {
                const int z = pz[q];
                pbccs_strand_result& dst = sres[z];
                dst.n_sites = pres[q].n_sites;
                dst.split = pres[q].split;
                if (!dst.split) continue;
                for (int side = 0; side < 2; ++side) {
                    pbccs_zmw_output& d = side ? dst.rev : dst.fwd;
                    int* const arr = d.add_read_results;
                    double* const zs = d.zscores;
                    d = side ? pres[q].rev : pres[q].fwd;
                    d.add_read_results = arr;
                    d.zscores = zs;
                    for (int r = 0; r < in[z].n_subreads; ++r) {
                        if (arr) arr[r] = -1;
                        if (zs) zs[r] = std::numeric_limits<double>::quiet_NaN();
                    }
                    const std::vector<int>& a = side ? arrR[q] : arrF[q];
                    const std::vector<double>& v = side ? zsR[q] : zsF[q];
                    for (int i = 0; i < pin[q].n_reads; ++i) {
                        const int k = order[z][i];
                        if (k < 0) continue;
                        if (arr) arr[k] = a[i];
                        if (zs) zs[k] = v[i];
                    }
                }
            }
        }
        if (draftRange) return fail(PBCCS_ERANGE, "draft buffer too small");
        if (splitRange) return fail(PBCCS_ERANGE, "split segment buffers too small");
        return strandRc == PBCCS_ERANGE ? fail(PBCCS_ERANGE, "strand site buffers too small") : PBCCS_OK;
    });
}

int pbccs_ccs_batch(pbccs_engine* eng, const pbccs_ccs_input* in, int n, long long max_poa_coverage,
                    const pbccs_polish_options* opts, pbccs_ccs_output* out)
{
    return ccs_batch_impl(eng, in, n, max_poa_coverage, false, false, opts, out);
}

void pbccs_ccs_options_default(pbccs_ccs_options* o)
{
    if (!o) return;
    o->max_poa_coverage = std::numeric_limits<long long>::max();
    o->map_past_cap = 0;
}

int pbccs_ccs_batch_ex(pbccs_engine* eng, const pbccs_ccs_input* in, int n, const pbccs_ccs_options* ccs,
                       const pbccs_polish_options* opts, pbccs_ccs_output* out)
{
    pbccs_ccs_options c;
    if (ccs) c = *ccs;
    else pbccs_ccs_options_default(&c);
    return ccs_batch_impl(eng, in, n, c.max_poa_coverage, c.map_past_cap != 0, false, opts, out);
}

int pbccs_ccs_batch_ex2(pbccs_engine* eng, const pbccs_ccs_input* in, int n, const pbccs_ccs_options* ccs,
                        const pbccs_poa_options* poa, const pbccs_polish_options* opts, pbccs_ccs_output* out)
{
    pbccs_ccs_options c;
    if (ccs) c = *ccs;
    else pbccs_ccs_options_default(&c);
    return ccs_batch_impl(eng, in, n, c.max_poa_coverage, c.map_past_cap != 0, poa && poa->banded != 0, opts, out);
}

int pbccs_ccs_batch_ex3(pbccs_engine* eng, const pbccs_ccs_input* in, int n, const pbccs_ccs_options* ccs,
                        const pbccs_poa_options* poa, const pbccs_window_options* win,
                        const pbccs_polish_options* opts, pbccs_ccs_output* out, pbccs_window_info* info)
{
    pbccs_ccs_options c;
    if (ccs) c = *ccs;
    else pbccs_ccs_options_default(&c);
    return ccs_batch_impl(eng, in, n, c.max_poa_coverage, c.map_past_cap != 0, poa && poa->banded != 0, opts, out, win,
                          info);
}

int pbccs_ccs_batch_ex4(pbccs_engine* eng, const pbccs_ccs_input* in, int n, const pbccs_ccs_options* ccs,
                        const pbccs_poa_options* poa, const pbccs_window_options* win,
                        const pbccs_polish_options* opts, const pbccs_polish_extras* extras, pbccs_ccs_output* out,
                        pbccs_window_info* info)
{
    pbccs_ccs_options c;
    if (ccs) c = *ccs;
    else pbccs_ccs_options_default(&c);
    return ccs_batch_impl(eng, in, n, c.max_poa_coverage, c.map_past_cap != 0, poa && poa->banded != 0, opts, out, win,
                          info, extras ? extras->rich : nullptr);
}

int pbccs_ccs_batch_strand(pbccs_engine* eng, const pbccs_ccs_input* in, int n, const pbccs_ccs_options* ccs,
                           const pbccs_poa_options* poa, const pbccs_polish_options* opts,
                           const pbccs_polish_extras* extras, const pbccs_strand_options* strand,
                           pbccs_strand_result* strand_out, pbccs_ccs_output* out)
{
    if (n > 0 && !strand_out) return fail(PBCCS_EINVAL, "bad argument");
    if (extras && extras->repeats) return fail(PBCCS_EINVAL, "the ccs calls take no repeat options");
    pbccs_ccs_options c;
    if (ccs) c = *ccs;
    else pbccs_ccs_options_default(&c);
    pbccs_strand_options so;
    pbccs_strand_options_default(&so);
    if (strand) so = *strand;
    return ccs_batch_impl(eng, in, n, c.max_poa_coverage, c.map_past_cap != 0, poa && poa->banded != 0, opts, out,
                          nullptr, nullptr, extras ? extras->rich : nullptr, &so, strand_out);
}

void pbccs_split_options_default(pbccs_split_options* o)
{
    if (!o) return;
    o->jump_penalty = PBCCS_SPLIT_JUMP_PENALTY;
    o->max_segments = PBCCS_SPLIT_MAX_SEGMENTS;
}

int pbccs_ccs_batch_split(pbccs_engine* eng, const pbccs_ccs_input* in, int n, const pbccs_ccs_options* ccs,
                          const pbccs_poa_options* poa, const pbccs_polish_options* opts,
                          const pbccs_polish_extras* extras, const pbccs_split_options* split,
                          pbccs_ccs_split_output* split_out, pbccs_ccs_output* out)
{
    if (n > 0 && !split_out) return fail(PBCCS_EINVAL, "bad argument");
    if (extras && extras->repeats) return fail(PBCCS_EINVAL, "the ccs calls take no repeat options");
    pbccs_ccs_options c;
    if (ccs) c = *ccs;
    else pbccs_ccs_options_default(&c);
    pbccs_split_options so;
    pbccs_split_options_default(&so);
    if (split) so = *split;
    if (so.jump_penalty < 0) so.jump_penalty = PBCCS_SPLIT_JUMP_PENALTY;
    if (so.max_segments <= 0) so.max_segments = PBCCS_SPLIT_MAX_SEGMENTS;
    if (so.max_segments > map::kSplitMaxSegments) return fail(PBCCS_EINVAL, "max_segments above 64");
    return ccs_batch_impl(eng, in, n, c.max_poa_coverage, c.map_past_cap != 0, poa && poa->banded != 0, opts, out,
                          nullptr, nullptr, extras ? extras->rich : nullptr, nullptr, nullptr, &so, split_out);
}

// ---- barcode demultiplexing (demux_kernels.hpp) -------------------------------------------------------------
void pbccs_demux_options_default(pbccs_demux_options* o)
{
    if (!o) return;
    *o = pbccs_demux_options{3, -5, -4, -4, PBCCS_DEMUX_ASYMMETRIC, 0, 3, PBCCS_DEMUX_MIN_QUALITY, 0};
}

namespace {
// The refusals of pbccs_demux_batch that need no read: PBCCS_OK, or the failure already recorded.  *o receives the
// resolved options (the window, the design, the thresholds).
int demux_check(const pbccs_demux_barcodes* bc, const pbccs_demux_options* opts, demux::DemuxOptions* o)
{
    if (!bc || !bc->seqs || !bc->lens) return fail(PBCCS_EINVAL, "bad pbccs_demux_barcodes");
    if (bc->n < 1 || bc->n > PBCCS_DEMUX_MAX_BARCODES) return fail(PBCCS_EINVAL, "1 to 65535 barcodes");
    int longest = 0;
    for (int b = 0; b < bc->n; ++b) {
        const int len = bc->lens[b];
        if (len < 1 || len > PBCCS_DEMUX_MAX_BARCODE_LEN || !bc->seqs[b])
            return fail(PBCCS_EINVAL, "a barcode has 1 to 64 bases");
        for (int k = 0; k < len; ++k) {
            const char c = bc->seqs[b][k];
            if (c != 'A' && c != 'C' && c != 'G' && c != 'T')
                return fail(PBCCS_EINVAL, "a barcode holds uppercase A, C, G and T only");
        }
        longest = std::max(longest, len);
    }
    pbccs_demux_options d;
    pbccs_demux_options_default(&d);
    if (opts) d = *opts;
    if (d.match <= 0 || d.insert > 0 || d.delete_ > 0)
        return fail(PBCCS_EINVAL, "demux needs Match > 0, Insert <= 0 and Delete <= 0");
    if (d.design != PBCCS_DEMUX_ASYMMETRIC && d.design != PBCCS_DEMUX_SYMMETRIC)
        return fail(PBCCS_EINVAL, "unknown demux design");
    const long long W = d.window > 0 ? d.window : (long long)(d.window_mult > 0 ? d.window_mult : 3) * longest;
    if (W < 1 || W > PBCCS_DEMUX_MAX_WINDOW) return fail(PBCCS_EINVAL, "the demux window is 1 to 1024 bases");
    const long long mx = std::max(std::max(std::llabs((long long)d.match), std::llabs((long long)d.mismatch)),
                                  std::max(std::llabs((long long)d.insert), std::llabs((long long)d.delete_)));
    if (2 * (longest + W) * mx > 0x7fffffffLL) return fail(PBCCS_EINVAL, "demux scores could leave int32");
    o->match = d.match;
    o->mismatch = d.mismatch;
    o->insert = d.insert;
    o->delete_ = d.delete_;
    o->symmetric = d.design == PBCCS_DEMUX_SYMMETRIC;
    o->window = (int)W;
    o->minQuality = d.min_quality < 0 ? PBCCS_DEMUX_MIN_QUALITY : d.min_quality;
    o->minScoreLead = d.min_score_lead;
    return PBCCS_OK;
}

// Runs the checked call and writes entry k of the device's answer to entry at[k] of the caller's arrays (at NULL:
// entry k).  scores only with at NULL.
void demux_run(pbccs_engine* eng, const pbccs_demux_barcodes* bc, const demux::DemuxOptions& o,
               const std::vector<const char*>& seqs, const std::vector<int>& lens, const int* at,
               pbccs_demux_output* out)
{
    const int n = (int)seqs.size();
    std::vector<demux::DemuxEnd> ends((size_t)2 * n);
    std::vector<demux::DemuxCall> calls((size_t)n);
    {
        std::lock_guard<std::mutex> lk(eng->demuxMu);
        eng->Demux().Run(bc->seqs, bc->lens, bc->n, o, seqs.data(), lens.data(), n, ends.data(), calls.data(),
                         at ? nullptr : out->scores);
    }
    for (int k = 0; k < n; ++k) {
        const size_t r = at ? (size_t)at[k] : (size_t)k;
        const demux::DemuxCall& c = calls[k];
        if (out->lead) out->lead[r] = c.lead;
        if (out->trail) out->trail[r] = c.trail;
        if (out->called) out->called[r] = c.called;
        if (out->score) out->score[r] = c.score;
        if (out->score_lead) out->score_lead[r] = c.scoreLead;
        if (out->quality) out->quality[r] = c.quality;
        if (out->extents) {
            const int v[4] = {c.leadBegin, c.leadEnd, c.trailBegin, c.trailEnd};
            std::copy(v, v + 4, out->extents + 4 * r);
        }
        const bool over = c.leadEnd > c.trailBegin;
        if (out->clip) {
            out->clip[2 * r] = over ? -1 : c.leadEnd;
            out->clip[2 * r + 1] = over ? -1 : c.trailBegin;
        }
        if (out->overlap) out->overlap[r] = over ? 1 : 0;
        if (out->best)
            for (int e = 0; e < 2; ++e) {
                const demux::DemuxEnd& x = ends[(size_t)2 * k + e];
                const int v[3] = {x.best, x.index, x.second};
                std::copy(v, v + 3, out->best + 6 * r + 3 * e);
            }
    }
}
}  // namespace

int pbccs_demux_batch(pbccs_engine* eng, const pbccs_demux_barcodes* barcodes, const pbccs_demux_options* opts,
                      const pbccs_demux_read* reads, int n, pbccs_demux_output* out)
{
    if (!eng || n < 0 || (n > 0 && (!reads || !out))) return fail(PBCCS_EINVAL, "bad argument");
    demux::DemuxOptions o;
    if (const int rc = demux_check(barcodes, opts, &o)) return rc;
    for (int r = 0; r < n; ++r)
        if (reads[r].len < 0 || (reads[r].len > 0 && !reads[r].seq))
            return fail(PBCCS_EINVAL, "bad read (NULL sequence or negative length)");
    if (n == 0) return PBCCS_OK;
    return guarded([&] {
        std::vector<const char*> seqs(n);
        std::vector<int> lens(n);
        for (int r = 0; r < n; ++r) {
            seqs[r] = reads[r].seq;
            lens[r] = reads[r].len;
        }
        demux_run(eng, barcodes, o, seqs, lens, nullptr, out);
        return PBCCS_OK;
    });
}

int pbccs_demux_stats_get(pbccs_engine* eng, pbccs_demux_stats* out, int reset)
{
    if (!eng || !out) return fail(PBCCS_EINVAL, "bad argument");
    return guarded([&] {
        std::lock_guard<std::mutex> lk(eng->demuxMu);
        const demux::DemuxStats s = eng->demuxRunner ? eng->demuxRunner->stats : demux::DemuxStats();
        *out = pbccs_demux_stats{s.reads, s.cells, s.launches, s.deviceMs};
        if (reset && eng->demuxRunner) eng->demuxRunner->stats = demux::DemuxStats();
        return PBCCS_OK;
    });
}

int pbccs_ccs_batch_demux(pbccs_engine* eng, const pbccs_ccs_input* in, int n, long long max_poa_coverage,
                          const pbccs_polish_options* opts, const pbccs_demux_barcodes* barcodes,
                          const pbccs_demux_options* demux_opts, pbccs_ccs_output* out, pbccs_demux_output* demux,
                          int* demuxed_mask)
{
    if (!eng || (n > 0 && !demux)) return fail(PBCCS_EINVAL, "bad argument");
    if (demux && demux->scores) return fail(PBCCS_EINVAL, "pbccs_ccs_batch_demux returns no score matrix");
    demux::DemuxOptions o;
    if (const int rc = demux_check(barcodes, demux_opts, &o)) return rc;
    const int rc = pbccs_ccs_batch(eng, in, n, max_poa_coverage, opts, out);
    if (rc != PBCCS_OK) return rc;
    return guarded([&] {
        std::vector<const char*> seqs;
        std::vector<int> lens, at;
        for (int z = 0; z < n; ++z) {
            const bool ok = out[z].polish.status == 0 && out[z].polish.consensus && out[z].polish.consensus_len > 0;
            if (demuxed_mask) demuxed_mask[z] = ok ? 1 : 0;
            if (!ok) continue;
            seqs.push_back(out[z].polish.consensus);
            lens.push_back(out[z].polish.consensus_len);
            at.push_back(z);
        }
        if (!seqs.empty()) demux_run(eng, barcodes, o, seqs, lens, at.data(), demux);
        return PBCCS_OK;
    });
}

}  // extern "C"

/*
 * pbccs_amd.h -- C ABI of the MI355X consensus-polishing engine (drop-in for pbccs' polish path).
 *
 * The reference's hot path is a C++ template API, not an FFI: pbccs' per-ZMW driver
 * (include/pacbio/ccs/Consensus.h:436-512) drives ConsensusCore's
 *   Arrow::MultiReadMutationScorer  (ConsensusCore/include/ConsensusCore/Arrow/MultiReadMutationScorer.hpp:82-284)
 *   RefineConsensus / ConsensusQVs  (ConsensusCore/include/ConsensusCore/Consensus.hpp:63-79, Consensus-inl.hpp:159-295)
 * Every entry point below replaces one of those calls (cited per function); include/pbccs_amd/ConsensusCore.hpp
 * wraps them back into the reference's C++ class names so a Consensus.h-equivalent compiles unchanged
 * (INTEGRATION.md).  Plain pointers and sizes only; nothing throws across this boundary.
 */
#ifndef PBCCS_AMD_H
#define PBCCS_AMD_H

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes -------------------------------------------------------------------------- */
#define PBCCS_OK 0
#define PBCCS_EINVAL (-1)   /* bad argument (InvalidInputError, std::out_of_range in the reference) */
#define PBCCS_EOOM (-2)     /* device allocation failed */
#define PBCCS_EDEVICE (-3)  /* HIP runtime / kernel failure */
#define PBCCS_ESTATE (-4)   /* call out of order (e.g. BadExecutionOrderException) */
#define PBCCS_ERANGE (-5)   /* caller buffer too small; the required size is returned through *len */

/* Mutation types (ConsensusCore/include/ConsensusCore/Mutation.hpp:50-53) */
#define PBCCS_INSERTION 0
#define PBCCS_DELETION 1
#define PBCCS_SUBSTITUTION 2
/* Strands (ConsensusCore/include/ConsensusCore/Read.hpp:66-70) */
#define PBCCS_FORWARD_STRAND 0
#define PBCCS_REVERSE_STRAND 1
/* AddReadResult (ConsensusCore/include/ConsensusCore/Arrow/MultiReadMutationScorer.hpp:60) */
#define PBCCS_ADD_SUCCESS 0
#define PBCCS_ADD_ALPHABETAMISMATCH 1
#define PBCCS_ADD_MEM_FAIL 2
#define PBCCS_ADD_POOR_ZSCORE 3
#define PBCCS_ADD_OTHER 4
/* Per-ZMW outcome (pbccs ResultType counters, include/pacbio/ccs/Consensus.h:150-210) */
#define PBCCS_ZMW_SUCCESS 0
#define PBCCS_ZMW_NO_SUBREADS 1
#define PBCCS_ZMW_TOO_SHORT 2
#define PBCCS_ZMW_TOO_MANY_UNUSABLE 3
#define PBCCS_ZMW_TOO_FEW_PASSES 4
#define PBCCS_ZMW_NON_CONVERGENT 5
#define PBCCS_ZMW_POOR_QUALITY 6
#define PBCCS_ZMW_OTHER 7

typedef struct pbccs_engine pbccs_engine; /* one per GPU; externally synchronised */
typedef struct pbccs_scorer pbccs_scorer; /* one ArrowMultiReadMutationScorer */

/* A single-base mutation: start/end as in ConsensusCore::Mutation (insertion: end == start). */
typedef struct {
    int type;
    int start;
    int end;
    char new_base; /* 'A','C','G','T'; ignored for deletions */
} pbccs_mutation;

/* ArrowConfig + BandingOptions (ConsensusCore/include/ConsensusCore/Arrow/ArrowConfig.hpp:104-128) */
typedef struct {
    double snr[4];               /* SNR(A, C, G, T) -> ContextParameters */
    double score_diff;           /* BandingOptions::ScoreDiff (ccs: 12.5) */
    double fast_score_threshold; /* ArrowConfig::FastScoreThreshold (default -12.5) */
    double add_threshold;        /* ArrowConfig::AddThreshold (default NaN = no z-score gate) */
} pbccs_arrow_config;

/* RefineOptions (ConsensusCore/include/ConsensusCore/Consensus.hpp:48-60), defaults 40/10/20 */
typedef struct {
    int max_iterations;
    int mutation_separation;
    int mutation_neighborhood;
} pbccs_refine_options;

/* ---- engine --------------------------------------------------------------------------------- */
int pbccs_engine_create(int device, pbccs_engine** out);
void pbccs_engine_destroy(pbccs_engine* eng);
const char* pbccs_last_error(void); /* thread-local message of the last failed call */
int pbccs_device_count(void);

/* ---- ArrowMultiReadMutationScorer (Arrow/MultiReadMutationScorer.cpp) ---------------------- */
/* MultiReadMutationScorer(const ArrowConfig&, std::string tpl)                       (.cpp:143-154) */
int pbccs_scorer_create(pbccs_engine* eng, const pbccs_arrow_config* cfg, const char* tpl, int tpl_len,
                        pbccs_scorer** out);
void pbccs_scorer_destroy(pbccs_scorer* s);
/* AddReadResult AddRead(const MappedArrowRead&, double threshold)                    (.cpp:275-325)
 * threshold NaN = no z-score gate; pass cfg->add_threshold for the one-argument overload (.cpp:334). */
int pbccs_scorer_add_read(pbccs_scorer* s, const char* seq, int len, int strand, int tstart, int tend,
                          double threshold, int* result);
/* double Score(const Mutation&, double fastScoreThreshold = -DBL_MAX)                (.cpp:338-368)
 * FastScore(m) == Score(m, cfg->fast_score_threshold)                                (.cpp:380-383) */
int pbccs_scorer_score(pbccs_scorer* s, const pbccs_mutation* m, double fast_threshold, double* score);
/* Batched Score over n mutations (same semantics per element). */
int pbccs_scorer_score_many(pbccs_scorer* s, const pbccs_mutation* m, int n, double fast_threshold, double* scores);
/* std::vector<double> Scores(const Mutation&, double unscoredValue)                  (.cpp:384-417)
 * per_read must hold NumReads() entries. */
int pbccs_scorer_scores(pbccs_scorer* s, const pbccs_mutation* m, double unscored, double* per_read);
/* IsFavorable / FastIsFavorable (score > 0.04)                                       (.cpp:428-440) */
int pbccs_scorer_is_favorable(pbccs_scorer* s, const pbccs_mutation* m, int fast, int* favorable);
/* void ApplyMutations(const std::vector<Mutation>&)                                  (.cpp:235-267) */
int pbccs_scorer_apply_mutations(pbccs_scorer* s, const pbccs_mutation* m, int n);
/* std::string Template(StrandEnum)                                                   (.cpp:183-188)
 * writes at most cap bytes (NUL-terminated); *len = template length. */
int pbccs_scorer_template(pbccs_scorer* s, int strand, char* out, int cap, int* len);
int pbccs_scorer_template_length(pbccs_scorer* s);                                 /* (.cpp:169-173) */
int pbccs_scorer_num_reads(pbccs_scorer* s);                                       /* (.cpp:176-180) */
/* Read(i): active flag and current mapping (MappedArrowRead*, NULL when inactive)    (.cpp:192-196) */
int pbccs_scorer_read_info(pbccs_scorer* s, int i, int* active, int* strand, int* tstart, int* tend);
/* double BaselineScore() / std::vector<double> BaselineScores()                      (.cpp:495-520) */
int pbccs_scorer_baseline_score(pbccs_scorer* s, double* score);
int pbccs_scorer_baseline_scores(pbccs_scorer* s, double* out, int cap, int* n);
/* ZScores(): ((zg, za), per-read z)  per_read must hold NumReads() entries      (.hpp:208-263) */
int pbccs_scorer_zscores(pbccs_scorer* s, double* zg, double* za, double* per_read);
/* NumFlipFlops() per read                                                            (.cpp:480-488) */
int pbccs_scorer_num_flipflops(pbccs_scorer* s, int* out);

/* bool RefineConsensus(MRMS&, size_t* nTested, size_t* nApplied, const RefineOptions&)
 *                                                       (Consensus.hpp:63-67, Consensus-inl.hpp:159-262) */
int pbccs_refine_consensus(pbccs_scorer* s, const pbccs_refine_options* opts, long long* n_tested,
                           long long* n_applied, int* converged);
/* std::vector<int> ConsensusQVs(MRMS&)                  (Consensus.hpp:77-78, Consensus-inl.hpp:274-295) */
int pbccs_consensus_qvs(pbccs_scorer* s, int* qvs, int cap, int* n);

/* ---- batched ccs polish: Consensus<>() after the POA, for many ZMWs per call ------------------
 * Mirrors include/pacbio/ccs/Consensus.h:436-552 from `ArrowConfig config(...)` on: AddRead(mr,
 * MinZScore) per read with status counts, the MinPasses / MaxDropFraction gates, ZScores(),
 * RefineConsensus(), ConsensusQVs(), predicted accuracy and the MinPredictedAccuracy gate.
 * Results are written in input order (WorkQueue.h:128-167 ordering). */
typedef struct {
    const char* draft;         /* POA consensus (ACGT) */
    int draft_len;
    double snr[4];
    int n_reads;
    const char* const* seqs;   /* read bases as passed to MappedArrowRead (already extent-clipped); NULL: a
                                * read the driver did not add (POA key -1 or ExtractMappedRead none,
                                * Consensus.h:448-451) -- counted in the drop fraction's denominator only */
    const int* lens;
    const int* strands;
    const int* tstarts;        /* mapped window on the draft [tstart, tend) */
    const int* tends;
    const unsigned char* full_pass; /* ADAPTER_BEFORE && ADAPTER_AFTER per read (NULL: all full passes) */
} pbccs_zmw_input;

typedef struct {
    int min_passes;               /* ConsensusSettings::MinPasses (3) */
    int min_length;               /* ConsensusSettings::MinLength (10): draft shorter -> TOO_SHORT */
    double min_zscore;            /* ConsensusSettings::MinZScore (-5; NaN disables) */
    double max_drop_fraction;     /* ConsensusSettings::MaxDropFraction (0.34) */
    double min_predicted_accuracy;/* ConsensusSettings::MinPredictedAccuracy (0.90) */
    double score_diff;            /* BandingOptions(12.5) */
    pbccs_refine_options refine;  /* {40, 10, 20} */
    int zmws_per_batch;           /* device batch size (0 = auto from the memory budget) */
} pbccs_polish_options;

typedef struct {
    int status;          /* PBCCS_ZMW_* */
    char* consensus;     /* caller buffer, consensus_cap bytes; NUL-terminated */
    int consensus_cap;
    int consensus_len;   /* -required length when the buffer was too small */
    int* qvs;            /* caller buffer, consensus_cap entries (raw, unclipped QVs) */
    int* add_read_results; /* caller buffer, n_reads entries (-1: read not added) */
    double* zscores;     /* caller buffer, n_reads entries */
    double zg, za;
    double predicted_accuracy;
    long long n_tested, n_applied;
    int n_passes;
    int status_counts[5]; /* AddReadResult histogram */
} pbccs_zmw_output;

void pbccs_polish_options_default(pbccs_polish_options* o);
/* One call: upload, polish and download n ZMWs -- the ZMW work queue of ccs (src/main/ccs.cpp:222-262,
 * WorkQueue.h:64-167) for a stream of heterogeneous ZMWs.  With opts->zmws_per_batch == 0 the ZMWs are
 * bucketed by template length and pass count into device batches sized to the free device memory
 * (pbccs_plan_batches), and the engine's workspace slots pull batches largest-first from a shared queue;
 * otherwise consecutive chunks of zmws_per_batch.  Outputs land in input order either way.  A batch that
 * runs the device out of memory (PBCCS_EOOM) while the other slots hold theirs is rerun alone after the
 * slots' band pools are unmapped, halved while it still does not fit. */
int pbccs_polish_batch(pbccs_engine* eng, const pbccs_zmw_input* in, int n, const pbccs_polish_options* opts,
                       pbccs_zmw_output* out);

/* Host-only batch plan behind pbccs_polish_batch (no device needed).  ZMWs are ordered by (draft length,
 * read count); a batch closes when it holds max_per_batch ZMWs, when its estimated FP64 band footprint
 * would pass budget_bytes, or when a draft is more than max_len_ratio times the batch's first draft
 * (length buckets limit divergence inside a launch).  A ZMW whose own estimate exceeds the budget gets a
 * batch of its own.  order[n] receives the ZMW permutation, batch_start[n + 1] the batch offsets into it
 * (batch b is order[batch_start[b] .. batch_start[b + 1])), est_bytes[n] (may be NULL) each ZMW's
 * estimate; *n_batches the batch count.  Batches are listed largest estimate first. */
int pbccs_plan_batches(const pbccs_zmw_input* in, int n, double budget_bytes, int max_per_batch,
                       double max_len_ratio, int* order, int* batch_start, double* est_bytes, int* n_batches);

/* The same in two phases, so that inputs can be made resident in HBM ahead of time:
 * pbccs_batch_create copies the ZMWs to the device; pbccs_batch_polish runs the hot path (AddRead fills,
 * gates, ZScores, RefineConsensus, ConsensusQVs) and writes the outputs.  A batch polishes once. */
typedef struct pbccs_batch pbccs_batch;
int pbccs_batch_create(pbccs_engine* eng, const pbccs_zmw_input* in, int n, const pbccs_polish_options* opts,
                       pbccs_batch** out);
int pbccs_batch_polish(pbccs_batch* b, pbccs_zmw_output* out);
void pbccs_batch_destroy(pbccs_batch* b);

/* Polish several batches of one engine concurrently: one host thread and one HIP stream per workspace
 * slot, so that one batch's convergence tail (the last refine rounds of a few ZMWs) overlaps the other
 * batches' work.  The analogue of ccs's ZMW thread pool (src/main/ccs.cpp:222-230, WorkQueue.h).
 * outs[i] receives batch i's outputs.  A batch that runs the device out of memory (PBCCS_EOOM) while the
 * others hold their band pools is rebuilt from its inputs (the batch keeps a host copy) and rerun alone once
 * every slot's pool is unmapped, halved while it still does not fit; pbccs_batch_polish does the same for
 * a single batch.  Returns the first failure. */
int pbccs_batch_polish_many(pbccs_batch* const* batches, int n, pbccs_zmw_output* const* outs);

/* Number of workspace slots = batches that may polish at the same time (default 4).  Set it before
 * creating batches; each slot holds its own resident band pools. */
int pbccs_engine_set_concurrency(pbccs_engine* eng, int batches_in_flight);

/* Map `bytes_per_slot` of band-value pool for every workspace slot now, instead of on first use.  Pool
 * memory stays mapped for the engine's lifetime and is reused by every batch the slot polishes, so a
 * long run pays the mapping once; this moves that one-time cost out of a timed region.  The mapped
 * memory is also written once (zeroed), so call it while no batch is polishing.  Optional. */
int pbccs_engine_reserve_pool(pbccs_engine* eng, size_t bytes_per_slot);

/* Work counters of the engine since the last reset (for roofline accounting). */
typedef struct {
    long long fill_launches, score_launches, score_tasks, mutations;
    long long band_top_bytes;    /* max over batches: band value pool handed out (the bump top) */
    long long band_region_bytes; /* max over batches: the reads' current band regions (2 x capacity each) */
    long long band_used_bytes;   /* max over batches: band cells the reads' last fills stored */
    long long pool_mapped_bytes; /* device memory the workspace slots' band pools hold mapped now */
    long long oom_retries;       /* device batches rerun after running the device out of memory */
    long long create_host_ns;    /* pbccs_batch_create: the batch's own copy of its inputs and the read pool */
    long long create_upload_ns;  /* pbccs_batch_create: device reservations + the read upload */
    long long derive_ns;         /* the per-ZMW setup of Consensus.h:437-453 (transition tables, expectations,
                                    reverse-complement template), run by the polish at its first device step */
    long long fill_work[16];     /* PBCCS_FILL_WORK=1 diagnostics, per fill kind k (0: 16-lane, 1: 64-lane) at
                                    [8 k + ...]: counted cells, cells thrown away by a tall abort, count-only
                                    regrow cells, count-only overflow cells, group chunk steps, wave chunk issues,
                                    reads, counted passes */
    long long scan_reads;        /* certified fast path: reads its tall fills took */
    long long uncertain_reads;   /* ... reads re-run exactly (a fill decision or the AddRead gate within the bound) */
    long long exact_rounds;      /* ... ZMW rounds re-scored on exact bands (a score decision within the bound) */
    long long uncertain_why[4];  /* ... uncertain fills by decision: band end, begin hint, loop entry, final mismatch */
    long long repeat_skipped_ckpt; /* pbccs_polish_batch_ex: ZMWs whose repeat round was skipped because a read keeps
                                    checkpointed bands */
} pbccs_counters;
int pbccs_engine_counters(pbccs_engine* eng, pbccs_counters* out, int reset);

/* Per-kernel profile (enabled by pbccs_engine_set_profiling): launches, summed device time from HIP
 * events on the engine's stream, and algorithmic work counted in-kernel: `cells` DP cell-updates,
 * `bytes` algorithmic band bytes (8 B per stored/read band cell + 16 B per column),
 * `wave_s` wavefront-seconds resident on the device (each wavefront's start-to-end time, summed; over a
 * timed region it gives the family's average resident waves; the fills, k_score family, k_suffix, k_reduce). */
typedef struct {
    char name[32];
    long long launches;
    double device_ms;
    double cells;
    double bytes;
    double wave_s;
} pbccs_kernel_stat;
int pbccs_engine_set_profiling(pbccs_engine* eng, int on);
int pbccs_engine_kernel_stats(pbccs_engine* eng, pbccs_kernel_stat* out, int cap, int* n, int reset);


/* ---- Quiver family (ConsensusCore/include/ConsensusCore/Quiver/) ---------------------------------
 * ccs does not call it; the north_star names it (QuiverConfig, QvEvaluator, SseRecursor).  One scorer =
 * MultiReadMutationScorer<SparseSseQvRecursor> (Viterbi) or <SparseSseQvSumProductRecursor>
 * (Quiver/MultiReadMutationScorer.hpp:242-245).  Scores are FP32 log-likelihoods. */
typedef struct pbccs_quiver_scorer pbccs_quiver_scorer;

/* QvModelParams (Quiver/QuiverConfig.hpp:79-176); merge / merge_s per template base A, C, G, T */
typedef struct {
    float match, mismatch, mismatch_s, branch, branch_s, deletion_n, deletion_with_tag, deletion_with_tag_s, nce,
        nce_s;
    float merge[4], merge_s[4];
} pbccs_qv_model_params;

/* Recursor types of ConsensusCore's Quiver MutationScorer typedefs (Quiver/MutationScorer.hpp:93-99):
 * SseRecursor or SimpleRecursor (Quiver/SimpleRecursor.cpp: row-by-row fills, moves combined Inc, Extra,
 * Del, Merge) over SparseMatrixF or DenseMatrixF storage (AllocatedEntries = Rows * Columns). */
#define PBCCS_QV_RECURSOR_SPARSE_SSE 0
#define PBCCS_QV_RECURSOR_SPARSE_SIMPLE 1
#define PBCCS_QV_RECURSOR_DENSE_SSE 2
#define PBCCS_QV_RECURSOR_DENSE_SIMPLE 3

/* QuiverConfig (QuiverConfig.hpp:181-199) + the recursor's combiner */
typedef struct {
    pbccs_qv_model_params params;
    int moves_available;         /* Move bits: INCORPORATE 1, EXTRA 2, DELETE 4, MERGE 8 (ALL_MOVES 15) */
    float score_diff;            /* BandingOptions::ScoreDiff (the diagonal-cross argument is ignored) */
    float fast_score_threshold;  /* QuiverConfig::FastScoreThreshold */
    float add_threshold;         /* QuiverConfig::AddThreshold (1.0 = no memory gate) */
    int sum_product;             /* 0: Viterbi (SparseSseQvRecursor), 1: sum-product (logAdd) */
    int recursor;                /* PBCCS_QV_RECURSOR_*: the recursor family and matrix storage */
} pbccs_quiver_config;

/* MultiReadMutationScorer(const QuiverConfigTable&, std::string tpl)  (Quiver/MultiReadMutationScorer.cpp:123-136)
 * The table: n configs with their chemistry names ("*" = the InsertDefault fallback, QuiverConfig.cpp:67-138). */
int pbccs_quiver_scorer_create(pbccs_engine* eng, const pbccs_quiver_config* configs, const char* const* chemistries,
                               int n_configs, const char* tpl, int tpl_len, pbccs_quiver_scorer** out);
void pbccs_quiver_scorer_destroy(pbccs_quiver_scorer* s);
/* bool AddRead(const MappedQvRead&, float threshold)                                    (.cpp:246-290)
 * QvSequenceFeatures tracks of len floats each (NULL = zeros); del_tag holds the tag bases as float(char).
 * threshold NaN = the read's config AddThreshold (the one-argument overload). *active = the return value. */
int pbccs_quiver_scorer_add_read(pbccs_quiver_scorer* s, const char* seq, int len, const float* ins_qv,
                                 const float* subs_qv, const float* del_qv, const float* del_tag,
                                 const float* merge_qv, const char* chemistry, int strand, int tstart, int tend,
                                 float threshold, int* active);
/* float Score(m) / FastScore(m) (.cpp:312-353); many at once */
int pbccs_quiver_scorer_score_many(pbccs_quiver_scorer* s, const pbccs_mutation* m, int n, int fast, float* scores);
/* MutationScorer<R>::ScoreMutation (Quiver/MutationScorer.cpp:113-226) on read i's own scorer: the mutation is
 * in the read's window coordinates and the absolute score of the mutated window is returned */
int pbccs_quiver_scorer_read_score_mutation(pbccs_quiver_scorer* s, int i, const pbccs_mutation* m, float* score);
/* std::vector<float> Scores(m, unscoredValue) (.cpp:355-371); per_read holds NumReads() entries */
int pbccs_quiver_scorer_scores(pbccs_quiver_scorer* s, const pbccs_mutation* m, float unscored, float* per_read);
/* IsFavorable / FastIsFavorable (.cpp:382-409) */
int pbccs_quiver_scorer_is_favorable(pbccs_quiver_scorer* s, const pbccs_mutation* m, int fast, int* favorable);
int pbccs_quiver_scorer_apply_mutations(pbccs_quiver_scorer* s, const pbccs_mutation* m, int n);   /* (.cpp:205-239) */
int pbccs_quiver_scorer_template(pbccs_quiver_scorer* s, int strand, char* out, int cap, int* len);
int pbccs_quiver_scorer_num_reads(pbccs_quiver_scorer* s);
int pbccs_quiver_scorer_read_info(pbccs_quiver_scorer* s, int i, int* active, int* strand, int* tstart, int* tend);
int pbccs_quiver_scorer_baseline_score(pbccs_quiver_scorer* s, float* score);          /* (.cpp:467-476) */
int pbccs_quiver_scorer_baseline_scores(pbccs_quiver_scorer* s, float* out, int cap, int* n);
int pbccs_quiver_scorer_num_flipflops(pbccs_quiver_scorer* s, int* out);
/* AllocatedEntries of read i's alpha / beta (SparseMatrix-inl.hpp:275-284) */
int pbccs_quiver_scorer_allocated_entries(pbccs_quiver_scorer* s, int i, long long* alpha, long long* beta);
/* RecursorBase::Alignment(e, alpha) (Quiver/detail/RecursorBase.cpp:124-264) of read i on its template window:
 * the Viterbi traceback through the read's alpha band, as PairwiseAlignment Target() / Query() (gapped,
 * len characters each).  PBCCS_ESTATE for a sum-product scorer (the reference's ShouldNotReachHere) or a
 * read without a scorer; PBCCS_ERANGE when cap < len. */
int pbccs_quiver_scorer_alignment(pbccs_quiver_scorer* s, int i, char* target, char* query, int cap, int* len);
int pbccs_quiver_refine_consensus(pbccs_quiver_scorer* s, const pbccs_refine_options* opts, long long* n_tested,
                                  long long* n_applied, int* converged);
int pbccs_quiver_consensus_qvs(pbccs_quiver_scorer* s, int* qvs, int cap, int* n);

/* ---- Quiver: mutations of any width ---------------------------------------------------------------
 * Mutation (Mutation.hpp) with its new-bases string: an insertion has start == end and n_bases >= 1, a
 * deletion start < end and n_bases == 0, a substitution n_bases == end - start (Mutation-inl.hpp:102-115).
 * Bases are A, C, G, T and the reference's phony test bases M and N, complements of each other
 * (Sequence.cpp:41-78).  n_bases <= 7: the reference's extend buffer has 8 columns (EXTEND_BUFFER_COLUMNS,
 * asserted at Quiver/MutationScorer.cpp:177).  The Arrow scorer takes them too, through its own _ex calls
 * below ("Arrow: mutations of any width"): A, C, G and T only there.  The reference's Arrow scorer refuses
 * |LengthDiff| > 1 (Arrow/MutationScorer.cpp:181-183); pbccs_mutation and the calls that take it stay
 * single-base. */
typedef struct {
    int type;
    int start;
    int end;
    const char* new_bases; /* n_bases characters (need not be NUL-terminated); ignored for deletions */
    int n_bases;
} pbccs_mutation_ex;
#define PBCCS_MAX_MUTATION_BASES 7

/* The single-base entry points' twins.  A (read, mutation) pair whose ScoreMutation would need more than 8
 * extend-buffer columns -- the begin / end cases of Quiver/MutationScorer.cpp:187-220, the whole fill of a
 * window of 7 or more columns, or an insertion of n bases needing 1 + n -- is found on the host from the
 * oriented mutation and the read's window before anything is launched: the call returns PBCCS_EINVAL and
 * computes nothing (the reference writes past its buffer there). */
int pbccs_quiver_scorer_score_many_ex(pbccs_quiver_scorer* s, const pbccs_mutation_ex* m, int n, int fast,
                                      float* scores);
int pbccs_quiver_scorer_scores_ex(pbccs_quiver_scorer* s, const pbccs_mutation_ex* m, float unscored,
                                  float* per_read);
int pbccs_quiver_scorer_is_favorable_ex(pbccs_quiver_scorer* s, const pbccs_mutation_ex* m, int fast,
                                        int* favorable);
int pbccs_quiver_scorer_read_score_mutation_ex(pbccs_quiver_scorer* s, int i, const pbccs_mutation_ex* m,
                                               float* score);
/* ApplyMutations (Mutation.cpp:115-128) with the reads' windows remapped by TargetToQueryPositions; A, C, G
 * and T only, so the template stays ACGT. */
int pbccs_quiver_scorer_apply_mutations_ex(pbccs_quiver_scorer* s, const pbccs_mutation_ex* m, int n);

/* RefineRepeats (Consensus.hpp:69-76): AbstractRefineConsensus (Consensus-inl.hpp:159-251) over
 * RepeatMutationEnumerator(repeat_length, min_repeat_elements).  The reference's RefineRepeatOptions sets
 * MaximumIterations = 1 and leaves MutationSeparation and MutationNeighborhood unset (Consensus-inl.hpp:57-68),
 * and its RefineRepeats body cannot be instantiated, so no reference run of the loop exists: the defaults
 * here for the two unset fields are DefaultRefineOptions' 10 and 20.  opts NULL = {2, 3, 1, 10, 20}.
 * repeat_length <= 7 (an insertion of one element needs 1 + repeat_length columns); a candidate that breaks
 * the 8-column rule ends the call with PBCCS_EINVAL. */
typedef struct {
    int repeat_length;
    int min_repeat_elements;  /* 3 */
    int max_iterations;       /* 1 */
    int mutation_separation;  /* 10 */
    int mutation_neighborhood; /* 20 */
} pbccs_repeat_options;
int pbccs_quiver_refine_repeats(pbccs_quiver_scorer* s, const pbccs_repeat_options* opts, long long* n_tested,
                                long long* n_applied, int* converged);

/* Host-only (no engine or device needed).
 * pbccs_repeat_mutations: RepeatMutationEnumerator::Mutations(begin, end) (MutationEnumerator.cpp:161-218) in
 * the reference's order: per repeat run the insertion, then the deletion, of one element.  new_bases of an
 * insertion points into tpl.  Nothing for min_repeat_elements <= 0 or repeat_length > 31.  *n = the count;
 * PBCCS_ERANGE when it exceeds cap (out may be NULL with cap 0 to size the call).
 * pbccs_apply_mutations: ApplyMutations (Mutation.cpp:115-128) into out (NUL-terminated, cap bytes) and
 * TargetToQueryPositions (Mutation.cpp:193-197) into mtp[tpl_len + 1] (may be NULL).  Any bases; overlapping
 * edits and edits outside the template are PBCCS_EINVAL. */
int pbccs_repeat_mutations(const char* tpl, int tpl_len, int repeat_length, int min_repeat_elements, int begin,
                           int end, pbccs_mutation_ex* out, int cap, int* n);
int pbccs_apply_mutations(const char* tpl, int tpl_len, const pbccs_mutation_ex* muts, int n, char* out, int cap,
                          int* len, int* mtp);

/* QvEvaluator (Quiver/QvEvaluator.hpp:90-317): the four move scores of one read (QvSequenceFeatures,
 * Features.hpp:69-100) against a template under QvModelParams, at n cells (i[k], j[k]), evaluated on the device
 * with the recursions' own evaluator.  Inc(i, j) (:160-167), Del(i, j) with the pinStart / pinEnd rule (:169-184),
 * Extra(i, j) (:186-193), Merge(i, j) (:195-207).  A cell outside a move's domain -- the reference's asserts:
 * Inc 0 <= i < I, 0 <= j < J; Del 0 <= i <= I, 0 <= j < J; Extra 0 <= i < I, 0 <= j <= J; Merge 0 <= i < I,
 * 0 <= j < J - 1 -- gives NaN.  Feature tracks of len floats (NULL = zeros; del_tag as float(char)); any output
 * array may be NULL. */
typedef struct {
    const char* seq;
    int len;
    const float* ins_qv;
    const float* subs_qv;
    const float* del_qv;
    const float* del_tag;
    const float* merge_qv;
} pbccs_qv_features;
int pbccs_qv_evaluator_moves(pbccs_engine* eng, const pbccs_qv_features* read, const char* tpl, int tpl_len,
                             const pbccs_qv_model_params* params, int pin_start, int pin_end, const int* i,
                             const int* j, int n, float* inc, float* del, float* extra, float* merge);

/* Batched Quiver polish: for every ZMW, what a caller of the scorer API above does with one scorer --
 * create over (configs, chemistries), AddRead each read (threshold NaN = its config's add_threshold),
 * RefineConsensus(opts), ConsensusQVs -- with every scorer's fills, mutation scores, Score /
 * FastIsFavorable reduction and BestSubset on the device in lock-step rounds (one refill launch per
 * round).  Results equal the per-scorer calls'.  consensus / qvs: caller buffers of consensus_cap; qvs
 * NULL skips ConsensusQVs.  ok = 0: RefineConsensus refused an edit (the scorer call's PBCCS_EINVAL). */
typedef struct {
    const char* seq;
    int len;
    const float* ins_qv;
    const float* subs_qv;
    const float* del_qv;
    const float* del_tag;   /* float(char) per base, as pbccs_quiver_scorer_add_read */
    const float* merge_qv;
    const char* chemistry;  /* NULL = "*" */
    int strand, tstart, tend;
    float threshold;
} pbccs_quiver_read;

typedef struct {
    const char* tpl;
    int tpl_len;
    const pbccs_quiver_read* reads;
    int n_reads;
} pbccs_quiver_zmw;

typedef struct {
    char* consensus;
    int consensus_cap;
    int consensus_len;
    int* qvs;
    long long n_tested, n_applied;
    int converged;
    int ok;
    int n_active;           /* reads AddRead kept */
} pbccs_quiver_result;

int pbccs_quiver_polish_batch(pbccs_engine* eng, const pbccs_quiver_config* configs, const char* const* chemistries,
                              int n_configs, const pbccs_quiver_zmw* zmws, int n, const pbccs_refine_options* opts,
                              pbccs_quiver_result* out);
/* The same with RefineRepeats between RefineConsensus and ConsensusQVs: per ZMW RefineConsensus(opts),
 * RefineRepeats(repeats), ConsensusQVs, the repeat rounds in lock-step too (one scoring launch series for all
 * scorers, one reduction and one refill per round; BestSubset on the host).  repeat_tested / repeat_applied
 * (n entries each, may be NULL) receive RefineRepeats' counts; n_tested / n_applied stay RefineConsensus'.
 * ok = 0 also where RefineRepeats ended with PBCCS_EINVAL.  repeats == NULL is exactly
 * pbccs_quiver_polish_batch. */
int pbccs_quiver_polish_batch_ex(pbccs_engine* eng, const pbccs_quiver_config* configs, const char* const* chemistries,
                                 int n_configs, const pbccs_quiver_zmw* zmws, int n, const pbccs_refine_options* opts,
                                 const pbccs_repeat_options* repeats, long long* repeat_tested,
                                 long long* repeat_applied, pbccs_quiver_result* out);

/* ---- Arrow: mutations of any width -------------------------------------------------
 * The twins of pbccs_scorer_score_many / _scores / _is_favorable / _apply_mutations for pbccs_mutation_ex, and
 * RefineRepeats for the Arrow scorer.  The reference's Arrow MutationScorer::ScoreMutation is written for any
 * length behind a guard that refuses |LengthDiff| > 1, and its template pair holds a two-slot virtual mutation;
 * these calls run ScoreMutation's four cases over a template view that holds the whole mutation (k_score_wide);
 * a mutation three or more bases wide takes the last of them, the refill of the window (k_score_wide_refill),
 * because the bands of the unmutated template do not hold its paths.
 * They always take that kernel, at width 1 too, where the scores equal the single-base calls' bit for bit.
 * The 8-column rule: the extension columns every active scoring read needs -- 1 + n_bases in the middle of its
 * window (2 for a deletion), up to the window's end or start in the edge cases -- are derived on the host from
 * the oriented, clipped mutation; more than 8 on any read, n_bases > 7, a base outside A, C, G, T or a mutation
 * outside the template is PBCCS_EINVAL before anything is launched.  A scorer with a read on checkpointed bands
 *  is PBCCS_EINVAL too: k_score_wide reads stored columns only.  The scorer stays usable. */
int pbccs_scorer_score_many_ex(pbccs_scorer* s, const pbccs_mutation_ex* m, int n, double fast_threshold,
                               double* scores);
/* per_read holds NumReads() entries; `unscored` where a read is inactive or does not score the mutation */
int pbccs_scorer_scores_ex(pbccs_scorer* s, const pbccs_mutation_ex* m, double unscored, double* per_read);
int pbccs_scorer_is_favorable_ex(pbccs_scorer* s, const pbccs_mutation_ex* m, int fast, int* favorable);
/* ApplyMutations with the reads' windows remapped by TargetToQueryPositions, then the refill.  Overlapping
 * edits, edits outside the template and an insertion at the template's end are PBCCS_EINVAL. */
int pbccs_scorer_apply_mutations_ex(pbccs_scorer* s, const pbccs_mutation_ex* m, int n);
/* RefineRepeats for the Arrow scorer: AbstractRefineConsensus (Consensus-inl.hpp:159-251) over
 * RepeatMutationEnumerator, the favourable test Score(m, FastScoreThreshold) > 0.04.  opts NULL = {2, 3, 1, 10, 20}
 * (see pbccs_quiver_refine_repeats).  n_tested / n_applied are set, not added to. */
int pbccs_refine_repeats(pbccs_scorer* s, const pbccs_repeat_options* opts, long long* n_tested,
                         long long* n_applied, int* converged);
/* Host-only: the extension columns one read with window [tstart, tend) on `strand` needs for the mutation.
 * *columns = -1: the read does not score it; 0: the whole-window refill (no extension buffer); -2: the mutated
 * window would be empty.  -2 and *columns > 8 are what the calls above refuse. */
int pbccs_wide_columns_needed(const pbccs_mutation_ex* m, int strand, int tstart, int tend, int* columns);
/* pbccs_polish_batch with RefineRepeats between RefineConsensus and ConsensusQVs for every ZMW RefineConsensus
 * converged on, the repeat rounds batched across the ZMWs of a device batch (one k_score_wide launch and one
 * refill per round).  Records equal the per-scorer sequence RefineConsensus, RefineRepeats, ConsensusQVs.
 * repeat_tested / repeat_applied (n entries each, may be NULL) receive RefineRepeats' counts (0 where it did not
 * run).  A ZMW with a read on checkpointed bands skips the repeat round and finishes as pbccs_polish_batch does
 * (pbccs_counters.repeat_skipped_ckpt counts it); a ZMW whose repeat round is refused (the 8-column rule, an
 * edit that cannot be applied) ends PBCCS_ZMW_OTHER.  With repeats the batch fills exactly (no certified fast
 * path, no band reclaim).  repeats == NULL is exactly pbccs_polish_batch. */
int pbccs_polish_batch_ex(pbccs_engine* eng, const pbccs_zmw_input* in, int n, const pbccs_polish_options* opts,
                          const pbccs_repeat_options* repeats, long long* repeat_tested, long long* repeat_applied,
                          pbccs_zmw_output* out);

/* ---- Diploid site calling (ConsensusCore Arrow/Diploid.cpp:94-241, Quiver/Diploid.cpp) -----------------
 * A site's scores are n_reads x 9 floats, rows in AddRead order (inactive reads included), columns
 * Scores(Substitution(p, "ACGT"[c]), 0) for c = 0..3 (the template base's own column is exactly 0),
 * Scores(Insertion(p, "ACGT"[c - 4]), 0) for c = 4..7 and Scores(Deletion(p), 0) for c = 8 -- the order
 * LENGTH_DIFFS (Diploid.cpp:99) assumes.  A read that is inactive or does not score a mutation contributes 0;
 * Arrow's doubles are rounded to float.  The site tensor of [begin, end) is [end - begin][n_reads][9]. */
typedef struct {
    int position;             /* template position of the site */
    int allele0;              /* DiploidSite::Allele0 / Allele1: column indices 0..8 */
    int allele1;
    float log_bayes_factor;   /* DiploidSite::LogBayesFactor */
} pbccs_diploid_site;

/* DiploidSite* IsSiteHeterozygous(const float* siteScores, int dim1, int dim2, float logPriorRatio)
 *                                                                                  (Diploid.cpp:219-239)
 * Host-only (no engine or device needed): float arithmetic in the reference's order with the host libm.
 * *is_het = (logBF - log_prior_ratio > 0); site (allele0, allele1, log_bayes_factor; position untouched) and
 * allele_for_read (n_reads entries, AssignReadsToAlleles :204-213) are written either way.
 * n_alleles != 9, n_reads <= 0 or a null pointer: PBCCS_EINVAL (the reference only asserts). */
int pbccs_is_site_heterozygous(const float* site_scores, int n_reads, int n_alleles, float log_prior_ratio,
                               int* is_het, pbccs_diploid_site* site, int* allele_for_read);

/* The site tensor of template positions [begin, end), scored on the device (8 mutations per site through the
 * scorer's scoring round, no fast threshold).  *n = the float count (end - begin) * NumReads() * 9;
 * PBCCS_ERANGE when cap is smaller (out may be NULL with cap 0 to size the call).  begin < 0, end >
 * TemplateLength or begin >= end: PBCCS_EINVAL before any launch; the scorer stays usable. */
int pbccs_scorer_site_scores(pbccs_scorer* s, int begin, int end, float* out, long long cap, long long* n);
int pbccs_quiver_scorer_site_scores(pbccs_quiver_scorer* s, int begin, int end, float* out, long long cap,
                                    long long* n);
/* IsSiteHeterozygous over every site of [begin, end): the device screens each site (k_diploid) and leaves to
 * the host primitive above every site that is heterozygous or lies within the screen's bound of being so, so
 * each reported site is pbccs_is_site_heterozygous' answer on the tensor pbccs_scorer_site_scores returns.
 * host_all != 0 sends every site to the host (same results).  Sites in ascending position; *n = their count,
 * PBCCS_ERANGE when it exceeds cap (nothing is written).  allele_for_read (may be NULL): cap x NumReads()
 * ints, row k for sites[k].  A scorer without reads reports no site. */
int pbccs_scorer_diploid_sites(pbccs_scorer* s, int begin, int end, float log_prior_ratio, int host_all,
                               pbccs_diploid_site* sites, int cap, int* n, int* allele_for_read);
int pbccs_quiver_scorer_diploid_sites(pbccs_quiver_scorer* s, int begin, int end, float log_prior_ratio,
                                      int host_all, pbccs_diploid_site* sites, int cap, int* n,
                                      int* allele_for_read);
/* The screen's work since the last reset */
typedef struct {
    long long sites_screened;      /* sites k_diploid looked at */
    long long sites_sent_to_host;  /* ... whose slices were downloaded and decided by the host primitive */
    long long sites_reported;      /* ... reported heterozygous */
} pbccs_diploid_stats;
int pbccs_diploid_stats_get(pbccs_engine* eng, pbccs_diploid_stats* out, int reset);

/* ---- POA draft (pbccs src/SparsePoa.cpp, ConsensusCore/src/C++/Poa) ---------------------------------
 * The read-vs-graph DP and its traceback run on the device (k_poa_fill / k_poa_trace); the graph lives on
 * the host.  Scores use DefaultPoaConfig (match 3, mismatch -5, insert -4, delete -4). */
#define PBCCS_POA_GLOBAL 0
#define PBCCS_POA_SEMIGLOBAL 1
#define PBCCS_POA_LOCAL 2

/* One ZMW's subreads in FilterReads order (include/pacbio/ccs/Consensus.h:223-292); a NULL sequence is a
 * read FilterReads dropped (key -1, as Consensus.h:378 passes nullptr reads). */
typedef struct {
    const char* const* seqs;
    const int* lens;
    int n_reads;
} pbccs_poa_input;

typedef struct {
    char* consensus;   /* caller buffer of cap bytes (not NUL-terminated); len = consensus length */
    int cap;
    int len;
    int* keys;         /* n_reads: SparsePoa::ReadKey per read; -1 not added; -2 not reached (maxPoaCov) */
    int* rc;           /* n_reads, by key: PoaAlignmentSummary::ReverseComplementedRead */
    int* extents;      /* 4 * n_reads, by key: ExtentOnRead begin/end, ExtentOnConsensus begin/end */
    int n_keys;
} pbccs_poa_output;

/* Consensus.h's PoaConsensus (:352-390) for n ZMWs at once: SparsePoa::OrientAndAddRead per read until
 * max_coverage reads were added, then FindConsensus(min_coverage) with the per-read summaries.
 * min_coverage < 0 uses Consensus.h's rule ((cov < 5) ? 1 : (cov + 1) / 2 - 1).  A consensus longer
 * than its buffer sets that output's len and makes the call return PBCCS_ERANGE after all outputs are
 * written.  A NULL sequence is a dropped read; an empty one is never added either (key -1). */
int pbccs_poa_batch(pbccs_engine* eng, const pbccs_poa_input* in, int n, long long max_coverage, int min_coverage,
                    pbccs_poa_output* out);

/* SparsePoa (include/pacbio/ccs/SparsePoa.h:94-131), one graph per handle */
typedef struct pbccs_sparse_poa pbccs_sparse_poa;
int pbccs_sparse_poa_create(pbccs_engine* eng, pbccs_sparse_poa** out);
void pbccs_sparse_poa_destroy(pbccs_sparse_poa* p);
/* ReadKey OrientAndAddRead(seq, alnOptions, minScoreToAdd)                       (src/SparsePoa.cpp:95-138) */
int pbccs_sparse_poa_orient_and_add_read(pbccs_sparse_poa* p, const char* seq, int len, float min_score_to_add,
                                         int* key);
/* FindConsensus(minCoverage, &summaries)                                          (src/SparsePoa.cpp:140-201)
 * rc / extents as in pbccs_poa_output, one entry per key. */
int pbccs_sparse_poa_find_consensus(pbccs_sparse_poa* p, int min_coverage, char* out, int cap, int* len, int* rc,
                                    int* extents, int* n_keys);
/* ToGraphViz(flags, pc) with pc = FindConsensus(min_coverage)'s consensus; flags: COLOR_NODES 1, VERBOSE_NODES 2 */
int pbccs_sparse_poa_graphviz(pbccs_sparse_poa* p, int flags, int min_coverage, char* out, int cap, int* len);

/* PoaConsensus::FindConsensus(reads, mode, minCoverage) (ConsensusCore PoaConsensus.cpp:86-115): every read
 * added with AddRead in the given mode (no orientation choice).  dot (optional) receives
 * pc->Graph.ToGraphViz(flags, pc).  PBCCS_EINVAL for an empty read (InvalidInputError). */
int pbccs_poa_consensus(pbccs_engine* eng, const char* const* reads, const int* lens, int n, int mode,
                        int min_coverage, char* out, int cap, int* len, int flags, char* dot, int dot_cap,
                        int* dot_len);
/* ---- ccs end to end: Consensus.h's per-ZMW driver for many ZMWs -------------------------------------
 * Each chunk is one ZMW after ccs.cpp's grouping gates (src/main/ccs.cpp:402-475: PoorSNR, read score,
 * TooFewPasses).  pbccs_ccs_batch runs include/pacbio/ccs/Consensus.h:395-552 for all of them:
 * FilterReads (NO_SUBREADS when nothing is left), the POA draft on the GPU (pbccs_poa_batch, with
 * max_poa_coverage), TOO_SHORT for a draft below opts->min_length, ExtractMappedRead per POA key, and the
 * polish (pbccs_polish_batch: AddRead gates, RefineConsensus, ConsensusQVs, the accuracy gate).
 * out[z].polish.add_read_results / zscores are indexed like in[z].seqs, the caller's subread order (size
 * them by n_subreads): a read FilterReads dropped, the POA did not add, ExtractMappedRead rejected or the
 * maxPoaCov stop never reached reads -1 / NaN, as does every read of a ZMW that ended before the polish.
 * A zero-length subread takes part in FilterReads but is never added to the POA (key -1); the same rule
 * holds in pbccs_poa_batch and pbccs_sparse_poa_orient_and_add_read.  A NULL sequence with a positive
 * length or a negative length is PBCCS_EINVAL.  out[z].draft (optional, draft_cap bytes) receives the POA
 * consensus; a draft longer than its buffer sets draft_len and makes the call return PBCCS_ERANGE after
 * all outputs are written.  out[z].add_order (optional, n_subreads ints) receives the caller subread index of
 * each AddRead call in the scorer's order -- FilterReads' stable order (Consensus.h:281, 451-453), which
 * ZScores() and the ccs.bam zs tag follow -- padded with -1. */
typedef struct {
    double snr[4];
    int n_subreads;
    const char* const* seqs;
    const int* lens;
    const unsigned char* flags;   /* LocalContextFlags per subread (ADAPTER_BEFORE 1, ADAPTER_AFTER 2); NULL: full passes */
} pbccs_ccs_input;

typedef struct {
    pbccs_zmw_output polish;
    char* draft;
    int draft_cap;
    int draft_len;
    int* add_order;   /* optional: AddRead order as caller subread indices, -1 padded (n_subreads ints) */
} pbccs_ccs_output;

int pbccs_ccs_batch(pbccs_engine* eng, const pbccs_ccs_input* in, int n, long long max_poa_coverage,
                    const pbccs_polish_options* opts, pbccs_ccs_output* out);

/* POA work counters since the last reset: alignments, DP cells, fill/trace device ms (profiling on) */
typedef struct {
    long long alignments, cells, launches, trace_steps;
    double fill_ms, trace_ms, bytes;
    double prog_ms, device_ms, thread_ms, consensus_ms, total_ms;   /* host wall time of each phase */
} pbccs_poa_stats;
int pbccs_poa_stats_get(pbccs_engine* eng, pbccs_poa_stats* out, int reset);

/* ---- Pairwise alignment (ConsensusCore/src/C++/Align/) ----------------------------------------------
 * Align (PairwiseAlignment.cpp:125-212: Needleman-Wunsch, int32, GLOBAL only), AlignAffine and
 * AlignAffineIupac (AffineAlignment.cpp:110-252: two-state affine, float32) for n independent pairs per call,
 * bit-exact: scores, ties and the traceback come out as the reference's.  The DP runs on the device
 * (k_align_fill, one move byte per cell and no score matrix in memory; k_align_trace).  AlignLinear is not
 * provided; long near-identical pairs have the certified band below (pbccs_align_batch_ex), which
 * keeps these answers in memory linear in the band's width.  These calls are GLOBAL, as the reference's Align;
 * the ends-free modes (SEMIGLOBAL, LOCAL) of the int32 aligner live in pbccs_align_batch_ends further down
 * (k_align_fill_ends / k_align_trace_ends). */
#define PBCCS_ALIGN_NW 0
#define PBCCS_ALIGN_AFFINE 1
#define PBCCS_ALIGN_AFFINE_IUPAC 2

/* kind PBCCS_ALIGN_NW reads mode (PBCCS_POA_GLOBAL only: any other is the reference's UnsupportedFeatureError)
 * and the four ints (AlignParams: Match, Mismatch, Insert, Delete; AlignConfig.cpp's default 0, -1, -1, -1);
 * the affine kinds read the five floats (AffineAlignmentParams; defaults 0, -1, -1, -0.5 and PartialMatchScore
 * 0, IUPAC-aware -0.25). */
typedef struct {
    int kind, mode;
    int match, mismatch, insert, delete_;
    float match_score, mismatch_score, gap_open, gap_extend, partial_match_score;
} pbccs_align_params;

typedef struct {
    const char* target;   /* columns (j) */
    int target_len;
    const char* query;    /* rows (i) */
    int query_len;
} pbccs_align_pair;

typedef struct {
    char* transcript;   /* caller buffer of cap bytes (not NUL-terminated): M R I D, Gusfield's transcript */
    int cap;
    int len;            /* transcript length, never more than target_len + query_len */
    int score_i;        /* NW: Score(I, J) */
    float score_f;      /* affine: max(M, GAP)(I, J) */
    int status;         /* PBCCS_OK, or this pair's PBCCS_EINVAL / PBCCS_EOOM / PBCCS_ERANGE */
} pbccs_align_result;

/* Results in input order.  An empty target gives all I, an empty query all D (no launch).  PBCCS_EINVAL before
 * any device work: a mode other than GLOBAL, non-finite affine parameters, a negative length, a null sequence
 * with a positive length; per pair (status) and for the call: an NW pair whose (I + J) * max|param| does not fit
 * in int32, or a traceback that would leave the matrix (the reference reads outside its matrices there; only
 * with pathological parameters).  The pairs are split into launches whose move stores fit the align workspace
 * budget (PBCCS_ALIGN_WORKSPACE_MB, default 2048); a pair that alone exceeds it gets PBCCS_EOOM, as does the
 * call, with no device work for that pair.  A transcript longer than its buffer sets len and makes the call
 * return PBCCS_ERANGE after all outputs are written.  The call returns the first failing pair's status
 * (PBCCS_ERANGE last). */
int pbccs_align_batch(pbccs_engine* eng, const pbccs_align_params* params, const pbccs_align_pair* pairs, int n,
                      pbccs_align_result* out);

/* Align work since the last reset: pairs given, DP cells filled, k_align_fill launches, transcript characters
 * walked; fill / trace device ms (profiling on); bytes = move-store bytes the launches covered; groups = the
 * launch groups the workspace budget split the batches into. */
typedef struct {
    long long pairs, cells, launches, trace_steps;
    double fill_ms, trace_ms, bytes;
    long long groups;
} pbccs_align_stats;
int pbccs_align_stats_get(pbccs_engine* eng, pbccs_align_stats* out, int reset);

/* ---- Certified banded fill for the pairwise aligners --------------------------------
 * An opt-in for long, near-identical pairs; with band NULL or mode PBCCS_BAND_OFF every call is what it was.
 * A band of half-width w holds the diagonals min(0, J - I) - w <= j - i <= max(0, J - I) + w.  The banded fill
 * (k_align_fill_band) leaves move bytes only for its strips' column windows, about I (W + 64 R + 62) bytes for W
 * band diagonals where the full fill leaves I J.  Its final score S bounds how far an optimal path can stray: every
 * path that leaves the band scores at most U(w) (+ a rounding margin E for affine parameters that are not exact in
 * float32), so when S > U(w) + E the banded score and transcript are the full fill's, bit for bit (a numerically
 * zero affine score may differ in the sign of zero).  At most two banded fills per pair: the first at w (or the
 * automatic width, 32), the second at the smallest width the first score certifies.  A pair that cannot be
 * certified (Insert + Delete > max(Match, Mismatch); 2 max(GapOpen, GapExtend) > the largest diagonal score; sums
 * out of the dead-cell value's range), whose band would cover the whole matrix or whose banded store would be no
 * smaller than the full one, takes the full fill.  No banded answer is returned without its certificate. */
#define PBCCS_BAND_OFF 0
#define PBCCS_BAND_AUTO 1    /* first half-width chosen by the library */
#define PBCCS_BAND_WIDTH 2   /* first half-width = w */
typedef struct {
    int mode;
    int w;
} pbccs_align_band;

/* fallback reasons */
#define PBCCS_BAND_CERTIFIED 0
#define PBCCS_BAND_NOT_CERTIFIABLE 1
#define PBCCS_BAND_COVERS_MATRIX 2
#define PBCCS_BAND_STORE_NOT_SMALLER 3
#define PBCCS_BAND_TRACE_FLAGGED 4
#define PBCCS_BAND_UNCERTIFIED 5
#define PBCCS_BAND_DEGENERATE 6   /* an empty sequence: answered on the host */
#define PBCCS_BAND_OVER_BUDGET 7  /* the banded store alone exceeds the workspace; so does the full one (PBCCS_EOOM) */
typedef struct {
    int banded;     /* 1: a certified banded fill's answer; 0: the full fill's */
    int w;          /* the last half-width tried */
    int attempts;   /* banded fills of this pair: 0, 1 or 2 */
    int reason;     /* PBCCS_BAND_*: why the pair took the full fill */
} pbccs_align_band_info;

/* pbccs_align_batch with the band.  info: NULL, or n entries. */
int pbccs_align_batch_ex(pbccs_engine* eng, const pbccs_align_params* params, const pbccs_align_pair* pairs, int n,
                         pbccs_align_result* out, const pbccs_align_band* band, pbccs_align_band_info* info);

/* U(w), E and whether the parameters can be certified at all, for a pair of query_len rows and target_len columns:
 * host code, no engine.  *u is -infinity when no path can leave the band. */
int pbccs_align_band_bound(const pbccs_align_params* params, int query_len, int target_len, int w, double* u,
                           double* e, int* certifiable);
/* The smallest half-width whose certificate a banded score (a lower bound of the full score) satisfies; -1 in *w
 * when the pair cannot be certified.  Host code, no engine. */
int pbccs_align_band_widen(const pbccs_align_params* params, int query_len, int target_len, double score, int* w);

/* Banded work since the last reset: pairs given to banded calls, pairs answered banded, second attempts, fallbacks
 * by reason (index PBCCS_BAND_*), cells inside the bands filled and I x J of the same pairs, banded move-store
 * bytes, launches and groups, fill / trace device ms (profiling on). */
typedef struct {
    long long pairs, banded_pairs, second_attempts;
    long long fallbacks[8];
    long long band_cells, full_cells, launches, groups, trace_steps;
    double store_bytes, fill_ms, trace_ms;
} pbccs_align_band_stats;
int pbccs_align_band_stats_get(pbccs_engine* eng, pbccs_align_band_stats* out, int reset);

/* ---- Ends-free pairwise alignment: SEMIGLOBAL and LOCAL ------------------------------
 * The reference's Align stops at GLOBAL; these are the rules of its POA (PoaGraphImpl.cpp:178-352) on a graph that
 * holds the target as one unbranched path, with the int32 AlignParams.  Query on rows i, target on columns j.
 * S(0, j) = 0 (Start).  Column 0: SEMIGLOBAL S(i, 0) = i * Insert (Extra), LOCAL 0 (Start).  A cell tries, a later
 * candidate winning only when strictly greater: (LOCAL) Start 0, the diagonal (Match / Mismatch by raw byte
 * equality), Delete S(i, j-1) + Delete, Extra S(i-1, j) + Insert -- the POA's order, not Align's ArgMax3.  End cell:
 * SEMIGLOBAL the smallest j holding the maximum of row I; LOCAL the maximum over all cells, ties to the smallest
 * j, then the smallest i.  The walk goes back to the first Start cell; the transcript (M R for a diagonal step, D
 * Delete, I Extra) covers target[target_begin, target_end) and query[query_begin, query_end), and the score is the
 * end cell's.  SEMIGLOBAL always covers the whole query. */
typedef struct {
    int mode;           /* PBCCS_POA_SEMIGLOBAL or PBCCS_POA_LOCAL */
    int both_strands;   /* != 0: the query is also aligned reverse complemented (ComplementArray, as pbccs_map_batch);
                           forward wins iff its score >= the other's */
} pbccs_align_ends;

typedef struct {
    int target_begin, target_end;
    int query_begin, query_end;   /* in the coordinates of the sequence that was aligned (the reverse complement
                                     when rc), as pbccs_map_batch's read extent */
    int rc;
} pbccs_align_extent;

/* params->kind must be PBCCS_ALIGN_NW (the reference defines free ends for linear scores only; an affine kind is
 * PBCCS_EINVAL); params->mode is ignored in favour of ends->mode.  PBCCS_EINVAL before any device work as well: a
 * mode other than SEMIGLOBAL or LOCAL (GLOBAL is pbccs_align_batch's), Insert > 0 or Delete > 0 (a rewarding gap
 * next to a free end has no reading), a bad pair.  out[k].score_i is the score; out[k].transcript the transcript of
 * the two substrings ext[k] names.  An empty query gives score 0, an empty transcript and a zero extent; an empty
 * target gives all I with score I * Insert (SEMIGLOBAL) or the same empty answer (LOCAL); neither launches.  The
 * per-pair status, the int32 range rule, the workspace budget with its PBCCS_EOOM and the PBCCS_ERANGE contract
 * are pbccs_align_batch's, and the work adds to pbccs_align_stats. */
int pbccs_align_batch_ends(pbccs_engine* eng, const pbccs_align_params* params, const pbccs_align_ends* ends,
                           const pbccs_align_pair* pairs, int n, pbccs_align_result* out, pbccs_align_extent* ext);

/* ---- MapToDraft: placing reads on a finished draft ---------------------------------------------------
 * What SparsePoa::OrientAndAddRead(read, minScoreToAdd) followed by FindConsensus reports for a read on a graph
 * that holds only the draft as one unbranched path: a LOCAL alignment of the read, as given and reverse
 * complemented, against the linear draft with DefaultPoaConfig's scores (match 3, mismatch -5, insert -4,
 * delete -4), ties as the reference's (candidates Start, diagonal, Delete, Extra, a later one only when strictly
 * greater; the end cell is the smallest draft column, then the smallest read row, holding the maximum).  The DP
 * runs on the device (k_map_fill): every cell carries its start cell, no matrix, move or path reaches memory.
 * The reference has no such call (Consensus.h:102-103 leaves it a TODO); it is what lets a POA capped by
 * max_poa_coverage keep the reads past the cap (pbccs_ccs_batch_ex). */
typedef struct {
    const char* draft;
    int draft_len;
    const char* const* seqs;   /* n_reads reads; a NULL or zero-length read is never mapped */
    const int* lens;
    int n_reads;
} pbccs_map_input;

typedef struct {
    int* mapped;    /* n_reads: 1 mapped, 0 not (both orientations below min_score_to_add, or no read) */
    int* rc;        /* n_reads: PoaAlignmentSummary::ReverseComplementedRead */
    int* extents;   /* 4 * n_reads: ExtentOnRead begin/end (in the reverse complement's coordinates when rc),
                       ExtentOnConsensus begin/end; a best score of 0 gives 0 0 0 0 */
    int* score;     /* n_reads: the chosen orientation's score (the larger of the two when not mapped) */
} pbccs_map_output;

/* Orientation as SparsePoa.cpp:112-132: forward if c1 >= c2 && c1 >= min_score_to_add, else reverse if c2 >= c1
 * && c2 >= min_score_to_add, else not mapped.  Any output array may be NULL.  PBCCS_EINVAL before any device
 * work: an empty or NULL draft, a negative length, a NULL read with a positive length, a draft or read longer
 * than 65535 (a start cell is packed in 32 bits).  Reads taller than one strip of rows hand their boundary row
 * through a per-job buffer; the batch is split into launches whose buffers fit PBCCS_MAP_WORKSPACE_KB (default
 * 262144), and a read whose own buffers exceed it is left unmapped and makes the call return PBCCS_EOOM after
 * every other read was mapped, with no device work for that read. */
int pbccs_map_batch(pbccs_engine* eng, const pbccs_map_input* in, int n, float min_score_to_add,
                    pbccs_map_output* out);

/* Mapping work since the last reset: reads given, DP cells (2 (I + 1) J per read that reached the device),
 * k_map_fill launches, row strips run, device ms (profiling on). */
typedef struct {
    long long jobs, cells, launches, strips;
    double device_ms;
} pbccs_map_stats;
int pbccs_map_stats_get(pbccs_engine* eng, pbccs_map_stats* out, int reset);

/* pbccs_ccs_batch with options.  map_past_cap != 0: once max_poa_coverage reads were added and the draft taken
 * exactly as without it, every later read of FilterReads' order is placed on the draft with pbccs_map_batch's
 * aligner (min_score_to_add 0) and goes through ExtractMappedRead like a POA read; a read FilterReads dropped or
 * the mapping refused is a placeholder that counts in the drop fraction's denominator, as a read the POA
 * rejected does.  AddRead order stays FilterReads' order.  map_past_cap == 0, or a cap no read lies past, is
 * pbccs_ccs_batch. */
typedef struct {
    long long max_poa_coverage;   /* >= 1 */
    int map_past_cap;
} pbccs_ccs_options;
void pbccs_ccs_options_default(pbccs_ccs_options* o);   /* no cap, map_past_cap 0 */
int pbccs_ccs_batch_ex(pbccs_engine* eng, const pbccs_ccs_input* in, int n, const pbccs_ccs_options* ccs,
                       const pbccs_polish_options* opts, pbccs_ccs_output* out);

/* ---- SparseAlign: K-mer seeds, their chain, alignable ranges -------------------------------------------
 * PacBio::CCS::SparseAlign<K>(seq1, seq2) (include/pacbio/ccs/SparseAlignment.h:275-310, src/ChainSeeds.cpp with
 * matchReward 3) for n independent pairs per call, equal to the reference anchor for anchor: every K-mer of the
 * query that is not a homopolymer seeds (h, v) at each target position holding it; the chain is the reference's
 * sparse dynamic programme (visible-left, visible-above and column-set candidates, in that order of precedence,
 * a later one only when strictly greater; the first best end in (v, h) order).  target is seq1 (H), query seq2
 * (V).  All of it runs on the device (k_sparse_count / _index / _visible / _sweep / _ranges).
 * Defined here rather than copied: an empty query gives an empty chain (the reference dereferences it), a letter
 * outside upper-case ACGT is that pair's PBCCS_EINVAL (SeqAn would read it as some base), and K is a parameter,
 * 4 <= k <= 8 (the product uses 6, the reference's tests 5). */
typedef struct {
    const char* target;
    int target_len;
    const char* query;
    int query_len;
    int reverse_complement;   /* != 0: chain the query's reverse complement (formed on the device) */
    int* anchors;             /* 2 * anchor_cap ints: (h, v) per anchor, ascending in both.  A chain never has more
                                 than min(target_len, query_len) - k + 1 anchors */
    int anchor_cap;
    int* ranges;              /* NULL, or 2 * target_len ints: [begin, end) of the query rows alignable to each target
                                 position, as SdpRangeFinder::InitRangeFinder (RangeFinder.cpp:71-165, WIDTH 30)
                                 reports them for a graph holding only the target as one unbranched path; positions
                                 before the first or after the last anchor inherit the inverted interval of
                                 RangeUnion({}), and with no anchor at all every position is (query_len, 0) */
} pbccs_sparse_align_input;

typedef struct {
    int status;          /* PBCCS_OK, or this pair's PBCCS_EINVAL / PBCCS_EOOM / PBCCS_ERANGE */
    int n_anchors;       /* chain length; with PBCCS_ERANGE (anchor_cap too small) nothing was written */
    long long n_seeds;   /* seeds found (also for a pair over the cap) */
    long long score;     /* the chain's score, 0 for an empty chain */
} pbccs_sparse_align_output;

/* PBCCS_EINVAL before any device work: k outside 4..8, a negative length, a null sequence with a positive length.
 * Per pair: PBCCS_EINVAL for a letter outside ACGT or a sequence longer than 1048576; PBCCS_EOOM, known after
 * the counting pass and with no further device work for that pair, when it has more seeds than the cap
 * (PBCCS_SPARSE_MAX_SEEDS, default 4194304: a seed takes 24 bytes on the device) or its own arrays exceed half
 * the workspace budget (PBCCS_SPARSE_WORKSPACE_KB, default 1048576), into which the batch is split.  The other
 * pairs complete, the engine stays usable, and the call returns the first failing pair's status. */
int pbccs_sparse_align_batch(pbccs_engine* eng, int k, const pbccs_sparse_align_input* in, int n,
                             pbccs_sparse_align_output* out);

/* SparseAlign work since the last reset: pairs given, seeds found, anchors returned, kernel launches, device ms
 * (profiling on), and over the pairs that asked for ranges the cells inside them and the full
 * target_len * (query_len + 1) cells a POA column fill visits. */
typedef struct {
    long long jobs, seeds, anchors, launches;
    double device_ms;
    long long range_cells, full_cells;
} pbccs_sparse_align_stats;
int pbccs_sparse_align_stats_get(pbccs_engine* eng, pbccs_sparse_align_stats* out, int reset);

/* ---- Banded POA fill: reads aligned to the graph inside SdpRangeFinder's ranges ------------------------
 * An opt-in; with the switch off every call is what it was.  LOCAL alignments only.  Before
 * each TryAddRead of a graph that holds a read: the consensus path (ConsensusPath(LOCAL, -INT_MAX)) and its
 * sequence; anchors = SparseAlign<6>(css, read) on the device; per vertex the range [B, E) of
 * SdpRangeFinder::InitRangeFinder (RangeFinder.cpp:71-165, WIDTH 30) on the branching graph.  A column holds the
 * rows B <= i <= min(E, I); a cell outside its column's band does not exist and offers no candidate, every
 * existing cell keeps LOCAL's Start, candidate order and the strict '>' are those of the full fill, and the exit
 * takes the first maximal existing row of the best column (ties to the lower vertex id).  An alignment without
 * anchors (which includes a read or consensus shorter than 6), with a letter outside ACGT, or whose seeding ran
 * out of memory takes the full fill and is counted as a fallback; its other orientation and the other ZMWs stay
 * banded. */
typedef struct {
    long long max_coverage;   /* >= 1 */
    int min_coverage;         /* as pbccs_poa_batch */
    int banded;
} pbccs_poa_options;
void pbccs_poa_options_default(pbccs_poa_options* o);   /* no cap, min_coverage -1, banded 0 */
/* pbccs_poa_batch with options; opts NULL is the defaults, banded 0 is pbccs_poa_batch */
int pbccs_poa_batch_ex(pbccs_engine* eng, const pbccs_poa_input* in, int n, const pbccs_poa_options* opts,
                       pbccs_poa_output* out);
/* pbccs_sparse_poa_orient_and_add_read of this handle fills banded from now on (on != 0) */
int pbccs_sparse_poa_set_banded(pbccs_sparse_poa* p, int on);

/* What the range finder sees for one read (rc != 0: its reverse complement) against the handle's current graph,
 * which must hold a read: the consensus path as vertex ids (css_path, css_cap ints, *css_len), the anchors as
 * (consensus position, read position) pairs (anchors, 2 * anchor_cap ints, *n_anchors) and [B, E) per vertex id
 * (ranges, 2 * range_cap ints, *n_vertices; $ = vertex 1 has no column and reads (0, 0)).  *fallback != 0: the
 * alignment would take the full fill (no anchors, a foreign letter, seeding out of memory); anchors and ranges
 * are then not written and their counts are 0.  PBCCS_ERANGE when a buffer is too small, counts set. */
int pbccs_sparse_poa_alignable_ranges(pbccs_sparse_poa* p, const char* seq, int len, int rc, int* css_path,
                                      int css_cap, int* css_len, int* anchors, int anchor_cap, int* n_anchors,
                                      int* ranges, int range_cap, int* n_vertices, int* fallback);

/* Moves of a traceback step (PoaGraphImpl.hpp:45-55) */
#define PBCCS_POA_MOVE_START 1
#define PBCCS_POA_MOVE_END 2
#define PBCCS_POA_MOVE_MATCH 3
#define PBCCS_POA_MOVE_MISMATCH 4
#define PBCCS_POA_MOVE_DELETE 5
#define PBCCS_POA_MOVE_EXTRA 6
/* TryAddRead without the commit: the exit score of the read (rc != 0: of its reverse complement) against the
 * handle's current graph, which must hold a read, and the traceback in the device's order -- steps[3 k] the
 * vertex, steps[3 k + 1] the move that reached the visited cell, steps[3 k + 2] the cell's row; step 0 is the End
 * move into $ (vertex 1, row len), the last step the Start move.  banded != 0 fills inside the ranges (or takes the full fill where the rules above
 * send the alignment back).  PBCCS_ERANGE when cap (in steps) is too small, *n_steps set. */
int pbccs_sparse_poa_try_add_read(pbccs_sparse_poa* p, const char* seq, int len, int rc, int banded, float* score,
                                  int* steps, int cap, int* n_steps);

/* pbccs_ccs_batch_ex with the POA's options: poa NULL or poa->banded 0 is pbccs_ccs_batch_ex.  Only poa->banded
 * is read: the coverage cap comes from ccs, the draft's min_coverage is Consensus.h's rule. */
int pbccs_ccs_batch_ex2(pbccs_engine* eng, const pbccs_ccs_input* in, int n, const pbccs_ccs_options* ccs,
                        const pbccs_poa_options* poa, const pbccs_polish_options* opts, pbccs_ccs_output* out);

/* Banded-fill work since the last reset: alignments filled banded, alignments that fell back to the full fill,
 * the cells inside the bands and the full cols x (I + 1) of the same alignments, seeds and anchors of the
 * seeding, device ms by phase (profiling on) and the score bytes the banded fills wrote. */
typedef struct {
    long long banded_alignments, fallbacks, band_cells, full_cells, seeds, anchors;
    double seed_ms, ranges_ms, fill_ms, trace_ms, score_bytes;
} pbccs_poa_band_stats;
int pbccs_poa_band_stats_get(pbccs_engine* eng, pbccs_poa_band_stats* out, int reset);

/* ---- Windowed polish: a long draft polished as overlapping windows and stitched ------------------------
 * An opt-in with no counterpart in the reference (DESIGN.md §3.18 states the rules).  A draft longer than
 * window + overlap is cut into n = ceil((L - overlap) / window) windows of step S = ceil((L - overlap) / n),
 * window i = [i S, min(L, i S + S + overlap)).  Every read is cut at the window boundaries through its
 * SparseAlign<k> chain against the draft (on the device; only the cuts come back), each window is polished as an
 * ordinary ZMW by pbccs_polish_batch with the caller's settings, and neighbouring windows are joined at a draft
 * position of their overlap around which both windows' Align transcripts (window draft -> window consensus,
 * GLOBAL, 0 -1 -1 -1) hold 2 guard neighbouring M.  A ZMW with a window that is not PBCCS_ZMW_SUCCESS, without a
 * join, or whose stitched predicted accuracy misses min_predicted_accuracy is polished whole instead, and its
 * record is the whole-template route's. */
typedef struct {
    int window;    /* W (2000) */
    int overlap;   /* V (200) */
    int guard;     /* g (8) */
    int k;         /* the seeds' K (6) */
} pbccs_window_options;
void pbccs_window_options_default(pbccs_window_options* o);
/* valid: window > overlap, overlap >= 2 guard, guard >= 1, 4 <= k <= 8; anything else is PBCCS_EINVAL before any
 * device work in every call below */

#define PBCCS_WINDOW_FALLBACK_NONE 0
#define PBCCS_WINDOW_FALLBACK_WINDOW 1     /* a window's status was not PBCCS_ZMW_SUCCESS */
#define PBCCS_WINDOW_FALLBACK_NO_JOIN 2    /* two neighbouring windows have no join, or the joins cross */
#define PBCCS_WINDOW_FALLBACK_ACCURACY 3   /* the stitched predicted accuracy is below min_predicted_accuracy */

/* Host only.  bounds receives 2 * *n_windows ints (begin, end); PBCCS_ERANGE when cap (in windows) is too small,
 * *n_windows set (bounds may be NULL with cap 0 to size the call). */
int pbccs_window_plan(int draft_len, const pbccs_window_options* w, int* bounds, int cap, int* n_windows);

/* Host only: the join rule on two transcripts (M R I D; target = the window's draft, query = its consensus) of
 * the windows [begin_a, end_a) and [begin_b, end_b), begin_a < begin_b.  Candidates p in [begin_b + guard,
 * end_a - guard] in the order mid, mid + 1, mid - 1, ... with mid = (begin_b + end_a) / 2; the first p whose draft
 * columns p - guard .. p + guard - 1 are taken by 2 guard neighbouring M of both transcripts is the join:
 * *found = 1, *p, and *cut_a / *cut_b = TargetToQueryPositions(transcript)[p - begin].  PBCCS_EINVAL for a
 * transcript that does not span its window or holds another character. */
int pbccs_window_join(const char* transcript_a, int len_a, int begin_a, int end_a, const char* transcript_b,
                      int len_b, int begin_b, int end_b, int guard, int* found, int* p, int* cut_a, int* cut_b);

/* The reads' slices per window.  n_windows[z] windows per ZMW; slices holds, ZMW after ZMW, n_windows[z] *
 * n_reads ints[4] in (window, read) order: the slice [begin, end) in the read's forward text (its sequence for
 * strand 0, the reverse complement for strand 1) and the read's mapped extent [ts', te') in window coordinates,
 * or -1 -1 -1 -1 where the read is a placeholder in that window (no sequence, an empty chain, a slice or extent
 * shorter than min_length).  A ZMW with one window reports its reads as they are.  unanchored[z] (may be NULL):
 * reads with a sequence and no chain.  *n_ints = the ints needed; PBCCS_ERANGE when cap is smaller (slices may be
 * NULL with cap 0 to size the call; nothing runs on the device then). */
int pbccs_window_slices(pbccs_engine* eng, const pbccs_zmw_input* in, int n, const pbccs_window_options* w,
                        int min_length, int* n_windows, int* slices, long long cap, long long* n_ints,
                        int* unanchored);

typedef struct {
    int begin, end;          /* draft bounds */
    int join;                /* the draft position of the join with the next window; -1: none (the last window) */
    int cut_begin, cut_end;  /* the piece [cut_begin, cut_end) of the window's consensus in the stitched one */
    int status;              /* PBCCS_ZMW_* of the window */
    long long n_tested, n_applied;
} pbccs_window_record;

typedef struct {
    int n_windows;
    int fallback;            /* PBCCS_WINDOW_FALLBACK_* */
    int unanchored_reads;
    pbccs_window_record* windows;   /* caller buffer of windows_cap records (may be NULL); the first
                                       min(n_windows, windows_cap) are written */
    int windows_cap;
} pbccs_window_info;

/* pbccs_polish_batch with windows.  A ZMW with one window goes through the first pbccs_polish_batch call beside
 * the windows and its record is pbccs_polish_batch's; all fallbacks of the call share a second one.  The stitched
 * record: consensus and qvs are the pieces; predicted_accuracy as Consensus.h:508-512 over the stitched QVs;
 * n_tested / n_applied the sums over the windows (mutations of an overlap count in both windows);
 * add_read_results[r] the first code other than SUCCESS among the windows the read takes part in, in window
 * order, else SUCCESS (-1 when it takes part in none); zscores[r] the minimum over its windows (NaN in none); za
 * the mean of the SUCCESS reads' zscores; zg the minimum of the windows' zg; n_passes and status_counts from the
 * per-read codes.  info (may be NULL): n entries. */
int pbccs_polish_windowed(pbccs_engine* eng, const pbccs_zmw_input* in, int n, const pbccs_polish_options* opts,
                          const pbccs_window_options* w, pbccs_zmw_output* out, pbccs_window_info* info);

/* pbccs_ccs_batch_ex2 whose polish is pbccs_polish_windowed: win NULL is pbccs_ccs_batch_ex2.  With windows every
 * chunk is drafted first and the chunks are then polished one after another.  info (may be NULL): n entries,
 * written for the ZMWs that reach the polish (n_windows 0 otherwise). */
int pbccs_ccs_batch_ex3(pbccs_engine* eng, const pbccs_ccs_input* in, int n, const pbccs_ccs_options* ccs,
                        const pbccs_poa_options* poa, const pbccs_window_options* win,
                        const pbccs_polish_options* opts, pbccs_ccs_output* out, pbccs_window_info* info);

/* Windowed-polish work since the last reset: multi-window ZMWs, their windows, fallbacks by reason, reads without
 * a chain, kernel launches, and host wall time by phase (seeds and cuts, the windows' polish, align and join, the
 * fallbacks' polish). */
typedef struct {
    long long zmws, windows, fallbacks[4], unanchored_reads, cut_tasks, joints, launches;
    double slices_ms, polish_ms, join_ms, fallback_ms;
} pbccs_window_stats;
int pbccs_window_stats_get(pbccs_engine* eng, pbccs_window_stats* out, int reset);

/* ---- per-base rich QVs --------------------------------------------------------------
 * ConsensusQVs folds the scores of a position's unique single-base mutations into one QV.  The rich QVs are the
 * same sum taken apart by mutation type: sub_qv / ins_qv / del_qv = ProbabilityToQV(1 - 1 / (1 + S)) with S the
 * sum of e^score over the position's substitutions / insertions / deletion with a score below 0, in enumeration
 * order (raw and unclipped, as qvs; an empty sum gives the value it gives there), and sub_tag / ins_tag = the base
 * of the best-scoring substitution / insertion (scores >= 0 included, the first in enumeration order on a tie;
 * 'N' only where none was enumerated).  The qvs returned beside them are pbccs_consensus_qvs', bit for bit.
 * Names follow the mutation type; file formats name by error type, the inverse: PacBio's DeletionQV / DeletionTag
 * (dq / dt: a base is missing before this one) are ins_qv / ins_tag, InsertionQV (iq: this base is spurious) is
 * del_qv, sq / st are sub_qv / sub_tag.
 * All five are caller buffers of cap entries (the tags are not NUL-terminated); len = the entries written, 0 for a
 * ZMW that ends neither SUCCESS nor POOR_QUALITY, -required when cap is too small (nothing is written then). */
typedef struct {
    int* sub_qv;
    int* ins_qv;
    int* del_qv;
    char* sub_tag;
    char* ins_tag;
    int cap;
    int len;
} pbccs_rich_qvs;

/* pbccs_consensus_qvs / pbccs_quiver_consensus_qvs with the rich QVs: the same sweep, then k_qv_rich / k_qqv_rich.
 * qvs has rich->cap entries; *n = the template length; PBCCS_ERANGE (and rich->len = -required) when cap is
 * smaller. */
int pbccs_consensus_qvs_rich(pbccs_scorer* s, int* qvs, pbccs_rich_qvs* rich, int* n);
int pbccs_quiver_consensus_qvs_rich(pbccs_quiver_scorer* s, int* qvs, pbccs_rich_qvs* rich, int* n);

/* What the batched calls take beyond their first form, one struct per family of calls; every member may be NULL,
 * and with all of them NULL each call is exactly the call it extends. */
typedef struct {
    const pbccs_repeat_options* repeats;   /* pbccs_polish_batch_ex's (not used by the windowed calls) */
    long long* repeat_tested;              /* n entries */
    long long* repeat_applied;
    pbccs_rich_qvs* rich;                  /* n entries, one per ZMW */
} pbccs_polish_extras;

/* pbccs_polish_batch_ex with extras. */
int pbccs_polish_batch_ex2(pbccs_engine* eng, const pbccs_zmw_input* in, int n, const pbccs_polish_options* opts,
                           const pbccs_polish_extras* extras, pbccs_zmw_output* out);
/* pbccs_quiver_polish_batch_ex with extras. */
int pbccs_quiver_polish_batch_ex2(pbccs_engine* eng, const pbccs_quiver_config* configs,
                                  const char* const* chemistries, int n_configs, const pbccs_quiver_zmw* zmws, int n,
                                  const pbccs_refine_options* opts, const pbccs_polish_extras* extras,
                                  pbccs_quiver_result* out);
/* pbccs_polish_windowed with extras: the stitched rich arrays are the pieces [cut_begin, cut_end) of the windows'
 * arrays, as the stitched qvs are; a fallback ZMW gets its whole-draft route's. */
int pbccs_polish_windowed_ex(pbccs_engine* eng, const pbccs_zmw_input* in, int n, const pbccs_polish_options* opts,
                             const pbccs_window_options* w, const pbccs_polish_extras* extras, pbccs_zmw_output* out,
                             pbccs_window_info* info);
/* pbccs_ccs_batch_ex3 with extras. */
int pbccs_ccs_batch_ex4(pbccs_engine* eng, const pbccs_ccs_input* in, int n, const pbccs_ccs_options* ccs,
                        const pbccs_poa_options* poa, const pbccs_window_options* win,
                        const pbccs_polish_options* opts, const pbccs_polish_extras* extras, pbccs_ccs_output* out,
                        pbccs_window_info* info);

/* ---- directional consensus: strand-discordance screen and per-strand polish -----------
 * Rules of this project's own: the reference declares ConsensusSettings::Directional and stops at a TODO
 * (include/pacbio/ccs/Consensus.h:94-109).  For a single-base mutation m of the final template, sum_fwd / sum_rev
 * are the sums of Scores(m, 0) over the active forward / reverse reads that score m, in AddRead order (plain FP64
 * adds, no fast-score break), and n_fwd / n_rev count those reads.  m qualifies when n_fwd >= min_reads, n_rev >=
 * min_reads and one sum lies above min_score while the other lies below -min_score (a NaN sum never qualifies).  A
 * template position is a discordant site when one of its unique single-base mutations qualifies; it reports the
 * qualifying mutation with the largest min(|sum_fwd|, |sum_rev|), the first in enumeration order on a tie.
 * min_score defaults to 12.5, the magnitude of the reference's FastScoreThreshold, and min_reads to 2. */
typedef struct {
    double min_score;
    int min_reads;
    int min_sites;     /* directional == 1: a ZMW is split when it has at least this many sites (default 1) */
    int directional;   /* 0: the screen only, 1: split the discordant ZMWs, 2: split every ZMW */
} pbccs_strand_options;
void pbccs_strand_options_default(pbccs_strand_options* o);

/* One per ZMW.  The five site arrays are caller buffers of cap entries (type: PBCCS_INSERTION / DELETION /
 * SUBSTITUTION; base '-' for a deletion); n_sites = the sites written, in template order, 0 for a ZMW that ends
 * neither SUCCESS nor POOR_QUALITY, -required when cap is too small (nothing is written then and the call returns
 * PBCCS_ERANGE after all outputs are written).  split: the ZMW was polished once more per strand; fwd / rev
 * (caller buffers as any pbccs_zmw_output; add_read_results and zscores sized by the ZMW's n_reads) then hold what
 * pbccs_polish_batch_ex2 returns for a ZMW of the same draft and SNR with only the strand-0 / strand-1 reads, in
 * their original order and windows, both in the draft's orientation; per-read entries are indexed like the joint
 * record's, -1 / NaN for the other strand's reads.  Not split: fwd and rev are left untouched. */
typedef struct {
    int n_sites;
    int cap;
    int* position;
    int* type;
    char* base;
    double* sum_fwd;
    double* sum_rev;
    int split;
    pbccs_zmw_output fwd, rev;
} pbccs_strand_result;

/* pbccs_polish_batch_ex2 with the strand screen: out is exactly pbccs_polish_batch_ex2's (the joint record is
 * always produced), strand_out[i] the sites of ZMW i's final template (k_strand_sums and k_strand_sites beside the
 * QV kernel, on the ConsensusQVs sweep's deltas) and, by strand->directional, its two per-strand records: the
 * split ZMWs' single-strand inputs go through the same batch path and options (gates and repeats included; the
 * rich QVs are the joint record's only) together.  strand NULL is the defaults.  pbccs_polish_extras keeps its
 * layout: a caller built against the four-member struct stays valid, so the strand members travel beside it. */
int pbccs_polish_batch_strand(pbccs_engine* eng, const pbccs_zmw_input* in, int n, const pbccs_polish_options* opts,
                              const pbccs_polish_extras* extras, const pbccs_strand_options* strand,
                              pbccs_strand_result* strand_out, pbccs_zmw_output* out);

/* pbccs_ccs_batch_ex4 (without windows: the windowed polish does not run the screen) with the strand screen, as
 * pbccs_polish_batch_strand adds it to pbccs_polish_batch_ex2: the screen runs in each chunk's polish, the split
 * ZMWs of all chunks are polished per strand together afterwards.  The per-read arrays of fwd / rev hold n_subreads
 * entries indexed by the caller's subreads, like the joint record's. */
int pbccs_ccs_batch_strand(pbccs_engine* eng, const pbccs_ccs_input* in, int n, const pbccs_ccs_options* ccs,
                           const pbccs_poa_options* poa, const pbccs_polish_options* opts,
                           const pbccs_polish_extras* extras, const pbccs_strand_options* strand,
                           pbccs_strand_result* strand_out, pbccs_ccs_output* out);

/* The per-strand sums of n single-base mutations of the scorer's current template: one scoring round without a
 * fast-score break, then k_strand_sums.  Bit-equal to summing pbccs_scorer_scores(m, 0) per strand in read order. */
int pbccs_scorer_strand_scores(pbccs_scorer* s, const pbccs_mutation* m, int n, double* sum_fwd, double* sum_rev,
                               int* n_fwd, int* n_rev);
/* The discordant sites of the scorer's current template (the full unique-mutation sweep, as pbccs_consensus_qvs
 * runs it).  *n = the sites; PBCCS_ERANGE when it exceeds cap (nothing is written).  opts NULL is the defaults;
 * min_sites and directional are not used. */
int pbccs_scorer_strand_sites(pbccs_scorer* s, const pbccs_strand_options* opts, int* position, int* type, char* base,
                              double* sum_fwd, double* sum_rev, int cap, int* n);

/* The screen's work since the last reset: ZMWs screened by the batch call, sites they reported, ZMWs split. */
typedef struct {
    long long strand_screened, strand_sites, strand_split;
} pbccs_strand_stats;
int pbccs_strand_stats_get(pbccs_engine* eng, pbccs_strand_stats* out, int reset);

/* ---- consensus kinetics: per-strand mean IPD and pulse width -------------------------
 * An opt-in with no counterpart in the reference (2015 pbccs has no kinetics); csrc/kinetics_kernels.hpp states
 * the rules.  Frames are unsigned 16-bit counts.  A read placed on the consensus [tb, te) with its oriented
 * positions from rb on contributes, for every M or R column of its transcript (target = consensus, query =
 * oriented read), its frames at original index q (rc == 0) or len - 1 - q (rc != 0); I columns contribute
 * nothing, D columns leave the position without this read.  Per strand (rc == 0 forward, rc != 0 reverse),
 * position and track: coverage n, integer sum S, mean (2 S + n) / (2 n) in integer division (0 where n == 0,
 * at most 65535) and the mean's CodecV1 code.  Forward arrays are indexed by consensus position; entry k of a
 * reverse array belongs to consensus position consensus_len - 1 - k. */
#define PBCCS_KIN_USED 0
#define PBCCS_KIN_UNMAPPED 1       /* MapToDraft did not place the read (or there is no read) */
#define PBCCS_KIN_EMPTY_EXTENT 2   /* no consensus position or no read position inside the extents */
#define PBCCS_KIN_ALIGN_FAILED 3   /* the read's alignment did not return PBCCS_OK */

typedef struct {
    const char* transcript;     /* M R I D */
    int transcript_len;
    int rc, rb, tb, te;
    int len;                    /* the read's length I */
    const unsigned short* ip;   /* len frames, or NULL: the read has no such track */
    const unsigned short* pw;
} pbccs_kinetics_read;

typedef struct {
    int consensus_len;
    int n_reads;
    const pbccs_kinetics_read* reads;
} pbccs_kinetics_pileup_input;

/* Index 2 * strand + track: forward ipd, forward pw, reverse ipd, reverse pw; consensus_len entries each.  Every
 * pointer may be NULL.  A read without a track is not counted in that track's coverage, hence one coverage per
 * track.  n_contributed: fn, rn -- the strand's reads with at least one M or R column and at least one track. */
typedef struct {
    unsigned short* mean[4];
    unsigned char* code[4];
    int* coverage[4];
    int n_contributed[2];
    int* read_status;   /* n_reads PBCCS_KIN_* */
} pbccs_kinetics_output;

/* k_kin_columns and k_kin_reduce only, on the caller's transcripts.  PBCCS_EINVAL before any device work: a
 * negative length, a character other than M R I D, a transcript whose target columns are not te - tb or whose
 * query columns run past len - rb, extents outside [0, consensus_len].  A read with te == tb or without a query
 * column is skipped as PBCCS_KIN_EMPTY_EXTENT. */
int pbccs_kinetics_pileup(pbccs_engine* eng, const pbccs_kinetics_pileup_input* in, int n, pbccs_kinetics_output* out);

typedef struct {
    const char* consensus;
    int consensus_len;
    int n_reads;
    const char* const* seqs;              /* a NULL or zero-length read is PBCCS_KIN_UNMAPPED */
    const int* lens;
    const unsigned short* const* ip;      /* NULL, or n_reads pointers: lens[r] frames each, NULL for no track */
    const unsigned short* const* pw;
} pbccs_kinetics_input;

typedef struct {
    pbccs_align_band band;   /* passed to the aligner; PBCCS_BAND_OFF by default */
} pbccs_kinetics_options;
void pbccs_kinetics_options_default(pbccs_kinetics_options* o);

/* Per read: pbccs_map_batch's placement on the consensus (min_score_to_add 0), then Align (NW, 0 -1 -1 -1) of
 * consensus[tb, te) and the oriented read's [rb, re), then the pileup, in one native call; the transcripts pass
 * through host memory between the aligner and the pileup.  opts NULL is the defaults.  A read that is not mapped,
 * whose extent is empty or whose alignment fails is skipped with its status and does not fail the call.
 * PBCCS_EINVAL before any device work: an empty consensus, a negative length, a NULL read with a positive length,
 * a consensus or read longer than 65535, an unknown band mode. */
int pbccs_kinetics_batch(pbccs_engine* eng, const pbccs_kinetics_input* in, int n, const pbccs_kinetics_options* opts,
                         pbccs_kinetics_output* out);

/* Kinetics work since the last reset: reads given, reads skipped by reason, transcript columns walked, (ZMW,
 * strand, position) threads of the reduction, kernel launches, device ms per kernel (profiling on). */
typedef struct {
    long long reads, skipped_unmapped, skipped_empty_extent, skipped_align_failed, columns, positions, launches;
    double columns_ms, reduce_ms;
} pbccs_kinetics_stats;
int pbccs_kinetics_stats_get(pbccs_engine* eng, pbccs_kinetics_stats* out, int reset);

/* ---- subread pileup on the consensus: base counts, ec, gapped rows --------------------
 * An opt-in with no counterpart in the reference; csrc/pileup_kernels.hpp states the rules.  Reads are placed and
 * vetted as the kinetics calls place and vet them, with the same PBCCS_KIN_* statuses; only PBCCS_KIN_USED reads
 * count.  Every array is indexed by consensus position, or by slot (slot s lies before position s, slot
 * consensus_len after the last one), in the consensus's own direction for both strands -- unlike the kinetics
 * arrays.  Strand 0 holds the rc == 0 reads, strand 1 the rc != 0 reads; codes are A C G T gap other = 0..5, a
 * read character outside ACGT being "other" in either orientation (its complement is N). */
typedef struct {
    const char* transcript;   /* M R I D */
    int transcript_len;
    int rc, rb, tb, te;
    const char* seq;          /* the read as sequenced, len characters */
    int len;
} pbccs_pileup_read;

typedef struct {
    const char* consensus;
    int consensus_len;
    int n_reads;
    const pbccs_pileup_read* reads;
} pbccs_pileup_columns_input;

/* Every pointer may be NULL.  With L = consensus_len: counts [2][L][6]; ins_reads, ins_bases [2][L + 1] (reads
 * with an insertion at the slot, and their inserted bases); slot_cov, max_ins, ins_plurality [L + 1]; cov,
 * plurality [L] (the code with the largest count of both strands among A C G T gap, a tie going to the
 * consensus's own base, else to the lowest code; 255 without coverage); ins_plurality[s] = 2 * inserting reads >
 * slot_cov[s].  Per read (n_reads entries each): the status, the transcript's column counts (0 for a read that is
 * not used) and the placement; re = rb + the read columns of the transcript.  transcripts / transcript_lens are
 * written by pbccs_pileup_batch only: n_reads pointers, each NULL or a buffer of consensus_len + lens[r] bytes
 * that receives the read's transcript (no terminator), and its length (0 for a read that is not used). */
typedef struct {
    int* counts;
    int* ins_reads;
    int* ins_bases;
    int* slot_cov;
    int* max_ins;
    int* cov;
    unsigned char* plurality;
    unsigned char* ins_plurality;
    int* read_status;
    int* n_match;
    int* n_mismatch;
    int* n_ins;
    int* n_del;
    int* rc;
    int* rb;
    int* re;
    int* tb;
    int* te;
    char* const* transcripts;
    int* transcript_lens;
    long long cov_sum;   /* the sum of cov; ec = cov_sum / consensus_len */
    int n_used[2];
} pbccs_pileup_output;

/* k_pile_columns and k_pile_reduce on the caller's transcripts.  Refuses, with PBCCS_EINVAL before any device
 * work, what pbccs_kinetics_pileup refuses. */
int pbccs_pileup_columns(pbccs_engine* eng, const pbccs_pileup_columns_input* in, int n, pbccs_pileup_output* out);

typedef struct {
    const char* consensus;
    int consensus_len;
    int n_reads;
    const char* const* seqs;              /* a NULL or zero-length read is PBCCS_KIN_UNMAPPED */
    const int* lens;
    const unsigned short* const* ip;      /* read only with `kinetics`: as pbccs_kinetics_input's */
    const unsigned short* const* pw;
    pbccs_kinetics_output* kinetics;      /* NULL, or where this ZMW's consensus kinetics go: the placement and
                                             alignment stage then runs once for both features */
} pbccs_pileup_input;

typedef struct {
    pbccs_align_band band;   /* passed to the aligner; PBCCS_BAND_OFF by default */
} pbccs_pileup_options;
void pbccs_pileup_options_default(pbccs_pileup_options* o);

/* pbccs_kinetics_batch's placement and alignment stage (the same band option, the same refusals), then the pileup;
 * also the kinetics of the ZMWs whose input names a kinetics output. */
int pbccs_pileup_batch(pbccs_engine* eng, const pbccs_pileup_input* in, int n, const pbccs_pileup_options* opts,
                       pbccs_pileup_output* out);

/* The gapped rows on the caller's transcripts (k_pile_scan, k_pile_rows).  widths[z] receives the row width, L + the
 * sum of max_ins; cols (NULL, or n pointers, each NULL or L ints) receives col[p], the cell of position p.  rows
 * NULL: the widths (and cols) only, to size the buffers.  Otherwise rows holds n pointers, each NULL or n_reads *
 * widths[z] bytes, with widths[z] on entry the width the buffer was sized for (PBCCS_EINVAL when it is not this
 * call's): one row per read in input order, blank for a read that is not used. */
int pbccs_pileup_msa(pbccs_engine* eng, const pbccs_pileup_columns_input* in, int n, int* widths, int* const* cols,
                     char* const* rows);

/* Pileup work since the last reset: reads given, reads skipped by reason, transcript columns walked, (ZMW, slot)
 * threads of the reduction, kernel launches, reads sent through pbccs_pileup_batch's placement and alignment
 * stage and how many of those also fed a kinetics output, device ms per kernel (profiling on). */
typedef struct {
    long long reads, skipped_unmapped, skipped_empty_extent, skipped_align_failed, columns, slots, launches;
    long long placed, shared;
    double columns_ms, reduce_ms, scan_ms, rows_ms;
} pbccs_pileup_stats;
int pbccs_pileup_stats_get(pbccs_engine* eng, pbccs_pileup_stats* out, int reset);

/* ---- split mapping: a read fused across a missed adapter, placed on the draft as a chain of segments -----------
 * The read as given is on the rows for both orientations; orientation 0 has the draft on the columns, orientation
 * 1 its reverse complement (N <-> M as pbccs_map_batch's complement).  With pbccs_map_batch's scores and candidate
 * order, every cell of row i has Start value G(i - 1), where G(0) = 0 and G(i) = max(G(i - 1), R(i).score -
 * jump_penalty), R(i) being row i's best cell over both orientations (the larger score, then orientation 0, then
 * the smaller column).  The chain ends at the first row with the largest R(i).score, which is the chain score; it
 * is walked back through the cells' start cells into segments (DESIGN.md §3.25 has the full rule).  The DP runs on
 * the device (k_split_fill, k_split_chain); one record per read row reaches device memory and only the segments
 * return.  The reference has no such step. */
#define PBCCS_SPLIT_JUMP_PENALTY 150   /* twice the measured null of unrelated sequence, DESIGN.md §3.25 */
#define PBCCS_SPLIT_MAX_SEGMENTS 8     /* the default; at most 64 */

typedef struct {
    int* n_segments;   /* n_reads: the chain's segment count; 0: not mapped (no read, or a chain score of 0) */
    int* truncated;    /* n_reads: 1 when the chain has more than max_segments segments */
    int* score;        /* n_reads: the chain score = sum of the segments' own scores - jump_penalty * (count - 1) */
    int* segments;     /* n_reads * max_segments * 6: per segment rc, extent on the read as given [begin, end),
                          extent on the draft [begin, end), own score; the chain's last min(count, max_segments)
                          segments in read order, the rest zero */
} pbccs_split_map_output;

/* jump_penalty < 0 is PBCCS_SPLIT_JUMP_PENALTY; max_segments <= 0 is PBCCS_SPLIT_MAX_SEGMENTS.  Any output array
 * may be NULL.  PBCCS_EINVAL before any device work as pbccs_map_batch, and for max_segments above 64.  The row
 * records (20 bytes per read row) and, for a draft wider than the widest register tile (512 columns), the per-read
 * row buffer (16 bytes per column) live in a workspace; the batch is split into launches that fit
 * PBCCS_SPLIT_WORKSPACE_KB (default 262144), and a read whose own buffers exceed it is left unmapped and makes the
 * call return PBCCS_EOOM after every other read was mapped, with no device work for that read. */
int pbccs_split_map_batch(pbccs_engine* eng, const pbccs_map_input* in, int n, int jump_penalty, int max_segments,
                          pbccs_split_map_output* out);

/* Split-mapping work since the last reset: reads given, DP cells (2 I J per read that reached the device), kernel
 * launches, reads that ran on the row-buffer path, device ms (profiling on). */
typedef struct {
    long long jobs, cells, launches, tiled;
    double device_ms;
} pbccs_split_map_stats;
int pbccs_split_map_stats_get(pbccs_engine* eng, pbccs_split_map_stats* out, int reset);

/* pbccs_ccs_batch that recovers missed-adapter reads.  Once a ZMW's draft exists, every subread FilterReads dropped
 * (at least twice the median full-pass length) whose placeholder the polish input would hold is split-mapped onto
 * the draft (pbccs_split_map_batch's rule, one call per POA chunk).  It is accepted as a missed-adapter read when
 * the chain is not truncated, has at least two segments, consecutive segments alternate orientation, and at least
 * two segments reach min_length read bases.  Each such segment becomes a polish read -- the read's bases [begin,
 * end) as given, in the read's own coordinates, on the segment's strand and draft extent -- and together they
 * replace the one placeholder in place, so they reach AddRead last, in read order.  Interior segments are full
 * passes; the first needs the read's ADAPTER_BEFORE, the last its ADAPTER_AFTER.  A read that is not accepted, or
 * that the mapper cannot take (longer than 65535, or a draft that long), stays the placeholder it is. */
typedef struct {
    int jump_penalty;   /* < 0: PBCCS_SPLIT_JUMP_PENALTY */
    int max_segments;   /* <= 0: PBCCS_SPLIT_MAX_SEGMENTS; at most 64 */
} pbccs_split_options;
void pbccs_split_options_default(pbccs_split_options* o);

typedef struct {
    int cap;                  /* in: segments the arrays below hold; add_order holds n_subreads + cap entries */
    int n_reads;              /* out: subreads accepted as missed-adapter reads */
    int n_segments;           /* out: their segments that became polish reads, in AddRead order */
    int n_missed_adapters;    /* out: sum over the accepted reads of chain segments - 1 */
    int n_added;              /* out: entries of add_order */
    int* subread;             /* per segment: the caller's subread index */
    int* segments;            /* per segment 6 ints: rc, read begin/end, draft begin/end, own score */
    unsigned char* full_pass; /* per segment */
    int* add_read_results;    /* per segment: as pbccs_zmw_output's */
    double* zscores;          /* per segment */
    int* add_order;           /* the ZMW's AddRead order in subread indices, a split subread once per added segment;
                                 pbccs_ccs_output's add_order holds its first n_subreads entries */
} pbccs_ccs_split_output;

/* As pbccs_ccs_batch_ex4 without windows (extras may carry rich, not repeats), plus the split step.  The
 * add_read_results / zscores of a split subread stay -1 / NaN in `out`; its segments' are in split_out.  PBCCS_ERANGE
 * after everything else was written when a ZMW has more segments than cap.  split NULL is the defaults. */
int pbccs_ccs_batch_split(pbccs_engine* eng, const pbccs_ccs_input* in, int n, const pbccs_ccs_options* ccs,
                          const pbccs_poa_options* poa, const pbccs_polish_options* opts,
                          const pbccs_polish_extras* extras, const pbccs_split_options* split,
                          pbccs_ccs_split_output* split_out, pbccs_ccs_output* out);

/* ---- barcode demultiplexing ---------------------------------------------------------------
 * Which barcode pair flanks a CCS read.  The reference has no demultiplexing; the rules are this project's own,
 * built from pbccs_align_batch_ends' SEMIGLOBAL rules, and tests/demux_restatement.py states them in full.
 *
 * W = window, or window_mult (<= 0: 3) times the longest barcode when window <= 0; 1 <= W <= 1024.  A read of
 * length n has the leading window [0, min(W, n)) and the trailing window [off, n), off = max(0, n - W).  lead[b] is
 * the SEMIGLOBAL score of barcode b (the query) inside the leading window (the target), trail[b] that of its reverse
 * complement inside the trailing window; read bytes are raw, a byte that is not exactly a barcode's byte matches
 * nothing.  An empty (or NULL) read launches nothing and scores len(b) * Insert on both ends.  Per end, best is the
 * smallest index holding the maximum and second the maximum over every other index (INT_MIN with one barcode).
 * Asymmetric design: i = best of lead, j = best of trail, score = lead[i] + trail[j], score_lead = the smaller of the
 * two ends' best - second.  Symmetric design: i = j = the best of lead + trail, score and score_lead from that sum.
 * A lead with no second is INT_MAX.  quality = clamp(floor(100 * score / (Match * (len_i + len_j))), 0, 100); the
 * read is called iff quality >= min_quality and score_lead >= min_score_lead.  The extents are the target extents of
 * the two called barcodes' alignments in read coordinates, as pbccs_align_batch_ends reports them. */
#define PBCCS_DEMUX_MIN_QUALITY 74   /* the midpoint of the measured null (64) and planted (84) qualities, §3.27 */
#define PBCCS_DEMUX_MAX_BARCODES 65535
#define PBCCS_DEMUX_MAX_BARCODE_LEN 64
#define PBCCS_DEMUX_MAX_WINDOW 1024
#define PBCCS_DEMUX_ASYMMETRIC 0
#define PBCCS_DEMUX_SYMMETRIC 1

typedef struct {
    const char* const* seqs;   /* n barcodes, each 1..64 bases of uppercase ACGT */
    const int* lens;
    int n;                     /* 1..65535 */
} pbccs_demux_barcodes;

typedef struct {
    int match, mismatch, insert, delete_;   /* Match > 0, Insert <= 0, Delete <= 0 */
    int design;                             /* PBCCS_DEMUX_ASYMMETRIC / PBCCS_DEMUX_SYMMETRIC */
    int window;                             /* <= 0: window_mult times the longest barcode */
    int window_mult;                        /* <= 0: 3 */
    int min_quality;                        /* < 0: PBCCS_DEMUX_MIN_QUALITY */
    int min_score_lead;
} pbccs_demux_options;
/* (3, -5, -4, -4), asymmetric, window 0, window_mult 3, min_quality PBCCS_DEMUX_MIN_QUALITY, min_score_lead 0 */
void pbccs_demux_options_default(pbccs_demux_options* o);

typedef struct {
    const char* seq;   /* may be NULL when len is 0 */
    int len;
} pbccs_demux_read;

/* Every array may be NULL; each holds one entry per read unless it says otherwise. */
typedef struct {
    int* lead;          /* the called barcodes i and j; filled for an uncalled read too */
    int* trail;
    int* called;        /* 1 / 0; the reported pair of an uncalled read is (-1, -1) */
    int* score;
    int* score_lead;
    int* quality;
    int* extents;       /* 4 per read: leading begin, end, trailing begin, end, in read coordinates */
    int* clip;          /* 2 per read: leading end, trailing begin; (-1, -1) when they cross */
    int* overlap;       /* 1 when leading end > trailing begin (the windows overlapped on a short read) */
    int* best;          /* 6 per read: leading best score, its index, second; the same for the trailing end */
    int* scores;        /* n * 2 * B: the full score matrix, [read][end][barcode] */
} pbccs_demux_output;

/* PBCCS_EINVAL before any device work: a bad barcode set (count, length, a byte that is not A C G T), Match <= 0,
 * Insert > 0, Delete > 0, an unknown design, W outside 1..1024, a negative read length, a NULL read with a positive
 * length, or scores that could leave int32: 2 * (longest barcode + W) * the largest |score| above INT_MAX
 * (pbccs_align_batch's rule applied to the sum of the two ends).  The batch is split into launches whose windows and
 * score rows fit PBCCS_DEMUX_WORKSPACE_KB (default 262144); a launch holds at least one read. */
int pbccs_demux_batch(pbccs_engine* eng, const pbccs_demux_barcodes* barcodes, const pbccs_demux_options* opts,
                      const pbccs_demux_read* reads, int n, pbccs_demux_output* out);

/* Demultiplexing work since the last reset: reads given, DP cells (2 * min(W, n) * the sum of the barcode lengths
 * per read that reached the device), kernel launches, device ms (profiling on). */
typedef struct {
    long long reads, cells, launches;
    double device_ms;
} pbccs_demux_stats;
int pbccs_demux_stats_get(pbccs_engine* eng, pbccs_demux_stats* out, int reset);

/* pbccs_ccs_batch followed by one pbccs_demux_batch over the consensuses of the ZMWs that ended Success.  demux
 * holds one entry per ZMW (entry z of every array belongs to ZMW z; scores must be NULL); demuxed_mask[z], when not
 * NULL, is 1 for the ZMWs that were demultiplexed and 0 for the others, whose entries are left untouched.  The
 * barcodes and options are refused before any device work. */
int pbccs_ccs_batch_demux(pbccs_engine* eng, const pbccs_ccs_input* in, int n, long long max_poa_coverage,
                          const pbccs_polish_options* opts, const pbccs_demux_barcodes* barcodes,
                          const pbccs_demux_options* demux_opts, pbccs_ccs_output* out, pbccs_demux_output* demux,
                          int* demuxed_mask);

#ifdef __cplusplus
}
#endif

#endif /* PBCCS_AMD_H */

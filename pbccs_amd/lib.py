"""ctypes declarations of include/pbccs_amd.h and the loader of the in-tree libpbccs_amd.so."""
import ctypes
import os

HERE = os.path.dirname(os.path.abspath(__file__))
# PBCCS_LIB: load another in-tree build of the same library (A/B experiments: tools/build_ab.sh, then the ab_lib
# step of tools/gpu_steps.sh)
LIB_PATH = os.environ.get("PBCCS_LIB") or os.path.join(HERE, "_lib", "libpbccs_amd.so")

PBCCS_OK = 0
ERRORS = {-1: "EINVAL", -2: "EOOM", -3: "EDEVICE", -4: "ESTATE", -5: "ERANGE"}

_lib = None


class PbccsError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"pbccs {ERRORS.get(code, code)}: {msg}")
        self.code = code


class CMutation(ctypes.Structure):
    _fields_ = [("type", ctypes.c_int), ("start", ctypes.c_int), ("end", ctypes.c_int), ("new_base", ctypes.c_char)]


class CMutationEx(ctypes.Structure):
    _fields_ = [("type", ctypes.c_int), ("start", ctypes.c_int), ("end", ctypes.c_int),
                ("new_bases", ctypes.c_char_p), ("n_bases", ctypes.c_int)]


class CRepeatOptions(ctypes.Structure):
    _fields_ = [("repeat_length", ctypes.c_int), ("min_repeat_elements", ctypes.c_int),
                ("max_iterations", ctypes.c_int), ("mutation_separation", ctypes.c_int),
                ("mutation_neighborhood", ctypes.c_int)]


class CArrowConfig(ctypes.Structure):
    _fields_ = [("snr", ctypes.c_double * 4), ("score_diff", ctypes.c_double),
                ("fast_score_threshold", ctypes.c_double), ("add_threshold", ctypes.c_double)]


class CRefineOptions(ctypes.Structure):
    _fields_ = [("max_iterations", ctypes.c_int), ("mutation_separation", ctypes.c_int),
                ("mutation_neighborhood", ctypes.c_int)]


class CZmwInput(ctypes.Structure):
    _fields_ = [("draft", ctypes.c_char_p), ("draft_len", ctypes.c_int), ("snr", ctypes.c_double * 4),
                ("n_reads", ctypes.c_int), ("seqs", ctypes.POINTER(ctypes.c_char_p)),
                ("lens", ctypes.POINTER(ctypes.c_int)), ("strands", ctypes.POINTER(ctypes.c_int)),
                ("tstarts", ctypes.POINTER(ctypes.c_int)), ("tends", ctypes.POINTER(ctypes.c_int)),
                ("full_pass", ctypes.POINTER(ctypes.c_ubyte))]


class CPolishOptions(ctypes.Structure):
    _fields_ = [("min_passes", ctypes.c_int), ("min_length", ctypes.c_int), ("min_zscore", ctypes.c_double),
                ("max_drop_fraction", ctypes.c_double), ("min_predicted_accuracy", ctypes.c_double),
                ("score_diff", ctypes.c_double), ("refine", CRefineOptions), ("zmws_per_batch", ctypes.c_int)]


class CZmwOutput(ctypes.Structure):
    _fields_ = [("status", ctypes.c_int), ("consensus", ctypes.c_char_p), ("consensus_cap", ctypes.c_int),
                ("consensus_len", ctypes.c_int), ("qvs", ctypes.POINTER(ctypes.c_int)),
                ("add_read_results", ctypes.POINTER(ctypes.c_int)), ("zscores", ctypes.POINTER(ctypes.c_double)),
                ("zg", ctypes.c_double), ("za", ctypes.c_double), ("predicted_accuracy", ctypes.c_double),
                ("n_tested", ctypes.c_longlong), ("n_applied", ctypes.c_longlong), ("n_passes", ctypes.c_int),
                ("status_counts", ctypes.c_int * 5)]


class CKernelStat(ctypes.Structure):
    _fields_ = [("name", ctypes.c_char * 32), ("launches", ctypes.c_longlong), ("device_ms", ctypes.c_double),
                ("cells", ctypes.c_double), ("bytes", ctypes.c_double), ("wave_s", ctypes.c_double)]


class CCounters(ctypes.Structure):
    _fields_ = [("fill_launches", ctypes.c_longlong), ("score_launches", ctypes.c_longlong),
                ("score_tasks", ctypes.c_longlong), ("mutations", ctypes.c_longlong),
                ("band_top_bytes", ctypes.c_longlong), ("band_region_bytes", ctypes.c_longlong),
                ("band_used_bytes", ctypes.c_longlong), ("pool_mapped_bytes", ctypes.c_longlong),
                ("oom_retries", ctypes.c_longlong), ("create_host_ns", ctypes.c_longlong),
                ("create_upload_ns", ctypes.c_longlong), ("derive_ns", ctypes.c_longlong),
                ("fill_work", ctypes.c_longlong * 16), ("scan_reads", ctypes.c_longlong),
                ("uncertain_reads", ctypes.c_longlong), ("exact_rounds", ctypes.c_longlong),
                ("uncertain_why", ctypes.c_longlong * 4), ("repeat_skipped_ckpt", ctypes.c_longlong)]


class CQvModelParams(ctypes.Structure):
    _fields_ = [(n, ctypes.c_float) for n in ("match", "mismatch", "mismatch_s", "branch", "branch_s", "deletion_n",
                                              "deletion_with_tag", "deletion_with_tag_s", "nce", "nce_s")] + \
               [("merge", ctypes.c_float * 4), ("merge_s", ctypes.c_float * 4)]


class CQuiverConfig(ctypes.Structure):
    _fields_ = [("params", CQvModelParams), ("moves_available", ctypes.c_int), ("score_diff", ctypes.c_float),
                ("fast_score_threshold", ctypes.c_float), ("add_threshold", ctypes.c_float),
                ("sum_product", ctypes.c_int), ("recursor", ctypes.c_int)]


class CQuiverRead(ctypes.Structure):
    _fields_ = [("seq", ctypes.c_char_p), ("len", ctypes.c_int), ("ins_qv", ctypes.POINTER(ctypes.c_float)),
                ("subs_qv", ctypes.POINTER(ctypes.c_float)), ("del_qv", ctypes.POINTER(ctypes.c_float)),
                ("del_tag", ctypes.POINTER(ctypes.c_float)), ("merge_qv", ctypes.POINTER(ctypes.c_float)),
                ("chemistry", ctypes.c_char_p), ("strand", ctypes.c_int), ("tstart", ctypes.c_int),
                ("tend", ctypes.c_int), ("threshold", ctypes.c_float)]


class CQvFeatures(ctypes.Structure):
    _fields_ = [("seq", ctypes.c_char_p), ("len", ctypes.c_int), ("ins_qv", ctypes.POINTER(ctypes.c_float)),
                ("subs_qv", ctypes.POINTER(ctypes.c_float)), ("del_qv", ctypes.POINTER(ctypes.c_float)),
                ("del_tag", ctypes.POINTER(ctypes.c_float)), ("merge_qv", ctypes.POINTER(ctypes.c_float))]


class CQuiverZmw(ctypes.Structure):
    _fields_ = [("tpl", ctypes.c_char_p), ("tpl_len", ctypes.c_int), ("reads", ctypes.POINTER(CQuiverRead)),
                ("n_reads", ctypes.c_int)]


class CQuiverResult(ctypes.Structure):
    _fields_ = [("consensus", ctypes.c_char_p), ("consensus_cap", ctypes.c_int), ("consensus_len", ctypes.c_int),
                ("qvs", ctypes.POINTER(ctypes.c_int)), ("n_tested", ctypes.c_longlong),
                ("n_applied", ctypes.c_longlong), ("converged", ctypes.c_int), ("ok", ctypes.c_int),
                ("n_active", ctypes.c_int)]


class CPoaInput(ctypes.Structure):
    _fields_ = [("seqs", ctypes.POINTER(ctypes.c_char_p)), ("lens", ctypes.POINTER(ctypes.c_int)),
                ("n_reads", ctypes.c_int)]


class CPoaOutput(ctypes.Structure):
    _fields_ = [("consensus", ctypes.c_char_p), ("cap", ctypes.c_int), ("len", ctypes.c_int),
                ("keys", ctypes.POINTER(ctypes.c_int)), ("rc", ctypes.POINTER(ctypes.c_int)),
                ("extents", ctypes.POINTER(ctypes.c_int)), ("n_keys", ctypes.c_int)]


class CCcsInput(ctypes.Structure):
    _fields_ = [("snr", ctypes.c_double * 4), ("n_subreads", ctypes.c_int), ("seqs", ctypes.POINTER(ctypes.c_char_p)),
                ("lens", ctypes.POINTER(ctypes.c_int)), ("flags", ctypes.POINTER(ctypes.c_ubyte))]


class CCcsOutput(ctypes.Structure):
    _fields_ = [("polish", CZmwOutput), ("draft", ctypes.c_char_p), ("draft_cap", ctypes.c_int),
                ("draft_len", ctypes.c_int), ("add_order", ctypes.POINTER(ctypes.c_int))]


class CPoaStats(ctypes.Structure):
    _fields_ = [("alignments", ctypes.c_longlong), ("cells", ctypes.c_longlong), ("launches", ctypes.c_longlong),
                ("trace_steps", ctypes.c_longlong), ("fill_ms", ctypes.c_double), ("trace_ms", ctypes.c_double),
                ("bytes", ctypes.c_double), ("prog_ms", ctypes.c_double), ("device_ms", ctypes.c_double),
                ("thread_ms", ctypes.c_double), ("consensus_ms", ctypes.c_double), ("total_ms", ctypes.c_double)]


class CDiploidSite(ctypes.Structure):
    _fields_ = [("position", ctypes.c_int), ("allele0", ctypes.c_int), ("allele1", ctypes.c_int),
                ("log_bayes_factor", ctypes.c_float)]


class CDiploidStats(ctypes.Structure):
    _fields_ = [("sites_screened", ctypes.c_longlong), ("sites_sent_to_host", ctypes.c_longlong),
                ("sites_reported", ctypes.c_longlong)]


class CAlignParams(ctypes.Structure):
    _fields_ = [("kind", ctypes.c_int), ("mode", ctypes.c_int), ("match", ctypes.c_int), ("mismatch", ctypes.c_int),
                ("insert", ctypes.c_int), ("delete_", ctypes.c_int), ("match_score", ctypes.c_float),
                ("mismatch_score", ctypes.c_float), ("gap_open", ctypes.c_float), ("gap_extend", ctypes.c_float),
                ("partial_match_score", ctypes.c_float)]


class CAlignPair(ctypes.Structure):
    _fields_ = [("target", ctypes.c_char_p), ("target_len", ctypes.c_int), ("query", ctypes.c_char_p),
                ("query_len", ctypes.c_int)]


class CAlignResult(ctypes.Structure):
    _fields_ = [("transcript", ctypes.c_char_p), ("cap", ctypes.c_int), ("len", ctypes.c_int),
                ("score_i", ctypes.c_int), ("score_f", ctypes.c_float), ("status", ctypes.c_int)]


class CAlignStats(ctypes.Structure):
    _fields_ = [("pairs", ctypes.c_longlong), ("cells", ctypes.c_longlong), ("launches", ctypes.c_longlong),
                ("trace_steps", ctypes.c_longlong), ("fill_ms", ctypes.c_double), ("trace_ms", ctypes.c_double),
                ("bytes", ctypes.c_double), ("groups", ctypes.c_longlong)]


class CAlignBand(ctypes.Structure):
    _fields_ = [("mode", ctypes.c_int), ("w", ctypes.c_int)]


class CAlignBandInfo(ctypes.Structure):
    _fields_ = [("banded", ctypes.c_int), ("w", ctypes.c_int), ("attempts", ctypes.c_int), ("reason", ctypes.c_int)]


class CAlignBandStats(ctypes.Structure):
    _fields_ = [("pairs", ctypes.c_longlong), ("banded_pairs", ctypes.c_longlong),
                ("second_attempts", ctypes.c_longlong), ("fallbacks", ctypes.c_longlong * 8),
                ("band_cells", ctypes.c_longlong), ("full_cells", ctypes.c_longlong),
                ("launches", ctypes.c_longlong), ("groups", ctypes.c_longlong), ("trace_steps", ctypes.c_longlong),
                ("store_bytes", ctypes.c_double), ("fill_ms", ctypes.c_double), ("trace_ms", ctypes.c_double)]


class CAlignEnds(ctypes.Structure):
    _fields_ = [("mode", ctypes.c_int), ("both_strands", ctypes.c_int)]


class CAlignExtent(ctypes.Structure):
    _fields_ = [("target_begin", ctypes.c_int), ("target_end", ctypes.c_int), ("query_begin", ctypes.c_int),
                ("query_end", ctypes.c_int), ("rc", ctypes.c_int)]


class CMapInput(ctypes.Structure):
    _fields_ = [("draft", ctypes.c_char_p), ("draft_len", ctypes.c_int), ("seqs", ctypes.POINTER(ctypes.c_char_p)),
                ("lens", ctypes.POINTER(ctypes.c_int)), ("n_reads", ctypes.c_int)]


class CMapOutput(ctypes.Structure):
    _fields_ = [("mapped", ctypes.POINTER(ctypes.c_int)), ("rc", ctypes.POINTER(ctypes.c_int)),
                ("extents", ctypes.POINTER(ctypes.c_int)), ("score", ctypes.POINTER(ctypes.c_int))]


class CMapStats(ctypes.Structure):
    _fields_ = [("jobs", ctypes.c_longlong), ("cells", ctypes.c_longlong), ("launches", ctypes.c_longlong),
                ("strips", ctypes.c_longlong), ("device_ms", ctypes.c_double)]


class CSplitMapOutput(ctypes.Structure):
    _fields_ = [("n_segments", ctypes.POINTER(ctypes.c_int)), ("truncated", ctypes.POINTER(ctypes.c_int)),
                ("score", ctypes.POINTER(ctypes.c_int)), ("segments", ctypes.POINTER(ctypes.c_int))]


class CSplitMapStats(ctypes.Structure):
    _fields_ = [("jobs", ctypes.c_longlong), ("cells", ctypes.c_longlong), ("launches", ctypes.c_longlong),
                ("tiled", ctypes.c_longlong), ("device_ms", ctypes.c_double)]


class CSplitOptions(ctypes.Structure):
    _fields_ = [("jump_penalty", ctypes.c_int), ("max_segments", ctypes.c_int)]


class CCcsSplitOutput(ctypes.Structure):
    _fields_ = [("cap", ctypes.c_int), ("n_reads", ctypes.c_int), ("n_segments", ctypes.c_int),
                ("n_missed_adapters", ctypes.c_int), ("n_added", ctypes.c_int),
                ("subread", ctypes.POINTER(ctypes.c_int)), ("segments", ctypes.POINTER(ctypes.c_int)),
                ("full_pass", ctypes.POINTER(ctypes.c_ubyte)), ("add_read_results", ctypes.POINTER(ctypes.c_int)),
                ("zscores", ctypes.POINTER(ctypes.c_double)), ("add_order", ctypes.POINTER(ctypes.c_int))]


class CCcsOptions(ctypes.Structure):
    _fields_ = [("max_poa_coverage", ctypes.c_longlong), ("map_past_cap", ctypes.c_int)]


class CPoaOptions(ctypes.Structure):
    _fields_ = [("max_coverage", ctypes.c_longlong), ("min_coverage", ctypes.c_int), ("banded", ctypes.c_int)]


class CPoaBandStats(ctypes.Structure):
    _fields_ = [("banded_alignments", ctypes.c_longlong), ("fallbacks", ctypes.c_longlong),
                ("band_cells", ctypes.c_longlong), ("full_cells", ctypes.c_longlong), ("seeds", ctypes.c_longlong),
                ("anchors", ctypes.c_longlong), ("seed_ms", ctypes.c_double), ("ranges_ms", ctypes.c_double),
                ("fill_ms", ctypes.c_double), ("trace_ms", ctypes.c_double), ("score_bytes", ctypes.c_double)]


class CSparseAlignInput(ctypes.Structure):
    _fields_ = [("target", ctypes.c_char_p), ("target_len", ctypes.c_int), ("query", ctypes.c_char_p),
                ("query_len", ctypes.c_int), ("reverse_complement", ctypes.c_int),
                ("anchors", ctypes.POINTER(ctypes.c_int)), ("anchor_cap", ctypes.c_int),
                ("ranges", ctypes.POINTER(ctypes.c_int))]


class CSparseAlignOutput(ctypes.Structure):
    _fields_ = [("status", ctypes.c_int), ("n_anchors", ctypes.c_int), ("n_seeds", ctypes.c_longlong),
                ("score", ctypes.c_longlong)]


class CSparseAlignStats(ctypes.Structure):
    _fields_ = [("jobs", ctypes.c_longlong), ("seeds", ctypes.c_longlong), ("anchors", ctypes.c_longlong),
                ("launches", ctypes.c_longlong), ("device_ms", ctypes.c_double),
                ("range_cells", ctypes.c_longlong), ("full_cells", ctypes.c_longlong)]


class CWindowOptions(ctypes.Structure):
    _fields_ = [("window", ctypes.c_int), ("overlap", ctypes.c_int), ("guard", ctypes.c_int), ("k", ctypes.c_int)]


class CWindowRecord(ctypes.Structure):
    _fields_ = [("begin", ctypes.c_int), ("end", ctypes.c_int), ("join", ctypes.c_int), ("cut_begin", ctypes.c_int),
                ("cut_end", ctypes.c_int), ("status", ctypes.c_int), ("n_tested", ctypes.c_longlong),
                ("n_applied", ctypes.c_longlong)]


class CWindowInfo(ctypes.Structure):
    _fields_ = [("n_windows", ctypes.c_int), ("fallback", ctypes.c_int), ("unanchored_reads", ctypes.c_int),
                ("windows", ctypes.POINTER(CWindowRecord)), ("windows_cap", ctypes.c_int)]


class CWindowStats(ctypes.Structure):
    _fields_ = [("zmws", ctypes.c_longlong), ("windows", ctypes.c_longlong), ("fallbacks", ctypes.c_longlong * 4),
                ("unanchored_reads", ctypes.c_longlong), ("cut_tasks", ctypes.c_longlong),
                ("joints", ctypes.c_longlong), ("launches", ctypes.c_longlong), ("slices_ms", ctypes.c_double),
                ("polish_ms", ctypes.c_double), ("join_ms", ctypes.c_double), ("fallback_ms", ctypes.c_double)]


class CRichQvs(ctypes.Structure):
    _fields_ = [("sub_qv", ctypes.POINTER(ctypes.c_int)), ("ins_qv", ctypes.POINTER(ctypes.c_int)),
                ("del_qv", ctypes.POINTER(ctypes.c_int)), ("sub_tag", ctypes.POINTER(ctypes.c_char)),
                ("ins_tag", ctypes.POINTER(ctypes.c_char)), ("cap", ctypes.c_int), ("len", ctypes.c_int)]


class CPolishExtras(ctypes.Structure):
    _fields_ = [("repeats", ctypes.POINTER(CRepeatOptions)), ("repeat_tested", ctypes.POINTER(ctypes.c_longlong)),
                ("repeat_applied", ctypes.POINTER(ctypes.c_longlong)), ("rich", ctypes.POINTER(CRichQvs))]


class CStrandOptions(ctypes.Structure):
    _fields_ = [("min_score", ctypes.c_double), ("min_reads", ctypes.c_int), ("min_sites", ctypes.c_int),
                ("directional", ctypes.c_int)]


class CStrandResult(ctypes.Structure):
    _fields_ = [("n_sites", ctypes.c_int), ("cap", ctypes.c_int), ("position", ctypes.POINTER(ctypes.c_int)),
                ("type", ctypes.POINTER(ctypes.c_int)), ("base", ctypes.POINTER(ctypes.c_char)),
                ("sum_fwd", ctypes.POINTER(ctypes.c_double)), ("sum_rev", ctypes.POINTER(ctypes.c_double)),
                ("split", ctypes.c_int), ("fwd", CZmwOutput), ("rev", CZmwOutput)]


class CStrandStats(ctypes.Structure):
    _fields_ = [("strand_screened", ctypes.c_longlong), ("strand_sites", ctypes.c_longlong),
                ("strand_split", ctypes.c_longlong)]


class CKineticsRead(ctypes.Structure):
    _fields_ = [("transcript", ctypes.c_char_p), ("transcript_len", ctypes.c_int), ("rc", ctypes.c_int),
                ("rb", ctypes.c_int), ("tb", ctypes.c_int), ("te", ctypes.c_int), ("len", ctypes.c_int),
                ("ip", ctypes.POINTER(ctypes.c_ushort)), ("pw", ctypes.POINTER(ctypes.c_ushort))]


class CKineticsPileupInput(ctypes.Structure):
    _fields_ = [("consensus_len", ctypes.c_int), ("n_reads", ctypes.c_int), ("reads", ctypes.POINTER(CKineticsRead))]


class CKineticsOutput(ctypes.Structure):
    _fields_ = [("mean", ctypes.POINTER(ctypes.c_ushort) * 4), ("code", ctypes.POINTER(ctypes.c_ubyte) * 4),
                ("coverage", ctypes.POINTER(ctypes.c_int) * 4), ("n_contributed", ctypes.c_int * 2),
                ("read_status", ctypes.POINTER(ctypes.c_int))]


class CKineticsInput(ctypes.Structure):
    _fields_ = [("consensus", ctypes.c_char_p), ("consensus_len", ctypes.c_int), ("n_reads", ctypes.c_int),
                ("seqs", ctypes.POINTER(ctypes.c_char_p)), ("lens", ctypes.POINTER(ctypes.c_int)),
                ("ip", ctypes.POINTER(ctypes.POINTER(ctypes.c_ushort))),
                ("pw", ctypes.POINTER(ctypes.POINTER(ctypes.c_ushort)))]


class CKineticsOptions(ctypes.Structure):
    _fields_ = [("band", CAlignBand)]


class CKineticsStats(ctypes.Structure):
    _fields_ = [("reads", ctypes.c_longlong), ("skipped_unmapped", ctypes.c_longlong),
                ("skipped_empty_extent", ctypes.c_longlong), ("skipped_align_failed", ctypes.c_longlong),
                ("columns", ctypes.c_longlong), ("positions", ctypes.c_longlong), ("launches", ctypes.c_longlong),
                ("columns_ms", ctypes.c_double), ("reduce_ms", ctypes.c_double)]


class CPileupRead(ctypes.Structure):
    _fields_ = [("transcript", ctypes.c_char_p), ("transcript_len", ctypes.c_int), ("rc", ctypes.c_int),
                ("rb", ctypes.c_int), ("tb", ctypes.c_int), ("te", ctypes.c_int), ("seq", ctypes.c_char_p),
                ("len", ctypes.c_int)]


class CPileupColumnsInput(ctypes.Structure):
    _fields_ = [("consensus", ctypes.c_char_p), ("consensus_len", ctypes.c_int), ("n_reads", ctypes.c_int),
                ("reads", ctypes.POINTER(CPileupRead))]


class CPileupOutput(ctypes.Structure):
    _fields_ = [("counts", ctypes.POINTER(ctypes.c_int)), ("ins_reads", ctypes.POINTER(ctypes.c_int)),
                ("ins_bases", ctypes.POINTER(ctypes.c_int)), ("slot_cov", ctypes.POINTER(ctypes.c_int)),
                ("max_ins", ctypes.POINTER(ctypes.c_int)), ("cov", ctypes.POINTER(ctypes.c_int)),
                ("plurality", ctypes.POINTER(ctypes.c_ubyte)), ("ins_plurality", ctypes.POINTER(ctypes.c_ubyte)),
                ("read_status", ctypes.POINTER(ctypes.c_int)), ("n_match", ctypes.POINTER(ctypes.c_int)),
                ("n_mismatch", ctypes.POINTER(ctypes.c_int)), ("n_ins", ctypes.POINTER(ctypes.c_int)),
                ("n_del", ctypes.POINTER(ctypes.c_int)), ("rc", ctypes.POINTER(ctypes.c_int)),
                ("rb", ctypes.POINTER(ctypes.c_int)), ("re", ctypes.POINTER(ctypes.c_int)),
                ("tb", ctypes.POINTER(ctypes.c_int)), ("te", ctypes.POINTER(ctypes.c_int)),
                ("transcripts", ctypes.POINTER(ctypes.c_char_p)), ("transcript_lens", ctypes.POINTER(ctypes.c_int)),
                ("cov_sum", ctypes.c_longlong), ("n_used", ctypes.c_int * 2)]


class CPileupInput(ctypes.Structure):
    _fields_ = [("consensus", ctypes.c_char_p), ("consensus_len", ctypes.c_int), ("n_reads", ctypes.c_int),
                ("seqs", ctypes.POINTER(ctypes.c_char_p)), ("lens", ctypes.POINTER(ctypes.c_int)),
                ("ip", ctypes.POINTER(ctypes.POINTER(ctypes.c_ushort))),
                ("pw", ctypes.POINTER(ctypes.POINTER(ctypes.c_ushort))),
                ("kinetics", ctypes.POINTER(CKineticsOutput))]


class CPileupOptions(ctypes.Structure):
    _fields_ = [("band", CAlignBand)]


class CPileupStats(ctypes.Structure):
    _fields_ = [("reads", ctypes.c_longlong), ("skipped_unmapped", ctypes.c_longlong),
                ("skipped_empty_extent", ctypes.c_longlong), ("skipped_align_failed", ctypes.c_longlong),
                ("columns", ctypes.c_longlong), ("slots", ctypes.c_longlong), ("launches", ctypes.c_longlong),
                ("placed", ctypes.c_longlong), ("shared", ctypes.c_longlong), ("columns_ms", ctypes.c_double),
                ("reduce_ms", ctypes.c_double), ("scan_ms", ctypes.c_double), ("rows_ms", ctypes.c_double)]


class CDemuxBarcodes(ctypes.Structure):
    _fields_ = [("seqs", ctypes.POINTER(ctypes.c_char_p)), ("lens", ctypes.POINTER(ctypes.c_int)),
                ("n", ctypes.c_int)]


class CDemuxOptions(ctypes.Structure):
    _fields_ = [("match", ctypes.c_int), ("mismatch", ctypes.c_int), ("insert", ctypes.c_int),
                ("delete_", ctypes.c_int), ("design", ctypes.c_int), ("window", ctypes.c_int),
                ("window_mult", ctypes.c_int), ("min_quality", ctypes.c_int), ("min_score_lead", ctypes.c_int)]


class CDemuxRead(ctypes.Structure):
    _fields_ = [("seq", ctypes.c_void_p), ("len", ctypes.c_int)]


class CDemuxOutput(ctypes.Structure):
    _fields_ = [(k, ctypes.POINTER(ctypes.c_int)) for k in
                ("lead", "trail", "called", "score", "score_lead", "quality", "extents", "clip", "overlap", "best",
                 "scores")]


class CDemuxStats(ctypes.Structure):
    _fields_ = [("reads", ctypes.c_longlong), ("cells", ctypes.c_longlong), ("launches", ctypes.c_longlong),
                ("device_ms", ctypes.c_double)]


# exported symbol -> (restype, argtypes); tests check that every symbol of include/pbccs_amd.h is exported
P = ctypes.c_void_p
I = ctypes.c_int
D = ctypes.c_double
PI = ctypes.POINTER(ctypes.c_int)
PD = ctypes.POINTER(ctypes.c_double)
PLL = ctypes.POINTER(ctypes.c_longlong)
PM = ctypes.POINTER(CMutation)
PF = ctypes.POINTER(ctypes.c_float)
PMX = ctypes.POINTER(CMutationEx)
SIGNATURES = {
    "pbccs_engine_create": (I, [I, ctypes.POINTER(P)]),
    "pbccs_engine_destroy": (None, [P]),
    "pbccs_last_error": (ctypes.c_char_p, []),
    "pbccs_device_count": (I, []),
    "pbccs_engine_counters": (I, [P, ctypes.POINTER(CCounters), I]),
    "pbccs_scorer_create": (I, [P, ctypes.POINTER(CArrowConfig), ctypes.c_char_p, I, ctypes.POINTER(P)]),
    "pbccs_scorer_destroy": (None, [P]),
    "pbccs_scorer_add_read": (I, [P, ctypes.c_char_p, I, I, I, I, D, PI]),
    "pbccs_scorer_score": (I, [P, PM, D, PD]),
    "pbccs_scorer_score_many": (I, [P, PM, I, D, PD]),
    "pbccs_scorer_scores": (I, [P, PM, D, PD]),
    "pbccs_scorer_is_favorable": (I, [P, PM, I, PI]),
    "pbccs_scorer_apply_mutations": (I, [P, PM, I]),
    "pbccs_scorer_template": (I, [P, I, ctypes.c_char_p, I, PI]),
    "pbccs_scorer_template_length": (I, [P]),
    "pbccs_scorer_num_reads": (I, [P]),
    "pbccs_scorer_read_info": (I, [P, I, PI, PI, PI, PI]),
    "pbccs_scorer_baseline_score": (I, [P, PD]),
    "pbccs_scorer_baseline_scores": (I, [P, PD, I, PI]),
    "pbccs_scorer_zscores": (I, [P, PD, PD, PD]),
    "pbccs_scorer_num_flipflops": (I, [P, PI]),
    "pbccs_refine_consensus": (I, [P, ctypes.POINTER(CRefineOptions), PLL, PLL, PI]),
    "pbccs_consensus_qvs": (I, [P, PI, I, PI]),
    "pbccs_polish_options_default": (None, [ctypes.POINTER(CPolishOptions)]),
    "pbccs_polish_batch": (I, [P, ctypes.POINTER(CZmwInput), I, ctypes.POINTER(CPolishOptions),
                               ctypes.POINTER(CZmwOutput)]),
    "pbccs_plan_batches": (I, [ctypes.POINTER(CZmwInput), I, D, I, D, PI, PI, PD, PI]),
    "pbccs_batch_create": (I, [P, ctypes.POINTER(CZmwInput), I, ctypes.POINTER(CPolishOptions), ctypes.POINTER(P)]),
    "pbccs_batch_polish": (I, [P, ctypes.POINTER(CZmwOutput)]),
    "pbccs_batch_destroy": (None, [P]),
    "pbccs_batch_polish_many": (I, [ctypes.POINTER(P), I, ctypes.POINTER(ctypes.POINTER(CZmwOutput))]),
    "pbccs_engine_set_concurrency": (I, [P, I]),
    "pbccs_engine_reserve_pool": (I, [P, ctypes.c_size_t]),
    "pbccs_engine_set_profiling": (I, [P, I]),
    "pbccs_engine_kernel_stats": (I, [P, ctypes.POINTER(CKernelStat), I, PI, I]),
    # Quiver family
    "pbccs_quiver_scorer_create": (I, [P, ctypes.POINTER(CQuiverConfig), ctypes.POINTER(ctypes.c_char_p), I,
                                       ctypes.c_char_p, I, ctypes.POINTER(P)]),
    "pbccs_quiver_scorer_destroy": (None, [P]),
    "pbccs_quiver_scorer_add_read": (I, [P, ctypes.c_char_p, I, PF, PF, PF, PF, PF, ctypes.c_char_p, I, I, I,
                                         ctypes.c_float, PI]),
    "pbccs_quiver_scorer_score_many": (I, [P, PM, I, I, PF]),
    "pbccs_quiver_scorer_scores": (I, [P, PM, ctypes.c_float, PF]),
    "pbccs_quiver_scorer_read_score_mutation": (I, [P, I, PM, PF]),
    "pbccs_quiver_scorer_is_favorable": (I, [P, PM, I, PI]),
    "pbccs_quiver_scorer_apply_mutations": (I, [P, PM, I]),
    "pbccs_quiver_scorer_template": (I, [P, I, ctypes.c_char_p, I, PI]),
    "pbccs_quiver_scorer_num_reads": (I, [P]),
    "pbccs_quiver_scorer_read_info": (I, [P, I, PI, PI, PI, PI]),
    "pbccs_quiver_scorer_baseline_score": (I, [P, PF]),
    "pbccs_quiver_scorer_baseline_scores": (I, [P, PF, I, PI]),
    "pbccs_quiver_scorer_num_flipflops": (I, [P, PI]),
    "pbccs_quiver_scorer_allocated_entries": (I, [P, I, PLL, PLL]),
    "pbccs_quiver_scorer_alignment": (I, [P, I, ctypes.c_char_p, ctypes.c_char_p, I, PI]),
    "pbccs_quiver_refine_consensus": (I, [P, ctypes.POINTER(CRefineOptions), PLL, PLL, PI]),
    "pbccs_quiver_consensus_qvs": (I, [P, PI, I, PI]),
    "pbccs_qv_evaluator_moves": (I, [P, ctypes.POINTER(CQvFeatures), ctypes.c_char_p, I, ctypes.POINTER(CQvModelParams),
                                     I, I, PI, PI, I, PF, PF, PF, PF]),
    "pbccs_quiver_polish_batch": (I, [P, ctypes.POINTER(CQuiverConfig), ctypes.POINTER(ctypes.c_char_p), I,
                                      ctypes.POINTER(CQuiverZmw), I, ctypes.POINTER(CRefineOptions),
                                      ctypes.POINTER(CQuiverResult)]),
    # Quiver: mutations of any width and repeat refinement
    "pbccs_quiver_scorer_score_many_ex": (I, [P, PMX, I, I, PF]),
    "pbccs_quiver_scorer_scores_ex": (I, [P, PMX, ctypes.c_float, PF]),
    "pbccs_quiver_scorer_is_favorable_ex": (I, [P, PMX, I, PI]),
    "pbccs_quiver_scorer_read_score_mutation_ex": (I, [P, I, PMX, PF]),
    "pbccs_quiver_scorer_apply_mutations_ex": (I, [P, PMX, I]),
    "pbccs_quiver_refine_repeats": (I, [P, ctypes.POINTER(CRepeatOptions), PLL, PLL, PI]),
    "pbccs_repeat_mutations": (I, [ctypes.c_char_p, I, I, I, I, I, PMX, I, PI]),
    "pbccs_apply_mutations": (I, [ctypes.c_char_p, I, PMX, I, ctypes.c_char_p, I, PI, PI]),
    "pbccs_quiver_polish_batch_ex": (I, [P, ctypes.POINTER(CQuiverConfig), ctypes.POINTER(ctypes.c_char_p), I,
                                         ctypes.POINTER(CQuiverZmw), I, ctypes.POINTER(CRefineOptions),
                                         ctypes.POINTER(CRepeatOptions), PLL, PLL, ctypes.POINTER(CQuiverResult)]),
    # Arrow: mutations of any width and repeat refinement
    "pbccs_scorer_score_many_ex": (I, [P, PMX, I, D, PD]),
    "pbccs_scorer_scores_ex": (I, [P, PMX, D, PD]),
    "pbccs_scorer_is_favorable_ex": (I, [P, PMX, I, PI]),
    "pbccs_scorer_apply_mutations_ex": (I, [P, PMX, I]),
    "pbccs_refine_repeats": (I, [P, ctypes.POINTER(CRepeatOptions), PLL, PLL, PI]),
    "pbccs_wide_columns_needed": (I, [PMX, I, I, I, PI]),
    "pbccs_polish_batch_ex": (I, [P, ctypes.POINTER(CZmwInput), I, ctypes.POINTER(CPolishOptions),
                                  ctypes.POINTER(CRepeatOptions), PLL, PLL, ctypes.POINTER(CZmwOutput)]),
    # Diploid site calling
    "pbccs_is_site_heterozygous": (I, [PF, I, I, ctypes.c_float, PI, ctypes.POINTER(CDiploidSite), PI]),
    "pbccs_scorer_site_scores": (I, [P, I, I, PF, ctypes.c_longlong, PLL]),
    "pbccs_quiver_scorer_site_scores": (I, [P, I, I, PF, ctypes.c_longlong, PLL]),
    "pbccs_scorer_diploid_sites": (I, [P, I, I, ctypes.c_float, I, ctypes.POINTER(CDiploidSite), I, PI, PI]),
    "pbccs_quiver_scorer_diploid_sites": (I, [P, I, I, ctypes.c_float, I, ctypes.POINTER(CDiploidSite), I, PI, PI]),
    "pbccs_diploid_stats_get": (I, [P, ctypes.POINTER(CDiploidStats), I]),
    # POA draft
    "pbccs_poa_batch": (I, [P, ctypes.POINTER(CPoaInput), I, ctypes.c_longlong, I, ctypes.POINTER(CPoaOutput)]),
    "pbccs_sparse_poa_create": (I, [P, ctypes.POINTER(P)]),
    "pbccs_sparse_poa_destroy": (None, [P]),
    "pbccs_sparse_poa_orient_and_add_read": (I, [P, ctypes.c_char_p, I, ctypes.c_float, PI]),
    "pbccs_sparse_poa_find_consensus": (I, [P, I, ctypes.c_char_p, I, PI, PI, PI, PI]),
    "pbccs_sparse_poa_graphviz": (I, [P, I, I, ctypes.c_char_p, I, PI]),
    "pbccs_poa_consensus": (I, [P, ctypes.POINTER(ctypes.c_char_p), PI, I, I, I, ctypes.c_char_p, I, PI, I,
                                ctypes.c_char_p, I, PI]),
    "pbccs_poa_stats_get": (I, [P, ctypes.POINTER(CPoaStats), I]),
    # pairwise alignment
    "pbccs_align_batch": (I, [P, ctypes.POINTER(CAlignParams), ctypes.POINTER(CAlignPair), I,
                              ctypes.POINTER(CAlignResult)]),
    "pbccs_align_stats_get": (I, [P, ctypes.POINTER(CAlignStats), I]),
    # the certified band
    "pbccs_align_batch_ex": (I, [P, ctypes.POINTER(CAlignParams), ctypes.POINTER(CAlignPair), I,
                                 ctypes.POINTER(CAlignResult), ctypes.POINTER(CAlignBand),
                                 ctypes.POINTER(CAlignBandInfo)]),
    "pbccs_align_band_bound": (I, [ctypes.POINTER(CAlignParams), I, I, I, ctypes.POINTER(ctypes.c_double),
                                   ctypes.POINTER(ctypes.c_double), PI]),
    "pbccs_align_band_widen": (I, [ctypes.POINTER(CAlignParams), I, I, ctypes.c_double, PI]),
    "pbccs_align_band_stats_get": (I, [P, ctypes.POINTER(CAlignBandStats), I]),
    # the ends-free modes
    "pbccs_align_batch_ends": (I, [P, ctypes.POINTER(CAlignParams), ctypes.POINTER(CAlignEnds),
                                   ctypes.POINTER(CAlignPair), I, ctypes.POINTER(CAlignResult),
                                   ctypes.POINTER(CAlignExtent)]),
    "pbccs_ccs_batch": (I, [P, ctypes.POINTER(CCcsInput), I, ctypes.c_longlong, ctypes.POINTER(CPolishOptions),
                            ctypes.POINTER(CCcsOutput)]),
    # MapToDraft and the capped ccs that keeps every pass
    "pbccs_map_batch": (I, [P, ctypes.POINTER(CMapInput), I, ctypes.c_float, ctypes.POINTER(CMapOutput)]),
    "pbccs_map_stats_get": (I, [P, ctypes.POINTER(CMapStats), I]),
    "pbccs_split_map_batch": (I, [P, ctypes.POINTER(CMapInput), I, I, I, ctypes.POINTER(CSplitMapOutput)]),
    "pbccs_split_map_stats_get": (I, [P, ctypes.POINTER(CSplitMapStats), I]),
    "pbccs_ccs_options_default": (None, [ctypes.POINTER(CCcsOptions)]),
    "pbccs_ccs_batch_ex": (I, [P, ctypes.POINTER(CCcsInput), I, ctypes.POINTER(CCcsOptions),
                               ctypes.POINTER(CPolishOptions), ctypes.POINTER(CCcsOutput)]),
    # SparseAlign: seeds, chain, alignable ranges
    "pbccs_sparse_align_batch": (I, [P, I, ctypes.POINTER(CSparseAlignInput), I,
                                     ctypes.POINTER(CSparseAlignOutput)]),
    "pbccs_sparse_align_stats_get": (I, [P, ctypes.POINTER(CSparseAlignStats), I]),
    # banded POA fill
    "pbccs_poa_options_default": (None, [ctypes.POINTER(CPoaOptions)]),
    "pbccs_poa_batch_ex": (I, [P, ctypes.POINTER(CPoaInput), I, ctypes.POINTER(CPoaOptions),
                               ctypes.POINTER(CPoaOutput)]),
    "pbccs_sparse_poa_set_banded": (I, [P, I]),
    "pbccs_sparse_poa_alignable_ranges": (I, [P, ctypes.c_char_p, I, I, PI, I, PI, PI, I, PI, PI, I, PI, PI]),
    "pbccs_sparse_poa_try_add_read": (I, [P, ctypes.c_char_p, I, I, I, PF, PI, I, PI]),
    "pbccs_poa_band_stats_get": (I, [P, ctypes.POINTER(CPoaBandStats), I]),
    # windowed polish
    "pbccs_window_options_default": (None, [ctypes.POINTER(CWindowOptions)]),
    "pbccs_window_plan": (I, [I, ctypes.POINTER(CWindowOptions), PI, I, PI]),
    "pbccs_window_join": (I, [ctypes.c_char_p, I, I, I, ctypes.c_char_p, I, I, I, I, PI, PI, PI, PI]),
    "pbccs_window_slices": (I, [P, ctypes.POINTER(CZmwInput), I, ctypes.POINTER(CWindowOptions), I, PI, PI,
                                ctypes.c_longlong, PLL, PI]),
    "pbccs_polish_windowed": (I, [P, ctypes.POINTER(CZmwInput), I, ctypes.POINTER(CPolishOptions),
                                  ctypes.POINTER(CWindowOptions), ctypes.POINTER(CZmwOutput),
                                  ctypes.POINTER(CWindowInfo)]),
    "pbccs_window_stats_get": (I, [P, ctypes.POINTER(CWindowStats), I]),
    # per-base rich QVs
    "pbccs_consensus_qvs_rich": (I, [P, PI, ctypes.POINTER(CRichQvs), PI]),
    "pbccs_quiver_consensus_qvs_rich": (I, [P, PI, ctypes.POINTER(CRichQvs), PI]),
    "pbccs_polish_windowed_ex": (I, [P, ctypes.POINTER(CZmwInput), I, ctypes.POINTER(CPolishOptions),
                                     ctypes.POINTER(CWindowOptions), ctypes.POINTER(CPolishExtras),
                                     ctypes.POINTER(CZmwOutput), ctypes.POINTER(CWindowInfo)]),
    # directional consensus
    "pbccs_strand_options_default": (None, [ctypes.POINTER(CStrandOptions)]),
    "pbccs_polish_batch_strand": (I, [P, ctypes.POINTER(CZmwInput), I, ctypes.POINTER(CPolishOptions),
                                      ctypes.POINTER(CPolishExtras), ctypes.POINTER(CStrandOptions),
                                      ctypes.POINTER(CStrandResult), ctypes.POINTER(CZmwOutput)]),
    "pbccs_ccs_batch_strand": (I, [P, ctypes.POINTER(CCcsInput), I, ctypes.POINTER(CCcsOptions),
                                   ctypes.POINTER(CPoaOptions), ctypes.POINTER(CPolishOptions),
                                   ctypes.POINTER(CPolishExtras), ctypes.POINTER(CStrandOptions),
                                   ctypes.POINTER(CStrandResult), ctypes.POINTER(CCcsOutput)]),
    "pbccs_split_options_default": (None, [ctypes.POINTER(CSplitOptions)]),
    "pbccs_ccs_batch_split": (I, [P, ctypes.POINTER(CCcsInput), I, ctypes.POINTER(CCcsOptions),
                                  ctypes.POINTER(CPoaOptions), ctypes.POINTER(CPolishOptions),
                                  ctypes.POINTER(CPolishExtras), ctypes.POINTER(CSplitOptions),
                                  ctypes.POINTER(CCcsSplitOutput), ctypes.POINTER(CCcsOutput)]),
    "pbccs_scorer_strand_scores": (I, [P, PM, I, PD, PD, PI, PI]),
    "pbccs_scorer_strand_sites": (I, [P, ctypes.POINTER(CStrandOptions), PI, PI, ctypes.POINTER(ctypes.c_char), PD,
                                      PD, I, PI]),
    "pbccs_strand_stats_get": (I, [P, ctypes.POINTER(CStrandStats), I]),
    # consensus kinetics
    "pbccs_kinetics_options_default": (None, [ctypes.POINTER(CKineticsOptions)]),
    "pbccs_kinetics_pileup": (I, [P, ctypes.POINTER(CKineticsPileupInput), I, ctypes.POINTER(CKineticsOutput)]),
    "pbccs_kinetics_batch": (I, [P, ctypes.POINTER(CKineticsInput), I, ctypes.POINTER(CKineticsOptions),
                                 ctypes.POINTER(CKineticsOutput)]),
    "pbccs_kinetics_stats_get": (I, [P, ctypes.POINTER(CKineticsStats), I]),
    # subread pileup
    "pbccs_pileup_options_default": (None, [ctypes.POINTER(CPileupOptions)]),
    "pbccs_pileup_columns": (I, [P, ctypes.POINTER(CPileupColumnsInput), I, ctypes.POINTER(CPileupOutput)]),
    "pbccs_pileup_batch": (I, [P, ctypes.POINTER(CPileupInput), I, ctypes.POINTER(CPileupOptions),
                               ctypes.POINTER(CPileupOutput)]),
    "pbccs_pileup_msa": (I, [P, ctypes.POINTER(CPileupColumnsInput), I, PI, ctypes.POINTER(PI),
                             ctypes.POINTER(ctypes.c_char_p)]),
    "pbccs_pileup_stats_get": (I, [P, ctypes.POINTER(CPileupStats), I]),
    # barcode demultiplexing
    "pbccs_demux_options_default": (None, [ctypes.POINTER(CDemuxOptions)]),
    "pbccs_demux_batch": (I, [P, ctypes.POINTER(CDemuxBarcodes), ctypes.POINTER(CDemuxOptions),
                              ctypes.POINTER(CDemuxRead), I, ctypes.POINTER(CDemuxOutput)]),
    "pbccs_demux_stats_get": (I, [P, ctypes.POINTER(CDemuxStats), I]),
    "pbccs_ccs_batch_demux": (I, [P, ctypes.POINTER(CCcsInput), I, ctypes.c_longlong, ctypes.POINTER(CPolishOptions),
                                  ctypes.POINTER(CDemuxBarcodes), ctypes.POINTER(CDemuxOptions),
                                  ctypes.POINTER(CCcsOutput), ctypes.POINTER(CDemuxOutput), PI]),
}
# bound like the rest; kept apart because SIGNATURES is compared with the header's names of letters and underscores
DIGIT_SIGNATURES = {
    "pbccs_ccs_batch_ex2": (I, [P, ctypes.POINTER(CCcsInput), I, ctypes.POINTER(CCcsOptions),
                                ctypes.POINTER(CPoaOptions), ctypes.POINTER(CPolishOptions),
                                ctypes.POINTER(CCcsOutput)]),
    "pbccs_ccs_batch_ex3": (I, [P, ctypes.POINTER(CCcsInput), I, ctypes.POINTER(CCcsOptions),
                                ctypes.POINTER(CPoaOptions), ctypes.POINTER(CWindowOptions),
                                ctypes.POINTER(CPolishOptions), ctypes.POINTER(CCcsOutput),
                                ctypes.POINTER(CWindowInfo)]),
    "pbccs_polish_batch_ex2": (I, [P, ctypes.POINTER(CZmwInput), I, ctypes.POINTER(CPolishOptions),
                                   ctypes.POINTER(CPolishExtras), ctypes.POINTER(CZmwOutput)]),
    "pbccs_quiver_polish_batch_ex2": (I, [P, ctypes.POINTER(CQuiverConfig), ctypes.POINTER(ctypes.c_char_p), I,
                                          ctypes.POINTER(CQuiverZmw), I, ctypes.POINTER(CRefineOptions),
                                          ctypes.POINTER(CPolishExtras), ctypes.POINTER(CQuiverResult)]),
    "pbccs_ccs_batch_ex4": (I, [P, ctypes.POINTER(CCcsInput), I, ctypes.POINTER(CCcsOptions),
                                ctypes.POINTER(CPoaOptions), ctypes.POINTER(CWindowOptions),
                                ctypes.POINTER(CPolishOptions), ctypes.POINTER(CPolishExtras),
                                ctypes.POINTER(CCcsOutput), ctypes.POINTER(CWindowInfo)]),
}


def load():
    """Load the HIP engine.  Raises (never falls back) when the library has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise PbccsError(-3, f"{LIB_PATH} is missing: run __graft_entry__.build() (no CPU fallback exists)")
        L = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in list(SIGNATURES.items()) + list(DIGIT_SIGNATURES.items()):
            f = getattr(L, name)
            f.restype = res
            f.argtypes = args
        _lib = L
    return _lib


def check(rc):
    if rc != PBCCS_OK:
        msg = load().pbccs_last_error()
        raise PbccsError(rc, msg.decode() if msg else "")
    return rc

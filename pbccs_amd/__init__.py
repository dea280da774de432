"""pbccs_amd -- MI355X-native consensus polishing (the pbccs / ConsensusCore Arrow hot path).

Python mirror of the reference's polishing API, calling the HIP engine through the C ABI in
include/pbccs_amd.h (libpbccs_amd.so, built in-tree by __graft_entry__.build()).  Names follow
ConsensusCore: ArrowConfig, ArrowMultiReadMutationScorer, Mutation, RefineConsensus, ConsensusQVs.
There is no CPU fallback: if the library is missing or no GPU is present, calls raise.
"""
import ctypes
import math
import os

# Batches in flight each polish on their own HIP streams; HIP's default of 4 hardware queues makes the
# streams of different batches share queues (a long fill of one batch then blocks the others).  Takes
# effect only if the HIP runtime has not been initialised yet in this process.
if int(os.environ.get("GPU_MAX_HW_QUEUES", "4") or 4) < 16:   # the boxes export HIP's default (4)
    os.environ["GPU_MAX_HW_QUEUES"] = "16"

from . import lib as _lib_mod
from .lib import PbccsError, load

INSERTION, DELETION, SUBSTITUTION = 0, 1, 2
FORWARD_STRAND, REVERSE_STRAND = 0, 1
SUCCESS, ALPHABETAMISMATCH, MEM_FAIL, POOR_ZSCORE, OTHER = 0, 1, 2, 3, 4
AddReadResultNames = ["SUCCESS", "ALPHA/BETA MISMATCH", "EXCESSIVE MEMORY USAGE", "POOR Z-SCORE", "OTHER"]
ZMW_STATUS = ["Success", "NoSubreads", "TooShort", "TooManyUnusable", "TooFewPasses", "NonConvergent",
              "PoorQuality", "Other"]
DBL_MAX = 1.7976931348623157e308


class Mutation:
    """ConsensusCore::Mutation (Mutation.hpp:56-129).  Mutation(type, position, base) is the single-base form;
    a multi-character `base` string or an `end` gives a mutation of any width (Mutation-inl.hpp:53-77): an
    insertion of the string at `position`, a substitution of [position, position + len(base)), a deletion of
    [position, end).  The Quiver scorer takes them as they come; the Arrow scorer takes them where the call says
    wide=True (k_score_wide) and refuses them otherwise, as the reference's does
    (Arrow/MutationScorer.cpp:181-183)."""

    __slots__ = ("type", "start", "end", "new_base")

    def __init__(self, mtype, position, base="-", end=None):
        self.type = mtype
        self.start = position
        width = 1 if mtype == DELETION else max(1, len(base))
        if end is not None:
            self.end = end
        else:
            self.end = position if mtype == INSERTION else position + width
        self.new_base = "-" if mtype == DELETION else base

    @property
    def new_bases(self):
        return "" if self.type == DELETION else self.new_base

    def is_single_base(self):
        return len(self.new_base) == 1 and self.end - self.start == (0 if self.type == INSERTION else 1)

    def LengthDiff(self):
        return len(self.new_bases) if self.type == INSERTION else (self.start - self.end if self.type == DELETION else 0)

    def _c(self):
        if not self.is_single_base():
            raise _lib_mod.PbccsError(-1, "multi-base mutation: the Arrow scorer takes it with wide=True, the Quiver "
                                          "scorer as it is")
        return _lib_mod.CMutation(self.type, self.start, self.end, self.new_base.encode()[:1] or b"-")

    def _cx(self):
        b = self.new_bases.encode()
        return _lib_mod.CMutationEx(self.type, self.start, self.end, b, len(b))

    def __repr__(self):
        name = ["Insertion", "Deletion", "Substitution"][self.type]
        if self.is_single_base():
            return f"{name}({self.new_base})@{self.start}"
        return f"{name}({self.new_bases})@{self.start}:{self.end}"

    def __eq__(self, o):
        return (self.type, self.start, self.end, self.new_base) == (o.type, o.start, o.end, o.new_base)

    def __lt__(self, o):   # Mutation-inl.hpp:179-186
        return (self.start, self.end, self.type, self.new_bases) < (o.start, o.end, o.type, o.new_bases)

    def __hash__(self):
        return hash((self.type, self.start, self.end, self.new_base))


class ArrowConfig:
    """ArrowConfig(ContextParameters(SNR), BandingOptions(scoreDiff), fastScoreThreshold, addThreshold)."""

    def __init__(self, snr, score_diff=12.5, fast_score_threshold=-12.5, add_threshold=float("nan")):
        self.snr = tuple(float(x) for x in snr)
        self.score_diff = float(score_diff)
        self.fast_score_threshold = float(fast_score_threshold)
        self.add_threshold = float(add_threshold)

    def _c(self):
        c = _lib_mod.CArrowConfig()
        for i in range(4):
            c.snr[i] = self.snr[i]
        c.score_diff = self.score_diff
        c.fast_score_threshold = self.fast_score_threshold
        c.add_threshold = self.add_threshold
        return c


class Engine:
    """One engine per GPU (device ordinal)."""

    def __init__(self, device=0):
        L = load()
        h = ctypes.c_void_p()
        _lib_mod.check(L.pbccs_engine_create(device, ctypes.byref(h)))
        self._h = h
        self._lib = L   # kept for interpreter shutdown, when module globals are already cleared
        self.device = device

    def __del__(self):
        if getattr(self, "_h", None):
            self._lib.pbccs_engine_destroy(self._h)
            self._h = None

    def set_concurrency(self, batches_in_flight):
        """Workspace slots = batches polished at the same time by polish_many (set before creating batches)."""
        _lib_mod.check(load().pbccs_engine_set_concurrency(self._h, int(batches_in_flight)))

    def reserve_pool(self, bytes_per_slot):
        """Map each workspace slot's band pool now (a one-time cost a long run pays once)."""
        _lib_mod.check(load().pbccs_engine_reserve_pool(self._h, int(bytes_per_slot)))

    def set_profiling(self, on=True):
        _lib_mod.check(load().pbccs_engine_set_profiling(self._h, 1 if on else 0))

    def kernel_stats(self, reset=False):
        arr = (_lib_mod.CKernelStat * 32)()
        n = ctypes.c_int()
        _lib_mod.check(load().pbccs_engine_kernel_stats(self._h, arr, 32, ctypes.byref(n), 1 if reset else 0))
        return {arr[i].name.decode(): {"launches": arr[i].launches, "device_ms": arr[i].device_ms,
                                       "cells": arr[i].cells, "bytes": arr[i].bytes, "wave_s": arr[i].wave_s}
                for i in range(n.value)}

    def counters(self, reset=False):
        c = _lib_mod.CCounters()
        _lib_mod.check(load().pbccs_engine_counters(self._h, ctypes.byref(c), 1 if reset else 0))
        return {k: (list(getattr(c, k)) if k in ("fill_work", "uncertain_why") else getattr(c, k))
                for k, _ in _lib_mod.CCounters._fields_}

    def diploid_stats(self, reset=False):
        """The diploid screen's work: sites_screened, sites_sent_to_host, sites_reported."""
        c = _lib_mod.CDiploidStats()
        _lib_mod.check(load().pbccs_diploid_stats_get(self._h, ctypes.byref(c), 1 if reset else 0))
        return {k: getattr(c, k) for k, _ in _lib_mod.CDiploidStats._fields_}


_default_engine = None


def default_engine():
    global _default_engine
    if _default_engine is None:
        _default_engine = Engine(int(os.environ.get("PBCCS_DEVICE", os.environ.get("LOCAL_RANK", "0"))))
    return _default_engine


class ArrowMultiReadMutationScorer:
    """ConsensusCore::Arrow::ArrowMultiReadMutationScorer on the GPU (MultiReadMutationScorer.hpp:82-284)."""

    def __init__(self, config, tpl, engine=None):
        self.engine = engine or default_engine()
        self.config = config
        h = ctypes.c_void_p()
        b = tpl.encode()
        _lib_mod.check(load().pbccs_scorer_create(self.engine._h, ctypes.byref(config._c()), b, len(b), ctypes.byref(h)))
        self._h = h

    def __del__(self):
        if getattr(self, "_h", None):
            load().pbccs_scorer_destroy(self._h)
            self._h = None

    def AddRead(self, seq, strand=FORWARD_STRAND, template_start=0, template_end=None, threshold=None):
        if template_end is None:
            template_end = self.TemplateLength()
        if threshold is None:
            threshold = self.config.add_threshold
        res = ctypes.c_int()
        b = seq.encode()
        _lib_mod.check(load().pbccs_scorer_add_read(self._h, b, len(b), strand, template_start, template_end,
                                                    float(threshold), ctypes.byref(res)))
        return res.value

    # wide=True: the pbccs_scorer_*_ex calls (k_score_wide), which take mutations of any width --
    # Mutation(type, pos, "AC") -- and single-base ones too, scored bit for bit as the default path scores them.
    # Without it a multi-base mutation is refused, as before.
    def Score(self, m, fast_score_threshold=-DBL_MAX, wide=False):
        if wide:
            return self.ScoreMany([m], fast_score_threshold, wide=True)[0]
        v = ctypes.c_double()
        _lib_mod.check(load().pbccs_scorer_score(self._h, ctypes.byref(m._c()), fast_score_threshold, ctypes.byref(v)))
        return v.value

    def FastScore(self, m, wide=False):
        return self.Score(m, self.config.fast_score_threshold, wide=wide)

    def ScoreMany(self, muts, fast_score_threshold=-DBL_MAX, wide=False):
        out = (ctypes.c_double * max(1, len(muts)))()
        if wide:
            cs = [m._cx() for m in muts]   # (the list keeps the base strings alive through the call)
            arr = (_lib_mod.CMutationEx * max(1, len(muts)))(*cs)
            _lib_mod.check(load().pbccs_scorer_score_many_ex(self._h, arr, len(muts), fast_score_threshold, out))
            return list(out[: len(muts)])
        arr = (_lib_mod.CMutation * max(1, len(muts)))(*[m._c() for m in muts])
        _lib_mod.check(load().pbccs_scorer_score_many(self._h, arr, len(muts), fast_score_threshold, out))
        return list(out[: len(muts)])

    def Scores(self, m, unscored_value=0.0, wide=False):
        out = (ctypes.c_double * max(1, self.NumReads()))()
        if wide:
            c = m._cx()
            _lib_mod.check(load().pbccs_scorer_scores_ex(self._h, ctypes.byref(c), unscored_value, out))
        else:
            _lib_mod.check(load().pbccs_scorer_scores(self._h, ctypes.byref(m._c()), unscored_value, out))
        return list(out[: self.NumReads()])

    def _favorable(self, m, fast, wide):
        f = ctypes.c_int()
        if wide:
            c = m._cx()
            _lib_mod.check(load().pbccs_scorer_is_favorable_ex(self._h, ctypes.byref(c), fast, ctypes.byref(f)))
        else:
            _lib_mod.check(load().pbccs_scorer_is_favorable(self._h, ctypes.byref(m._c()), fast, ctypes.byref(f)))
        return bool(f.value)

    def IsFavorable(self, m, wide=False):
        return self._favorable(m, 0, wide)

    def FastIsFavorable(self, m, wide=False):
        return self._favorable(m, 1, wide)

    def ApplyMutations(self, muts, wide=False):
        if wide:
            cs = [m._cx() for m in muts]
            arr = (_lib_mod.CMutationEx * max(1, len(muts)))(*cs)
            _lib_mod.check(load().pbccs_scorer_apply_mutations_ex(self._h, arr, len(muts)))
            return
        arr = (_lib_mod.CMutation * max(1, len(muts)))(*[m._c() for m in muts])
        _lib_mod.check(load().pbccs_scorer_apply_mutations(self._h, arr, len(muts)))

    def Template(self, strand=FORWARD_STRAND):
        n = ctypes.c_int()
        cap = self.TemplateLength() + 1
        buf = ctypes.create_string_buffer(cap)
        _lib_mod.check(load().pbccs_scorer_template(self._h, strand, buf, cap, ctypes.byref(n)))
        return buf.value.decode()

    def TemplateLength(self):
        return load().pbccs_scorer_template_length(self._h)

    def NumReads(self):
        return load().pbccs_scorer_num_reads(self._h)

    def ReadInfo(self, i):
        a, s, ts, te = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        _lib_mod.check(load().pbccs_scorer_read_info(self._h, i, ctypes.byref(a), ctypes.byref(s), ctypes.byref(ts),
                                                     ctypes.byref(te)))
        return {"active": bool(a.value), "strand": s.value, "template_start": ts.value, "template_end": te.value}

    def BaselineScore(self):
        v = ctypes.c_double()
        _lib_mod.check(load().pbccs_scorer_baseline_score(self._h, ctypes.byref(v)))
        return v.value

    def BaselineScores(self):
        out = (ctypes.c_double * max(1, self.NumReads()))()
        n = ctypes.c_int()
        _lib_mod.check(load().pbccs_scorer_baseline_scores(self._h, out, self.NumReads(), ctypes.byref(n)))
        return list(out[: n.value])

    def ZScores(self):
        zg, za = ctypes.c_double(), ctypes.c_double()
        out = (ctypes.c_double * max(1, self.NumReads()))()
        _lib_mod.check(load().pbccs_scorer_zscores(self._h, ctypes.byref(zg), ctypes.byref(za), out))
        return (zg.value, za.value), list(out[: self.NumReads()])

    def NumFlipFlops(self):
        out = (ctypes.c_int * max(1, self.NumReads()))()
        _lib_mod.check(load().pbccs_scorer_num_flipflops(self._h, out))
        return list(out[: self.NumReads()])

    def StrandScores(self, muts):
        """Per-strand sums of single-base mutations: StrandSums(sum_fwd, sum_rev, n_fwd, n_rev) per mutation, the
        sums of Scores(m, 0) per strand in read order, bit for bit (k_strand_sums)."""
        from . import strand
        return strand.scorer_strand_scores(self, muts)

    def StrandSites(self, min_score=12.5, min_reads=2):
        """The strand-discordant sites of the current template: StrandSite(pos, type, base, sum_fwd, sum_rev) in
        template order (the ConsensusQVs sweep, then k_strand_sums and k_strand_sites)."""
        from . import strand
        return strand.scorer_strand_sites(self, min_score, min_reads)

    def SiteScores(self, begin=0, end=None):
        """The site tensor of template positions [begin, end): float32 ndarray (sites, reads, 9), see diploid.py."""
        from . import diploid
        return diploid.site_scores(load().pbccs_scorer_site_scores, self._h, self.NumReads(), self.TemplateLength(),
                                   begin, end)

    def DiploidSites(self, log_prior_ratio, begin=0, end=None, host_all=False):
        """IsSiteHeterozygous at every position of [begin, end): the heterozygous DiploidSites, by Position."""
        from . import diploid
        return diploid.diploid_sites(load().pbccs_scorer_diploid_sites, self._h, self.NumReads(),
                                     self.TemplateLength(), log_prior_ratio, begin, end, host_all)


def RefineConsensus(mms, max_iterations=40, mutation_separation=10, mutation_neighborhood=20):
    """bool RefineConsensus(MRMS&, size_t* nTested, size_t* nApplied, const RefineOptions&) -> (converged, nT, nA).
    Templated on the scorer in the reference (Consensus.hpp:63-67): Arrow or Quiver scorers."""
    if isinstance(mms, _quiver.QuiverMultiReadMutationScorer):
        return _quiver.RefineConsensus(mms, max_iterations, mutation_separation, mutation_neighborhood)
    o = _lib_mod.CRefineOptions(max_iterations, mutation_separation, mutation_neighborhood)
    nt, na, conv = ctypes.c_longlong(0), ctypes.c_longlong(0), ctypes.c_int()
    _lib_mod.check(load().pbccs_refine_consensus(mms._h, ctypes.byref(o), ctypes.byref(nt), ctypes.byref(na),
                                                 ctypes.byref(conv)))
    return bool(conv.value), nt.value, na.value


def ConsensusQVs(mms):
    if isinstance(mms, _quiver.QuiverMultiReadMutationScorer):
        return _quiver.ConsensusQVs(mms)
    cap = mms.TemplateLength()
    out = (ctypes.c_int * max(1, cap))()
    n = ctypes.c_int()
    _lib_mod.check(load().pbccs_consensus_qvs(mms._h, out, cap, ctypes.byref(n)))
    return list(out[: n.value])


def QVsToASCII(qvs):
    """include/pacbio/ccs/Consensus.h:327-338"""
    return "".join(chr(min(max(0, q), 93) + 33) for q in qvs)


from .polish import (ConsensusSettings, PreparedBatch, plan_batches, polish_many, polish_stream,  # noqa: E402
                     polish_windowed, polish_zmws)  # batched ccs driver
from . import quiver as _quiver  # noqa: E402
from .quiver import (QvModelParams, QuiverConfig, QuiverConfigTable,  # noqa: E402,F401
                     QuiverMultiReadMutationScorer, QvEvaluator, QvSequenceFeatures, ALL_MOVES, BASIC_MOVES,
                     RepeatMutationEnumerator, DinucleotideRepeatMutationEnumerator)


def RefineRepeats(mms, repeat_length, min_repeat_elements=3, max_iterations=1, mutation_separation=10,
                  mutation_neighborhood=20):
    """RefineRepeats (Consensus.hpp:69-76): AbstractRefineConsensus over RepeatMutationEnumerator -> (converged, nT,
    nA).  Templated on the scorer in the reference: Quiver scorers (quiver.RefineRepeats) or Arrow scorers
    (pbccs_refine_repeats: k_score_wide, favourable = Score(m, FastScoreThreshold) > 0.04)."""
    if isinstance(mms, _quiver.QuiverMultiReadMutationScorer):
        return _quiver.RefineRepeats(mms, repeat_length, min_repeat_elements, max_iterations, mutation_separation,
                                     mutation_neighborhood)
    o = _lib_mod.CRepeatOptions(repeat_length, min_repeat_elements, max_iterations, mutation_separation,
                                mutation_neighborhood)
    nt, na, conv = ctypes.c_longlong(0), ctypes.c_longlong(0), ctypes.c_int()
    _lib_mod.check(load().pbccs_refine_repeats(mms._h, ctypes.byref(o), ctypes.byref(nt), ctypes.byref(na),
                                               ctypes.byref(conv)))
    return bool(conv.value), nt.value, na.value


def RefineDinucleotideRepeats(mms, min_elements=3):
    return RefineRepeats(mms, 2, min_elements)


def wide_columns_needed(m, strand, template_start, template_end):
    """The extension columns one read with window [template_start, template_end) on `strand` needs for mutation m
    on the Arrow scorer's wide path (host only): -1 the read does not score it, 0 the whole-window refill, -2 the
    mutated window would be empty; -2 and more than 8 are what the wide calls refuse."""
    c = m._cx()
    n = ctypes.c_int()
    _lib_mod.check(load().pbccs_wide_columns_needed(ctypes.byref(c), int(strand), int(template_start),
                                                    int(template_end), ctypes.byref(n)))
    return n.value
from .diploid import DiploidSite, IsSiteHeterozygous  # noqa: E402,F401
from .richqv import ConsensusRichQVs, rich_feature_tracks  # noqa: E402,F401
from .align import (AffineAlignmentParams, Align, AlignAffine, AlignAffineIupac, AlignConfig,  # noqa: E402,F401
                    AlignParams, DefaultAffineAlignmentParams, IupacAwareAffineAlignmentParams, PairwiseAlignment,
                    TargetToQueryPositions, UnsupportedFeatureError, align_band_stats, align_batch, align_stats)
from .align import AlignLocal, AlignSemiglobal, align_ends_batch  # noqa: E402,F401
from .mapping import (map_batch, map_stats, map_to_draft, split_map_batch, split_map_stats,  # noqa: E402,F401
                      split_map_to_draft)
from .sparse import SparseAlign, sparse_align_batch, sparse_align_stats  # noqa: E402,F401
from .strand import StrandSite, StrandSums, strand_stats  # noqa: E402,F401
from .kinetics import (codec_v1_decode, codec_v1_encode, kinetics_batch, kinetics_pileup,  # noqa: E402,F401
                       kinetics_stats)
from .pileup import pileup_batch, pileup_columns, pileup_msa, pileup_stats  # noqa: E402,F401
from .demux import BarcodeSet, clip_read, demux_batch, demux_stats  # noqa: E402,F401

__all__ = [
    "ArrowConfig", "ArrowMultiReadMutationScorer", "ConsensusQVs", "ConsensusSettings", "Engine", "Mutation",
    "PbccsError", "QVsToASCII", "RefineConsensus", "polish_many", "polish_zmws", "polish_stream", "polish_windowed", "plan_batches", "INSERTION", "DELETION", "SUBSTITUTION",
    "FORWARD_STRAND", "REVERSE_STRAND",
]

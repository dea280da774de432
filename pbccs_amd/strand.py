"""Directional consensus: the strand-discordance screen and the per-strand polish.

Rules of this project's own: the reference declares ConsensusSettings::Directional and stops at a TODO
(include/pacbio/ccs/Consensus.h:94-109).  For a single-base mutation m of the final template, sum_fwd / sum_rev are
the sums of Scores(m, 0) over the active forward / reverse reads that score m, in AddRead order.  m qualifies when at
least min_reads reads of each strand score it and one sum lies above min_score while the other lies below
-min_score; a position with a qualifying mutation is a discordant site and reports the qualifying mutation with the
largest min(|sum_fwd|, |sum_rev|), the first in enumeration order on a tie.
"""
import collections
import ctypes

from . import lib as L

StrandSite = collections.namedtuple("StrandSite", "pos type base sum_fwd sum_rev")
StrandSums = collections.namedtuple("StrandSums", "sum_fwd sum_rev n_fwd n_rev")
DIRECTIONAL = {None: 0, "discordant": 1, "always": 2}
SUB_KEYS = ("fwd", "rev")


def strand_options(strand_sites=True, directional=None):
    """pbccs_strand_options from the batch keywords: strand_sites True or a dict with any of min_score, min_reads,
    min_sites; directional None, "discordant" or "always"."""
    if directional not in DIRECTIONAL:
        raise ValueError('directional: None, "discordant" or "always"')
    o = L.CStrandOptions()
    L.load().pbccs_strand_options_default(ctypes.byref(o))
    if isinstance(strand_sites, dict):
        for k, v in strand_sites.items():
            if k not in ("min_score", "min_reads", "min_sites"):
                raise ValueError(f"strand_sites: unknown option {k}")
            setattr(o, k, float(v) if k == "min_score" else int(v))
    o.directional = DIRECTIONAL[directional]
    return o


def scorer_strand_scores(mms, muts):
    """The per-strand sums of single-base mutations on an Arrow scorer (pbccs_scorer_strand_scores): one StrandSums
    per mutation, bit-equal to summing Scores(m, 0) per strand in read order."""
    n = len(muts)
    arr = (L.CMutation * max(1, n))(*[m._c() for m in muts])
    sf, sr = (ctypes.c_double * max(1, n))(), (ctypes.c_double * max(1, n))()
    nf, nr = (ctypes.c_int * max(1, n))(), (ctypes.c_int * max(1, n))()
    L.check(L.load().pbccs_scorer_strand_scores(mms._h, arr, n, sf, sr, nf, nr))
    return [StrandSums(sf[i], sr[i], nf[i], nr[i]) for i in range(n)]


def scorer_strand_sites(mms, min_score=12.5, min_reads=2):
    """The discordant sites of an Arrow scorer's current template (pbccs_scorer_strand_sites), in template order."""
    o = strand_options({"min_score": min_score, "min_reads": min_reads})
    cap = mms.TemplateLength()
    b = SiteBuffers([cap])
    r = b.arr[0]
    n = ctypes.c_int()
    L.check(L.load().pbccs_scorer_strand_sites(mms._h, ctypes.byref(o), r.position, r.type, r.base, r.sum_fwd,
                                               r.sum_rev, cap, ctypes.byref(n)))
    r.n_sites = n.value
    return b.sites(0)


class SiteBuffers:
    """A pbccs_strand_result array for n ZMWs and the buffers it points at: caps[i] site entries for ZMW i, and for
    its two per-strand records a consensus of caps[i] bytes and per-read arrays of n_reads[i] entries."""

    def __init__(self, caps, n_reads=None):
        n = len(caps)
        self.arr = (L.CStrandResult * max(1, n))()
        self.n_reads = list(n_reads) if n_reads is not None else [0] * n
        self._keep = []
        for i, cap in enumerate(caps):
            cap = max(1, int(cap))
            nr = max(1, self.n_reads[i])
            ints = [(ctypes.c_int * cap)() for _ in range(2)]
            base = ctypes.create_string_buffer(cap)
            sums = [(ctypes.c_double * cap)() for _ in range(2)]
            r = self.arr[i]
            r.position, r.type = ints
            r.base = ctypes.cast(base, ctypes.POINTER(ctypes.c_char))
            r.sum_fwd, r.sum_rev = sums
            r.cap = cap
            subs = []
            for o in (r.fwd, r.rev) if n_reads is not None else ():
                cons = ctypes.create_string_buffer(cap)
                qv = (ctypes.c_int * cap)()
                arr = (ctypes.c_int * nr)()
                zs = (ctypes.c_double * nr)()
                o.consensus = ctypes.cast(cons, ctypes.c_char_p)
                o.consensus_cap = cap
                o.qvs = qv
                o.add_read_results = arr
                o.zscores = zs
                subs.append((cons, qv, arr, zs))
            self._keep.append((ints, base, sums, subs))

    def sites(self, i):
        r = self.arr[i]
        if r.n_sites < 0:
            raise L.PbccsError(-5, "strand sites outgrew their buffers")
        ints, base, sums, _ = self._keep[i]
        return [StrandSite(ints[0][k], ints[1][k], base.raw[k:k + 1].decode(), sums[0][k], sums[1][k])
                for k in range(r.n_sites)]

    def sub_records(self, i):
        """{"fwd": record, "rev": record} of a split ZMW (records as polish_zmws'), {} otherwise."""
        from . import ZMW_STATUS
        r = self.arr[i]
        if not r.split:
            return {}
        out = {}
        nr = self.n_reads[i]
        for key, o, (cons, qv, arr, zs) in zip(SUB_KEYS, (r.fwd, r.rev), self._keep[i][3]):
            ln = max(0, o.consensus_len)
            ok = o.status in (0, 6)
            out[key] = {
                "status": ZMW_STATUS[o.status], "status_code": o.status,
                "consensus": cons.raw[:ln].decode() if ok else "", "qvs": list(qv[:ln]) if ok else [],
                "add_read_results": list(arr[:nr]), "zscores": list(zs[:nr]), "zg": o.zg, "za": o.za,
                "predicted_accuracy": o.predicted_accuracy, "n_tested": o.n_tested, "n_applied": o.n_applied,
                "n_passes": o.n_passes, "status_counts": list(o.status_counts),
            }
        return out


def strand_stats(engine=None, reset=False):
    """The screen's work since the last reset (pbccs_strand_stats_get)."""
    from . import default_engine
    engine = engine or default_engine()
    s = L.CStrandStats()
    L.check(L.load().pbccs_strand_stats_get(engine._h, ctypes.byref(s), 1 if reset else 0))
    return {k: getattr(s, k) for k, _ in L.CStrandStats._fields_}

"""Pairwise alignment on the GPU: the Python mirror of ConsensusCore's Align/ (PairwiseAlignment.hpp,
AffineAlignment.hpp, AlignConfig.hpp) over the C ABI's pbccs_align_batch.

Align (Needleman-Wunsch, int32), AlignAffine and AlignAffineIupac (two-state affine, float32) run in HIP
(k_align_fill / k_align_trace), bit-exact with the reference: ties and the traceback come out the same.
PairwiseAlignment, FromTranscript and TargetToQueryPositions are host-side value code.  There is no CPU
fallback for the aligners: without the library or a GPU they raise.  AlignLinear is not provided.

band= on align_batch and the three aligners turns on the certified banded fill: long,
near-identical pairs are filled inside a band of diagonals and the answer is returned only when the banded score
certifies that it is the full fill's; every other pair takes the full fill.  Off by default."""
import ctypes
import math

from . import lib as _L
from .lib import load

GLOBAL, SEMIGLOBAL, LOCAL = 0, 1, 2
NW, AFFINE, AFFINE_IUPAC = 0, 1, 2


class InvalidInputError(ValueError):
    """ConsensusCore::InvalidInputError"""


class UnsupportedFeatureError(NotImplementedError):
    """ConsensusCore::UnsupportedFeatureError"""


class AlignParams:
    """AlignConfig.hpp: AlignParams(Match, Mismatch, Insert, Delete); Default() is edit distance."""

    def __init__(self, match=0, mismatch=-1, insert=-1, delete=-1):
        self.Match, self.Mismatch, self.Insert, self.Delete = int(match), int(mismatch), int(insert), int(delete)

    @staticmethod
    def Default():
        return AlignParams(0, -1, -1, -1)


class AlignConfig:
    def __init__(self, params=None, mode=GLOBAL):
        self.Params = params if params is not None else AlignParams.Default()
        self.Mode = mode

    @staticmethod
    def Default():
        return AlignConfig(AlignParams.Default(), GLOBAL)


class AffineAlignmentParams:
    def __init__(self, match_score, mismatch_score, gap_open, gap_extend, partial_match_score=0.0):
        self.MatchScore = float(match_score)
        self.MismatchScore = float(mismatch_score)
        self.GapOpen = float(gap_open)
        self.GapExtend = float(gap_extend)
        self.PartialMatchScore = float(partial_match_score)

    def _values(self):
        return (self.MatchScore, self.MismatchScore, self.GapOpen, self.GapExtend, self.PartialMatchScore)


def DefaultAffineAlignmentParams():
    return AffineAlignmentParams(0, -1.0, -1.0, -0.5, 0)


def IupacAwareAffineAlignmentParams():
    return AffineAlignmentParams(0, -1.0, -1.0, -0.5, -0.25)


class PairwiseAlignment:
    """ConsensusCore::PairwiseAlignment (PairwiseAlignment.cpp:51-123): gapped target and query of equal length and
    Gusfield's transcript (M match, R mismatch, I target gap, D query gap)."""

    def __init__(self, target, query):
        if len(target) != len(query):
            raise InvalidInputError("target and query differ in length")
        tr = []
        for t, q in zip(target, query):
            if t == "-" and q == "-":
                raise InvalidInputError("gap aligned to gap")
            tr.append("M" if t == q else "I" if t == "-" else "D" if q == "-" else "R")
        self._target, self._query, self._transcript = target, query, "".join(tr)

    def Target(self):
        return self._target

    def Query(self):
        return self._query

    def Transcript(self):
        return self._transcript

    def Length(self):
        return len(self._target)

    def Matches(self):
        return self._transcript.count("M")

    def Errors(self):
        return self.Length() - self.Matches()

    def Mismatches(self):
        return self._transcript.count("R")

    def Insertions(self):
        return self._transcript.count("I")

    def Deletions(self):
        return self._transcript.count("D")

    def Accuracy(self):
        return self.Matches() / self.Length() if self.Length() else float("nan")

    @staticmethod
    def FromTranscript(transcript, unaln_target, unaln_query):
        """The alignment the transcript spells over the two sequences, or None where it does not map the target
        onto the query (PairwiseAlignment.cpp:309-368)."""
        t_len, q_len = len(unaln_target), len(unaln_query)
        tp = qp = 0
        at, aq = [], []
        for x in transcript:
            if tp > t_len or qp > q_len:
                return None
            t = unaln_target[tp] if tp < t_len else "\0"
            q = unaln_query[qp] if qp < q_len else "\0"
            if x == "M" or x == "R":
                if (t == q) != (x == "M"):
                    return None
                at.append(t)
                aq.append(q)
                tp += 1
                qp += 1
            elif x == "I":
                at.append("-")
                aq.append(q)
                qp += 1
            elif x == "D":
                at.append(t)
                aq.append("-")
                tp += 1
            else:
                return None
        if tp != t_len or qp != q_len:
            return None
        return PairwiseAlignment("".join(at), "".join(aq))

    def __repr__(self):
        return f"PairwiseAlignment({self._target!r}, {self._query!r})"

    def __eq__(self, o):
        return isinstance(o, PairwiseAlignment) and (self._target, self._query) == (o._target, o._query)

    def __hash__(self):
        return hash((self._target, self._query))


def TargetToQueryPositions(transcript):
    """For each target position (and one past the end) the query position the alignment maps it to
    (PairwiseAlignment.cpp:264-303).  Takes a transcript string or a PairwiseAlignment."""
    if isinstance(transcript, PairwiseAlignment):
        transcript = transcript.Transcript()
    ntp = []
    qp = 0
    for c in transcript:
        if c == "M" or c == "R":
            ntp.append(qp)
            qp += 1
        elif c == "D":
            ntp.append(qp)
        elif c == "I":
            qp += 1
        else:
            raise InvalidInputError(f"not a transcript character: {c!r}")
    ntp.append(qp)
    return ntp


def _c_params(kind, params):
    """Validates on the host (before any engine is touched) and returns the C struct."""
    c = _L.CAlignParams()
    c.kind = kind
    c.mode = GLOBAL
    if kind == NW:
        cfg = params if params is not None else AlignConfig.Default()
        if isinstance(cfg, AlignParams):
            cfg = AlignConfig(cfg, GLOBAL)
        if cfg.Mode != GLOBAL:
            raise UnsupportedFeatureError("Only GLOBAL alignment supported at present")
        c.mode = cfg.Mode
        c.match, c.mismatch, c.insert, c.delete_ = (cfg.Params.Match, cfg.Params.Mismatch, cfg.Params.Insert,
                                                      cfg.Params.Delete)
    elif kind in (AFFINE, AFFINE_IUPAC):
        if params is None:
            params = DefaultAffineAlignmentParams() if kind == AFFINE else IupacAwareAffineAlignmentParams()
        vals = params._values()
        if not all(math.isfinite(v) for v in vals):
            raise InvalidInputError("affine alignment parameters must be finite")
        c.match_score, c.mismatch_score, c.gap_open, c.gap_extend, c.partial_match_score = vals
    else:
        raise InvalidInputError(f"unknown alignment kind {kind!r}")
    return c


def _encode(s):
    return s if isinstance(s, bytes) else s.encode("latin-1")


BAND_REASONS = ("certified", "not_certifiable", "covers_matrix", "store_not_smaller", "trace_flagged", "uncertified",
                "degenerate", "over_budget")


def _c_band(band):
    """band=None / False: off; True: automatic first half-width; an int w >= 0: first half-width w."""
    if band is None or band is False:
        return None
    b = _L.CAlignBand()
    if band is True:
        b.mode, b.w = 1, 0
    else:
        w = int(band)
        if w < 0:
            raise InvalidInputError("band half-width must be >= 0")
        b.mode, b.w = 2, min(w, 2**31 - 1)
    return b


def align_band_bound(kind, query_len, target_len, w, params=None):
    """(U(w), E, certifiable) of the band certificate for a pair of query_len rows and target_len columns: every
    path that leaves the band of half-width w scores at most U + E.  Host code: no engine, no GPU."""
    c = _c_params(kind, params)
    u, e, ok = ctypes.c_double(), ctypes.c_double(), ctypes.c_int()
    _L.check(load().pbccs_align_band_bound(ctypes.byref(c), int(query_len), int(target_len), int(w), ctypes.byref(u),
                                           ctypes.byref(e), ctypes.byref(ok)))
    return u.value, e.value, bool(ok.value)


def align_band_widen(kind, query_len, target_len, score, params=None):
    """The smallest half-width that a banded score certifies, or -1.  Host code: no engine, no GPU."""
    c = _c_params(kind, params)
    w = ctypes.c_int()
    _L.check(load().pbccs_align_band_widen(ctypes.byref(c), int(query_len), int(target_len), float(score),
                                           ctypes.byref(w)))
    return w.value


def align_batch_raw(pairs, kind, params=None, engine=None, caps=None, band=None, info=None):
    """pbccs_align_batch as it stands: (return code, [(transcript, score, status, len) per pair]).  pairs are
    (target, query) strings; caps overrides the transcript capacities (default target + query lengths).
    Marshalling is flat: one blob with pointer tables and one shared transcript buffer.  band: see _c_band; info:
    a list that receives one {"banded", "w", "attempts", "reason"} per pair of a banded call."""
    import numpy as np
    from .quiver import _struct_dtype
    c = _c_params(kind, params)
    if engine is None:
        from . import default_engine
        engine = default_engine()
    n = len(pairs)
    enc = [_encode(s) for p in pairs for s in p]
    lens = np.fromiter((len(e) for e in enc), dtype=np.int64, count=2 * n)
    blob = ctypes.create_string_buffer(b"".join(enc), max(1, int(lens.sum())))
    starts = np.zeros(2 * n + 1, dtype=np.int64)
    np.cumsum(lens, out=starts[1:])
    ptrs = (ctypes.addressof(blob) + starts[:-1]).astype(np.uint64)
    cap = (lens[0::2] + lens[1::2]) if caps is None else np.asarray(caps, dtype=np.int64)
    ostart = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(cap, out=ostart[1:])
    obuf = ctypes.create_string_buffer(max(1, int(ostart[-1])))
    ins = np.zeros(max(1, n), dtype=_struct_dtype(_L.CAlignPair))
    outs = np.zeros(max(1, n), dtype=_struct_dtype(_L.CAlignResult))
    if n:
        ins["target"][:n] = ptrs[0::2]
        ins["target_len"][:n] = lens[0::2]
        ins["query"][:n] = ptrs[1::2]
        ins["query_len"][:n] = lens[1::2]
        outs["transcript"][:n] = ctypes.addressof(obuf) + ostart[:-1]
        outs["cap"][:n] = cap
    cb = _c_band(band)
    if cb is None:
        rc = load().pbccs_align_batch(engine._h, ctypes.byref(c),
                                      ctypes.cast(ins.ctypes.data, ctypes.POINTER(_L.CAlignPair)), n,
                                      ctypes.cast(outs.ctypes.data, ctypes.POINTER(_L.CAlignResult)))
    else:
        binfo = (_L.CAlignBandInfo * max(1, n))()
        rc = load().pbccs_align_batch_ex(engine._h, ctypes.byref(c),
                                         ctypes.cast(ins.ctypes.data, ctypes.POINTER(_L.CAlignPair)), n,
                                         ctypes.cast(outs.ctypes.data, ctypes.POINTER(_L.CAlignResult)),
                                         ctypes.byref(cb), binfo)
        if info is not None:
            info[:] = [{"banded": bool(binfo[k].banded), "w": binfo[k].w, "attempts": binfo[k].attempts,
                        "reason": BAND_REASONS[binfo[k].reason]} for k in range(n)]
    raw = obuf.raw
    os_, ln, caps_l, st = ostart.tolist(), outs["len"][:n].tolist(), cap.tolist(), outs["status"][:n].tolist()
    score = outs["score_i"][:n].tolist() if kind == NW else outs["score_f"][:n].tolist()
    res = []
    for k in range(n):
        tr = raw[os_[k]:os_[k] + ln[k]].decode("latin-1") if st[k] == 0 and ln[k] <= caps_l[k] else None
        res.append((tr, score[k], st[k], ln[k]))
    return rc, res


def _from_device_transcript(tr, target, query):
    """FromTranscript for the batch path, column-wise in numpy instead of a per-character Python loop.  The same
    refusals: None unless the transcript maps the target onto the query."""
    import numpy as np
    x = np.frombuffer(tr.encode("latin-1"), dtype=np.uint8)
    t = np.frombuffer(_encode(target), dtype=np.uint8)
    q = np.frombuffer(_encode(query), dtype=np.uint8)
    on_t, on_q = x != ord("I"), x != ord("D")
    if int(on_t.sum()) != len(t) or int(on_q.sum()) != len(q) or not np.isin(x, np.frombuffer(b"MRID", np.uint8)).all():
        return None
    at = np.full(len(x), ord("-"), dtype=np.uint8)
    aq = np.full(len(x), ord("-"), dtype=np.uint8)
    at[on_t] = t
    aq[on_q] = q
    both = on_t & on_q
    if not ((at == aq)[both] == (x == ord("M"))[both]).all():
        return None
    a = PairwiseAlignment.__new__(PairwiseAlignment)
    a._target, a._query, a._transcript = at.tobytes().decode("latin-1"), aq.tobytes().decode("latin-1"), tr
    return a


def align_batch(pairs, kind, params=None, engine=None, band=None, return_info=False):
    """Aligns many (target, query) pairs in one call.  kind: NW (params: AlignConfig), AFFINE or AFFINE_IUPAC
    (params: AffineAlignmentParams).  Returns ([PairwiseAlignment], [score]) in input order; the score is
    Score(I, J) (int) for NW and max(M, GAP)(I, J) (float32 value) for the affine kinds.  band=True (automatic
    first half-width) or band=w turns on the certified banded fill, whose answers are the full fill's;
    return_info=True appends the per-pair records (banded, w, attempts, reason) as a third value."""
    info = []
    rc, res = align_batch_raw(pairs, kind, params, engine, band=band, info=info)
    _L.check(rc)
    alns = []
    for (t, q), (tr, _, _, _) in zip(pairs, res):
        a = _from_device_transcript(tr, t, q)
        if a is None:
            raise _L.PbccsError(-3, "the device returned a transcript that does not map the target onto the query")
        alns.append(a)
    if return_info:
        if not info:
            info = [{"banded": False, "w": 0, "attempts": 0, "reason": "certified"} for _ in pairs]
        return alns, [r[1] for r in res], info
    return alns, [r[1] for r in res]


def Align(target, query, config=None, return_score=False, engine=None, band=None):
    """PairwiseAlignment* Align(target, query, int* score, AlignConfig) (PairwiseAlignment.cpp:125-212)."""
    alns, scores = align_batch([(target, query)], NW, config, engine, band=band)
    return (alns[0], scores[0]) if return_score else alns[0]


def AlignAffine(target, query, params=None, engine=None, band=None):
    """AlignAffine(target, query, AffineAlignmentParams = DefaultAffineAlignmentParams())."""
    return align_batch([(target, query)], AFFINE, params, engine, band=band)[0][0]


def AlignAffineIupac(target, query, params=None, engine=None, band=None):
    """AlignAffineIupac(target, query, AffineAlignmentParams = IupacAwareAffineAlignmentParams())."""
    return align_batch([(target, query)], AFFINE_IUPAC, params, engine, band=band)[0][0]


def _c_ends(mode, params, both_strands, kind, band):
    """The refusals of the ends-free modes, all on the host (before any engine is touched), and the C structs."""
    if kind != NW or isinstance(params, AffineAlignmentParams):
        raise UnsupportedFeatureError("SEMIGLOBAL and LOCAL alignment are defined for the linear (NW) scores only")
    if not (band is None or band is False):
        raise UnsupportedFeatureError("the certified band is GLOBAL only: it cannot be combined with a mode")
    if mode == GLOBAL:
        raise InvalidInputError("GLOBAL alignment is Align's / align_batch's")
    if mode not in (SEMIGLOBAL, LOCAL):
        raise InvalidInputError(f"unknown alignment mode {mode!r}")
    if isinstance(params, AlignConfig):
        params = params.Params
    if params is None:
        params = AlignParams.Default()
    if params.Insert > 0 or params.Delete > 0:
        raise InvalidInputError("SEMIGLOBAL and LOCAL alignment need Insert <= 0 and Delete <= 0")
    c = _L.CAlignParams()
    c.kind, c.mode = NW, mode
    c.match, c.mismatch, c.insert, c.delete_ = params.Match, params.Mismatch, params.Insert, params.Delete
    e = _L.CAlignEnds()
    e.mode, e.both_strands = mode, 1 if both_strands else 0
    return c, e


def align_ends_batch(pairs, mode, params=None, both_strands=False, engine=None, kind=NW, band=None):
    """Ends-free alignment of many (target, query) pairs in one call: mode SEMIGLOBAL (the whole
    query inside the target: the target's ends are free) or LOCAL (the best pair of substrings).  The rules are the
    reference POA's on a graph that holds the target as one unbranched path, with the int32 AlignParams (params;
    default edit distance): candidates (LOCAL: Start,) diagonal, Delete, Extra, a later one only when strictly
    greater; end cell the smallest target column, then the smallest query row, holding the maximum.

    Returns ([PairwiseAlignment of the two substrings], [score], [extent]); an extent is {"target": (b, e),
    "query": (b, e), "rc"}.  both_strands also aligns the reverse complement of the query and keeps the forward
    answer iff its score >= the other's; "query" is then in the coordinates of the sequence that was aligned, as
    map_batch's "read".  Refused: Insert > 0 or Delete > 0 and mode GLOBAL (InvalidInputError); an affine kind or
    band= (UnsupportedFeatureError)."""
    import numpy as np
    from .quiver import _struct_dtype
    c, e = _c_ends(mode, params, both_strands, kind, band)
    if engine is None:
        from . import default_engine
        engine = default_engine()
    n = len(pairs)
    enc = [_encode(s) for p in pairs for s in p]
    lens = np.fromiter((len(x) for x in enc), dtype=np.int64, count=2 * n)
    blob = ctypes.create_string_buffer(b"".join(enc), max(1, int(lens.sum())))
    starts = np.zeros(2 * n + 1, dtype=np.int64)
    np.cumsum(lens, out=starts[1:])
    ptrs = (ctypes.addressof(blob) + starts[:-1]).astype(np.uint64)
    cap = lens[0::2] + lens[1::2]
    ostart = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(cap, out=ostart[1:])
    obuf = ctypes.create_string_buffer(max(1, int(ostart[-1])))
    ins = np.zeros(max(1, n), dtype=_struct_dtype(_L.CAlignPair))
    outs = np.zeros(max(1, n), dtype=_struct_dtype(_L.CAlignResult))
    exts = np.zeros(max(1, n), dtype=_struct_dtype(_L.CAlignExtent))
    if n:
        ins["target"][:n] = ptrs[0::2]
        ins["target_len"][:n] = lens[0::2]
        ins["query"][:n] = ptrs[1::2]
        ins["query_len"][:n] = lens[1::2]
        outs["transcript"][:n] = ctypes.addressof(obuf) + ostart[:-1]
        outs["cap"][:n] = cap
    _L.check(load().pbccs_align_batch_ends(engine._h, ctypes.byref(c), ctypes.byref(e),
                                           ctypes.cast(ins.ctypes.data, ctypes.POINTER(_L.CAlignPair)), n,
                                           ctypes.cast(outs.ctypes.data, ctypes.POINTER(_L.CAlignResult)),
                                           ctypes.cast(exts.ctypes.data, ctypes.POINTER(_L.CAlignExtent))))
    raw = obuf.raw
    os_, ln, score = ostart.tolist(), outs["len"][:n].tolist(), outs["score_i"][:n].tolist()
    tb, te = exts["target_begin"][:n].tolist(), exts["target_end"][:n].tolist()
    qb, qe, rc = exts["query_begin"][:n].tolist(), exts["query_end"][:n].tolist(), exts["rc"][:n].tolist()
    alns, extents = [], []
    for k, (t, q) in enumerate(pairs):
        tr = raw[os_[k]:os_[k] + ln[k]].decode("latin-1")
        if rc[k]:
            q = reverse_complement(q)
        a = _from_device_transcript(tr, t[tb[k]:te[k]], q[qb[k]:qe[k]])
        if a is None:
            raise _L.PbccsError(-3, "the device returned a transcript that does not map the target onto the query")
        alns.append(a)
        extents.append({"target": (tb[k], te[k]), "query": (qb[k], qe[k]), "rc": bool(rc[k])})
    return alns, score, extents


def _complement_table():
    t = bytearray([127]) * 256   # ComplementArray's value for every byte it does not name
    for a, b in zip(b"ACGTacgtNMnm-\x00\x01\x02\x03", b"TGCAtgcaMNmn-\x03\x02\x01\x00"):
        t[a] = b
    return bytes(t)


_COMPLEMENT = _complement_table()


def reverse_complement(seq):
    """ConsensusCore::ReverseComplement (Sequence.cpp's ComplementArray; note N <-> M): the sequence both_strands
    aligns, and the one an rc extent's "query" indexes."""
    out = _encode(seq)[::-1].translate(_COMPLEMENT)
    return out if isinstance(seq, bytes) else out.decode("latin-1")


def AlignSemiglobal(target, query, params=None, both_strands=False, engine=None, kind=NW, band=None):
    """The whole query placed inside the target (the target's ends are free): (alignment of target[b:e] and the
    query, score, extent).  See align_ends_batch."""
    a, s, x = align_ends_batch([(target, query)], SEMIGLOBAL, params, both_strands, engine, kind, band)
    return a[0], s[0], x[0]


def AlignLocal(target, query, params=None, both_strands=False, engine=None, kind=NW, band=None):
    """The best local match of the two sequences: (alignment of the two substrings, score, extent).  See
    align_ends_batch."""
    a, s, x = align_ends_batch([(target, query)], LOCAL, params, both_strands, engine, kind, band)
    return a[0], s[0], x[0]


def align_stats(engine=None, reset=False):
    if engine is None:
        from . import default_engine
        engine = default_engine()
    s = _L.CAlignStats()
    _L.check(load().pbccs_align_stats_get(engine._h, ctypes.byref(s), 1 if reset else 0))
    return {k: getattr(s, k) for k, _ in _L.CAlignStats._fields_}


def align_band_stats(engine=None, reset=False):
    """Banded-fill work since the last reset; fallbacks is a dict by reason."""
    if engine is None:
        from . import default_engine
        engine = default_engine()
    s = _L.CAlignBandStats()
    _L.check(load().pbccs_align_band_stats_get(engine._h, ctypes.byref(s), 1 if reset else 0))
    d = {k: getattr(s, k) for k, _ in _L.CAlignBandStats._fields_ if k != "fallbacks"}
    d["fallbacks"] = {BAND_REASONS[k]: s.fallbacks[k] for k in range(1, len(BAND_REASONS))}
    return d

"""Barcode demultiplexing on the GPU: which barcode pair flanks a CCS read.

Every barcode is placed inside a window at each end of every read by the SEMIGLOBAL rules of align.align_ends_batch
(the barcode is the query, the window the target; the trailing end takes the barcode's reverse complement), on the
device in one call for all reads and barcodes (k_demux_score, k_demux_call, k_demux_extent).  The reference has no
demultiplexing: the rules are this project's own, stated in full in tests/demux_restatement.py.  The SAM / BAM tags
that carry a call (bc, bq, bx) follow PacBio's BAM convention as published; they are restated and unpinned.
"""
import ctypes

from . import lib as _L
from .align import AlignConfig, AlignParams, InvalidInputError
from .lib import load

MAX_BARCODES, MAX_BARCODE_LEN, MAX_WINDOW = 65535, 64, 1024
# the midpoint of the measured null (64) and planted (84) qualities: profiles/demux.json, DESIGN.md §3.27
MIN_QUALITY = 74
DESIGNS = {"asymmetric": 0, "symmetric": 1}
INT_MIN, INT_MAX = -2**31, 2**31 - 1


def default_params():
    """DefaultPoaConfig's scores (Match 3, Mismatch -5, Insert -4, Delete -4), as mapping.map_batch uses them."""
    return AlignParams(3, -5, -4, -4)


class BarcodeSet:
    """B barcodes, 1 <= B <= 65535, each 1..64 bases of uppercase ACGT (anything else: InvalidInputError).  Names
    are optional; duplicate sequences are allowed (the smaller index wins a tie)."""

    def __init__(self, seqs, names=None):
        seqs = [s.decode("latin-1") if isinstance(s, bytes) else str(s) for s in seqs]
        if not 1 <= len(seqs) <= MAX_BARCODES:
            raise InvalidInputError(f"a barcode set holds 1 to {MAX_BARCODES} barcodes, not {len(seqs)}")
        for k, s in enumerate(seqs):
            if not 1 <= len(s) <= MAX_BARCODE_LEN:
                raise InvalidInputError(f"barcode {k} has {len(s)} bases (1 to {MAX_BARCODE_LEN})")
            if s.strip("ACGT"):
                raise InvalidInputError(f"barcode {k} holds a character other than uppercase A, C, G, T")
        if names is not None:
            names = [str(x) for x in names]
            if len(names) != len(seqs):
                raise InvalidInputError("one name per barcode")
        self.seqs = seqs
        self.names = names
        self.longest = max(len(s) for s in seqs)

    @classmethod
    def from_fasta(cls, path):
        from .ccsio import read_fasta
        recs = read_fasta(path)
        return cls([s for _, s in recs], [n for n, _ in recs])

    def __len__(self):
        return len(self.seqs)

    def name(self, k):
        return self.names[k] if self.names is not None else str(k)

    def _c(self):
        """(pbccs_demux_barcodes, the buffers it points into)."""
        enc = [s.encode() for s in self.seqs]
        ptrs = (ctypes.c_char_p * len(enc))(*enc)
        lens = (ctypes.c_int * len(enc))(*[len(s) for s in enc])
        return _L.CDemuxBarcodes(ptrs, lens, len(enc)), (enc, ptrs, lens)


def _options(barcodes, params, design, window, window_mult, min_quality, min_score_lead):
    """The checked pbccs_demux_options: every refusal is raised here, before an engine exists."""
    if not isinstance(barcodes, BarcodeSet):
        barcodes = BarcodeSet(barcodes)
    if isinstance(params, AlignConfig):
        params = params.Params
    if params is None:
        params = default_params()
    if params.Match <= 0 or params.Insert > 0 or params.Delete > 0:
        raise InvalidInputError("demux needs Match > 0, Insert <= 0 and Delete <= 0")
    if design not in DESIGNS:
        raise InvalidInputError(f"unknown design {design!r} (asymmetric or symmetric)")
    W = int(window) if window is not None else int(window_mult) * barcodes.longest
    if not 1 <= W <= MAX_WINDOW:
        raise InvalidInputError(f"the demux window is 1 to {MAX_WINDOW} bases, not {W}")
    mx = max(abs(params.Match), abs(params.Mismatch), abs(params.Insert), abs(params.Delete))
    if 2 * (barcodes.longest + W) * mx > INT_MAX:
        raise InvalidInputError("demux scores could leave int32")
    q = MIN_QUALITY if min_quality is None else int(min_quality)
    if q < 0:
        raise InvalidInputError("min_quality >= 0")
    o = _L.CDemuxOptions(params.Match, params.Mismatch, params.Insert, params.Delete, DESIGNS[design], W, 0, q,
                         int(min_score_lead))
    return barcodes, o


def _entries(n, out):
    """The per-read dicts from the flat output arrays (numpy int32)."""
    lead, trail, called = out["lead"].tolist(), out["trail"].tolist(), out["called"].tolist()
    score, sl, q = out["score"].tolist(), out["score_lead"].tolist(), out["quality"].tolist()
    ext, clip, over, best = out["extents"].tolist(), out["clip"].tolist(), out["overlap"].tolist(), out["best"].tolist()
    res = []
    for r in range(n):
        i, j = lead[r], trail[r]
        b = best[6 * r:6 * r + 6]
        res.append({"lead": i, "trail": j, "pair": (min(i, j), max(i, j)) if called[r] else (-1, -1),
                    "called": bool(called[r]), "score": score[r], "score_lead": sl[r], "quality": q[r],
                    "lead_extent": (ext[4 * r], ext[4 * r + 1]), "trail_extent": (ext[4 * r + 2], ext[4 * r + 3]),
                    "clip": None if over[r] else (clip[2 * r], clip[2 * r + 1]), "overlap": bool(over[r]),
                    "best": ((b[1], b[0]), (b[4], b[3])),
                    "second": (None if b[2] == INT_MIN else b[2], None if b[5] == INT_MIN else b[5])})
    return res


_SIZES = {"lead": 1, "trail": 1, "called": 1, "score": 1, "score_lead": 1, "quality": 1, "extents": 4, "clip": 2,
          "overlap": 1, "best": 6}


def _outputs(n, n_scores=0):
    import numpy as np
    arrs = {k: np.zeros(max(1, n * m), dtype=np.int32) for k, m in _SIZES.items()}
    if n_scores:
        arrs["scores"] = np.zeros(n_scores, dtype=np.int32)
    c = _L.CDemuxOutput()
    for k, a in arrs.items():
        setattr(c, k, ctypes.cast(a.ctypes.data, ctypes.POINTER(ctypes.c_int)))
    return c, arrs


def demux_batch(reads, barcodes, params=None, design="asymmetric", window=None, window_mult=3, min_quality=None,
                min_score_lead=0, return_scores=False, engine=None):
    """Calls the barcode pair of every read (str or bytes; any length, empty included) in one native call.

    barcodes: a BarcodeSet (or a list of sequences).  params: AlignParams, default (3, -5, -4, -4); Match > 0,
    Insert <= 0, Delete <= 0.  The window is `window`, else window_mult times the longest barcode, 1..1024.
    design "asymmetric": the leading and the trailing barcode are called independently; "symmetric": one barcode
    for both ends, the best of the two ends' summed scores.  min_quality None is MIN_QUALITY (measured, §3.27).

    Returns one dict per read: "lead" / "trail" (the called barcodes i and j, filled for an uncalled read too),
    "pair" ((min, max), or (-1, -1) when uncalled), "called", "score", "score_lead" (INT_MAX with one barcode),
    "quality" (0..100), "lead_extent" / "trail_extent" (where the two barcodes lie, in read coordinates), "clip"
    ((leading end, trailing begin): the insert is read[clip[0]:clip[1]]; None when they cross), "overlap", and per
    end "best" ((index, score) for the leading and the trailing end) and "second" (the best score over the other
    barcodes, None with one barcode).  With return_scores: (the list, the (n, 2, B) int32 score matrix).
    Every refusal (InvalidInputError) is raised before an engine is touched."""
    import numpy as np
    from .quiver import _struct_dtype
    barcodes, o = _options(barcodes, params, design, window, window_mult, min_quality, min_score_lead)
    enc = [r if isinstance(r, bytes) else r.encode("latin-1") for r in reads]
    n, B = len(enc), len(barcodes)
    if engine is None:
        from . import default_engine
        engine = default_engine()
    lens = np.fromiter((len(x) for x in enc), dtype=np.int64, count=n)
    blob = ctypes.create_string_buffer(b"".join(enc), max(1, int(lens.sum())))
    starts = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(lens, out=starts[1:])
    ins = np.zeros(max(1, n), dtype=_struct_dtype(_L.CDemuxRead))
    if n:
        ins["seq"][:n] = (ctypes.addressof(blob) + starts[:-1]).astype(np.uint64)
        ins["len"][:n] = lens
    c, arrs = _outputs(n, max(1, n * 2 * B) if return_scores else 0)
    bc, keep = barcodes._c()
    _L.check(load().pbccs_demux_batch(engine._h, ctypes.byref(bc), ctypes.byref(o),
                                      ctypes.cast(ins.ctypes.data, ctypes.POINTER(_L.CDemuxRead)), n, ctypes.byref(c)))
    del keep, blob
    res = _entries(n, arrs)
    if return_scores:
        return res, arrs["scores"][:n * 2 * B].reshape(n, 2, B)
    return res


def demux_options(spec):
    """ccs_batch(barcodes=...): a BarcodeSet, or a dict with "barcodes" and any of demux_batch's keywords ->
    (BarcodeSet, keywords, the checked pbccs_demux_options)."""
    kw = {}
    if isinstance(spec, dict):
        kw = {k: v for k, v in spec.items() if k != "barcodes"}
        bad = set(kw) - {"params", "design", "window", "window_mult", "min_quality", "min_score_lead"}
        if bad or "barcodes" not in spec:
            raise InvalidInputError('barcodes=: a BarcodeSet, or a dict with "barcodes" and any of params, design, '
                                    "window, window_mult, min_quality, min_score_lead")
        spec = spec["barcodes"]
    barcodes, o = _options(spec, kw.get("params"), kw.get("design", "asymmetric"), kw.get("window"),
                           kw.get("window_mult", 3), kw.get("min_quality"), kw.get("min_score_lead", 0))
    return barcodes, kw, o


def demux_stats(engine=None, reset=False):
    """Demultiplexing work since the last reset: reads, cells (2 * min(W, n) * the sum of the barcode lengths per
    read that reached the device), launches, device_ms (profiling on)."""
    if engine is None:
        from . import default_engine
        engine = default_engine()
    s = _L.CDemuxStats()
    _L.check(load().pbccs_demux_stats_get(engine._h, ctypes.byref(s), 1 if reset else 0))
    return {k: getattr(s, k) for k, _ in _L.CDemuxStats._fields_}


def clip_read(seq, entry):
    """The insert of a read: seq without its two barcodes, seq[clip[0]:clip[1]].  An uncalled read and one whose
    barcodes overlap come back whole."""
    if not entry["called"] or entry["clip"] is None:
        return seq
    return seq[entry["clip"][0]:entry["clip"][1]]

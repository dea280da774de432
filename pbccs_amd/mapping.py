"""MapToDraft on the GPU: placing reads on a finished draft (pbccs_map_batch).

What SparsePoa::OrientAndAddRead followed by FindConsensus reports for a read on a graph that holds only the draft
as one unbranched path -- orientation, extent on the read, extent on the draft -- from a LOCAL alignment of the
read against the linear draft (k_map_fill: no graph, no stored matrix, no traceback).  It is what lets a POA
capped by max_poa_coverage keep the reads past the cap (driver.ccs_batch(..., map_past_cap=True)).
There is no CPU fallback: without the library or a GPU these raise."""
import ctypes

from . import lib as _L
from .lib import load


def _engine(engine):
    if engine is None:
        from . import default_engine
        engine = default_engine()
    return engine


MAP_PARAMS = (3, -5, -4, -4)   # DefaultPoaConfig's Match, Mismatch, Insert, Delete: k_map_fill's scores


def _add_transcripts(zmws, res, eng):
    """map_batch(transcripts=True): the path of every mapped read, from one LOCAL call of the ends-free aligner
    (align.align_ends_batch) with the mapper's scores on the read in the orientation the mapper
    chose.  Same rules, same ties, so the path covers the summary's own extents."""
    from . import align as A
    pairs, where = [], []
    for z, (draft, reads) in enumerate(zmws):
        for k, r in enumerate(reads):
            m = res[z][k]
            if m is not None:
                pairs.append((draft, A.reverse_complement(r) if m["rc"] else r))
                where.append(m)
    if not pairs:
        return
    alns, _, _ = A.align_ends_batch(pairs, A.LOCAL, A.AlignParams(*MAP_PARAMS), engine=eng)
    for m, a in zip(where, alns):
        m["transcript"] = a.Transcript()


def map_batch(zmws, min_score_to_add=0.0, engine=None, transcripts=False):
    """zmws: [(draft, [read or None, ...])].  Returns per ZMW a list with one entry per read: None for a read that
    was not mapped (no read, or both orientations below min_score_to_add), else {"rc", "read": (b, e), "tpl":
    (b, e), "score"} -- the PoaAlignmentSummary driver.extract_mapped_read takes, plus the alignment score.
    transcripts=True adds "transcript" to each summary: the LOCAL path (M R I D, draft as target) over
    draft[tpl] and the oriented read[read], from a second device call (_add_transcripts).

    Marshalling is flat, as poa.poa_batch's: all sequences in one buffer with a pointer table, all outputs in
    shared arrays, the per-ZMW structs written column-wise."""
    import numpy as np
    from .quiver import _struct_dtype
    eng = _engine(engine)
    n = len(zmws)
    counts = np.fromiter((len(reads) for _, reads in zmws), dtype=np.int64, count=n)
    drafts = [d.encode() for d, _ in zmws]
    enc = [b"" if r is None else r.encode() for _, reads in zmws for r in reads]
    nr = len(enc)
    lens = np.fromiter((len(e) for e in enc), dtype=np.int32, count=nr)
    dlens = np.fromiter((len(d) for d in drafts), dtype=np.int64, count=n)
    blob = ctypes.create_string_buffer(b"".join(enc) + b"".join(drafts), max(1, int(lens.sum()) + int(dlens.sum())))
    starts = np.zeros(nr + 1, dtype=np.int64)
    np.cumsum(lens, out=starts[1:])
    ptrs = (ctypes.addressof(blob) + starts[:-1]).astype(np.uint64)
    ptrs[lens == 0] = 0                                   # NULL: no read
    dstarts = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(dlens, out=dstarts[1:])
    first = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(counts, out=first[1:])
    mapped = np.zeros(max(1, nr), dtype=np.int32)
    rc = np.zeros(max(1, nr), dtype=np.int32)
    score = np.zeros(max(1, nr), dtype=np.int32)
    ext = np.zeros(max(4, 4 * nr), dtype=np.int32)
    ins = np.zeros(max(1, n), dtype=_struct_dtype(_L.CMapInput))
    outs = np.zeros(max(1, n), dtype=_struct_dtype(_L.CMapOutput))
    if n:
        f0 = first[:-1]
        ins["draft"][:n] = ctypes.addressof(blob) + int(starts[-1]) + dstarts[:-1]
        ins["draft_len"][:n] = dlens
        ins["seqs"][:n] = ptrs.ctypes.data + 8 * f0
        ins["lens"][:n] = lens.ctypes.data + 4 * f0
        ins["n_reads"][:n] = counts
        outs["mapped"][:n] = mapped.ctypes.data + 4 * f0
        outs["rc"][:n] = rc.ctypes.data + 4 * f0
        outs["extents"][:n] = ext.ctypes.data + 16 * f0
        outs["score"][:n] = score.ctypes.data + 4 * f0
    _L.check(load().pbccs_map_batch(eng._h, ctypes.cast(ins.ctypes.data, ctypes.POINTER(_L.CMapInput)), n,
                                    float(min_score_to_add), ctypes.cast(outs.ctypes.data, ctypes.POINTER(_L.CMapOutput))))
    m_l, rc_l, sc_l, ext_l = mapped.tolist(), rc.tolist(), score.tolist(), ext.tolist()
    firsts, cnts = first.tolist(), counts.tolist()
    res = []
    for z in range(n):
        f = firsts[z]
        res.append([{"rc": bool(rc_l[k]), "read": (ext_l[4 * k], ext_l[4 * k + 1]),
                     "tpl": (ext_l[4 * k + 2], ext_l[4 * k + 3]), "score": sc_l[k]} if m_l[k] else None
                    for k in range(f, f + cnts[z])])
    if transcripts:
        _add_transcripts(zmws, res, eng)
    return res


def map_to_draft(draft, reads, min_score_to_add=0.0, engine=None, transcripts=False):
    """MapToDraft(draft, reads, minScoreToAdd): one entry per read, None when it was not mapped, else the summary
    {"rc", "read", "tpl", "score"} (and "transcript" with transcripts=True, see map_batch)."""
    return map_batch([(draft, list(reads))], min_score_to_add, engine, transcripts)[0]


def map_stats(engine=None, reset=False):
    eng = _engine(engine)
    s = _L.CMapStats()
    _L.check(load().pbccs_map_stats_get(eng._h, ctypes.byref(s), 1 if reset else 0))
    return {k: getattr(s, k) for k, _ in _L.CMapStats._fields_}


SPLIT_JUMP_PENALTY = 150   # PBCCS_SPLIT_JUMP_PENALTY: twice the measured null of unrelated sequence


def split_map_batch(zmws, jump_penalty=None, max_segments=8, engine=None):
    """Split mapping (pbccs_split_map_batch): every read is placed on its draft as a chain of LOCAL
    segments, on either strand, at jump_penalty per extra segment -- what a read that holds several passes fused
    across a missed adapter needs.  zmws: [(draft, [read or None, ...])].  Returns per ZMW a list with one entry per
    read: None for a read that was not mapped (no read, or a chain score of 0), else {"score", "n_segments",
    "truncated", "segments": [{"rc", "read": (b, e), "tpl": (b, e), "score"}]} -- the chain's last max_segments
    segments in read order, extents on the read as given and on the draft, each with its own score; "score" is
    their sum less jump_penalty per jump.  jump_penalty None is SPLIT_JUMP_PENALTY.

    Marshalling is flat, as map_batch's."""
    import numpy as np
    from .quiver import _struct_dtype
    eng = _engine(engine)
    P = SPLIT_JUMP_PENALTY if jump_penalty is None else int(jump_penalty)
    ms = int(max_segments)
    if P < 0 or not 1 <= ms <= 64:
        raise ValueError("split_map_batch: jump_penalty >= 0 and 1 <= max_segments <= 64")
    n = len(zmws)
    counts = np.fromiter((len(reads) for _, reads in zmws), dtype=np.int64, count=n)
    drafts = [d.encode() for d, _ in zmws]
    enc = [b"" if r is None else r.encode() for _, reads in zmws for r in reads]
    nr = len(enc)
    lens = np.fromiter((len(e) for e in enc), dtype=np.int32, count=nr)
    dlens = np.fromiter((len(d) for d in drafts), dtype=np.int64, count=n)
    blob = ctypes.create_string_buffer(b"".join(enc) + b"".join(drafts), max(1, int(lens.sum()) + int(dlens.sum())))
    starts = np.zeros(nr + 1, dtype=np.int64)
    np.cumsum(lens, out=starts[1:])
    ptrs = (ctypes.addressof(blob) + starts[:-1]).astype(np.uint64)
    ptrs[lens == 0] = 0                                   # NULL: no read
    dstarts = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(dlens, out=dstarts[1:])
    first = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(counts, out=first[1:])
    nseg = np.zeros(max(1, nr), dtype=np.int32)
    trunc = np.zeros(max(1, nr), dtype=np.int32)
    score = np.zeros(max(1, nr), dtype=np.int32)
    segs = np.zeros(max(1, nr) * ms * 6, dtype=np.int32)
    ins = np.zeros(max(1, n), dtype=_struct_dtype(_L.CMapInput))
    outs = np.zeros(max(1, n), dtype=_struct_dtype(_L.CSplitMapOutput))
    if n:
        f0 = first[:-1]
        ins["draft"][:n] = ctypes.addressof(blob) + int(starts[-1]) + dstarts[:-1]
        ins["draft_len"][:n] = dlens
        ins["seqs"][:n] = ptrs.ctypes.data + 8 * f0
        ins["lens"][:n] = lens.ctypes.data + 4 * f0
        ins["n_reads"][:n] = counts
        outs["n_segments"][:n] = nseg.ctypes.data + 4 * f0
        outs["truncated"][:n] = trunc.ctypes.data + 4 * f0
        outs["score"][:n] = score.ctypes.data + 4 * f0
        outs["segments"][:n] = segs.ctypes.data + 24 * ms * f0
    _L.check(load().pbccs_split_map_batch(eng._h, ctypes.cast(ins.ctypes.data, ctypes.POINTER(_L.CMapInput)), n, P, ms,
                                          ctypes.cast(outs.ctypes.data, ctypes.POINTER(_L.CSplitMapOutput))))
    n_l, t_l, sc_l, sg_l = nseg.tolist(), trunc.tolist(), score.tolist(), segs.tolist()
    firsts, cnts = first.tolist(), counts.tolist()
    res = []
    for z in range(n):
        row = []
        for k in range(firsts[z], firsts[z] + cnts[z]):
            if n_l[k] == 0:
                row.append(None)
                continue
            at = 6 * ms * k
            row.append({"score": sc_l[k], "n_segments": n_l[k], "truncated": bool(t_l[k]),
                        "segments": [{"rc": bool(sg_l[a]), "read": (sg_l[a + 1], sg_l[a + 2]),
                                      "tpl": (sg_l[a + 3], sg_l[a + 4]), "score": sg_l[a + 5]}
                                     for a in range(at, at + 6 * min(n_l[k], ms), 6)]})
        res.append(row)
    return res


def split_map_to_draft(draft, reads, jump_penalty=None, max_segments=8, engine=None):
    """One entry per read, None when it was not mapped, else split_map_batch's chain."""
    return split_map_batch([(draft, list(reads))], jump_penalty, max_segments, engine)[0]


def split_map_stats(engine=None, reset=False):
    eng = _engine(engine)
    s = _L.CSplitMapStats()
    _L.check(load().pbccs_split_map_stats_get(eng._h, ctypes.byref(s), 1 if reset else 0))
    return {k: getattr(s, k) for k, _ in _L.CSplitMapStats._fields_}

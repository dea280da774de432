"""SparseAlign on the GPU: K-mer seeds, their SDP chain and alignable ranges (pbccs_sparse_align_batch, DESIGN.md
§3.16).

PacBio::CCS::SparseAlign<K>(seq1, seq2) -- what SdpRangeFinder::FindAnchors calls with K = 6 -- for many pairs per
call, anchor for anchor as the reference: seeds from every non-homopolymer K-mer of the query, chained by the
reference's sparse dynamic programme.  Optionally the rows of the query that SdpRangeFinder::InitRangeFinder would
allow each position of the target, taken as a linear draft.  There is no CPU fallback: without the library or a GPU
these raise."""
import ctypes

from . import lib as _L
from .lib import load


def _engine(engine):
    if engine is None:
        from . import default_engine
        engine = default_engine()
    return engine


def sparse_align_batch_raw(pairs, k=6, reverse_complement=None, ranges=False, engine=None, anchor_caps=None):
    """pbccs_sparse_align_batch as it stands: (return code, [result per pair]).  pairs: [(target, query)];
    reverse_complement: None or one flag per pair; anchor_caps (tests): anchor buffer sizes other than the bound
    min(len1, len2) - k + 1.  A result is {"status", "n_seeds", "score", "anchors": [(h, v), ...]} plus, with
    ranges, "ranges": [(begin, end) per target position]; anchors and ranges are None unless status is PBCCS_OK.

    Marshalling is flat, as mapping.map_batch's: all sequences in one buffer, all anchors and ranges in shared
    arrays, the per-pair structs written column-wise."""
    import numpy as np
    from .quiver import _struct_dtype
    eng = _engine(engine)
    n = len(pairs)
    enc = [s.encode() for p in pairs for s in p]
    lens = np.fromiter((len(e) for e in enc), dtype=np.int64, count=2 * n)
    blob = ctypes.create_string_buffer(b"".join(enc), max(1, int(lens.sum())))
    starts = np.zeros(2 * n + 1, dtype=np.int64)
    np.cumsum(lens, out=starts[1:])
    l1, l2 = lens[0::2], lens[1::2]
    if anchor_caps is None:
        caps = np.maximum(np.minimum(l1, l2) - int(k) + 1, 0)
    else:
        caps = np.asarray(anchor_caps, dtype=np.int64)
    astart = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(caps, out=astart[1:])
    rstart = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(l1, out=rstart[1:])
    anchors = np.zeros(max(2, 2 * int(astart[-1])), dtype=np.int32)
    rng = np.zeros(max(2, 2 * int(rstart[-1])) if ranges else 2, dtype=np.int32)
    ins = np.zeros(max(1, n), dtype=_struct_dtype(_L.CSparseAlignInput))
    outs = np.zeros(max(1, n), dtype=_struct_dtype(_L.CSparseAlignOutput))
    if n:
        base = ctypes.addressof(blob)
        ins["target"][:n] = base + starts[0:-1:2]
        ins["target_len"][:n] = l1
        ins["query"][:n] = base + starts[1::2]
        ins["query_len"][:n] = l2
        if reverse_complement is not None:
            ins["reverse_complement"][:n] = np.asarray([1 if f else 0 for f in reverse_complement], dtype=np.int32)
        ins["anchors"][:n] = anchors.ctypes.data + 8 * astart[:-1]
        ins["anchor_cap"][:n] = caps
        if ranges:
            ins["ranges"][:n] = rng.ctypes.data + 8 * rstart[:-1]
    rc = load().pbccs_sparse_align_batch(eng._h, int(k), ctypes.cast(ins.ctypes.data, ctypes.POINTER(_L.CSparseAlignInput)),
                                         n, ctypes.cast(outs.ctypes.data, ctypes.POINTER(_L.CSparseAlignOutput)))
    st, na = outs["status"][:n].tolist(), outs["n_anchors"][:n].tolist()
    ns, sc = outs["n_seeds"][:n].tolist(), outs["score"][:n].tolist()
    a_l, r_l = astart.tolist(), rstart.tolist()
    res = []
    for g in range(n):
        r = {"status": st[g], "n_seeds": ns[g], "n_anchors": na[g], "score": sc[g], "anchors": None}
        if ranges:
            r["ranges"] = None
        if st[g] == _L.PBCCS_OK:
            flat = anchors[2 * a_l[g]:2 * (a_l[g] + na[g])].tolist()
            r["anchors"] = list(zip(flat[0::2], flat[1::2]))
            if ranges:
                flat = rng[2 * r_l[g]:2 * r_l[g + 1]].tolist()
                r["ranges"] = list(zip(flat[0::2], flat[1::2]))
        res.append(r)
    return rc, res


def sparse_align_batch(pairs, k=6, reverse_complement=None, ranges=False, engine=None):
    """One result per (target, query) pair, see sparse_align_batch_raw; raises PbccsError when any pair failed."""
    rc, res = sparse_align_batch_raw(pairs, k, reverse_complement, ranges, engine)
    _L.check(rc)
    return res


def SparseAlign(target, query, k=6, engine=None):
    """SparseAlign<K>(seq1, seq2): the chain as a list of (h, v)."""
    return sparse_align_batch([(target, query)], k, engine=engine)[0]["anchors"]


def sparse_align_stats(engine=None, reset=False):
    eng = _engine(engine)
    s = _L.CSparseAlignStats()
    _L.check(load().pbccs_sparse_align_stats_get(eng._h, ctypes.byref(s), 1 if reset else 0))
    return {k: getattr(s, k) for k, _ in _L.CSparseAlignStats._fields_}

"""Consensus kinetics on the GPU: per-strand mean inter-pulse duration (IPD) and pulse width (PW) of a consensus,
from the subreads' `ip` / `pw` tracks (pbccs_kinetics_pileup / pbccs_kinetics_batch).

Each read is placed on the consensus as mapping.map_batch places it, aligned to its extent as align.Align does, and
every M / R column of the transcript carries the read's frames at that base onto the consensus position; the
passes of a strand are folded into a rounded integer mean and its CodecV1 code (k_kin_columns, k_kin_reduce).
The reference (2015 pbccs) has no kinetics: the rules are this project's own, and the codec is pbbam's published
CodecV1 restated without pbbam at hand (unpinned).  There is no CPU fallback: without the library or a GPU the
device calls raise; the codec functions are host code."""
import ctypes

from . import lib as _L
from .lib import load

READ_STATUS = ("used", "unmapped", "empty_extent", "align_failed")
_BASE = (0, 64, 192, 448)
_NAMES = ("fwd_ipd", "fwd_pw", "rev_ipd", "rev_pw")   # index 2 * strand + track


def codec_v1_decode(codes):
    """CodecV1 codes (0..255) -> frames: base[g] + ((c & 63) << g), g = c >> 6, base = 0, 64, 192, 448."""
    out = []
    for c in codes:
        c = int(c)
        if not 0 <= c <= 255:
            raise ValueError(f"not a CodecV1 code: {c}")
        g = c >> 6
        out.append(_BASE[g] + ((c & 63) << g))
    return out


def codec_v1_encode(frames):
    """Frames -> CodecV1 codes: 255 above 952, else the nearest representable value, a tie to the larger one."""
    out = []
    for f in frames:
        f = int(f)
        if f < 0:
            raise ValueError(f"negative frame count: {f}")
        if f > 952:
            out.append(255)
            continue
        g = (f >= 64) + (f >= 192) + (f >= 448)
        out.append(min(255, (g << 6) + ((f - _BASE[g] + ((1 << g) >> 1)) >> g)))
    return out


def _engine(engine):
    if engine is None:
        from . import default_engine
        engine = default_engine()
    return engine


def _tracks(reads_tracks, lens, what):
    """Host validation, before any engine is touched: one uint16 array per read and track (None: absent), each as
    long as its read.  Returns (pool, offsets in frames or -1)."""
    import numpy as np
    parts, offs, at = [], [], 0
    for k, t in enumerate(reads_tracks):
        if t is None:
            offs.append(-1)
            continue
        a = np.asarray(t)
        if a.ndim != 1 or len(a) != lens[k]:
            raise _L.PbccsError(-1, f"kinetics: read {k}: the {what} track has {a.size} frames, the read {lens[k]} bases")
        if len(a) and (a.min() < 0 or a.max() > 65535):
            raise _L.PbccsError(-1, f"kinetics: read {k}: {what} frames outside 0..65535")
        parts.append(a.astype(np.uint16))
        offs.append(at)
        at += len(a)
    pool = np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint16)
    if len(pool) == 0:
        pool = np.zeros(1, dtype=np.uint16)
    return pool, np.asarray(offs, dtype=np.int64)


def _track_ptrs(pool, offs):
    import numpy as np
    p = (pool.ctypes.data + 2 * offs).astype(np.uint64)
    p[offs < 0] = 0
    return p


class _Outputs:
    """Shared output arrays for n ZMWs of lengths Ls and the pbccs_kinetics_output structs over them."""

    def __init__(self, Ls, counts):
        import numpy as np
        from .quiver import _struct_dtype
        n = len(Ls)
        self.n = n
        self.Ls = [int(x) for x in Ls]
        self.off = np.zeros(n + 1, dtype=np.int64)
        np.cumsum(np.asarray(Ls, dtype=np.int64), out=self.off[1:])
        self.first = np.zeros(n + 1, dtype=np.int64)
        np.cumsum(np.asarray(counts, dtype=np.int64), out=self.first[1:])
        tot = max(1, int(self.off[-1]))
        self.mean = np.zeros((4, tot), dtype=np.uint16)
        self.code = np.zeros((4, tot), dtype=np.uint8)
        self.cov = np.zeros((4, tot), dtype=np.int32)
        self.status = np.zeros(max(1, int(self.first[-1])), dtype=np.int32)
        self.outs = np.zeros(max(1, n), dtype=_struct_dtype(_L.CKineticsOutput))
        if n:
            for v in range(4):
                self.outs["mean"][:n, v] = self.mean[v].ctypes.data + 2 * self.off[:-1]
                self.outs["code"][:n, v] = self.code[v].ctypes.data + self.off[:-1]
                self.outs["coverage"][:n, v] = self.cov[v].ctypes.data + 4 * self.off[:-1]
            self.outs["read_status"][:n] = self.status.ctypes.data + 4 * self.first[:-1]

    def pointer(self):
        return ctypes.cast(self.outs.ctypes.data, ctypes.POINTER(_L.CKineticsOutput))

    def results(self):
        res = []
        nc = self.outs["n_contributed"][:self.n].tolist()
        st = self.status.tolist()
        for z in range(self.n):
            a, b = int(self.off[z]), int(self.off[z + 1])
            d = {"fn": nc[z][0], "rn": nc[z][1],
                 "read_status": [READ_STATUS[s] for s in st[int(self.first[z]):int(self.first[z + 1])]]}
            for v, name in enumerate(_NAMES):
                d[name] = self.code[v, a:b].tolist()
                d[name + "_mean"] = self.mean[v, a:b].tolist()
                d[name + "_cov"] = self.cov[v, a:b].tolist()
            res.append(d)
        return res


def kinetics_pileup(zmws, engine=None):
    """The two kernels on the caller's transcripts.  zmws: [(L, [read, ...])], read = {"transcript", "rc", "rb",
    "tb", "te", "len", "ip", "pw"} (ip / pw: `len` frames, or None / missing for an absent track).  Returns per
    ZMW {"fwd_ipd", "fwd_pw", "rev_ipd", "rev_pw" (CodecV1 codes), the same names with "_mean" (frames) and "_cov"
    (coverage), "fn", "rn", "read_status"}; reverse-strand arrays run in the reverse strand's direction (entry k is
    consensus position L - 1 - k).

    Marshalling is flat, as mapping.map_batch's: one transcript blob, one frame pool per track, shared outputs,
    the structs written column-wise."""
    import numpy as np
    from .quiver import _struct_dtype
    n = len(zmws)
    flat = [r for _, reads in zmws for r in reads]
    nr = len(flat)
    lens = [int(r["len"]) for r in flat]
    ip_pool, ip_off = _tracks([r.get("ip") for r in flat], lens, "ip")
    pw_pool, pw_off = _tracks([r.get("pw") for r in flat], lens, "pw")
    eng = _engine(engine)
    counts = [len(reads) for _, reads in zmws]
    enc = [r["transcript"].encode("latin-1") if isinstance(r["transcript"], str) else bytes(r["transcript"])
           for r in flat]
    tlens = np.fromiter((len(e) for e in enc), dtype=np.int64, count=nr)
    blob = ctypes.create_string_buffer(b"".join(enc), max(1, int(tlens.sum())))
    tstart = np.zeros(nr + 1, dtype=np.int64)
    np.cumsum(tlens, out=tstart[1:])
    rd = np.zeros(max(1, nr), dtype=_struct_dtype(_L.CKineticsRead))
    if nr:
        rd["transcript"][:nr] = ctypes.addressof(blob) + tstart[:-1]
        rd["transcript_len"][:nr] = tlens
        for key in ("rc", "rb", "tb", "te"):
            rd[key][:nr] = [int(r[key]) for r in flat]
        rd["len"][:nr] = lens
        rd["ip"][:nr] = _track_ptrs(ip_pool, ip_off)
        rd["pw"][:nr] = _track_ptrs(pw_pool, pw_off)
    out = _Outputs([L for L, _ in zmws], counts)
    ins = np.zeros(max(1, n), dtype=_struct_dtype(_L.CKineticsPileupInput))
    if n:
        ins["consensus_len"][:n] = out.Ls
        ins["n_reads"][:n] = counts
        ins["reads"][:n] = rd.ctypes.data + rd.dtype.itemsize * out.first[:-1]
    _L.check(load().pbccs_kinetics_pileup(eng._h, ctypes.cast(ins.ctypes.data, ctypes.POINTER(_L.CKineticsPileupInput)),
                                          n, out.pointer()))
    return out.results()


def kinetics_batch(zmws, band=None, engine=None):
    """zmws: [(consensus, [read, ...])], read = {"seq", "ip", "pw"} (a track None or missing: absent) or None for no
    read.  Per read: MapToDraft onto the consensus, Align of the extents (NW, default parameters), then the
    pileup, in one native call.  band: as align.align_batch's (off by default; the answers are the same).  Returns
    what kinetics_pileup returns."""
    import numpy as np
    from .align import _c_band
    from .quiver import _struct_dtype
    n = len(zmws)
    flat = [r for _, reads in zmws for r in reads]
    nr = len(flat)
    enc = [b"" if r is None else r["seq"].encode() for r in flat]
    lens = np.fromiter((len(e) for e in enc), dtype=np.int32, count=nr)
    lens_l = lens.tolist()
    ip_pool, ip_off = _tracks([None if r is None else r.get("ip") for r in flat], lens_l, "ip")
    pw_pool, pw_off = _tracks([None if r is None else r.get("pw") for r in flat], lens_l, "pw")
    cb = _c_band(band)
    eng = _engine(engine)
    counts = np.fromiter((len(reads) for _, reads in zmws), dtype=np.int64, count=n)
    cons = [c.encode() for c, _ in zmws]
    clens = np.fromiter((len(c) for c in cons), dtype=np.int64, count=n)
    blob = ctypes.create_string_buffer(b"".join(enc) + b"".join(cons), max(1, int(lens.sum()) + int(clens.sum())))
    starts = np.zeros(nr + 1, dtype=np.int64)
    np.cumsum(lens, out=starts[1:])
    ptrs = (ctypes.addressof(blob) + starts[:-1]).astype(np.uint64)
    ptrs[lens == 0] = 0                                   # NULL: no read
    cstarts = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(clens, out=cstarts[1:])
    ipp, pwp = _track_ptrs(ip_pool, ip_off), _track_ptrs(pw_pool, pw_off)
    out = _Outputs(clens.tolist(), counts.tolist())
    ins = np.zeros(max(1, n), dtype=_struct_dtype(_L.CKineticsInput))
    if n:
        f0 = out.first[:-1]
        ins["consensus"][:n] = ctypes.addressof(blob) + int(starts[-1]) + cstarts[:-1]
        ins["consensus_len"][:n] = clens
        ins["n_reads"][:n] = counts
        ins["seqs"][:n] = ptrs.ctypes.data + 8 * f0
        ins["lens"][:n] = lens.ctypes.data + 4 * f0
        ins["ip"][:n] = ipp.ctypes.data + 8 * f0
        ins["pw"][:n] = pwp.ctypes.data + 8 * f0
    opts = _L.CKineticsOptions()
    load().pbccs_kinetics_options_default(ctypes.byref(opts))
    if cb is not None:
        opts.band = cb
    _L.check(load().pbccs_kinetics_batch(eng._h, ctypes.cast(ins.ctypes.data, ctypes.POINTER(_L.CKineticsInput)), n,
                                         ctypes.byref(opts), out.pointer()))
    return out.results()


def kinetics_stats(engine=None, reset=False):
    eng = _engine(engine)
    s = _L.CKineticsStats()
    _L.check(load().pbccs_kinetics_stats_get(eng._h, ctypes.byref(s), 1 if reset else 0))
    return {k: getattr(s, k) for k, _ in _L.CKineticsStats._fields_}

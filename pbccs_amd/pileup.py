"""The subread pileup on a consensus, on the GPU: which subread bases stand over each consensus position
(pbccs_pileup_columns / pbccs_pileup_batch / pbccs_pileup_msa).

Each read is placed on the consensus as mapping.map_batch places it and aligned to its extent as align.Align does
(the stage kinetics.kinetics_batch runs); the transcript then gives, per strand, the count of A C G T gap other at
every consensus position, the insertions at every slot between positions, the plurality call, the effective coverage
`ec`, each read's concordance with the consensus and, on request, the gapped row-per-read view of the ZMW
(k_pile_columns, k_pile_reduce, k_pile_scan, k_pile_rows).  The reference (2015 pbccs) has no pileup: the rules are
this project's own, all integer arithmetic.

Orientation: every array is indexed by consensus position, or by slot (slot s lies before position s, slot L after
the last one), in the consensus's own direction for both strands.  This differs from the kinetics arrays, whose
reverse-strand entries run in the reverse strand's direction.

There is no CPU fallback: without the library or a GPU the device calls raise; cigar() is host code."""
import ctypes

from . import lib as _L
from .kinetics import READ_STATUS
from .lib import load

CODES = "ACGT-"          # the characters of codes 0..4; code 5 is "other", 255 "no coverage"
GAP, OTHER, NONE = 4, 5, 255
REDUCE_THREADS = 256     # k_pile_reduce's and k_pile_scan's block sizes (slots per block / per tile)
SCAN_THREADS = 256
_CIGAR_OP = {"M": "=", "R": "X", "I": "I", "D": "D"}


def cigar(transcript, rb, read_len):
    """The extended CIGAR of a read of read_len bases whose transcript starts at oriented position rb: rb S, the
    transcript's runs with M -> =, R -> X, I, D, then read_len - re S; zero-length clips are omitted."""
    rb, read_len = int(rb), int(read_len)
    out, run, n, nq = [], None, 0, 0
    for ch in transcript:
        op = _CIGAR_OP.get(ch)
        if op is None:
            raise ValueError(f"not a transcript character: {ch!r}")
        nq += ch != "D"
        if op == run:
            n += 1
            continue
        if run is not None:
            out.append(f"{n}{run}")
        run, n = op, 1
    if run is not None:
        out.append(f"{n}{run}")
    tail = read_len - rb - nq
    if rb < 0 or tail < 0:
        raise ValueError("cigar: the transcript leaves the read")
    return (f"{rb}S" if rb else "") + "".join(out) + (f"{tail}S" if tail else "")


def _engine(engine):
    if engine is None:
        from . import default_engine
        engine = default_engine()
    return engine


def _text(x, what):
    if isinstance(x, str):
        try:
            return x.encode("latin-1")
        except UnicodeEncodeError:
            raise _L.PbccsError(-1, f"pileup: {what} holds a character outside latin-1") from None
    if isinstance(x, (bytes, bytearray)):
        return bytes(x)
    raise _L.PbccsError(-1, f"pileup: {what} is neither text nor bytes")


def _columns_input(zmws):
    """Host validation and flat marshalling of [(consensus, [read, ...])], read = {"transcript", "seq", "rc", "rb",
    "tb", "te"}: one blob, the structs written column-wise.  Nothing here touches an engine."""
    import numpy as np
    from .quiver import _struct_dtype
    n = len(zmws)
    cons = [_text(c, f"the consensus of ZMW {z}") for z, (c, _) in enumerate(zmws)]
    flat = []
    for z, (_, reads) in enumerate(zmws):
        for k, r in enumerate(reads):
            if not isinstance(r, dict) or any(key not in r for key in ("transcript", "seq", "rc", "rb", "tb", "te")):
                raise _L.PbccsError(-1, f"pileup: ZMW {z} read {k}: a dict with transcript, seq, rc, rb, tb, te")
            flat.append(r)
    nr = len(flat)
    trs = [_text(r["transcript"], "a transcript") for r in flat]
    seqs = [_text(r["seq"], "a read") for r in flat]
    try:
        ints = {key: np.fromiter((int(r[key]) for r in flat), dtype=np.int64, count=nr) for key in ("rb", "tb", "te")}
        rc = np.fromiter((1 if r["rc"] else 0 for r in flat), dtype=np.int32, count=nr)
    except (TypeError, ValueError):
        raise _L.PbccsError(-1, "pileup: rb, tb and te are integers") from None
    for v in ints.values():
        if nr and (v.min() < -2**31 or v.max() >= 2**31):
            raise _L.PbccsError(-1, "pileup: an extent outside the int range")
    counts = np.fromiter((len(reads) for _, reads in zmws), dtype=np.int64, count=n)
    tlens = np.fromiter(map(len, trs), dtype=np.int64, count=nr)
    slens = np.fromiter(map(len, seqs), dtype=np.int64, count=nr)
    clens = np.fromiter(map(len, cons), dtype=np.int64, count=n)
    blob = ctypes.create_string_buffer(b"".join(trs) + b"".join(seqs) + b"".join(cons),
                                       max(1, int(tlens.sum() + slens.sum() + clens.sum())))

    def starts(lens):
        s = np.zeros(len(lens) + 1, dtype=np.int64)
        np.cumsum(lens, out=s[1:])
        return s
    ts, ss, cs, first = starts(tlens), starts(slens), starts(clens), starts(counts)
    base = ctypes.addressof(blob)
    rd = np.zeros(max(1, nr), dtype=_struct_dtype(_L.CPileupRead))
    if nr:
        rd["transcript"][:nr] = base + ts[:-1]
        rd["transcript_len"][:nr] = tlens
        rd["seq"][:nr] = base + int(ts[-1]) + ss[:-1]
        rd["len"][:nr] = slens
        rd["rc"][:nr] = rc
        for key, v in ints.items():
            rd[key][:nr] = v
    ins = np.zeros(max(1, n), dtype=_struct_dtype(_L.CPileupColumnsInput))
    if n:
        ins["consensus"][:n] = base + int(ts[-1]) + int(ss[-1]) + cs[:-1]
        ins["consensus_len"][:n] = clens
        ins["n_reads"][:n] = counts
        ins["reads"][:n] = rd.ctypes.data + rd.dtype.itemsize * first[:-1]
    keep = (blob, rd)
    return ins, keep, [c.decode("latin-1") for c in cons], counts.tolist()


class _Outputs:
    """Shared output arrays for ZMWs with the given consensus texts and read counts, and the pbccs_pileup_output
    structs over them."""

    def __init__(self, cons, counts, transcript_caps=None):
        import numpy as np
        from .quiver import _struct_dtype
        n = len(cons)
        self.n, self.cons = n, cons
        Ls = np.asarray([len(c) for c in cons], dtype=np.int64)
        self.pos = np.zeros(n + 1, dtype=np.int64)
        np.cumsum(Ls, out=self.pos[1:])
        self.slot = self.pos + np.arange(n + 1, dtype=np.int64)
        self.first = np.zeros(n + 1, dtype=np.int64)
        np.cumsum(np.asarray(counts, dtype=np.int64), out=self.first[1:])
        npos, nslot, nr = max(1, int(self.pos[-1])), max(1, int(self.slot[-1])), max(1, int(self.first[-1]))
        self.counts = np.zeros(12 * npos, dtype=np.int32)
        self.slots = {k: np.zeros(2 * nslot, dtype=np.int32) for k in ("ins_reads", "ins_bases")}
        self.slot1 = {k: np.zeros(nslot, dtype=np.int32) for k in ("slot_cov", "max_ins")}
        self.cov = np.zeros(npos, dtype=np.int32)
        self.plur = np.zeros(npos, dtype=np.uint8)
        self.insplur = np.zeros(nslot, dtype=np.uint8)
        self.per_read = {k: np.zeros(nr, dtype=np.int32) for k in
                         ("read_status", "n_match", "n_mismatch", "n_ins", "n_del", "rc", "rb", "re", "tb", "te")}
        self.outs = np.zeros(max(1, n), dtype=_struct_dtype(_L.CPileupOutput))
        self.tbuf = None
        o = self.outs
        if n:
            p0, s0, f0 = self.pos[:-1], self.slot[:-1], self.first[:-1]
            o["counts"][:n] = self.counts.ctypes.data + 48 * p0
            for k, a in self.slots.items():
                o[k][:n] = a.ctypes.data + 8 * s0
            for k, a in self.slot1.items():
                o[k][:n] = a.ctypes.data + 4 * s0
            o["cov"][:n] = self.cov.ctypes.data + 4 * p0
            o["plurality"][:n] = self.plur.ctypes.data + p0
            o["ins_plurality"][:n] = self.insplur.ctypes.data + s0
            for k, a in self.per_read.items():
                o[k][:n] = a.ctypes.data + 4 * f0
            if transcript_caps is not None:   # one buffer of consensus_len + read_len bytes per read
                caps = np.asarray(transcript_caps, dtype=np.int64)
                self.tstart = np.zeros(len(caps) + 1, dtype=np.int64)
                np.cumsum(caps, out=self.tstart[1:])
                self.tbuf = np.zeros(max(1, int(self.tstart[-1])), dtype=np.uint8)
                self.tptr = (self.tbuf.ctypes.data + self.tstart[:-1]).astype(np.uint64)
                self.tlen = np.zeros(max(1, len(caps)), dtype=np.int32)
                o["transcripts"][:n] = self.tptr.ctypes.data + 8 * f0
                o["transcript_lens"][:n] = self.tlen.ctypes.data + 4 * f0

    def pointer(self):
        return ctypes.cast(self.outs.ctypes.data, ctypes.POINTER(_L.CPileupOutput))

    def results(self, arrays=False):
        import numpy as np
        lut = np.full(256, OTHER, dtype=np.uint8)
        lut[np.frombuffer(b"ACGT", dtype=np.uint8)] = np.arange(4, dtype=np.uint8)
        give = (lambda a: a.copy()) if arrays else (lambda a: a.tolist())
        res = []
        cov_sum = self.outs["cov_sum"][:self.n].tolist()
        n_used = self.outs["n_used"][:self.n].tolist()
        per = {k: a.tolist() for k, a in self.per_read.items()}
        tlen = self.tlen.tolist() if self.tbuf is not None else None
        for z in range(self.n):
            c = self.cons[z]
            L = len(c)
            p0, s0, f0, f1 = int(self.pos[z]), int(self.slot[z]), int(self.first[z]), int(self.first[z + 1])
            d = {"counts": give(self.counts[12 * p0:12 * (p0 + L)].reshape(2, L, 6))}
            for k, a in self.slots.items():
                d[k] = give(a[2 * s0:2 * (s0 + L + 1)].reshape(2, L + 1))
            for k, a in self.slot1.items():
                d[k] = give(a[s0:s0 + L + 1])
            d["cov"] = give(self.cov[p0:p0 + L])
            plur, insp = self.plur[p0:p0 + L], self.insplur[s0:s0 + L + 1]
            d["plurality"], d["ins_plurality"] = give(plur), give(insp)
            # the few positions whose call differs from the consensus, and the slots with an insertion call
            own = lut[np.frombuffer(c.encode("latin-1"), dtype=np.uint8)] if L else plur
            calls = [(int(p), 1) for p in np.flatnonzero((plur != NONE) & (plur != own))]
            calls += [(int(p), 0) for p in np.flatnonzero(insp)]
            sites = []
            for p, sub in sorted(calls):   # position order, a slot before its position
                if sub:
                    code = int(plur[p])
                    sites.append(("del" if code == GAP else "sub", p, c[p], CODES[code]))
                else:
                    sites.append(("ins", p, c[p] if p < L else "", "+"))
            d["plurality_sites"] = sites
            d["cov_sum"] = int(cov_sum[z])
            d["ec"] = d["cov_sum"] / L if L else 0.0
            d["n_used"] = list(n_used[z])
            reads = []
            for k in range(f0, f1):
                st = per["read_status"][k]
                r = {"status": READ_STATUS[st]}
                r.update({key: per[key][k] for key in ("n_match", "n_mismatch", "n_ins", "n_del", "rc", "rb", "re", "tb",
                                                       "te")})
                cols = r["n_match"] + r["n_mismatch"] + r["n_ins"] + r["n_del"]
                r["concordance"] = r["n_match"] / cols if st == 0 and cols else float("nan")
                if tlen is not None:
                    a = int(self.tstart[k])
                    r["transcript"] = self.tbuf[a:a + tlen[k]].tobytes().decode() if st == 0 else None
                reads.append(r)
            d["reads"] = reads
            res.append(d)
        return res


def pileup_columns(zmws, engine=None, arrays=False):
    """The pileup kernels on the caller's transcripts.  zmws: [(consensus, [read, ...])], read = {"transcript",
    "seq", "rc", "rb", "tb", "te"} (seq: the read as sequenced; the transcript aligns consensus[tb:te] to the
    oriented read from rb on).  Returns per ZMW, with L = len(consensus):
      counts [2][L][6] (strand, position, A C G T gap other), ins_reads / ins_bases [2][L + 1], slot_cov, max_ins,
      ins_plurality [L + 1], cov, plurality [L] (a code 0..4, or 255 without coverage), plurality_sites
      [("sub" | "del" | "ins", pos, consensus_char, call_char)] in position order, cov_sum, ec, n_used [fwd, rev] and
      reads: per read {"status", "n_match", "n_mismatch", "n_ins", "n_del", "rc", "rb", "re", "tb", "te",
      "concordance"} (concordance NaN for a read that is not used).
    Every array runs in the consensus's own direction for both strands (the kinetics arrays do not).
    arrays=True: the per-position and per-slot arrays come as numpy arrays of those shapes instead of nested lists
    (building 21 L list entries per ZMW is most of what a large call costs on the host)."""
    ins, keep, cons, counts = _columns_input(zmws)
    out = _Outputs(cons, counts)
    eng = _engine(engine)
    _L.check(load().pbccs_pileup_columns(eng._h, ctypes.cast(ins.ctypes.data, ctypes.POINTER(_L.CPileupColumnsInput)),
                                         len(zmws), out.pointer()))
    del keep
    return out.results(arrays)


def pileup_msa(zmws, engine=None):
    """The gapped row-per-read view on the caller's transcripts (input as pileup_columns').  Returns per ZMW
    {"width", "col": the cell of every consensus position, "rows": one string of `width` characters per read, in
    the consensus's direction}: bases, '-' for a gap, ' ' outside the read's extent; a read that is not used keeps
    a blank row.  Two native calls: the widths, then the rows."""
    import numpy as np
    ins, keep, cons, counts = _columns_input(zmws)
    n = len(zmws)
    eng = _engine(engine)
    pin = ctypes.cast(ins.ctypes.data, ctypes.POINTER(_L.CPileupColumnsInput))
    widths = np.zeros(max(1, n), dtype=np.int32)
    pw = widths.ctypes.data_as(_L.PI)
    _L.check(load().pbccs_pileup_msa(eng._h, pin, n, pw, None, None))
    Ls = np.asarray([len(c) for c in cons], dtype=np.int64)
    pos = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(Ls, out=pos[1:])
    rstart = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.asarray(counts, dtype=np.int64) * widths[:n], out=rstart[1:])
    col = np.zeros(max(1, int(pos[-1])), dtype=np.int32)
    rows = np.zeros(max(1, int(rstart[-1])), dtype=np.uint8)
    colp = (col.ctypes.data + 4 * pos[:-1]).astype(np.uint64) if n else np.zeros(1, dtype=np.uint64)
    rowp = (rows.ctypes.data + rstart[:-1]).astype(np.uint64) if n else np.zeros(1, dtype=np.uint64)
    _L.check(load().pbccs_pileup_msa(eng._h, pin, n, pw, ctypes.cast(colp.ctypes.data, ctypes.POINTER(_L.PI)),
                                     ctypes.cast(rowp.ctypes.data, ctypes.POINTER(ctypes.c_char_p))))
    del keep
    res = []
    for z in range(n):
        w, a = int(widths[z]), int(rstart[z])
        res.append({"width": w, "col": col[int(pos[z]):int(pos[z + 1])].tolist(),
                    "rows": [rows[a + k * w:a + (k + 1) * w].tobytes().decode("latin-1") for k in range(counts[z])]})
    return res


def _batch(zmws, band, transcripts, msa, engine, kinetics, arrays=False):
    """pileup_batch, and with kinetics=True also kinetics_batch's results from the same placement and alignment."""
    import numpy as np
    from . import kinetics as _K
    from .align import _c_band
    from .quiver import _struct_dtype
    n = len(zmws)
    flat = [({"seq": r} if isinstance(r, str) else r) for _, reads in zmws for r in reads]
    for r in flat:
        if r is not None and not (isinstance(r, dict) and isinstance(r.get("seq"), str)):
            raise _L.PbccsError(-1, "pileup: a read is None, its text, or a dict with its text as \"seq\"")
    nr = len(flat)
    enc = [b"" if r is None else _text(r["seq"], "a read") for r in flat]
    lens = np.fromiter(map(len, enc), dtype=np.int32, count=nr)
    cons = [_text(c, f"the consensus of ZMW {z}") for z, (c, _) in enumerate(zmws)]
    counts = np.fromiter((len(reads) for _, reads in zmws), dtype=np.int64, count=n)
    kout = None
    if kinetics:
        lens_l = lens.tolist()
        ip_pool, ip_off = _K._tracks([None if r is None else r.get("ip") for r in flat], lens_l, "ip")
        pw_pool, pw_off = _K._tracks([None if r is None else r.get("pw") for r in flat], lens_l, "pw")
    cb = _c_band(band)
    eng = _engine(engine)
    clens = np.fromiter(map(len, cons), dtype=np.int64, count=n)
    blob = ctypes.create_string_buffer(b"".join(enc) + b"".join(cons), max(1, int(lens.sum()) + int(clens.sum())))
    starts = np.zeros(nr + 1, dtype=np.int64)
    np.cumsum(lens, out=starts[1:])
    ptrs = (ctypes.addressof(blob) + starts[:-1]).astype(np.uint64)
    ptrs[lens == 0] = 0                                   # NULL: no read
    cstarts = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(clens, out=cstarts[1:])
    want_tr = transcripts or msa
    caps = (np.repeat(clens, counts) + lens) if want_tr else None
    out = _Outputs([c.decode("latin-1") for c in cons], counts.tolist(), caps)
    ins = np.zeros(max(1, n), dtype=_struct_dtype(_L.CPileupInput))
    if n:
        f0 = out.first[:-1]
        ins["consensus"][:n] = ctypes.addressof(blob) + int(starts[-1]) + cstarts[:-1]
        ins["consensus_len"][:n] = clens
        ins["n_reads"][:n] = counts
        ins["seqs"][:n] = ptrs.ctypes.data + 8 * f0
        ins["lens"][:n] = lens.ctypes.data + 4 * f0
        if kinetics:
            ipp, pwp = _K._track_ptrs(ip_pool, ip_off), _K._track_ptrs(pw_pool, pw_off)
            kout = _K._Outputs(clens.tolist(), counts.tolist())
            ins["ip"][:n] = ipp.ctypes.data + 8 * f0
            ins["pw"][:n] = pwp.ctypes.data + 8 * f0
            ins["kinetics"][:n] = kout.outs.ctypes.data + kout.outs.dtype.itemsize * np.arange(n, dtype=np.int64)
    elif kinetics:
        kout = _K._Outputs([], [])
    opts = _L.CPileupOptions()
    load().pbccs_pileup_options_default(ctypes.byref(opts))
    if cb is not None:
        opts.band = cb
    _L.check(load().pbccs_pileup_batch(eng._h, ctypes.cast(ins.ctypes.data, ctypes.POINTER(_L.CPileupInput)), n,
                                       ctypes.byref(opts), out.pointer()))
    res = out.results(arrays)
    if msa:
        blank = {"transcript": "", "seq": "", "rc": 0, "rb": 0, "tb": 0, "te": 0}
        rows = pileup_msa([(c, [dict(seq=r["seq"], **{k: g[k] for k in ("transcript", "rc", "rb", "tb", "te")})
                                if g["status"] == "used" else blank
                                for r, g in zip([({"seq": r} if isinstance(r, str) else r) for r in reads], d["reads"])])
                           for (c, reads), d in zip(zmws, res)], engine=eng)
        for d, m in zip(res, rows):
            d.update(width=m["width"], col=m["col"], rows=m["rows"])
    if not transcripts:
        for d in res:
            for r in d["reads"]:
                r.pop("transcript", None)
    return res, (kout.results() if kout is not None else None)


def pileup_batch(zmws, band=None, transcripts=False, msa=False, engine=None, arrays=False):
    """zmws: [(consensus, [read, ...])], read = {"seq"} (or the text itself), or None for no read.  Per read:
    MapToDraft onto the consensus and Align of the extents (the stage kinetics.kinetics_batch runs; band as
    align.align_batch's, off by default, the answers are the same), then the pileup, in one native call.  Returns
    what pileup_columns returns; the per-read dicts also carry the placement found.  transcripts=True: each used
    read's dict also carries its "transcript" (None for the others).  msa=True: each ZMW also carries "width", "col"
    and "rows" as pileup_msa gives them.  arrays: as pileup_columns'.  All arrays run in the consensus's own direction."""
    return _batch(zmws, band, transcripts, msa, engine, False, arrays)[0]


def pileup_stats(engine=None, reset=False):
    eng = _engine(engine)
    s = _L.CPileupStats()
    _L.check(load().pbccs_pileup_stats_get(eng._h, ctypes.byref(s), 1 if reset else 0))
    return {k: getattr(s, k) for k, _ in _L.CPileupStats._fields_}

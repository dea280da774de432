"""A literal Python restatement of the consensus-kinetics rules, written apart from the kernels:
the CodecV1 codec, the column walk over a transcript and the per-strand reduction.  A helper, not a test."""

CODEC_BASE = (0, 64, 192, 448)
REPRESENTABLE = [CODEC_BASE[c >> 6] + ((c & 63) << (c >> 6)) for c in range(256)]


def decode(c):
    return REPRESENTABLE[c]


def encode(frames):
    """Above 952: 255.  Otherwise the nearest representable value, a tie to the larger one -- by search over the
    table, not by arithmetic."""
    if frames > 952:
        return 255
    best = None
    for c, v in enumerate(REPRESENTABLE):
        d = abs(v - frames)
        if best is None or d < best[0] or (d == best[0] and v > REPRESENTABLE[best[1]]):
            best = (d, c)
    return best[1]


def revcomp(s):
    return s[::-1].translate(str.maketrans("ACGTacgt", "TGCAtgca"))


def columns(transcript, rc, rb, tb, length):
    """{consensus position: original read index} of the M / R columns; D columns are absent.  The bookkeeping is
    TargetToQueryPositions': one target cursor and one query cursor moved by the transcript's characters."""
    out = {}
    p, q = tb, rb
    for ch in transcript:
        if ch in "MR":
            out[p] = length - 1 - q if rc else q
            p += 1
            q += 1
        elif ch == "D":
            p += 1
        elif ch == "I":
            q += 1
        else:
            raise ValueError(ch)
    return out, p


def rounded_mean(values):
    n = len(values)
    if n == 0:
        return 0
    return min(65535, (2 * sum(values) + n) // (2 * n))


def pileup(L, reads):
    """reads: dicts with transcript, rc, rb, tb, te, len, ip, pw (a track may be None / missing).  A read with
    "skip" set, with te == tb or without a query column is skipped.  Returns the dict kinetics_pileup returns,
    without read_status."""
    vals = {(s, t): [[] for _ in range(L)] for s in (0, 1) for t in ("ip", "pw")}
    contributed = [0, 0]
    for r in reads:
        if r is None or r.get("skip"):
            continue
        tr = r["transcript"]
        if r["te"] == r["tb"] or not any(ch in "MRI" for ch in tr):
            continue
        cols, end = columns(tr, r["rc"], r["rb"], r["tb"], r["len"])
        assert end == r["te"]
        s = 1 if r["rc"] else 0
        tracks = [t for t in ("ip", "pw") if r.get(t) is not None]
        if cols and tracks:
            contributed[s] += 1
        for t in tracks:
            assert len(r[t]) == r["len"]
            for p, qi in cols.items():
                vals[(s, t)][p].append(int(r[t][qi]))
    res = {"fn": contributed[0], "rn": contributed[1]}
    for s, sname in ((0, "fwd"), (1, "rev")):
        for t, tname in (("ip", "ipd"), ("pw", "pw")):
            per = vals[(s, t)]
            if s:
                per = per[::-1]          # the reverse strand's own direction: entry k is position L - 1 - k
            mean = [rounded_mean(v) for v in per]
            res[f"{sname}_{tname}_mean"] = mean
            res[f"{sname}_{tname}_cov"] = [len(v) for v in per]
            res[f"{sname}_{tname}"] = [encode(m) for m in mean]
    return res


def batch(consensus, reads, placements, transcripts):
    """The restatement fed with the public map_batch / align_batch results.  reads: {"seq", "ip", "pw"} or None;
    placements: map_batch's entries (None: not mapped); transcripts: per read the Align transcript of
    consensus[tb:te] against oriented[rb:re], or None where the read was not aligned."""
    rs = []
    for r, pl, tr in zip(reads, placements, transcripts):
        if r is None or pl is None or tr is None:
            rs.append(None)
            continue
        (rb, re_), (tb, te) = pl["read"], pl["tpl"]
        if re_ <= rb or te <= tb:
            rs.append(None)
            continue
        rs.append({"transcript": tr, "rc": 1 if pl["rc"] else 0, "rb": rb, "tb": tb, "te": te, "len": len(r["seq"]),
                   "ip": r.get("ip"), "pw": r.get("pw")})
    return pileup(len(consensus), rs)


def pairs_for(consensus, reads, placements):
    """The (target, query) pairs align_batch takes for the mapped reads with non-empty extents, and their read
    indices."""
    pairs, idx = [], []
    for k, (r, pl) in enumerate(zip(reads, placements)):
        if r is None or pl is None:
            continue
        (rb, re_), (tb, te) = pl["read"], pl["tpl"]
        if re_ <= rb or te <= tb:
            continue
        oriented = revcomp(r["seq"]) if pl["rc"] else r["seq"]
        pairs.append((consensus[tb:te], oriented[rb:re_]))
        idx.append(k)
    return pairs, idx

"""The barcode-calling rules, in plain Python: what k_demux_score, k_demux_call and
k_demux_extent must equal.  The reference has no demultiplexing; the rules are this project's own, built from the
ends-free alignment rules of tests/align_modes_restatement.py (§3.26), to which tests/test_demux_cpu.py pins this file.

  windows    W = window, else window_mult x the longest barcode, 1 <= W <= 1024.  A read r of length n has the
             leading window r[0 : min(W, n)] and the trailing window r[off : n], off = max(0, n - W).  Bytes are raw:
             a byte that is not exactly a barcode's byte matches nothing.
  scores     lead[b]  = the SEMIGLOBAL score of barcode b (query) inside the leading window (target);
             trail[b] = the same for revcomp(b) inside the trailing window.  An empty window scores len(b) * Insert.
  SEMIGLOBAL query on rows i = 0..I, target on columns j = 0..J; S(0, j) = 0, S(i, 0) = i * Insert; a cell takes, in
             this order and a later one only when strictly greater, the diagonal, Delete S(i, j-1) + Delete, Extra
             S(i-1, j) + Insert; the end cell is row I's smallest column holding its maximum; the target extent is
             (j0, j1), j0 being the column where the walk back along the chosen candidates reaches row 0.
  per end    best = the smallest index holding the maximum; second = the maximum over every other index (equal to
             the best under a duplicate; None with one barcode, INT_MIN in C).
  call       asymmetric: i = best of lead, j = best of trail, score = lead[i] + trail[j], score_lead = the smaller
             of the two ends' best - second.  symmetric: total = lead + trail, i = j = its best, score = total[i],
             score_lead = best - second of total.  A lead with no second is INT_MAX; every lead is clamped to it.
             quality = clamp(floor(100 * score / (Match * (len_i + len_j))), 0, 100).
             called iff quality >= min_quality and score_lead >= min_score_lead; pair = (min, max), else (-1, -1).
  extents    of barcode i in the leading and revcomp(barcode j) in the trailing window, in read coordinates (the
             trailing one has off added); clip = (leading end, trailing begin); when clip[0] > clip[1] the windows
             overlapped: clip is None and overlap is set.

semiglobal / end_scores / demux_one are the plain forms.  scores_np computes the score matrix with numpy, one DP row
at a time over all barcodes and all windows of one length, for the larger shapes of the GPU tests and for the
min_quality measurement; tests/test_demux_cpu.py pins it to the plain form."""
import numpy as np

INT_MAX = 2**31 - 1
DEFAULT_PARAMS = (3, -5, -4, -4)     # DefaultPoaConfig's scores (Match, Mismatch, Insert, Delete)

_COMP = bytearray([127]) * 256
for _a, _b in zip(b"ACGTacgtNMnm-\x00\x01\x02\x03", b"TGCAtgcaMNmn-\x03\x02\x01\x00"):
    _COMP[_a] = _b
_COMP = bytes(_COMP)


def _bytes(s):
    return s if isinstance(s, bytes) else s.encode("latin-1")


def revcomp(s):
    out = _bytes(s)[::-1].translate(_COMP)
    return out if isinstance(s, bytes) else out.decode("latin-1")


def semiglobal(target, query, params=DEFAULT_PARAMS):
    """(score, (j0, j1)): the query placed inside the target, by the rules above."""
    t, q = _bytes(target), _bytes(query)
    match, mismatch, ins, dele = params
    I, J = len(q), len(t)
    S = [[0] * (J + 1) for _ in range(I + 1)]
    mv = [["S"] * (J + 1) for _ in range(I + 1)]
    for i in range(1, I + 1):
        S[i][0], mv[i][0] = i * ins, "E"
        for j in range(1, J + 1):
            best, move = S[i - 1][j - 1] + (match if q[i - 1] == t[j - 1] else mismatch), "M"
            if S[i][j - 1] + dele > best:
                best, move = S[i][j - 1] + dele, "D"
            if S[i - 1][j] + ins > best:
                best, move = S[i - 1][j] + ins, "E"
            S[i][j], mv[i][j] = best, move
    j1 = 0
    for j in range(1, J + 1):
        if S[I][j] > S[I][j1]:
            j1 = j
    i, j = I, j1
    while mv[i][j] != "S":
        if mv[i][j] == "M":
            i, j = i - 1, j - 1
        elif mv[i][j] == "D":
            j -= 1
        else:
            i -= 1
    return S[I][j1], (j, j1)


def window_of(barcodes, window=None, window_mult=3):
    W = window if window is not None else window_mult * max(len(b) for b in barcodes)
    if not 1 <= W <= 1024:
        raise ValueError("1 <= W <= 1024")
    return W


def windows(read, W):
    """(leading window, trailing window, off)."""
    n = len(read)
    off = max(0, n - W)
    return read[0:min(W, n)], read[off:n], off


def end_scores(read, barcodes, W, params=DEFAULT_PARAMS):
    """(lead, trail): one score per barcode and end."""
    lw, tw, _ = windows(read, W)
    return ([semiglobal(lw, b, params)[0] for b in barcodes],
            [semiglobal(tw, revcomp(b), params)[0] for b in barcodes])


def best_second(scores):
    """(best index, best, second): the smallest index holding the maximum; the maximum over the others, or None."""
    bi = 0
    for k in range(1, len(scores)):
        if scores[k] > scores[bi]:
            bi = k
    rest = [s for k, s in enumerate(scores) if k != bi]
    return bi, scores[bi], (max(rest) if rest else None)


def _lead(best, second):
    return INT_MAX if second is None else min(INT_MAX, best - second)


def quality(score, match, len_i, len_j):
    return max(0, min(100, (100 * score) // (match * (len_i + len_j))))


def call(lead, trail, lens, match, design="asymmetric", min_quality=0, min_score_lead=0):
    """The call of one read from its two score rows (no extents)."""
    if design not in ("asymmetric", "symmetric"):
        raise ValueError(f"unknown design {design!r}")
    li, lb, ls = best_second(lead)
    ti, tb, ts = best_second(trail)
    if design == "asymmetric":
        i, j, score, sl = li, ti, lb + tb, min(_lead(lb, ls), _lead(tb, ts))
    else:
        i, score, sec = best_second([a + b for a, b in zip(lead, trail)])
        j, sl = i, _lead(score, sec)
    q = quality(score, match, lens[i], lens[j])
    called = q >= min_quality and sl >= min_score_lead
    return {"lead": i, "trail": j, "pair": (min(i, j), max(i, j)) if called else (-1, -1), "called": called,
            "score": score, "score_lead": sl, "quality": q,
            "best": ((li, lb), (ti, tb)), "second": (ls, ts)}


def demux_one(read, barcodes, params=DEFAULT_PARAMS, design="asymmetric", window=None, window_mult=3,
              min_quality=0, min_score_lead=0, scores=None):
    """The whole entry of one read.  scores: its (lead, trail) rows when they are already known."""
    W = window_of(barcodes, window, window_mult)
    lead, trail = scores if scores is not None else end_scores(read, barcodes, W, params)
    e = call(list(lead), list(trail), [len(b) for b in barcodes], params[0], design, min_quality, min_score_lead)
    lw, tw, off = windows(read, W)
    _, (lb, le) = semiglobal(lw, barcodes[e["lead"]], params)
    _, (tb, te) = semiglobal(tw, revcomp(barcodes[e["trail"]]), params)
    e["lead_extent"], e["trail_extent"] = (lb, le), (off + tb, off + te)
    e["overlap"] = le > off + tb
    e["clip"] = None if e["overlap"] else (le, off + tb)
    return e


def demux(reads, barcodes, **kw):
    return [demux_one(r, barcodes, **kw) for r in reads]


def _rows_np(tw, Q, lens, params):
    """Scores (N, B) of B queries (Q: (B, Lmax) uint8, lens) inside N targets of one length (tw: (N, J) uint8).  A
    row's Delete chain is a running maximum, as align_modes_restatement.fill_np's."""
    match, mismatch, ins, dele = params
    N, J = tw.shape
    B, L = Q.shape
    out = np.zeros((N, B), dtype=np.int64)
    prev = np.zeros((N, B, J + 1), dtype=np.int64)
    ramp = np.arange(J + 1, dtype=np.int64) * dele
    for i in range(1, L + 1):
        x = np.empty_like(prev)
        x[:, :, 0] = i * ins
        sub = np.where(tw[:, None, :] == Q[None, :, i - 1, None], match, mismatch)
        x[:, :, 1:] = np.maximum(prev[:, :, :-1] + sub, prev[:, :, 1:] + ins)
        prev = np.maximum.accumulate(x - ramp, axis=2) + ramp
        done = lens == i
        if done.any():
            out[:, done] = prev[:, done, :].max(axis=2)
    return out


def pack(seqs):
    """(Q, lens): the sequences as rows of one uint8 array, padded with 0 (a byte no read row is compared to)."""
    enc = [_bytes(s) for s in seqs]
    lens = np.array([len(s) for s in enc], dtype=np.int64)
    Q = np.zeros((len(enc), max(1, int(lens.max()))), dtype=np.uint8)
    for k, s in enumerate(enc):
        Q[k, :len(s)] = np.frombuffer(s, dtype=np.uint8)
    return Q, lens


def scores_np(reads, barcodes, W, params=DEFAULT_PARAMS, chunk=256):
    """The score matrix (n, 2, B) of end_scores, through _rows_np: windows of one length are filled together."""
    fq, lens = pack(barcodes)
    rq, _ = pack([revcomp(b) for b in barcodes])
    out = np.zeros((len(reads), 2, len(barcodes)), dtype=np.int64)
    by_len = {}
    for k, r in enumerate(reads):
        by_len.setdefault(min(W, len(r)), []).append(k)
    for J, ks in by_len.items():
        for c in range(0, len(ks), chunk):
            sel = ks[c:c + chunk]
            for e, Q in ((0, fq), (1, rq)):
                tw = np.zeros((len(sel), J), dtype=np.uint8)
                for a, k in enumerate(sel):
                    tw[a] = np.frombuffer(_bytes(windows(reads[k], W)[e]), dtype=np.uint8)
                out[sel, e, :] = _rows_np(tw, Q, lens, params)
    return out

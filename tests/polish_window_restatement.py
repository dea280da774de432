"""A plain Python restatement of the windowed polish: the window plan, the cuts of a read at the
window boundaries, the join of two neighbouring windows and the stitched record.  The chains come from
tests/sparse_restatement.py, the draft-to-consensus transcripts from the ref_align restatement of
tests/test_align_cpu.py, and every window is polished by the oracle (oracle.polish_zmw) with the driver's gates
applied around it.  Shared by tests/test_polish_window_cpu.py and tests/test_polish_window_gpu.py; it is not a test
itself.

Nothing here is shaped like the device code: the cuts walk the chain from its start, the join spells out both
transcripts column by column and looks at slices of the resulting lists."""
import functools
import math

import sparse_restatement as SR
from test_align_cpu import ref_align, transcript_of

SUCCESS, TOO_FEW_PASSES, TOO_MANY_UNUSABLE, NON_CONVERGENT, POOR_QUALITY = 0, 4, 3, 5, 6
STATUS_NAME = {0: "Success", 3: "TooManyUnusable", 4: "TooFewPasses", 5: "NonConvergent", 6: "PoorQuality"}
FALLBACK_WINDOW, FALLBACK_NO_JOIN, FALLBACK_ACCURACY = 1, 2, 3
SETTINGS = dict(min_passes=3, min_length=10, min_zscore=-5.0, max_drop_fraction=0.34, min_predicted_accuracy=0.90)


def ceil_div(a, b):
    return -(-a // b)


def options_valid(window, overlap, guard, k):
    return window > overlap and overlap >= 2 * guard and guard >= 1 and 4 <= k <= 8


def plan(L, window, overlap):
    """Rule 1: the windows [begin, end) of a draft of length L."""
    if L <= window + overlap:
        return [(0, L)]
    n = ceil_div(L - overlap, window)
    step = ceil_div(L - overlap, n)
    return [(i * step, min(L, i * step + step + overlap)) for i in range(n)]


def forward_text(read):
    return read["seq"] if not read.get("strand", 0) else SR.revcomp(read["seq"])


def cut(chain, b, flen):
    """Rule 2: where draft position b falls in the read's forward text.  chain: (h, v) with h in draft coordinates."""
    before = [a for a in chain if a[0] <= b]
    after = [a for a in chain if a[0] > b]
    if before:
        h, v = before[-1]
        c = v + (b - h)
        if after:
            c = min(c, after[0][1])
    else:
        h, v = after[0]
        c = max(0, v - (h - b))
    return min(c, flen)


def read_chain(draft, read, k):
    f = forward_text(read)
    ts, te = read["ts"], read["te"]
    return [(h + ts, v) for h, v in SR.sparse_align(draft[ts:te], f, k)]


def slices(zmw, window, overlap, k, min_length=10):
    """Rule 2 for one ZMW: (windows, per window a list with one entry per read -- None for a placeholder, else
    (begin, end, ts', te') with [begin, end) in the forward text --, the number of reads with an empty chain)."""
    draft = zmw["draft"]
    wins = plan(len(draft), window, overlap)
    out = [[None] * len(zmw["reads"]) for _ in wins]
    if len(wins) == 1:
        for r, read in enumerate(zmw["reads"]):
            if read["seq"] is not None:
                out[0][r] = (0, len(read["seq"]), read["ts"], read["te"])
        return wins, out, 0
    unanchored = 0
    for r, read in enumerate(zmw["reads"]):
        if read["seq"] is None:
            continue
        chain = read_chain(draft, read, k)
        if not chain:
            unanchored += 1
            continue
        flen, ts, te = len(read["seq"]), read["ts"], read["te"]

        def at(b):
            return 0 if b == ts else flen if b == te else cut(chain, b, flen)
        for w, (s, e) in enumerate(wins):
            lo, hi = max(ts, s), min(te, e)
            if hi - lo < min_length:
                continue
            cb, ce = at(lo), at(hi)
            if ce - cb < min_length:
                continue
            out[w][r] = (cb, ce, lo - s, hi - s)
    return wins, out, unanchored


def slice_as_sequenced(read, cb, ce):
    """The slice as the scorer takes it: for the reverse strand seq[|f| - ce : |f| - cb)."""
    n = len(read["seq"])
    return read["seq"][cb:ce] if not read.get("strand", 0) else read["seq"][n - ce:n - cb]


def target_to_query(transcript):
    """TargetToQueryPositions: target length + 1 entries."""
    out, q = [], 0
    for c in transcript:
        if c in "MR":
            out.append(q)
            q += 1
        elif c == "D":
            out.append(q)
        else:
            q += 1
    out.append(q)
    return out


def column_ops(transcript):
    """Per target column: (index of its op in the transcript, the op)."""
    return [(x, c) for x, c in enumerate(transcript) if c != "I"]


def good_at(transcript, rel, guard):
    """Rule 4 on one transcript: the ops of columns rel - g .. rel + g - 1 are 2g neighbouring M."""
    cols = column_ops(transcript)
    if rel - guard < 0 or rel + guard > len(cols):
        return False
    x0 = cols[rel - guard][0]
    return transcript[x0:x0 + 2 * guard] == "M" * (2 * guard) and cols[rel + guard - 1][0] == x0 + 2 * guard - 1


def candidate_order(lo, hi, mid):
    out, d = [], 0
    while mid - d >= lo or mid + d <= hi:
        for p in ([mid] if d == 0 else [mid + d, mid - d]):
            if lo <= p <= hi:
                out.append(p)
        d += 1
    return out


def join(ta, wa, tb, wb, guard):
    """Rule 4: (p, cut in a's consensus, cut in b's consensus) or None.  wa, wb: the windows' draft bounds."""
    lo, hi = wb[0] + guard, wa[1] - guard
    if lo > hi:
        return None
    for p in candidate_order(lo, hi, (wb[0] + wa[1]) // 2):
        if good_at(ta, p - wa[0], guard) and good_at(tb, p - wb[0], guard):
            return p, target_to_query(ta)[p - wa[0]], target_to_query(tb)[p - wb[0]]
    return None


def transcript(target, query):
    at, aq, _ = ref_align(target, query)
    return transcript_of(at, aq)


def predicted_accuracy(qvs):
    return 1.0 - sum(10.0 ** (v / -10.0) for v in qvs) / len(qvs)


def polish_gated(draft, reads, snr, settings=SETTINGS):
    """The driver's record for one (pseudo-)ZMW from the oracle: reads with seq None are placeholders."""
    from oracle import oracle as O
    nr = len(reads)
    rec = {"status": None, "consensus": "", "qvs": [], "add_read_results": [-1] * nr, "zscores": [math.nan] * nr,
           "zg": math.nan, "za": math.nan, "predicted_accuracy": 0.0, "n_tested": 0, "n_applied": 0, "n_passes": 0,
           "status_counts": [0] * 5}
    live = [r for r in range(nr) if reads[r]["seq"] is not None]
    e = O.polish_zmw(draft, [reads[r] for r in live], snr, min_zscore=settings["min_zscore"])
    dropped = 0
    for j, r in enumerate(live):
        st = e["add_read_results"][j]
        rec["add_read_results"][r] = st
        rec["status_counts"][st] += 1
        if st == 0 and reads[r].get("full_pass", True):
            rec["n_passes"] += 1
        elif st != 0:
            dropped += 1
    if rec["n_passes"] < settings["min_passes"]:
        rec["status"] = TOO_FEW_PASSES
        return rec
    if dropped / nr > settings["max_drop_fraction"]:
        rec["status"] = TOO_MANY_UNUSABLE
        return rec
    rec["zg"], rec["za"] = e["zg"], e["za"]
    for j, r in enumerate(live):
        rec["zscores"][r] = e["zscores"][j]
    rec["n_tested"], rec["n_applied"] = e["n_tested"], e["n_applied"]
    if not e["converged"]:
        rec["status"] = NON_CONVERGENT
        return rec
    rec["consensus"], rec["qvs"] = e["template"], list(e["qvs"])
    rec["predicted_accuracy"] = predicted_accuracy(rec["qvs"])
    rec["status"] = POOR_QUALITY if rec["predicted_accuracy"] < settings["min_predicted_accuracy"] else SUCCESS
    return rec


def window_inputs(zmw, wins, sl):
    """Rule 3: the pseudo-ZMWs of one ZMW."""
    out = []
    for (s, e), row in zip(wins, sl):
        reads = []
        for read, x in zip(zmw["reads"], row):
            if x is None:
                reads.append({"seq": None, "strand": read.get("strand", 0), "ts": 0, "te": e - s,
                              "full_pass": read.get("full_pass", True)})
            else:
                reads.append({"seq": slice_as_sequenced(read, x[0], x[1]), "strand": read.get("strand", 0),
                              "ts": x[2], "te": x[3], "full_pass": read.get("full_pass", True)})
        out.append({"draft": zmw["draft"][s:e], "snr": zmw["snr"], "reads": reads})
    return out


def polish_windowed(zmw, window, overlap, guard, k, settings=SETTINGS):
    """Rules 1-6 for one ZMW.  Returns the record with `windowed`, `fallback`, `unanchored_reads` and `windows`;
    with a fallback the record fields are None (the whole-template route's record takes their place)."""
    wins, sl, unanchored = slices(zmw, window, overlap, k, settings["min_length"])
    if len(wins) == 1:
        rec = polish_gated(zmw["draft"], zmw["reads"], zmw["snr"], settings)
        rec.update(windowed=False, fallback=0, unanchored_reads=0,
                   windows=[{"begin": 0, "end": wins[0][1], "join": -1, "cut_begin": 0,
                             "cut_end": len(rec["consensus"]), "status": rec["status"], "n_tested": rec["n_tested"],
                             "n_applied": rec["n_applied"]}])
        return rec
    recs = [polish_gated(p["draft"], p["reads"], p["snr"], settings) for p in window_inputs(zmw, wins, sl)]
    info = [{"begin": s, "end": e, "join": -1, "cut_begin": 0, "cut_end": 0, "status": r["status"],
             "n_tested": r["n_tested"], "n_applied": r["n_applied"]} for (s, e), r in zip(wins, recs)]
    out = {"windowed": True, "fallback": 0, "unanchored_reads": unanchored, "windows": info}
    if any(r["status"] != SUCCESS for r in recs):
        out["fallback"] = FALLBACK_WINDOW
        return out
    trs = [transcript(zmw["draft"][s:e], r["consensus"]) for (s, e), r in zip(wins, recs)]
    begin = 0
    for i in range(len(wins) - 1):
        j = join(trs[i], wins[i], trs[i + 1], wins[i + 1], guard)
        if j is None or j[1] < begin:
            out["fallback"] = FALLBACK_NO_JOIN
            return out
        info[i]["join"], info[i]["cut_begin"], info[i]["cut_end"] = j[0], begin, j[1]
        begin = j[2]
    info[-1]["cut_begin"], info[-1]["cut_end"] = begin, len(recs[-1]["consensus"])
    cons = "".join(r["consensus"][w["cut_begin"]:w["cut_end"]] for r, w in zip(recs, info))
    qvs = [q for r, w in zip(recs, info) for q in r["qvs"][w["cut_begin"]:w["cut_end"]]]
    acc = predicted_accuracy(qvs)
    if acc < settings["min_predicted_accuracy"]:
        out["fallback"] = FALLBACK_ACCURACY
        return out
    nr = len(zmw["reads"])
    codes, zs = [], []
    for r in range(nr):
        mine = [rec["add_read_results"][r] for rec in recs if rec["add_read_results"][r] >= 0]
        bad = [c for c in mine if c != 0]
        codes.append(-1 if not mine else bad[0] if bad else 0)
        z = [rec["zscores"][r] for rec in recs if not math.isnan(rec["zscores"][r])]
        zs.append(min(z) if z else math.nan)
    counts = [0] * 5
    for c in codes:
        if c >= 0:
            counts[c] += 1
    good = [zs[r] for r in range(nr) if codes[r] == 0 and not math.isnan(zs[r])]
    out.update(status=SUCCESS, consensus=cons, qvs=qvs, predicted_accuracy=acc,
               n_tested=sum(r["n_tested"] for r in recs), n_applied=sum(r["n_applied"] for r in recs),
               add_read_results=codes, zscores=zs, za=sum(good) / len(good) if good else math.nan,
               zg=min(r["zg"] for r in recs), status_counts=counts,
               n_passes=sum(1 for r in range(nr) if codes[r] == 0 and zmw["reads"][r].get("full_pass", True)))
    return out


@functools.lru_cache(maxsize=None)
def synthetic_case(n, length, passes, seed, window, overlap, guard, k):
    """(zmws, restated records) of synth.make_zmws(n, length, passes, seed): computed once per process."""
    from pbccs_amd import synth
    zmws = synth.make_zmws(n, length, passes, seed=seed)
    return zmws, [polish_windowed(z, window, overlap, guard, k) for z in zmws]


@functools.lru_cache(maxsize=None)
def whole_template(n, length, passes, seed):
    from pbccs_amd import synth
    return [polish_gated(z["draft"], z["reads"], z["snr"]) for z in synth.make_zmws(n, length, passes, seed=seed)]

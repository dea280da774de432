"""A literal Python restatement of the subread-pileup rules, written apart from the kernels: one
cursor pair moved by the transcript's characters, dictionaries and lists, no scan.  A helper, not a test."""
import math

CODES = "ACGT"
GAP, OTHER = 4, 5
_COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}


def oriented(seq, rc):
    """The read as placed: itself, or its reverse complement with N for every character outside ACGT."""
    return "".join(_COMP.get(c, "N") for c in reversed(seq)) if rc else seq


def code_of(ch):
    return CODES.index(ch) if ch in CODES else OTHER


def status_of(r):
    """used / empty_extent for a read given by transcript; a read with "skip" keeps that status."""
    if r is None:
        return "unmapped"
    if r.get("skip"):
        return r["skip"]
    tr = r["transcript"]
    if not any(c in "MRD" for c in tr) or not any(c in "MRI" for c in tr):
        return "empty_extent"
    return "used"


def walk(r):
    """(cells, ins): cells[p] = the oriented base at consensus position p or "-" for a D column; ins[s] = the
    inserted bases at slot s ("" where there are none), for every slot of [tb, te]."""
    o = oriented(r["seq"], r["rc"])
    p, q = r["tb"], r["rb"]
    cells, ins = {}, {r["tb"]: ""}
    for ch in r["transcript"]:
        if ch in "MR":
            cells[p] = o[q]
            p += 1
            q += 1
            ins[p] = ""
        elif ch == "D":
            cells[p] = "-"
            p += 1
            ins[p] = ""
        elif ch == "I":
            ins[p] += o[q]
            q += 1
        else:
            raise ValueError(ch)
    assert p == r["te"] and q <= len(o)
    return cells, ins, q


def pileup(consensus, reads):
    """reads: dicts with transcript, seq, rc, rb, tb, te (or None / with "skip").  Returns what pileup_columns
    returns for one ZMW."""
    L = len(consensus)
    counts = [[[0] * 6 for _ in range(L)] for _ in (0, 1)]
    ins_reads = [[0] * (L + 1) for _ in (0, 1)]
    ins_bases = [[0] * (L + 1) for _ in (0, 1)]
    slot_cov = [0] * (L + 1)
    max_ins = [0] * (L + 1)
    per_read, n_used = [], [0, 0]
    for r in reads:
        st = status_of(r)
        rec = {"status": st, "n_match": 0, "n_mismatch": 0, "n_ins": 0, "n_del": 0, "concordance": float("nan")}
        if r is not None and "transcript" in r:
            rec.update(rc=1 if r["rc"] else 0, rb=r["rb"], tb=r["tb"], te=r["te"])
        per_read.append(rec)
        if st != "used":
            continue
        tr = r["transcript"]
        s = 1 if r["rc"] else 0
        n_used[s] += 1
        cells, ins, q_end = walk(r)
        rec.update(n_match=tr.count("M"), n_mismatch=tr.count("R"), n_ins=tr.count("I"), n_del=tr.count("D"), re=q_end)
        rec["concordance"] = tr.count("M") / len(tr)
        for p, ch in cells.items():
            counts[s][p][GAP if ch == "-" else code_of(ch)] += 1
        for slot, bases in ins.items():
            slot_cov[slot] += 1
            if bases:
                ins_reads[s][slot] += 1
                ins_bases[s][slot] += len(bases)
                max_ins[slot] = max(max_ins[slot], len(bases))
    cov = [sum(counts[0][p]) + sum(counts[1][p]) for p in range(L)]
    plurality = []
    for p in range(L):
        J = [counts[0][p][c] + counts[1][p][c] for c in range(5)]
        best = max(J)
        if best == 0:
            plurality.append(255)
            continue
        tied = [c for c in range(5) if J[c] == best]
        own = code_of(consensus[p])
        plurality.append(own if own in tied else tied[0])
    ins_plur = [1 if 2 * (ins_reads[0][s] + ins_reads[1][s]) > slot_cov[s] else 0 for s in range(L + 1)]
    sites = []
    for p in range(L + 1):
        if ins_plur[p]:
            sites.append(("ins", p, consensus[p] if p < L else "", "+"))
        if p < L and plurality[p] != 255 and plurality[p] != code_of(consensus[p]):
            sites.append(("del", p, consensus[p], "-") if plurality[p] == GAP
                         else ("sub", p, consensus[p], CODES[plurality[p]]))
    cov_sum = sum(cov)
    return {"counts": counts, "ins_reads": ins_reads, "ins_bases": ins_bases, "slot_cov": slot_cov, "max_ins": max_ins,
            "cov": cov, "plurality": plurality, "ins_plurality": ins_plur, "plurality_sites": sites,
            "cov_sum": cov_sum, "ec": cov_sum / L if L else 0.0, "n_used": n_used, "reads": per_read}


def msa(consensus, reads):
    """{"width", "col", "rows"}: the gapped rows, cell by cell from the rules."""
    L = len(consensus)
    walked = [walk(r)[:2] + (r,) if status_of(r) == "used" else None for r in reads]
    max_ins = [0] * (L + 1)
    for w in walked:
        if w:
            for s, bases in w[1].items():
                max_ins[s] = max(max_ins[s], len(bases))
    first = [s + sum(max_ins[:s]) for s in range(L + 1)]
    col = [first[p] + max_ins[p] for p in range(L)]
    width = L + sum(max_ins)
    rows = []
    for w in walked:
        row = [" "] * width
        if w:
            cells, ins, r = w
            for p, ch in cells.items():
                row[col[p]] = ch
            for s, bases in ins.items():
                k = len(bases)
                at = first[s] + max_ins[s] - k if s == r["tb"] else first[s]
                row[at:at + k] = bases
                if r["tb"] < s < r["te"]:
                    for c in range(first[s] + k, first[s] + max_ins[s]):
                        row[c] = "-"
        rows.append("".join(row))
    return {"width": width, "col": col, "rows": rows}


def cigar(transcript, rb, read_len):
    """rb S, the runs (M -> =, R -> X, I, D), read_len - re S; no zero-length clips."""
    out = [f"{rb}S"] if rb else []
    runs = []
    for ch in transcript:
        op = {"M": "=", "R": "X", "I": "I", "D": "D"}[ch]
        if runs and runs[-1][0] == op:
            runs[-1][1] += 1
        else:
            runs.append([op, 1])
    out += [f"{n}{op}" for op, n in runs]
    tail = read_len - rb - sum(ch in "MRI" for ch in transcript)
    if tail:
        out.append(f"{tail}S")
    return "".join(out)


def batch(consensus, reads, placements, transcripts):
    """The restatement fed with the public map_batch / align_batch results.  reads: {"seq"} or None; placements:
    map_batch's entries (None: not mapped); transcripts: per read the Align transcript or None."""
    rs = []
    for r, pl, tr in zip(reads, placements, transcripts):
        if r is None or pl is None:
            rs.append(None)
            continue
        (rb, re_), (tb, te) = pl["read"], pl["tpl"]
        d = {"seq": r["seq"], "rc": 1 if pl["rc"] else 0, "rb": rb, "tb": tb, "te": te, "transcript": tr or ""}
        if re_ <= rb or te <= tb:
            d["skip"] = "empty_extent"
        elif tr is None:
            d["skip"] = "align_failed"
        rs.append(d)
    return pileup(consensus, rs)


def same_concordance(a, b):
    return (math.isnan(a) and math.isnan(b)) or a == b

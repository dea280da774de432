"""Shared by tests/test_arrow_multibase_cpu.py and tests/test_arrow_multibase_gpu.py: the slipped-repeat ZMW
generator, the CPU restatement's refill likelihoods (the reference value of a wide score) and the measurement of
the single-base gap g1 between ScoreMutation and a refill.  Everything here runs on the CPU with oracle/ alone.

    python -m tests.arrow_multibase_common search   # the seeds behind tests/golden/arrow_repeat_slips.json
    python -m tests.arrow_multibase_common g1       # the constants G1 and EXCLUDED_CLASSES below
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import oracle as O  # noqa: E402
from pbccs_amd import Mutation  # noqa: E402
from pbccs_amd import quiver as Q  # noqa: E402  (host-only helpers: ApplyMutations, RepeatMutationEnumerator)

INS, DEL, SUB = 0, 1, 2
SNR = [10.0, 7.0, 5.0, 11.0]
BASES = np.frombuffer(b"ACGT", dtype=np.uint8)
COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}
SLIPS = os.path.join(ROOT, "tests", "golden", "arrow_repeat_slips.json")
MIN_MARGIN = 0.04   # MIN_FAVORABLE_SCOREDIFF


def revcomp(s):
    return "".join(COMP[c] for c in reversed(s))


def noisy(rng, seq, p_ins=0.04, p_del=0.03, p_sub=0.01):
    """A read of `seq` at about 8 % error."""
    out = []
    for c in seq:
        while rng.random() < p_ins:
            out.append("ACGT"[int(rng.integers(0, 4))])
        if rng.random() < p_del:
            continue
        if rng.random() < p_sub:
            c = "ACGT"[("ACGT".index(c) + int(rng.integers(1, 4))) % 4]
        out.append(c)
    return "".join(out)


def slip_zmw(seed, unit_len=2, n_reads=6):
    """30 random bases + (unit) x 5..8 + 30 random bases; the draft is the truth with one element more or less;
    six reads of the truth, alternating strands, each mapped to the whole draft."""
    rng = np.random.Generator(np.random.PCG64(seed))
    rnd = lambda n: "".join("ACGT"[int(x)] for x in rng.integers(0, 4, size=n))   # noqa: E731
    while True:
        unit = rnd(unit_len)
        if len(set(unit)) > 1:
            break
    k = int(rng.integers(5, 9))
    left, right = rnd(30), rnd(30)
    truth = left + unit * k + right
    dk = k + (1 if rng.random() < 0.5 else -1)
    draft = left + unit * dk + right
    reads = []
    for i in range(n_reads):
        s = noisy(rng, truth)
        reads.append({"seq": revcomp(s) if i % 2 else s, "strand": i % 2, "ts": 0, "te": len(draft)})
    return {"seed": seed, "unit": unit, "truth": truth, "draft": draft, "snr": SNR, "reads": reads}


def oracle_on(tpl, reads, windows=None, snr=SNR):
    s = O.Scorer(tpl, snr)
    for k, r in enumerate(reads):
        ts, te = windows[k] if windows else (r["ts"], r["te"])
        s.add_read(r["seq"], r["strand"], ts, te)
    return s


def read_lls(tpl, reads, windows=None, snr=SNR):
    """Per read (active, LL) of a fresh CPU scorer on tpl."""
    s = oracle_on(tpl, reads, windows, snr)
    info = [s.read_info(k) for k in range(s.num_reads())]
    return [(i["active"], i["ll"]) for i in info]


def apply_wide(tpl, m):
    """T' = apply_mutations(T, [m]) and the target-to-query map (host only)."""
    return Q.ApplyMutations([m], tpl)


def refill_deltas(tpl, reads, m, snr=SNR, base=None):
    """LL_r(T') - LL_r(T) per read from two unmodified CPU scorers, the read windows remapped through mtp; None
    for a read that is inactive on either template."""
    base = base or read_lls(tpl, reads, None, snr)
    t2, mtp = apply_wide(tpl, m)
    win = [(mtp[r["ts"]], mtp[r["te"]]) for r in reads]
    after = read_lls(t2, reads, win, snr)
    return [(b[1] - a[1]) if (a[0] and b[0]) else None for a, b in zip(base, after)]


def scores_read(m, r):
    """ReadScoresMutation (Arrow/MultiReadMutationScorer.cpp:70-80)."""
    if m.type == INS:
        return r["ts"] <= m.end and m.start <= r["te"]
    return r["ts"] < m.end and m.start < r["te"]


def overhangs(m, r):
    return m.start < r["ts"] or m.end > r["te"]


def mutation_class(m, L):
    """The class a mutation's gap to the refill is measured in: its type and how close it lies to the template's
    two ends (capped at 3, where ScoreMutation's edge cases end)."""
    return (m.type, min(m.start, 3), min(L - m.end, 3))


def g1_measure(zmw):
    """Largest |orc_scorer_scores - refill| per class over every unique single-base mutation of the ZMW's template."""
    tpl, reads = zmw["tpl"], zmw["reads"]
    s = oracle_on(tpl, reads)
    base = read_lls(tpl, reads)
    per_class = {}
    for (t, p, b) in O.unique_mutations(tpl):
        m = Mutation(t, p, b)
        got = s.scores(t, p, b)
        want = refill_deltas(tpl, reads, m, base=base)
        for k, r in enumerate(reads):
            if want[k] is None or not scores_read(m, r) or overhangs(m, r):
                continue
            c = mutation_class(m, len(tpl))
            per_class[c] = max(per_class.get(c, 0.0), abs(got[k] - want[k]))
    return per_class


def score_zmws():
    """The two 74-base ZMWs of the wide-score comparison: the truth of a 7-element slip ZMW as the template, its six
    reads on the whole template."""
    out = []
    seed = 0
    while len(out) < 2:
        z = slip_zmw(seed)
        seed += 1
        if len(z["truth"]) != 74:
            continue
        reads = [dict(r, te=74) for r in z["reads"]]
        out.append({"tpl": z["truth"], "snr": SNR, "reads": reads, "seed": z["seed"]})
    return out


def repeat_candidates(tpl, unit_len, min_elements=3):
    return Q.RepeatMutationEnumerator(tpl, unit_len, min_elements).Mutations()


def summed_margin(tpl_a, tpl_b, reads_a, reads_b):
    """sum over reads of LL(tpl_b) - LL(tpl_a), over the reads active on both."""
    a = read_lls(tpl_a, reads_a)
    b = read_lls(tpl_b, reads_b)
    return sum(y[1] - x[1] for x, y in zip(a, b) if x[0] and y[0])


def qualify(z, unit_len):
    """None, or the fixture record of a slip ZMW the CPU restatement's RefineConsensus stalls on: it ends on a
    template that is not the truth, one repeat candidate of that template gives the truth, and the truth's refill
    likelihood summed over the reads beats the stalled template's by more than 0.04."""
    s = oracle_on(z["draft"], z["reads"])
    ref = s.refine()
    final = s.template()
    if final == z["truth"] or not ref["converged"]:
        return None
    wins = [(s.read_info(k)["ts"], s.read_info(k)["te"]) for k in range(s.num_reads())]
    hit = [m for m in repeat_candidates(final, unit_len) if apply_wide(final, m)[0] == z["truth"]]
    if not hit:
        return None
    m = hit[0]
    _, mtp = apply_wide(final, m)
    reads_f = [dict(r, ts=w[0], te=w[1]) for r, w in zip(z["reads"], wins)]
    reads_t = [dict(r, ts=mtp[w[0]], te=mtp[w[1]]) for r, w in zip(z["reads"], wins)]
    margin = summed_margin(final, z["truth"], reads_f, reads_t)
    if not margin > MIN_MARGIN:
        return None
    return {"seed": z["seed"], "unit_len": unit_len, "truth": z["truth"], "draft": z["draft"], "snr": z["snr"],
            "reads": z["reads"], "oracle_final": final, "oracle_n_tested": ref["n_tested"],
            "oracle_n_applied": ref["n_applied"], "margin": margin}


def load_slips():
    return json.load(open(SLIPS))


def _main(argv):
    if argv[:1] == ["g1"]:
        for z in score_zmws():
            pc = g1_measure(z)
            small = max(v for v in pc.values() if v <= 1e-6)
            print("seed", z["seed"], "g1", repr(small), "excluded", sorted(c for c, v in pc.items() if v > 1e-6),
                  [repr(v) for c, v in sorted(pc.items()) if v > 1e-6])
    elif argv[:1] == ["search"]:
        n = int(argv[1]) if len(argv) > 1 else 40
        for unit_len in (2, 3):
            for seed in range(n):
                rec = qualify(slip_zmw(seed, unit_len), unit_len)
                print("unit", unit_len, "seed", seed, "->", None if rec is None else round(rec["margin"], 3),
                      flush=True)
    elif argv[:1] == ["write"]:
        picks = [(int(a.split(":")[0]), int(a.split(":")[1])) for a in argv[1:]]
        recs = [qualify(slip_zmw(seed, ul), ul) for ul, seed in picks]
        assert all(r is not None for r in recs)
        json.dump(recs, open(SLIPS, "w"), indent=1)
        print("wrote", SLIPS, [round(r["margin"], 3) for r in recs])


if __name__ == "__main__":
    _main(sys.argv[1:])

"""Shared by tests/test_strand_cpu.py, tests/test_strand_gpu.py and tests/test_cpp_strand.py: the heteroduplex ZMW
generator behind tests/golden/strand_zmws.json and the CPU restatement of the strand screen over oracle scores
(DESIGN.md §3.23).  Everything here runs on the CPU with oracle/ alone.

    python -m tests.strand_common search [n]      # which seeds meet conditions (a)-(d)
    python -m tests.strand_common make 4 6 ...    # write the fixture from the given seeds

Recipe per ZMW, in this order: PCG64(seed); truth = 150 iid bases; alt = truth with the base at 75 moved one step in
ACGT order; draft = synth._mutate(truth, .005, .005, .002); 12 passes of synth._mutate(src, .07, .04, .01), src = alt
on the odd passes (reverse-complemented, strand 1) and the truth on the even ones.  The homoduplex control of a seed
is the same draw with alt = truth.
"""
import json
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import oracle as O  # noqa: E402
from pbccs_amd import synth  # noqa: E402
from tests import strand_restatement as R  # noqa: E402

SNR = [10.0, 7.0, 5.0, 11.0]
LENGTH, SITE, PASSES = 150, 75, 12
MIN_SCORE, MIN_READS = R.DEFAULT_MIN_SCORE, R.DEFAULT_MIN_READS
MIN_ZSCORE = -5.0
FIXTURE = os.path.join(ROOT, "tests", "golden", "strand_zmws.json")
NAN = float("nan")


def make_zmw(seed, hetero=True):
    rng = np.random.Generator(np.random.PCG64(seed))
    truth = synth.BASES[rng.integers(0, 4, size=LENGTH)]
    alt = truth.copy()
    if hetero:
        alt[SITE] = synth.BASES[(int(np.searchsorted(synth.BASES, truth[SITE])) + 1) % 4]
    draft = synth._mutate(rng, truth, 0.005, 0.005, 0.002)
    reads = []
    for k in range(PASSES):
        r = synth._mutate(rng, alt if k % 2 else truth, 0.07, 0.04, 0.01)
        if k % 2:
            r = synth.COMP[r[::-1]]
        reads.append({"seq": r.tobytes().decode(), "strand": k % 2, "ts": 0, "te": int(draft.shape[0])})
    return {"seed": seed, "hetero": bool(hetero), "truth": truth.tobytes().decode(), "alt": alt.tobytes().decode(),
            "draft": draft.tobytes().decode(), "snr": list(SNR), "reads": reads}


def single_strand(zmw, strand):
    """The hand-built ZMW with only one strand's reads, in their original order and windows."""
    return {"draft": zmw["draft"], "snr": zmw["snr"], "reads": [r for r in zmw["reads"] if r["strand"] == strand]}


def oracle_polished(zmw):
    """The CPU restatement's scorer after the batch polish's AddRead gate and RefineConsensus: (scorer, refine)."""
    s = O.Scorer(zmw["draft"], zmw["snr"])
    for r in zmw["reads"]:
        s.add_read(r["seq"], r["strand"], r["ts"], r["te"], MIN_ZSCORE)
    return s, s.refine()


def oracle_sums(s, strands, mutations=None):
    """[(type, pos, base)], [strand_sums] of the scorer's current template from oracle.Scorer.scores per read (NaN
    marks a read that does not enter the sums)."""
    muts = mutations if mutations is not None else O.unique_mutations(s.template())
    sums = []
    for t, p, b in muts:
        per = [None if math.isnan(v) else v for v in s.scores(t, p, b, NAN)]
        sums.append(R.strand_sums(per, strands))
    return muts, sums


def oracle_sites(s, strands, min_score=MIN_SCORE, min_reads=MIN_READS):
    muts, sums = oracle_sums(s, strands)
    return R.strand_sites(muts, sums, min_score, min_reads), sums


def threshold_distance(sums, min_score=MIN_SCORE):
    """The smallest distance of any strand sum from +-min_score (condition (d))."""
    return min(min(abs(abs(v) - min_score) for v in s[:2]) for s in sums)


def qualify(seed):
    """None, or the fixture records (heteroduplex, control) of a seed that meets (a)-(d)."""
    out = []
    for hetero in (True, False):
        z = make_zmw(seed, hetero)
        s, ref = oracle_polished(z)
        if not ref["converged"]:
            return None                                                        # (a)
        strands = [r["strand"] for r in z["reads"]]
        sites, sums = oracle_sites(s, strands)
        if hetero and not any(x[0] in (SITE, SITE + 1) for x in sites):
            return None                                                        # (b)
        if not hetero and sites:
            return None
        if threshold_distance(sums) < 1e-6:
            return None                                                        # (d)
        finals = []
        for strand, want in ((0, z["truth"]), (1, z["alt"])):
            sub = single_strand(z, strand)
            e = O.polish_zmw(sub["draft"], sub["reads"], sub["snr"], qvs=False)
            if not e["converged"] or e["template"] != want:
                return None                                                    # (c)
            finals.append(e["template"])
        z["oracle_final"] = s.template()
        z["oracle_sites"] = [list(x) for x in sites]
        z["oracle_fwd_final"], z["oracle_rev_final"] = finals
        out.append(z)
    return out


def revcomp(s):
    return synth.COMP[np.frombuffer(s.encode(), dtype=np.uint8)[::-1]].tobytes().decode()


def scorer_case():
    """A 64-base template with five reads for the per-strand sums: both strands, read 2 on the partial window
    [5, 58), read 3 a junk read that AddRead's z-score gate (-5) rejects, so it is inactive."""
    rng = np.random.Generator(np.random.PCG64(23))
    tpl = synth.BASES[rng.integers(0, 4, size=64)]
    reads = []
    for k in range(5):
        ts, te = (5, 58) if k == 2 else (0, 64)
        strand = k % 2
        if k == 3:
            seq = ("ACGT" * 16)
        else:
            seq = synth._mutate(rng, tpl[ts:te], 0.07, 0.04, 0.01).tobytes().decode()
        reads.append({"seq": revcomp(seq) if strand else seq, "strand": strand, "ts": ts, "te": te})
    return tpl.tobytes().decode(), reads


def load_fixture():
    return json.load(open(FIXTURE))


def polish_inputs(zmws):
    return [{"draft": z["draft"], "snr": z["snr"], "reads": z["reads"]} for z in zmws]


def _main(argv):
    if argv[:1] == ["search"]:
        n = int(argv[1]) if len(argv) > 1 else 12
        for seed in range(1, n + 1):
            rec = qualify(seed)
            print("seed", seed, "->", None if rec is None else [tuple(x[:3]) for x in rec[0]["oracle_sites"]], flush=True)
    elif argv[:1] == ["make"]:
        recs = []
        for seed in [int(a) for a in argv[1:]]:
            rec = qualify(seed)
            assert rec is not None, seed
            recs += rec
        json.dump(recs, open(FIXTURE, "w"), indent=1)
        print("wrote", FIXTURE, len(recs), "ZMWs")


if __name__ == "__main__":
    _main(sys.argv[1:])

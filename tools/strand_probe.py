#!/usr/bin/env python3
"""Measures what the strand-discordance screen and the directional polish cost and how well the
screen separates heteroduplex molecules from ordinary ones, and writes profiles/strand.json.

Shape: 2 kb inserts, 10 passes, synth's read errors (7 / 4 / 1 %); --zmws ZMWs (600) per polish_zmws call.  A
--hetero-share (0.1) of them are heteroduplexes: their odd passes (the reverse strand) are read from the truth with
one substitution planted at the middle of the insert, as tests/strand_common.py plants it.

Legs, each timed --repeat times in alternating order in one process after one warm-up call per leg: the keywords off,
strand_sites=True, directional="discordant", directional="always".  With profiling on, one more strand_sites=True
call gives the two kernels' device time (pbccs_engine_kernel_stats) beside the QV sweep's k_score and k_qv.
Sensitivity = heteroduplex ZMWs with a site within one base of the planted position (and, beside it, within five:
an indel-shaped report of the difference lands where the aligner puts it in the local repeat); false positives =
ordinary ZMWs with any site, and sites of heteroduplex ZMWs farther than five bases away.
Not a test and not part of bench.py.  Usage: strand_probe.py [--out profiles/strand.json]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_work(n, share, seed, length=2000, passes=10):
    import numpy as np
    from pbccs_amd import synth
    rng = np.random.Generator(np.random.PCG64(seed))
    out = []
    for i in range(n):
        hetero = (i % max(1, round(1 / share))) == 0 if share > 0 else False
        truth = synth.BASES[rng.integers(0, 4, size=length)]
        alt = truth.copy()
        site = length // 2
        if hetero:
            alt[site] = synth.BASES[(int(np.searchsorted(synth.BASES, truth[site])) + 1) % 4]
        draft = synth._mutate(rng, truth, 0.005, 0.005, 0.002)
        reads = []
        for k in range(passes):
            r = synth._mutate(rng, alt if k % 2 else truth, 0.07, 0.04, 0.01)
            if k % 2:
                r = synth.COMP[r[::-1]]
            reads.append({"seq": r.tobytes().decode(), "strand": k % 2, "ts": 0, "te": int(draft.shape[0])})
        # the planted position in the truth's coordinates; the consensus' may differ by the draft's indels, which
        # RefineConsensus removes, so the final template's coordinates are the truth's when it converges on it
        out.append({"draft": draft.tobytes().decode(), "snr": [10.0, 7.0, 5.0, 11.0], "reads": reads,
                    "hetero": hetero, "site": site})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "strand.json"))
    ap.add_argument("--zmws", type=int, default=600)
    ap.add_argument("--hetero-share", type=float, default=0.1)
    ap.add_argument("--repeat", type=int, default=3)
    a = ap.parse_args()
    import pbccs_amd as P
    work = make_work(a.zmws, a.hetero_share, 1)
    warm = make_work(64, a.hetero_share, 1001)
    inputs = [{k: z[k] for k in ("draft", "snr", "reads")} for z in work]
    warm_in = [{k: z[k] for k in ("draft", "snr", "reads")} for z in warm]
    eng = P.Engine(0)
    legs = [("off", {}), ("strand_sites", {"strand_sites": True}), ("discordant", {"directional": "discordant"}),
            ("always", {"directional": "always"})]
    for _, kw in legs:
        P.polish_zmws(warm_in, engine=eng, **kw)
    walls = {name: [] for name, _ in legs}
    last = {}
    for rep in range(a.repeat):
        for name, kw in (legs if rep % 2 == 0 else legs[::-1]):
            t0 = time.perf_counter()
            last[name] = P.polish_zmws(inputs, engine=eng, **kw)
            walls[name].append(round(time.perf_counter() - t0, 4))
            print(rep, name, walls[name][-1], flush=True)
    n_het = sum(1 for z in work if z["hetero"])
    hit = hit5 = miss = fp_zmws = fp_sites = stray = 0
    for z, r in zip(work, last["strand_sites"]):
        sites = r["strand_sites"]
        if z["hetero"]:
            # (the final template's coordinates are the truth's up to the consensus' own residual indels)
            near = [s for s in sites if abs(s.pos - z["site"]) <= 1]
            near5 = [s for s in sites if abs(s.pos - z["site"]) <= 5]
            hit += 1 if near else 0
            hit5 += 1 if near5 else 0
            miss += 0 if near5 else 1
            stray += len(sites) - len(near5)
        elif sites:
            fp_zmws += 1
            fp_sites += len(sites)
    split = sum(1 for r in last["discordant"] if "fwd" in r)
    eng.set_profiling(True)
    eng.kernel_stats(reset=True)
    P.strand_stats(eng, reset=True)
    P.polish_zmws(inputs, engine=eng, strand_sites=True)
    ks = eng.kernel_stats(reset=True)
    doc = {"shape": f"2000 bp, 10 passes, {a.zmws} ZMWs per polish_zmws call, {n_het} heteroduplexes "
                    f"(one substitution at 1000 on the reverse strand)", "repeat": a.repeat,
           "wall_s": walls, "median_wall_s": {k: sorted(v)[len(v) // 2] for k, v in walls.items()},
           "statuses": {name: {s: sum(1 for r in res if r["status"] == s) for s in {r["status"] for r in res}}
                        for name, res in last.items()},
           "screen": {"heteroduplex_zmws": n_het, "found_within_1": hit, "found_within_5": hit5, "missed": miss,
                      "sites_farther_than_5_in_heteroduplex_zmws": stray,
                      "ordinary_zmws": len(work) - n_het, "ordinary_zmws_with_sites": fp_zmws,
                      "sites_in_ordinary_zmws": fp_sites, "min_score": 12.5, "min_reads": 2},
           "discordant_split_zmws": split, "strand_stats": P.strand_stats(eng, reset=True),
           "device_ms_profiled": {k: {"launches": ks[k]["launches"], "device_ms": round(ks[k]["device_ms"], 4)}
                                  for k in ("k_score", "k_reduce", "k_qv", "k_strand_sums", "k_strand_sites")}}
    res_path = os.path.join(ROOT, "pbccs_amd", "_lib", "kernel_resources.json")
    if os.path.exists(res_path):
        doc["kernel_resources"] = {k: v for k, v in json.load(open(res_path)).items() if "k_strand_" in k}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", a.out)
    print(json.dumps({k: doc[k] for k in ("median_wall_s", "screen", "device_ms_profiled")}))


if __name__ == "__main__":
    main()

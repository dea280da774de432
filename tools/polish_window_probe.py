#!/usr/bin/env python3
"""Measures the windowed polish (pbccs_polish_windowed) against the whole-template route and writes
profiles/polish_window.json.

Shapes, from synth.make_zmws: 2 kb x 10 passes, 10 kb x 8 passes, 20 kb x 6 passes.  One shape per process
(--shape NAME --part FILE); --merge FILE... joins the parts into --out.  Per shape and per (window, k) of the sweep
window {1000, 2000, 4000} x k {6, 8} (overlap 200, guard 8): after one warm-up call of each route, three repeats of
"the whole-template route (polish_stream: pbccs_polish_batch), then the windowed route under each (window, k)", all
in one process on one engine, so the two routes alternate and each is timed three times (--budget-s: no further
repeat starts after that many seconds; the record says how many ran).  Recorded: every wall time and the medians,
the spread of the whole-template route's times over the shape as the noise floor, the windowed route's split (seeds
and cuts, window polish, align and join, fallback polish; pbccs_window_stats of the median run), the fallback share
by reason and the failed windows by status, the share of ZMWs whose stitched consensus equals the whole-template
consensus, and for the ZMWs that differ the edit distance of both consensuses to the synthetic truth (Align on the
GPU, 0 -1 -1 -1).
Not a test and not part of bench.py.
Usage: polish_window_probe.py --shape 10kb --part part_10kb.json
       polish_window_probe.py --merge part_2kb.json part_10kb.json part_20kb.json --out profiles/polish_window.json"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = {"2kb": dict(length=2000, passes=10, n=512, seed=1), "10kb": dict(length=10000, passes=8, n=96, seed=2),
          "20kb": dict(length=20000, passes=6, n=32, seed=3)}
SWEEP = [(w, k) for w in (1000, 2000, 4000) for k in (6, 8)]
OVERLAP, GUARD, REPEAT = 200, 8, 3


def edit_distances(A, eng, pairs):
    if not pairs:
        return []
    rc, res = A.align_batch_raw(pairs, A.NW, None, engine=eng)
    if rc != 0:
        raise RuntimeError(f"align_batch failed ({rc})")
    return [-int(r[1]) for r in res]


def measure(shape, budget_s):
    sys.path.insert(0, ROOT)
    import pbccs_amd
    from pbccs_amd import align as A
    from pbccs_amd import polish as P
    from pbccs_amd import synth
    spec = SHAPES[shape]
    zmws = synth.make_zmws(spec["n"], spec["length"], spec["passes"], seed=spec["seed"])
    eng = pbccs_amd.Engine(0)
    out = {"shape": shape, "zmws": spec["n"], "length": spec["length"], "passes": spec["passes"], "overlap": OVERLAP,
           "guard": GUARD, "configs": []}
    t_begin = time.perf_counter()
    P.polish_stream(zmws, engine=eng)   # warm-up: pools mapped, kernels loaded
    P.polish_windowed(zmws, engine=eng, window=SWEEP[0][0], overlap=OVERLAP, guard=GUARD, k=SWEEP[0][1])
    whole_all, whole = [], None
    tv = {c: [] for c in SWEEP}
    splits = {c: [] for c in SWEEP}
    got = {}
    for rep in range(REPEAT):
        if rep and time.perf_counter() - t_begin > budget_s:   # a bounded step: fewer repeats, said in the record
            break
        t0 = time.perf_counter()
        whole = P.polish_stream(zmws, engine=eng)
        whole_all.append(time.perf_counter() - t0)
        for window, k in SWEEP:
            P.window_stats(eng, reset=True)
            t0 = time.perf_counter()
            got[(window, k)] = P.polish_windowed(zmws, engine=eng, window=window, overlap=OVERLAP, guard=GUARD, k=k)
            tv[(window, k)].append(time.perf_counter() - t0)
            splits[(window, k)].append(P.window_stats(eng, reset=True))
        print(f"repeat {rep}: whole {whole_all[-1]:.3f} s, windowed " +
              " ".join(f"{tv[c][-1]:.3f}" for c in SWEEP), flush=True)
    out["repeats"] = len(whole_all)
    tw = whole_all
    ok = [i for i, w in enumerate(whole) if w["status"] == "Success"]
    for window, k in SWEEP:
        g, t = got[(window, k)], tv[(window, k)]
        med = sorted(range(len(t)), key=lambda i: t[i])[len(t) // 2]
        same = [i for i in ok if g[i]["consensus"] == whole[i]["consensus"]]
        differ = [i for i in ok if i not in same and g[i]["status"] == "Success"]
        dw = edit_distances(A, eng, [(zmws[i]["truth"], whole[i]["consensus"]) for i in differ])
        dv = edit_distances(A, eng, [(zmws[i]["truth"], g[i]["consensus"]) for i in differ])
        s = splits[(window, k)][med]
        bad = {}
        for r in g:
            if r["fallback"] == 1:
                for w in r["windows"]:
                    if w["status"] != 0:
                        name = pbccs_amd.ZMW_STATUS[w["status"]]
                        bad[name] = bad.get(name, 0) + 1
        out["configs"].append({
            "window": window, "k": k, "whole_s": tw, "windowed_s": t,
            "whole_median_s": statistics.median(tw), "windowed_median_s": statistics.median(t),
            "ratio_whole_over_windowed": statistics.median(tw) / statistics.median(t),
            "split_ms": {"seeds_and_cuts": s["slices_ms"], "window_polish": s["polish_ms"],
                         "align_and_join": s["join_ms"], "fallback_polish": s["fallback_ms"]},
            "windowed_zmws": s["zmws"], "windows": s["windows"], "unanchored_reads": s["unanchored_reads"],
            "fallbacks_by_reason": {"window_status": s["fallbacks"][1], "no_join": s["fallbacks"][2],
                                    "accuracy": s["fallbacks"][3]},
            "failed_windows_by_status": bad,
            "fallback_share": sum(s["fallbacks"]) / max(1, spec["n"]),
            "whole_success": len(ok), "windowed_success": sum(1 for r in g if r["status"] == "Success"),
            "identical_share_of_whole_success": len(same) / max(1, len(ok)),
            "differing": [{"zmw": i, "whole_to_truth": a, "windowed_to_truth": b} for i, a, b in zip(differ, dw, dv)],
        })
        print(json.dumps(out["configs"][-1]), flush=True)
    out["whole_noise_floor"] = {"min_s": min(whole_all), "max_s": max(whole_all), "median_s": statistics.median(whole_all),
                                "spread": (max(whole_all) - min(whole_all)) / statistics.median(whole_all)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=sorted(SHAPES))
    ap.add_argument("--part")
    ap.add_argument("--budget-s", type=float, default=1e9, help="start no further repeat after this many seconds")
    ap.add_argument("--merge", nargs="*")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "polish_window.json"))
    a = ap.parse_args()
    if a.merge:
        parts = [json.load(open(p)) for p in a.merge]
        doc = {"tool": "tools/polish_window_probe.py", "gpus": 1,
               "method": "per shape, one process and engine: after a warm-up of each route, `repeats` rounds of the "
                         "whole-template route followed by the windowed route under each (window, k); medians; noise "
                         "floor = spread of the whole-template times of the shape",
               "shapes": parts}
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
        return 0
    res = measure(a.shape, a.budget_s)
    with open(a.part, "w") as f:
        json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())

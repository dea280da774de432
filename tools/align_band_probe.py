#!/usr/bin/env python3
"""Measures the certified banded fill (pbccs_align_batch_ex) against the unbanded align_batch and
writes profiles/align_band.json.  The method is profiles/align_batch.json's: best of 5 calls, fill and trace device
ms from the engine's event counters (profiling on), wall ms around the whole call including marshalling.

Shapes: 64 pairs of 5000 x 5000 at 1% divergence, 32 pairs of 20 kb x 20 kb at 0.2%, 16 pairs of 20 kb x 20 kb at
15% (the certified band is thousands of diagonals wide) and 4096 pairs of 500 x 500 at 15% (where the band is not
expected to pay), each with Align's default parameters and with the default affine parameters.

The unbanded side runs in a child process.  With --baseline-tree DIR (a checkout of the parent commit with its
library built) the child imports pbccs_amd from DIR, so the comparison is against the parent commit's align_batch on
the same box; without it the child runs this tree's unbanded path, and the profile says which.
Not a test and not part of bench.py.  There is no gate: the feature is off by default.
With --rows-sweep the tool instead measures the banded fill of the three long shapes with every rows-per-lane R
forced (PBCCS_ALIGN_ROWS_PER_LANE; best of 3 by fill ms) and adds the table to the profile under
"rows_per_lane_sweep": the basis of band_rows_per_lane's thresholds.
Usage: align_band_probe.py [--out profiles/align_band.json] [--repeat 5] [--baseline-tree DIR] [--rows-sweep]"""
import argparse
import hashlib
import json
import os
import random
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = {"nw": 0, "affine": 1}


def mutated(rng, n, rate):
    q = [rng.choice("ACGT") for _ in range(n)]
    t = []
    for c in q:
        u = rng.random()
        if u < rate / 3:
            continue
        t.append(rng.choice("ACGT") if u < 2 * rate / 3 else c)
        if 2 * rate / 3 <= u < rate:
            t.append(rng.choice("ACGT"))
    while len(t) < n:
        t.append(rng.choice("ACGT"))
    return "".join(t[:n]), "".join(q)


def shapes():
    rng = random.Random(31415)
    return {
        "64 x (5000 x 5000) at 1%": [mutated(rng, 5000, 0.01) for _ in range(64)],
        "32 x (20000 x 20000) at 0.2%": [mutated(rng, 20000, 0.002) for _ in range(32)],
        "16 x (20000 x 20000) at 15%": [mutated(rng, 20000, 0.15) for _ in range(16)],
        "4096 x (500 x 500) at 15%": [mutated(rng, 500, 0.15) for _ in range(4096)],
    }


def measure(tree, banded, repeat):
    """Every shape and kind in this process, with pbccs_amd imported from tree."""
    sys.path.insert(0, tree)
    import pbccs_amd
    from pbccs_amd import align as A
    eng = pbccs_amd.Engine(0)
    eng.set_profiling(True)
    all_shapes = shapes()
    A.align_batch([mutated(random.Random(1), 600, 0.01)] * 4, A.AFFINE, engine=eng)   # warm-up: stream, buffers
    out = {}
    for name, pairs in all_shapes.items():
        for kname, kind in KINDS.items():
            runs = []
            digest = None
            for _ in range(repeat):
                A.align_stats(eng, reset=True)
                if banded:
                    A.align_band_stats(eng, reset=True)
                t0 = time.perf_counter()
                if banded:
                    alns, scores, info = A.align_batch(pairs, kind, engine=eng, band=True, return_info=True)
                else:
                    alns, scores = A.align_batch(pairs, kind, engine=eng)
                wall = (time.perf_counter() - t0) * 1e3
                st = A.align_stats(eng, reset=True)
                run = {"wall_ms": wall, "full_fill_ms": st["fill_ms"], "full_trace_ms": st["trace_ms"],
                       "full_store_bytes": st["bytes"], "full_cells": st["cells"]}
                if banded:
                    b = A.align_band_stats(eng, reset=True)
                    run.update({"band_fill_ms": b["fill_ms"], "band_trace_ms": b["trace_ms"],
                                "band_store_bytes": b["store_bytes"], "band_cells": b["band_cells"],
                                "cells_of_the_banded_pairs": b["full_cells"], "banded_pairs": b["banded_pairs"],
                                "second_attempts": b["second_attempts"],
                                "fallbacks": {k: v for k, v in b["fallbacks"].items() if v},
                                "w_min": min(i["w"] for i in info), "w_max": max(i["w"] for i in info)})
                runs.append(run)
                h = hashlib.sha1()
                for aln, sc in zip(alns, scores):
                    h.update(aln.Transcript().encode() + b" " + float(sc).hex().encode() + b"\n")
                digest = h.hexdigest()
            best = min(runs, key=lambda r: r["wall_ms"])
            out[f"{name} | {kname}"] = {"pairs": len(pairs), "best": best, "runs": runs, "digest": digest}
            print(("banded   " if banded else "unbanded ") + f"{name} | {kname}", json.dumps(best), flush=True)
    return out


def rows_sweep(out_path):
    sys.path.insert(0, ROOT)
    import pbccs_amd
    from pbccs_amd import align as A
    eng = pbccs_amd.Engine(0)
    eng.set_profiling(True)
    table = {}
    for name, pairs in shapes().items():
        if name.startswith("4096"):
            continue
        for kname, kind in KINDS.items():
            for rows in (0, 2, 4, 8):   # 0: the engine's own choice
                os.environ.pop("PBCCS_ALIGN_ROWS_PER_LANE", None)
                if rows:
                    os.environ["PBCCS_ALIGN_ROWS_PER_LANE"] = str(rows)
                runs = []
                for _ in range(3):
                    A.align_band_stats(eng, reset=True)
                    t0 = time.perf_counter()
                    A.align_batch(pairs, kind, engine=eng, band=True)
                    wall = (time.perf_counter() - t0) * 1e3
                    b = A.align_band_stats(eng, reset=True)
                    runs.append({"wall_ms": wall, "band_fill_ms": b["fill_ms"], "band_trace_ms": b["trace_ms"],
                                 "band_store_bytes": b["store_bytes"], "banded_pairs": b["banded_pairs"],
                                 "fallbacks": {k: v for k, v in b["fallbacks"].items() if v}})
                best = min(runs, key=lambda r: r["band_fill_ms"])
                table[f"{name} | {kname} | R={rows or 'chosen'}"] = best
                print(f"{name} | {kname} | R={rows or 'chosen'}", json.dumps(best), flush=True)
    os.environ.pop("PBCCS_ALIGN_ROWS_PER_LANE", None)
    doc = json.load(open(out_path)) if os.path.exists(out_path) else {}
    doc["rows_per_lane_sweep"] = table
    with open(out_path, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", out_path)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "align_band.json"))
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--baseline-tree", default=None)
    ap.add_argument("--rows-sweep", action="store_true")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.rows_sweep:
        rows_sweep(a.out)
        return
    if a.child:   # the unbanded side, in a process of its own
        json.dump(measure(a.child, False, a.repeat), open(a.out, "w"))
        return
    base_tree = os.path.abspath(a.baseline_tree) if a.baseline_tree else ROOT
    tmp = a.out + ".unbanded.tmp"
    env = dict(os.environ)
    env.pop("PBCCS_LIB", None)
    subprocess.check_call([sys.executable, os.path.abspath(__file__), "--child", base_tree, "--out", tmp,
                           "--repeat", str(a.repeat)], env=env)
    unbanded = json.load(open(tmp))
    os.remove(tmp)
    banded = measure(ROOT, True, a.repeat)
    doc = {"method": "best of %d calls by wall ms; device ms from events (profiling on); wall ms around the whole "
                     "align_batch call, marshalling included" % a.repeat,
           "unbanded_side": "parent commit's align_batch (--baseline-tree)" if a.baseline_tree
                            else "this tree's unbanded align_batch (the full-fill path, which this change does not touch)",
           "repeat": a.repeat, "shapes": {}}
    for key, b in banded.items():
        u = unbanded[key]
        bb, ub = b["best"], u["best"]
        dev_b = bb["band_fill_ms"] + bb["band_trace_ms"] + bb["full_fill_ms"] + bb["full_trace_ms"]
        dev_u = ub["full_fill_ms"] + ub["full_trace_ms"]
        doc["shapes"][key] = {
            "pairs": b["pairs"], "unbanded": ub, "banded": bb, "results_equal": b["digest"] == u["digest"],
            "wall_ratio_unbanded_over_banded": ub["wall_ms"] / bb["wall_ms"],
            "device_ratio_unbanded_over_banded": dev_u / dev_b if dev_b else None,
            "store_ratio_banded_over_unbanded": (bb["band_store_bytes"] + bb["full_store_bytes"]) / ub["full_store_bytes"],
            "unbanded_runs_wall_ms": [r["wall_ms"] for r in u["runs"]],
            "banded_runs_wall_ms": [r["wall_ms"] for r in b["runs"]],
        }
        print(key, "wall x%.2f device x%.2f" % (ub["wall_ms"] / bb["wall_ms"], dev_u / dev_b if dev_b else 0.0))
    from pbccs_amd import lib
    res_path = os.path.join(os.path.dirname(lib.LIB_PATH), "kernel_resources.json")
    if os.path.exists(res_path):
        doc["kernel_resources"] = {k: v for k, v in json.load(open(res_path)).items() if "k_align_" in k}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()

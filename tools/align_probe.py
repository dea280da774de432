#!/usr/bin/env python3
"""Measures the batched pairwise aligner (pbccs_align_batch) and writes profiles/align_batch.json.

Three shapes with the default affine parameters: 4096 pairs of 500 x 500, 64 pairs of 5000 x 5000, and 256 copies
of the reference's LargeGap pair (1010 x 1191, tests/golden/align_kats.json).  Per shape: fill and trace device ms
from the engine's counters (profiling on), wall ms of the whole call including marshalling, GCUPS over both, and
the move-store bytes; plus the aligner kernels' register, LDS and waves-per-SIMD lines from kernel_resources.json.
Not a test and not part of bench.py.  Usage: align_probe.py [--out profiles/align_batch.json] [--repeat 3]"""
import argparse
import json
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def mutated(rng, n, rate=0.1):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "align_batch.json"))
    ap.add_argument("--repeat", type=int, default=3)
    a = ap.parse_args()
    import pbccs_amd
    from pbccs_amd import align as A
    from pbccs_amd import lib
    eng = pbccs_amd.Engine(0)
    eng.set_profiling(True)
    rng = random.Random(2718)
    kats = json.load(open(os.path.join(ROOT, "tests", "golden", "align_kats.json")))
    lg = (kats["affine_large_gap"]["target"], kats["affine_large_gap"]["query"])
    shapes = {
        "4096 x (500 x 500)": [mutated(rng, 500) for _ in range(4096)],
        "64 x (5000 x 5000)": [mutated(rng, 5000) for _ in range(64)],
        "256 x LargeGap (1010 x 1191)": [lg] * 256,
    }
    A.align_batch(shapes["256 x LargeGap (1010 x 1191)"][:4], A.AFFINE, engine=eng)   # warm-up: stream, buffers
    doc = {"parameters": "DefaultAffineAlignmentParams (0, -1, -1, -0.5, 0)", "repeat": a.repeat, "shapes": {}}
    for name, pairs in shapes.items():
        runs = []
        for _ in range(a.repeat):
            A.align_stats(eng, reset=True)
            t0 = time.perf_counter()
            A.align_batch(pairs, A.AFFINE, engine=eng)
            wall = (time.perf_counter() - t0) * 1e3
            st = A.align_stats(eng, reset=True)
            runs.append({"wall_ms": wall, "fill_ms": st["fill_ms"], "trace_ms": st["trace_ms"],
                         "launches": st["launches"], "groups": st["groups"], "cells": st["cells"],
                         "trace_steps": st["trace_steps"], "move_store_bytes": st["bytes"],
                         "gcups_fill": st["cells"] / (st["fill_ms"] * 1e6) if st["fill_ms"] else None,
                         "gcups_wall": st["cells"] / (wall * 1e6)})
        best = min(runs, key=lambda r: r["wall_ms"])
        doc["shapes"][name] = {"pairs": len(pairs), "best": best, "runs": runs}
        print(name, json.dumps(best))
    res_path = os.path.join(os.path.dirname(lib.LIB_PATH), "kernel_resources.json")
    if os.path.exists(res_path):
        res = json.load(open(res_path))
        doc["kernel_resources"] = {k: v for k, v in res.items() if "k_align_" in k}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()

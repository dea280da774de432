#!/usr/bin/env python3
"""Measures the ends-free modes of the pairwise aligner (pbccs_align_batch_ends) and writes
profiles/align_modes.json.

Shapes: DESIGN §3.14's two (4096 pairs of 500 x 500, 64 pairs of 5000 x 5000) and 4096 pairs of a 45-base query (the
adapter, noisy) against 20 kb targets.  Each shape runs SEMIGLOBAL, LOCAL and, on the same pairs in the same process,
GLOBAL through pbccs_align_batch (kind NW), all with the scores 3, -5, -4, -4: best of --repeat by wall time; fill
and trace device ms from the align stream's events (profiling on), wall ms of the whole call with marshalling.  On
the 500 x 500 pairs it also times k_map_fill (pbccs_map_batch: LOCAL, both strands, no path) next to LOCAL with both
strands (the same cells, with the path).  The aligner kernels' lines of kernel_resources.json are recorded, and
whether those of the GLOBAL kernels still equal the ones profiles/align_batch.json holds.
Not a test and not part of bench.py.  Usage: align_modes_probe.py [--out profiles/align_modes.json] [--repeat 5]"""
import argparse
import json
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SCORES = (3, -5, -4, -4)


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


def adapter_pair(rng, nrng, n):
    """A random target of n bases holding the adapter with a tenth of its letters redrawn; the query is the adapter."""
    from pbccs_amd import synth
    ad = "".join(c if rng.random() > 0.1 else rng.choice("ACGT") for c in synth.ADAPTER)
    at = rng.randrange(0, n - len(ad))
    t = synth.BASES[nrng.integers(0, 4, size=n)].tobytes().decode()
    return t[:at] + ad + t[at + len(ad):], synth.ADAPTER


def timed(call, stats, repeat):
    runs = []
    for _ in range(repeat):
        stats(True)
        t0 = time.perf_counter()
        call()
        wall = (time.perf_counter() - t0) * 1e3
        st = stats(True)
        st["wall_ms"] = wall
        runs.append(st)
    return min(runs, key=lambda r: r["wall_ms"]), runs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "align_modes.json"))
    ap.add_argument("--repeat", type=int, default=5)
    a = ap.parse_args()
    import pbccs_amd
    from pbccs_amd import align as A
    from pbccs_amd import lib, mapping
    eng = pbccs_amd.Engine(0)
    eng.set_profiling(True)
    import numpy as np
    rng = random.Random(2718)
    nrng = np.random.default_rng(2718)
    shapes = {
        "4096 x (500 x 500)": [mutated(rng, 500) for _ in range(4096)],
        "64 x (5000 x 5000)": [mutated(rng, 5000) for _ in range(64)],
        "4096 x (45 x 20000)": [adapter_pair(rng, nrng, 20000) for _ in range(4096)],
    }
    params = A.AlignParams(*SCORES)

    def align_stats(reset):
        st = A.align_stats(eng, reset=reset)
        out = {"fill_ms": st["fill_ms"], "trace_ms": st["trace_ms"], "launches": st["launches"],
               "groups": st["groups"], "cells": st["cells"], "trace_steps": st["trace_steps"],
               "move_store_bytes": st["bytes"]}
        out["fill_ns_per_kcell"] = 1e9 * st["fill_ms"] / st["cells"] if st["cells"] else None
        return out

    calls = {
        "GLOBAL": lambda pairs: A.align_batch(pairs, A.NW, A.AlignConfig(params), engine=eng),
        "SEMIGLOBAL": lambda pairs: A.align_ends_batch(pairs, A.SEMIGLOBAL, params, engine=eng),
        "LOCAL": lambda pairs: A.align_ends_batch(pairs, A.LOCAL, params, engine=eng),
    }
    for call in calls.values():   # warm-up: stream, buffers, code objects
        call(shapes["4096 x (500 x 500)"][:8])
    doc = {"scores": list(SCORES), "repeat": a.repeat, "shapes": {}}
    for name, pairs in shapes.items():
        doc["shapes"][name] = {"pairs": len(pairs)}
        for mode, call in calls.items():
            best, runs = timed(lambda: call(pairs), align_stats, a.repeat)
            doc["shapes"][name][mode] = {"best": best, "runs": runs}
            print(name, mode, json.dumps(best), flush=True)

    # k_map_fill next to LOCAL on both strands: the same 2 x 500 x 500 cells per pair, without and with the path
    pairs = shapes["4096 x (500 x 500)"]
    zmws = [(t, [q]) for t, q in pairs]
    mapping.map_batch(zmws[:8], engine=eng)

    def map_stats(reset):
        st = mapping.map_stats(eng, reset=reset)
        return {"device_ms": st["device_ms"], "cells": st["cells"], "launches": st["launches"]}

    best, runs = timed(lambda: mapping.map_batch(zmws, engine=eng), map_stats, a.repeat)
    doc["local_both_strands_500x500"] = {"k_map_fill (no path)": {"best": best, "runs": runs}}
    best, runs = timed(lambda: A.align_ends_batch(pairs, A.LOCAL, params, both_strands=True, engine=eng), align_stats,
                       a.repeat)
    doc["local_both_strands_500x500"]["k_align_fill_ends + trace (path)"] = {"best": best, "runs": runs}
    best, runs = timed(lambda: mapping.map_batch(zmws, engine=eng, transcripts=True), map_stats, a.repeat)
    doc["local_both_strands_500x500"]["map_batch(transcripts=True), wall only"] = {"best_wall_ms": best["wall_ms"]}
    print(json.dumps(doc["local_both_strands_500x500"]), flush=True)

    res_path = os.path.join(os.path.dirname(lib.LIB_PATH), "kernel_resources.json")
    if os.path.exists(res_path):
        res = json.load(open(res_path))
        doc["kernel_resources"] = {k: v for k, v in res.items() if "k_align_" in k and "band" not in k}
        earlier = os.path.join(ROOT, "profiles", "align_batch.json")
        if os.path.exists(earlier):
            old = json.load(open(earlier)).get("kernel_resources", {})
            doc["global_kernels_equal_align_batch_json"] = bool(old) and all(res.get(k) == v for k, v in old.items())
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()

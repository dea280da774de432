#!/usr/bin/env python3
"""Measures split mapping (pbccs_split_map_batch) and the ccs call that recovers missed-adapter reads, and writes
profiles/split_map.json.

Null (CPU, --null-trials N, no GPU): the best plain local-alignment score (3 / -5 / -4 / -4, both strands) of N
uniform-random 4000-base reads against unrelated 2000-base drafts; the default jump penalty is twice the maximum,
rounded up to a multiple of 10.

Kernel: map_probe.py's 4096 reads of 2000 x 2000 (noisy copies of their drafts, half of them reverse complemented)
through pbccs_map_batch and through pbccs_split_map_batch; per call the kernels' device ms from HIP events (profiling
on) and GCUPS over each call's own cell count (2 (I + 1) J and 2 I J per read), best of --repeat.

End to end: bench.py's --stage ccs shape (2 kb, 10 passes, 2000 ZMWs per step, --steps steps in one call, eight
workspace slots) with 0% and with 2% of the subreads fused to their successor across a noisy adapter, each with the
keyword off and on; each timed call in a fresh child process after one warm-up call, the legs interleaved
--e2e-repeat times in alternating order, plus "parent" (another checkout of the project given by --parent-root, its
own package and library, keyword off; skipped without it).  Per leg: ZMWs/s of every repeat, the status counts, the
passes used (n_passes summed), the reads added and the missed adapters recovered.
Not a test and not part of bench.py.  Usage: split_map_probe.py [--out profiles/split_map.json] [--parent-root DIR]"""
import argparse
import json
import os
import pickle
import random
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def measure_null(trials, seed=20261021):
    import numpy as np

    def best_local(draft, read):
        n_j = len(draft)
        ramp = 4 * np.arange(1, n_j + 1, dtype=np.int64)
        prev = np.zeros(n_j + 1, dtype=np.int64)
        best = 0
        for b in read:
            v = np.maximum(0, np.maximum(prev[:-1] + np.where(draft == b, 3, -5), prev[1:] - 4))
            h = np.maximum.accumulate(v + ramp) - ramp   # the Delete chain: H(j) = max(V(j), H(j - 1) - 4)
            prev[1:] = h
            best = max(best, int(h.max()))
        return best
    rng = np.random.default_rng(seed)
    scores = []
    for _ in range(trials):
        d, r = rng.integers(0, 4, 2000), rng.integers(0, 4, 4000)
        scores.append(max(best_local(d, r), best_local((3 - d)[::-1], r)))
    mx = max(scores)
    return {"trials": trials, "read": 4000, "draft": 2000, "seed": seed, "max": mx, "mean": sum(scores) / trials,
            "default_jump_penalty": -(-2 * mx // 10) * 10}


def measure_kernel(repeat):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import pbccs_amd
    from map_probe import kernel_shapes
    from pbccs_amd import lib, mapping
    eng = pbccs_amd.Engine(0)
    eng.set_profiling(True)
    name = "4096 x (2000 x 2000)"
    zmws = kernel_shapes(random.Random(2718))[name]
    mapping.map_to_draft("ACGTACGTAC", ["ACGTACG"], engine=eng)         # warm-up: stream, buffers
    mapping.split_map_to_draft("ACGTACGTAC", ["ACGTACG"], engine=eng)
    doc = {"shape": name, "reads": sum(len(r) for _, r in zmws)}
    for leg, call, stats in (("k_map_fill", mapping.map_batch, mapping.map_stats),
                             ("k_split_fill", mapping.split_map_batch, mapping.split_map_stats)):
        runs = []
        for _ in range(repeat):
            stats(eng, reset=True)
            t0 = time.perf_counter()
            res = call(zmws, engine=eng)
            wall = (time.perf_counter() - t0) * 1e3
            st = stats(eng, reset=True)
            runs.append({"wall_ms": wall, "device_ms": st["device_ms"], "cells": st["cells"], "launches": st["launches"],
                         "gcups_device": st["cells"] / (st["device_ms"] * 1e6), "gcups_wall": st["cells"] / (wall * 1e6)})
        doc[leg] = {"best": min(runs, key=lambda r: r["device_ms"]), "runs": runs}
        if leg == "k_split_fill":
            doc[leg]["one_segment_reads"] = sum(1 for rs in res for r in rs if r and r["n_segments"] == 1)
        print(leg, json.dumps(doc[leg]["best"]), flush=True)
    doc["split_over_map"] = doc["k_split_fill"]["best"]["gcups_device"] / doc["k_map_fill"]["best"]["gcups_device"]
    res_path = os.path.join(os.path.dirname(lib.LIB_PATH), "kernel_resources.json")
    res = json.load(open(res_path)) if os.path.exists(res_path) else {}
    return doc, {k: v for k, v in res.items() if "k_split_" in k}


def leg_child(root, work_path, split, out_path):
    """One timed ccs_batch in this process, with the package of the checkout at `root`."""
    sys.path.insert(0, root)
    import pbccs_amd
    from pbccs_amd import driver
    work, warm = pickle.load(open(work_path, "rb"))
    eng = pbccs_amd.Engine(0)
    eng.set_concurrency(8)
    kw = {"split_long_reads": True} if split else {}
    driver.ccs_batch(warm, engine=eng, **kw)
    if split:
        from pbccs_amd import mapping
        mapping.split_map_stats(eng, reset=True)
    t0 = time.perf_counter()
    res = driver.ccs_batch(work, engine=eng, **kw)
    wall = time.perf_counter() - t0
    statuses = {}
    for r in res:
        statuses[r["status"]] = statuses.get(r["status"], 0) + 1
    out = {"wall_s": wall, "zmws_per_s": len(work) / wall, "statuses": statuses,
           "passes_used": sum(r["n_passes"] for r in res),
           "reads_added": sum(len(r["add_order"]) for r in res),
           "missed_adapters_recovered": sum(r.get("n_missed_adapters", 0) for r in res),
           "split_reads": sum(len(r.get("split_reads", [])) for r in res)}
    if split:
        out["split_map_stats"] = mapping.split_map_stats(eng)
    json.dump(out, open(out_path, "w"))


def fuse(chunks, fraction, seed):
    """Fuses `fraction` of the subreads to their successor (the passes alternate strands) across a noisy adapter."""
    import numpy as np
    from pbccs_amd import synth
    rng = np.random.Generator(np.random.PCG64(seed))
    ad = np.frombuffer(synth.ADAPTER.encode(), dtype=np.uint8)
    fused = 0
    for c in chunks:
        reads, k = [], 0
        while k < len(c["reads"]):
            if k + 1 < len(c["reads"]) and rng.random() < fraction:
                a = synth._mutate(rng, ad, 0.07, 0.04, 0.01).tobytes().decode()
                reads.append({"seq": c["reads"][k]["seq"] + a + c["reads"][k + 1]["seq"]})
                k += 2
                fused += 1
            else:
                reads.append(c["reads"][k])
                k += 1
        c["reads"] = reads
    return fused


def measure_e2e(a, tmp):
    sys.path.insert(0, ROOT)
    from pbccs_amd import synth

    def chunks(n, seed):
        return [{"snr": z["snr"], "reads": [{"seq": r["seq"]} for r in z["reads"]]}
                for z in synth.make_zmws(n, 2000, 10, seed=seed)]
    paths, n_fused = {}, {}
    for pct in (0, 2):
        work = [c for k in range(a.steps) for c in chunks(2000, 1 + k)]
        warm = chunks(2000, 1001)
        n_fused[pct] = fuse(work, pct / 100.0, 7) if pct else 0
        if pct:
            fuse(warm, pct / 100.0, 8)
        paths[pct] = os.path.join(tmp, f"work{pct}.pkl")
        pickle.dump((work, warm), open(paths[pct], "wb"))
        n_work = len(work)
    legs = [(f"{pct}% fused, keyword {'on' if on else 'off'}", ROOT, pct, on) for pct in (0, 2) for on in (False, True)]
    if a.parent_root:
        legs.insert(0, ("parent, 0% fused", os.path.abspath(a.parent_root), 0, False))
    runs = {name: [] for name, _, _, _ in legs}
    for rep in range(a.e2e_repeat):
        for name, root, pct, on in (legs if rep % 2 == 0 else legs[::-1]):   # no leg always runs after the same one
            out_path = os.path.join(tmp, "leg.json")
            subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", root, paths[pct], "1" if on else "0",
                            out_path], check=True, timeout=600)
            runs[name].append(json.load(open(out_path)))
            print(rep, name, round(runs[name][-1]["zmws_per_s"], 1), flush=True)
    doc = {}
    for name, rs in runs.items():
        doc[name] = dict(rs[-1], zmws_per_s=[round(r["zmws_per_s"], 1) for r in rs])
        doc[name].pop("wall_s")
    return {"zmws_per_call": n_work, "shape": "2000 bp, 10 passes, 2000 ZMWs per step",
            "subreads_fused": {f"{k}%": v for k, v in n_fused.items()}, "legs": doc}


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--leg":
        _, _, root, work_path, split, out_path = sys.argv
        return leg_child(root, work_path, split == "1", out_path)
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "split_map.json"))
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--e2e-repeat", type=int, default=2)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--parent-root", default=None)
    ap.add_argument("--null-trials", type=int, default=0, help="measure the null on the CPU (minutes for 200 trials)")
    ap.add_argument("--skip-kernel", action="store_true")
    ap.add_argument("--skip-e2e", action="store_true")
    a = ap.parse_args()
    doc = json.load(open(a.out)) if os.path.exists(a.out) else {}   # a section not measured this time is kept
    if a.null_trials:
        doc["null"] = measure_null(a.null_trials)
        print("null", json.dumps(doc["null"]), flush=True)
    if not a.skip_e2e:   # first: its children must not share the device's memory with this process's engine
        with tempfile.TemporaryDirectory() as tmp:
            doc["end_to_end"] = measure_e2e(a, tmp)
    if not a.skip_kernel:
        doc["kernel"], doc["kernel_resources"] = measure_kernel(a.repeat)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()

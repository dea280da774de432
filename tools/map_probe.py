#!/usr/bin/env python3
"""Measures MapToDraft (pbccs_map_batch) and the capped ccs that keeps every pass, and writes
profiles/map_batch.json.

Kernel: 4096 reads of 2000 x 2000 and 64 reads of 20000 x 20000 (noisy copies of their drafts, half of them reverse
complemented); per shape k_map_fill's device ms from HIP events (profiling on), GCUPS over 2 (I + 1) J cells per read,
and the wall ms of the whole call including marshalling, best of --repeat.

End to end: bench.py's --stage ccs shape (2 kb, 10 passes, 2000 ZMWs per step, --steps steps in one call, eight
workspace slots), each timed call in a fresh child process after one warm-up call, the legs interleaved
--e2e-repeat times in alternating order: "parent" (another checkout of the project given by --parent-root, its own package and library;
skipped without it), this tree uncapped, and this tree with max_poa_coverage 3 / 5 / 7 and map_past_cap.  Per leg:
ZMWs/s of every repeat, the POA and map counters, the Success count, the reads AddRead rejected as POOR_ZSCORE, the
mutations the refine loops tested and applied, and the share of the uncapped run's Success ZMWs whose consensus
the leg reproduces.
Not a test and not part of bench.py.  Usage: map_probe.py [--out profiles/map_batch.json] [--parent-root DIR]"""
import argparse
import hashlib
import json
import os
import pickle
import random
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMP = str.maketrans("ACGT", "TGCA")


def noisy(rng, s, ins=0.07, dele=0.04, sub=0.01):
    out = []
    for c in s:
        if rng.random() < ins:
            out.append(rng.choice("ACGT"))
        u = rng.random()
        if u < dele:
            continue
        out.append(rng.choice("ACGT") if u < dele + sub else c)
    return "".join(out)


def kernel_shapes(rng):
    def shape(n, length, per_draft):
        zmws = []
        for _ in range(n // per_draft):
            d = "".join(rng.choice("ACGT") for _ in range(length))
            reads = [noisy(rng, d)[:length] for _ in range(per_draft)]
            zmws.append((d, [r[::-1].translate(COMP) if k % 2 else r for k, r in enumerate(reads)]))
        return zmws
    return {"4096 x (2000 x 2000)": shape(4096, 2000, 8), "64 x (20000 x 20000)": shape(64, 20000, 4)}


def measure_kernel(repeat):
    sys.path.insert(0, ROOT)
    import pbccs_amd
    from pbccs_amd import lib, mapping
    eng = pbccs_amd.Engine(0)
    eng.set_profiling(True)
    rng = random.Random(2718)
    shapes = kernel_shapes(rng)
    mapping.map_to_draft("ACGTACGTAC", ["ACGTACG"], engine=eng)   # warm-up: stream, buffers
    doc = {}
    for name, zmws in shapes.items():
        runs = []
        for _ in range(repeat):
            mapping.map_stats(eng, reset=True)
            t0 = time.perf_counter()
            res = mapping.map_batch(zmws, engine=eng)
            wall = (time.perf_counter() - t0) * 1e3
            st = mapping.map_stats(eng, reset=True)
            runs.append({"wall_ms": wall, "fill_ms": st["device_ms"], "cells": st["cells"], "launches": st["launches"],
                         "strips": st["strips"], "gcups_fill": st["cells"] / (st["device_ms"] * 1e6),
                         "gcups_wall": st["cells"] / (wall * 1e6)})
        full = sum(1 for (d, _), rs in zip(zmws, res) for r in rs if r and r["tpl"][1] - r["tpl"][0] > 0.9 * len(d))
        doc[name] = {"reads": sum(len(r) for _, r in zmws), "reads_spanning_the_draft": full,
                     "best": min(runs, key=lambda r: r["fill_ms"]), "runs": runs}
        print(name, json.dumps(doc[name]["best"]), flush=True)
    res_path = os.path.join(os.path.dirname(lib.LIB_PATH), "kernel_resources.json")
    res = json.load(open(res_path)) if os.path.exists(res_path) else {}
    return doc, {k: v for k, v in res.items() if "k_map_" in k}


def leg_child(root, work_path, cap, out_path):
    """One timed ccs_batch in this process, with the package of the checkout at `root`."""
    sys.path.insert(0, root)
    import pbccs_amd
    from pbccs_amd import driver, poa
    work, warm = pickle.load(open(work_path, "rb"))
    eng = pbccs_amd.Engine(0)
    eng.set_concurrency(8)
    kw = {} if cap is None else {"max_poa_coverage": cap, "map_past_cap": True}
    driver.ccs_batch(warm, engine=eng, **kw)
    poa.poa_stats(eng, reset=True)
    if cap is not None:
        from pbccs_amd import mapping
        mapping.map_stats(eng, reset=True)
    t0 = time.perf_counter()
    res = driver.ccs_batch(work, engine=eng, **kw)
    wall = time.perf_counter() - t0
    statuses = {}
    for r in res:
        statuses[r["status"]] = statuses.get(r["status"], 0) + 1
    out = {"wall_s": wall, "zmws_per_s": len(work) / wall, "statuses": statuses,
           "reads_added": sum(1 for r in res for a in r["add_read_results"] if a == 0),
           "reads_poor_zscore": sum(1 for r in res for a in r["add_read_results"] if a == 3),
           "reads_not_added": sum(1 for r in res for a in r["add_read_results"] if a < 0),
           "mutations_tested": sum(r["n_tested"] for r in res), "mutations_applied": sum(r["n_applied"] for r in res),
           "poa_stats": poa.poa_stats(eng),
           "consensus_md5": [hashlib.md5(r["consensus"].encode()).hexdigest()[:12] if r["status"] == "Success" else None
                             for r in res]}
    if cap is not None:
        out["map_stats"] = mapping.map_stats(eng)
    json.dump(out, open(out_path, "w"))


def measure_e2e(a, tmp):
    sys.path.insert(0, ROOT)
    from pbccs_amd import synth

    def chunks(n, seed):
        return [{"snr": z["snr"], "reads": [{"seq": r["seq"]} for r in z["reads"]]}
                for z in synth.make_zmws(n, 2000, 10, seed=seed)]
    work = [c for k in range(a.steps) for c in chunks(2000, 1 + k)]
    work_path = os.path.join(tmp, "work.pkl")
    pickle.dump((work, chunks(2000, 1001)), open(work_path, "wb"))
    legs = [("uncapped", ROOT, None)] + [(f"cap {k} + map", ROOT, k) for k in a.caps]
    if a.parent_root:
        legs.insert(0, ("parent uncapped", os.path.abspath(a.parent_root), None))
    runs = {name: [] for name, _, _ in legs}
    for rep in range(a.e2e_repeat):
        for name, root, cap in (legs if rep % 2 == 0 else legs[::-1]):   # no leg always runs after the same one
            out_path = os.path.join(tmp, "leg.json")
            subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", root, work_path,
                            "none" if cap is None else str(cap), out_path], check=True, timeout=600)
            runs[name].append(json.load(open(out_path)))
            print(rep, name, round(runs[name][-1]["zmws_per_s"], 1), flush=True)
    base = runs["uncapped"][0]["consensus_md5"]
    doc = {}
    for name, rs in runs.items():
        last = rs[-1]
        both = [(x, y) for x, y in zip(last["consensus_md5"], base) if y is not None]
        doc[name] = {"zmws_per_s": [round(r["zmws_per_s"], 1) for r in rs], "statuses": last["statuses"],
                     "reads_added": last["reads_added"], "reads_poor_zscore": last["reads_poor_zscore"],
                     "reads_not_added": last["reads_not_added"], "mutations_tested": last["mutations_tested"],
                     "mutations_applied": last["mutations_applied"],
                     "consensus_equal_to_uncapped": sum(1 for x, y in both if x == y) / max(1, len(both)),
                     "poa_stats": last["poa_stats"], "map_stats": last.get("map_stats")}
    return {"zmws_per_call": len(work), "shape": "2000 bp, 10 passes, 2000 ZMWs per step", "legs": doc}


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--leg":
        _, _, root, work_path, cap, out_path = sys.argv
        return leg_child(root, work_path, None if cap == "none" else int(cap), out_path)
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "map_batch.json"))
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--e2e-repeat", type=int, default=3)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--parent-root", default=None)
    ap.add_argument("--caps", type=lambda v: [int(x) for x in v.split(",") if x], default=[3, 5, 7],
                    help="the capped legs, comma separated (empty: only the uncapped legs, e.g. a parent A/B)")
    ap.add_argument("--skip-kernel", action="store_true")
    ap.add_argument("--skip-e2e", action="store_true")
    a = ap.parse_args()
    doc = {"repeat": a.repeat}
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

#!/usr/bin/env python3
"""Measures SparseAlign (pbccs_sparse_align_batch) and writes profiles/sparse_align.json.

Shapes: 4096 pairs of 2000 x 2000 and 64 pairs of 20000 x 20000 at K = 6 (a random target and a copy with 15% errors,
half of the copies reverse complemented and flagged so), ranges asked for.  Per shape, best of --repeat by device
ms: the five kernels' device ms from HIP events (profiling on), the wall ms of the whole Python call including
marshalling, seeds, anchors, and the cells inside the ranges over the len1 (len2 + 1) cells of the full product.

Beside them the POA's cost for the same reads: poa_batch over ZMWs of two reads (target, then the copy), whose
second AddRead fills the copy, both strands, against a graph that holds only the target; fill_ms and device_ms from
poa_stats.  At 20 kb the POA leg runs --poa-long pairs only (its score columns take gigabytes per ZMW) and is
reported per pair.  Not a test and not part of bench.py.  Usage: sparse_probe.py [--out profiles/sparse_align.json]"""
import argparse
import json
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMP = str.maketrans("ACGT", "TGCA")


def noisy(rng, s, ins=0.07, dele=0.05, sub=0.03):
    out = []
    for c in s:
        if rng.random() < ins:
            out.append(rng.choice("ACGT"))
        u = rng.random()
        if u < dele:
            continue
        out.append(rng.choice("ACGT") if u < dele + sub else c)
    return "".join(out)


def shape(rng, n, length):
    pairs, flags = [], []
    for k in range(n):
        t = "".join(rng.choice("ACGT") for _ in range(length))
        q = noisy(rng, t)[:length]
        pairs.append((t, q[::-1].translate(COMP) if k % 2 else q))
        flags.append(k % 2)
    return pairs, flags


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sparse_align.json"))
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--k", type=int, default=6)
    ap.add_argument("--poa-long", type=int, default=4, help="pairs of the 20 kb shape the POA leg runs (0: skip)")
    ap.add_argument("--no-poa", action="store_true", help="skip the POA leg (a kernel-trace run of SparseAlign alone)")
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import pbccs_amd
    from pbccs_amd import lib, poa, sparse
    eng = pbccs_amd.Engine(0)
    eng.set_profiling(True)
    rng = random.Random(1618)
    shapes = {"4096 x (2000 x 2000)": shape(rng, 4096, 2000), "64 x (20000 x 20000)": shape(rng, 64, 20000)}
    sparse.SparseAlign("ACGTACGTACGGT", "ACGTACGTACGGT", a.k, engine=eng)   # warm-up: stream, code objects
    doc = {"k": a.k, "repeat": a.repeat, "shapes": {}}
    for name, (pairs, flags) in shapes.items():
        runs = []
        for _ in range(a.repeat):
            sparse.sparse_align_stats(eng, reset=True)
            t0 = time.perf_counter()
            res = sparse.sparse_align_batch(pairs, a.k, reverse_complement=flags, ranges=True, engine=eng)
            wall = (time.perf_counter() - t0) * 1e3
            st = sparse.sparse_align_stats(eng, reset=True)
            runs.append({"wall_ms": wall, "device_ms": st["device_ms"], "seeds": st["seeds"], "anchors": st["anchors"],
                         "launches": st["launches"], "range_cells": st["range_cells"], "full_cells": st["full_cells"],
                         "cells_in_range_over_full": st["range_cells"] / max(1, st["full_cells"])})
        best = min(runs, key=lambda r: r["device_ms"])
        entry = {"pairs": len(pairs), "best": best, "runs": runs,
                 "seeds_per_query_base": best["seeds"] / max(1, sum(len(q) for _, q in pairs)),
                 "anchors_per_pair": best["anchors"] / len(pairs),
                 "pairs_with_anchors_over_half_the_target":
                     sum(1 for (t, _), r in zip(pairs, res) if r["anchors"] and
                         r["anchors"][-1][0] - r["anchors"][0][0] > len(t) // 2)}
        # the POA's fill of the same reads: ZMWs of (target, copy as given)
        n_poa = len(pairs) if len(pairs[0][0]) <= 4000 else min(len(pairs), a.poa_long)
        if n_poa and not a.no_poa:
            try:
                zmws = [[t, q] for t, q in pairs[:n_poa]]
                poa.poa_batch(zmws[:2], engine=eng)
                best_poa = None
                for _ in range(max(1, min(a.repeat, 3))):
                    poa.poa_stats(eng, reset=True)
                    t0 = time.perf_counter()
                    poa.poa_batch(zmws, engine=eng)
                    wall = (time.perf_counter() - t0) * 1e3
                    ps = poa.poa_stats(eng, reset=True)
                    run = {"pairs": n_poa, "wall_ms": wall, "fill_ms": ps["fill_ms"], "device_ms": ps["device_ms"],
                           "cells": ps["cells"], "alignments": ps["alignments"]}
                    if best_poa is None or run["fill_ms"] < best_poa["fill_ms"]:
                        best_poa = run
                entry["poa_same_reads"] = best_poa
                per_pair_sparse = best["device_ms"] / len(pairs)
                per_pair_fill = best_poa["fill_ms"] / n_poa
                entry["sparse_device_ms_over_poa_fill_ms"] = per_pair_sparse / per_pair_fill if per_pair_fill else None
            except Exception as e:   # the POA leg is context; the SparseAlign figures stand without it
                entry["poa_same_reads"] = {"error": repr(e)}
        doc["shapes"][name] = entry
        print(name, json.dumps({k: v for k, v in entry.items() if k != "runs"}), flush=True)
    res_path = os.path.join(os.path.dirname(lib.LIB_PATH), "kernel_resources.json")
    res = json.load(open(res_path)) if os.path.exists(res_path) else {}
    doc["kernel_resources"] = {k: v for k, v in res.items() if "k_sparse_" in k}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Measures the banded POA fill against the full fill (poa_batch both ways, same engine, same run) and writes
profiles/poa_band.json.

Shapes, as ZMWs of noisy copies of a random template at 15% errors (7% insertions, 5% deletions, 3% substitutions),
every other pass reverse complemented: 2 kb x 10 passes and 20 kb x 6 passes (the two shapes of
profiles/sparse_align.json), and a set near 600 bases x 8 passes.  Per shape and per way, best of --repeat by wall ms:
the wall ms of the Python call, the device ms by phase from HIP events (profiling on) -- the full fill's fill and
trace from poa_stats, the banded way's seeding, ranges, fill and trace from poa_band_stats -- the score bytes the
fills wrote, band cells over full cells, the fallbacks, and the share of ZMWs whose draft, keys, strands and extents
equal the unbanded call's.  At 2 kb also the ccs Success counts through driver.ccs_batch both ways.
Not a test and not part of bench.py.  Usage: poa_band_probe.py [--out profiles/poa_band.json]"""
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


def zmws(rng, n, length, passes, jitter=0):
    out = []
    for _ in range(n):
        ln = length + (rng.randrange(-jitter, jitter + 1) if jitter else 0)
        t = "".join(rng.choice("ACGT") for _ in range(ln))
        reads = [noisy(rng, t) for _ in range(passes)]
        out.append([r[::-1].translate(COMP) if k % 2 else r for k, r in enumerate(reads)])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "poa_band.json"))
    ap.add_argument("--repeat", type=int, default=2)
    ap.add_argument("--n-2kb", type=int, default=128)
    ap.add_argument("--n-20kb", type=int, default=4)
    ap.add_argument("--n-600", type=int, default=512)
    ap.add_argument("--n-ccs", type=int, default=32, help="ZMWs of the 2 kb shape that also go through ccs_batch")
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import pbccs_amd
    from pbccs_amd import driver, lib, poa
    eng = pbccs_amd.Engine(0)
    eng.set_profiling(True)
    rng = random.Random(2718)
    shapes = [("2 kb x 10 passes", zmws(rng, a.n_2kb, 2000, 10), a.repeat),
              ("20 kb x 6 passes", zmws(rng, a.n_20kb, 20000, 6), 1),
              ("600 bases x 8 passes", zmws(rng, a.n_600, 600, 8, jitter=60), a.repeat)]
    warm = zmws(rng, 2, 300, 3)
    poa.poa_batch(warm, engine=eng)
    poa.poa_batch(warm, engine=eng, banded=True)
    doc = {"errors": {"insertions": 0.07, "deletions": 0.05, "substitutions": 0.03}, "shapes": {}}
    for name, zs, repeat in shapes:
        entry = {"zmws": len(zs), "reads": sum(len(z) for z in zs), "read_bases": sum(len(r) for z in zs for r in z)}
        results = {}
        for way, banded in (("unbanded", False), ("banded", True)):
            best = None
            for _ in range(max(1, repeat)):
                poa.poa_stats(eng, reset=True)
                poa.poa_band_stats(eng, reset=True)
                t0 = time.perf_counter()
                res = poa.poa_batch(zs, engine=eng, banded=banded)
                wall = (time.perf_counter() - t0) * 1e3
                ps, bs = poa.poa_stats(eng, reset=True), poa.poa_band_stats(eng, reset=True)
                run = {"wall_ms": wall, "alignments": ps["alignments"], "cells_filled": ps["cells"],
                       "score_bytes": ps["bytes"], "score_bytes_per_zmw": ps["bytes"] / len(zs),
                       "full_fill_ms": ps["fill_ms"], "full_trace_ms": ps["trace_ms"],
                       "host_prog_ms": ps["prog_ms"], "host_thread_ms": ps["thread_ms"], "device_phase_wall_ms": ps["device_ms"]}
                if banded:
                    run.update({"seed_ms": bs["seed_ms"], "ranges_ms": bs["ranges_ms"], "band_fill_ms": bs["fill_ms"],
                                "band_trace_ms": bs["trace_ms"], "banded_alignments": bs["banded_alignments"],
                                "fallbacks": bs["fallbacks"], "band_cells": bs["band_cells"],
                                "full_cells": bs["full_cells"],
                                "band_cells_over_full_cells": bs["band_cells"] / max(1, bs["full_cells"]),
                                "band_score_bytes": bs["score_bytes"], "seeds": bs["seeds"], "anchors": bs["anchors"],
                                "device_ms": bs["seed_ms"] + bs["ranges_ms"] + bs["fill_ms"] + bs["trace_ms"] +
                                             ps["fill_ms"] + ps["trace_ms"]})
                else:
                    run["device_ms"] = ps["fill_ms"] + ps["trace_ms"]
                if best is None or run["wall_ms"] < best["wall_ms"]:
                    best = run
            entry[way] = best
            results[way] = res
        same = sum(1 for u, b in zip(results["unbanded"], results["banded"]) if u == b)
        entry["zmws_equal_to_unbanded"] = same
        entry["share_equal_to_unbanded"] = same / len(zs)
        entry["same_draft"] = sum(1 for u, b in zip(results["unbanded"], results["banded"])
                                  if u["consensus"] == b["consensus"]) / len(zs)
        entry["banded_device_ms_over_unbanded"] = entry["banded"]["device_ms"] / max(1e-9, entry["unbanded"]["device_ms"])
        entry["banded_wall_ms_over_unbanded"] = entry["banded"]["wall_ms"] / max(1e-9, entry["unbanded"]["wall_ms"])
        if name.startswith("2 kb") and a.n_ccs:
            chunks = [{"snr": [10.0, 7.0, 5.0, 11.0], "reads": [{"seq": r} for r in z]} for z in zs[:a.n_ccs]]
            ccs = {}
            for way, banded in (("unbanded", False), ("banded", True)):
                t0 = time.perf_counter()
                got = driver.ccs_batch(chunks, engine=eng, banded_poa=banded)
                ccs[way] = {"wall_ms": (time.perf_counter() - t0) * 1e3,
                            "success": sum(1 for g in got if g["status"] == "Success"),
                            "statuses": {s: sum(1 for g in got if g["status"] == s) for s in sorted({g["status"] for g in got})}}
                ccs[way + "_consensus"] = [g["consensus"] for g in got]
            ccs["same_consensus"] = sum(1 for x, y in zip(ccs.pop("unbanded_consensus"), ccs.pop("banded_consensus")) if x == y)
            ccs["zmws"] = len(chunks)
            entry["ccs_batch"] = ccs
        doc["shapes"][name] = entry
        print(name, json.dumps(entry), flush=True)
    res_path = os.path.join(os.path.dirname(lib.LIB_PATH), "kernel_resources.json")
    res = json.load(open(res_path)) if os.path.exists(res_path) else {}
    doc["kernel_resources"] = {k: v for k, v in res.items()
                               if any(s in k for s in ("k_poa_ranges", "k_poa_fill_band", "k_poa_trace_band"))}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()

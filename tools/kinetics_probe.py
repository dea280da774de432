#!/usr/bin/env python3
"""Measures what consensus kinetics (driver.ccs_batch(kinetics=True)) cost, and writes
profiles/kinetics.json.

Shape: bench.py's --stage ccs shape -- 2 kb inserts, 10 passes, --zmws ZMWs (4000) in one ccs_batch call, eight
workspace slots; every read carries random ip / pw tracks as uint16 arrays.  Legs: this tree without kinetics, this
tree with kinetics, and the parent commit without kinetics (another checkout of the project given by --parent-root,
its own package and library; skipped without it), which should sit inside this tree's own spread for
kinetics=False since that path is unchanged.  Each timed call runs in a fresh child process after one warm-up call,
under its own timeout; the legs are interleaved --repeat times in alternating order.

One more child, with profiling on, runs the kinetics step alone on the consensuses of a ccs_batch call and reports
the device ms of k_map_fill, the align fill and trace, k_kin_columns and k_kin_reduce from map_stats / align_stats
/ kinetics_stats; a last one runs the same step with band=True on --band-zmws ZMWs and records what the certified
band did (align_band_stats' fallback reasons).
Not a test and not part of bench.py.  Usage: kinetics_probe.py [--out profiles/kinetics.json] [--parent-root DIR]"""
import argparse
import json
import os
import pickle
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def make_work(n, seed):
    import numpy as np
    sys.path.insert(0, ROOT)
    from pbccs_amd import synth
    rng = np.random.Generator(np.random.PCG64(seed + 99))
    out = []
    for z in synth.make_zmws(n, 2000, 10, seed=seed):
        reads = []
        for r in z["reads"]:
            m = len(r["seq"])
            reads.append({"seq": r["seq"], "ip": rng.integers(0, 400, m).astype(np.uint16),
                          "pw": rng.integers(0, 60, m).astype(np.uint16)})
        out.append({"snr": z["snr"], "reads": reads})
    return out


def leg_child(root, work_path, mode, out_path):
    """One timed ccs_batch in this process, with the package of the checkout at `root`."""
    sys.path.insert(0, root)
    import pbccs_amd
    from pbccs_amd import driver
    work, warm = pickle.load(open(work_path, "rb"))
    eng = pbccs_amd.Engine(0)
    eng.set_concurrency(8)
    kw = {"kinetics": True} if mode == "kinetics" else {}
    driver.ccs_batch(warm, engine=eng, **kw)
    t0 = time.perf_counter()
    res = driver.ccs_batch(work, engine=eng, **kw)
    wall = time.perf_counter() - t0
    statuses = {}
    for r in res:
        statuses[r["status"]] = statuses.get(r["status"], 0) + 1
    out = {"wall_s": wall, "zmws_per_s": len(work) / wall, "statuses": statuses}
    if mode == "kinetics":
        from pbccs_amd import kinetics
        out["kinetics_stats"] = kinetics.kinetics_stats(eng)
        out["passes"] = [sum(r.get("fn", 0) for r in res), sum(r.get("rn", 0) for r in res)]
    json.dump(out, open(out_path, "w"))


def stage_child(work_path, band_zmws, out_path):
    """The kinetics step alone with profiling on, then with the certified band on a sample."""
    sys.path.insert(0, ROOT)
    import pbccs_amd
    from pbccs_amd import align, driver, kinetics, mapping
    work, warm = pickle.load(open(work_path, "rb"))
    eng = pbccs_amd.Engine(0)
    eng.set_concurrency(8)
    res = driver.ccs_batch(work, engine=eng)
    zmws = [(r["consensus"], [x for x, a in zip(c["reads"], r["add_read_results"]) if a == 0])
            for c, r in zip(work, res) if r["status_code"] in (0, 6) and r["consensus"]]
    kinetics.kinetics_batch(zmws[:64], engine=eng)   # warm-up: streams, buffers
    eng.set_profiling(True)
    for f in (mapping.map_stats, align.align_stats, align.align_band_stats, kinetics.kinetics_stats):
        f(eng, reset=True)
    t0 = time.perf_counter()
    kinetics.kinetics_batch(zmws, engine=eng)
    wall = time.perf_counter() - t0
    out = {"zmws": len(zmws), "reads": sum(len(r) for _, r in zmws), "wall_s": wall,
           "map_stats": mapping.map_stats(eng, reset=True), "align_stats": align.align_stats(eng, reset=True),
           "kinetics_stats": kinetics.kinetics_stats(eng, reset=True)}
    sample = zmws[:band_zmws]
    align.align_band_stats(eng, reset=True)
    t0 = time.perf_counter()
    banded = kinetics.kinetics_batch(sample, band=True, engine=eng)
    out["banded"] = {"zmws": len(sample), "wall_s": time.perf_counter() - t0,
                     "align_band_stats": align.align_band_stats(eng, reset=True),
                     "align_stats": align.align_stats(eng, reset=True),
                     "kinetics_stats": kinetics.kinetics_stats(eng, reset=True)}
    t0 = time.perf_counter()
    plain = kinetics.kinetics_batch(sample, engine=eng)
    out["banded"]["unbanded_wall_s"] = time.perf_counter() - t0
    out["banded"]["equal_to_unbanded"] = banded == plain
    json.dump(out, open(out_path, "w"))


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--leg":
        _, _, root, work_path, mode, out_path = sys.argv
        return leg_child(root, work_path, mode, out_path)
    if len(sys.argv) > 1 and sys.argv[1] == "--stage":
        _, _, work_path, band_zmws, out_path = sys.argv
        return stage_child(work_path, int(band_zmws), out_path)
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kinetics.json"))
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--zmws", type=int, default=4000)
    ap.add_argument("--band-zmws", type=int, default=400)
    ap.add_argument("--leg-timeout", type=int, default=300)
    ap.add_argument("--parent-root", default=None)
    a = ap.parse_args()
    doc = {"shape": f"2000 bp, 10 passes, {a.zmws} ZMWs in one ccs_batch call", "repeat": a.repeat}
    with tempfile.TemporaryDirectory() as tmp:
        work_path = os.path.join(tmp, "work.pkl")
        pickle.dump((make_work(a.zmws, 1), make_work(200, 1001)), open(work_path, "wb"))
        legs = [("without kinetics", ROOT, "none"), ("with kinetics", ROOT, "kinetics")]
        if a.parent_root:
            legs.append(("parent without kinetics", os.path.abspath(a.parent_root), "none"))
        runs = {name: [] for name, _, _ in legs}
        out_path = os.path.join(tmp, "leg.json")
        for rep in range(a.repeat):
            for name, root, mode in (legs if rep % 2 == 0 else legs[::-1]):   # no leg always runs after the same one
                subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", root, work_path, mode, out_path],
                               check=True, timeout=a.leg_timeout)
                runs[name].append(json.load(open(out_path)))
                print(rep, name, round(runs[name][-1]["zmws_per_s"], 1), flush=True)
        doc["legs"] = {name: {"zmws_per_s": [round(r["zmws_per_s"], 1) for r in rs],
                              "wall_s": [round(r["wall_s"], 3) for r in rs], "statuses": rs[-1]["statuses"],
                              "kinetics_stats": rs[-1].get("kinetics_stats"), "passes": rs[-1].get("passes")}
                       for name, rs in runs.items()}
        subprocess.run([sys.executable, os.path.abspath(__file__), "--stage", work_path, str(a.band_zmws), out_path],
                       check=True, timeout=a.leg_timeout)
        doc["kinetics_step_profiled"] = json.load(open(out_path))
        print("stage", json.dumps(doc["kinetics_step_profiled"]["kinetics_stats"]), flush=True)
    res_path = os.path.join(ROOT, "pbccs_amd", "_lib", "kernel_resources.json")
    if os.path.exists(res_path):
        doc["kernel_resources"] = {k: v for k, v in json.load(open(res_path)).items() if "k_kin_" in k}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()

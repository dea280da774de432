#!/usr/bin/env python3
"""Measures what the subread pileup (driver.ccs_batch(pileup=True)) costs, and writes
profiles/pileup.json.

Shape: the kinetics section's -- 2 kb inserts, 10 passes, --zmws ZMWs (4000) in one ccs_batch call, eight workspace
slots; every read carries random ip / pw tracks as uint16 arrays.  Legs: this tree without a keyword, with
pileup=True, with kinetics=True, with both, the two pileup legs again with pileup={"arrays": True} (numpy arrays
instead of nested lists in the records), and the parent commit without a keyword (another checkout of the
project given by --parent-root, its own package and library; skipped without it), which should sit inside this
tree's own spread since that path is unchanged.  Each timed call runs in a fresh child process after one warm-up
call, under its own timeout; the legs are interleaved --repeat times in alternating order.

One more child, with profiling on, runs the pileup step alone on the consensuses of a ccs_batch call and reports the
device ms of k_map_fill, the align fill and trace, and k_pile_columns / k_pile_reduce from map_stats / align_stats /
pileup_stats; then the gapped rows of --msa-zmws ZMWs for k_pile_scan and k_pile_rows.
Not a test and not part of bench.py.  Usage: pileup_probe.py [--out profiles/pileup.json] [--parent-root DIR]"""
import argparse
import json
import os
import pickle
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = {"none": {}, "pileup": {"pileup": True}, "kinetics": {"kinetics": True},
         "both": {"kinetics": True, "pileup": True}, "pileup_arrays": {"pileup": {"arrays": True}},
         "both_arrays": {"kinetics": True, "pileup": {"arrays": True}}}


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
    kw = MODES[mode]
    driver.ccs_batch(warm, engine=eng, **kw)
    t0 = time.perf_counter()
    res = driver.ccs_batch(work, engine=eng, **kw)
    wall = time.perf_counter() - t0
    statuses = {}
    for r in res:
        statuses[r["status"]] = statuses.get(r["status"], 0) + 1
    out = {"wall_s": wall, "zmws_per_s": len(work) / wall, "statuses": statuses}
    if "pileup" in kw:
        from pbccs_amd import pileup
        out["pileup_stats"] = pileup.pileup_stats(eng)
        ecs = [r["ec"] for r in res if "ec" in r]
        out["mean_ec"] = sum(ecs) / max(1, len(ecs))
    json.dump(out, open(out_path, "w"))


def stage_child(work_path, msa_zmws, out_path):
    """The pileup step alone with profiling on, then the gapped rows of a sample."""
    sys.path.insert(0, ROOT)
    import pbccs_amd
    from pbccs_amd import align, driver, mapping, pileup
    work, warm = pickle.load(open(work_path, "rb"))
    eng = pbccs_amd.Engine(0)
    eng.set_concurrency(8)
    res = driver.ccs_batch(work, engine=eng)
    zmws = [(r["consensus"], [{"seq": x["seq"]} for x, a in zip(c["reads"], r["add_read_results"]) if a == 0])
            for c, r in zip(work, res) if r["status_code"] in (0, 6) and r["consensus"]]
    pileup.pileup_batch(zmws[:64], msa=True, engine=eng)   # warm-up: streams, buffers
    eng.set_profiling(True)
    for f in (mapping.map_stats, align.align_stats, pileup.pileup_stats):
        f(eng, reset=True)
    t0 = time.perf_counter()
    pileup.pileup_batch(zmws, engine=eng)
    wall = time.perf_counter() - t0
    out = {"zmws": len(zmws), "reads": sum(len(r) for _, r in zmws), "wall_s": wall,
           "map_stats": mapping.map_stats(eng, reset=True), "align_stats": align.align_stats(eng, reset=True),
           "pileup_stats": pileup.pileup_stats(eng, reset=True)}
    sample = zmws[:msa_zmws]
    t0 = time.perf_counter()
    rows = pileup.pileup_batch(sample, msa=True, engine=eng)
    out["msa"] = {"zmws": len(sample), "wall_s": time.perf_counter() - t0,
                  "mean_width": sum(g["width"] for g in rows) / max(1, len(rows)),
                  "pileup_stats": pileup.pileup_stats(eng, reset=True)}
    json.dump(out, open(out_path, "w"))


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--leg":
        _, _, root, work_path, mode, out_path = sys.argv
        return leg_child(root, work_path, mode, out_path)
    if len(sys.argv) > 1 and sys.argv[1] == "--stage":
        _, _, work_path, msa_zmws, out_path = sys.argv
        return stage_child(work_path, int(msa_zmws), out_path)
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pileup.json"))
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--zmws", type=int, default=4000)
    ap.add_argument("--msa-zmws", type=int, default=400)
    ap.add_argument("--leg-timeout", type=int, default=300)
    ap.add_argument("--parent-root", default=None)
    a = ap.parse_args()
    doc = {"shape": f"2000 bp, 10 passes, {a.zmws} ZMWs in one ccs_batch call", "repeat": a.repeat}
    with tempfile.TemporaryDirectory() as tmp:
        work_path = os.path.join(tmp, "work.pkl")
        pickle.dump((make_work(a.zmws, 1), make_work(200, 1001)), open(work_path, "wb"))
        legs = [("without keyword", ROOT, "none"), ("pileup", ROOT, "pileup"), ("kinetics", ROOT, "kinetics"),
                ("kinetics and pileup", ROOT, "both"), ("pileup as arrays", ROOT, "pileup_arrays"),
                ("kinetics and pileup as arrays", ROOT, "both_arrays")]
        if a.parent_root:
            legs.append(("parent without keyword", os.path.abspath(a.parent_root), "none"))
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
                              "pileup_stats": rs[-1].get("pileup_stats"), "mean_ec": rs[-1].get("mean_ec")}
                       for name, rs in runs.items()}
        subprocess.run([sys.executable, os.path.abspath(__file__), "--stage", work_path, str(a.msa_zmws), out_path],
                       check=True, timeout=a.leg_timeout)
        doc["pileup_step_profiled"] = json.load(open(out_path))
        print("stage", json.dumps(doc["pileup_step_profiled"]["pileup_stats"]), flush=True)
    res_path = os.path.join(ROOT, "pbccs_amd", "_lib", "kernel_resources.json")
    if os.path.exists(res_path):
        doc["kernel_resources"] = {k: v for k, v in json.load(open(res_path)).items() if "k_pile_" in k}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()

"""Barcode demultiplexing probe.

  python tools/demux_probe.py null [--reads 2000] [--out FILE]
      the min_quality measurement, on the CPU with the restatement alone (tests/demux_restatement.py): 96 random
      16-mers, W = 48, the default scores; (a) the largest quality over barcode-free random 400-base reads, (b) the
      smallest quality over planted reads mutated at CCS-like rates (0.2% insertion, 0.2% deletion, 0.1%
      substitution).  The default is the midpoint, rounded down.
  python tools/demux_probe.py device [--reads 4000] [--barcodes 384] [--rounds 5] [--out FILE]
      on the GPU, alternating after a warm-up: demux_batch (k_demux_score and the two small kernels) at reads x
      barcodes x W = 48, and the same score matrix for a 200-read sample through align_ends_batch(SEMIGLOBAL), the
      alternative it replaces, scaled per pair.
  python tools/demux_probe.py ccs [--reads 4000] [--barcodes 384] [--rounds 3] [--out FILE]
      on the GPU, alternating after a warm-up: driver.ccs_batch on the ccs benchmark stage's shape (2 kb, 10 passes,
      --reads ZMWs per call) without and with barcodes= of 384 16-mers.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def rand_seq(rng, n):
    return "".join("ACGT"[k] for k in rng.integers(0, 4, n))


def mutate(rng, seq, p_ins=0.002, p_del=0.002, p_sub=0.001):
    out = []
    for c in seq:
        u = rng.random()
        if u < p_del:
            continue
        if u < p_del + p_sub:
            c = "ACGT"[("ACGT".index(c) + int(rng.integers(1, 4))) % 4]
        out.append(c)
        if rng.random() < p_ins:
            out.append("ACGT"[int(rng.integers(0, 4))])
    return "".join(out)


def measure_null(n_reads, seed=20261021):
    import demux_restatement as R
    rng = np.random.default_rng(seed)
    barcodes = [rand_seq(rng, 16) for _ in range(96)]
    lens = [16] * 96
    W = 48
    free = [rand_seq(rng, 400) for _ in range(n_reads)]
    pairs = [(int(rng.integers(0, 96)), int(rng.integers(0, 96))) for _ in range(n_reads)]
    planted = [mutate(rng, barcodes[i] + rand_seq(rng, 400) + R.revcomp(barcodes[j])) for i, j in pairs]
    out = {}
    for name, reads in (("free", free), ("planted", planted)):
        S = R.scores_np(reads, barcodes, W)
        out[name] = [R.call(S[k, 0].tolist(), S[k, 1].tolist(), lens, R.DEFAULT_PARAMS[0]) for k in range(len(reads))]
    a = max(c["quality"] for c in out["free"])
    b = min(c["quality"] for c in out["planted"])
    right = sum((c["lead"], c["trail"]) == p for c, p in zip(out["planted"], pairs))
    return {"barcodes": 96, "barcode_length": 16, "window": W, "params": list(R.DEFAULT_PARAMS), "seed": seed,
            "free_reads": n_reads, "planted_reads": n_reads, "free_max_quality": a, "planted_min_quality": b,
            "planted_pairs_right": right, "min_quality_default": (a + b) // 2,
            "free_quality_histogram": np.bincount([c["quality"] for c in out["free"]], minlength=101).tolist(),
            "planted_quality_histogram": np.bincount([c["quality"] for c in out["planted"]], minlength=101).tolist()}


def measure_device(n_reads, n_barcodes, rounds, seed=7):
    import pbccs_amd
    from pbccs_amd import align, demux
    rng = np.random.default_rng(seed)
    barcodes = demux.BarcodeSet([rand_seq(rng, 16) for _ in range(n_barcodes)])
    reads = [rand_seq(rng, 2000) for _ in range(n_reads)]
    eng = pbccs_amd.Engine(0)
    eng.set_profiling(True)
    W = 48
    sample = reads[:200]
    pairs = []
    for r in sample:
        for b in barcodes.seqs:
            pairs.append((r[:W], b))
            pairs.append((r[-W:], align.reverse_complement(b)))
    params = demux.default_params()

    def run_demux():
        demux.demux_stats(eng, reset=True)
        t = time.perf_counter()
        demux.demux_batch(reads, barcodes, window=W, engine=eng)
        wall = time.perf_counter() - t
        s = demux.demux_stats(eng, reset=True)
        return {"wall_s": wall, "device_ms": s["device_ms"], "cells": s["cells"],
                "gcups": s["cells"] / max(1e-9, s["device_ms"]) / 1e6}

    def run_align():
        t = time.perf_counter()
        align.align_ends_batch(pairs, align.SEMIGLOBAL, params, engine=eng)
        return {"wall_s": time.perf_counter() - t, "pairs": len(pairs)}

    run_demux(), run_align()   # warm-up
    d, a = [], []
    for _ in range(rounds):
        d.append(run_demux())
        a.append(run_align())
    med = lambda xs: float(np.median(xs))
    per_pair_demux = med([x["wall_s"] for x in d]) / (2 * n_reads * n_barcodes)
    per_pair_align = med([x["wall_s"] for x in a]) / len(pairs)
    return {"reads": n_reads, "barcodes": n_barcodes, "window": W, "rounds": rounds, "demux": d, "align_ends": a,
            "demux_device_ms_median": med([x["device_ms"] for x in d]),
            "demux_gcups_median": med([x["gcups"] for x in d]),
            "demux_wall_s_median": med([x["wall_s"] for x in d]),
            "align_ends_wall_s_median_200_reads": med([x["wall_s"] for x in a]),
            "align_ends_wall_s_scaled_to_call": per_pair_align * 2 * n_reads * n_barcodes,
            "wall_per_pair_ratio_align_over_demux": per_pair_align / per_pair_demux}


def measure_ccs(n_zmws, n_barcodes, rounds, seed=11):
    import pbccs_amd
    from pbccs_amd import demux, driver, synth
    from pbccs_amd.polish import ConsensusSettings
    rng = np.random.default_rng(seed)
    barcodes = demux.BarcodeSet([rand_seq(rng, 16) for _ in range(n_barcodes)])
    work = [{"snr": z["snr"], "reads": [{"seq": r["seq"]} for r in z["reads"]]}
            for z in synth.make_zmws(n_zmws, 2000, 10, seed=seed)]
    eng = pbccs_amd.Engine(0)
    settings = ConsensusSettings()

    def run(bc):
        t = time.perf_counter()
        res = driver.ccs_batch(work, settings, eng, barcodes=bc)
        wall = time.perf_counter() - t
        return {"wall_s": wall, "zmws_per_s": n_zmws / wall, "success": sum(r["status"] == "Success" for r in res),
                "with_barcode_entry": sum("barcode" in r for r in res)}

    run(None), run(barcodes)   # warm-up
    off, on = [], []
    for _ in range(rounds):
        off.append(run(None))
        on.append(run(barcodes))
    med = lambda xs: float(np.median(xs))
    a, b = med([x["zmws_per_s"] for x in off]), med([x["zmws_per_s"] for x in on])
    return {"zmws": n_zmws, "length": 2000, "passes": 10, "barcodes": n_barcodes, "rounds": rounds,
            "without_barcodes": off, "with_barcodes": on, "zmws_per_s_without_median": a,
            "zmws_per_s_with_median": b, "with_over_without": b / a}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("null", "device", "ccs"))
    ap.add_argument("--reads", type=int, default=None)
    ap.add_argument("--barcodes", type=int, default=384)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.mode == "null":
        res = measure_null(a.reads or 2000)
    elif a.mode == "ccs":
        res = measure_ccs(a.reads or 4000, a.barcodes, min(a.rounds, 3))
    else:
        res = measure_device(a.reads or 4000, a.barcodes, a.rounds)
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()

"""Shared by tests/test_hostile_inputs_cpu.py and tests/test_hostile_inputs_gpu.py: ZMWs on low-complexity templates,
reads no i.i.d. generator draws (indel bursts, junk, wrong strand, duplicated, truncated) and ZMWs whose refine
deactivates a read AddRead took.  Everything here runs on the CPU with numpy and oracle/ alone.

    python -m tests.hostile_inputs heights        # tallest columns and AddRead results of every set
    python -m tests.hostile_inputs search [N]     # the seeds of DEACTIVATION_SEEDS below
    python -m tests.hostile_inputs g1             # the refill gaps tests/test_hostile_inputs_cpu.py asserts
"""
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import oracle as O  # noqa: E402
from pbccs_amd import synth  # noqa: E402

SNR = [10.0, 7.0, 5.0, 11.0]
NAN = float("nan")
READ_ERRORS = (0.07, 0.04, 0.01)
BURSTS = (5, 10, 20, 40, 80)


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def _arr(s):
    return np.frombuffer(s.encode(), dtype=np.uint8)


def _str(a):
    return a.tobytes().decode()


def random_bases(rng, n, alphabet="ACGT"):
    return "".join(alphabet[int(x)] for x in rng.integers(0, len(alphabet), size=n))


def revcomp(s):
    return _str(synth.COMP[_arr(s)[::-1]])


def noisy_pass(rng, truth, errors=READ_ERRORS):
    """One forward pass of truth (a str) at synth.make_zmw's read error rates."""
    return _str(synth._mutate(rng, _arr(truth), *errors))


def zmw_of_truth(rng, truth, passes=5, snr=SNR, read_errors=READ_ERRORS):
    """synth.make_zmw with a given truth: the draft is the truth at 0.5 / 0.5 / 0.2 % errors, `passes` reads at
    read_errors, odd passes reverse-complemented, every read over the whole draft."""
    t = _arr(truth)
    draft = synth._mutate(rng, t, 0.005, 0.005, 0.002)
    reads = []
    for k in range(passes):
        r = synth._mutate(rng, t, *read_errors)
        if k % 2:
            r = synth.COMP[r[::-1]]
        reads.append({"seq": _str(r), "strand": k % 2, "ts": 0, "te": int(draft.shape[0])})
    return {"truth": truth, "draft": _str(draft), "snr": list(snr), "reads": reads}


def _run_length(rng, n=30, lo=1, hi=11):
    return "".join("ACGT"[int(b)] * int(k) for b, k in zip(rng.integers(0, 4, size=n), rng.integers(lo, hi + 1, size=n)))


# name -> (seed, truth builder).  The seeds are fixed; tests/test_hostile_inputs_cpu.py asserts what the GPU tests
# rely on (every read adds, the refines converge, the band heights named there).
_LOW_COMPLEXITY = [
    ("A120", 1211, lambda g: "A" * 120),
    ("G120", 1202, lambda g: "G" * 120),
    ("A400", 1203, lambda g: "A" * 400),
    ("AC60", 1204, lambda g: "AC" * 60),
    ("CAG40", 1205, lambda g: "CAG" * 40),
    ("CT300", 1206, lambda g: "CT" * 300),
    ("AT150", 1207, lambda g: random_bases(g, 150, "AT")),
    ("runlength", 1208, lambda g: _run_length(g)),
    ("flank_T40", 1209, lambda g: random_bases(g, 40) + "T" * 40 + random_bases(g, 40)),
    ("flank_GA30", 1210, lambda g: random_bases(g, 40) + "GA" * 30 + random_bases(g, 40)),
]
LOW_COMPLEXITY_NAMES = [n for n, _, _ in _LOW_COMPLEXITY]
_cache = {}


def low_complexity_zmws():
    """[(name, zmw)] in LOW_COMPLEXITY_NAMES order; 5 passes each.  Built once per process: treat as read-only."""
    if "low" not in _cache:
        out = []
        for name, seed, build in _LOW_COMPLEXITY:
            g = _rng(seed)
            out.append((name, zmw_of_truth(g, build(g))))
        _cache["low"] = out
    return _cache["low"]


def hostile_reads(zmw, rng):
    """[(name, read)]: reads of zmw's truth that no i.i.d. error model draws, all declared forward over the whole
    draft.  `b` is a fresh noisy pass of the truth for every read."""
    truth, L = zmw["truth"], len(zmw["truth"])
    te = len(zmw["draft"])
    b = lambda: noisy_pass(rng, truth)   # noqa: E731
    out = []

    def add(name, seq):
        out.append((name, {"seq": seq, "strand": 0, "ts": 0, "te": te}))

    def at(s):   # a position in the read's middle half
        return int(rng.integers(len(s) // 4, 3 * len(s) // 4))

    for n in BURSTS:
        s = b()
        q = at(s)
        add(f"ins_random_{n}", s[:q] + random_bases(rng, n) + s[q:])
    for n in BURSTS:
        s = b()
        q = at(s)
        add(f"ins_homopolymer_{n}", s[:q] + "ACGT"[int(rng.integers(0, 4))] * n + s[q:])
    for n in BURSTS:
        s = b()
        q = int(rng.integers(len(s) // 4, max(len(s) // 4 + 1, 3 * len(s) // 4 - n)))
        add(f"del_{n}", s[:q] + s[q + n:])
    s = b()
    add("half_junk", s[:len(s) // 2] + random_bases(rng, len(s) - len(s) // 2))
    add("junk_head_30", random_bases(rng, 30) + b())
    add("junk_tail_30", b() + random_bases(rng, 30))
    add("cut_head_40", b()[40:])
    add("cut_tail_40", b()[:-40])
    add("wrong_strand", revcomp(b()))
    for p in (15, 10, 5):
        add(f"errors_{p}pct", noisy_pass(rng, truth, (p / 100.0 * 7 / 12, p / 100.0 * 4 / 12, p / 100.0 / 12)))
    add("junk_L", random_bases(rng, L))
    add("junk_2L", random_bases(rng, 2 * L))
    s = b()
    add("duplicate", s + s)
    add("one_base", b()[:1])
    for n in range(60, L + 1, 20):
        s = b()
        q = len(s) // 2
        add(f"ins_mid_{n}", s[:q] + random_bases(rng, n) + s[q:])
    return out


HOSTILE_ZMW_SEEDS = {150: 1501, 300: 3001}   # synth.make_zmws(1, L, 5, seed); the hostile reads draw from seed + 1


def hostile_zmw(L):
    """The random L bp ZMW (5 passes) with its hostile reads: {"zmw", "names", "reads"}; reads = the ZMW's own five
    followed by every hostile read, names aligned with reads.  Built once per process: treat as read-only."""
    key = ("hostile", L)
    if key not in _cache:
        z = synth.make_zmws(1, L, 5, seed=HOSTILE_ZMW_SEEDS[L])[0]
        hr = hostile_reads(z, _rng(HOSTILE_ZMW_SEEDS[L] + 1))
        names = [f"pass_{k}" for k in range(len(z["reads"]))] + [n for n, _ in hr]
        _cache[key] = {"zmw": z, "names": names, "reads": list(z["reads"]) + [r for _, r in hr]}
    return _cache[key]


def add_reads(tpl, reads, threshold, snr=SNR):
    """A CPU scorer on tpl with `reads` added at `threshold`: (scorer, AddRead results)."""
    s = O.Scorer(tpl, snr)
    return s, [s.add_read(r["seq"], r["strand"], r["ts"], r["te"], threshold) for r in reads]


def tallest(s, r):
    """The tallest column (alpha or beta) of read r's band in CPU scorer s."""
    st = s.band_stats(r)
    return max(st[2], st[3])


# ---------------------------------------------------------------- a read lost during the refine
DEACTIVATION_INSERTS = tuple(range(60, 301, 20))   # 13 reads per ZMW


def deactivation_zmw(L, seed):
    """synth.make_zmws(1, L, 4, seed)[0] plus 13 reads noisy_truth[:q] + random(n) + noisy_truth[q:], n = 60 .. 300:
    {"zmw", "names", "reads"}."""
    z = synth.make_zmws(1, L, 4, seed=seed)[0]
    g = _rng(100000 + seed)
    reads, names = list(z["reads"]), [f"pass_{k}" for k in range(4)]
    for n in DEACTIVATION_INSERTS:
        s = noisy_pass(g, z["truth"])
        q = int(g.integers(len(s) // 4, 3 * len(s) // 4))
        reads.append({"seq": s[:q] + random_bases(g, n) + s[q:], "strand": 0, "ts": 0, "te": len(z["draft"])})
        names.append(f"ins_{n}")
    return {"zmw": z, "names": names, "reads": reads}


def deactivated_reads(L, seed):
    """Names of the reads AddRead (threshold NaN) took and the CPU restatement's default refine left inactive."""
    d = deactivation_zmw(L, seed)
    s, res = add_reads(d["zmw"]["draft"], d["reads"], NAN, d["zmw"]["snr"])
    s.refine()
    return [d["names"][k] for k in range(len(res)) if res[k] == 0 and not s.read_info(k)["active"]]


def find_deactivation(max_seeds, want=3):
    """The first `want` (L, seed, names) over seeds 0 .. max_seeds - 1 and L in {150, 300} with a deactivated read."""
    out = []
    for seed in range(max_seeds):
        for L in (150, 300):
            names = deactivated_reads(L, seed)
            if names:
                out.append((L, seed, names))
                if len(out) >= want:
                    return out
    return out


# python -m tests.hostile_inputs search 69   (the CPU restatement alone, about three minutes) prints
#   L 150 seed 22 deactivated ['ins_220']
#   L 150 seed 23 deactivated ['ins_220']
#   L 150 seed 24 deactivated ['ins_220']
#   L 300 seed 60 deactivated ['ins_220']
#   L 300 seed 68 deactivated ['ins_220']
# In each, ins_60 .. ins_220 add as SUCCESS (tallest columns 122 .. 294 rows at L = 150, 158 .. 334 at L = 300),
# ins_240 .. ins_300 as ALPHABETAMISMATCH, and the refine (27 to 95 mutations applied: the 13 burst reads outvote
# the four passes) drops ins_220.  Seed 60 is left out for its refine's length (19555 mutations tested).
DEACTIVATION_SEEDS = [(150, 22, ("ins_220",)), (150, 23, ("ins_220",)), (300, 68, ("ins_220",))]


# ---------------------------------------------------------------- Quiver on low-complexity templates
_QUIVER_LOW = [
    ("A100", 2101, lambda g: "A" * 100),
    ("AC50", 2102, lambda g: "AC" * 50),
    ("CAG34", 2103, lambda g: "CAG" * 34),
    ("runlength", 2104, lambda g: _run_length(g, n=20, hi=9)),
    ("flank_T40", 2105, lambda g: random_bases(g, 30) + "T" * 40 + random_bases(g, 30)),
]


def quiver_low_complexity_zmws():
    """[(name, {"tpl", "reads"})] built as synth.make_quiver_zmws builds its ZMWs (its read error rates, five feature
    tracks per read drawn from seed + 17), on low-complexity truths; 5 passes."""
    if "quiver" not in _cache:
        out = []
        for name, seed, build in _QUIVER_LOW:
            g, f = _rng(seed), _rng(seed + 17)
            z = zmw_of_truth(g, build(g), read_errors=synth.QUIVER_READ_ERRORS)
            reads = []
            for r in z["reads"]:
                m = len(r["seq"])
                feats = {"ins": f.integers(0, 25, m).astype(np.float32), "subs": f.integers(0, 25, m).astype(np.float32),
                         "del": f.integers(0, 25, m).astype(np.float32),
                         "del_tag": np.frombuffer(b"ACGTN", dtype=np.uint8)[f.integers(0, 5, m)].copy(),
                         "merge": f.integers(0, 25, m).astype(np.float32)}
                reads.append(dict(r, features=feats))
            out.append((name, {"tpl": z["draft"], "reads": reads}))
        _cache["quiver"] = out
    return _cache["quiver"]


# ---------------------------------------------------------------- the restatement against itself
G1_CASES = ("A120", "AC60", "runlength", "flank_T40")


def g1_gaps(name):
    """arrow_multibase_common.g1_measure on one low-complexity ZMW: the largest |scores - refill| per mutation class."""
    from tests import arrow_multibase_common as C
    z = dict(low_complexity_zmws())[name]
    return C.g1_measure({"tpl": z["draft"], "reads": z["reads"]})


def _main(argv):
    if argv[:1] == ["heights"]:
        for name, z in low_complexity_zmws():
            s, res = add_reads(z["draft"], z["reads"], -5.0)
            ref = s.refine()
            q = s.qvs() if ref["converged"] else []
            acc = 1.0 - sum(10.0 ** (-v / 10.0) for v in q) / max(1, len(q))
            s2, _ = add_reads(z["draft"], z["reads"], -5.0)
            print(name, "len", len(z["draft"]), "add", res, "tallest", [tallest(s2, k) for k in range(len(res))],
                  "refine", ref["converged"], ref["n_tested"], ref["n_applied"], "min qv", min(q) if q else None,
                  "acc", round(acc, 4), flush=True)
        for L in (150, 300):
            h = hostile_zmw(L)
            for thr in (NAN, -5.0):
                s, res = add_reads(h["zmw"]["draft"], h["reads"], thr)
                print("hostile", L, "threshold", thr, "counts", [res.count(k) for k in range(5)])
                if math.isnan(thr):
                    for k, n in enumerate(h["names"]):
                        print("  ", n, "len", len(h["reads"][k]["seq"]), "result", res[k],
                              "tallest", tallest(s, k) if res[k] == 0 else None)
                else:
                    print("  ", [(n, r) for n, r in zip(h["names"], res)])
    elif argv[:1] == ["search"]:
        for L, seed, names in find_deactivation(int(argv[1]) if len(argv) > 1 else 40, want=10**9):
            print("L", L, "seed", seed, "deactivated", names, flush=True)
    elif argv[:1] == ["g1"]:
        for name in G1_CASES:
            pc = g1_gaps(name)
            top = sorted(pc.items(), key=lambda kv: -kv[1])
            print(name, "largest gaps by class (type, from start, from end):", [(c, repr(v)) for c, v in top[:3]],
                  flush=True)


if __name__ == "__main__":
    _main(sys.argv[1:])

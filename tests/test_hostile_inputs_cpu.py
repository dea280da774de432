"""The inputs of tests/test_hostile_inputs_gpu.py do what that file relies on -- conditions on the inputs, checked
with the CPU restatement alone -- and the restatement agrees with itself on low-complexity templates, where it was
never pinned: ScoreMutation against the refill of two fresh scorers (tests/arrow_multibase_common.refill_deltas).

Observed here (python -m tests.hostile_inputs heights):
  low-complexity tallest columns per read   A120 55/37/46/38/38   G120 62/57/51/60/50   A400 85/61/74/64/82
                                            AC60 27-40   CAG40 26-31   CT300 65/93/67/74/59   the rest 19-33
  low-complexity refines (tested, applied)  CT300 15498, 51; runlength 4034, 19; AC60 3183, 15; A400 5664, 15
  lowest QV / predicted accuracy            A120 2 / 0.9778; runlength 2 / 0.9700; CT300 3 / 0.9691; CAG40 6 / 0.9935
  hostile L = 150 AddRead results           NaN: 37 SUCCESS, 1 ALPHABETAMISMATCH;  -5.0: 15 / 1 / 22 POOR_ZSCORE
  hostile L = 300 AddRead results           NaN: 38 SUCCESS, 8 ALPHABETAMISMATCH;  -5.0: 20 / 8 / 18 POOR_ZSCORE
  hostile L = 300 tallest SUCCESS columns   19 (a clean pass) to 298 (ins_mid_200); 266 / 262 / 298 rows take three
                                            128-row chunks, 131-233 rows two
"""
import math

import pytest

from tests import hostile_inputs as H

SUCCESS, ALPHABETAMISMATCH, POOR_ZSCORE = 0, 1, 3

# python -m tests.hostile_inputs g1   (the CPU restatement alone): the largest |ScoreMutation - refill| over the
# classes g1_measure keeps, per ZMW, and the class it leaves out:
#   A120       1.7598371684357517e-05 at (INS, 3, 3)   excluded (INS, 0, 3): 6.592177034041136
#   AC60       3.5661072814718864e-06 at (INS, 3, 3)   excluded (INS, 0, 3): 9.807436284381758
#   runlength  4.637016104425129e-09  at (INS, 3, 3)   excluded (INS, 0, 3): 6.650740666328673
#   flank_T40  3.5339553505764343e-09 at (SUB, 3, 3)   excluded (INS, 0, 3): 8.360223227717249
# The random-template value is G1 = 4.29e-08 (tests/test_arrow_multibase_cpu.py).  Homopolymer and dinucleotide
# templates sit 100 to 400 times higher: their bands are wide and flat, so the cells ScoreMutation's extension leaves
# outside the old template's band carry more of the likelihood than on a random template (the band cut is e^-12.5 =
# 3.7e-06 of a column's maximum).  The bound is ten times the largest measured value, the margin WIDE_TOL's argument
# takes per extension column (tests/test_arrow_multibase_gpu.py).
G1 = 4.294581756880689e-08
G1_LOW = {"A120": 1.7598371684357517e-05, "AC60": 3.5661072814718864e-06, "runlength": 4.637016104425129e-09,
          "flank_T40": 3.5339553505764343e-09}
G1_LOW_TOL = 10 * max(G1_LOW.values())
EXCLUDED_CLASSES = {(0, 0, 3)}   # insertions at template position 0, as on random templates: 6.4 to 9.8 nats here


@pytest.fixture(scope="module")
def low():
    """Per low-complexity ZMW: AddRead results at -5.0, tallest column per read, the refine's record, QVs, accuracy."""
    out = {}
    for name, z in H.low_complexity_zmws():
        s, res = H.add_reads(z["draft"], z["reads"], -5.0, z["snr"])
        tall = [H.tallest(s, k) for k in range(len(res))]
        ref = s.refine()
        q = s.qvs() if ref["converged"] else []
        acc = 1.0 - sum(10.0 ** (-v / 10.0) for v in q) / max(1, len(q))
        out[name] = {"res": res, "tallest": tall, "refine": ref, "qvs": q, "acc": acc}
        print(name, res, tall, ref["converged"], ref["n_tested"], ref["n_applied"], min(q) if q else None, acc)
    return out


def test_low_complexity_set_is_complete():
    zs = H.low_complexity_zmws()
    assert [n for n, _ in zs] == H.LOW_COMPLEXITY_NAMES and len(zs) == 10
    t = {n: z["truth"] for n, z in zs}
    assert (t["A120"], t["G120"], t["A400"]) == ("A" * 120, "G" * 120, "A" * 400)
    assert (t["AC60"], t["CAG40"], t["CT300"]) == ("AC" * 60, "CAG" * 40, "CT" * 300)
    assert len(t["AT150"]) == 150 and set(t["AT150"]) == {"A", "T"}
    assert t["flank_T40"][40:80] == "T" * 40 and t["flank_GA30"][40:100] == "GA" * 30
    for _, z in zs:
        assert len(z["reads"]) == 5 and [r["strand"] for r in z["reads"]] == [0, 1, 0, 1, 0]
        assert all((r["ts"], r["te"]) == (0, len(z["draft"])) for r in z["reads"]) and z["snr"] == H.SNR
    assert H.low_complexity_zmws()[0][1] == H.zmw_of_truth(H._rng(1211), "A" * 120)   # fixed seeds


def test_low_complexity_reads_add_and_refines_converge(low):
    for name, r in low.items():
        assert r["res"] == [SUCCESS] * 5, name
        assert r["refine"]["converged"], name


def test_low_complexity_band_heights(low):
    """G120 brushes the 16-lane path's 64-row buffer from below; A400 and CT300 pass it during the fill."""
    assert any(56 <= h <= 63 for h in low["G120"]["tallest"]), low["G120"]["tallest"]
    assert max(low["A400"]["tallest"]) >= 65 and max(low["CT300"]["tallest"]) >= 65


def test_low_complexity_qvs_reach_both_sides_of_the_cut(low):
    assert any(min(r["qvs"]) <= 3 for r in low.values())
    assert any(r["acc"] < 0.98 for r in low.values()) and any(r["acc"] > 0.99 for r in low.values())
    # a ZMW within 1e-3 of the 0.98 cut would leave the GPU test's PoorQuality side open: none is
    assert sum(abs(r["acc"] - 0.98) > 1e-3 for r in low.values()) >= 8


def test_hostile_reads_are_the_named_set():
    for L in (150, 300):
        h = H.hostile_zmw(L)
        names = h["names"][5:]
        want = [f"ins_random_{n}" for n in H.BURSTS] + [f"ins_homopolymer_{n}" for n in H.BURSTS]
        want += [f"del_{n}" for n in H.BURSTS]
        want += ["half_junk", "junk_head_30", "junk_tail_30", "cut_head_40", "cut_tail_40", "wrong_strand",
                 "errors_15pct", "errors_10pct", "errors_5pct", "junk_L", "junk_2L", "duplicate", "one_base"]
        want += [f"ins_mid_{n}" for n in range(60, L + 1, 20)]
        assert names == want
        r = dict(zip(h["names"], h["reads"]))
        assert all((x["strand"], x["ts"], x["te"]) == (0, 0, len(h["zmw"]["draft"])) for x in h["reads"][5:])
        assert len(r["junk_L"]["seq"]) == L and len(r["junk_2L"]["seq"]) == 2 * L and len(r["one_base"]["seq"]) == 1
        d = r["duplicate"]["seq"]
        assert d[:len(d) // 2] == d[len(d) // 2:]
        assert h["reads"][:5] == H.synth.make_zmws(1, L, 5, seed=H.HOSTILE_ZMW_SEEDS[L])[0]["reads"]


def test_hostile_set_at_nan_reaches_multi_chunk_columns_and_mismatches():
    h = H.hostile_zmw(300)
    s, res = H.add_reads(h["zmw"]["draft"], h["reads"], H.NAN)
    tall = {n: H.tallest(s, k) for k, n in enumerate(h["names"]) if res[k] == SUCCESS}
    print(sorted(tall.items(), key=lambda kv: kv[1]))
    assert any(129 <= v <= 256 for v in tall.values()) and any(v > 256 for v in tall.values())
    assert min(tall[f"pass_{k}"] for k in range(5)) <= 30   # next to a 20-30-row read in the same ZMW
    mism = {n for n, x in zip(h["names"], res) if x == ALPHABETAMISMATCH and n != "one_base"}
    assert len(mism) >= 3, mism
    assert set(res) <= {SUCCESS, ALPHABETAMISMATCH}
    # L = 150: the same reads stay shorter; its tallest column still leaves the 16-lane buffer
    h = H.hostile_zmw(150)
    s, res = H.add_reads(h["zmw"]["draft"], h["reads"], H.NAN)
    assert max(H.tallest(s, k) for k in range(len(res)) if res[k] == SUCCESS) > 64


@pytest.mark.parametrize("L", [150, 300])
def test_hostile_set_at_minus_five_is_gated(L):
    h = H.hostile_zmw(L)
    _, res = H.add_reads(h["zmw"]["draft"], h["reads"], -5.0)
    print(L, [res.count(k) for k in range(5)])
    assert res[:5] == [SUCCESS] * 5
    assert res.count(POOR_ZSCORE) >= 5
    assert res[5:].count(SUCCESS) >= 1


@pytest.mark.parametrize("L,seed,names", H.DEACTIVATION_SEEDS)
def test_committed_deactivation_seeds_still_deactivate(L, seed, names):
    got = H.deactivated_reads(L, seed)
    assert got and got == list(names)


def test_deactivation_seeds_are_committed():
    assert len(H.DEACTIVATION_SEEDS) >= 2


@pytest.mark.parametrize("name", H.G1_CASES)
def test_restatement_scores_match_its_own_refills_on_low_complexity(name):
    per_class = H.g1_gaps(name)
    worst = max(v for c, v in per_class.items() if c not in EXCLUDED_CLASSES)
    print(name, "largest gap", repr(worst), "bound", G1_LOW_TOL, sorted(per_class.items(), key=lambda kv: -kv[1])[:3])
    assert {c for c, v in per_class.items() if v > G1_LOW_TOL} == EXCLUDED_CLASSES
    assert all(per_class[c] > 1.0 for c in EXCLUDED_CLASSES)
    assert worst <= G1_LOW_TOL
    assert worst == pytest.approx(G1_LOW[name], rel=1e-3)   # the constants above are what this measures
    assert not math.isnan(worst)

"""Pairwise alignment on the GPU (pbccs_align_batch: k_align_fill / k_align_trace) against the restatement of the
reference's two routines in tests/test_align_cpu.py.  Everything is compared for equality: transcripts as strings,
Align's int score exactly, the affine score through float.hex.  Shapes are the smallest that reach every path of
the fill: each compiled rows-per-lane R at its strip edges (64 R - 1, 64 R, 64 R + 1, 2 * 64 R + 1 query rows), the
lane edges 63 / 64 / 65, targets shorter than, equal to and longer than a wavefront's skew."""
import random
import subprocess

import numpy as np
import pytest

from tests.test_align_cpu import (AFFINE_DEFAULT, KATS, WalkLeavesMatrix, build_driver, ref,
                                  transcript_of)

pytestmark = pytest.mark.gpu

NW, AFFINE, IUPAC = 0, 1, 2
KINDS = (NW, AFFINE, IUPAC)
ROWS_PER_LANE = (2, 4, 8)   # align_kernels.hpp: kRowsPerLane
EINVAL, EOOM, ERANGE = -1, -2, -5


@pytest.fixture(scope="module")
def eng():
    import pbccs_amd
    return pbccs_amd.Engine(0)


def params_of(kind, values):
    import pbccs_amd as P
    if values is None:
        return None
    if kind == NW:
        return P.AlignConfig(P.AlignParams(*values))
    return P.AffineAlignmentParams(*values)


def fhex(x):
    return float(x).hex()


def check(eng, pairs, kind, values=None):
    """One align_batch call; every pair equals the restatement."""
    from pbccs_amd import align as A
    alns, scores = A.align_batch(pairs, kind, params_of(kind, values), engine=eng)
    assert len(alns) == len(scores) == len(pairs)
    for k, ((t, q), a, s) in enumerate(zip(pairs, alns, scores)):
        tr, es = ref(kind, t, q, values)
        assert a.Transcript() == tr, (kind, k, len(t), len(q))
        assert a.Target().replace("-", "") == t and a.Query().replace("-", "") == q
        if kind == NW:
            assert s == es, (k, len(t), len(q))
        else:
            assert fhex(s) == fhex(es), (kind, k, len(t), len(q))
    return alns, scores


def mutated_pair(rng, qlen, tlen, alphabet="ACGT", rate=0.15):
    """A seeded mutated copy: the query is a base sequence, the target its copy with substitutions and indels, cut
    or extended to tlen."""
    q = [rng.choice(alphabet) for _ in range(qlen)]
    t = []
    for c in q:
        u = rng.random()
        if u < rate / 3:
            continue
        if u < 2 * rate / 3:
            t.append(rng.choice(alphabet))
        elif u < rate:
            t.extend((c, rng.choice(alphabet)))
        else:
            t.append(c)
    while len(t) < tlen:
        t.append(rng.choice(alphabet))
    return "".join(t[:tlen]), "".join(q)


# ---- 1. the reference's known answers --------------------------------------------------------------------------
def test_golden_cases_all_kinds(eng):
    cases = KATS["align"] + KATS["affine"] + KATS["iupac"] + [KATS["affine_large_gap"], KATS["align_peer"]]
    pairs = [(c["target"], c["query"]) for c in cases]
    for kind in KINDS:
        alns, _ = check(eng, pairs, kind)
        own = {NW: KATS["align"], AFFINE: KATS["affine"] + [KATS["affine_large_gap"]], IUPAC: KATS["iupac"]}[kind]
        for c, a in zip(cases, alns):
            if any(c is o for o in own):   # the reference's own expectation for this aligner
                e = c["expect"]
                assert a.Target() == e.get("Target", a.Target()) and a.Query() == e.get("Query", a.Query())
                assert a.Transcript() == e.get("Transcript", a.Transcript())
    c = KATS["align_peer"]
    _, scores = check(eng, [(c["target"], c["query"])], NW, tuple(c["params"]))
    assert scores == [134]


def test_single_pair_entry_points(eng):
    import pbccs_amd as P
    a, s = P.Align("GATTACA", "TT", return_score=True, engine=eng)
    assert (a.Target(), a.Query(), s) == ("GATTACA", "--TT---", -5)
    a = P.AlignAffine("GATTACA", "GATTTACA", engine=eng)
    assert (a.Target(), a.Query()) == ("GA-TTACA", "GATTTACA")
    a = P.AlignAffineIupac("GATTTT", "GMTTT", engine=eng)
    assert (a.Target(), a.Query()) == ("GATTTT", "GM-TTT")
    assert P.TargetToQueryPositions(a) == [0, 1, 2, 2, 3, 4, 5]


# ---- 2. strip and lane edges -------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", ROWS_PER_LANE)
def test_strip_edges_forced_rows_per_lane(eng, monkeypatch, rows):
    monkeypatch.setenv("PBCCS_ALIGN_ROWS_PER_LANE", str(rows))
    rng = random.Random(1000 + rows)
    strip = 64 * rows
    pairs = [mutated_pair(rng, I, J) for I in (strip - 1, strip, strip + 1, 2 * strip + 1) for J in (1, 2, 70)]
    for kind in KINDS:
        check(eng, pairs, kind)


def test_strip_edges_chosen_rows_per_lane(eng):
    """The same query lengths with the engine's own choice of R (the thresholds at 128, 256 and 512 rows)."""
    rng = random.Random(77)
    lens = sorted({I for r in ROWS_PER_LANE for I in (64 * r - 1, 64 * r, 64 * r + 1, 2 * 64 * r + 1)})
    pairs = [mutated_pair(rng, I, J) for I in lens for J in (1, 2, 70)]
    for kind in KINDS:
        check(eng, pairs, kind)


@pytest.mark.parametrize("rows", (0,) + ROWS_PER_LANE)
def test_lane_edges(eng, monkeypatch, rows):
    if rows:
        monkeypatch.setenv("PBCCS_ALIGN_ROWS_PER_LANE", str(rows))
    rng = random.Random(5 + rows)
    pairs = [mutated_pair(rng, I, J) for I in (1, 63, 64, 65) for J in (1, 64, 200)]
    for kind in KINDS:
        check(eng, pairs, kind)


# ---- 3. ties -----------------------------------------------------------------------------------------------------
def tie_pairs():
    rng = random.Random(31337)
    pairs = []
    for k in range(200):
        n = 1 + k
        unit = rng.choice(["A", "C", "AC", "GT", "TA"])
        q = (unit * n)[:n]
        t = list((unit * (n + 4))[:max(1, n + rng.randint(-3, 3))])
        for _ in range(rng.randint(0, 3)):   # indels and the odd foreign base
            p = rng.randrange(len(t) + 1)
            if rng.random() < 0.5 and len(t) > 1:
                del t[min(p, len(t) - 1)]
            else:
                t.insert(p, rng.choice(unit + unit[0]))
        pairs.append(("".join(t)[:200], q))
    return pairs


@pytest.mark.parametrize("kind,values", [(NW, None), (NW, (2, -1, -2, -2)), (AFFINE, None), (IUPAC, None)])
def test_tie_heavy_batch(eng, kind, values):
    pairs = tie_pairs()
    assert len(pairs) == 200 and {len(q) for _, q in pairs} == set(range(1, 201))
    check(eng, pairs, kind, values)


# ---- 4. parameters that are not exactly representable ---------------------------------------------------------------
@pytest.mark.parametrize("kind", (AFFINE, IUPAC))
def test_affine_parameters_not_dyadic(eng, kind):
    rng = random.Random(404)
    pairs = [mutated_pair(rng, rng.randint(1, 120), rng.randint(1, 120), rate=0.25) for _ in range(20)]
    pairs[0] = mutated_pair(rng, 120, 120, rate=0.25)
    check(eng, pairs, kind, (0.3, -1.1, -2.7, -0.4, -0.6))


# ---- 5. IUPAC ----------------------------------------------------------------------------------------------------
def test_iupac_codes_lowercase_and_n(eng):
    rng = random.Random(909)
    pairs = []
    for _ in range(24):
        t, q = mutated_pair(rng, rng.randint(20, 150), rng.randint(20, 150), rate=0.1)
        q = list(q)
        for p in range(len(q)):
            u = rng.random()
            if u < 0.15:
                q[p] = rng.choice("RYSWKM")
            elif u < 0.20:
                q[p] = rng.choice("acgtrymN")   # score as plain mismatches
        t = list(t)
        for p in range(len(t)):
            if rng.random() < 0.05:
                t[p] = rng.choice("RYSWKMNn")
        pairs.append(("".join(t), "".join(q)))
    alns, _ = check(eng, pairs, IUPAC)
    check(eng, pairs, IUPAC, (0.0, -1.0, -1.0, -0.5, -0.3))
    check(eng, pairs, AFFINE)
    assert any("R" in a.Transcript() for a in alns)
    # a partial match is a mismatch in the transcript
    a = check(eng, [("GATTTT", "GMTTT")], IUPAC)[0][0]
    assert a.Transcript() == "MRDMMM"


# ---- 6. batch semantics --------------------------------------------------------------------------------------------
def test_batch_order_degenerate_and_duplicates(eng):
    from pbccs_amd import align as A
    rng = random.Random(6)
    big = mutated_pair(rng, 300, 280)
    small = mutated_pair(rng, 7, 9)
    pairs = [small, ("", "ACGT"), big, ("ACGTT", ""), ("", ""), small, mutated_pair(rng, 130, 3), big, ("A", "A"),
             ("A", "C")]
    for kind in KINDS:
        alns, scores = check(eng, pairs, kind)
        assert alns[1].Transcript() == "IIII" and alns[3].Transcript() == "DDDDD" and alns[4].Transcript() == ""
        assert alns[0] == alns[5] and alns[2] == alns[7]
        for (t, q), a, s in zip(pairs, alns, scores):
            one, s1 = A.align_batch([(t, q)], kind, engine=eng)
            assert one[0] == a and (s1[0] == s if kind == NW else fhex(s1[0]) == fhex(s))


def test_short_cap_is_erange_with_len_set(eng):
    from pbccs_amd import align as A
    rng = random.Random(66)
    pairs = [mutated_pair(rng, 40, 44), mutated_pair(rng, 90, 80), ("ACGT", ""), mutated_pair(rng, 10, 12)]
    for kind in KINDS:
        rc0, full = A.align_batch_raw(pairs, kind, engine=eng)
        assert rc0 == 0
        caps = [len(t) + len(q) for t, q in pairs]
        caps[1] = full[1][3] - 1
        caps[2] = 0
        rc, res = A.align_batch_raw(pairs, kind, engine=eng, caps=caps)
        assert rc == ERANGE
        assert [r[2] for r in res] == [0, ERANGE, ERANGE, 0]
        assert res[1][3] == full[1][3] and res[2][3] == 4          # len set to what is needed
        assert res[0] == full[0] and res[3] == full[3]             # the other outputs are intact
        assert res[1][1] == full[1][1]                             # the score is there all the same


# ---- 7. the workspace split ------------------------------------------------------------------------------------------
def test_workspace_split_and_oversize_pair(monkeypatch):
    import pbccs_amd
    from pbccs_amd import align as A
    rng = random.Random(7)
    distinct = [mutated_pair(rng, 300, 300) for _ in range(10)]
    pairs = [distinct[k % 10] for k in range(50)]
    eng = pbccs_amd.Engine(0)
    want, want_scores = check(eng, pairs, AFFINE)
    A.align_stats(eng, reset=True)
    monkeypatch.setenv("PBCCS_ALIGN_WORKSPACE_MB", "4")   # one 300 x 300 pair's move store is 363 * 512 bytes
    got, got_scores = check(eng, pairs, AFFINE)
    st = A.align_stats(eng, reset=True)
    assert st["groups"] >= 2 and st["launches"] >= 2 and st["pairs"] == 50 and st["cells"] == 50 * 300 * 300
    assert got == want and [fhex(s) for s in got_scores] == [fhex(s) for s in want_scores]
    assert st["trace_steps"] == sum(a.Length() for a in got)
    # 3000 x 3000: 6 strips x 3063 steps x 512 bytes > 4 MB
    huge = ("ACGT" * 750, "ACGA" * 750)
    rc, res = A.align_batch_raw([pairs[0], huge, pairs[1]], AFFINE, engine=eng)
    assert rc == EOOM and [r[2] for r in res] == [0, EOOM, 0]
    assert res[0][0] == want[0].Transcript() and res[2][0] == want[1].Transcript()
    with pytest.raises(pbccs_amd.PbccsError) as e:
        A.align_batch([huge], NW, engine=eng)
    assert e.value.code == EOOM
    assert A.align_stats(eng)["cells"] == 2 * 300 * 300   # no device work for the oversize pair
    check(eng, pairs[:3], AFFINE)
    monkeypatch.delenv("PBCCS_ALIGN_WORKSPACE_MB")
    check(eng, pairs[:3] + [mutated_pair(rng, 600, 40)], NW)


def test_pathological_parameters_flag_the_pair(eng):
    """A gap extension so negative that GAP(i, 0) overflows to -inf: where the reference's walk would then read
    outside its matrices (the restatement raises), the pair is refused with PBCCS_EINVAL; otherwise it is equal."""
    from pbccs_amd import align as A
    vals = (0.0, -1.0, -1.0, -3e38, 0.0)
    ok = ("ACGT", "ACGT")
    for bad in [("A", "AAAA"), ("AAAA", "A"), ("ACGTAC", "AC")]:
        try:
            exp = ref(AFFINE, bad[0], bad[1], vals)
        except WalkLeavesMatrix:
            exp = None
        rc, res = A.align_batch_raw([ok, bad, ok], AFFINE, params_of(AFFINE, vals), engine=eng)
        assert res[0][0] == res[2][0] == "MMMM"
        if exp is None:
            assert rc == EINVAL and res[1][2] == EINVAL
        else:
            assert rc == 0 and res[1][0] == exp[0] and fhex(res[1][1]) == fhex(exp[1])
    # int32 overflow of the NW scores is refused per pair
    import pbccs_amd as P
    rc, res = A.align_batch_raw([ok, ("ACGT" * 3, "ACGT" * 3)], NW,
                                P.AlignConfig(P.AlignParams(1 << 27, -1, -1, -1)), engine=eng)   # 8 << 27 fits, 24 << 27 not
    assert rc == EINVAL and [r[2] for r in res] == [0, EINVAL]


# ---- 8. coexistence with the polish ------------------------------------------------------------------------------------
def test_polish_is_unchanged_by_align_on_the_same_engine():
    import pbccs_amd
    from pbccs_amd import synth
    eng = pbccs_amd.Engine(0)
    zmws = synth.make_zmws(4, 300, 6, seed=2024)
    before = pbccs_amd.polish_zmws(zmws, engine=eng)
    rng = random.Random(8)
    check(eng, [mutated_pair(rng, 200, 210) for _ in range(8)], AFFINE)
    check(eng, [mutated_pair(rng, 200, 210) for _ in range(8)], NW)
    after = pbccs_amd.polish_zmws(zmws, engine=eng)
    assert before == after


# ---- 9. the C++ facade ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,values", [(NW, (2, -1, -2, -2)), (AFFINE, AFFINE_DEFAULT),
                                         (IUPAC, (0.3, -1.1, -2.7, -0.4, -0.6))])
def test_align_facade_driver(eng, tmp_path, kind, values):
    from pbccs_amd import align as A
    rng = random.Random(99 + kind)
    pairs = [mutated_pair(rng, 150, 140), ("", "ACG"), ("GATTTT", "GMTTT"), ("ACGT", ""), mutated_pair(rng, 30, 70)]
    head = " ".join(str(v) for v in values) if kind == NW else " ".join(fhex(np.float32(v)) for v in values)
    lines = [f"{kind} {head}", str(len(pairs))] + [f"{t or '.'} {q or '.'}" for t, q in pairs]
    case = tmp_path / "align_case.txt"
    case.write_text("\n".join(lines) + "\n")
    out = subprocess.run([build_driver(), str(case)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    alns, scores = A.align_batch(pairs, kind, params_of(kind, values), engine=eng)
    want = [f"aln {a.Transcript()}." + (f" {s}" if kind == NW else "") for a, s in zip(alns, scores)]
    want.append(f"one {alns[0].Transcript()}.")
    assert out.stdout.split("\n")[:len(want)] == want
    assert [transcript_of(a.Target(), a.Query()) for a in alns] == [a.Transcript() for a in alns]

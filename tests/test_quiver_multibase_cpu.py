"""Multi-base Quiver mutations without a GPU: the reference's known answers (tests/golden/
quiver_multibase_kats.json: TestMultiReadMutationScorer.cpp:545-595, TestMutationScorer.cpp:227-277,
TestMutationEnumerator.cpp:107-137, TestMutations.cpp:89-181) against the CPU restatement and against the
host-only entry points pbccs_repeat_mutations / pbccs_apply_mutations.  Scores are compared for equality."""
import json
import os
import subprocess

import numpy as np
import pytest

from oracle import oracle as O
from pbccs_amd import Mutation
from pbccs_amd import quiver as Q
from pbccs_amd.lib import PbccsError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KATS = json.load(open(os.path.join(ROOT, "tests", "golden", "quiver_multibase_kats.json")))
RECURSORS = ("SparseSse", "SparseSimple", "DenseSse", "DenseSimple")


def mk(m):
    t, s, e, b = m
    return Mutation(t, s, b if t != 1 else "-", end=e)


def oracle_score(o, m, fast=False):
    t, s, e, b = m
    return O._qlib().qorc_scorer_score(o._h, t, s, e, b.encode(), 1 if fast else 0)


def oracle_ms_score(o, r, m):
    t, s, e, b = m
    return O._qlib().qorc_ms_score(o._h, r, t, s, e, b.encode())


@pytest.mark.parametrize("recursor", RECURSORS)
def test_oracle_bounds_known_answers(recursor):
    k = KATS["bounds"]
    o = O.QuiverScorer(k["tpl"], KATS["params"], moves=k["moves"], score_diff=k["score_diff"],
                       fast_threshold=k["fast_threshold"], recursor=recursor)
    for r in k["reads"]:
        assert o.add_read(r["seq"], r["strand"], r["ts"], r["te"])
    for c in k["checks"]:
        assert oracle_score(o, c["mut"]) == c["expected"], c


def test_oracle_dinucleotide_known_answers():
    d = KATS["dinucleotide"]
    for sc in d["scorers"]:
        o = O.QuiverScorer(sc["tpl"], KATS["params"], moves=d["moves"], score_diff=d["score_diff"],
                           recursor=d["recursor"])
        assert o.add_read(sc["read"])
        for c in sc["checks"]:
            assert oracle_ms_score(o, 0, c["mut"]) == c["expected"], (sc["name"], c)
            # the reference's expectation is ReadScorer::Score(expected_template, read)
            e = O.QuiverScorer(c["expected_template"], KATS["params"], moves=d["moves"], score_diff=d["score_diff"],
                               recursor=d["recursor"])
            assert e.add_read(sc["read"])
            assert e.baseline() == c["expected"], (sc["name"], c)


def as_tuple(m):
    return (m.type, m.start, m.end, m.new_bases)


def test_repeat_mutations_known_answers():
    for c in KATS["enumerator"]["cases"]:
        got = Q.RepeatMutationEnumerator(c["tpl"], c["repeat_length"], c["min_repeat_elements"]).Mutations()
        assert len(got) == len(c["expected"])
        assert {as_tuple(m) for m in got} == {tuple(e) for e in c["expected"]}
    c = KATS["enumerator"]["cases"][0]
    assert {as_tuple(m) for m in Q.DinucleotideRepeatMutationEnumerator(c["tpl"], 3).Mutations()} == \
        {tuple(e) for e in c["expected"]}


def test_repeat_mutations_early_return():
    tpl = "AC" * 40
    assert Q.RepeatMutationEnumerator(tpl, 2, 0).Mutations() == []
    assert Q.RepeatMutationEnumerator(tpl, 2, -1).Mutations() == []
    assert Q.RepeatMutationEnumerator("A" * 200, 32, 1).Mutations() == []
    assert len(Q.RepeatMutationEnumerator("A" * 200, 31, 3).Mutations()) > 0


def test_repeat_mutations_window_and_stepping():
    """Only repeats that start in the window; after a run the scan resumes on the second base of its last
    element, so the shifted run CACAC of ACACAC is not reported again (MutationEnumerator.cpp:206-214)."""
    tpl = "TTACACACGG"
    e = Q.DinucleotideRepeatMutationEnumerator(tpl, 3)
    assert [as_tuple(m) for m in e.Mutations()] == [(0, 2, 2, "AC"), (1, 2, 4, "")]
    assert e.Mutations(3, 10) == []             # CACAC has only two whole CA elements
    assert [as_tuple(m) for m in e.Mutations(2, 4)] == [(0, 2, 2, "AC"), (1, 2, 4, "")]   # runs past the window's end
    assert e.Mutations(-5, 2) == []
    # with two elements enough, the stepping is what keeps the shifted run CACA at 3 out
    two = Q.DinucleotideRepeatMutationEnumerator(tpl, 2)
    assert [as_tuple(m) for m in two.Mutations()] == [(0, 2, 2, "AC"), (1, 2, 4, "")]


def transcript_to_mtp(tx):   # TargetToQueryPositions(transcript), PairwiseAlignment.cpp:264-297
    out, q = [], 0
    for c in tx:
        if c in "MR":
            out.append(q)
            q += 1
        elif c == "D":
            out.append(q)
        else:
            q += 1
    return out + [q]


def test_apply_mutations_known_answers():
    for c in KATS["apply"]["cases"]:
        tpl, mtp = Q.ApplyMutations([mk(m) for m in c["muts"]], c["tpl"])
        assert len(mtp) == len(c["tpl"]) + 1
        if "template" in c:
            assert tpl == c["template"]
        if "mtp" in c:
            assert mtp == c["mtp"]
        if "transcript" in c:
            assert mtp == transcript_to_mtp(c["transcript"])


def slice_edit(t, muts, s, e):
    """m[s, e) applied to t[s, e): the edits of the slice, an insertion at the slice's own start excluded (it lands
    before t'[mtp[s]], Mutation.cpp:173-191) and one at its end included."""
    out, pos = [], max(s, 0)   # s = -1: the whole template, an insertion at 0 included
    for m in sorted(muts):
        if m.type == 0:
            if not (s < m.start <= e):
                continue
        elif not (s <= m.start and m.end <= e):
            continue
        out.append(t[pos:m.start])
        out.append(m.new_bases)
        pos = m.end
    out.append(t[pos:e])
    return "".join(out)


def test_apply_mutations_random_slices():
    rng = np.random.default_rng(20240)
    for _ in range(40):
        L = int(rng.integers(30, 120))
        t = "".join(rng.choice(list("ACGT"), L))
        muts, p = [], int(rng.integers(0, 4))
        while p + 8 < L:
            kind, w = int(rng.integers(0, 3)), int(rng.integers(1, 5))
            bases = "".join(rng.choice(list("ACGT"), w))
            muts.append(Mutation(0, p, bases) if kind == 0 else
                        Mutation(1, p, "-", end=p + w) if kind == 1 else Mutation(2, p, bases))
            p += w + int(rng.integers(3, 12))   # well separated
        order = rng.permutation(len(muts))
        tp, mtp = Q.ApplyMutations([muts[i] for i in order], t)
        assert tp == slice_edit(t, muts, -1, L)
        assert mtp[0] == (len(muts[0].new_bases) if muts and muts[0].type == 0 and muts[0].start == 0 else 0)
        assert mtp[L] == len(tp)
        inside = set()
        for m in muts:
            inside.update(range(m.start + 1, m.end))   # a slice bound strictly inside an edited span cuts it
        for _ in range(25):
            s, e = sorted(int(x) for x in rng.integers(0, L + 1, 2))
            if s in inside or e in inside:
                continue
            assert tp[mtp[s]:mtp[e]] == slice_edit(t, muts, s, e), (t, muts, s, e)


def test_apply_mutations_refusals():
    for muts in ([Mutation(1, 5, "-", end=9)], [Mutation(0, 9, "AC")], [Mutation(2, 6, "ACG")],
                 [Mutation(2, 1, "AC", end=4)], [Mutation(1, 1, "-", end=4), Mutation(2, 2, "AC")]):
        with pytest.raises(PbccsError):
            Q.ApplyMutations(muts, "GATTACAG")
    assert Q.ApplyMutations([Mutation(0, 8, "AC")], "GATTACAG")[0] == "GATTACAGAC"


def test_mutation_value():
    m = Mutation(0, 3, "AC")
    assert (m.start, m.end, m.new_bases, m.LengthDiff(), m.is_single_base()) == (3, 3, "AC", 2, False)
    d = Mutation(1, 3, "-", end=6)
    assert (d.new_bases, d.LengthDiff()) == ("", -3)
    s = Mutation(2, 3, "ACG")
    assert (s.end, s.LengthDiff()) == (6, 0)
    one = Mutation(2, 3, "A")
    assert one.is_single_base() and one.new_base == "A" and repr(one) == "Substitution(A)@3"
    assert sorted([s, d, m, one]) == [m, one, d, s]   # start, end, type, bases (Mutation-inl.hpp:179-186)
    with pytest.raises(PbccsError):
        m._c()   # the single-base ABI (and with it the Arrow scorer) refuses it


def test_model_driver_builds_and_runs(tmp_path):
    """The stand-alone driver over arrow_model.cpp (tests/cpp/model_multibase_driver.cpp): the enumerator and
    apply known answers in plain C++, no engine."""
    exe = str(tmp_path / "model_multibase_driver")
    src = [os.path.join(ROOT, "tests", "cpp", "model_multibase_driver.cpp"),
           os.path.join(ROOT, "pbccs_amd", "csrc", "arrow_model.cpp")]
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "pbccs_amd", "csrc"), *src, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "ok" in out.stdout

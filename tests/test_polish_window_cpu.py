"""Windowed polish, the parts that need no device: the restatement's own known answers (plan,
cuts, join), the library's host-only entry points against the restatement, the refusals, and the restatement end to
end with the oracle polishing each window."""
import ctypes
import os
import random
import subprocess

import pytest

import polish_window_restatement as W
import sparse_restatement as SR


# ---- rule 1: the plan ----------------------------------------------------------------------------------------
def test_plan_known_answers():
    assert W.plan(700, 200, 100) == [(0, 300), (200, 500), (400, 700)]
    assert W.plan(701, 200, 100) == [(0, 251), (151, 402), (302, 553), (453, 701)]


def test_plan_short_drafts_have_one_window():
    for L in (0, 1, 10, 299, 300):
        assert W.plan(L, 200, 100) == [(0, L)]
    assert len(W.plan(301, 200, 100)) == 2


def test_plan_covers_the_draft_with_overlaps():
    rng = random.Random(1)
    for _ in range(300):
        w = rng.randint(3, 3000)
        v = rng.randint(2, w - 1)
        L = rng.randint(0, 25000)
        wins = W.plan(L, w, v)
        assert wins[0][0] == 0 and wins[-1][1] == L
        for (s0, e0), (s1, e1) in zip(wins, wins[1:]):
            assert s0 < s1 <= e0 <= e1
            assert e0 - s0 <= w + v


# ---- rule 2: the cuts ----------------------------------------------------------------------------------------
CHAIN = [(10, 12), (20, 22), (30, 40), (50, 41)]


def test_cut_before_the_first_anchor():
    assert W.cut(CHAIN, 4, 100) == 6      # 12 - (10 - 4)
    assert W.cut([(10, 3)], 2, 100) == 0   # never below the read's start


def test_cut_after_the_last_anchor():
    assert W.cut(CHAIN, 55, 100) == 46
    assert W.cut(CHAIN, 200, 100) == 100   # never past the read's end


def test_cut_is_clamped_by_the_next_anchor():
    assert W.cut(CHAIN, 25, 100) == 27
    assert W.cut(CHAIN, 45, 100) == 41     # 40 + 15 lowered to the next anchor's 41
    assert W.cut(CHAIN, 30, 100) == 40


def test_cuts_are_monotone_over_boundaries():
    rng = random.Random(2)
    for _ in range(200):
        h = sorted(rng.sample(range(400), 12))
        v = sorted(rng.sample(range(450), 12))
        chain = list(zip(h, v))
        got = [W.cut(chain, b, 430) for b in range(0, 420)]
        assert got == sorted(got)
        assert all(0 <= c <= 430 for c in got)


def test_strand_one_slice_is_a_pointer_into_the_read():
    read = {"seq": "ACGGTTACGATCGATTTGCA", "strand": 1}
    f = W.forward_text(read)
    for cb, ce in ((0, 20), (3, 11), (7, 7), (19, 20)):
        assert SR.revcomp(W.slice_as_sequenced(read, cb, ce)) == f[cb:ce]
        n = len(read["seq"])
        assert W.slice_as_sequenced(read, cb, ce) == read["seq"][n - ce:n - cb]


# ---- rule 4: the join ----------------------------------------------------------------------------------------
def test_join_found_at_mid():
    ta, tb = "M" * 300, "M" * 300
    assert W.join(ta, (0, 300), tb, (200, 500), 8) == (250, 250, 50)


def test_join_pushed_aside_by_an_indel_at_mid():
    # a deleted draft column at 250 in the left window: every p with p - 8 <= 250 <= p + 7, 243..258, sees it; the
    # order mid, +1, -1, ... tries 258 (refused) and then 242
    ta = "M" * 250 + "D" + "M" * 49
    tb = "M" * 300
    assert W.join(ta, (0, 300), tb, (200, 500), 8) == (242, 242, 42)
    # a mismatch at column 242 as well: 259 is next
    ta = "M" * 242 + "R" + "M" * 7 + "D" + "M" * 49
    assert W.join(ta, (0, 300), tb, (200, 500), 8) == (259, 258, 59)
    # an inserted consensus base between columns 249 and 250 of the right window's transcript: 243..257 straddle it
    tb = "M" * 50 + "I" + "M" * 250
    assert W.join("M" * 300, (0, 300), tb, (200, 500), 8) == (258, 258, 59)


def test_join_none():
    ta = ("M" * 7 + "R") * 38
    assert W.join(ta[:300], (0, 300), "M" * 300, (200, 500), 8) is None
    assert W.join("M" * 300, (0, 300), "M" * 300, (290, 590), 8) is None   # an overlap shorter than 2 guard


# ---- the library's host-only entry points ------------------------------------------------------------------------
def _random_transcript(rng, width):
    out, c = [], 0
    while c < width:
        x = rng.random()
        if x < 0.85:
            out.append("M")
            c += 1
        elif x < 0.90:
            out.append("R")
            c += 1
        elif x < 0.95:
            out.append("D")
            c += 1
        else:
            out.append("I")
    if rng.random() < 0.3:
        out.append("I")
    return "".join(out)


def test_library_plan_equals_the_restatement():
    from pbccs_amd import polish as P
    rng = random.Random(3)
    cases = [(700, 200, 100), (701, 200, 100), (300, 200, 100), (301, 200, 100), (0, 200, 100), (20000, 2000, 200),
             (10000, 2000, 200), (1234, 7, 6), (50, 3, 2)]
    cases += [(rng.randint(0, 30000), w, rng.randint(2, w - 1)) for w in (rng.randint(3, 4000) for _ in range(200))]
    for L, w, v in cases:
        assert P.window_plan(L, w, v) == W.plan(L, w, v), (L, w, v)


def test_library_join_equals_the_restatement():
    from pbccs_amd import polish as P
    rng = random.Random(5)
    found = 0
    for _ in range(1500):
        g = rng.choice([1, 2, 3, 8])
        sa = rng.randint(0, 50)
        ea = sa + rng.randint(2 * g, 120)
        sb = rng.randint(sa + 1, ea)
        eb = max(sb, ea + rng.randint(-5, 60))
        ta, tb = _random_transcript(rng, ea - sa), _random_transcript(rng, eb - sb)
        got = P.window_join(ta, (sa, ea), tb, (sb, eb), g)
        assert got == W.join(ta, (sa, ea), tb, (sb, eb), g), (ta, tb, sa, ea, sb, eb, g)
        found += got is not None
    assert 300 < found < 1200
    for ta, wa, tb, wb in (("M" * 300, (0, 300), "M" * 300, (200, 500)),
                           ("M" * 250 + "D" + "M" * 49, (0, 300), "M" * 300, (200, 500)),
                           ("M" * 300, (0, 300), "M" * 50 + "I" + "M" * 250, (200, 500)),
                           (("M" * 7 + "R") * 38, (0, 304), "M" * 300, (200, 500))):
        assert P.window_join(ta, wa, tb, wb, 8) == W.join(ta, wa, tb, wb, 8)


def test_einval_cases():
    from pbccs_amd import lib as L
    from pbccs_amd import polish as P
    lib = L.load()
    nw = ctypes.c_int()
    for w, v, g, k in ((200, 200, 8, 8), (100, 200, 8, 8), (200, 15, 8, 8), (200, 100, 0, 8), (200, 100, 8, 3),
                       (200, 100, 8, 9), (200, 100, -1, 8)):
        assert not W.options_valid(w, v, g, k)
        wo = L.CWindowOptions(w, v, g, k)
        assert lib.pbccs_window_plan(700, ctypes.byref(wo), None, 0, ctypes.byref(nw)) == -1
        # refused before the engine is looked at: a null engine would otherwise be the error
        assert lib.pbccs_polish_windowed(None, None, 0, None, ctypes.byref(wo), None, None) == -1
        assert b"window options" in lib.pbccs_last_error()
        need = ctypes.c_longlong()
        assert lib.pbccs_window_slices(None, None, 0, ctypes.byref(wo), 10, None, None, 0, ctypes.byref(need), None) == -1
        assert b"window options" in lib.pbccs_last_error()
        assert lib.pbccs_ccs_batch_ex3(None, None, 0, None, None, ctypes.byref(wo), None, None, None) == -1
        with pytest.raises(ValueError):
            P.window_options(w, v, g, k)
    assert W.options_valid(200, 16, 8, 4) and W.options_valid(2000, 200, 8, 8)
    wo = L.CWindowOptions(200, 16, 8, 4)
    assert lib.pbccs_window_plan(700, ctypes.byref(wo), None, 0, ctypes.byref(nw)) == -5 and nw.value == 4
    # a transcript that does not span its window, or holds another character
    with pytest.raises(L.PbccsError):
        P.window_join("M" * 299, (0, 300), "M" * 300, (200, 500), 8)
    with pytest.raises(L.PbccsError):
        P.window_join("M" * 299 + "X", (0, 300), "M" * 300, (200, 500), 8)


def test_defaults():
    from pbccs_amd import lib as L
    wo = L.CWindowOptions()
    L.load().pbccs_window_options_default(ctypes.byref(wo))
    assert (wo.window, wo.overlap, wo.guard, wo.k) == (2000, 200, 8, 6)


# ---- the restatement end to end ------------------------------------------------------------------------------
def test_restatement_end_to_end_matches_the_whole_template_oracle():
    """make_zmws(6, 700, 8, seed=7) with W 200, V 100, k 6, g 8: no fallback, and every stitched consensus is the
    whole-template oracle consensus.  tests/test_polish_window_gpu.py relies on the zero fallbacks."""
    zmws, recs = W.synthetic_case(6, 700, 8, 7, 200, 100, 8, 6)
    whole = W.whole_template(6, 700, 8, 7)
    assert [r["fallback"] for r in recs] == [0] * 6
    for z, r, e in zip(zmws, recs, whole):
        assert r["windowed"] and len(r["windows"]) == len(W.plan(len(z["draft"]), 200, 100)) >= 3
        assert e["status"] == W.SUCCESS
        assert r["consensus"] == e["consensus"]
        assert len(r["qvs"]) == len(r["consensus"])
        assert r["add_read_results"] == e["add_read_results"] == [0] * 8
        assert r["n_passes"] == 8 and r["status_counts"] == [8, 0, 0, 0, 0]
        pieces = [w["cut_end"] - w["cut_begin"] for w in r["windows"]]
        assert sum(pieces) == len(r["consensus"]) and min(pieces) > 0


# ---- the C++ facade's host-only parts --------------------------------------------------------------------------
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "window_driver.cpp")
BIN = os.path.join(ROOT, "tests", "cpp", "_build", "window_driver")
LIBDIR = os.path.join(ROOT, "pbccs_amd", "_lib")


def build_driver():
    os.makedirs(os.path.dirname(BIN), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-I" + os.path.join(ROOT, "include"), SRC, "-L" + LIBDIR,
                           "-lpbccs_amd", "-Wl,-rpath," + LIBDIR, "-o", BIN])
    return BIN


def test_window_facade_driver_compiles_links_and_knows_the_answers():
    out = subprocess.run([build_driver()], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.split("\n")[0] == "known answers ok"

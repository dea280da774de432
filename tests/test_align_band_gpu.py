"""The certified banded fill on the GPU (pbccs_align_batch_ex: k_align_fill_band / k_align_trace_band, DESIGN.md
§3.19) against the unbanded align_batch on the same engine, and below about 600 x 600 also against the restatement
of tests/test_align_cpu.py.  Everything is compared for equality: transcripts as strings, Align's int score exactly,
the affine score through float.hex (a numerically zero score is exempt from the sign of zero).  The per-pair info
says which pairs were answered by a certified banded fill and which took the full fill, and why."""
import random

import pytest

from tests.align_band_restatement import block_indel_pair
from tests.test_align_cpu import ref
from tests.test_align_gpu import fhex, mutated_pair, params_of

pytestmark = pytest.mark.gpu

NW, AFFINE, IUPAC = 0, 1, 2
KINDS = (NW, AFFINE, IUPAC)
EOOM = -2
REASONS = {"certified", "not_certifiable", "covers_matrix", "store_not_smaller", "trace_flagged", "uncertified",
           "degenerate", "over_budget"}
NOT_DYADIC = (0.3, -1.1, -2.7, -0.4, -0.6)


@pytest.fixture(scope="module")
def eng():
    import pbccs_amd
    return pbccs_amd.Engine(0)


def same_score(kind, a, b):
    if kind == NW:
        return a == b
    if float(a) == 0.0 and float(b) == 0.0:
        return True
    return fhex(a) == fhex(b)


def check_band(eng, pairs, kind, band, values=None, with_ref=True):
    """One banded and one unbanded align_batch call on the same engine: every pair equal, info well-formed."""
    from pbccs_amd import align as A
    want, want_s = A.align_batch(pairs, kind, params_of(kind, values), engine=eng)
    got, got_s, info = A.align_batch(pairs, kind, params_of(kind, values), engine=eng, band=band, return_info=True)
    assert len(got) == len(got_s) == len(info) == len(pairs)
    for k, ((t, q), a, s, b, bs, inf) in enumerate(zip(pairs, want, want_s, got, got_s, info)):
        where = (kind, band, k, len(q), len(t), inf)
        assert b.Transcript() == a.Transcript(), where
        assert same_score(kind, bs, s), where + (bs, s)
        assert inf["reason"] in REASONS and 0 <= inf["attempts"] <= 2, where
        assert inf["banded"] == (inf["reason"] == "certified" and inf["attempts"] >= 1), where
        if with_ref and len(t) <= 600 and len(q) <= 600:
            tr, es = ref(kind, t, q, values)
            assert b.Transcript() == tr and same_score(kind, bs, es), where
    return got, got_s, info


def mutated(I, J, rate=0.02, alphabet="ACGT", salt=0):
    """The same pair for the same (I, J): the restatement's answers are shared between the cases that use it."""
    return mutated_pair(random.Random(I * 100003 + J * 17 + salt), I, J, alphabet, rate)


# ---- 1. strip edges with every rows-per-lane ------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("rows", (2, 4, 8))
def test_strip_edges_forced_rows_per_lane(eng, monkeypatch, rows, kind):
    monkeypatch.setenv("PBCCS_ALIGN_ROWS_PER_LANE", str(rows))
    from pbccs_amd import align as A
    strip = 64 * rows
    A.align_band_stats(eng, reset=True)
    n_banded = n_second = 0
    for w in (1, 2, 31, 32, 33):
        deltas = sorted({0, 1, -1, w, -w, w + 1, -(w + 1)})
        pairs = [mutated(I, I + d) for I in (strip - 1, strip, strip + 1, 2 * strip + 1) for d in deltas]
        # further strip counts, where a narrow band's store is far below the full one: an exact multiple of the
        # strip, one row short of it, and a fourth strip of one row
        pairs += [mutated(I, I + d) for I in (2 * strip - 1, 3 * strip, 3 * strip + 1) for d in (0, w, -(w + 1))]
        _, _, info = check_band(eng, pairs, kind, w)
        n_banded += sum(i["banded"] for i in info)
        n_second += sum(i["attempts"] == 2 for i in info)
        assert all(i["w"] >= w or not i["banded"] for i in info)
    st = A.align_band_stats(eng, reset=True)
    assert n_banded >= 30 and n_second >= 5            # both schedules ran through the banded kernels
    assert st["banded_pairs"] == n_banded and st["band_cells"] < st["full_cells"]


# ---- 2. the certificate's edge ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", (1, 5, 12))
def test_block_indel_one_and_two_attempts(eng, k):
    pair = block_indel_pair(k)
    for kind in KINDS:
        _, _, info = check_band(eng, [pair], kind, k)
        if kind == NW:
            assert info == [{"banded": True, "w": k, "attempts": 1, "reason": "certified"}]
        _, _, info = check_band(eng, [pair], kind, k - 1)
        if kind == NW:
            assert info[0]["banded"] and info[0]["attempts"] == 2 and info[0]["w"] >= k


# ---- 3. ties, strangers, parameters ------------------------------------------------------------------------------------
def repeat_pairs():
    rng = random.Random(4242)
    pairs = [("A" * 400, "A" * 390), ("A" * 385, "A" * 400), ("AC" * 200, "AC" * 193), ("AC" * 195 + "A", "AC" * 200),
             ("GT" * 150 + "G" * 9 + "GT" * 50, "GT" * 205)]
    t = list("AC" * 210)
    for _ in range(4):
        del t[rng.randrange(len(t))]
    pairs.append(("".join(t), "AC" * 206))
    return pairs


def test_homopolymer_and_dinucleotide_pairs(eng):
    pairs = repeat_pairs()
    assert all(len(t) != len(q) for t, q in pairs)
    for kind in KINDS:
        for band in (True, 3):
            _, _, info = check_band(eng, pairs, kind, band)
            assert sum(i["banded"] for i in info) >= 4


def test_unrelated_pairs_take_the_full_fill(eng):
    """Random pairs: the first score calls for a band hundreds of diagonals wide, whose store (for these one-strip
    shapes: the same steps as the full fill's) is no smaller than the full one."""
    rng = random.Random(777)
    pairs = [("".join(rng.choice("ACGT") for _ in range(J)), "".join(rng.choice("ACGT") for _ in range(I)))
             for I, J in ((512, 512), (512, 470), (512, 500))]
    for kind in KINDS:
        _, _, info = check_band(eng, pairs, kind, True)
        assert all(not i["banded"] and i["attempts"] == 1 and i["reason"] in ("covers_matrix", "store_not_smaller")
                   for i in info), info


def test_uncertifiable_parameters_take_the_full_fill(eng):
    pairs = [mutated(400, 404), mutated(300, 300)]
    _, _, info = check_band(eng, pairs, AFFINE, True, (0.0, -1.0, 0.5, -0.5, 0.0))    # a positive gap score
    assert [(i["banded"], i["reason"], i["attempts"]) for i in info] == [(False, "not_certifiable", 0)] * 2
    _, _, info = check_band(eng, pairs, NW, 8, (0, -1, 1, 1))
    assert [(i["banded"], i["reason"], i["attempts"]) for i in info] == [(False, "not_certifiable", 0)] * 2


@pytest.mark.parametrize("kind", (AFFINE, IUPAC))
def test_affine_parameters_not_dyadic(eng, kind):
    pairs = [mutated(I, I + d, rate) for I, d, rate in ((580, 3, 0.02), (600, -2, 0.01), (400, 0, 0.03), (1300, 5, 0.01))]
    for band in (True, 4):
        _, _, info = check_band(eng, pairs, kind, band, NOT_DYADIC)
        assert sum(i["banded"] for i in info) >= 3


def test_band_wider_than_the_matrix_and_a_one_column_target(eng):
    for kind in KINDS:
        _, _, info = check_band(eng, [mutated(300, 310), mutated(40, 9)], kind, 100000)
        assert [(i["banded"], i["reason"]) for i in info] == [(False, "covers_matrix")] * 2
        for band in (True, 0, 5):
            check_band(eng, [("A", "ACGT" * 75), ("ACGT" * 75, "C")], kind, band)


def test_mixed_batch_keeps_the_input_order(eng):
    rng = random.Random(31)
    pairs = [mutated(700, 703), ("", "ACGT"), block_indel_pair(5), ("ACGTT", ""), ("", ""), mutated(257, 250),
             ("A", "ACGT" * 75), repeat_pairs()[0], mutated(700, 703), mutated(1025, 1030),
             ("".join(rng.choice("ACGT") for _ in range(300)), "".join(rng.choice("ACGT") for _ in range(300))),
             repeat_pairs()[3], ("A", "C"), mutated(385, 385, 0.05)]
    for kind in KINDS:
        for band in (True, 2):
            got, got_s, info = check_band(eng, pairs, kind, band)
            assert [i["reason"] for i in info][1] == [i["reason"] for i in info][3] == "degenerate"
            assert got[0] == got[8] and info[0] == info[8] and info[0]["banded"]
            assert got[1].Transcript() == "IIII" and got[3].Transcript() == "DDDDD" and got[4].Transcript() == ""


# ---- 4. memory ------------------------------------------------------------------------------------------------------------
def test_banded_pair_fits_a_workspace_the_full_fill_exceeds(monkeypatch):
    import pbccs_amd
    from pbccs_amd import align as A
    eng = pbccs_amd.Engine(0)
    pair = mutated(1100, 1100, 0.01)
    want, want_s = A.align_batch([pair], NW, engine=eng)
    monkeypatch.setenv("PBCCS_ALIGN_WORKSPACE_MB", "1")
    rc, res = A.align_batch_raw([pair], NW, engine=eng)
    assert rc == EOOM and res[0][2] == EOOM                       # 3 strips x 1163 steps x 512 bytes
    got, got_s, info = A.align_batch([pair], NW, engine=eng, band=True, return_info=True)
    assert info[0]["banded"] and info[0]["reason"] == "certified"
    monkeypatch.delenv("PBCCS_ALIGN_WORKSPACE_MB")
    assert got[0].Transcript() == want[0].Transcript() and got_s == want_s


def test_20kb_pair_is_certified_at_the_auto_width():
    import pbccs_amd
    from pbccs_amd import align as A
    eng = pbccs_amd.Engine(0)
    pair = mutated(20000, 20000, 0.002)
    A.align_band_stats(eng, reset=True)
    A.align_stats(eng, reset=True)
    got, got_s, info = A.align_batch([pair], NW, engine=eng, band=True, return_info=True)
    bst = A.align_band_stats(eng, reset=True)
    assert A.align_stats(eng)["cells"] == 0                       # no full fill ran
    assert info == [{"banded": True, "w": 32, "attempts": 1, "reason": "certified"}]
    want, want_s = A.align_batch([pair], NW, engine=eng)
    full_bytes = A.align_stats(eng, reset=True)["bytes"]
    assert got[0].Transcript() == want[0].Transcript() and got_s == want_s
    assert 0 < bst["store_bytes"] < 0.05 * full_bytes, (bst["store_bytes"], full_bytes)
    assert bst["full_cells"] == 20000 * 20000 and bst["band_cells"] < 66 * 20000


# ---- 5. counters -------------------------------------------------------------------------------------------------------------
def test_stats_counters_add_up(eng):
    from pbccs_amd import align as A
    rng = random.Random(5)
    pairs = [mutated(700, 700), mutated(650, 655, 0.03), ("", "AC"), mutated(300, 310),
             ("".join(rng.choice("ACGT") for _ in range(500)), "".join(rng.choice("ACGT") for _ in range(500))),
             block_indel_pair(12)]
    A.align_band_stats(eng, reset=True)
    _, _, info = A.align_batch(pairs, NW, engine=eng, band=1, return_info=True)
    st = A.align_band_stats(eng, reset=True)
    assert st["pairs"] == len(pairs)
    assert st["banded_pairs"] == sum(i["banded"] for i in info) >= 3
    assert st["second_attempts"] == sum(i["attempts"] == 2 for i in info) >= 2
    assert st["banded_pairs"] + sum(st["fallbacks"].values()) == st["pairs"]
    for reason, count in st["fallbacks"].items():
        assert count == sum(i["reason"] == reason for i in info), reason
    assert st["fallbacks"]["degenerate"] == 1
    tried = [p for p, i in zip(pairs, info) if i["attempts"] >= 1]
    assert st["full_cells"] == sum(len(t) * len(q) for t, q in tried)
    assert 0 < st["band_cells"] and st["store_bytes"] > 0 and st["launches"] >= 2
    assert A.align_band_stats(eng)["pairs"] == 0
    # band=None leaves the counters alone
    A.align_batch(pairs, NW, engine=eng)
    assert A.align_band_stats(eng)["pairs"] == 0


# ---- 6. coexistence with the polish ------------------------------------------------------------------------------------------
def test_polish_is_unchanged_by_a_banded_call_on_the_same_engine():
    import pbccs_amd
    from pbccs_amd import synth
    eng = pbccs_amd.Engine(0)
    zmws = synth.make_zmws(4, 300, 6, seed=2024)
    before = pbccs_amd.polish_zmws(zmws, engine=eng)
    _, _, info = check_band(eng, [mutated(700, 704), mutated(900, 890)], AFFINE, True)
    assert all(i["banded"] for i in info)
    check_band(eng, [mutated(700, 704)], NW, 2)
    after = pbccs_amd.polish_zmws(zmws, engine=eng)
    assert before == after


def test_single_pair_entry_points_take_the_band(eng):
    import pbccs_amd as P
    t, q = mutated(700, 706)
    a, s = P.Align(t, q, return_score=True, engine=eng, band=True)
    b, s0 = P.Align(t, q, return_score=True, engine=eng)
    assert a == b and s == s0
    assert P.AlignAffine(t, q, engine=eng, band=8) == P.AlignAffine(t, q, engine=eng)
    assert P.AlignAffineIupac(t, q, engine=eng, band=True) == P.AlignAffineIupac(t, q, engine=eng)

"""The ends-free alignment rules without a GPU: the restatement against brute force, its numpy
form against its plain form, the tie rules on homopolymers with their exact extents, and every refusal of the Python
surface before an engine is touched."""
import itertools
import random

import pytest

from tests import align_modes_restatement as R

PARAM_SETS = ((0, -1, -1, -1), (3, -5, -4, -4), (2, -1, -1, -2), (2, -3, 0, -1))
MODES = (R.SEMIGLOBAL, R.LOCAL)


def random_pairs(seed, n, alphabet, max_t=9, max_q=7):
    rng = random.Random(seed)
    return [("".join(rng.choice(alphabet) for _ in range(rng.randint(0, max_t))),
             "".join(rng.choice(alphabet) for _ in range(rng.randint(0, max_q)))) for _ in range(n)]


def from_transcript(tr, t, q):
    from pbccs_amd import align as A
    return A.PairwiseAlignment.FromTranscript(tr, t, q)


def prefix_scores(t, q, params):
    """GLOBAL scores of every (t[:b], q[:d]): one Needleman-Wunsch matrix."""
    match, mismatch, ins, dele = params
    S = [[0] * (len(t) + 1) for _ in range(len(q) + 1)]
    for j in range(1, len(t) + 1):
        S[0][j] = j * dele
    for i in range(1, len(q) + 1):
        S[i][0] = i * ins
        for j in range(1, len(t) + 1):
            S[i][j] = max(S[i - 1][j - 1] + (match if q[i - 1] == t[j - 1] else mismatch), S[i][j - 1] + dele,
                          S[i - 1][j] + ins)
    return S


@pytest.mark.parametrize("alphabet", ("AC", "ACGT"))
@pytest.mark.parametrize("params", PARAM_SETS)
def test_restatement_against_brute_force(params, alphabet):
    for t, q in random_pairs(1000 * PARAM_SETS.index(params) + len(alphabet), 40, alphabet):
        # brute force: the GLOBAL score of every substring pair
        semi, local = None, 0
        for a in range(len(t) + 1):
            for c in range(len(q) + 1):
                S = prefix_scores(t[a:], q[c:], params)
                local = max(local, max(max(row) for row in S))
                if c == 0:
                    best = max(S[len(q)])
                    semi = best if semi is None else max(semi, best)
        for mode, want in ((R.SEMIGLOBAL, semi), (R.LOCAL, local)):
            tr, score, ext = R.align_ends(t, q, mode, params)
            (tb, te), (qb, qe) = ext["target"], ext["query"]
            where = (t, q, mode, params, tr, score, ext)
            assert score == want, where
            assert 0 <= tb <= te <= len(t) and 0 <= qb <= qe <= len(q), where
            assert score == R.global_score(t[tb:te], q[qb:qe], params), where
            assert from_transcript(tr, t[tb:te], q[qb:qe]) is not None, where
            if mode == R.SEMIGLOBAL:
                assert (qb, qe) == (0, len(q)), where


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("params", PARAM_SETS)
def test_numpy_form_equals_plain_form(params, mode):
    pairs = random_pairs(7, 60, "AC", 12, 12) + random_pairs(8, 60, "ACGTNa", 40, 30)
    pairs += [("A" * 9, "A" * 4), ("ACACACAC", "CACA"), ("", "ACG"), ("ACG", ""), ("", "")]
    for t, q in pairs:
        for both in (False, True):
            assert R.align_ends_np(t, q, mode, params, both) == R.align_ends(t, q, mode, params, both), (t, q, both)


def test_tie_rules_on_homopolymers():
    ed, poa = (0, -1, -1, -1), (3, -5, -4, -4)
    # SEMIGLOBAL ends at the smallest j that holds the row's maximum
    assert R.align_ends("AAAA", "AA", R.SEMIGLOBAL, ed) == ("MM", 0, {"target": (0, 2), "query": (0, 2), "rc": False})
    assert R.align_ends("AAAA", "AA", R.SEMIGLOBAL, poa) == ("MM", 6, {"target": (0, 2), "query": (0, 2), "rc": False})
    # LOCAL: the smallest j, then the smallest i
    assert R.align_ends("AAAA", "AA", R.LOCAL, poa) == ("MM", 6, {"target": (0, 2), "query": (0, 2), "rc": False})
    assert R.align_ends("AA", "AAAA", R.LOCAL, poa) == ("MM", 6, {"target": (0, 2), "query": (0, 2), "rc": False})
    # nothing positive: LOCAL stays at (0, 0); with edit distance every cell is <= 0
    assert R.align_ends("AAAA", "AA", R.LOCAL, ed) == ("", 0, {"target": (0, 0), "query": (0, 0), "rc": False})
    assert R.align_ends("CCCC", "AA", R.LOCAL, poa) == ("", 0, {"target": (0, 0), "query": (0, 0), "rc": False})
    # a query that matches nothing under a harsh Mismatch: all Extra in column 0, the end cell at j = 0
    assert R.align_ends("CCCC", "AA", R.SEMIGLOBAL, (0, -9, -1, -1)) == \
        ("II", -2, {"target": (0, 0), "query": (0, 2), "rc": False})
    # a tie in the last row goes to the smallest j even when that path is all Extra
    assert R.align_ends("CTTG", "CAG", R.SEMIGLOBAL, ed) == \
        ("MII", -2, {"target": (0, 1), "query": (0, 3), "rc": False})
    # the candidate order is diagonal, Delete, Extra (not Align's diagonal, up, left).  ACA on ACA, cell (2, 3):
    # diagonal S(1, 2) - 1 = -2, Delete S(2, 2) - 1 = -1, Extra S(1, 3) - 1 = -1: Delete, where ArgMax3 takes up
    S, mv = R.fill("ACA", "ACA", R.SEMIGLOBAL, ed)
    assert (S[1][2], S[2][2], S[1][3], S[2][3]) == (-1, 0, 0, -1) and mv[2][3] == R.DELETE
    # both strands: forward wins a tie
    assert R.align_ends("ACGT", "ACGT", R.LOCAL, poa, True)[2]["rc"] is False
    assert R.align_ends("AAAA", "TTT", R.LOCAL, poa, True) == \
        ("MMM", 9, {"target": (0, 3), "query": (0, 3), "rc": True})


class _NoEngine:
    def __getattr__(self, name):
        raise AssertionError("the engine was touched")


def test_refusals_before_any_engine():
    from pbccs_amd import align as A
    eng = _NoEngine()
    pairs = [("GATT", "GAT")]
    calls = [lambda **kw: A.align_ends_batch(pairs, kw.pop("mode"), engine=eng, **kw),
             lambda **kw: (A.AlignSemiglobal if kw.pop("mode") == A.SEMIGLOBAL else A.AlignLocal)(
                 "GATT", "GAT", engine=eng, **kw)]
    for call, mode in itertools.product(calls, (A.SEMIGLOBAL, A.LOCAL)):
        for bad in (A.AlignParams(0, -1, 1, -1), A.AlignParams(0, -1, -1, 1), A.AlignParams(0, -1, 2, 3)):
            with pytest.raises(A.InvalidInputError):
                call(mode=mode, params=bad)
        for kind in (A.AFFINE, A.AFFINE_IUPAC):
            with pytest.raises(A.UnsupportedFeatureError):
                call(mode=mode, kind=kind)
            with pytest.raises(A.UnsupportedFeatureError):
                call(mode=mode, kind=kind, params=A.DefaultAffineAlignmentParams())
        with pytest.raises(A.UnsupportedFeatureError):
            call(mode=mode, params=A.DefaultAffineAlignmentParams())
        for band in (True, 0, 16):
            with pytest.raises(A.UnsupportedFeatureError):
                call(mode=mode, band=band)
    with pytest.raises(A.InvalidInputError):
        A.align_ends_batch(pairs, A.GLOBAL, engine=eng)
    with pytest.raises(A.InvalidInputError):
        A.align_ends_batch(pairs, 7, engine=eng)
    # the reference's own entry goes on refusing the modes
    for mode in (A.SEMIGLOBAL, A.LOCAL):
        with pytest.raises(A.UnsupportedFeatureError):
            A.Align("GATT", "GAT", A.AlignConfig(A.AlignParams.Default(), mode), engine=eng)
    # the mapper's new option is off by default and validated the same way
    from pbccs_amd import mapping
    import inspect
    assert inspect.signature(mapping.map_batch).parameters["transcripts"].default is False
    assert inspect.signature(mapping.map_to_draft).parameters["transcripts"].default is False


def test_reverse_complement_is_the_mappers_table():
    from pbccs_amd import align as A
    assert A.reverse_complement("ACGTN") == "MACGT" == R.revcomp("ACGTN")
    assert A.reverse_complement("nmX-") == "-\x7fnm"
    assert A.reverse_complement(b"AC\x00") == b"\x03GT"
    for s in ("", "A", "GATTACA", "acgtNM-xyz"):
        assert A.reverse_complement(s) == R.revcomp(s)

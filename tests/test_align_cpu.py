"""Pairwise alignment, the host side: a restatement of ConsensusCore's Align (PairwiseAlignment.cpp:125-212) and
AlignAffineGeneric (AffineAlignment.cpp:110-209) that the GPU tests use as their oracle, checked here against the
reference's own known answers (tests/golden/align_kats.json, values parsed out of TestPairwiseAlignment.cpp by
tests/golden/make_align_golden.py), and the host-side value code of pbccs_amd.align and include/pbccs_amd/Align.hpp.

The restatement fills the reference's full matrices one anti-diagonal at a time (the cells of an anti-diagonal do not
depend on each other), every affine sum a single numpy.float32 add, and then walks the reference's traceback over
them, recomputing each decision from the matrices as the reference does."""
import functools
import json
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KATS = json.load(open(os.path.join(ROOT, "tests", "golden", "align_kats.json")))
SRC = os.path.join(ROOT, "tests", "cpp", "align_driver.cpp")
BIN = os.path.join(ROOT, "tests", "cpp", "_build", "align_driver")
LIBDIR = os.path.join(ROOT, "pbccs_amd", "_lib")

F32 = np.float32
NEG = F32(-np.finfo(np.float32).max)   # -FLT_MAX
NW_DEFAULT = (0, -1, -1, -1)
AFFINE_DEFAULT = (0.0, -1.0, -1.0, -0.5, 0.0)
IUPAC_DEFAULT = (0.0, -1.0, -1.0, -0.5, -0.25)


class WalkLeavesMatrix(Exception):
    """The reference would read outside its matrices here (a walk in M on row 0 or column 0, or a GAP move off it)."""


def transcript_of(aln_target, aln_query):
    return "".join("M" if t == q else "I" if t == "-" else "D" if q == "-" else "R" for t, q in zip(aln_target, aln_query))


@functools.lru_cache(maxsize=None)
def ref_align(target, query, params=NW_DEFAULT):
    """(aligned target, aligned query, Score(I, J)) of Align(target, query, &score, AlignConfig(params, GLOBAL))."""
    match, mismatch, insert, delete = params
    I, J = len(query), len(target)
    q = np.frombuffer(query.encode("latin-1"), dtype=np.uint8)
    t = np.frombuffer(target.encode("latin-1"), dtype=np.uint8)
    sub = np.where(q[:, None] == t[None, :], match, mismatch).astype(np.int64) if I and J else np.zeros((I, J), np.int64)
    S = np.zeros((I + 1, J + 1), dtype=np.int64)
    S[:, 0] = np.arange(I + 1) * insert
    S[0, :] = np.arange(J + 1) * delete
    for d in range(2, I + J + 1):
        ii = np.arange(max(1, d - J), min(I, d - 1) + 1)
        jj = d - ii
        S[ii, jj] = np.maximum(S[ii - 1, jj - 1] + sub[ii - 1, jj - 1],
                               np.maximum(S[ii - 1, jj] + insert, S[ii, jj - 1] + delete))
    ra_q, ra_t = [], []
    i, j = I, J
    while i > 0 or j > 0:
        if i == 0:
            move = 2
        elif j == 0:
            move = 1
        else:
            a = int(S[i - 1, j - 1]) + (match if query[i - 1] == target[j - 1] else mismatch)
            b = int(S[i - 1, j]) + insert
            c = int(S[i, j - 1]) + delete
            move = 0 if (a >= b and a >= c) else (1 if b >= c else 2)   # ArgMax3
        if move == 0:
            i -= 1
            j -= 1
            ra_q.append(query[i])
            ra_t.append(target[j])
        elif move == 1:
            i -= 1
            ra_q.append(query[i])
            ra_t.append("-")
        else:
            j -= 1
            ra_q.append("-")
            ra_t.append(target[j])
    return "".join(reversed(ra_t)), "".join(reversed(ra_q)), int(S[I, J])


def is_iupac_partial_match(code, b):   # AffineAlignment.cpp:65-78
    return {"R": "AG", "Y": "CT", "S": "GC", "W": "AT", "K": "GT", "M": "AC"}.get(code, "").find(b) >= 0


def match_score(t, q, p, iupac):
    if t == q:
        return p[0]
    if iupac and (is_iupac_partial_match(t, q) or is_iupac_partial_match(q, t)):
        return p[4]
    return p[1]


def smax(a, b):   # std::max on arrays: a unless a < b
    return np.where(a < b, b, a)


@functools.lru_cache(maxsize=None)
def ref_affine(target, query, params=AFFINE_DEFAULT, iupac=False):
    """(aligned target, aligned query, max(M, GAP)(I, J) as numpy.float32) of AlignAffine / AlignAffineIupac."""
    p = tuple(F32(x) for x in params)
    open_, ext = p[2], p[3]
    I, J = len(query), len(target)
    table = np.zeros((256, 256), dtype=F32)   # MatchScore<C>(t, q) of every pair of bytes that occurs
    for a in set(target):
        for b in set(query):
            table[ord(a), ord(b)] = match_score(a, b, p, iupac)
    tb = np.frombuffer(target.encode("latin-1"), dtype=np.uint8)
    qb = np.frombuffer(query.encode("latin-1"), dtype=np.uint8)
    sub = table[tb[None, :], qb[:, None]] if I and J else np.zeros((I, J), dtype=F32)
    with np.errstate(over="ignore", invalid="ignore"):
        M = np.full((I + 1, J + 1), NEG, dtype=F32)
        G = np.full((I + 1, J + 1), NEG, dtype=F32)
        M[0, 0] = 0
        if I:
            G[1:, 0] = open_ + np.arange(I, dtype=F32) * ext
        if J:
            G[0, 1:] = open_ + np.arange(J, dtype=F32) * ext
        for d in range(2, I + J + 1):
            ii = np.arange(max(1, d - J), min(I, d - 1) + 1)
            jj = d - ii
            M[ii, jj] = smax(M[ii - 1, jj - 1], G[ii - 1, jj - 1]) + sub[ii - 1, jj - 1]
            G[ii, jj] = smax(smax(M[ii, jj - 1] + open_, G[ii, jj - 1] + ext),
                             smax(M[ii - 1, jj] + open_, G[ii - 1, jj] + ext))
        assert M.dtype == F32 and G.dtype == F32
        ra_q, ra_t = [], []
        i, j = I, J
        in_m = bool(M[I, J] >= G[I, J])
        while i > 0 or j > 0:
            if in_m:
                if i == 0 or j == 0:
                    raise WalkLeavesMatrix()
                prev_m = bool(M[i - 1, j - 1] >= G[i - 1, j - 1])
                i, j = i - 1, j - 1
                ra_q.append(query[i])
                ra_t.append(target[j])
            else:
                s = [M[i, j - 1] + open_ if j > 0 else NEG, G[i, j - 1] + ext if j > 0 else NEG,
                     M[i - 1, j] + open_ if i > 0 else NEG, G[i - 1, j] + ext if i > 0 else NEG]
                arg = 0
                for k in range(1, 4):   # std::max_element: the first maximum
                    if s[arg] < s[k]:
                        arg = k
                prev_m = arg in (0, 2)
                if arg < 2:
                    if j == 0:
                        raise WalkLeavesMatrix()
                    j -= 1
                    ra_q.append("-")
                    ra_t.append(target[j])
                else:
                    if i == 0:
                        raise WalkLeavesMatrix()
                    i -= 1
                    ra_q.append(query[i])
                    ra_t.append("-")
            in_m = prev_m
        score = M[I, J] if M[I, J] >= G[I, J] else G[I, J]
    return "".join(reversed(ra_t)), "".join(reversed(ra_q)), F32(score)


def ref(kind, target, query, params=None):
    """Oracle by kind (0 NW, 1 affine, 2 IUPAC-aware affine): (transcript, score)."""
    if kind == 0:
        t, q, s = ref_align(target, query, tuple(params) if params else NW_DEFAULT)
    else:
        t, q, s = ref_affine(target, query, tuple(params) if params else (AFFINE_DEFAULT if kind == 1 else IUPAC_DEFAULT),
                             kind == 2)
    return transcript_of(t, q), s


def _expect(got_target, got_query, case):
    e = case["expect"]
    if "Target" in e:
        assert got_target == e["Target"]
    if "Query" in e:
        assert got_query == e["Query"]
    if "Transcript" in e:
        assert transcript_of(got_target, got_query) == e["Transcript"]
    if "Accuracy" in e:
        tr = transcript_of(got_target, got_query)
        assert tr.count("M") / len(tr) == pytest.approx(e["Accuracy"], rel=1e-6)   # EXPECT_FLOAT_EQ


# ---- 1. the restatement reproduces the reference's known answers ------------------------------------------
def test_restatement_align_known_answers():
    assert len(KATS["align"]) == 3
    for c in KATS["align"]:
        t, q, _ = ref_align(c["target"], c["query"])
        _expect(t, q, c)


def test_restatement_affine_known_answers():
    assert len(KATS["affine"]) == 7 and len(KATS["iupac"]) == 2
    for c in KATS["affine"]:
        t, q, _ = ref_affine(c["target"], c["query"])
        _expect(t, q, c)
    for c in KATS["iupac"]:
        t, q, _ = ref_affine(c["target"], c["query"], IUPAC_DEFAULT, True)
        _expect(t, q, c)


def test_restatement_large_gap():
    c = KATS["affine_large_gap"]
    assert (len(c["target"]), len(c["query"])) == (1010, 1191)
    t, q, s = ref_affine(c["target"], c["query"])
    _expect(t, q, c)
    assert q == c["query"] and float(s) == -91.0


def test_restatement_align_peer_score():
    c = KATS["align_peer"]
    assert c["params"] == [2, -1, -2, -2]
    assert ref_align(c["target"], c["query"], tuple(c["params"]))[2] == 134


def test_restatement_rounds_every_add_to_float32():
    # 0.1f + 0.2f differs from float32(0.1 + 0.2): a restatement in doubles would score this pair differently
    p = (0.1, -1.1, -2.7, -0.4, -0.6)
    _, _, s = ref_affine("ACGTACGTAC", "ACGTACGTAC", p)
    acc = F32(0)
    for _ in range(10):
        acc = F32(acc + F32(0.1))
    assert s.dtype == F32 and float(s).hex() == float(acc).hex()
    assert float(acc) != float(F32(10 * 0.1))


def test_restatement_degenerate_inputs():
    assert ref(0, "", "") == ("", 0)
    assert ref(0, "ACG", "") == ("DDD", -3)
    assert ref(0, "", "AC") == ("II", -2)
    assert ref(1, "ACG", "") == ("DDD", F32(-2.0))
    assert ref(1, "", "AC") == ("II", F32(-1.5))
    assert ref(2, "", "") == ("", F32(0))


# ---- 2. the host-side value code of pbccs_amd.align --------------------------------------------------------
def test_pairwise_alignment_representation():
    from pbccs_amd.align import PairwiseAlignment
    assert len(KATS["representation"]) == 2
    for c in KATS["representation"]:
        a = PairwiseAlignment(c["target"], c["query"])
        for name, want in c["expect"].items():
            got = getattr(a, name)()
            assert got == (pytest.approx(want, rel=1e-6) if name == "Accuracy" else want), name
        assert a.Errors() == a.Length() - a.Matches()


def test_pairwise_alignment_refusals():
    from pbccs_amd.align import InvalidInputError, PairwiseAlignment
    with pytest.raises(InvalidInputError):
        PairwiseAlignment("GATC", "GAC")
    with pytest.raises(InvalidInputError):
        PairwiseAlignment("GA-C", "GA-C")


def test_target_to_query_positions():
    from pbccs_amd.align import InvalidInputError, PairwiseAlignment, TargetToQueryPositions
    assert len(KATS["target_to_query_positions"]) == 10
    for c in KATS["target_to_query_positions"]:
        assert TargetToQueryPositions(c["transcript"]) == c["expected"]
    assert TargetToQueryPositions(PairwiseAlignment("GATTA-CA", "CA-TAACA")) == [0, 1, 2, 2, 3, 5, 6, 7]
    with pytest.raises(InvalidInputError):
        TargetToQueryPositions("MXM")


def test_from_transcript():
    from pbccs_amd.align import PairwiseAlignment
    a = PairwiseAlignment.FromTranscript("RMDMMIMM", "GATTACA", "CATAACA")
    assert (a.Target(), a.Query(), a.Transcript()) == ("GATTA-CA", "CA-TAACA", "RMDMMIMM")
    for c in KATS["align"] + KATS["affine"] + KATS["iupac"]:
        e = c["expect"]
        if "Target" in e and "Query" in e:
            a = PairwiseAlignment.FromTranscript(transcript_of(e["Target"], e["Query"]), c["target"], c["query"])
            assert (a.Target(), a.Query()) == (e["Target"], e["Query"])
    assert PairwiseAlignment.FromTranscript("", "", "").Length() == 0
    # transcripts that do not map the target onto the query: the reference's NULL
    assert PairwiseAlignment.FromTranscript("MMMM", "GATT", "GAT") is None    # runs past the query
    assert PairwiseAlignment.FromTranscript("MMM", "GATT", "GAT") is None     # leaves target unconsumed
    assert PairwiseAlignment.FromTranscript("MMRM", "GATT", "GATT") is None   # R over equal characters
    assert PairwiseAlignment.FromTranscript("MMMM", "GATT", "GACT") is None   # M over unequal characters
    assert PairwiseAlignment.FromTranscript("MMXM", "GATT", "GATT") is None   # not a transcript character
    assert PairwiseAlignment.FromTranscript("MMMMD", "GATT", "GATT") is None
    assert PairwiseAlignment.FromTranscript("IMMMM", "GATT", "GATT") is None


def test_batch_path_reconstruction_equals_from_transcript():
    """align_batch rebuilds the gapped strings column-wise; it must agree with FromTranscript, refusals included."""
    import random
    from pbccs_amd.align import PairwiseAlignment, _from_device_transcript
    rng = random.Random(12)
    cases = [("RMDMMIMM", "GATTACA", "CATAACA"), ("", "", ""), ("DDD", "ACG", ""), ("II", "", "AC"),
             ("MMMM", "GATT", "GAT"), ("MMM", "GATT", "GAT"), ("MMRM", "GATT", "GATT"), ("MMMM", "GATT", "GACT"),
             ("MMXM", "GATT", "GATT"), ("MMMMD", "GATT", "GATT"), ("IMMMM", "GATT", "GATT")]
    for _ in range(200):
        t = "".join(rng.choice("ACGT") for _ in range(rng.randint(0, 12)))
        q = "".join(rng.choice("ACGT") for _ in range(rng.randint(0, 12)))
        at, aq, _ = ref_align(t, q)
        tr = list(transcript_of(at, aq))
        if tr and rng.random() < 0.5:   # spoil half of them
            tr[rng.randrange(len(tr))] = rng.choice("MRID")
        cases.append(("".join(tr), t, q))
    n_none = 0
    for tr, t, q in cases:
        a, b = PairwiseAlignment.FromTranscript(tr, t, q), _from_device_transcript(tr, t, q)
        assert (a is None) == (b is None), (tr, t, q)
        n_none += a is None
        if a is not None:
            assert (a.Target(), a.Query(), a.Transcript()) == (b.Target(), b.Query(), b.Transcript())
    assert 20 < n_none < len(cases) - 20


# ---- 3. refusals come before any engine is touched ----------------------------------------------------------
class _NoEngine:
    def __getattr__(self, name):
        raise AssertionError("the engine was touched")


def test_refusals_before_the_engine():
    import pbccs_amd as P
    from pbccs_amd import align as A
    for mode in (A.SEMIGLOBAL, A.LOCAL):
        with pytest.raises(P.UnsupportedFeatureError):
            P.Align("GATT", "GAT", P.AlignConfig(P.AlignParams.Default(), mode), engine=_NoEngine())
    for k in range(5):
        for bad in (float("nan"), float("inf"), float("-inf")):
            v = list(AFFINE_DEFAULT)
            v[k] = bad
            with pytest.raises(A.InvalidInputError):
                P.AlignAffine("GATT", "GAT", P.AffineAlignmentParams(*v), engine=_NoEngine())
            with pytest.raises(A.InvalidInputError):
                P.AlignAffineIupac("GATT", "GAT", P.AffineAlignmentParams(*v), engine=_NoEngine())
            with pytest.raises(A.InvalidInputError):
                P.align_batch([("GATT", "GAT")], A.AFFINE, P.AffineAlignmentParams(*v), engine=_NoEngine())
    d, u = P.DefaultAffineAlignmentParams(), P.IupacAwareAffineAlignmentParams()
    assert d._values() == AFFINE_DEFAULT and u._values() == IUPAC_DEFAULT
    c = P.AlignConfig.Default()
    assert (c.Params.Match, c.Params.Mismatch, c.Params.Insert, c.Params.Delete, c.Mode) == NW_DEFAULT + (A.GLOBAL,)


# ---- 4. the C++ facade's host-only parts ---------------------------------------------------------------------
def build_driver():
    os.makedirs(os.path.dirname(BIN), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-I" + os.path.join(ROOT, "include"), SRC, "-L" + LIBDIR,
                           "-lpbccs_amd", "-Wl,-rpath," + LIBDIR, "-o", BIN])
    return BIN


def test_align_facade_driver_compiles_links_and_knows_the_answers():
    out = subprocess.run([build_driver()], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.split("\n")[0] == "known answers ok"

"""Diploid site calling, host side: pbccs_is_site_heterozygous (the float restatement of ConsensusCore's
Arrow/Diploid.cpp:110-239 behind pbccs_amd.diploid.IsSiteHeterozygous) against a numpy restatement of the same
file, on site tensors made by the CPU oracle's per-read Scores() for seeded heterozygous ZMWs, plus analytic known
answers and the refusals.  This module also holds the input recipe and the comparison the GPU tests share.

Tolerance: T = 4 x max |logBF_f32 - logBF_f64| over the case's sites, measured from the numpy restatement alone
(the float32-against-float64 gap is of the order of the libm differences between glibc's and numpy's float
functions, an ulp per call; the factor 4 covers them).  A site whose logBF lies within T of the prior, or whose best
two pair totals lie within T, may be left out of the discrete comparison -- at most one per (case, prior)."""
import ctypes
import functools
import math

import numpy as np
import pytest

from oracle import oracle as O
from pbccs_amd import synth

INS, DEL, SUB = 0, 1, 2
LENGTH_DIFFS = (0, 0, 0, 0, 1, 1, 1, 1, -1)   # Diploid.cpp:99
PAIRS = [(g0, g1) for g0 in range(9) for g1 in range(g0 + 1, 9) if LENGTH_DIFFS[g0] == LENGTH_DIFFS[g1]]
ARROW_SNR = (10.0, 7.0, 5.0, 11.0)
ARROW_ERRORS = (0.07, 0.04, 0.01)
CASES = [(7, 60, 8, (20, 41)), (9, 120, 10, (30, 90))]
FAMILIES = ("arrow", "quiver")
PRIORS = (0.0, 5.0)


# ---- the shared input recipe ---------------------------------------------------------------------------------
def het_case(seed, L, P, het_positions, errors):
    """A ZMW whose reads come from two haplotypes: `truth`, and `alt` = truth with each planted base moved to the
    next of ACGT.  Read k is drawn from truth when (k // 2) % 2 == 0, else from alt; strand k % 2."""
    rng = np.random.Generator(np.random.PCG64(seed))
    truth = synth.BASES[rng.integers(0, 4, size=L)]
    alt = truth.copy()
    for p in het_positions:
        alt[p] = synth.BASES[(int(np.searchsorted(synth.BASES, truth[p])) + 1) % 4]
    reads = []
    for k in range(P):
        src = truth if (k // 2) % 2 == 0 else alt
        r = synth._mutate(rng, src, *errors)
        strand = k % 2
        if strand == 1:
            r = synth.COMP[r[::-1]]
        reads.append({"seq": r.tobytes().decode(), "strand": strand, "ts": 0, "te": L})
    return truth.tobytes().decode(), reads


def arrow_case(seed, L, P, het):
    return het_case(seed, L, P, het, ARROW_ERRORS)


def quiver_case(seed, L, P, het):
    from tests.test_quiver_gpu import _features
    tpl, reads = het_case(seed, L, P, het, synth.QUIVER_READ_ERRORS)
    rng = np.random.default_rng(seed)
    return tpl, [dict(r, features=_features(rng, r["seq"])) for r in reads]


def make_case(family, case):
    return arrow_case(*case) if family == "arrow" else quiver_case(*case)


def oracle_scorer(family, tpl, reads):
    if family == "arrow":
        o = O.Scorer(tpl, ARROW_SNR)
        for r in reads:
            o.add_read(r["seq"], r["strand"], r["ts"], r["te"])
        return o
    from tests.test_quiver_gpu import PARAMS2
    o = O.QuiverScorer(tpl, PARAMS2)
    for r in reads:
        o.add_read(r["seq"], r["strand"], r["ts"], r["te"], r["features"])
    return o


def oracle_site_tensor(o, tpl, n_reads, dtype=np.float32):
    """[site][read][9] from the oracle's per-read Scores(m, 0): Substitution(p, ACGT) with the template base's own
    column 0 and not scored, Insertion(p, ACGT), Deletion(p)."""
    t = np.zeros((len(tpl), n_reads, 9), dtype=np.float64)
    for p in range(len(tpl)):
        for c, b in enumerate("ACGT"):
            if b != tpl[p]:
                t[p, :, c] = o.scores(SUB, p, b, 0.0)
            t[p, :, 4 + c] = o.scores(INS, p, b, 0.0)
        t[p, :, 8] = o.scores(DEL, p, "-", 0.0)
    return t.astype(dtype)


@functools.lru_cache(maxsize=None)
def oracle_case(family, case):
    """(template, reads, oracle float64 tensor) of a case, made once and shared (do not modify)."""
    tpl, reads = make_case(family, case)
    o = oracle_scorer(family, tpl, reads)
    t = oracle_site_tensor(o, tpl, len(reads), np.float64)
    t.setflags(write=False)
    return tpl, reads, t


# ---- Diploid.cpp in numpy, generic over dtype, the reference's operation order --------------------------------
def _logaddexp(x, y):   # :110-118
    diff = x - y
    if diff > 0:
        return x + np.log1p(np.exp(-diff))
    return y + np.log1p(np.exp(diff))


def restate_site(m, prior, dtype=np.float32):
    """IsSiteHeterozygous (:219-239) -> dict(is_het, a0, a1, logbf, afr, best, second)."""
    m = np.asarray(m, dtype=dtype)
    n_reads = m.shape[0]
    flt_max = dtype(np.finfo(np.float32).max)
    with np.errstate(all="ignore"):
        hom = -flt_max
        for g in range(9):
            s = dtype(0)
            for i in range(n_reads):
                s = s + m[i, g]
            hom = _logaddexp(hom, s)
        log2 = dtype(math.log(2.0))
        totals = []
        best, second, a0, a1 = -flt_max, -flt_max, -1, -1
        for g0, g1 in PAIRS:
            total = dtype(-n_reads) * log2
            for i in range(n_reads):
                total = total + _logaddexp(m[i, g0], m[i, g1])
            totals.append(total)
            if total > best:
                second, best, a0, a1 = best, total, g0, g1
            elif total > second:
                second = total
        het = -flt_max
        for t in totals:
            het = _logaddexp(het, t)
        logbf = het - hom
        is_het = bool(logbf - dtype(prior) > 0)
    afr = [0 if m[i, a0] > m[i, a1] else 1 for i in range(n_reads)]
    return dict(is_het=is_het, a0=a0, a1=a1, logbf=logbf, afr=afr, best=best, second=second)


@functools.lru_cache(maxsize=None)
def _restated(shape, data):
    tensor = np.frombuffer(data, dtype=np.float32).reshape(shape)
    r32 = [restate_site(tensor[s], 0.0, np.float32) for s in range(shape[0])]
    r64 = [restate_site(tensor[s], 0.0, np.float64) for s in range(shape[0])]
    return r32, r64


def restate_tensor(tensor):
    """(float32 restatement per site at prior 0, the float64 one, T) of a float32 tensor; computed once per tensor."""
    r32, r64 = _restated(tensor.shape, np.ascontiguousarray(tensor, dtype=np.float32).tobytes())
    tol = 4.0 * max(abs(float(a["logbf"]) - float(b["logbf"])) for a, b in zip(r32, r64))
    return r32, r64, tol


def check_sites(got, tensor, prior, planted=None, first_site=0):
    """got: {site index within tensor: (allele0, allele1, logBF, AlleleForRead)} of the sites reported at `prior`,
    against the float32 numpy restatement of every site of `tensor`.  Prints the figures, then asserts."""
    r32, r64, tol = restate_tensor(tensor)
    left_out = []
    n_ref = 0
    for s, ref in enumerate(r32):
        lb = float(ref["logbf"])
        ref_het = bool(np.float32(lb) - np.float32(prior) > 0)
        n_ref += ref_het
        near_prior = abs(lb - prior) <= tol
        tie = abs(float(ref["best"]) - float(ref["second"])) <= tol
        if (s in got) != ref_het:
            assert near_prior, (first_site + s, lb, prior, tol, s in got)
            left_out.append(first_site + s)
            continue
        if not ref_het:
            continue
        a0, a1, g_lb, afr = got[s]
        assert abs(float(g_lb) - lb) <= tol, (first_site + s, g_lb, lb, tol)
        if (a0, a1, list(afr)) != (ref["a0"], ref["a1"], ref["afr"]):
            assert near_prior or tie, (first_site + s, (a0, a1, list(afr)), ref)
            left_out.append(first_site + s)
    print(f"prior {prior}: reported {len(got)} of {len(r32)} sites (restatement {n_ref}), T = {tol:.3g}, "
          f"left out {left_out}")
    assert len(left_out) <= 1, left_out
    if planted is not None:
        assert set(planted) <= {first_site + s for s in got}, (planted, sorted(got))
    return tol


# ---- 1. the host primitive against the restatement -------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=lambda c: f"seed{c[0]}")
@pytest.mark.parametrize("family", FAMILIES)
def test_host_primitive_matches_restatement(family, case):
    from pbccs_amd.diploid import IsSiteHeterozygous
    tpl, reads, t64 = oracle_case(family, case)
    tensor = t64.astype(np.float32)
    assert tensor.shape == (case[1], case[2], 9)
    for prior in PRIORS:
        got = {}
        for s in range(tensor.shape[0]):
            d = IsSiteHeterozygous(tensor[s], prior)
            if d is not None:
                assert d.Position is None
                got[s] = (d.Allele0, d.Allele1, d.LogBayesFactor, d.AlleleForRead)
        check_sites(got, tensor, prior, planted=case[3] if prior == 0.0 else None)


# ---- 2. analytic known answers ---------------------------------------------------------------------------------
def test_all_zero_matrix():
    from pbccs_amd.diploid import IsSiteHeterozygous
    m = np.zeros((8, 9), dtype=np.float32)
    d = IsSiteHeterozygous(m, 0.0)
    # every pair total is 8 (ln 2 - ln 2) = 0 and every column sum 0: logBF = ln 12 - ln 9
    assert d is not None and abs(d.LogBayesFactor - math.log(12.0 / 9.0)) <= 1e-5
    assert (d.Allele0, d.Allele1) == (0, 1) and d.AlleleForRead == [1] * 8
    assert IsSiteHeterozygous(m, 1.0) is None


def test_two_clean_alleles():
    from pbccs_amd.diploid import IsSiteHeterozygous
    m = np.full((8, 9), -50.0, dtype=np.float32)
    m[:, 0:2] = 0.0
    m[1::2, 0] = -20.0
    m[0::2, 1] = -20.0
    d = IsSiteHeterozygous(m, 0.0)
    # pair (0, 1) totals 8 (0 - ln 2) and dominates; columns 0 and 1 sum to -80 each: logBF = 80 - 9 ln 2
    assert d is not None and abs(d.LogBayesFactor - (80.0 - 9.0 * math.log(2.0))) <= 1e-4
    assert (d.Allele0, d.Allele1) == (0, 1) and d.AlleleForRead == [0, 1] * 4


# ---- 3. refusals -----------------------------------------------------------------------------------------------
def test_refusals():
    from pbccs_amd import lib
    L = lib.load()
    m = np.zeros((8, 9), dtype=np.float32)
    p = m.ctypes.data_as(lib.PF)
    het, site, afr = ctypes.c_int(), lib.CDiploidSite(), (ctypes.c_int * 8)()
    call = L.pbccs_is_site_heterozygous
    assert call(p, 8, 9, 0.0, ctypes.byref(het), ctypes.byref(site), afr) == 0
    assert call(p, 9, 8, 0.0, ctypes.byref(het), ctypes.byref(site), afr) == -1   # n_alleles = 8
    assert call(p, 0, 9, 0.0, ctypes.byref(het), ctypes.byref(site), afr) == -1   # n_reads = 0
    assert call(None, 8, 9, 0.0, ctypes.byref(het), ctypes.byref(site), afr) == -1
    assert call(p, 8, 9, 0.0, None, ctypes.byref(site), afr) == -1
    assert call(p, 8, 9, 0.0, ctypes.byref(het), None, afr) == -1
    assert call(p, 8, 9, 0.0, ctypes.byref(het), ctypes.byref(site), None) == -1
    with pytest.raises(lib.PbccsError):
        from pbccs_amd.diploid import IsSiteHeterozygous
        IsSiteHeterozygous(np.zeros((8, 8), dtype=np.float32), 0.0)

"""Diploid site calling on the GPU: the site tensor (k_site_scores over the scorers' scoring rounds) against the CPU
oracle's per-read Scores(), and DiploidSites (k_diploid's screen, then the host primitive on the marked sites)
against the numpy restatement of Diploid.cpp on the tensor SiteScores returned.  Inputs, restatement, tolerance T and
the leave-out rule are tests/test_diploid_cpu.py's.

Site tensor: the Quiver family is bit-exact FP32; Arrow's doubles agree with the oracle's within the project's 1e-9
(relative and absolute) before they are rounded, so each float lies within one float32 spacing of float32(oracle).
Cells that are 0 by construction -- the template base's own column, inactive reads, reads that do not score a
mutation -- are exactly 0."""
import ctypes
import functools

import numpy as np
import pytest

from tests.test_diploid_cpu import (ARROW_SNR, CASES, FAMILIES, PRIORS, SUB, check_sites, make_case, oracle_case,
                                    oracle_scorer, oracle_site_tensor)

pytestmark = pytest.mark.gpu

CASE_IDS = [f"seed{c[0]}" for c in CASES]


def revcomp(s):
    return s[::-1].translate(str.maketrans("ACGT", "TGCA"))


def gpu_scorer(family, tpl, reads):
    import pbccs_amd as P
    if family == "arrow":
        s = P.ArrowMultiReadMutationScorer(P.ArrowConfig(ARROW_SNR), tpl)
        for r in reads:
            s.AddRead(r["seq"], r["strand"], r["ts"], r["te"])
        return s
    from tests.test_quiver_gpu import PARAMS2, GpuQuiver
    g = GpuQuiver(tpl, PARAMS2)
    for r in reads:
        g.add_read(r["seq"], r["strand"], r["ts"], r["te"], r["features"])
    return g.s


@functools.lru_cache(maxsize=None)
def gpu_case(family, case):
    """(scorer, its full site tensor) of a case, made once and shared (do not modify either)."""
    tpl, reads, _ = oracle_case(family, case)
    s = gpu_scorer(family, tpl, reads)
    t = s.SiteScores()
    t.setflags(write=False)
    return s, t


def structural_zeros(family, tpl, infos):
    """Mask of the cells that are 0 by construction, from ReadScoresMutation (Arrow MultiReadMutationScorer.cpp:70-80,
    Quiver MultiReadMutationScorer.cpp:60-71) and the reads' active flags."""
    z = np.zeros((len(tpl), len(infos), 9), dtype=bool)
    for p in range(len(tpl)):
        z[p, :, "ACGT".index(tpl[p])] = True
        for k, ri in enumerate(infos):
            ts, te = ri["template_start"], ri["template_end"]
            ins = (ts <= p <= te) if family == "arrow" else (ts < p <= te)
            other = ts < p + 1 and p < te
            if not ri["active"]:
                z[p, k, :] = True
            if not ins:
                z[p, k, 4:8] = True
            if not other:
                z[p, k, 0:4] = True
                z[p, k, 8] = True
    return z


def assert_tensor_matches(family, got, t64, tpl, s):
    assert got.dtype == np.float32 and got.shape == t64.shape
    exp = t64.astype(np.float32)
    zeros = structural_zeros(family, tpl, [s.ReadInfo(k) for k in range(s.NumReads())])
    assert not got[zeros].any()
    assert zeros.sum() >= len(tpl) * s.NumReads()
    if family == "quiver":
        assert np.array_equal(got.view(np.uint32), exp.view(np.uint32))
    else:
        err = np.abs(got.astype(np.float64) - exp.astype(np.float64))
        print("max |site score - float32(oracle)| in float32 spacings:", float((err / np.spacing(np.abs(exp))).max()))
        assert (err <= np.spacing(np.abs(exp))).all()
        assert (np.abs(got - t64) <= 1e-9 + 1e-9 * np.abs(t64) + np.spacing(np.abs(exp))).all()


# ---- 1. SiteScores against the oracle --------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
@pytest.mark.parametrize("family", FAMILIES)
def test_site_scores_match_oracle(family, case):
    tpl, reads, t64 = oracle_case(family, case)
    s, got = gpu_case(family, case)
    assert [s.ReadInfo(k)["active"] for k in range(len(reads))].count(False) >= (1 if family == "quiver" else 0)
    assert_tensor_matches(family, got, t64, tpl, s)


@pytest.mark.parametrize("family", FAMILIES)
def test_site_scores_partial_window_reads(family):
    """The seed-9 case plus two partial-window reads: template[10:50] forward and template[30:75] reverse."""
    tpl, reads = make_case(family, CASES[1])
    reads = list(reads)
    rng = np.random.default_rng(CASES[1][0] + 1000)
    for seq, strand, ts, te in ((tpl[10:50], 0, 10, 50), (revcomp(tpl[30:75]), 1, 30, 75)):
        r = {"seq": seq, "strand": strand, "ts": ts, "te": te}
        if family == "quiver":
            from tests.test_quiver_gpu import _features
            r["features"] = _features(rng, seq)
        reads.append(r)
    o = oracle_scorer(family, tpl, reads)
    t64 = oracle_site_tensor(o, tpl, len(reads), np.float64)
    s = gpu_scorer(family, tpl, reads)
    assert s.ReadInfo(len(reads) - 1)["active"] and s.ReadInfo(len(reads) - 2)["active"]
    assert_tensor_matches(family, s.SiteScores(), t64, tpl, s)
    assert np.array_equal(s.SiteScores(28, 52), s.SiteScores()[28:52])


# ---- 2. DiploidSites against the restatement on the returned tensor --------------------------------------------
def _as_got(sites, first=0):
    return {d.Position - first: (d.Allele0, d.Allele1, d.LogBayesFactor, d.AlleleForRead) for d in sites}


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
@pytest.mark.parametrize("family", FAMILIES)
def test_diploid_sites_match_restatement(family, case):
    s, tensor = gpu_case(family, case)
    for prior in PRIORS:
        sites = s.DiploidSites(prior)
        assert [d.Position for d in sites] == sorted(d.Position for d in sites)
        check_sites(_as_got(sites), tensor, prior, planted=case[3] if prior == 0.0 else None)
        sub = s.DiploidSites(prior, 17, 45)
        assert sub == [d for d in sites if 17 <= d.Position < 45]
    assert len(s.DiploidSites(0.0, 17, 45)) > 0


# ---- 3. the screen loses nothing -------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
@pytest.mark.parametrize("family", FAMILIES)
def test_screen_equals_host_all(family, case):
    s, _ = gpu_case(family, case)
    eng = s.engine if family == "arrow" else s._eng
    n_sites = case[1]
    for prior in PRIORS:
        eng.diploid_stats(reset=True)
        screened = s.DiploidSites(prior)
        st = eng.diploid_stats(reset=True)
        print(f"prior {prior}: {st}")
        assert st["sites_screened"] == n_sites and st["sites_reported"] == len(screened)
        assert st["sites_reported"] <= st["sites_sent_to_host"] <= n_sites // 2
        everything = s.DiploidSites(prior, host_all=True)
        st = eng.diploid_stats(reset=True)
        assert st["sites_sent_to_host"] == st["sites_screened"] == n_sites
        assert [float(d.LogBayesFactor).hex() for d in screened] == [float(d.LogBayesFactor).hex() for d in everything]
        assert screened == everything


@pytest.mark.parametrize("family", FAMILIES)
def test_screen_sends_boundary_sites_to_the_host(family):
    """A prior equal to a site's own logBF: the host's test logBF - prior > 0 fails there, the screen cannot know
    that (the site lies within its bound) and must leave it to the host; both paths then agree."""
    s, tensor = gpu_case(family, CASES[0])
    eng = s.engine if family == "arrow" else s._eng
    first = s.DiploidSites(0.0)[0]
    prior = float(np.float32(first.LogBayesFactor))
    eng.diploid_stats(reset=True)
    screened = s.DiploidSites(prior)
    st = eng.diploid_stats(reset=True)
    assert first.Position not in [d.Position for d in screened]
    assert st["sites_sent_to_host"] >= st["sites_reported"] + 1
    assert screened == s.DiploidSites(prior, host_all=True)
    assert screened == [d for d in s.DiploidSites(0.0) if np.float32(d.LogBayesFactor) - np.float32(prior) > 0]


@pytest.mark.parametrize("family", FAMILIES)
def test_site_scores_in_several_rounds(family, monkeypatch):
    """The site range is scored in rounds of a fixed number of sites; with 7 sites per round (no divisor of the
    template length) the tensor and the reported sites are the ones a single round gives."""
    s, tensor = gpu_case(family, CASES[0])
    whole = s.DiploidSites(0.0)
    monkeypatch.setenv("PBCCS_SITE_CHUNK", "7")
    assert np.array_equal(s.SiteScores().view(np.uint32), tensor.view(np.uint32))
    assert np.array_equal(s.SiteScores(3, 31).view(np.uint32), tensor[3:31].view(np.uint32))
    assert s.DiploidSites(0.0) == whole


# ---- 4. after ApplyMutations -----------------------------------------------------------------------------------
@pytest.mark.parametrize("family", FAMILIES)
def test_site_scores_after_apply_mutations(family):
    import pbccs_amd as P
    tpl, reads = make_case(family, CASES[0])
    o = oracle_scorer(family, tpl, reads)
    s = gpu_scorer(family, tpl, reads)
    p = CASES[0][3][0]
    b = "ACGT"[("ACGT".index(tpl[p]) + 1) % 4]
    o.apply([(SUB, p, b)])
    s.ApplyMutations([P.Mutation(SUB, p, b)])
    new = tpl[:p] + b + tpl[p + 1:]
    assert s.Template() == new
    assert_tensor_matches(family, s.SiteScores(), oracle_site_tensor(o, new, len(reads), np.float64), new, s)


# ---- 5. refusals -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", FAMILIES)
def test_refusals_leave_the_scorer_usable(family):
    import pbccs_amd as P
    from pbccs_amd import diploid, lib
    tpl, reads = make_case(family, CASES[0])
    s = gpu_scorer(family, tpl, reads)
    m = P.Mutation(SUB, 5, "ACGT"[("ACGT".index(tpl[5]) + 1) % 4])
    before = (s.BaselineScore(), s.Score(m))
    L = lib.load()
    sites_fn = L.pbccs_scorer_diploid_sites if family == "arrow" else L.pbccs_quiver_scorer_diploid_sites
    scores_fn = L.pbccs_scorer_site_scores if family == "arrow" else L.pbccs_quiver_scorer_site_scores
    n_reads = s.NumReads()
    for begin, end in ((-1, 10), (0, len(tpl) + 1), (10, 10), (12, 3)):
        with pytest.raises(lib.PbccsError) as e:
            s.SiteScores(begin, end)
        assert e.value.code == -1
        with pytest.raises(lib.PbccsError) as e:
            s.DiploidSites(0.0, begin, end)
        assert e.value.code == -1
        assert (s.BaselineScore(), s.Score(m)) == before
    # a capacity too small: PBCCS_ERANGE with the needed count
    full = s.DiploidSites(0.0)
    assert len(full) >= 2
    buf = (lib.CDiploidSite * 1)()
    afr = (ctypes.c_int * n_reads)()
    n = ctypes.c_int()
    assert sites_fn(s._h, 0, len(tpl), 0.0, 0, buf, 1, ctypes.byref(n), afr) == -5
    assert n.value == len(full)
    assert (s.BaselineScore(), s.Score(m)) == before
    out = (ctypes.c_float * 9)()
    nn = ctypes.c_longlong()
    assert scores_fn(s._h, 0, 4, out, 9, ctypes.byref(nn)) == -5
    assert nn.value == 4 * n_reads * 9
    assert (s.BaselineScore(), s.Score(m)) == before
    assert diploid.diploid_sites(sites_fn, s._h, n_reads, len(tpl), 0.0, 0, None, False) == full

"""Directional consensus on the GPU: k_strand_sums against the scorer's own per-read scores bit for
bit, the screen against the CPU restatement over oracle scores, the batch keywords, the per-strand polish and the
site buffers.  Fixture: tests/golden/strand_zmws.json (tests/strand_common.py makes it)."""
import ctypes
import math

import pytest

from oracle import oracle as O
from tests import strand_common as C
from tests import strand_restatement as R

pytestmark = pytest.mark.gpu

SUB_FIELDS = ("status", "status_code", "consensus", "qvs", "add_read_results", "zg", "za", "predicted_accuracy",
              "n_tested", "n_applied", "n_passes", "status_counts")


@pytest.fixture(scope="module")
def P():
    import pbccs_amd
    return pbccs_amd


@pytest.fixture(scope="module")
def eng(P):
    return P.default_engine()


@pytest.fixture(scope="module")
def fx():
    return C.load_fixture()


@pytest.fixture(scope="module")
def plain(P, eng, fx):
    """polish_zmws without the keywords: computed once, shared, left unchanged."""
    return P.polish_zmws(C.polish_inputs(fx), engine=eng)


@pytest.fixture(scope="module")
def always(P, eng, fx):
    return P.polish_zmws(C.polish_inputs(fx), engine=eng, directional="always")


def _close(a, b, rel=1e-9, abs_=1e-9):   # tests/test_gpu_parity.py's tolerance for scores
    return abs(a - b) <= abs_ + rel * max(abs(a), abs(b))


def same(a, b):
    """== with NaN equal to NaN (zscores, zg / za of records without them)."""
    if isinstance(a, float) and isinstance(b, float):
        return a == b or (math.isnan(a) and math.isnan(b))
    if isinstance(a, (list, tuple)) and isinstance(b, (list, tuple)):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if isinstance(a, dict) and isinstance(b, dict):
        return set(a) == set(b) and all(same(a[k], b[k]) for k in a)
    return a == b


def gpu_polished(P, eng, z):
    s = P.ArrowMultiReadMutationScorer(P.ArrowConfig(z["snr"]), z["draft"], eng)
    for r in z["reads"]:
        s.AddRead(r["seq"], r["strand"], r["ts"], r["te"], C.MIN_ZSCORE)
    conv, _, _ = P.RefineConsensus(s)
    return s, conv


# ---- 1. the sums ---------------------------------------------------------------------------------------------------
def test_scorer_sums_equal_the_per_read_scores_bit_for_bit(P, eng):
    """Every unique single-base mutation of a 64-base template with five reads (both strands, one partial window,
    one read the z-score gate rejected): StrandScores == the sums of Scores(m, 0) per strand in read order, and
    the counts == the reads that enter them."""
    tpl, reads = C.scorer_case()
    s = P.ArrowMultiReadMutationScorer(P.ArrowConfig(C.SNR), tpl, eng)
    res = [s.AddRead(r["seq"], r["strand"], r["ts"], r["te"], C.MIN_ZSCORE) for r in reads]
    assert res == [0, 0, 0, 3, 0]
    strands = [r["strand"] for r in reads]
    muts = [P.Mutation(t, p, b) for (t, p, b) in O.unique_mutations(tpl)]
    got = s.StrandScores(muts)
    assert len(got) == len(muts) == 439
    counts = set()
    for m, g in zip(muts, got):
        zero = s.Scores(m, 0.0)
        mask = s.Scores(m, float("nan"))
        per = [None if math.isnan(v) else z for v, z in zip(mask, zero)]
        want = R.strand_sums(per, strands)
        assert tuple(g) == want, m
        counts.add((g.n_fwd, g.n_rev))
    assert counts == {(3, 1), (2, 1)}   # the partial window drops out at the ends, the rejected read everywhere
    assert s.StrandScores([]) == []
    with pytest.raises(P.PbccsError):
        s.StrandScores([P.Mutation(2, 64, "A")])


# ---- 2. the screen against the oracle ------------------------------------------------------------------------------
@pytest.mark.parametrize("idx", range(6))
def test_scorer_sites_match_the_restatement_over_oracle_scores(P, eng, fx, idx):
    z = fx[idx]
    s, conv = gpu_polished(P, eng, z)
    assert conv and s.Template() == z["oracle_final"]
    got = s.StrandSites()
    want = z["oracle_sites"]
    print("sites", z["seed"], z["hetero"], got)
    assert [(g.pos, g.type, g.base) for g in got] == [tuple(w[:3]) for w in want]
    for g, w in zip(got, want):
        assert _close(g.sum_fwd, w[3]) and _close(g.sum_rev, w[4]), (g, w)
    if z["hetero"]:
        assert any(g.pos in (C.SITE, C.SITE + 1) for g in got)
    else:
        assert got == []
    # the sites are the restatement's over the scorer's own sums, bit for bit
    um = O.unique_mutations(s.Template())
    sums = [tuple(x) for x in s.StrandScores([P.Mutation(t, p, b) for (t, p, b) in um])]
    assert [tuple(g) for g in got] == R.strand_sites(um, sums)
    # other thresholds: a higher bar than any sum has no sites; min_reads above the passes per strand neither
    assert s.StrandSites(min_score=1e3) == [] and s.StrandSites(min_reads=C.PASSES // 2 + 1) == []


# ---- 3. the batch keyword ------------------------------------------------------------------------------------------
def test_batch_sites_leave_every_other_field_alone(P, eng, fx, plain, monkeypatch):
    zmws = C.polish_inputs(fx)
    got = P.polish_zmws(zmws, engine=eng, strand_sites=True)
    for g, p, z in zip(got, plain, fx):
        assert set(g) == set(p) | {"strand_sites"}
        for k in p:
            assert same(g[k], p[k]), k
        assert [tuple(x[:3]) for x in g["strand_sites"]] == [tuple(w[:3]) for w in z["oracle_sites"]]
    # on exact fills the batch's sites are the per-scorer call's, bit for bit
    monkeypatch.setenv("PBCCS_CERTIFIED_SCAN", "0")
    exact = P.polish_zmws(zmws, engine=eng, strand_sites=True)
    for e, z in zip(exact, fx):
        s, _ = gpu_polished(P, eng, z)
        assert e["strand_sites"] == s.StrandSites()
    # the work queue's call takes the keyword too
    stream = P.polish_stream(zmws, engine=eng, strand_sites=True)
    monkeypatch.delenv("PBCCS_CERTIFIED_SCAN")
    for a, e in zip(stream, exact):
        assert a["strand_sites"] == e["strand_sites"] and a["consensus"] == e["consensus"]


def test_batch_sites_under_band_reclaim(P, eng, fx, monkeypatch):
    """QVs taken in the round a ZMW converges (PBCCS_RECLAIM=1): the same sweep, the same sites."""
    zmws = C.polish_inputs(fx)
    base = P.polish_zmws(zmws, engine=eng, strand_sites=True)
    monkeypatch.setenv("PBCCS_RECLAIM", "1")
    again = P.polish_zmws(zmws, engine=eng, strand_sites=True)
    for a, b in zip(again, base):
        assert a["strand_sites"] == b["strand_sites"] and a["consensus"] == b["consensus"] and a["qvs"] == b["qvs"]


def test_batch_options_and_stats(P, fx):
    e = P.Engine(0)
    e.set_profiling(True)
    e.kernel_stats(reset=True)
    P.strand_stats(e, reset=True)
    zmws = C.polish_inputs(fx)
    got = P.polish_zmws(zmws, engine=e, strand_sites={"min_score": 1e3})
    assert all(g["strand_sites"] == [] for g in got)
    got = P.polish_zmws(zmws, engine=e, strand_sites={"min_sites": 3}, directional="discordant")
    assert all("fwd" not in g for g in got)          # no fixture ZMW has three sites
    st = P.strand_stats(e, reset=True)
    n_sites = sum(len(z["oracle_sites"]) for z in fx)
    assert st == {"strand_screened": 2 * len(fx), "strand_sites": n_sites, "strand_split": 0}
    ks = e.kernel_stats(reset=True)
    assert ks["k_strand_sums"]["launches"] == 2 and ks["k_strand_sites"]["launches"] == 2
    P.polish_zmws(zmws, engine=e)
    ks = e.kernel_stats(reset=True)
    assert ks["k_strand_sums"]["launches"] == 0 and ks["k_strand_sites"]["launches"] == 0   # off unless asked for


# ---- 4. the per-strand polish --------------------------------------------------------------------------------------
def test_always_gives_each_strand_its_own_record(P, eng, fx, plain, always):
    hand = {s: P.polish_zmws([C.single_strand(z, s) for z in fx], engine=eng) for s in (0, 1)}
    for i, (g, p, z) in enumerate(zip(always, plain, fx)):
        assert set(g) == set(p) | {"strand_sites", "fwd", "rev"}
        for k in p:
            assert same(g[k], p[k]), k
        for key, strand in (("fwd", 0), ("rev", 1)):
            sub, h = g[key], hand[strand][i]
            for k in SUB_FIELDS:
                if k != "add_read_results":
                    assert same(sub[k], h[k]), (key, k)
            # per-read entries indexed like the joint record's
            idx = [k for k, r in enumerate(z["reads"]) if r["strand"] == strand]
            assert [sub["add_read_results"][k] for k in idx] == h["add_read_results"]
            assert same([sub["zscores"][k] for k in idx], h["zscores"])
            other = [k for k in range(len(z["reads"])) if k not in idx]
            assert all(sub["add_read_results"][k] == -1 and math.isnan(sub["zscores"][k]) for k in other)
        assert g["fwd"]["consensus"] == z["truth"] and g["rev"]["consensus"] == z["alt"]
        assert g["fwd"]["status"] == g["rev"]["status"] == "Success"


def test_discordant_splits_the_heteroduplex_zmws_only(P, eng, fx, plain, always):
    got = P.polish_zmws(C.polish_inputs(fx), engine=eng, directional="discordant")
    for g, p, a, z in zip(got, plain, always, fx):
        assert g["strand_sites"] == a["strand_sites"]
        if z["hetero"]:
            assert same(g["fwd"], a["fwd"]) and same(g["rev"], a["rev"])
            assert all(same(g[k], a[k]) for k in a)
        else:
            assert "fwd" not in g and "rev" not in g and g["strand_sites"] == []
            assert set(g) == set(p) | {"strand_sites"}
            for k in p:
                assert same(g[k], p[k]), k


def test_a_strand_without_reads_ends_as_an_empty_zmw(P, eng, fx):
    z = fx[1]
    only_fwd = {"draft": z["draft"], "snr": z["snr"], "reads": [r for r in z["reads"] if r["strand"] == 0]}
    g = P.polish_zmws([only_fwd], engine=eng, directional="always")[0]
    empty = P.polish_zmws([{"draft": z["draft"], "snr": z["snr"], "reads": []}], engine=eng)[0]
    assert g["rev"]["status"] == empty["status"] == "NoSubreads" and g["rev"]["consensus"] == ""
    assert g["fwd"]["consensus"] == g["consensus"] and g["strand_sites"] == []   # min_reads: no reverse read scores


# ---- 6. the site buffers -------------------------------------------------------------------------------------------
def test_site_buffers_one_entry_too_small(P, eng, fx):
    from pbccs_amd import lib as L
    from pbccs_amd import polish, strand
    z = fx[0]
    need = len(z["oracle_sites"])
    assert need == 2
    m = polish._Marshalled(C.polish_inputs([z]))
    opts = P.ConsensusSettings()._c()
    so = strand.strand_options(True, None)
    sb = strand.SiteBuffers([need - 1], [len(z["reads"])])
    rc = L.load().pbccs_polish_batch_strand(eng._h, m._ins, 1, ctypes.byref(opts), None, ctypes.byref(so), sb.arr,
                                            m._outs)
    assert rc == -5 and sb.arr[0].n_sites == -need
    assert m.results()[0]["consensus"] == z["oracle_final"]      # the joint record is written all the same
    with pytest.raises(L.PbccsError):
        sb.sites(0)
    # the scorer's call: the needed size, nothing written
    s, _ = gpu_polished(P, eng, z)
    n = ctypes.c_int()
    pos = (ctypes.c_int * 1)(-7)
    rc = L.load().pbccs_scorer_strand_sites(s._h, None, pos, (ctypes.c_int * 1)(), ctypes.create_string_buffer(1),
                                            (ctypes.c_double * 1)(), (ctypes.c_double * 1)(), need - 1, ctypes.byref(n))
    assert rc == -5 and n.value == need and pos[0] == -7
    # the engine stays usable
    again = P.polish_zmws(C.polish_inputs([z]), engine=eng, strand_sites=True)[0]
    assert [tuple(x[:3]) for x in again["strand_sites"]] == [tuple(w[:3]) for w in z["oracle_sites"]]
    assert [tuple(x[:3]) for x in s.StrandSites()] == [tuple(x[:3]) for x in again["strand_sites"]]


# ---- 5. ccs ----------------------------------------------------------------------------------------------------------
def test_ccs_batch_equals_the_driver_then_polish(P, eng, fx):
    """From raw subreads: the native call's records equal zmw_inputs_batch then polish_zmws(directional="always");
    per-read entries are indexed by input subread, each subread in at most one strand's record."""
    from pbccs_amd import driver
    chunks = [{"snr": z["snr"], "reads": [{"seq": r["seq"]} for r in z["reads"]]} for z in fx[:4]]
    native = driver.ccs_batch(chunks, engine=eng, directional="always")
    ins = driver.zmw_inputs_batch(chunks, engine=eng)
    assert all(st is None for st, _ in ins)
    exp = P.polish_zmws([z for _, z in ins], engine=eng, directional="always")
    plain = driver.ccs_batch(chunks, engine=eng)
    for got, e, p, c in zip(native, exp, plain, chunks):
        assert set(got) == set(p) | {"strand_sites", "fwd", "rev"}
        for k in p:
            assert same(got[k], p[k]), k                       # the joint record is the plain call's
        assert got["strand_sites"] == e["strand_sites"]
        for k in ("status", "consensus", "qvs", "n_tested", "n_applied", "predicted_accuracy", "n_passes"):
            assert same(got[k], e[k]), k
        for key in ("fwd", "rev"):
            for k in SUB_FIELDS:
                if k != "add_read_results":
                    assert same(got[key][k], e[key][k]), (key, k)
            assert len(got[key]["add_read_results"]) == len(got[key]["zscores"]) == len(c["reads"])
            assert sorted(a for a in got[key]["add_read_results"] if a >= 0) == \
                sorted(a for a in e[key]["add_read_results"] if a >= 0)
        both = [k for k in range(len(c["reads"]))
                if got["fwd"]["add_read_results"][k] >= 0 and got["rev"]["add_read_results"][k] >= 0]
        either = [k for k in range(len(c["reads"]))
                  if got["fwd"]["add_read_results"][k] >= 0 or got["rev"]["add_read_results"][k] >= 0]
        assert both == [] and either == [k for k, a in enumerate(got["add_read_results"]) if a >= 0]
    with pytest.raises(ValueError):
        driver.ccs_batch(chunks, engine=eng, directional="always", polish_window={"window": 2000})
    with pytest.raises(ValueError):
        driver.ccs_batch(chunks, engine=eng, strand_sites=True, polish_window={})

"""Per-base rich consensus QVs on the GPU (k_qv_rich / k_qqv_rich): the substitution, insertion
and deletion QVs and the substitution / insertion tags of every template position, through ConsensusRichQVs and the
rich_qvs=True keyword of polish_zmws, polish_windowed, quiver.polish_batch and driver.ccs_batch.

The reference has no such function; the rules are a decomposition of its ConsensusQVs sum, so the CPU restatement's
per-mutation scores (oracle.Scorer.score / QuiverScorer.score over oracle.unique_mutations, full sums) give the
expected values through tests/rich_qvs_common.py.  Arrow: typed QVs within the project's +-1 (equal where the partial
sum is empty), tags equal wherever the two best scores of the type differ by more than 1e-6 in the oracle.  Quiver:
typed QVs equal, since its scores are the reference's floats bit for bit and the host libm decides every rounding the
device could get wrong.  The overall qvs returned beside them equal ConsensusQVs' exactly."""
import math

import pytest

import rich_qvs_common as C
from oracle import oracle as O
from pbccs_amd.richqv import RICH_KEYS
from tests import test_quiver_gpu as TQ

pytestmark = pytest.mark.gpu

ALL_KEYS = ("qvs",) + RICH_KEYS
EMPTY = C.empty_sum_qv()


@pytest.fixture(scope="module")
def P():
    import pbccs_amd
    return pbccs_amd


@pytest.fixture(scope="module")
def eng(P):
    return P.default_engine()


def same_value(a, b):
    if isinstance(a, float) and isinstance(b, float):
        return (math.isnan(a) and math.isnan(b)) or a == b
    if isinstance(a, (list, tuple)) and isinstance(b, (list, tuple)):
        return len(a) == len(b) and all(same_value(x, y) for x, y in zip(a, b))
    return a == b


def arrow_scorer(P, tpl, reads, snr, eng, threshold=None):
    s = P.ArrowMultiReadMutationScorer(P.ArrowConfig(snr), tpl, eng)
    res = [s.AddRead(r["seq"], r["strand"], r["ts"], r["te"], threshold) for r in reads]
    return s, res


# ---- Arrow, single scorer ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def arrow_single(P, eng):
    """(rich dict of the GPU scorer, ConsensusQVs of the same scorer, oracle reference, oracle scores by position)."""
    reads = C.arrow_reads()
    s, res = arrow_scorer(P, C.TPL, reads, C.SNR, eng)
    o = O.Scorer(C.TPL, C.SNR)
    assert res == [o.add_read(r["seq"], r["strand"], r["ts"], r["te"]) for r in reads] == [0] * 5
    plain = P.ConsensusQVs(s)
    got = P.ConsensusRichQVs(s)
    ref, by_pos = C.oracle_rich(C.TPL, lambda t, p, b: o.score(t, p, b))
    assert ref["qvs"] == o.qvs()   # the reference computation restates ConsensusQVs' own sum
    return got, plain, ref, by_pos


def test_arrow_overall_qvs_are_consensus_qvs(arrow_single):
    got, plain, ref, _ = arrow_single
    assert set(got) == set(ALL_KEYS)
    assert got["qvs"] == plain
    assert all(len(got[k]) == len(C.TPL) for k in ALL_KEYS)
    assert max(abs(a - b) for a, b in zip(got["qvs"], ref["qvs"])) <= 1


def test_arrow_typed_qvs_against_the_oracle(arrow_single):
    got, _, ref, _ = arrow_single
    for k in ("sub_qv", "ins_qv", "del_qv"):
        print(k, "max |gpu - oracle|", max(abs(a - b) for a, b in zip(got[k], ref[k])))
    C.assert_typed_close(got, ref)


def test_arrow_tags_against_the_oracle(arrow_single):
    """Near-ties (two best scores of a type within 1e-6 in the oracle) are skipped: 0 of the fixture's 56 positions
    (0 %), measured with the oracle alone; at most 5 % may be."""
    got, _, ref, by_pos = arrow_single
    bad, skipped = C.tag_mismatches(got, ref, by_pos)
    print("near-tie positions skipped:", sorted(skipped))
    assert len(skipped) <= 0.05 * len(C.TPL)
    assert not bad, bad


def test_arrow_structure(arrow_single):
    got, _, _, _ = arrow_single
    tpl = C.TPL
    b, e = C.HOMOPOLYMER
    assert len(set(tpl[b:e])) == 1 and e - b >= 3 and tpl[0] != tpl[-1]
    for p in range(b + 1, e):   # the deletion belongs to the run's first base; no insertion of the run's base
        assert got["del_qv"][p] == EMPTY
        assert got["ins_tag"][p] != tpl[b]
    assert got["del_qv"][b] != EMPTY
    assert all(got["sub_tag"][p] != tpl[p] for p in range(len(tpl)))
    assert all(p == 0 or got["ins_tag"][p] != tpl[p - 1] for p in range(len(tpl)))
    assert set(got["sub_tag"]) <= set("ACGT") and set(got["ins_tag"]) <= set("ACGT")
    from pbccs_amd import richqv
    assert [t for t, _ in richqv.unique_mutations(tpl, 0)].count(0) == 4   # M(0): four insertions


# ---- Arrow, batch ---------------------------------------------------------------------------------------------------
def per_scorer_rich(P, z, eng, repeats=None):
    s, res = arrow_scorer(P, z["draft"], z["reads"], z["snr"], eng, threshold=-5.0)
    conv, _, _ = P.RefineConsensus(s)
    assert conv
    if repeats:
        P.RefineRepeats(s, *repeats)
    rec = P.ConsensusRichQVs(s)
    rec["consensus"] = s.Template()
    return rec


@pytest.fixture(scope="module")
def batch3(P, eng):
    """Three ZMWs of different lengths in one device batch (the work-item search of k_qv_rich crosses items)."""
    from pbccs_amd import synth
    zmws = [synth.make_zmws(1, n, 5, seed=seed)[0] for n, seed in ((70, 970), (150, 1050), (97, 998))]   # all converge
    return zmws, P.polish_zmws(zmws, engine=eng, rich_qvs=True)


def test_batch_equals_per_scorer(P, eng, batch3):
    zmws, got = batch3
    for z, g in zip(zmws, got):
        assert g["status"] in ("Success", "PoorQuality")
        e = per_scorer_rich(P, z, eng)
        for k in ("consensus",) + ALL_KEYS:
            assert g[k] == e[k], k
        assert len(g["sub_tag"]) == len(g["consensus"])
    stream = P.polish_stream(zmws, engine=eng, rich_qvs=True)
    assert all(a.keys() == b.keys() and all(same_value(a[k], b[k]) for k in a) for a, b in zip(stream, got))


def test_batch_without_the_keyword_is_unchanged(P, eng, batch3):
    zmws, got = batch3
    plain = P.polish_zmws(zmws, engine=eng)
    for g, p in zip(got, plain):
        assert not set(RICH_KEYS) & set(p)
        assert set(g) == set(p) | set(RICH_KEYS)
        for k in p:
            assert same_value(g[k], p[k]), k


def test_batch_with_repeats(P, eng):
    from tests import arrow_multibase_common as M
    z = M.load_slips()[0]
    zmw = {"draft": z["draft"], "snr": z["snr"], "reads": z["reads"]}
    got = P.polish_zmws([zmw], engine=eng, repeats=(2, 3), rich_qvs=True)[0]
    assert got["n_repeat_applied"] == 1 and got["consensus"] == z["truth"] != z["oracle_final"]
    e = per_scorer_rich(P, zmw, eng, repeats=(2, 3))
    for k in ("consensus",) + ALL_KEYS:
        assert got[k] == e[k], k
        assert len(got[k]) == len(z["truth"])
    plain = P.polish_zmws([zmw], engine=eng, repeats=(2, 3))[0]
    assert not set(RICH_KEYS) & set(plain) and all(same_value(got[k], plain[k]) for k in plain)


@pytest.mark.parametrize("env,value", [("PBCCS_CKPT_ALL", "4"), ("PBCCS_RECLAIM", "1")])
def test_batch_on_checkpointed_bands_and_with_reclaim(P, eng, batch3, monkeypatch, env, value):
    """Reads on checkpointed bands, and QVs taken in the round a ZMW converges (band reclaim): the sweep's scores are
    what they are on every path, so the rich records equal the unset run's."""
    zmws, got = batch3
    monkeypatch.setenv(env, value)
    again = P.polish_zmws(zmws, engine=eng, rich_qvs=True)
    for g, a in zip(got, again):
        for k in ("status", "consensus") + ALL_KEYS:
            assert a[k] == g[k], k


# ---- Quiver -----------------------------------------------------------------------------------------------------------
def quiver_reference(o):
    """The definition over the restatement's float scores, with the host libm (math.exp / math.log10)."""
    ref, _ = C.oracle_rich(o.template(), lambda t, p, b: o.score(t, p, b))
    return ref


@pytest.mark.parametrize("sum_product", [True, False])
def test_quiver_typed_qvs_equal_the_host_libm(P, sum_product, monkeypatch):
    tpl, reads = TQ._zmw(121 + int(sum_product), 90, 4)
    g, o = TQ._pair(tpl, reads, sum_product)
    conv, _, _ = P.RefineConsensus(g.s)
    o.refine()
    assert g.template() == o.template()
    plain = P.ConsensusQVs(g.s)
    got = P.ConsensusRichQVs(g.s)
    ref = quiver_reference(o)
    assert got["qvs"] == plain == o.qvs() == ref["qvs"]
    for k in RICH_KEYS:
        assert got[k] == ref[k], k
    monkeypatch.setenv("PBCCS_QQV_HOST", "1")   # every position left to the host
    host = P.ConsensusRichQVs(g.s)
    assert host == got


def test_quiver_batch_equals_per_scorer(P, eng):
    from pbccs_amd import quiver as Q
    zmws = []
    for seed, n in ((131, 60), (132, 110)):
        tpl, reads = TQ._zmw(seed, n, 4)
        zmws.append({"tpl": tpl, "reads": reads})
    cfg = Q.QuiverConfig(Q.QvModelParams(**TQ.PARAMS2), sum_product=True)
    got = Q.polish_batch(zmws, cfg, engine=eng, rich_qvs=True)
    plain = Q.polish_batch(zmws, cfg, engine=eng)
    for z, g, p in zip(zmws, got, plain):
        assert not set(RICH_KEYS) & set(p) and all(g[k] == p[k] for k in p)
        s = P.QuiverMultiReadMutationScorer(cfg, z["tpl"], eng)
        for r in z["reads"]:
            f = r["features"]
            s.AddRead(r["seq"], r["strand"], r["ts"], r["te"], ins_qv=f["ins"], subs_qv=f["subs"], del_qv=f["del"],
                      del_tag=f["del_tag"], merge_qv=f["merge"])
        P.RefineConsensus(s)
        e = P.ConsensusRichQVs(s)
        assert g["consensus"] == s.Template()
        for k in ALL_KEYS:
            assert g[k] == e[k], k


# ---- windowed and ccs -------------------------------------------------------------------------------------------------
def test_windowed_stitches_the_windows_pieces(P, eng):
    """The smallest two-window shape (the restatement joins it without a fallback).  The windows' pseudo-ZMWs
    (tests/polish_window_restatement.py, rules 2 and 3) are polished on their own and the stitched arrays must be
    their recorded pieces."""
    import polish_window_restatement as W
    from pbccs_amd import polish, synth
    opts = dict(window=200, overlap=40, guard=8, k=6)
    z = synth.make_zmws(1, 320, 4, seed=3203)[0]
    got = polish.polish_windowed([z], engine=eng, rich_qvs=True, **opts)[0]
    assert got["windowed"] and got["fallback"] == 0 and len(got["windows"]) == 2 and got["status"] == "Success"
    bounds, rows, _ = W.slices(z, 200, 40, 6)
    wins = P.polish_zmws(W.window_inputs(z, bounds, rows), engine=eng, rich_qvs=True)
    for k in ("consensus",) + ALL_KEYS:
        want = wins[0][k][:0]
        for w, rec in zip(wins, got["windows"]):
            want = want + w[k][rec["cut_begin"]:rec["cut_end"]]
        assert got[k] == want, k
        assert len(got[k]) == len(got["consensus"])
    plain = polish.polish_windowed([z], engine=eng, **opts)[0]
    assert not set(RICH_KEYS) & set(plain) and all(same_value(got[k], plain[k]) for k in plain)


def test_ccs_batch_equals_the_driver_then_polish(P, eng):
    from pbccs_amd import driver, synth
    zmws = synth.make_zmws(3, 90, 5, seed=4107)
    chunks = [{"snr": z["snr"], "reads": [{"seq": r["seq"]} for r in z["reads"]]} for z in zmws]
    native = driver.ccs_batch(chunks, engine=eng, rich_qvs=True)
    ins = driver.zmw_inputs_batch(chunks, engine=eng)
    assert all(st is None for st, _ in ins)
    exp = P.polish_zmws([z for _, z in ins], engine=eng, rich_qvs=True)
    done = 0
    for got, e in zip(native, exp):
        for k in ("status", "consensus") + ALL_KEYS:
            assert got[k] == e[k], k
        if got["status"] in ("Success", "PoorQuality"):
            done += 1
            assert all(len(got[k]) == len(got["consensus"]) > 0 for k in ALL_KEYS)
        else:   # no consensus: nothing is written
            assert all(len(got[k]) == 0 for k in ALL_KEYS)
    assert done >= 2
    plain = driver.ccs_batch(chunks, engine=eng)
    for got, p in zip(native, plain):
        assert not set(RICH_KEYS) & set(p) and all(same_value(got[k], p[k]) for k in p)


# ---- cost of asking (printed, not asserted) ------------------------------------------------------------------------
def test_kernel_stats_name_the_rich_kernel(P, batch3):
    zmws, _ = batch3
    e = P.Engine(0)
    e.set_profiling(True)
    e.kernel_stats(reset=True)
    P.polish_zmws(zmws, engine=e, rich_qvs=True)
    st = e.kernel_stats(reset=True)
    assert st["k_qv_rich"]["launches"] >= 1 and st["k_qv"]["launches"] == 0
    P.polish_zmws(zmws, engine=e)
    st = e.kernel_stats(reset=True)
    assert st["k_qv"]["launches"] >= 1 and st["k_qv_rich"]["launches"] == 0

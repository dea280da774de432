"""The Arrow and Quiver engines on low-complexity templates and hostile reads (tests/hostile_inputs.py), against the
CPU restatement: homopolymer, dinucleotide and run-length templates whose short reads brush and pass the 16-lane
fill's 64-row buffer; reads with indel bursts, junk and the wrong strand, whose columns run to two and three 128-row
chunks next to a 20-row read of the same ZMW; AddRead results other than SUCCESS from real multi-base reads; a read
that turns inactive in mid-refine; QVs down to 2 and the PoorQuality cut at a threshold ZMWs fall under.
tests/test_hostile_inputs_cpu.py checks that the inputs do all that.

Tolerances are the suite's: AddRead results, flip-flops, nTested / nApplied, templates and active sets exact; fill LLs
1e-12 relative and absolute (tests/test_fill_operands_gpu._check_fills); mutation scores and z-scores 1e-9 relative
(tests/test_gpu_parity._close); QVs +-1, on the scorer path at most max(1, len // 1000) positions differing;
predicted accuracy 1e-3; Quiver bit-exact.
"""
import math

import pytest

from oracle import oracle as O
from tests import hostile_inputs as H
from tests.test_fill_operands_gpu import EXACT_PATHS, _check_fills
from tests.test_gpu_parity import P, _close   # noqa: F401  (P: the module fixture)
from tests.test_quiver_gpu import GpuQuiver, _qvs_exact

pytestmark = pytest.mark.gpu

NAN = float("nan")
LOW = H.LOW_COMPLEXITY_NAMES
HOSTILE_SETTINGS = dict(min_zscore=-1e9, max_drop_fraction=1.0)   # the hostile reads stay in, the refine runs with them


def _oracle_fills(tpl, reads, threshold=NAN, snr=H.SNR):
    o, res = H.add_reads(tpl, reads, threshold, snr)
    return o, res, [o.read_info(k) for k in range(len(reads))]


def _gpu_fills(P, tpl, reads, monkeypatch, env=None, threshold=NAN, muts=(), snr=H.SNR):
    """The scorer filled under `env`, plus test_fill_operands_gpu._gpu_fills' tuple: AddRead results, flip-flop counts,
    the active reads' LLs and the scores of `muts`."""
    env = env or {}
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    try:
        g = P.ArrowMultiReadMutationScorer(P.ArrowConfig(snr), tpl)
        res = [g.AddRead(r["seq"], r["strand"], r["ts"], r["te"], threshold) for r in reads]
        flips, lls = g.NumFlipFlops(), g.BaselineScores()
        scores = g.ScoreMany([P.Mutation(t, s, b) for (t, s, b) in muts]) if muts else []
    finally:
        for k in env:
            monkeypatch.delenv(k)
    return g, (res, flips, lls, scores)


def _check_read_scores(P, g, o, muts):
    """Scores(m, -1e300) per read against the restatement's."""
    for (t, s, b) in muts:
        sg, so = g.Scores(P.Mutation(t, s, b), -1e300), o.scores(t, s, b, -1e300)
        assert len(sg) == len(so)
        for k, (x, y) in enumerate(zip(sg, so)):
            assert _close(x, y), ((t, s, b), k, x, y)


def _check_record(r, e, qv_exact_count=None):
    """A polish_zmws record against O.polish_zmw's."""
    assert r["add_read_results"] == e["add_read_results"]
    assert (r["n_tested"], r["n_applied"]) == (e["n_tested"], e["n_applied"])
    assert _close(r["zg"], e["zg"]) and _close(r["za"], e["za"])
    for x, y in zip(r["zscores"], e["zscores"]):
        assert _close(x, y), (x, y)
    if not e["converged"]:
        assert r["status"] == "NonConvergent"
        return
    assert r["status"] in ("Success", "PoorQuality")
    assert r["consensus"] == e["template"]
    assert len(r["qvs"]) == len(e["qvs"]) and max(abs(a - b) for a, b in zip(r["qvs"], e["qvs"])) <= 1
    assert abs(r["predicted_accuracy"] - e["pred_acc"]) < 1e-3


def _same_records(a, b):
    """test_certified_scan_equals_exact_path's comparison of two runs of one batch."""
    for x, y in zip(a, b):
        for k in ("status", "consensus", "n_tested", "n_applied", "add_read_results", "n_passes", "status_counts"):
            assert x[k] == y[k], k
        assert len(x["qvs"]) == len(y["qvs"]) and all(abs(p - q) <= 1 for p, q in zip(x["qvs"], y["qvs"]))
        assert all(_close(p, q) for p, q in zip(x["zscores"], y["zscores"]))


COUNTED = ("fill_launches", "scan_reads", "uncertain_reads", "exact_rounds")


def _polish(zs, monkeypatch, settings=None, **env):
    """polish_zmws under `env` on the process's default engine, and what the call added to the engine's counters.
    (No engine of its own per call: a band pool never maps an address range the process has mapped before, and each
    engine that comes and goes uses ranges up -- the suite runs in one process.)"""
    import pbccs_amd
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    try:
        eng = pbccs_amd.default_engine()
        before = eng.counters()
        res = pbccs_amd.polish_zmws(zs, settings, engine=eng)
        after = eng.counters()
    finally:
        for k in env:
            monkeypatch.delenv(k)
    c = {k: after[k] - before[k] for k in COUNTED}
    c["fill_work"] = [a - b for a, b in zip(after["fill_work"], before["fill_work"])]
    return res, c


# ================================================================ 1. low-complexity fills and scores
@pytest.mark.parametrize("name", LOW)
def test_low_complexity_fills_and_scores_match_oracle(P, monkeypatch, name):
    """Default path (the reads of G120 stay under the 16-lane buffer's 64 rows by one to seven, those of A400 and CT300
    move to the 64-lane path in mid-fill): fills, every unique mutation's full and fast score, and the per-read scores
    of every third mutation."""
    z = dict(H.low_complexity_zmws())[name]
    ref = _oracle_fills(z["draft"], z["reads"])
    g, got = _gpu_fills(P, z["draft"], z["reads"], monkeypatch)
    _check_fills(got, ref)
    o = ref[0]
    assert _close(g.BaselineScore(), o.baseline())
    muts = O.unique_mutations(z["draft"])
    gm = [P.Mutation(t, s, b) for (t, s, b) in muts]
    for (t, s, b), vf, vq in zip(muts, g.ScoreMany(gm), g.ScoreMany(gm, -12.5)):
        assert _close(vf, o.score(t, s, b)), (t, s, b, vf)
        assert _close(vq, o.score(t, s, b, -12.5)), (t, s, b, vq)
    _check_read_scores(P, g, o, muts[::3])


# ================================================================ 2. low-complexity refine and QVs
@pytest.mark.parametrize("name", LOW)
def test_low_complexity_refine_and_qvs_match_oracle(P, name):
    """RefineConsensus and ConsensusQVs through the scorer (CT300: 15498 mutations tested, 51 applied; QVs down to 2)."""
    z = dict(H.low_complexity_zmws())[name]
    g = P.ArrowMultiReadMutationScorer(P.ArrowConfig(z["snr"]), z["draft"])
    o = O.Scorer(z["draft"], z["snr"])
    rg = [g.AddRead(r["seq"], r["strand"], r["ts"], r["te"], -5.0) for r in z["reads"]]
    ro = [o.add_read(r["seq"], r["strand"], r["ts"], r["te"], -5.0) for r in z["reads"]]
    assert rg == ro
    conv, nt, na = P.RefineConsensus(g)
    ref = o.refine()
    assert conv == ref["converged"]
    assert (nt, na) == (ref["n_tested"], ref["n_applied"])
    assert g.Template() == o.template()
    assert _close(g.BaselineScore(), o.baseline(), 1e-9)
    qg, qo = P.ConsensusQVs(g), o.qvs()
    print(name, nt, na, "min qv", min(qg), min(qo))
    assert len(qg) == len(qo)
    assert max(abs(a - b) for a, b in zip(qg, qo)) <= 1
    assert sum(a != b for a, b in zip(qg, qo)) <= max(1, len(qo) // 1000)


@pytest.fixture(scope="module")
def low_batch():
    zs = [z for _, z in H.low_complexity_zmws()]
    return zs, [O.polish_zmw(z["draft"], z["reads"], z["snr"]) for z in zs]


def test_low_complexity_batch_matches_oracle_with_and_without_certified_scan(low_batch, monkeypatch):
    zs, ref = low_batch
    fast, cf = _polish(zs, monkeypatch)
    exact, ce = _polish(zs, monkeypatch, PBCCS_CERTIFIED_SCAN="0")
    print("scan_reads", cf["scan_reads"], "uncertain_reads", cf["uncertain_reads"], "exact_rounds", cf["exact_rounds"])
    assert ce["scan_reads"] == 0
    for res in (fast, exact):
        for r, e in zip(res, ref):
            assert e["converged"]
            _check_record(r, e)
    _same_records(fast, exact)


# ================================================================ 3. the PoorQuality cut
def test_poor_quality_cut_at_a_threshold_zmws_fall_under(low_batch, monkeypatch):
    """min_predicted_accuracy = 0.98 (capi.hip polish_one's cut; the default 0.90 lies under every ZMW of the suite):
    the restatement puts AC60, CT300, A120, runlength under it and CAG40, AT150, flank_T40 over it."""
    from pbccs_amd.polish import ConsensusSettings
    zs, ref = low_batch
    res, _ = _polish(zs, monkeypatch, ConsensusSettings(min_predicted_accuracy=0.98))
    sides = set()
    for name, r, e in zip(LOW, res, ref):
        assert e["converged"] and r["status"] in ("Success", "PoorQuality"), name
        print(name, r["status"], r["predicted_accuracy"], e["pred_acc"])
        assert (r["status"] == "PoorQuality") == (r["predicted_accuracy"] < 0.98), name
        acc = 1.0 - sum(10.0 ** (-q / 10.0) for q in r["qvs"]) / len(r["qvs"])
        assert abs(r["predicted_accuracy"] - acc) <= 1e-12, name
        if abs(e["pred_acc"] - 0.98) > 1e-3:
            assert (r["status"] == "PoorQuality") == (e["pred_acc"] < 0.98), name
            sides.add(r["status"])
        assert r["consensus"] == e["template"] and len(r["qvs"]) == len(r["consensus"])   # a cut ZMW keeps its record
    assert sides == {"Success", "PoorQuality"}


# ================================================================ 4. hostile fills
@pytest.fixture(scope="module")
def hostile_refs():
    """Per (L, threshold): the restatement's scorer, AddRead results and read infos of the hostile ZMW."""
    out = {}
    for L in (150, 300):
        h = H.hostile_zmw(L)
        for thr in (NAN, -5.0):
            out[(L, math.isnan(thr))] = _oracle_fills(h["zmw"]["draft"], h["reads"], thr)
    return out


@pytest.mark.parametrize("L", [150, 300])
def test_hostile_fills_match_oracle(P, monkeypatch, hostile_refs, L):
    """The ZMW's five passes plus every hostile read, at thresholds NaN and -5.0: AddRead results (NaN: SUCCESS and
    ALPHABETAMISMATCH -- one base, 2 L of junk, b + b, 220 and more inserted bases; -5.0: POOR_ZSCORE too), flip-flops,
    LLs, z-scores, and at NaN every read's score of every fifth unique mutation."""
    h = H.hostile_zmw(L)
    tpl, reads = h["zmw"]["draft"], h["reads"]
    for thr in (NAN, -5.0):
        ref = hostile_refs[(L, math.isnan(thr))]
        g, got = _gpu_fills(P, tpl, reads, monkeypatch, threshold=thr)
        print(L, thr, [got[0].count(k) for k in range(5)])
        _check_fills(got, ref)
        o = ref[0]
        assert [g.ReadInfo(k)["active"] for k in range(len(reads))] == [i["active"] for i in ref[2]]
        assert _close(g.BaselineScore(), o.baseline())
        (zg, za), zs = g.ZScores()
        ozg, oza, ozs = o.zscores()
        assert _close(zg, ozg) and _close(za, oza)
        for k, (a, b) in enumerate(zip(zs, ozs)):
            assert _close(a, b), (h["names"][k], a, b)
        if math.isnan(thr):
            _check_read_scores(P, g, o, O.unique_mutations(tpl)[::5])


@pytest.mark.parametrize("L", [150, 300])
def test_hostile_fills_agree_bit_for_bit_on_every_exact_path(P, monkeypatch, hostile_refs, L):
    """The threshold-NaN set started on every exact instantiation of k_fill_coop (a read too tall for the path it is
    started on re-routes): AddRead results, flip-flops, LL bits and one round's mutation scores are the same."""
    h = H.hostile_zmw(L)
    tpl, reads = h["zmw"]["draft"], h["reads"]
    muts = O.unique_mutations(tpl)[::5]
    outs = [_gpu_fills(P, tpl, reads, monkeypatch, env, muts=muts)[1] for _, env in EXACT_PATHS]
    _check_fills(outs[0], hostile_refs[(L, True)])
    for (name, _), got in zip(EXACT_PATHS[1:], outs[1:]):
        assert got[0] == outs[0][0], name
        assert got[1] == outs[0][1], name
        assert got[2] == outs[0][2], name
        assert got[3] == outs[0][3], name
    _, default = _gpu_fills(P, tpl, reads, monkeypatch, muts=muts)
    assert default == outs[0]


def test_hostile_reads_leave_the_16_lane_path(monkeypatch, hostile_refs):
    """The scorer's own batch does not report into the engine's counters, so the paths are read off a polish_zmws
    call whose only fills are AddRead's (min_passes out of reach: the ZMW is gated TooFewPasses after the fill and
    never refined), certified scan off.  fill_launches counts one launch per path per attempt: a batch that stays on
    the 16-lane path is one launch, every promotion adds one.  fill_launches alone cannot tell a promotion from the
    relaunch of a read whose band pool overflowed; the plain ZMW beside it is the control (one launch), and the
    restatement's columns of more than 64 rows cannot be held by the 16-lane path's 64-row buffer.  fill_work names
    the fill kind outright, but PBCCS_FILL_WORK is read once per process: it is checked when the process runs with it.
    Observed on an MI355X: fill_launches 1 for the plain ZMW, 2 for either hostile ZMW."""
    from pbccs_amd import synth
    from pbccs_amd.polish import ConsensusSettings
    gate = ConsensusSettings(min_passes=10**6)
    plain = synth.make_zmws(1, 300, 5, seed=3002)
    _, c0 = _polish(plain, monkeypatch, gate, PBCCS_CERTIFIED_SCAN="0")
    assert c0["fill_launches"] == 1
    for L in (150, 300):
        h = H.hostile_zmw(L)
        o, res, _ = hostile_refs[(L, True)]
        assert max(H.tallest(o, k) for k in range(len(res)) if res[k] == 0) > 64
        z = dict(h["zmw"], reads=h["reads"])
        out, c = _polish([z], monkeypatch, gate, PBCCS_CERTIFIED_SCAN="0")
        print(L, "fill_launches", c["fill_launches"], "fill_work", c["fill_work"])
        assert out[0]["status"] == "TooFewPasses"
        assert c["fill_launches"] >= 2
        if any(c["fill_work"]):
            assert c["fill_work"][6] > 0 and c["fill_work"][8 + 6] > 0   # reads the 16-lane and the 64-lane kind filled


# ================================================================ 5. hostile batch
@pytest.fixture(scope="module")
def hostile_batch():
    from pbccs_amd import synth
    zs = [dict(H.hostile_zmw(L)["zmw"], reads=H.hostile_zmw(L)["reads"]) for L in (150, 300)]
    zs.append(dict(H.low_complexity_zmws())["G120"])
    zs.append(synth.make_zmws(1, 300, 5, seed=3003)[0])
    gated = [O.polish_zmw(z["draft"], z["reads"], z["snr"]) for z in zs]
    kept = [O.polish_zmw(z["draft"], z["reads"], z["snr"], min_zscore=-1e9) for z in zs]
    return zs, gated, kept


def test_hostile_batch_gates_follow_the_oracle(hostile_batch, monkeypatch):
    """Default settings: the hostile ZMWs lose 23 of 38 and 26 of 46 reads to the gate and end TooManyUnusable
    (Consensus.h:473-490 over the restatement's AddRead results); G120 and the plain ZMW polish beside them.
    Observed on an MI355X with the certified scan on: scan_reads 49, uncertain_reads 5."""
    zs, gated, _ = hostile_batch
    runs = []
    for scan in ("1", "0"):
        res, c = _polish(zs, monkeypatch, PBCCS_CERTIFIED_SCAN=scan)
        print("scan", scan, "scan_reads", c["scan_reads"], "uncertain_reads", c["uncertain_reads"])
        # the hostile reads' columns pass 64 rows, so they move to the LDS-only 64-lane path, whose launches the
        # certified fast path takes (ArrowBatch::FillReads: scanPaths bit 0)
        assert (c["scan_reads"] > 0) == (scan == "1")
        runs.append(res)
        statuses = []
        for z, r, e in zip(zs, res, gated):
            st = e["add_read_results"]
            assert r["add_read_results"] == st
            assert r["status_counts"] == [st.count(k) for k in range(5)]
            assert r["n_passes"] == st.count(0)
            statuses.append(r["status"])
            if st.count(0) < 3:
                assert r["status"] == "TooFewPasses"
                continue
            if sum(1 for s in st if s != 0) / len(st) > 0.34:
                assert r["status"] == "TooManyUnusable"
                continue
            _check_record(r, e)
        assert statuses[:2] == ["TooManyUnusable", "TooManyUnusable"] and "TooManyUnusable" not in statuses[2:]
    _same_records(*runs)


def test_hostile_batch_refines_with_the_hostile_reads_kept(hostile_batch, monkeypatch):
    """min_zscore = -1e9, max_drop_fraction = 1: every read AddRead fills stays and the refine runs with 37 and 38
    reads, columns of up to 298 rows among them.  Observed on an MI355X with the certified scan on: scan_reads 114,
    uncertain_reads 5 (re-run exactly), exact_rounds 0; the records equal the exact path's and the restatement's."""
    from pbccs_amd.polish import ConsensusSettings
    zs, _, kept = hostile_batch
    runs = []
    for scan in ("1", "0"):
        res, c = _polish(zs, monkeypatch, ConsensusSettings(**HOSTILE_SETTINGS), PBCCS_CERTIFIED_SCAN=scan)
        print("scan", scan, "scan_reads", c["scan_reads"], "uncertain_reads", c["uncertain_reads"],
              "exact_rounds", c["exact_rounds"])
        assert (c["scan_reads"] > 0) == (scan == "1")
        runs.append(res)
        for r, e in zip(res, kept):
            st = e["add_read_results"]
            assert r["status_counts"] == [st.count(k) for k in range(5)] and r["n_passes"] == st.count(0)
            _check_record(r, e)
    _same_records(*runs)


# ================================================================ 6. a read lost during the refine
@pytest.mark.parametrize("L,seed,names", H.DEACTIVATION_SEEDS)
def test_read_deactivated_in_mid_refine_matches_oracle(P, monkeypatch, L, seed, names):
    """A refill that fails for one read while its ZMW keeps going (ApplyMutations: rs.active = false)."""
    from pbccs_amd.polish import ConsensusSettings
    d = H.deactivation_zmw(L, seed)
    tpl, reads, snr = d["zmw"]["draft"], d["reads"], d["zmw"]["snr"]
    ref = _oracle_fills(tpl, reads, NAN, snr)
    g, got = _gpu_fills(P, tpl, reads, monkeypatch, snr=snr)
    _check_fills(got, ref)
    o = ref[0]
    conv, nt, na = P.RefineConsensus(g)
    r = o.refine()
    assert (conv, nt, na) == (r["converged"], r["n_tested"], r["n_applied"])
    assert g.Template() == o.template()
    info = [o.read_info(k) for k in range(len(reads))]
    lost = [d["names"][k] for k in range(len(reads)) if ref[1][k] == 0 and not info[k]["active"]]
    assert lost == list(names)
    assert [g.ReadInfo(k)["active"] for k in range(len(reads))] == [i["active"] for i in info]
    lls = g.BaselineScores()
    active = [k for k, i in enumerate(info) if i["active"]]
    assert len(lls) == len(active)
    for k, x in zip(active, lls):
        assert _close(x, info[k]["ll"], 1e-12, 1e-12), (d["names"][k], x, info[k]["ll"])
    assert _close(g.BaselineScore(), o.baseline())
    final = g.Template()
    muts = O.unique_mutations(final)[::7]
    for (t, s, b), v in zip(muts, g.ScoreMany([P.Mutation(t, s, b) for (t, s, b) in muts])):
        assert _close(v, o.score(t, s, b)), (t, s, b, v)
    _check_read_scores(P, g, o, muts[::5])
    # the same ZMW through the batch, with and without the band pool's reclaim
    e = O.polish_zmw(tpl, reads, snr, min_zscore=-1e9)
    assert e["template"] == final
    z = dict(d["zmw"], reads=reads)
    for env in ({}, {"PBCCS_RECLAIM": "1"}):
        res, _ = _polish([z], monkeypatch, ConsensusSettings(**HOSTILE_SETTINGS), **env)
        _check_record(res[0], e)


# ================================================================ 7. Quiver on low-complexity templates
@pytest.mark.parametrize("sum_product", [False, True])
@pytest.mark.parametrize("name", [n for n, _ in H.quiver_low_complexity_zmws()])
def test_quiver_low_complexity_matches_oracle(name, sum_product):
    """Homopolymer runs keep the Merge move and its MergeS slope live at every column.  Bit-exact FP32, as
    test_quiver_scores_match_oracle and test_quiver_refine_and_qvs_match_oracle."""
    import pbccs_amd as P
    from pbccs_amd import synth
    z = dict(H.quiver_low_complexity_zmws())[name]
    tpl, reads = z["tpl"], z["reads"]
    g = GpuQuiver(tpl, synth.QUIVER_PARAMS, score_diff=synth.QUIVER_SCORE_DIFF, sum_product=sum_product)
    o = O.QuiverScorer(tpl, synth.QUIVER_PARAMS, score_diff=synth.QUIVER_SCORE_DIFF, sum_product=sum_product)
    for r in reads:
        a = g.add_read(r["seq"], r["strand"], r["ts"], r["te"], r["features"])
        b = o.add_read(r["seq"], r["strand"], r["ts"], r["te"], r["features"])
        assert bool(a) == bool(b)
    n = len(reads)
    active = [k for k in range(n) if o.read_info(k)["active"]]
    assert len(active) == n
    assert [g.s.ReadInfo(k)["active"] for k in range(n)] == [True] * n
    assert g.s.BaselineScores() == [o.read_info(k)["score"] for k in active]
    assert g.s.NumFlipFlops() == [o.read_info(k)["flipflops"] for k in active]
    assert g.baseline() == o.baseline()
    muts = O.unique_mutations(tpl)
    gm = [P.Mutation(t, s, b) for (t, s, b) in muts]
    for (t, s, b), v, f in zip(muts, g.s.ScoreMany(gm), g.s.ScoreMany(gm, fast=True)):
        assert v == o.score(t, s, b), (t, s, b)
        assert f == o.score(t, s, b, fast=True), (t, s, b)
    conv, nt, na = P.RefineConsensus(g.s)
    ref = o.refine()
    print(name, sum_product, ref)
    assert ref["converged"]
    assert (conv, nt, na) == (ref["converged"], ref["n_tested"], ref["n_applied"])
    assert g.template() == o.template()
    assert [g.s.ReadInfo(k)["active"] for k in range(n)] == [o.read_info(k)["active"] for k in range(n)]
    assert _qvs_exact(P.ConsensusQVs(g.s), o.qvs())

"""Arrow mutations of any width and repeat refinement on the GPU (k_score_wide through the pbccs_scorer_*_ex entry
points, pbccs_refine_repeats and pbccs_polish_batch_ex).

The CPU restatement is frozen and single-base, as the reference's Arrow scorer is, so a wide score has no literal CPU
twin.  Four things pin the kernels: their single-base scores equal the default path's bit for bit (1); its wide scores
agree with the difference of two refills of the CPU restatement within 100 x the gap g1 that single-base scores
show against the same refills (2); scoring is strand-symmetric bit for bit (3); and RefineRepeats repairs the
slipped repeats that the CPU restatement's RefineConsensus stalls on (5).

On the Python scorer a multi-base mutation needs wide=True: without it the scorer refuses it as before."""
import numpy as np
import pytest

from tests import arrow_multibase_common as C
from tests.arrow_multibase_common import DEL, INS, SUB, SNR

pytestmark = pytest.mark.gpu

# python -m tests.arrow_multibase_common g1   (the CPU restatement alone; tests/test_arrow_multibase_cpu.py re-derives it)
#   seed 0 g1 4.294581756880689e-08 excluded [(0, 0, 3)] ['9.962615324467805']
#   seed 6 g1 3.6310581208454096e-09 excluded [(0, 0, 3)] ['9.9783394942109']
G1 = 4.294581756880689e-08
WIDE_TOL = 100 * G1          # a wide extension runs up to six more columns through bands sized for the old template
EXCLUDED_CLASSES = {(INS, 0, 3)}   # insertions at template position 0: their single-base gap is 10 nats


@pytest.fixture(scope="module")
def P():
    import pbccs_amd
    return pbccs_amd


def gpu_on(P, tpl, reads, snr=SNR, engine=None, threshold=None):
    s = P.ArrowMultiReadMutationScorer(P.ArrowConfig(snr), tpl, engine)
    res = [s.AddRead(r["seq"], r["strand"], r["ts"], r["te"], threshold) for r in reads]
    return s, res


def windows(s):
    return [(s.ReadInfo(k)["template_start"], s.ReadInfo(k)["template_end"]) for k in range(s.NumReads())]


# ---- 1. single-base twins, bit for bit -------------------------------------------------------------------------
@pytest.fixture(scope="module")
def twin_case():
    rng = np.random.Generator(np.random.PCG64(11))
    tpl = "".join("ACGT"[int(x)] for x in rng.integers(0, 4, size=64))
    reads = []
    for k in range(5):
        ts, te = (5, 58) if k == 2 else (0, 64)
        if k == 3:   # three bases more than the template
            seq = tpl
            for p in sorted(int(x) for x in rng.integers(5, 60, size=3))[::-1]:
                seq = seq[:p] + "ACGT"[int(rng.integers(0, 4))] + seq[p:]
        else:
            seq = C.noisy(rng, tpl[ts:te])
        strand = k % 2
        reads.append({"seq": C.revcomp(seq) if strand else seq, "strand": strand, "ts": ts, "te": te})
    return tpl, reads


def test_single_base_twins_bit_for_bit(P, twin_case):
    """Every unique single-base mutation: the wide path's per-read scores, sums and fast-threshold sums equal the
    default path's with ==.  Positions 0-2 and J-2..J of the whole and the partial window reach ExtendBeta,
    ExtendAlpha to the end and the middle case on both strands."""
    tpl, reads = twin_case
    s, res = gpu_on(P, tpl, reads)
    assert res == [0] * 5 and len(reads[3]["seq"]) == 67
    muts = [P.Mutation(t, p, b) for t, p, b in C.O.unique_mutations(tpl)]
    assert len(muts) > 400
    assert s.ScoreMany(muts, wide=True) == s.ScoreMany(muts)
    fast = s.config.fast_score_threshold
    assert s.ScoreMany(muts, fast, wide=True) == s.ScoreMany(muts, fast)
    # a threshold the ordered sums do cross, so the read-ordered break is taken at many mutations
    broke = [a != b for a, b in zip(s.ScoreMany(muts, -1.0), s.ScoreMany(muts))]
    assert sum(broke) > 20
    assert s.ScoreMany(muts, -1.0, wide=True) == s.ScoreMany(muts, -1.0)
    for m in muts:
        assert s.Scores(m, wide=True) == s.Scores(m), m
    for m in muts[::37]:
        assert s.Score(m, wide=True) == s.Score(m) and s.FastScore(m, wide=True) == s.FastScore(m)
        assert s.IsFavorable(m, wide=True) == s.IsFavorable(m)
        assert s.FastIsFavorable(m, wide=True) == s.FastIsFavorable(m)


# ---- 2. wide scores against the CPU restatement's refill ------------------------------------------------------
def wide_mutations(P, z, seed):
    """The repeat enumerator's candidates for repeat lengths 2 and 3 plus seeded substitutions, insertions and
    deletions of width 2-4, kept where every read's extension fits eight columns."""
    tpl = z["tpl"]
    rng = np.random.Generator(np.random.PCG64(seed))
    muts = C.repeat_candidates(tpl, 2) + C.repeat_candidates(tpl, 3)
    for _ in range(60):
        w = int(rng.integers(2, 5))
        t = int(rng.integers(0, 3))
        p = int(rng.integers(0, len(tpl) - w))
        bases = "".join("ACGT"[int(x)] for x in rng.integers(0, 4, size=w))
        muts.append(P.Mutation(t, p, bases) if t != DEL else P.Mutation(DEL, p, "-", end=p + w))
    fit = [m for m in muts
           if all(-2 < P.wide_columns_needed(m, r["strand"], r["ts"], r["te"]) <= 8 for r in z["reads"])]
    assert len(fit) >= 50
    return fit


def wide_gaps(P, which, score_diff):
    """Every scored (mutation, read) pair of ZMW `which`: its gap |wide score - refill| or None where the pair is
    left out of the comparison; also checks that every score is finite and Score the read-ordered sum of Scores."""
    z = C.score_zmws()[which]
    tpl, reads = z["tpl"], z["reads"]
    assert len(tpl) == 74
    s = P.ArrowMultiReadMutationScorer(P.ArrowConfig(SNR, score_diff=score_diff), tpl)
    assert [s.AddRead(r["seq"], r["strand"], r["ts"], r["te"]) for r in reads] == [0] * len(reads)

    def lls(t, win=None):
        o = C.O.Scorer(t, SNR, score_diff=score_diff)
        for k, r in enumerate(reads):
            o.add_read(r["seq"], r["strand"], *(win[k] if win else (r["ts"], r["te"])))
        return [(o.read_info(k)["active"], o.read_info(k)["ll"]) for k in range(len(reads))]

    base = lls(tpl)
    out = []
    for m in wide_mutations(P, z, 100 + which):
        got = s.Scores(m, wide=True)
        total = s.Score(m, wide=True)
        assert all(np.isfinite(got)) and np.isfinite(total), (m, got)
        acc = 0.0
        for k in range(len(reads)):   # Score is the read-ordered sum of Scores
            if C.scores_read(m, reads[k]):
                acc += got[k]
        assert total == acc
        t2, mtp = C.apply_wide(tpl, m)
        after = lls(t2, [(mtp[r["ts"]], mtp[r["te"]]) for r in reads])
        for k, r in enumerate(reads):
            if not C.scores_read(m, r):
                assert got[k] == 0.0
                continue
            ok = base[k][0] and after[k][0] and not C.overhangs(m, r) and \
                C.mutation_class(m, len(tpl)) not in EXCLUDED_CLASSES
            out.append((m, k, got[k], abs(got[k] - (after[k][1] - base[k][1])) if ok else None))
    return out


def report(pairs, label):
    gaps = [p for p in pairs if p[3] is not None]
    over = [p for p in gaps if p[3] > WIDE_TOL]
    worst = max(gaps, key=lambda p: p[3])
    print(f"{label}: {len(pairs)} pairs, {len(pairs) - len(gaps)} left out, {len(over)} over the bound "
          f"{WIDE_TOL:.3e}, worst gap {worst[3]:.3e} at {worst[0]} read {worst[1]} (score {worst[2]:.3f})")
    return gaps, over


@pytest.mark.parametrize("which", [0, 1])
def test_wide_scores_against_refill(P, which):
    """At the default ScoreDiff 12.5 every compared pair lies within 100 x g1 of the refill.

    Mutations one or two bases wide are scored through the stored bands (k_score_wide); measured worst gaps 2.7e-07
    and 7.4e-07 (2-base deletions).  Through the stored bands a mutation 3 or 4 bases wide missed the bound (28 and
    30 of 372 pairs, worst 2.6e-03 and 4.8e-03: it moves the likely path 3-4 rows, into cells the fills of the
    unmutated template cut away), so mutations that wide are scored by a refill of the window on the device
    (k_score_wide_refill): measured worst gap 2.0e-09."""
    pairs = wide_gaps(P, which, 12.5)
    gaps, over = report(pairs, f"ZMW {which}, ScoreDiff 12.5")
    assert len(pairs) - len(gaps) <= 0.10 * len(pairs)
    assert not over, [(str(m), k, g) for m, k, _, g in over[:5]]


@pytest.mark.parametrize("which", [0, 1])
def test_wide_scores_against_refill_with_wide_bands(P, which):
    """The same comparison with scorer and refill at ScoreDiff 40, where no band cuts a path either side takes: what
    is left is arithmetic against arithmetic (measured: 5e-14), for the extension path and the refill path alike."""
    pairs = wide_gaps(P, which, 40.0)
    gaps, over = report(pairs, f"ZMW {which}, ScoreDiff 40")
    assert len(pairs) - len(gaps) <= 0.10 * len(pairs)
    assert not over, [(str(m), k, g) for m, k, _, g in over[:5]]


# ---- 3. strand symmetry, bit for bit --------------------------------------------------------------------------
def test_strand_symmetry_bit_for_bit(P, twin_case):
    tpl, reads = twin_case
    L = len(tpl)
    s, _ = gpu_on(P, tpl, reads)
    flipped = [{"seq": r["seq"], "strand": 1 - r["strand"], "ts": L - r["te"], "te": L - r["ts"]} for r in reads]
    f, res = gpu_on(P, C.revcomp(tpl), flipped)
    assert res == [0] * 5
    rng = np.random.Generator(np.random.PCG64(3))
    n = 0
    for _ in range(80):
        w = int(rng.integers(1, 5))
        t = int(rng.integers(0, 3))
        p = int(rng.integers(0, L - w))
        bases = "".join("ACGT"[int(x)] for x in rng.integers(0, 4, size=w))
        m = P.Mutation(t, p, bases) if t != DEL else P.Mutation(DEL, p, "-", end=p + w)
        if not all(-2 < P.wide_columns_needed(m, r["strand"], r["ts"], r["te"]) <= 8 for r in reads):
            continue
        rc = (P.Mutation(t, L - m.end, C.revcomp(bases)) if t != DEL
              else P.Mutation(DEL, L - m.end, "-", end=L - m.start))
        assert s.Scores(m, wide=True) == f.Scores(rc, wide=True), (m, rc)
        n += 1
    assert n >= 40


# ---- 4. apply ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_apply_wide_mutations(P, twin_case, seed):
    tpl, reads = twin_case
    rng = np.random.Generator(np.random.PCG64(seed))
    muts, p = [], 3
    while p < len(tpl) - 8:
        w = int(rng.integers(2, 5))
        t = int(rng.integers(0, 3))
        bases = "".join("ACGT"[int(x)] for x in rng.integers(0, 4, size=w))
        muts.append(P.Mutation(t, p, bases) if t != DEL else P.Mutation(DEL, p, "-", end=p + w))
        p += w + int(rng.integers(6, 14))
    assert len(muts) >= 3
    s, _ = gpu_on(P, tpl, reads)
    want, mtp = P.quiver.ApplyMutations(muts, tpl)
    s.ApplyMutations(muts, wide=True)
    assert s.Template() == want and s.Template(1) == C.revcomp(want)
    assert windows(s) == [(mtp[r["ts"]], mtp[r["te"]]) for r in reads]
    moved = [dict(r, ts=mtp[r["ts"]], te=mtp[r["te"]]) for r in reads]
    fresh, _ = gpu_on(P, want, moved)
    a, b = s.BaselineScores(), fresh.BaselineScores()
    assert len(a) == len(b) and len(a) >= 4
    for x, y in zip(a, b):
        assert abs(x - y) <= 1e-9 * max(abs(x), abs(y))


# ---- 5. RefineRepeats end to end -------------------------------------------------------------------------------
SLIPS = C.load_slips()   # three dinucleotide slips and one trinucleotide slip (the search yields both)


@pytest.mark.parametrize("k", range(len(SLIPS)))
def test_refine_repeats_repairs_the_slip(P, k):
    """RefineConsensus stalls where the CPU restatement's did; RefineRepeats then reaches the truth with one edit;
    a second call applies nothing and reports converged."""
    z = SLIPS[k]
    s, _ = gpu_on(P, z["draft"], z["reads"])
    conv, nt, na = P.RefineConsensus(s)
    assert (conv, nt, na, s.Template()) == (True, z["oracle_n_tested"], z["oracle_n_applied"], z["oracle_final"])
    assert s.Template() != z["truth"]
    conv, nt, na = P.RefineRepeats(s, z["unit_len"])
    assert na == 1 and nt >= 2 and s.Template() == z["truth"]
    conv, nt, na = P.RefineRepeats(s, z["unit_len"])
    assert (conv, na) == (True, 0) and s.Template() == z["truth"]
    if z["unit_len"] == 2:
        assert P.RefineDinucleotideRepeats(s) == (True, nt, 0)


# ---- 6. batch and refusals ----------------------------------------------------------------------------------------
def batch_zmws():
    from pbccs_amd import synth
    slips = [{"draft": z["draft"], "snr": z["snr"], "reads": z["reads"]} for z in SLIPS]
    plain = [{"draft": z["draft"], "snr": z["snr"], "reads": z["reads"]} for z in synth.make_zmws(2, 70, 6, seed=21)]
    return slips + plain


def per_scorer(P, z, repeats, engine=None):
    s, res = gpu_on(P, z["draft"], z["reads"], z["snr"], engine, threshold=-5.0)
    conv, nt, na = P.RefineConsensus(s)
    rec = {"add_read_results": res, "n_tested": nt, "n_applied": na, "converged": conv}
    if conv and repeats:
        _, rec["n_repeat_tested"], rec["n_repeat_applied"] = P.RefineRepeats(s, *repeats)
    rec["consensus"] = s.Template()
    rec["qvs"] = P.ConsensusQVs(s)
    return rec


def test_batch_equals_per_scorer_sequence(P):
    zmws = batch_zmws()
    assert len(zmws) == 6
    eng = P.Engine(0)
    eng.set_profiling(True)
    eng.kernel_stats(reset=True)
    got = P.polish_zmws(zmws, engine=eng, repeats=(2, 3))
    wide = eng.kernel_stats(reset=True)["k_score_wide"]
    eng.set_profiling(False)
    print("repeat round of the batch: k_score_wide", wide)
    assert wide["launches"] >= 1
    repaired = 0
    for z, g in zip(zmws, got):
        e = per_scorer(P, z, (2, 3))
        assert e["converged"] and g["status"] in ("Success", "PoorQuality")
        for key in ("add_read_results", "n_tested", "n_applied", "n_repeat_tested", "n_repeat_applied", "consensus",
                    "qvs"):
            assert g[key] == e[key], key
        repaired += g["n_repeat_applied"]
    assert repaired >= 3 and [g["n_repeat_applied"] for g in got[:3]] == [1, 1, 1]
    assert [g["consensus"] for g in got[:3]] == [z["truth"] for z in SLIPS[:3]]
    assert P.polish_stream(zmws, engine=eng, repeats=(2, 3)) == got
    # without the keyword: today's records, no new keys
    plain = P.polish_zmws(zmws, engine=eng)
    for z, g in zip(zmws, plain):
        e = per_scorer(P, z, None)
        assert "n_repeat_tested" not in g and "n_repeat_applied" not in g
        for key in ("add_read_results", "n_tested", "n_applied", "consensus", "qvs"):
            assert g[key] == e[key], key
    assert [g["consensus"] for g in plain[:4]] == [z["oracle_final"] for z in SLIPS]


def test_refusals_leave_the_scorer_usable(P, twin_case):
    tpl, reads = twin_case
    s, _ = gpu_on(P, tpl, reads)
    probe = P.Mutation(SUB, 20, "A" if tpl[20] != "A" else "C")
    ref, base = s.Score(probe), s.BaselineScore()
    nine = P.Mutation(INS, 1, "ACGTACG")   # ExtendBeta from column 1: 7 + 1 + 1 columns
    assert P.wide_columns_needed(nine, 0, 0, 64) == 9
    bad = [nine, P.Mutation(INS, 30, "ACGTACGT"), P.Mutation(SUB, 20, "AN"), P.Mutation(DEL, 60, "-", end=70)]
    for m in bad:
        for call in (lambda x: s.Score(x, wide=True), lambda x: s.Scores(x, wide=True),
                     lambda x: s.FastIsFavorable(x, wide=True), lambda x: s.ScoreMany([probe, x], wide=True)):
            with pytest.raises(P.PbccsError) as e:
                call(m)
            assert e.value.code == -1
        assert s.BaselineScore() == base and s.Score(probe) == ref
    with pytest.raises(P.PbccsError):   # overlapping edits
        s.ApplyMutations([P.Mutation(DEL, 10, "-", end=13), P.Mutation(SUB, 12, "AC")], wide=True)
    with pytest.raises(P.PbccsError):   # the template stays ACGT
        s.ApplyMutations([P.Mutation(INS, 20, "MN")], wide=True)
    with pytest.raises(P.PbccsError):   # without wide=True a multi-base mutation is refused, as before
        s.Score(P.Mutation(INS, 10, "AC"))
    assert s.Template() == tpl and s.BaselineScore() == base and s.Score(probe, wide=True) == ref


def test_checkpointed_reads_skip_the_repeat_round(P, monkeypatch):
    """With every read on checkpointed bands (PBCCS_CKPT_ALL) k_score_wide has no stored columns to read: the batch
    returns the consensus it returns without the keyword and counts the ZMWs; the single-scorer calls raise."""
    zmws = batch_zmws()[:3]
    monkeypatch.setenv("PBCCS_CKPT_ALL", "8")
    eng = P.Engine(0)
    eng.counters(reset=True)
    got = P.polish_zmws(zmws, engine=eng, repeats=(2, 3))
    assert eng.counters(reset=True)["repeat_skipped_ckpt"] == 3
    plain = P.polish_zmws(zmws, engine=eng)
    for g, p in zip(got, plain):
        assert (g["n_repeat_tested"], g["n_repeat_applied"]) == (0, 0)
        for key in ("status", "consensus", "qvs", "n_tested", "n_applied"):
            assert g[key] == p[key]
    assert [g["consensus"] for g in got] == [z["oracle_final"] for z in SLIPS[:3]]
    s, _ = gpu_on(P, zmws[0]["draft"], zmws[0]["reads"], engine=eng)
    probe = P.Mutation(SUB, 20, "A" if zmws[0]["draft"][20] != "A" else "C")
    ref = s.Score(probe)
    with pytest.raises(P.PbccsError) as e:
        s.Score(P.Mutation(INS, 20, "AC"), wide=True)
    assert e.value.code == -1 and "checkpoint" in str(e.value)
    with pytest.raises(P.PbccsError):
        P.RefineRepeats(s, 2)
    assert s.Score(probe) == ref

"""The ends-free modes on the GPU (pbccs_align_batch_ends: k_align_fill_ends / k_align_trace_ends)
against the restatement (tests/align_modes_restatement.py): transcript, score and extents must be equal.  The shapes
are chosen for where the kernel can go wrong: strip and lane edges with every rows-per-lane, the end cell in the first,
the last and a partly padded lane, in a strip that is not the last, at j = 0 and at (0, 0), ties, raw bytes, a split
workspace.  The cross-kernel checks need no restatement: Align's GLOBAL score on the reported extents, k_map_fill's
placement, and the mapper's own extents."""
import functools
import random

import numpy as np
import pytest

from tests import align_modes_restatement as R
from tests.test_align_gpu import mutated_pair

pytestmark = pytest.mark.gpu

SEMIGLOBAL, LOCAL = R.SEMIGLOBAL, R.LOCAL
MODES = (SEMIGLOBAL, LOCAL)
EDIT, POA = (0, -1, -1, -1), (3, -5, -4, -4)
EOOM = -2


@pytest.fixture(scope="module")
def eng():
    import pbccs_amd
    return pbccs_amd.Engine(0)


@functools.lru_cache(maxsize=None)
def want(t, q, mode, params, both=False):
    tr, score, ext = R.align_ends_np(t, q, mode, params, both)
    return tr, score, (ext["target"], ext["query"], ext["rc"])


def check(eng, pairs, mode, params, both=False):
    """One device call; every pair equal to the restatement and well-formed."""
    from pbccs_amd import align as A
    alns, scores, exts = A.align_ends_batch(pairs, mode, A.AlignParams(*params), both_strands=both, engine=eng)
    assert len(alns) == len(scores) == len(exts) == len(pairs)
    for k, ((t, q), a, s, x) in enumerate(zip(pairs, alns, scores, exts)):
        got = (a.Transcript(), s, (x["target"], x["query"], x["rc"]))
        assert got == want(t, q, mode, params, both), (mode, params, both, k, len(q), len(t))
    return alns, scores, exts


@functools.lru_cache(maxsize=None)
def shaped(qlen, tlen, salt=0):
    """A pair of exactly qlen x tlen that shares a noisy stretch, placed off both ends where there is room."""
    rng = random.Random(qlen * 100003 + tlen * 17 + salt)
    core = min(qlen, tlen)
    flank_q, flank_t = qlen - core, tlen - core
    t_core, q_core = mutated_pair(rng, core, core, rate=0.12)
    rnd = lambda n: "".join(rng.choice("ACGT") for _ in range(n))  # noqa: E731
    a, b = rng.randint(0, flank_q), rng.randint(0, flank_t)
    return rnd(b) + t_core + rnd(flank_t - b), rnd(a) + q_core + rnd(flank_q - a)


QUERY_LENS = (1, 2, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1025)   # 1025: three strips at R = 8
TARGET_LENS = (1, 63, 64, 65)


# ---- 1. strip and lane edges ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("params", (EDIT, POA))
@pytest.mark.parametrize("mode", MODES)
def test_strip_and_lane_edges(eng, mode, params):
    pairs = [shaped(I, J) for I in QUERY_LENS for J in TARGET_LENS]
    pairs += [shaped(I, 300 + (37 * k) % 401) for k, I in enumerate(QUERY_LENS)]   # targets of 300..700
    check(eng, pairs, mode, params)


@pytest.mark.parametrize("rows", (2, 4, 8))
@pytest.mark.parametrize("mode", MODES)
def test_strip_edges_forced_rows_per_lane(eng, monkeypatch, mode, rows):
    monkeypatch.setenv("PBCCS_ALIGN_ROWS_PER_LANE", str(rows))
    strip = 64 * rows
    pairs = [shaped(I, J, salt=rows) for I in (strip - 1, strip, strip + 1, 2 * strip, 2 * strip + 1) for J in (65, 150)]
    check(eng, pairs, mode, POA)
    check(eng, pairs[::3], mode, POA, both=True)


# ---- 2. where the end cell lies -----------------------------------------------------------------------------------
def planted(tlen, qlen, at, motif, seed):
    """A target of random ACGT and a query of N (which matches nothing) with target[40:40 + motif] planted at row
    `at`: the LOCAL end cell is the motif's last row."""
    rng = random.Random(seed)
    t = "".join(rng.choice("ACGT") for _ in range(tlen))
    q = "N" * at + t[40:40 + motif] + "N" * (qlen - at - motif)
    assert len(q) == qlen
    return t, q


def test_end_cell_placement(eng):
    pairs = [
        planted(200, 102, 0, 2, 1),        # R = 2: the end cell in lane 0
        planted(200, 128, 126, 2, 2),      # R = 2: in lane 63, the strip's last row
        planted(200, 129, 119, 10, 3),     # R = 4: row 129 shares lane 32 with three padded rows
        planted(200, 130, 118, 12, 4),     # R = 4: the last real row next to padded rows, lane 33 all padded
        planted(300, 1025, 100, 60, 5),    # R = 8: in strip 0 of three
        planted(300, 1025, 500, 60, 6),    # R = 8: across the first strip boundary
        planted(300, 1025, 965, 60, 7),    # R = 8: in the last strip's only row
    ]
    _, scores, exts = check(eng, pairs, LOCAL, POA)
    assert exts[0]["query"][1] == 2 and exts[1]["query"][1] == 128 and exts[2]["query"][1] == 129
    assert exts[4]["query"] == (100, 160) and exts[5]["query"] == (500, 560) and exts[6]["query"] == (965, 1025)
    assert scores[4:] == [180, 180, 180]
    check(eng, pairs, SEMIGLOBAL, POA)
    check(eng, pairs, SEMIGLOBAL, EDIT)
    # a padded row gains Mismatch > 0 with every column and must never win
    check(eng, pairs[:4] + [shaped(129, 300), shaped(1, 64), shaped(513, 80)], LOCAL, (2, 1, -1, -1))
    check(eng, pairs[:4] + [shaped(129, 300), shaped(513, 80)], SEMIGLOBAL, (2, 1, -1, -1))


def test_end_cell_on_the_borders(eng):
    harsh = (0, -9, -1, -1)
    nothing = [("C" * 70, "A" * 5), ("C" * 70, "A" * 130), ("C" * 7, "A" * 600), ("ACGT" * 20, "N" * 257)]
    _, scores, exts = check(eng, nothing, SEMIGLOBAL, harsh)     # all Extra down column 0: the end cell at j = 0
    assert [x["target"] for x in exts] == [(0, 0)] * 4 and scores == [-5, -130, -600, -257]
    for params in (EDIT, POA):
        _, scores, exts = check(eng, nothing, LOCAL, params)     # nothing positive: the (0, 0) Start cell
        assert scores == [0] * 4 and all(x == {"target": (0, 0), "query": (0, 0), "rc": False} for x in exts)
    check(eng, [shaped(130, 200), shaped(300, 64)], LOCAL, EDIT)  # a real pair under edit distance: still (0, 0)
    # degenerate pairs are answered on the host, in batch order
    from pbccs_amd import align as A
    mixed = [("", "ACG"), ("ACG", ""), ("", ""), ("GATTACA", "TTAC")]
    alns, scores, exts = check(eng, mixed, SEMIGLOBAL, EDIT)
    assert [a.Transcript() for a in alns] == ["III", "", "", "MMMM"] and scores == [-3, 0, 0, 0]
    alns, scores, exts = check(eng, mixed, LOCAL, POA)
    assert [a.Transcript() for a in alns] == ["", "", "", "MMMM"] and scores == [0, 0, 0, 12]
    assert A.align_ends_batch([], LOCAL, engine=eng) == ([], [], [])


# ---- 3. ties --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("params", (EDIT, POA, (2, -3, 0, -1)))
@pytest.mark.parametrize("mode", MODES)
def test_tie_heavy_batch(eng, mode, params):
    pairs = [("A" * n, "A" * m) for n, m in ((4, 2), (2, 4), (64, 64), (200, 129), (130, 300), (65, 513))]
    pairs += [("AC" * n, "CA" * m) for n, m in ((3, 2), (40, 64), (100, 65), (33, 300))]
    pairs += [("AAC" * 50, "ACC" * 43), ("ACGT" * 40, "TGCA" * 33), ("A" * 100 + "C" * 100, "C" * 70 + "A" * 70)]
    check(eng, pairs, mode, params)
    check(eng, pairs[:8], mode, params, both=True)


# ---- 4. raw bytes ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
def test_lowercase_and_n(eng, mode):
    rng = random.Random(4)
    pairs = [mutated_pair(rng, I, J, alphabet="ACGTacgtN") for I, J in ((60, 90), (129, 140), (300, 200))]
    pairs += [("ACGTACGTNNNNacgtacgt", "acgtNNNNACGT"), ("NNNNNNNN", "NNNN"), ("acgt" * 10, "ACGT" * 10)]
    for params in (EDIT, POA):
        check(eng, pairs, mode, params)
        check(eng, pairs, mode, params, both=True)   # n <-> m, N <-> M under the complement


# ---- 5. the workspace split, the stats --------------------------------------------------------------------------------
def test_workspace_split_and_oversize_pair(monkeypatch):
    import pbccs_amd
    from pbccs_amd import align as A
    eng = pbccs_amd.Engine(0)
    distinct = [shaped(300, 300, salt=k) for k in range(6)]
    pairs = [distinct[k % 6] for k in range(24)]
    A.align_stats(eng, reset=True)
    whole, _, _ = check(eng, pairs, LOCAL, POA)
    st = A.align_stats(eng, reset=True)
    assert st["groups"] == 1 and st["launches"] == 1 and st["pairs"] == 24 and st["cells"] == 24 * 300 * 300
    assert st["bytes"] == 24 * 363 * 512 and st["trace_steps"] == sum(a.Length() for a in whole)
    monkeypatch.setenv("PBCCS_ALIGN_WORKSPACE_MB", "1")   # one 300 x 300 pair's move store is 363 * 512 bytes
    for mode in MODES:
        check(eng, pairs, mode, POA)
        st = A.align_stats(eng, reset=True)
        assert st["groups"] >= 4 and st["launches"] == st["groups"] and st["pairs"] == 24
    check(eng, pairs[:7], LOCAL, POA, both=True)
    st = A.align_stats(eng, reset=True)
    assert st["pairs"] == 7 and st["cells"] == 2 * 7 * 300 * 300 and st["groups"] >= 2
    # 513 x 2000 at R = 8: 2 strips x 2063 steps x 512 bytes > 1 MB
    with pytest.raises(pbccs_amd.PbccsError) as e:
        A.align_ends_batch([pairs[0], ("ACGT" * 500, "ACGA" * 128 + "A"), pairs[1]], SEMIGLOBAL, engine=eng)
    assert e.value.code == EOOM
    assert A.align_stats(eng, reset=True)["cells"] == 2 * 300 * 300   # no device work for the oversize pair
    monkeypatch.delenv("PBCCS_ALIGN_WORKSPACE_MB")
    check(eng, pairs[:3], SEMIGLOBAL, EDIT)


def test_c_entry_refusals_and_short_cap(eng):
    """pbccs_align_batch_ends itself: PBCCS_EINVAL before any device work, PBCCS_ERANGE with len set."""
    import ctypes
    from pbccs_amd import align as A
    from pbccs_amd import lib as L
    fn = L.load().pbccs_align_batch_ends
    t, q = b"TTGATTACATT", b"GATTACA"
    pair = L.CAlignPair(t, len(t), q, len(q))
    buf = ctypes.create_string_buffer(32)

    def call(kind=0, mode=LOCAL, insert=-4, delete=-4, cap=32):
        p = L.CAlignParams()
        p.kind, p.mode, p.match, p.mismatch, p.insert, p.delete_ = kind, 0, 3, -5, insert, delete
        e = L.CAlignEnds(mode, 0)
        out = L.CAlignResult(ctypes.cast(buf, ctypes.c_char_p), cap, 0, 0, 0.0, 0)
        x = L.CAlignExtent()
        rc = fn(eng._h, ctypes.byref(p), ctypes.byref(e), ctypes.byref(pair), 1, ctypes.byref(out), ctypes.byref(x))
        return rc, out, x

    A.align_stats(eng, reset=True)
    for bad in (dict(kind=1), dict(kind=2), dict(mode=0), dict(mode=3), dict(insert=1), dict(delete=1)):
        assert call(**bad)[0] == -1, bad
    assert A.align_stats(eng, reset=True)["pairs"] == 0
    rc, out, x = call()
    assert rc == 0 and buf.raw[:out.len] == b"MMMMMMM" and out.score_i == 21 and out.status == 0
    assert (x.target_begin, x.target_end, x.query_begin, x.query_end, x.rc) == (2, 9, 0, 7, 0)
    rc, out, x = call(cap=3)
    assert rc == -5 and out.status == -5 and out.len == 7


# ---- 6. coexistence with the polish -----------------------------------------------------------------------------------
def test_polish_is_unchanged_by_the_modes_on_the_same_engine():
    import pbccs_amd
    from pbccs_amd import synth
    eng = pbccs_amd.Engine(0)
    zmws = synth.make_zmws(4, 300, 6, seed=2024)
    before = pbccs_amd.polish_zmws(zmws, engine=eng)
    pairs = [shaped(200, 210, salt=k) for k in range(8)]
    check(eng, pairs, SEMIGLOBAL, EDIT)
    check(eng, pairs, LOCAL, POA, both=True)
    after = pbccs_amd.polish_zmws(zmws, engine=eng)
    assert before == after


# ---- 7. cross-kernel checks -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("params", (EDIT, POA))
@pytest.mark.parametrize("mode", MODES)
def test_score_is_aligns_global_score_on_the_extents(eng, mode, params):
    from pbccs_amd import align as A
    pairs = [shaped(I, J, salt=9) for I, J in ((40, 300), (129, 200), (257, 257), (300, 90), (513, 600))]
    _, scores, exts = A.align_ends_batch(pairs, mode, A.AlignParams(*params), engine=eng)
    subs = [(t[x["target"][0]:x["target"][1]], q[x["query"][0]:x["query"][1]]) for (t, q), x in zip(pairs, exts)]
    _, glob = A.align_batch(subs, A.NW, A.AlignConfig(A.AlignParams(*params)), engine=eng)
    assert scores == glob
    if mode == SEMIGLOBAL:
        assert [x["query"] for x in exts] == [(0, len(q)) for _, q in pairs]


@functools.lru_cache(maxsize=None)
def zmw_reads():
    from pbccs_amd import synth
    z = synth.make_zmw(np.random.default_rng(11), 300, 6)
    return z["draft"], tuple(r["seq"] for r in z["reads"])


def test_local_both_strands_equals_map_batch(eng):
    from pbccs_amd import align as A
    from pbccs_amd import mapping
    draft, reads = zmw_reads()
    placed = mapping.map_batch([(draft, list(reads))], engine=eng)[0]
    _, scores, exts = A.align_ends_batch([(draft, r) for r in reads], LOCAL, A.AlignParams(*POA), both_strands=True,
                                         engine=eng)
    assert all(m is not None for m in placed) and {m["rc"] for m in placed} == {False, True}
    for m, s, x in zip(placed, scores, exts):
        assert (m["rc"], m["score"], m["read"], m["tpl"]) == (x["rc"], s, x["query"], x["target"])


def test_map_batch_transcripts_consume_their_own_extents(eng):
    from pbccs_amd import align as A
    from pbccs_amd import mapping
    draft, reads = zmw_reads()
    plain = mapping.map_batch([(draft, list(reads) + [None])], engine=eng)[0]
    got = mapping.map_batch([(draft, list(reads) + [None])], engine=eng, transcripts=True)[0]
    assert got[-1] is None and plain[-1] is None
    assert all("transcript" not in m for m in plain[:-1])
    for r, m, p in zip(reads, got, plain):
        assert {k: v for k, v in m.items() if k != "transcript"} == p
        seq = A.reverse_complement(r) if m["rc"] else r
        a = A.PairwiseAlignment.FromTranscript(m["transcript"], draft[m["tpl"][0]:m["tpl"][1]],
                                               seq[m["read"][0]:m["read"][1]])
        assert a is not None and a.Matches() * 3 - a.Mismatches() * 5 - (a.Insertions() + a.Deletions()) * 4 == m["score"]
    one = mapping.map_to_draft(draft, reads[:2], engine=eng, transcripts=True)
    assert [m["transcript"] for m in one] == [m["transcript"] for m in got[:2]]


# ---- 8. one use: the adapter inside a fused read ------------------------------------------------------------------------
@pytest.mark.parametrize("params", (EDIT, POA))
def test_adapter_is_found_between_the_passes(eng, params):
    from pbccs_amd import align as A
    from pbccs_amd import synth
    fused = []
    for seed in range(12):
        rng = np.random.default_rng(seed)
        truth = synth.BASES[rng.integers(0, 4, size=200)].tobytes().decode()
        fused.append(synth.make_fused_read(rng, truth, 2))
    for seed, f in enumerate(fused):
        a, score, x = A.AlignSemiglobal(f["seq"], synth.ADAPTER, A.AlignParams(*params), engine=eng)
        (_, gap_begin, _), (gap_end, _, _) = f["passes"]
        print(seed, params, x["target"], (gap_begin, gap_end), score)
        assert x["query"] == (0, len(synth.ADAPTER))
        assert abs(x["target"][0] - gap_begin) <= 8 and abs(x["target"][1] - gap_end) <= 8, (seed, x, f["passes"])

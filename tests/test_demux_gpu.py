"""Barcode demultiplexing on the GPU (pbccs_demux_batch: k_demux_score, k_demux_call, k_demux_extent; DESIGN.md
§3.27) against the restatement (tests/demux_restatement.py): the full score matrix, the winners and the extents must
be equal.  The shapes are chosen for where the kernels can go wrong: the padding and LMAX edges of the barcode
lengths, the lane-pass edges of the barcode count, windows shorter than a barcode, overlapping windows, raw bytes,
ties.  The cross-kernel checks need no restatement: align_ends_batch(SEMIGLOBAL) on the same pairs, a split
workspace, the cell count."""
import functools

import numpy as np
import pytest

import align_modes_restatement as AM
import demux_restatement as R

pytestmark = pytest.mark.gpu

PARAMS = [(3, -5, -4, -4), (1, -1, -1, -1), (4, -13, -7, -7)]
MIXED_LENS = (1, 2, 15, 16, 17, 31, 32, 33, 63, 64)     # the padding and LMAX edges


@pytest.fixture(scope="module")
def eng():
    import pbccs_amd
    return pbccs_amd.Engine(0)


def rand_seq(rng, n, alphabet="ACGT"):
    return "".join(alphabet[k] for k in rng.integers(0, len(alphabet), n))


@functools.lru_cache(maxsize=None)
def barcode_set(name):
    rng = np.random.default_rng(sum(name.encode()))
    if name == "mixed":
        return tuple(rand_seq(rng, k) for k in MIXED_LENS)
    if name.startswith("longest"):                       # longest16 / longest32 / longest64: the last row is LMAX
        top = int(name[7:])
        B = {16: 63, 32: 64, 64: 65}[top]
        lens = [top] + [int(rng.integers(max(1, top // 2), top + 1)) for _ in range(B - 1)]
        return tuple(rand_seq(rng, k) for k in lens)
    return tuple(rand_seq(rng, 16) for _ in range(int(name[1:])))   # b1 / b129: B 16-mers


@functools.lru_cache(maxsize=None)
def reads_for(name, W):
    """Read lengths 0, 1, one less than a barcode, W, W + 1, 2 W - 1 (overlapping windows) and 400, with planted and
    mutated barcodes, lowercase and N."""
    rng = np.random.default_rng(W * 7 + sum(name.encode()))
    bc = barcode_set(name)
    longest = max(len(b) for b in bc)
    out = []
    for n in sorted({0, 1, max(0, longest - 1), W, W + 1, 2 * W - 1, 400}):
        i, j = int(rng.integers(0, len(bc))), int(rng.integers(0, len(bc)))
        flanked = bc[i] + rand_seq(rng, max(0, n - len(bc[i]) - len(bc[j]))) + R.revcomp(bc[j])
        out += [rand_seq(rng, n), flanked[:n] if n >= len(flanked) else rand_seq(rng, n, "AC")]
    noisy = list(bc[0] + rand_seq(rng, 100) + R.revcomp(bc[-1]))
    for k in range(0, len(noisy), 9):
        noisy[k] = "N" if k % 2 else noisy[k].lower()
    return tuple(out + ["".join(noisy), "acgt" * 20, "N" * 70])


def check(eng, reads, barcodes, params=R.DEFAULT_PARAMS, **kw):
    """One device call; the score matrix and every entry equal the restatement's."""
    from pbccs_amd import demux
    from pbccs_amd.align import AlignParams
    reads, barcodes = list(reads), list(barcodes)
    got, scores = demux.demux_batch(reads, barcodes, params=AlignParams(*params), return_scores=True, engine=eng, **kw)
    W = R.window_of(barcodes, kw.get("window"), kw.get("window_mult", 3))
    S = R.scores_np(reads, barcodes, W, params)
    assert scores.shape == S.shape
    bad = np.argwhere(scores != S)
    assert bad.size == 0, (bad[:5].tolist(), scores[tuple(bad[0])], S[tuple(bad[0])])
    rkw = dict(kw)
    rkw["min_quality"] = demux.MIN_QUALITY if kw.get("min_quality") is None else kw["min_quality"]
    for k, r in enumerate(reads):
        want = R.demux_one(r, barcodes, params, scores=(S[k, 0].tolist(), S[k, 1].tolist()), **rkw)
        assert got[k] == want, (k, len(r))
    # without the matrix: the same entries
    assert demux.demux_batch(reads, barcodes, params=AlignParams(*params), engine=eng, **kw) == got
    return got, scores


# ---- 1. the full score matrix ---------------------------------------------------------------------------------------
CONFIGS = [("mixed", 1), ("mixed", 16), ("mixed", 48), ("mixed", 1024), ("longest16", 48), ("longest32", 48),
           ("longest64", 48), ("b1", 48), ("b129", 48)]


@pytest.mark.parametrize("params", PARAMS)
@pytest.mark.parametrize("name,W", CONFIGS)
def test_score_matrix_winners_and_extents_equal_the_restatement(eng, name, W, params):
    check(eng, reads_for(name, W), barcode_set(name), params, window=W)


def test_default_window_is_three_times_the_longest_barcode(eng):
    bc = barcode_set("longest16")
    got, _ = check(eng, reads_for("longest16", 48), bc)
    assert got == check(eng, reads_for("longest16", 48), bc, window=48)[0]
    check(eng, reads_for("longest16", 48)[:6], bc, window_mult=1)


# ---- 2. winners -----------------------------------------------------------------------------------------------------
def tie_cases():
    """Duplicated barcodes and tie-heavy windows."""
    rng = np.random.default_rng(77)
    uniq = [rand_seq(rng, 12) for _ in range(40)]
    bc = [uniq[k % 40] for k in range(130)]               # every barcode at least three times, across lane passes
    bc[64], bc[3] = "AAAAAAAAAAAA", "ACACACACACAC"
    reads = ["A" * 60, "AC" * 40, "A" * 11, "CA" * 5 + "C", "T" * 50,
             uniq[39] + rand_seq(rng, 80) + R.revcomp(uniq[39]), uniq[7] + "A" * 70 + R.revcomp(uniq[2]),
             "AAAAAAAAAAAA" + "G" * 40 + "TTTTTTTTTTTT", "ACACACACACAC" + "G" * 30 + "GTGTGTGTGTGT"]
    return reads, bc


@pytest.mark.parametrize("design", ["asymmetric", "symmetric"])
def test_winners_with_duplicates_and_ties(eng, design):
    reads, bc = tie_cases()
    got, _ = check(eng, reads, bc, design=design, min_quality=0)
    planted = got[5]
    assert planted["lead"] == planted["trail"] == 39 and planted["score_lead"] == 0   # 39, 79 and 119 are equal
    assert planted["second"] == (36, 36) and planted["called"]
    assert not check(eng, reads, bc, design=design, min_quality=0, min_score_lead=1)[0][5]["called"]


@pytest.mark.parametrize("design", ["asymmetric", "symmetric"])
def test_one_barcode(eng, design):
    reads = ["ACGTACGTAC" + "G" * 50 + "GTACGTACGT", "T" * 30, "", "ACG"]
    got, _ = check(eng, reads, ["ACGTACGTAC"], design=design, min_score_lead=1000)
    assert got[0]["called"] and got[0]["pair"] == (0, 0) and got[0]["score_lead"] == 2**31 - 1
    assert got[0]["second"] == (None, None) and not got[1]["called"] and got[1]["pair"] == (-1, -1)


# ---- 3. extents -------------------------------------------------------------------------------------------------------
def test_symmetric_call_that_is_no_end_s_best(eng):
    rng = np.random.default_rng(21)
    x, y, z = (rand_seq(rng, 16) for _ in range(3))
    x1 = x[:5] + ("A" if x[5] != "A" else "C") + x[6:]
    x2 = x[:11] + ("G" if x[11] != "G" else "T") + x[12:]
    read = "TT" + y + "GG" + x1 + rand_seq(rng, 120) + R.revcomp(x2) + "CC" + R.revcomp(z)
    bc = [y, z, x] + [rand_seq(rng, 16) for _ in range(70)]
    got, _ = check(eng, [read, read[:90]], bc, design="symmetric", window=48)
    e = got[0]
    assert e["lead"] == e["trail"] == 2 and e["best"][0][0] == 0 and e["best"][1][0] == 1
    assert e["lead_extent"] == (20, 36) and e["trail_extent"] == (len(read) - 34, len(read) - 18)
    a = check(eng, [read], bc, design="asymmetric", window=48)[0][0]
    assert (a["lead"], a["trail"]) == (0, 1) and a["lead_extent"] == (2, 18)


def test_overlapping_windows_and_homopolymer_ties(eng):
    bc = ["AAAAAAAA", "AAAA", "ACACACAC", "TTTTTTTT", "ACGTACGT", "A"]
    reads = ["ACGTAC", "A" * 5, "A" * 9, "AAAACAAAA", "ACGTACGT", "ACGTACGTT", "AC" * 7, "A" * 23, "AAAATTTT",
             "TTTTAAAA", "CAAAAAAAAC", "ACGTACGTAAAAAAAA"]
    for W in (8, 12):
        for design in ("asymmetric", "symmetric"):
            got, _ = check(eng, reads, bc, window=W, design=design, min_quality=0)
            assert any(e["overlap"] and e["clip"] is None for e in got)
            assert any(not e["overlap"] for e in got)
    got, _ = check(eng, ["A" * 20 + "T" * 20, "C" + "A" * 30], ["AAAA"], window=16, min_quality=0)
    assert got[0]["lead_extent"] == (0, 4) and got[0]["trail_extent"] == (24, 28)   # the first maximum, walked back
    assert got[1]["lead_extent"] == (1, 5)


# ---- 4. cross-kernel, no restatement ---------------------------------------------------------------------------------
def test_align_ends_batch_returns_the_same_scores_and_extents(eng):
    from pbccs_amd import align as A
    from pbccs_amd import demux
    bc = list(barcode_set("mixed"))
    reads = [r for r in reads_for("mixed", 48) if r]
    W = 48
    got, scores = demux.demux_batch(reads, bc, window=W, return_scores=True, engine=eng)
    pairs, where = [], []
    for k, r in enumerate(reads):
        off = max(0, len(r) - W)
        for b in sorted({got[k]["lead"], got[k]["trail"], k % len(bc)}):
            pairs += [(r[:W], bc[b]), (r[off:], A.reverse_complement(bc[b]))]
            where += [(k, 0, b, 0), (k, 1, b, off)]
    _, s, x = A.align_ends_batch(pairs, A.SEMIGLOBAL, demux.default_params(), engine=eng)
    for (k, e, b, off), sc, ext in zip(where, s, x):
        assert scores[k, e, b] == sc
        if b == got[k]["trail" if e else "lead"]:
            assert got[k]["trail_extent" if e else "lead_extent"] == (off + ext["target"][0], off + ext["target"][1])


def test_a_split_workspace_gives_the_same_answer_and_the_stats_count_cells(eng, monkeypatch):
    from pbccs_amd import demux
    bc = list(barcode_set("b129"))
    reads = list(reads_for("b129", 48))
    demux.demux_stats(eng, reset=True)
    whole, ws = demux.demux_batch(reads, bc, window=48, return_scores=True, engine=eng)
    one = demux.demux_stats(eng, reset=True)
    assert one["reads"] == len(reads) and one["launches"] == 3
    assert one["cells"] == sum(2 * min(48, len(r)) * 16 * 129 for r in reads)
    for design in ("asymmetric", "symmetric"):
        want = demux.demux_batch(reads, bc, window=48, design=design, engine=eng)
        demux.demux_stats(eng, reset=True)
        monkeypatch.setenv("PBCCS_DEMUX_WORKSPACE_KB", "4")      # 1 KB of score rows per read: a few reads a launch
        parts, ps = demux.demux_batch(reads, bc, window=48, design=design, return_scores=True, engine=eng)
        monkeypatch.delenv("PBCCS_DEMUX_WORKSPACE_KB")
        many = demux.demux_stats(eng, reset=True)
        assert parts == want and (ps == ws).all()
        assert many["launches"] > 3 * 3 and many["cells"] == one["cells"]
    assert whole == demux.demux_batch(reads, bc, window=48, engine=eng)


# ---- 5. the driver ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def barcoded_zmws():
    from pbccs_amd import synth
    rng = np.random.Generator(np.random.PCG64(2027))
    bc = tuple(rand_seq(rng, 16) for _ in range(16))
    pairs = [(int(rng.integers(0, 16)), int(rng.integers(0, 16))) for _ in range(24)]
    return bc, tuple(synth.make_barcoded_zmw(rng, 300, 8, bc, p) for p in pairs)


def test_ccs_batch_calls_the_planted_pairs(eng):
    from pbccs_amd import demux, driver
    bc, zmws = barcoded_zmws()
    for z in zmws:                                        # on the CPU first: the truth itself is called right
        e = R.demux_one(z["truth"], list(bc), min_quality=demux.MIN_QUALITY)
        assert e["called"] and (e["lead"], e["trail"]) == z["pair"] and z["truth"][e["clip"][0]:e["clip"][1]] == z["insert"]
    chunks = [{"snr": z["snr"], "reads": [{"seq": r["seq"]} for r in z["reads"]]} for z in zmws]
    plain = driver.ccs_batch(chunks, engine=eng)
    got = driver.ccs_batch(chunks, engine=eng, barcodes=demux.BarcodeSet(bc))
    assert [{k: v for k, v in g.items() if k != "barcode"} for g in got] == plain   # nothing else changes
    ok = [k for k, g in enumerate(got) if g["status"] == "Success"]
    assert len(ok) >= 20 and all(("barcode" in g) == (g["status"] == "Success") for g in got)
    again = demux.demux_batch([got[k]["consensus"] for k in ok], list(bc), engine=eng)
    for k, e in zip(ok, again):
        g, z = got[k], zmws[k]
        assert g["barcode"] == e
        assert e["called"] and e["pair"] == tuple(sorted(z["pair"]))
        # the consensus comes out on either strand: on the reverse one the two ends have changed places
        fwd = -AM.global_score(z["truth"], g["consensus"], (0, -1, -1, -1)) <= 8
        assert (e["lead"], e["trail"]) == (z["pair"] if fwd else z["pair"][::-1])
        insert = demux.clip_read(g["consensus"], e)
        assert -AM.global_score(z["insert"] if fwd else R.revcomp(z["insert"]), insert, (0, -1, -1, -1)) <= 2
    # beside another option the entries come from a call of their own, and the keywords reach it
    spec = driver.ccs_batch(chunks[:6], engine=eng, rich_qvs=True,
                            barcodes={"barcodes": list(bc), "design": "symmetric", "min_quality": 0})
    for g, p in zip(spec, got):
        if g["status"] == "Success":
            assert g["consensus"] == p["consensus"] and "sub_qv" in g
            assert g["barcode"] == demux.demux_batch([g["consensus"]], list(bc), design="symmetric", min_quality=0,
                                                     engine=eng)[0]
            assert g["barcode"]["lead"] == g["barcode"]["trail"]

"""MapToDraft on the GPU (pbccs_map_batch / k_map_fill) and the capped ccs that keeps every pass
(pbccs_ccs_batch_ex, map_past_cap).  The yardstick is the oracle's SparsePoa holding the draft twice and then the
read (test_map_cpu.oracle_map): orientation and both extents are compared for equality."""
import math
import random
import threading

import pytest

from oracle import oracle as O
from test_map_cpu import (OraclePoa, edge_cases, noisy, oracle_map, revcomp, seeded_cases, summary_of)

pytestmark = pytest.mark.gpu

ROWS_PER_LANE = (4, 8, 16)   # map_kernels.hpp's kRowsPerLane


@pytest.fixture(scope="module")
def M():
    import pbccs_amd
    from pbccs_amd import mapping
    eng = pbccs_amd.Engine(0)
    mapping.map_stats(eng, reset=True)
    return mapping, eng


def _rand(rng, n, alphabet="ACGT"):
    return "".join(rng.choice(alphabet) for _ in range(n))


_RNG = random.Random(31)
DRAFT = _rand(_RNG, 300)
_EXPECTED = {}


def _expect(draft, read):
    """The oracle's summary, computed once per (draft, read)."""
    key = (draft, read)
    if key not in _EXPECTED:
        css, s = oracle_map(draft, read)
        assert css == draft
        _EXPECTED[key] = s
    return _EXPECTED[key]


def _read_of_length(rng, n):
    """A read of exactly n bases that carries a noisy copy of (a window of) DRAFT between random flanks."""
    if n <= 3:
        return DRAFT[100:100 + n]
    core = noisy(rng, DRAFT[20:280] if n > 400 else DRAFT[20:20 + max(1, 2 * n // 3)])[:n]
    lead = (n - len(core)) // 2
    read = _rand(rng, lead) + core + _rand(rng, n - len(core) - lead)
    return revcomp(read) if rng.random() < 0.5 else read


def _check(M, pairs, **kw):
    mapping, eng = M
    by_draft = {}
    for d, r in pairs:
        by_draft.setdefault(d, []).append(r)
    got = mapping.map_batch(list(by_draft.items()), engine=eng, **kw)
    for (d, reads), res in zip(by_draft.items(), got):
        for r, g in zip(reads, res):
            assert summary_of(g) == _expect(d, r), (len(d), len(r), g, _expect(d, r))


def test_lane_and_strip_edges(M):
    """Every compiled R at 64 R - 1, 64 R, 64 R + 1 rows (the last of them is the next R, or two strips), the first
    lane's edges, and a read of three strips."""
    rng = random.Random(1)
    lengths = [1, 63, 64, 65] + [64 * r + d for r in ROWS_PER_LANE for d in (-1, 0, 1)] + [2 * 64 * 16 + 1]
    assert 64 * ROWS_PER_LANE[-1] + 1 in lengths
    _check(M, [(DRAFT, _read_of_length(rng, n)) for n in lengths])


@pytest.mark.parametrize("rows", ROWS_PER_LANE)
def test_strips_with_every_rows_per_lane(M, monkeypatch, rows):
    """PBCCS_MAP_ROWS_PER_LANE forces R: one, two and three strips, and the strip edges, with each kernel."""
    monkeypatch.setenv("PBCCS_MAP_ROWS_PER_LANE", str(rows))
    rng = random.Random(rows)
    s = 64 * rows
    _check(M, [(DRAFT, _read_of_length(rng, n)) for n in (s - 1, s, s + 1, 2 * s, 2 * s + 1, 3 * s - 1)])


def test_short_drafts(M):
    rng = random.Random(2)
    read = _rand(rng, 100)
    pairs = []
    for n in (1, 2, 63, 64, 65):
        d = read[17:17 + n]
        pairs += [(d, read), (d, revcomp(read))]
    _check(M, pairs)


def test_ties(M):
    rng = random.Random(3)
    d = _rand(rng, 120)
    half = _rand(rng, 60)
    pal = half + revcomp(half)
    pairs = [("A" * 150, "A" * 40), ("A" * 150, noisy(rng, "A" * 90, alphabet="AC")),
             ("AC" * 80, "AC" * 30), ("AC" * 80, noisy(rng, "CA" * 50, alphabet="AC")),
             (_rand(rng, 140, "AG"), _rand(rng, 90, "AG")),
             (d, revcomp(d)), (pal, pal[20:100]), (pal, noisy(rng, pal)),
             ("A" * 30, "C" * 12)]
    _check(M, pairs + edge_cases() + seeded_cases(24, seed=99))
    mapping, eng = M
    assert mapping.map_to_draft("A" * 30, ["C" * 12], engine=eng) == [
        {"rc": False, "read": (0, 0), "tpl": (0, 0), "score": 0}]


def test_alignment_starts_and_ends_on_lane_and_strip_rows(M):
    """An exact copy of a draft window between flanks that match nothing puts the first and the last Match on chosen
    rows: a lane's first and last row, and the rows either side of a strip boundary."""
    rng = random.Random(4)
    draft = _rand(rng, 300, "AC")
    win = draft[40:240]
    pairs = []
    for total, edges in ((250, (3, 4, 5, 7, 8, 9)), (1100, (1023, 1024, 1025)), (2100, (2047, 2048, 2049))):
        for e in edges:
            pairs.append((draft, "G" * e + win + "G" * (total - e - len(win))))           # first Match on row e + 1
        for e in edges:
            if e > len(win):
                pairs.append((draft, "G" * (e - len(win)) + win + "G" * (total - e)))     # last Match on row e
    for d, r in pairs:
        s = _expect(d, r)
        assert s["read"][1] - s["read"][0] == len(win) and not s["rc"]
    _check(M, pairs)


def test_min_score_to_add(M):
    """Against the product's own SparsePoa holding [draft, draft]: OrientAndAddRead(read, min_score) gives key -1 if
    and only if the read is not mapped."""
    mapping, eng = M
    from pbccs_amd import poa
    rng = random.Random(5)
    draft = _rand(rng, 200)
    reads = [draft[50:60], revcomp(draft[50:60]), draft[10:110], _rand(rng, 40), noisy(rng, draft[30:90])]
    for min_score in (29.0, 30.0, 30.5, 120.0, 1000.0):
        got = mapping.map_to_draft(draft, reads, min_score_to_add=min_score, engine=eng)
        for r, g in zip(reads, got):
            sp = poa.SparsePoa(eng)
            assert sp.OrientAndAddRead(draft) == 0 and sp.OrientAndAddRead(draft) == 1
            key = sp.OrientAndAddRead(r, min_score)
            assert (key == -1) == (g is None), (min_score, r, key, g)
            if g is not None:
                assert g["score"] >= min_score and summary_of(g) == _expect(draft, r)
    assert [g is None for g in mapping.map_to_draft(draft, reads[:2], min_score_to_add=30.5, engine=eng)] == [True] * 2


def _mixed_batch():
    rng = random.Random(6)
    zmws = []
    for k, n in enumerate((40, 300, 700, 1500)):
        d = _rand(rng, n)
        reads = [noisy(rng, d[a:b]) for a, b in ((0, n), (n // 4, n), (0, n // 2), (n // 3, n // 3 + 5))]
        reads = [revcomp(r) if i % 2 else r for i, r in enumerate(reads)]
        reads.insert(k % 3, None)
        if n == 700:
            reads.append(_rand(rng, 300) + noisy(rng, d) + _rand(rng, 300))   # two strips
        zmws.append((d, reads))
    return zmws


def test_batch_equals_one_by_one(M):
    mapping, eng = M
    zmws = _mixed_batch()
    got = mapping.map_batch(zmws, engine=eng)
    for (d, reads), res in zip(zmws, got):
        assert len(res) == len(reads)
        for r, g in zip(reads, res):
            assert [g] == mapping.map_to_draft(d, [r], engine=eng)
            assert summary_of(g) == (None if r is None else _expect(d, r))
    assert mapping.map_batch([], engine=eng) == [] and mapping.map_batch([("ACGT", [])], engine=eng) == [[]]


def test_batch_beside_a_polish_on_the_same_engine(M):
    import pbccs_amd
    from pbccs_amd import synth
    mapping, eng = M
    zmws = _mixed_batch()
    pz = synth.make_zmws(4, 300, 6, seed=77)
    want_map, want_pol = mapping.map_batch(zmws, engine=eng), pbccs_amd.polish_zmws(pz, engine=eng)
    box = {}
    t = threading.Thread(target=lambda: box.setdefault("pol", pbccs_amd.polish_zmws(pz, engine=eng)))
    t.start()
    got = [mapping.map_batch(zmws, engine=eng) for _ in range(3)]
    t.join()
    assert all(g == want_map for g in got)
    assert [(r["status"], r["consensus"], r["add_read_results"]) for r in box["pol"]] == [
        (r["status"], r["consensus"], r["add_read_results"]) for r in want_pol]


def test_over_budget_job_is_eoom_and_the_engine_stays_usable(M, monkeypatch):
    import pbccs_amd
    mapping, eng = M
    rng = random.Random(8)
    long_read = _read_of_length(rng, 1100)        # two strips: 2 x 301 boundary words, more than 1 KB holds
    short_read = _read_of_length(rng, 200)        # one strip: no boundary buffer
    monkeypatch.setenv("PBCCS_MAP_WORKSPACE_KB", "1")
    before = mapping.map_stats(eng)
    with pytest.raises(pbccs_amd.PbccsError) as err:
        mapping.map_to_draft(DRAFT, [long_read], engine=eng)
    assert err.value.code == -2
    after = mapping.map_stats(eng)
    assert (after["cells"], after["launches"]) == (before["cells"], before["launches"])   # no device work
    _check(M, [(DRAFT, short_read)])
    monkeypatch.delenv("PBCCS_MAP_WORKSPACE_KB")
    _check(M, [(DRAFT, long_read), (DRAFT, short_read)])


def test_invalid_inputs(M):
    import pbccs_amd
    mapping, eng = M
    with pytest.raises(pbccs_amd.PbccsError) as err:
        mapping.map_to_draft("", ["ACGT"], engine=eng)
    assert err.value.code == -1
    assert mapping.map_to_draft("ACGT", ["", None], engine=eng) == [None, None]


def test_counters(M):
    mapping, eng = M
    rng = random.Random(9)
    reads = [_read_of_length(rng, n) for n in (10, 300, 1100)]
    mapping.map_stats(eng, reset=True)
    mapping.map_to_draft(DRAFT, reads + [None], engine=eng)
    s = mapping.map_stats(eng)
    assert s["jobs"] == 4
    assert s["cells"] == sum(2 * (len(r) + 1) * len(DRAFT) for r in reads)
    assert s["launches"] == 3 and s["strips"] == 2 * (1 + 1 + 2)


# ---------------------------------------------------------------- end to end

def _e2e_chunks():
    """A dozen ZMWs of 300-500 bases with 9-12 passes on alternating strands, the first and the last pass partial,
    and in every third ZMW one read of more than twice the median length."""
    from pbccs_amd import driver
    rng = random.Random(12)
    chunks = []
    for z in range(12):
        n = rng.randint(300, 500)
        tpl = _rand(rng, n)
        reads = []
        passes = rng.randint(9, 12)
        for p in range(passes):
            s = noisy(rng, tpl, 0.03, 0.02, 0.01)
            flags = driver.FULL_PASS
            if p == 0:
                s, flags = s[len(s) // 3:], driver.ADAPTER_AFTER
            elif p == passes - 1:
                s, flags = s[: 2 * len(s) // 3], driver.ADAPTER_BEFORE
            reads.append({"seq": revcomp(s) if p % 2 else s, "flags": flags})
        if z % 3 == 0:
            reads.insert(4, {"seq": noisy(rng, tpl + revcomp(tpl) + tpl[:30], 0.03, 0.02, 0.01),
                             "flags": driver.FULL_PASS})
        chunks.append({"snr": [10.0, 7.0, 5.0, 11.0], "reads": reads})
    return chunks


def _oracle_mapper(draft, reads):
    return [_expect(draft, r) for r in reads]


_E2E = {}


def _e2e_reference(cap):
    """oracle.sparse_poa(max_coverage=cap) -> oracle mapping of the rest -> extract_mapped_read -> oracle.polish_zmw,
    computed once per cap."""
    from pbccs_amd import driver
    if cap not in _E2E:
        out = []
        for c in _e2e_chunks():
            st, zmw = driver.zmw_input(c, OraclePoa(), max_poa_coverage=cap, mapper=_oracle_mapper)
            assert st is None
            added = [r for r in zmw["reads"] if r["seq"] is not None]
            out.append((c, zmw, O.polish_zmw(zmw["draft"], added, zmw["snr"])))
        _E2E[cap] = out
    return _E2E[cap]


def _close(a, b, rel=1e-9, abs_=1e-9):
    if math.isnan(a) or math.isnan(b):
        return math.isnan(a) and math.isnan(b)
    return abs(a - b) <= abs_ + rel * max(abs(a), abs(b))


@pytest.mark.parametrize("cap", [3, 5])
def test_capped_ccs_with_mapping_matches_the_oracle_composition(M, cap):
    """ccs_batch(max_poa_coverage=cap, map_past_cap=True) against the composition of oracles.  Draft, consensus,
    AddRead results, add_order, nTested and nApplied are equal; per-read z-scores (the per-read LLs, normalised)
    within the project's 1e-9 relative; QVs within 1.  The status is compared with the product's polish of the
    oracle-composed inputs (the oracle has no pass / drop gates)."""
    import pbccs_amd
    from pbccs_amd import driver
    mapping, eng = M
    ref = _e2e_reference(cap)
    got = driver.ccs_batch([c for c, _, _ in ref], engine=eng, max_poa_coverage=cap, map_past_cap=True)
    pol = pbccs_amd.polish_zmws([zmw for _, zmw, _ in ref], engine=eng)
    n_success = 0
    for (c, zmw, e), g, p in zip(ref, got, pol):
        nr = len(c["reads"])
        order = [None if r is None else next(j for j, x in enumerate(c["reads"]) if x is r)
                 for r in driver.filter_reads(c["reads"], 10)]
        assert len(zmw["reads"]) == nr == len(order)
        assert g["draft"] == zmw["draft"]
        it_a, it_z = iter(e["add_read_results"]), iter(e["zscores"])
        want_arr, want_z, want_order = [-1] * nr, [float("nan")] * nr, []
        for k, r in zip(order, zmw["reads"]):
            if r["seq"] is None:
                continue
            want_arr[k], want_z[k] = next(it_a), next(it_z)
            want_order.append(k)
        assert g["add_read_results"] == want_arr
        assert g["add_order"] == [k for k in want_order if want_arr[k] >= 0]
        assert sum(1 for a in want_arr if a >= 0) > cap          # reads past the cap reached AddRead
        assert all(_close(a, b) for a, b in zip(g["zscores"], want_z)), (g["zscores"], want_z)
        assert g["status"] == p["status"]
        assert (g["n_tested"], g["n_applied"]) == (e["n_tested"], e["n_applied"])
        if g["status"] == "Success":
            n_success += 1
            assert e["converged"] and g["consensus"] == e["template"]
            assert max(abs(a - b) for a, b in zip(g["qvs"], e["qvs"])) <= 1
    assert n_success >= 9
    # the Python path over the same kernels gives the same polish inputs
    ins = driver.zmw_inputs_batch([c for c, _, _ in ref], max_poa_coverage=cap, engine=eng, map_past_cap=True)
    assert ins == [(None, zmw) for _, zmw, _ in ref]


def test_unchanged_paths(M):
    """map_past_cap=False is pbccs_ccs_batch field by field (pbccs_ccs_batch_ex with the flag off too); a cap at or
    above the read count equals the uncapped run, with or without the flag."""
    import ctypes
    from pbccs_amd import driver, lib as L
    mapping, eng = M
    chunks = _e2e_chunks()[:4]

    def same(a, b):
        assert len(a) == len(b)
        for x, y in zip(a, b):
            assert x.keys() == y.keys()
            for k in x:
                if k == "zscores":
                    assert all((math.isnan(p) and math.isnan(q)) or p == q for p, q in zip(x[k], y[k]))
                elif isinstance(x[k], float) and math.isnan(x[k]):
                    assert math.isnan(y[k])
                else:
                    assert x[k] == y[k], k

    for cap in (3, None):
        same(driver.ccs_batch(chunks, engine=eng, max_poa_coverage=cap, map_past_cap=False),
             driver.ccs_batch(chunks, engine=eng, max_poa_coverage=cap))
    uncapped = driver.ccs_batch(chunks, engine=eng)
    big = max(len(c["reads"]) for c in chunks)
    for flag in (False, True):
        same(driver.ccs_batch(chunks, engine=eng, max_poa_coverage=big, map_past_cap=flag), uncapped)
    same(driver.ccs_batch(chunks, engine=eng, map_past_cap=True), uncapped)
    assert (driver.zmw_inputs_batch(chunks, max_poa_coverage=3, engine=eng, map_past_cap=False) ==
            driver.zmw_inputs_batch(chunks, max_poa_coverage=3, engine=eng))
    # the _ex entry with the flag off and the default initialiser
    co = L.CCcsOptions()
    L.load().pbccs_ccs_options_default(ctypes.byref(co))
    assert co.map_past_cap == 0 and co.max_poa_coverage >= 2**62
    assert L.load().pbccs_ccs_batch_ex(eng._h, None, 0, ctypes.byref(co), None, None) == 0
    assert L.load().pbccs_ccs_batch_ex(eng._h, None, 0, None, None, None) == 0

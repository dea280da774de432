"""Split mapping on the GPU (pbccs_split_map_batch: k_split_fill, k_split_chain) and the ccs call that recovers
missed-adapter reads (pbccs_ccs_batch_split).  The yardstick is tests/split_map_restatement.py, which
tests/test_split_map_cpu.py pins; segments, scores and flags are compared for equality."""
import math
import random

import pytest

from split_map_restatement import split_map
from test_map_cpu import edge_cases, noisy, revcomp, seeded_cases
from test_split_map_cpu import ADAPTER, P_TEST, fused_cases, planted_cases, rand_seq, tie_cases

pytestmark = pytest.mark.gpu

COLS_PER_LANE = (2, 4, 8)   # split_map_kernels.hpp's kSplitColsPerLane
# (PBCCS_SPLIT_COLS_PER_LANE, PBCCS_SPLIT_TILED): the default choice, every compiled C on the register path (a draft
# wider than 64 C runs tiled with that C), every C on the row-buffer path
VARIANTS = [(None, None)] + [(c, None) for c in COLS_PER_LANE] + [(c, "1") for c in COLS_PER_LANE]
J_SIZES = (1, 2, 63, 64, 65, 127, 128, 129, 300)
I_SIZES = (1, 2, 10, 64, 65, 200, 700)


@pytest.fixture(scope="module")
def M():
    import pbccs_amd
    from pbccs_amd import mapping
    eng = pbccs_amd.Engine(0)
    mapping.split_map_stats(eng, reset=True)
    return mapping, eng


def _pair(rng, n_j, n_i):
    """A draft of n_j bases and a read of exactly n_i: noisy copies of the draft on alternating strands, fused with
    short random spacers and cut to length."""
    draft = rand_seq(rng, n_j)
    parts, strand = [], rng.random() < 0.5
    while sum(map(len, parts)) < n_i:
        p = noisy(rng, draft, 0.05, 0.04, 0.01)
        parts += [revcomp(p) if strand else p, rand_seq(rng, rng.randint(0, 6))]
        strand = not strand
    return draft, "".join(parts)[:n_i]


def grid_cases():
    rng = random.Random(4)
    return [_pair(rng, j, i) for j in J_SIZES for i in I_SIZES]


def all_cases():
    """(draft, read, jump penalty): the seeded and edge cases, tie-heavy cases, the size grid, fused reads."""
    small = seeded_cases() + edge_cases() + tie_cases() + grid_cases()
    return ([(d, r, P_TEST) for d, r in small] + [(d, r, 0) for d, r in tie_cases()] +
            [(d, r, 150) for d, r in fused_cases()] + [(d, r, p) for d, r, p, _ in planted_cases()])


_CASES = all_cases()
_EXPECTED = {}


def _expect(draft, read, jump, max_segments=8):
    """The restatement's chain, computed once per case."""
    key = (draft, read, jump, max_segments)
    if key not in _EXPECTED:
        _EXPECTED[key] = split_map(draft, read, jump, max_segments)
    return _EXPECTED[key]


def _check(M, cases, max_segments=8):
    mapping, eng = M
    by_jump = {}
    for d, r, p in cases:
        by_jump.setdefault(p, []).append((d, r))
    for jump, pairs in by_jump.items():
        got = mapping.split_map_batch([(d, [r]) for d, r in pairs], jump, max_segments, engine=eng)
        for (d, r), (g,) in zip(pairs, got):
            assert g == _expect(d, r, jump, max_segments), (len(d), len(r), jump, g, _expect(d, r, jump, max_segments))


@pytest.mark.parametrize("cols,tiled", VARIANTS)
def test_split_map_equals_the_restatement(M, monkeypatch, cols, tiled):
    mapping, eng = M
    if cols is not None:
        monkeypatch.setenv("PBCCS_SPLIT_COLS_PER_LANE", str(cols))
    if tiled is not None:
        monkeypatch.setenv("PBCCS_SPLIT_TILED", tiled)
    before = mapping.split_map_stats(eng)
    _check(M, _CASES)
    after = mapping.split_map_stats(eng)
    mapped = [(d, r) for d, r, _ in _CASES if r]
    assert after["jobs"] - before["jobs"] == len(_CASES)
    assert after["cells"] - before["cells"] == sum(2 * len(d) * len(r) for d, r in mapped)
    # the path each draft took: the row buffer when forced, or when the draft is wider than the tile
    width = 64 * (cols or COLS_PER_LANE[-1])
    assert after["tiled"] - before["tiled"] == sum(1 for d, _ in mapped if tiled or len(d) > width)


def test_the_cases_reach_every_branch():
    """The shapes the variants above rely on: drafts at, below and above every tile width; chains of several segments
    on both strands; ties; truncated chains."""
    widths = {len(d) for d, _, _ in _CASES}
    assert set(J_SIZES) <= widths and max(widths) > 64 * COLS_PER_LANE[-1]
    chains = [_expect(d, r, p) for d, r, p in _CASES]
    assert sum(1 for c in chains if c is None) >= 1
    assert sum(1 for c in chains if c and c["n_segments"] >= 3) >= 20
    assert sum(1 for c in chains if c and c["truncated"]) >= 5
    assert any(c and {s["rc"] for s in c["segments"]} == {False, True} for c in chains)


def test_one_batch_with_no_reads_an_over_budget_read_and_a_truncated_chain(M, monkeypatch):
    import pbccs_amd
    mapping, eng = M
    draft, four = fused_cases()[2]                 # four passes
    short = draft[10:50]                           # 41 row records: 820 bytes
    long_read = four[:400]                         # 401 row records: more than 1 KB holds
    monkeypatch.setenv("PBCCS_SPLIT_WORKSPACE_KB", "1")
    before = mapping.split_map_stats(eng)
    with pytest.raises(pbccs_amd.PbccsError) as err:
        mapping.split_map_batch([(draft, [None, long_read, "", short])], 150, 2, engine=eng)
    assert err.value.code == -2
    after = mapping.split_map_stats(eng)
    assert after["cells"] - before["cells"] == 2 * len(draft) * len(short)   # no device work for the long read
    monkeypatch.delenv("PBCCS_SPLIT_WORKSPACE_KB")
    got = mapping.split_map_batch([(draft, [None, long_read, "", short, four])], 150, 2, engine=eng)[0]
    assert got[0] is None and got[2] is None
    assert got[1] == _expect(draft, long_read, 150, 2) and got[3] == _expect(draft, short, 150, 2)
    assert got[4] == _expect(draft, four, 150, 2)
    assert got[4]["truncated"] and got[4]["n_segments"] == 4 and len(got[4]["segments"]) == 2
    assert mapping.split_map_to_draft(draft, [four], engine=eng)[0] == _expect(draft, four, mapping.SPLIT_JUMP_PENALTY)


def test_invalid_inputs(M):
    import pbccs_amd
    mapping, eng = M
    with pytest.raises(pbccs_amd.PbccsError) as err:
        mapping.split_map_to_draft("", ["ACGT"], engine=eng)
    assert err.value.code == -1
    with pytest.raises(ValueError):
        mapping.split_map_to_draft("ACGT", ["ACGT"], max_segments=65, engine=eng)
    assert mapping.split_map_to_draft("ACGT", ["", None], engine=eng) == [None, None]


# ---- the ccs call ----------------------------------------------------------------------------------------------

def _zmw_chunk(rng, clean, fused_passes, length=120, flags=None):
    """One ZMW's raw subreads: `clean` noisy passes on alternating strands and, when fused_passes, one read that
    holds that many passes fused across missed adapters."""
    from pbccs_amd import driver
    tpl = rand_seq(rng, length)
    reads = []
    for p in range(clean):
        s = noisy(rng, tpl, 0.03, 0.02, 0.01)
        reads.append({"seq": revcomp(s) if p % 2 else s, "flags": driver.FULL_PASS})
    if fused_passes:
        parts = []
        for p in range(fused_passes):
            s = noisy(rng, tpl, 0.03, 0.02, 0.01)
            parts.append(revcomp(s) if (clean + p) % 2 else s)
        reads.insert(1, {"seq": ADAPTER.join(parts), "flags": driver.FULL_PASS if flags is None else flags})
    return {"snr": [9.0, 8.0, 7.0, 10.0], "reads": reads}


def _chunks():
    from pbccs_amd import driver
    rng = random.Random(2026)
    return [_zmw_chunk(rng, 2, 2),                                 # MinPasses = 3 only with the fused pair
            _zmw_chunk(rng, 5, 3, flags=driver.ADAPTER_AFTER),     # three fused passes, the first one partial
            _zmw_chunk(rng, 4, 0),                                 # nothing dropped
            _zmw_chunk(rng, 6, 2),
            {"snr": [9.0, 8.0, 7.0, 10.0], "reads": []}]           # NoSubreads


def _same_float(a, b):
    return (math.isnan(a) and math.isnan(b)) or a == b


def _same(a, b):
    """Equality in which NaN equals NaN."""
    if isinstance(a, float) and isinstance(b, float):
        return _same_float(a, b)
    if isinstance(a, dict) and isinstance(b, dict):
        return a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)) and isinstance(b, (list, tuple)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return a == b


def test_ccs_batch_with_split_long_reads(M):
    import pbccs_amd
    from pbccs_amd import driver
    _, eng = M
    chunks = _chunks()
    off = driver.ccs_batch(chunks, engine=eng)
    assert all("split_reads" not in r for r in off)
    on = driver.ccs_batch(chunks, engine=eng, split_long_reads=True)
    # the ZMW with two clean passes and a fused pair
    assert off[0]["status"] != "Success" and off[0]["n_passes"] < 3
    assert on[0]["status"] == "Success" and on[0]["n_passes"] >= 3 and on[0]["n_missed_adapters"] == 1
    assert [r["n_missed_adapters"] for r in on] == [1, 2, 0, 1, 0]
    # the Python path: the POA, the split mapping and the polish as three calls
    inputs = driver.zmw_inputs_batch(chunks, engine=eng, split_long_reads=True)
    live = [z for z, (st, _) in enumerate(inputs) if st is None]
    assert live == [0, 1, 2, 3] and inputs[4][0] == "NoSubreads" and on[4]["status"] == "NoSubreads"
    pol = pbccs_amd.polish_zmws([inputs[z][1] for z in live], engine=eng)
    for z, p in zip(live, pol):
        zmw, got = inputs[z][1], on[z]
        assert (got["status"], got["consensus"], got["qvs"], got["draft"]) == (p["status"], p["consensus"], p["qvs"],
                                                                               zmw["draft"])
        assert (got["n_passes"], got["n_tested"], got["n_applied"]) == (p["n_passes"], p["n_tested"], p["n_applied"])
        assert got["n_missed_adapters"] == zmw["n_missed_adapters"]
        assert [s["subread"] for s in got["split_reads"]] == [s["subread"] for s in zmw["split_reads"]]
        added = 0
        for gs, ws in zip(got["split_reads"], zmw["split_reads"]):
            assert got["add_read_results"][gs["subread"]] == -1 and math.isnan(got["zscores"][gs["subread"]])
            assert len(gs["segments"]) == len(ws["segments"])
            for k, (a, b) in enumerate(zip(gs["segments"], ws["segments"])):
                pos = ws["first"] + k
                assert {f: a[f] for f in ("rc", "read", "tpl", "score")} == b
                assert a["full_pass"] == zmw["reads"][pos]["full_pass"]
                assert a["add_read_result"] == p["add_read_results"][pos]
                assert _same_float(a["zscore"], p["zscores"][pos])
                added += a["add_read_result"] == 0
            assert got["add_order"].count(gs["subread"]) == sum(s["add_read_result"] >= 0 for s in gs["segments"])
        assert added >= 2 * len(got["split_reads"])
        assert len(got["add_order"]) == sum(1 for a in p["add_read_results"] if a >= 0)
    # flags: the partial first pass of ZMW 1's fused read is no full pass, the interior and last ones are
    assert [s["full_pass"] for s in on[1]["split_reads"][0]["segments"]] == [False, True, True]
    assert [s["full_pass"] for s in on[0]["split_reads"][0]["segments"]] == [True, True]
    # ZMWs with nothing to split are what they were
    for z in (2, 4):
        assert _same({k: v for k, v in on[z].items() if k not in ("split_reads", "n_missed_adapters")}, off[z])
        assert on[z]["split_reads"] == []


def test_keyword_off_records_are_todays(M):
    from pbccs_amd import driver
    _, eng = M
    chunks = _chunks()
    a = driver.ccs_batch(chunks, engine=eng)
    b = driver.ccs_batch(chunks, engine=eng, split_long_reads=False)
    assert [sorted(r) for r in a] == [sorted(r) for r in b]
    assert _same(a, b)
    # tests/golden/split_ccs_off.json: what the commit before the feature returned for these chunks
    import json
    import os
    golden = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "split_ccs_off.json")))
    assert len(golden) == len(a)
    for x, g in zip(a, golden):
        assert sorted(x) == sorted(g)
        for k, v in g.items():
            if k in ("zscores", "zg", "za", "predicted_accuracy"):   # doubles: the device's summation order is free
                xs, vs = (x[k], v) if isinstance(v, list) else ([x[k]], [v])
                assert len(xs) == len(vs)
                assert all((math.isnan(p) and math.isnan(q)) or math.isclose(p, q, rel_tol=1e-9, abs_tol=1e-9)
                           for p, q in zip(xs, vs)), k
            else:
                assert x[k] == v, k
    assert a[0]["add_read_results"][1] == -1 and len(a[0]["add_order"]) == 2   # the fused read is dropped today

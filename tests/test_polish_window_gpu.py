"""Windowed polish on the GPU (pbccs_window_slices, pbccs_polish_windowed: k_window_cuts / k_window_join) against the
restatement of tests/polish_window_restatement.py, whose windows the oracle polishes.  Bounds, joins, cuts, the
consensus, the counts and the per-read codes are compared for equality; QVs within the project's +-1; z-scores to
1e-6.  The inputs are 700-base ZMWs under windows of 200 with overlaps of 100 and 60: three or four windows each,
so that first, inner and last windows, joints at and off the middle, and a fallback all occur."""
import math
import random
import subprocess

import pytest

import polish_window_restatement as W
import sparse_restatement as SR
from test_polish_window_cpu import build_driver

pytestmark = pytest.mark.gpu

OPTS = dict(window=200, overlap=100, guard=8, k=6)
CASE = (6, 700, 8, 7, 200, 100, 8, 6)   # the six ZMWs of the issue's first row


@pytest.fixture(scope="module")
def eng():
    """The package's default engine.  It lives as long as the process, so its band pools' address ranges are never
    handed back: an engine of this module's own would leave its ranges behind for every later pool of the process to
    step over (VmPool::reserve gives up after 64 such ranges)."""
    import pbccs_amd
    return pbccs_amd.default_engine()


@pytest.fixture(scope="module")
def six(eng):
    """(zmws, restated records, polish_windowed's records) of the six 700-base ZMWs."""
    from pbccs_amd import polish as P
    zmws, want = W.synthetic_case(*CASE)
    return zmws, want, P.polish_windowed(zmws, engine=eng, **OPTS)


def same_value(a, b):
    if isinstance(a, float) and isinstance(b, float):
        return (math.isnan(a) and math.isnan(b)) or a == b
    if isinstance(a, (list, tuple)) and isinstance(b, (list, tuple)):
        return len(a) == len(b) and all(same_value(x, y) for x, y in zip(a, b))
    if isinstance(a, dict) and isinstance(b, dict):
        return a.keys() == b.keys() and all(same_value(a[k], b[k]) for k in a)
    return a == b


def same_record(got, exp):
    """Field for field what polish_zmws returns (NaN equal to NaN)."""
    return all(same_value(got[k], exp[k]) for k in exp)


def close(a, b, tol=1e-6):
    return (math.isnan(a) and math.isnan(b)) or abs(a - b) <= tol * max(1.0, abs(a), abs(b))


def check_against_restatement(got, want):
    assert got["windowed"] and got["fallback"] == want["fallback"] == 0
    assert got["unanchored_reads"] == want["unanchored_reads"]
    assert len(got["windows"]) == len(want["windows"])
    for g, w in zip(got["windows"], want["windows"]):
        for key in ("begin", "end", "join", "cut_begin", "cut_end", "status", "n_tested", "n_applied"):
            assert g[key] == w[key], (key, g, w)
    assert got["status"] == "Success"
    assert got["consensus"] == want["consensus"]
    assert len(got["qvs"]) == len(want["qvs"])
    assert max(abs(a - b) for a, b in zip(got["qvs"], want["qvs"])) <= 1
    assert abs(got["predicted_accuracy"] - want["predicted_accuracy"]) < 1e-3
    for key in ("n_tested", "n_applied", "n_passes", "status_counts", "add_read_results"):
        assert got[key] == want[key], key
    assert all(close(a, b) for a, b in zip(got["zscores"], want["zscores"]))
    assert close(got["zg"], want["zg"]) and close(got["za"], want["za"])


def check_slices(eng, zmws, window, overlap, k, min_length=10):
    from pbccs_amd import polish as P
    got = P.window_slices(zmws, window=window, overlap=overlap, k=k, min_length=min_length, engine=eng)
    for z, g in zip(zmws, got):
        wins, rows, unanchored = W.slices(z, window, overlap, k, min_length)
        assert g["windows"] == wins
        assert g["slices"] == rows
        assert g["unanchored_reads"] == unanchored
    return got


# ---- window_slices -------------------------------------------------------------------------------------------
def test_slices_of_the_six_zmws(eng):
    zmws, _ = W.synthetic_case(*CASE)
    got = check_slices(eng, zmws, 200, 100, 6)
    assert all(x is not None for g in got for row in g["slices"] for x in row)   # every read in every window
    check_slices(eng, zmws, 200, 60, 8)
    check_slices(eng, zmws[:2], 97, 33, 4)   # many windows, boundaries off every multiple of 64


def _partial(zmw, r, ts, te):
    """Read r of the ZMW mapped to draft[ts:te) only: its forward text is cut in proportion."""
    read = zmw["reads"][r]
    f = W.forward_text(read)
    L = len(zmw["draft"])
    part = f[len(f) * ts // L:len(f) * te // L]
    return {"seq": part if not read["strand"] else SR.revcomp(part), "strand": read["strand"], "ts": ts, "te": te}


def test_slices_of_partly_mapped_reads_on_both_strands(eng):
    zmws, _ = W.synthetic_case(*CASE)
    z = dict(zmws[0])
    L = len(z["draft"])
    z["reads"] = [_partial(z, 0, 150, 560), _partial(z, 1, 150, 560), _partial(z, 2, 0, 205), _partial(z, 3, 395, L),
                  _partial(z, 4, 203, 300), _partial(z, 5, 296, 404), z["reads"][6], {"seq": None, "strand": 0, "ts": 0, "te": 0}]
    assert {r["strand"] for r in z["reads"][:6]} == {0, 1}
    got = check_slices(eng, [z], 200, 100, 6)[0]
    assert got["slices"][0][3] is None and got["slices"][2][2] is None   # reads that miss a window
    assert all(row[7] is None for row in got["slices"])
    # an extent of a few bases inside a window is a placeholder there: read 2 reaches 5 bases into window 1
    assert got["slices"][1][2] is None and got["slices"][0][2] is not None


def test_slices_of_a_read_with_an_empty_chain(eng):
    zmws, _ = W.synthetic_case(*CASE)
    z = dict(zmws[1])
    rng = random.Random(11)
    while True:   # a random read no 8-mer of which is in the draft
        junk = "".join(rng.choice("ACGT") for _ in range(40))
        if not SR.sparse_align(z["draft"], junk, 8) and not SR.sparse_align(z["draft"], SR.revcomp(junk), 8):
            break
    z["reads"] = list(z["reads"][:3]) + [{"seq": junk, "strand": 0, "ts": 0, "te": len(z["draft"])},
                                         {"seq": junk, "strand": 1, "ts": 100, "te": 650}]
    got = check_slices(eng, [z], 200, 100, 8)[0]
    assert got["unanchored_reads"] == 2
    assert all(row[3] is None and row[4] is None for row in got["slices"])


# ---- polish_windowed -----------------------------------------------------------------------------------------
def test_windowed_equals_the_restatement(six):
    zmws, want, got = six
    assert [w["fallback"] for w in want] == [0] * 6   # pinned by tests/test_polish_window_cpu.py
    for g, w in zip(got, want):
        check_against_restatement(g, w)


def test_host_join_rule_gives_the_same_records(eng, six, monkeypatch):
    """PBCCS_WINDOW_HOST_JOIN=1 downloads the transcripts and joins them with pbccs_window_join."""
    from pbccs_amd import polish as P
    zmws, _, got = six
    monkeypatch.setenv("PBCCS_WINDOW_HOST_JOIN", "1")
    host = P.polish_windowed(zmws[:3], engine=eng, **OPTS)
    for h, g in zip(host, got):
        assert same_record(h, g)


def test_one_window_zmw_is_the_existing_route(eng):
    import pbccs_amd
    from pbccs_amd import polish as P, synth
    zmws = synth.make_zmws(2, 300, 6, seed=2028)
    assert [len(z["draft"]) for z in zmws] == [300, 299]   # window + overlap itself, and one below
    exp = pbccs_amd.polish_zmws(zmws, engine=eng)
    got = P.polish_windowed(zmws, engine=eng, **OPTS)
    for g, e in zip(got, exp):
        assert same_record(g, e)
        assert not g["windowed"] and g["fallback"] == 0 and len(g["windows"]) == 1
        assert g["windows"][0]["cut_end"] == len(g["consensus"]) and g["windows"][0]["join"] == -1


def test_fallbacks_are_the_restatements_and_their_records_the_whole_routes(eng):
    import pbccs_amd
    from pbccs_amd import polish as P
    zmws, want = W.synthetic_case(8, 700, 4, 7, 200, 60, 8, 6)
    assert sum(1 for w in want if w["fallback"]) == 1
    got = P.polish_windowed(zmws, engine=eng, window=200, overlap=60, guard=8, k=6)
    assert [g["fallback"] for g in got] == [w["fallback"] for w in want]
    back = [i for i, w in enumerate(want) if w["fallback"]]
    whole = pbccs_amd.polish_zmws([zmws[i] for i in back], engine=eng)
    for i, e in zip(back, whole):
        assert same_record(got[i], e)
        assert [w["status"] for w in got[i]["windows"]] == [w["status"] for w in want[i]["windows"]]
    for g, w in zip(got, want):
        if not w["fallback"]:
            check_against_restatement(g, w)


def test_a_rewritten_overlap_has_no_join(eng):
    import pbccs_amd
    from pbccs_amd import polish as P
    zmws, _ = W.synthetic_case(*CASE)
    z = dict(zmws[2])
    (s0, e0), (s1, e1) = W.plan(len(z["draft"]), 200, 100)[:2]
    d = list(z["draft"])
    for p in range(s1 - 2, e0 + 2, 7):   # a wrong base every 7 columns of the first overlap: no 16 matches in a row
        d[p] = "ACGT"[("ACGT".index(d[p]) + 1) % 4]
    z["draft"] = "".join(d)
    want = W.polish_windowed(z, 200, 100, 8, 6)
    assert want["fallback"] == W.FALLBACK_NO_JOIN
    got = P.polish_windowed([z], engine=eng, **OPTS)[0]
    assert got["fallback"] == W.FALLBACK_NO_JOIN and P.WINDOW_FALLBACK[got["fallback"]] == "no join"
    assert same_record(got, pbccs_amd.polish_zmws([z], engine=eng)[0])
    assert [w["status"] for w in got["windows"]] == [0] * len(got["windows"])


def test_mixed_lengths_keep_their_order_and_polish_zmws_is_unchanged(eng, six):
    import pbccs_amd
    from pbccs_amd import polish as P, synth
    zmws, _, got6 = six
    short = synth.make_zmws(2, 300, 6, seed=2028)
    before = pbccs_amd.polish_zmws(short + zmws[:1], engine=eng)
    mixed = [short[0], zmws[0], short[1], zmws[1]]
    got = P.polish_windowed(mixed, engine=eng, **OPTS)
    after = pbccs_amd.polish_zmws(short + zmws[:1], engine=eng)
    assert all(same_record(a, b) for a, b in zip(after, before))
    assert same_record(got[0], before[0]) and same_record(got[2], before[1])
    assert same_record(got[1], got6[0]) and same_record(got[3], got6[1])
    assert [g["windowed"] for g in got] == [False, True, False, True]


def test_ccs_batch_with_windows_equals_the_driver_then_polish_windowed(eng):
    from pbccs_amd import driver, polish as P, synth
    zmws = synth.make_zmws(2, 700, 8, seed=7) + synth.make_zmws(1, 250, 6, seed=2028)   # the POA drafts: two long, one short
    chunks = [{"snr": z["snr"], "reads": [{"seq": r["seq"]} for r in z["reads"]]} for z in zmws]
    native = driver.ccs_batch(chunks, engine=eng, polish_window=dict(window=200, overlap=100, k=6))
    ins = driver.zmw_inputs_batch(chunks, engine=eng)
    assert all(st is None for st, _ in ins)
    exp = P.polish_windowed([z for _, z in ins], engine=eng, **OPTS)
    assert [e["windowed"] for e in exp] == [True, True, False]
    for c, got, e in zip(chunks, native, exp):
        for k in ("status", "consensus", "qvs", "n_tested", "n_applied", "n_passes", "status_counts", "windowed", "fallback"):
            assert got[k] == e[k], k
        assert got["n_windows"] == len(e["windows"])
        order = [next(j for j, x in enumerate(c["reads"]) if x is r)
                 for r in driver.filter_reads(c["reads"], 10) if r is not None]
        want_arr, want_z = [-1] * len(c["reads"]), [float("nan")] * len(c["reads"])
        for i, (a, zz) in enumerate(zip(e["add_read_results"], e["zscores"])):
            want_arr[order[i]], want_z[order[i]] = a, zz
        assert got["add_read_results"] == want_arr
        assert same_value(got["zscores"], want_z)
    plain = driver.ccs_batch(chunks, engine=eng)
    assert "windowed" not in plain[0] and plain[2]["consensus"] == native[2]["consensus"]


def test_cpp_driver_prints_the_same_records(eng, six, tmp_path):
    zmws, _, got = six
    zmws, got = zmws[:2], got[:2]
    case = tmp_path / "case.txt"
    lines = ["200 100 8 6", str(len(zmws))]
    for z in zmws:
        lines.append(" ".join([z["draft"]] + [repr(float(v)) for v in z["snr"]] + [str(len(z["reads"]))]))
        for r in z["reads"]:
            lines.append(f"{r['seq']} {r['strand']} {r['ts']} {r['te']} 1")
    case.write_text("\n".join(lines) + "\n")
    out = subprocess.run([build_driver(), str(case)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    want = []
    for g in got:
        want.append(f"zmw {g['status_code']} {g['fallback']} {len(g['windows'])} {g['unanchored_reads']} {g['n_tested']} "
                    f"{g['n_applied']} {g['n_passes']} {g['consensus']}.")
        want.append(" ".join(["qvs"] + [str(q) for q in g["qvs"]]))
        want.append(" ".join(["reads"] + [str(c) for c in g["add_read_results"]]))
        for w in g["windows"]:
            want.append(f"win {w['begin']} {w['end']} {w['join']} {w['cut_begin']} {w['cut_end']} {w['status']} "
                        f"{w['n_tested']} {w['n_applied']}")
    assert out.stdout.strip().split("\n") == want

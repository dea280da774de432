"""The banded POA fill on the device against the plain Python restatement of its rules
(tests/poa_band_restatement.py, tests/sparse_restatement.py), for equality throughout: anchors, ranges vertex for
vertex, exit score and traceback step for step; the fallbacks; the containment property that ties the banded results
to the unbanded ones; the batched, ccs and C++ entry points; and the switch-off paths byte for byte."""
import ctypes
import json
import os
import subprocess

import pytest

import poa_band_restatement as B
import sparse_restatement as R

pytestmark = pytest.mark.gpu

ROOT = R.ROOT


@pytest.fixture(scope="module")
def P():
    import pbccs_amd
    from pbccs_amd import poa
    eng = pbccs_amd.Engine(0)
    poa.poa_band_stats(eng, reset=True)
    return poa, eng


def _graph(h):
    return B.graph_from_dot(h.ToGraphViz())


def _oriented(read, rc):
    return R.revcomp(read) if rc else read


def _expected(h, read, rc):
    """(graph, css path, anchors, ranges) of the restatement for this read against the handle's graph; ranges None
    where rule 5 sends the alignment to the full fill."""
    ar = h.AlignableRanges(read, rc)
    g = _graph(h)
    q = _oriented(read, rc)
    css = "".join(g.bases[v] for v in ar["css_path"])
    assert css == h.FindConsensus(-B.INT_MAX)[0]
    anchors = R.sparse_align(css, q, B.K) if set(q) <= set("ACGT") else []
    if not anchors:
        assert ar["fallback"] and not ar["anchors"] and not ar["ranges"]
        return g, ar, None
    assert not ar["fallback"]
    assert ar["anchors"] == anchors
    lit = B.ranges_literal(g, ar["css_path"], anchors, len(q))
    assert ar["ranges"] == {v: lit[v] for v in lit if v != B.EXIT}
    return g, ar, lit


def _check_step(h, read, rc):
    """AlignableRanges and TryAddRead(banded=True) of one alignment against the restatement."""
    g, ar, lit = _expected(h, read, rc)
    score, steps = h.TryAddRead(read, rc, banded=True, rows=True)
    if lit is None:
        assert (score, steps) == h.TryAddRead(read, rc, banded=False, rows=True)
        return None
    exp_score, exp_steps, _ = B.fill_and_trace(g, _oriented(read, rc), lit)
    assert score == exp_score
    assert steps == exp_steps
    return lit


def _walk_zmw(poa, eng, reads, both=True):
    """Every step of a ZMW: both orientations checked, then the read committed banded."""
    h = poa.SparsePoa(eng, banded=True)
    assert h.OrientAndAddRead(reads[0]) == 0
    for r in reads[1:]:
        for rc in ((False, True) if both else (False,)):
            _check_step(h, r, rc)
        h.OrientAndAddRead(r)
    return h


def _zmw(seed, n, passes, err, flip=True):
    g = R.Lcg(seed)
    t = g.seq(n)
    reads = [g.noisy(t, err) for _ in range(passes)]
    return [R.revcomp(r) if flip and k % 2 else r for k, r in enumerate(reads)], t, g


@pytest.mark.parametrize("committed", [1, 2, 5])
def test_alignable_ranges_after_committed_reads(P, committed):
    poa, eng = P
    reads, _, _ = _zmw(500 + committed, 180, committed + 1, 10)
    h = poa.SparsePoa(eng, banded=True)
    for r in reads[:committed]:
        assert h.OrientAndAddRead(r) >= 0
    for rc in (False, True):
        assert _expected(h, reads[committed], rc) is not None
    # the matching strand has a chain
    assert h.AlignableRanges(reads[committed], committed % 2 == 1)["anchors"]


@pytest.mark.parametrize("n", [64, 300])
def test_try_add_read_equals_the_restatement_six_reads(P, n):
    poa, eng = P
    reads, _, _ = _zmw(610 + n, n, 6, 10)
    _walk_zmw(poa, eng, reads)


def test_reads_of_63_64_65(P):
    poa, eng = P
    g = R.Lcg(77)
    t = g.seq(70)
    reads = [t[:64]]
    for k, ln in enumerate((63, 64, 65, 64, 65)):
        r = g.noisy(t, 8)
        while len(r) < ln:
            r = g.noisy(t, 8)
        reads.append(r[:ln])
    assert [len(r) for r in reads[1:4]] == [63, 64, 65]
    _walk_zmw(poa, eng, reads)


def test_reads_shorter_than_the_width(P):
    """I < 30: every band is clipped at both ends."""
    poa, eng = P
    g = R.Lcg(78)
    t = g.seq(26)
    reads = [t] + [g.noisy(t, 6) for _ in range(5)]
    assert all(len(r) < 30 for r in reads)
    _walk_zmw(poa, eng, reads)


@pytest.mark.parametrize("ins", [70, 150, 300])
def test_a_long_insertion(P, ins):
    """70 bases: bands between the anchors on either side of the insertion exceed 64 rows (more than one pass of the
    wave).  150 bases: the branch's merge column has a predecessor more than two 64-column blocks of the program
    back.  300 bases (in a template long enough for the chain to pay the jump): the bands exceed the 256 rows of
    an LDS ring slot and of one group of passes."""
    poa, eng = P
    g = R.Lcg(79 + ins)
    n = 240 if ins < 300 else 700
    t = g.seq(n)
    reads = [g.noisy(t, 6) for _ in range(6 if ins < 300 else 4)]
    reads[2] = reads[2][:n // 2] + g.seq(ins) + reads[2][n // 2:]
    h = poa.SparsePoa(eng, banded=True)
    h.OrientAndAddRead(reads[0])
    widest = 0
    for r in reads[1:]:
        lit = _check_step(h, r, False)
        _check_step(h, r, True)
        widest = max(widest, max(len(B.band_rows(x, len(r))) for x in lit.values()))
        h.OrientAndAddRead(r)
    assert widest > {70: 64, 150: 128, 300: 256}[ins]


def test_a_read_overhanging_the_graph_at_both_ends(P):
    """The graph's first and last columns then hold only a reverse or only a forward mark, and the read's ends fork."""
    poa, eng = P
    g = R.Lcg(80)
    t = g.seq(260)
    reads = [t[50:210], g.noisy(t, 6), g.noisy(t[50:210], 8), g.noisy(t, 10), g.noisy(t[20:240], 8), g.noisy(t, 6)]
    _walk_zmw(poa, eng, reads)


def test_a_bubble_older_than_four_columns(P):
    """An 8-base insertion leaves a branch whose merge column has a predecessor more than four columns back."""
    poa, eng = P
    g = R.Lcg(81)
    t = g.seq(150)
    bub = t[:70] + "GATTACAG" + t[70:]
    reads = [t, bub, g.noisy(t, 6), g.noisy(bub, 6), g.noisy(t, 10), g.noisy(bub, 10)]
    h = _walk_zmw(poa, eng, reads)
    gr = _graph(h)
    assert any(len(p) > 1 for p in gr.preds)


def test_an_unrelated_second_read_gives_empty_columns(P):
    """A two-read graph whose second read is unrelated to the first up to its last twelve bases: its 150 new vertices
    run from ^ to the first read's tail.  A third read that covers the first read's head only has its anchors there,
    so the new vertices have neither an anchored ancestor nor an anchored descendant: their interval is the inverted
    (I, 0) and their columns are empty."""
    poa, eng = P
    g = R.Lcg(82)
    t = g.seq(200)
    h = poa.SparsePoa(eng, banded=True)
    h.OrientAndAddRead(t)
    assert h.OrientAndAddRead(g.seq(150) + t[188:]) == 1      # min_score_to_add 0: any local hit commits
    third = g.noisy(t[:150], 8)
    lit = _check_step(h, third, False)
    empty = [v for v, x in lit.items() if v != B.EXIT and len(B.band_rows(x, len(third))) == 0]
    print("empty columns: %d of %d" % (len(empty), len(lit) - 1))
    assert empty
    _check_step(h, third, True)
    # and a second read that is unrelated throughout
    h = poa.SparsePoa(eng, banded=True)
    h.OrientAndAddRead(t)
    assert h.OrientAndAddRead(g.seq(150)) == 1
    for rc in (False, True):
        _check_step(h, g.noisy(t, 8), rc)


def test_a_read_past_16_bit_scores_takes_the_int32_kernels(P):
    """3 (I + 1) >= 65536: the banded scores are int32 (k_poa_fill_band<int>, k_poa_trace_band<int>).  The restatement
    is too slow at 22 kb, so the check is containment against the device's own full fill, which is pinned."""
    poa, eng = P
    g = R.Lcg(88)
    t = g.seq(22100)
    read = g.noisy(t, 3)
    assert 3 * (len(read) + 1) >= 65536
    h = poa.SparsePoa(eng, banded=True)
    h.OrientAndAddRead(t)
    poa.poa_band_stats(eng, reset=True)
    full = h.TryAddRead(read, False, banded=False, rows=True)
    band = h.TryAddRead(read, False, banded=True, rows=True)
    s = poa.poa_band_stats(eng, reset=True)
    assert (s["banded_alignments"], s["fallbacks"]) == (1, 0) and s["score_bytes"] == 4 * s["band_cells"]
    ar = h.AlignableRanges(read, False)
    assert all(row in B.band_rows(ar["ranges"][v], len(read)) for v, _, row in full[1][1:])
    assert band == full


def test_fallbacks_short_and_homopolymer(P):
    poa, eng = P
    g = R.Lcg(83)
    t = g.seq(120)
    for read in (t[40:45], "A" * 40):
        h = poa.SparsePoa(eng, banded=True)
        h.OrientAndAddRead(t)
        poa.poa_band_stats(eng, reset=True)
        for rc in (False, True):
            assert h.AlignableRanges(read, rc)["fallback"]
            assert h.TryAddRead(read, rc, banded=True, rows=True) == h.TryAddRead(read, rc, banded=False, rows=True)
        s = poa.poa_band_stats(eng, reset=True)
        assert (s["fallbacks"], s["banded_alignments"]) == (2, 0)
        # committing it banded is committing it unbanded
        u = poa.SparsePoa(eng)
        u.OrientAndAddRead(t)
        assert h.OrientAndAddRead(read) == u.OrientAndAddRead(read)
        assert h.ToGraphViz() == u.ToGraphViz()


def test_a_foreign_letter_falls_back(P):
    poa, eng = P
    g = R.Lcg(84)
    t = g.seq(100)
    read = t[:50] + "N" + t[50:]
    h = poa.SparsePoa(eng, banded=True)
    h.OrientAndAddRead(t)
    assert h.AlignableRanges(read)["fallback"]
    assert h.TryAddRead(read, banded=True, rows=True) == h.TryAddRead(read, banded=False, rows=True)


def test_seeding_out_of_memory_falls_back_alone(P, monkeypatch):
    """PBCCS_SPARSE_MAX_SEEDS between the repeat ZMW's seed count and the others': its two forward alignments take
    the full fill, the other ZMWs stay banded."""
    poa, eng = P
    heavy = ["AC" * 100] * 3
    za, _, _ = _zmw(91, 200, 3, 10, flip=False)
    zb, _, _ = _zmw(92, 260, 3, 10, flip=False)
    n_heavy = len(R.find_seeds(heavy[0], heavy[1], B.K))
    n_light = max(len(R.find_seeds(a, b, B.K)) for z in (za, zb) for a in z for b in z)
    assert n_heavy > 4 * n_light
    batch = [za, heavy, zb]
    poa.poa_band_stats(eng, reset=True)
    free = poa.poa_batch(batch, engine=eng, banded=True)
    s_free = poa.poa_band_stats(eng, reset=True)
    monkeypatch.setenv("PBCCS_SPARSE_MAX_SEEDS", str(2 * n_light))
    capped = poa.poa_batch(batch, engine=eng, banded=True)
    s_cap = poa.poa_band_stats(eng, reset=True)
    monkeypatch.delenv("PBCCS_SPARSE_MAX_SEEDS")
    plain = poa.poa_batch(batch, engine=eng)
    assert capped[1] == plain[1]
    assert (capped[0], capped[2]) == (free[0], free[2])
    assert s_cap["fallbacks"] == s_free["fallbacks"] + 2
    assert s_cap["banded_alignments"] == s_free["banded_alignments"] - 2 > 0


def _containment_zmws():
    out = []
    for k in range(24):
        g = R.Lcg(7000 + k)
        n = 200 + g.below(401)
        passes = 4 + g.below(5)
        out.append(_zmw(7100 + k, n, passes, 10)[0])
    return out


def test_containment_on_the_device(P):
    """Wherever the unbanded walk lies inside the bands, the banded score and walk are the unbanded ones."""
    poa, eng = P
    contained = total = 0
    for reads in _containment_zmws():
        h = poa.SparsePoa(eng, banded=True)
        h.OrientAndAddRead(reads[0])
        for k, r in enumerate(reads[1:], 1):
            rc = k % 2 == 1          # the strand that matches the graph
            full = h.TryAddRead(r, rc, banded=False, rows=True)
            ar = h.AlignableRanges(r, rc)
            total += 1
            if not ar["fallback"] and all(
                    row in B.band_rows(ar["ranges"][v], len(r)) or (v == B.ENTER and row == 0)
                    for v, _, row in full[1][1:]):
                contained += 1
                assert h.TryAddRead(r, rc, banded=True, rows=True) == full
            h.OrientAndAddRead(r)
    print("containment: %d of %d walks inside their bands" % (contained, total))
    assert contained >= 0.9 * total, "vacuous: %d of %d" % (contained, total)


def _by_handle(poa, eng, reads, banded):
    h = poa.SparsePoa(eng, banded=banded)
    keys = [h.OrientAndAddRead(r) if r else -1 for r in reads]
    cov = sum(1 for k in keys if k >= 0)
    css, summ = h.FindConsensus(1 if cov < 5 else (cov + 1) // 2 - 1)
    return {"consensus": css, "keys": keys, "summaries": [dict(s, read=tuple(s["read"]), tpl=tuple(s["tpl"])) for s in summ]}


def test_poa_batch_banded_equals_the_handle(P):
    poa, eng = P
    zmws = [_zmw(300 + k, n, p, 10)[0] for k, (n, p) in enumerate(((120, 3), (333, 6), (64, 4), (500, 5), (210, 8)))]
    zmws[1][2] = "A" * 50          # a fallback inside a banded batch
    got = poa.poa_batch(zmws, engine=eng, banded=True)
    for reads, g in zip(zmws, got):
        assert g == _by_handle(poa, eng, reads, True)


def _chunks():
    out = []
    for k, (n, p) in enumerate(((300, 5), (450, 6), (600, 4), (350, 8))):
        out.append({"snr": [10.0, 7.0, 5.0, 11.0], "reads": [{"seq": s} for s in _zmw(400 + k, n, p, 8)[0]]})
    out.append({"snr": [9.0, 9.0, 9.0, 9.0], "reads": [{"seq": "ACG"}]})
    return out


def test_ccs_batch_banded_is_the_banded_draft_then_the_polish(P):
    import math
    import pbccs_amd
    from pbccs_amd import driver
    poa, eng = P
    chunks = _chunks()
    native = driver.ccs_batch(chunks, engine=eng, banded_poa=True)
    ins = driver.zmw_inputs_batch(chunks, engine=eng, banded_poa=True)
    pol = iter(pbccs_amd.polish_zmws([z for st, z in ins if st is None], engine=eng))
    # the draft's reads in FilterReads' order, as Consensus.h hands them to the POA
    drafts = poa.poa_batch([[None if r is None else r["seq"] for r in driver.filter_reads(c["reads"], 10)]
                            for c in chunks[:-1]], engine=eng, banded=True)
    for k, (c, (st, z), got) in enumerate(zip(chunks, ins, native)):
        if st is not None:
            assert got["status"] == st
            continue
        exp = next(pol)
        assert got["draft"] == z["draft"] == drafts[k]["consensus"]
        for key in ("status", "consensus", "qvs", "n_tested", "n_applied", "n_passes", "status_counts"):
            assert got[key] == exp[key], key
        # polish input position i is FilterReads' i-th read; map it back to the subread's input index
        nr = len(c["reads"])
        order = [next(j for j, x in enumerate(c["reads"]) if x is r)
                 for r in driver.filter_reads(c["reads"], 10) if r is not None]
        want_arr, want_z = [-1] * nr, [float("nan")] * nr
        for i, (a, zz) in enumerate(zip(exp["add_read_results"], exp["zscores"])):
            want_arr[order[i]], want_z[order[i]] = a, zz
        assert got["add_read_results"] == want_arr
        for a, b in zip(got["zscores"], want_z):
            assert (math.isnan(a) and math.isnan(b)) or a == b
    assert native[-1]["status"] == "NoSubreads"


def test_switch_off_is_the_old_entry_point_byte_for_byte(P):
    from pbccs_amd import driver, lib as L
    poa, eng = P
    zmws = [_zmw(350 + k, n, p, 10)[0] for k, (n, p) in enumerate(((150, 4), (320, 6)))]
    assert json.dumps(poa.poa_batch(zmws, engine=eng, banded=False)) == json.dumps(poa.poa_batch(zmws, engine=eng))
    po = L.CPoaOptions()
    L.load().pbccs_poa_options_default(ctypes.byref(po))
    assert (po.banded, po.min_coverage) == (0, -1) and po.max_coverage >= 2 ** 62
    # pbccs_poa_batch_ex with banded 0, and with NULL options, against pbccs_poa_batch on the same buffers
    enc = [r.encode() for r in zmws[1]]
    n = len(enc)

    def run(call):
        seqs = (ctypes.c_char_p * n)(*enc)
        lens = (ctypes.c_int * n)(*[len(e) for e in enc])
        cbuf = ctypes.create_string_buffer(4096)
        keys, rc, ext = (ctypes.c_int * n)(), (ctypes.c_int * n)(), (ctypes.c_int * (4 * n))()
        cin = L.CPoaInput(seqs, lens, n)
        cout = L.CPoaOutput(ctypes.cast(cbuf, ctypes.c_char_p), 4096, 0, keys, rc, ext, 0)
        assert call(ctypes.byref(cin), ctypes.byref(cout)) == 0
        return cbuf.raw[:cout.len], list(keys), list(rc), list(ext), cout.n_keys

    lib = L.load()
    old = run(lambda i, o: lib.pbccs_poa_batch(eng._h, i, 1, 2 ** 62, -1, o))
    po.max_coverage = 2 ** 62
    assert run(lambda i, o: lib.pbccs_poa_batch_ex(eng._h, i, 1, ctypes.byref(po), o)) == old
    assert run(lambda i, o: lib.pbccs_poa_batch_ex(eng._h, i, 1, None, o)) == old
    # a handle with the switch off, and one switched on and off again
    a, b = poa.SparsePoa(eng), poa.SparsePoa(eng, banded=True)
    assert lib.pbccs_sparse_poa_set_banded(b._h, 0) == 0
    for r in zmws[0]:
        assert a.OrientAndAddRead(r) == b.OrientAndAddRead(r)
    assert a.ToGraphViz(poa.VERBOSE_NODES) == b.ToGraphViz(poa.VERBOSE_NODES)
    # ccs: banded_poa=False, pbccs_ccs_batch_ex2 with NULL POA options and with banded 0
    chunks = _chunks()[:2]
    base = json.dumps(driver.ccs_batch(chunks, engine=eng))
    assert json.dumps(driver.ccs_batch(chunks, engine=eng, banded_poa=False)) == base
    real = lib.pbccs_ccs_batch_ex2
    for opts in (None, L.CPoaOptions(2 ** 62, -1, 0)):
        seen = []

        def ex2(h, i, n_, co, po_, so, o, opts=opts, seen=seen):
            seen.append(1)
            return real(h, i, n_, co, ctypes.byref(opts) if opts is not None else None, so, o)
        lib.pbccs_ccs_batch_ex2 = ex2
        try:
            assert json.dumps(driver.ccs_batch(chunks, engine=eng, banded_poa=True)) == base and seen
        finally:
            lib.pbccs_ccs_batch_ex2 = real


def test_band_stats_at_600_bases(P):
    poa, eng = P
    zmws = [_zmw(900 + k, 600, 6, 10)[0] for k in range(4)]
    poa.poa_band_stats(eng, reset=True)
    poa.poa_batch(zmws, engine=eng, banded=True)
    s = poa.poa_band_stats(eng, reset=True)
    print("600-base ZMWs: band cells / full cells = %d / %d = %.4f; fallbacks %d of %d alignments" %
          (s["band_cells"], s["full_cells"], s["band_cells"] / s["full_cells"], s["fallbacks"],
           s["fallbacks"] + s["banded_alignments"]))
    assert s["banded_alignments"] > 0 and s["seeds"] > 0 and s["anchors"] > 0
    assert 0 < s["band_cells"] < s["full_cells"]
    assert s["score_bytes"] == 2 * s["band_cells"]


def test_cpp_facade_banded_agrees_with_the_c_abi(P):
    poa, eng = P
    src = os.path.join(ROOT, "tests", "cpp", "poa_band_driver.cpp")
    exe = os.path.join(ROOT, "tests", "cpp", "_build", "poa_band_driver")
    libdir = os.path.join(ROOT, "pbccs_amd", "_lib")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-I" + os.path.join(ROOT, "include"), src, "-L" + libdir,
                           "-lpbccs_amd", "-Wl,-rpath," + libdir, "-o", exe])
    reads = _zmw(950, 220, 5, 10)[0]
    run = subprocess.run([exe], input="\n".join(reads) + "\n", capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    lines = run.stdout.splitlines()
    assert len(lines) == 2 * (len(reads) - 1) + 1
    h = poa.SparsePoa(eng, banded=True)
    at = 0
    for k, r in enumerate(reads):
        for rc in ((0, 1) if k else ()):
            word = lines[at].split()
            at += 1
            assert word[:3] == ["step", str(k), str(rc)]
            assert int(word[3]) == len(h.AlignableRanges(r, bool(rc))["anchors"])
            assert float(word[4]) == h.TryAddRead(r, bool(rc))[0]
        h.OrientAndAddRead(r)
    assert lines[-1] == "consensus " + h.FindConsensus(1)[0]

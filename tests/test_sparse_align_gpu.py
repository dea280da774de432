"""SparseAlign on the device (pbccs_sparse_align_batch) against the reference's recorded chains and against the plain
Python restatement of its rules (tests/sparse_restatement.py), for equality throughout."""
import os
import re
import threading

import pytest

import sparse_restatement as R
from test_sparse_align_cpu import SAME_COLUMN_CASES

pytestmark = pytest.mark.gpu

# the kernels' compile-time edges (pbccs_amd/csrc/sparse_kernels.hpp / .hip)
SWEEP_LDS_COLS = 6144      # kSweepLdsCols: column sets of len1 + K + 1 <= this many columns live in LDS
BLOCK = 256                # kBlock: the chunk of the block scans over positions and K-mer tables
WAVE = 64                  # lanes of the sweep, and the chunk of the position lists
PBCCS_OK, PBCCS_EINVAL, PBCCS_EOOM, PBCCS_ERANGE = 0, -1, -2, -5


@pytest.fixture(scope="module")
def S():
    import pbccs_amd
    from pbccs_amd import sparse
    eng = pbccs_amd.Engine(0)
    sparse.sparse_align_stats(eng, reset=True)
    return sparse, eng


_EXPECTED = {}


def _expect(target, query, k):
    """The restatement's (n_seeds, chain, score), computed once per input."""
    key = (target, query, k)
    if key not in _EXPECTED:
        _EXPECTED[key] = R.sparse_align_full(target, query, k)
    return _EXPECTED[key]


def _check(S, pairs, k, **kw):
    sparse, eng = S
    got = sparse.sparse_align_batch(pairs, k, engine=eng, **kw)
    for (t, q), g in zip(pairs, got):
        n_seeds, chain, score = _expect(t, q, k)
        assert (g["n_seeds"], g["anchors"], g["score"]) == (n_seeds, chain, score), (k, len(t), len(q))
    return got


def test_constants_named_here_are_the_kernels():
    root = os.path.join(R.ROOT, "pbccs_amd", "csrc")
    hpp = open(os.path.join(root, "sparse_kernels.hpp")).read()
    hip = open(os.path.join(root, "sparse_kernels.hip")).read()
    assert int(re.search(r"kSweepLdsCols = (\d+)", hpp).group(1)) == SWEEP_LDS_COLS
    assert int(re.search(r"kBlock = (\d+)", hip).group(1)) == BLOCK


def test_every_golden_case_singly(S):
    sparse, eng = S
    for name, k, t, q, n_seeds, chain in R.golden_cases():
        g, = sparse.sparse_align_batch([(t, q)], k, engine=eng)
        assert g["anchors"] == chain, name
        assert g["n_seeds"] == n_seeds, name


def test_every_golden_case_as_one_batch_per_k(S):
    sparse, eng = S
    cases = R.golden_cases()
    for k in (4, 5, 6, 8):
        mine = [c for c in cases if c[1] == k]
        got = sparse.sparse_align_batch([(c[2], c[3]) for c in mine], k, engine=eng)
        for c, g in zip(mine, got):
            assert (g["anchors"], g["n_seeds"]) == (c[5], c[4]), c[0]
        assert sparse.SparseAlign(mine[0][2], mine[0][3], k, engine=eng) == mine[0][5]


def test_seed_counts_zero_and_one(S):
    g = R.Lcg(5)
    t = g.seq(120)
    one = next(q for q in (g.seq(3) + t[40:46] + g.seq(3) for _ in range(50)) if _expect(t, q, 6)[0] == 1)
    got = _check(S, [(t, "A" * 30), (t, one), ("", "ACGTACGT"), ("ACGTACGT", ""), ("ACG", "ACG"), (t, t[:5])], 6)
    assert [r["n_seeds"] for r in got] == [0, 1, 0, 0, 0, 0]
    assert all(r["anchors"] == [] for r in got)   # one seed alone is no chain: a chain end needs a predecessor


def test_row_groups_and_windows_of_63_64_65(S):
    """Period-2 and period-3 repeats at K = 4: each K-mer's row group holds every second / third target position."""
    pairs = []
    for length in (129, 130, 131, 132):           # period 2: 63/63, 64/63, 64/64, 65/64 positions per K-mer
        pairs.append((("AC" * 80)[:length], ("AC" * 80)[:length - 7]))
        pairs.append((("AC" * 80)[:length], ("CA" * 20)))
    for length in (192, 193, 195, 196):           # period 3: 63, 64/63/63, 64, 65/64/64
        pairs.append((("ACG" * 80)[:length], ("ACG" * 80)[1:length - 20]))
    for t, _ in pairs[:8:2]:
        groups = sorted({sum(1 for i in range(len(t) - 3) if t[i:i + 4] == km) for km in ("ACAC", "CACA")})
        assert groups in ([63], [63, 64], [64], [64, 65])
    _check(S, pairs, 4)


def test_position_chunks_and_scan_chunks(S):
    """Targets and queries whose K-mer positions end one short of, on and one past a 64-position wave chunk and a
    256-element scan chunk."""
    g = R.Lcg(11)
    base = g.seq(600)
    pairs = []
    for k in (4, 6):
        for n in (WAVE - 1, WAVE, WAVE + 1, BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK + 1):
            t = base[:n + k - 1]                  # n K-mer positions
            pairs.append((k, t, g.noisy(t, 10)))
            pairs.append((k, g.noisy(t, 10), t))
    for k in (4, 6):
        _check(S, [(t, q) for kk, t, q in pairs if kk == k], k)


def test_lds_threshold_of_the_column_set(S, monkeypatch):
    """A column set of len1 + K + 1 columns lives in LDS up to kSweepLdsCols and in global memory past it: targets
    one short of, on and one past the compiled threshold, and the same around a threshold forced low, where both
    kinds share one launch.  These three targets of about 6.1 kb, against 300-base queries, are the only inputs of the
    file above 1500 bases: the compiled threshold cannot be met below that."""
    g = R.Lcg(17)
    k = 6
    long_t = g.seq(SWEEP_LDS_COLS)
    pairs = []
    for cols in (SWEEP_LDS_COLS - 1, SWEEP_LDS_COLS, SWEEP_LDS_COLS + 1):
        t = long_t[:cols - k - 1]
        assert len(t) + k + 1 == cols
        pairs.append((t, g.noisy(t[-300:], 12)))
    _check(S, pairs, k)
    monkeypatch.setenv("PBCCS_SPARSE_LDS_COLS", "200")
    small = []
    for cols in (199, 200, 201, 400):
        t = long_t[1000:1000 + cols - k - 1]
        small.append((t, g.noisy(t, 15)))
    _check(S, small, k)
    monkeypatch.setenv("PBCCS_SPARSE_LDS_COLS", "0")   # everything in global memory
    _check(S, small, k)


def test_same_column_keeps_its_old_seed(S):
    for k, spec in SAME_COLUMN_CASES:
        t, q = R.make_pair(spec)
        seeds = R.find_seeds(t, q, k)
        got = _check(S, [(t, q)], k)[0]
        assert got["anchors"] != R.chain_seeds(seeds, k, None, replace_same_column=True)[0]


def test_an_insert_as_in_insert_align(S):
    g = R.Lcg(23)
    t = g.seq(400)
    q = t[:200] + "A" * 40 + t[200:]
    got = _check(S, [(t, q)], 5)[0]["anchors"]
    assert got[0] == (0, 0) and got[-1] == (len(t) - 5, len(q) - 5)


def test_the_largest_input(S):
    g = R.Lcg(29)
    t = g.seq(1500)
    q = (g.noisy(t, 15) + g.seq(200))[:1500]
    got = _check(S, [(t, q)], 6)[0]
    assert 500 < got["n_seeds"] < 8000 and len(got["anchors"]) > 300


def test_reverse_complement_is_formed_on_the_device(S):
    sparse, eng = S
    g = R.Lcg(31)
    jobs = []
    for n, k in ((90, 4), (300, 6), (301, 6), (500, 8)):
        t = g.seq(n)
        q = g.noisy(t, 12)
        jobs += [(k, t, R.revcomp(q), 1), (k, t, q, 0)]
    for k in (4, 6, 8):
        mine = [j for j in jobs if j[0] == k]
        got = sparse.sparse_align_batch([(t, q) for _, t, q, _ in mine], k,
                                        reverse_complement=[f for _, _, _, f in mine], engine=eng)
        for (_, t, q, flag), r in zip(mine, got):
            want = _expect(t, R.revcomp(q) if flag else q, k)
            assert (r["n_seeds"], r["anchors"], r["score"]) == want
            assert len(r["anchors"]) > 10


def test_ranges_equal_the_literal_recursion(S):
    sparse, eng = S
    g = R.Lcg(37)
    t = g.seq(500)
    pairs = [(t, g.noisy(t, 15)),                    # anchors throughout
             (g.seq(500, "AC"), g.seq(300, "GT")),   # nothing shared: no anchors, every position (I, 0)
             (t, t[200:320]),                        # anchors in the middle only: inverted halves on both sides
             (t[:257], g.noisy(t[:257], 5)),
             ("", "ACGTACGT"), (t[:40], "")]
    got = sparse.sparse_align_batch(pairs, 6, ranges=True, engine=eng)
    before = sparse.sparse_align_stats(eng)
    for (tt, q), r in zip(pairs, got):
        _, chain, _ = _expect(tt, q, 6)
        assert r["anchors"] == chain
        assert r["ranges"] == R.ranges_literal(chain, len(tt), len(q))
    assert got[1]["anchors"] == [] and got[1]["ranges"] == [(300, 0)] * 500
    # the cell counters cover exactly the jobs that asked for ranges
    sparse.sparse_align_stats(eng, reset=True)
    sparse.sparse_align_batch(pairs[:3], 6, ranges=True, engine=eng)
    sparse.sparse_align_batch(pairs[:3], 6, engine=eng)
    st = sparse.sparse_align_stats(eng)
    assert st["range_cells"] == sum(R.cells_in_ranges(r["ranges"]) for r in got[:3])
    assert st["full_cells"] == sum(len(tt) * (len(q) + 1) for tt, q in pairs[:3])
    assert st["jobs"] == 6 and st["seeds"] == 2 * sum(r["n_seeds"] for r in got[:3])
    assert st["anchors"] == 2 * sum(len(r["anchors"]) for r in got[:3]) and st["launches"] > 0
    assert before["jobs"] >= 6


def test_a_job_over_the_seed_cap_is_eoom_and_its_neighbours_are_right(S, monkeypatch):
    import pbccs_amd
    sparse, eng = S
    g = R.Lcg(41)
    t = g.seq(300)
    ok_a, ok_b = (t, g.noisy(t, 10)), (t[:150], g.noisy(t[:150], 20))
    heavy = (("AC" * 100), ("AC" * 100))
    n_heavy = _expect(heavy[0], heavy[1], 4)[0]
    assert n_heavy > 4 * max(_expect(*ok_a, 4)[0], _expect(*ok_b, 4)[0])
    monkeypatch.setenv("PBCCS_SPARSE_MAX_SEEDS", str(n_heavy))        # just fits
    _check(S, [ok_a, heavy, ok_b], 4)
    monkeypatch.setenv("PBCCS_SPARSE_MAX_SEEDS", str(n_heavy - 1))    # just exceeds
    sparse.sparse_align_stats(eng, reset=True)
    rc, got = sparse.sparse_align_batch_raw([ok_a, heavy, ok_b], 4, engine=eng)
    assert rc == PBCCS_EOOM
    assert [r["status"] for r in got] == [PBCCS_OK, PBCCS_EOOM, PBCCS_OK]
    assert got[1]["n_seeds"] == n_heavy and got[1]["anchors"] is None
    for pair, r in ((ok_a, got[0]), (ok_b, got[2])):
        assert (r["n_seeds"], r["anchors"], r["score"]) == _expect(*pair, 4)
    assert sparse.sparse_align_stats(eng)["anchors"] == len(got[0]["anchors"]) + len(got[2]["anchors"])
    with pytest.raises(pbccs_amd.PbccsError) as err:
        sparse.sparse_align_batch([heavy], 4, engine=eng)
    assert err.value.code == PBCCS_EOOM
    _check(S, [ok_a, ok_b], 4)                                         # the next call on the engine
    monkeypatch.delenv("PBCCS_SPARSE_MAX_SEEDS")
    _check(S, [heavy], 4)


def test_a_small_workspace_splits_the_batch(S, monkeypatch):
    g = R.Lcg(43)
    pairs = []
    for n in (100, 180, 260, 340):
        t = g.seq(n)
        pairs.append((t, g.noisy(t, 12)))
    monkeypatch.setenv("PBCCS_SPARSE_WORKSPACE_KB", "96")    # half of it, 48 KB, holds one or two of these jobs' arrays (21 to 33 KB at K = 5)
    _check(S, pairs, 5)


def test_invalid_inputs(S):
    import pbccs_amd
    sparse, eng = S
    g = R.Lcg(47)
    t = g.seq(100)
    for k in (3, 9):
        with pytest.raises(pbccs_amd.PbccsError) as err:
            sparse.sparse_align_batch([(t, t)], k, engine=eng)
        assert err.value.code == PBCCS_EINVAL
    rc, got = sparse.sparse_align_batch_raw([(t, t), (t, t[:50] + "N" + t[51:]), (t[:20] + "a" + t[21:], t)], 6,
                                            engine=eng)
    assert rc == PBCCS_EINVAL and [r["status"] for r in got] == [PBCCS_OK, PBCCS_EINVAL, PBCCS_EINVAL]
    assert got[0]["anchors"] == _expect(t, t, 6)[1]
    # an anchor buffer smaller than the chain
    rc, got = sparse.sparse_align_batch_raw([(t, t), (t, t)], 6, engine=eng, anchor_caps=[10, 95])
    assert rc == PBCCS_ERANGE and [r["status"] for r in got] == [PBCCS_ERANGE, PBCCS_OK]
    assert got[0]["n_anchors"] == 95 and got[1]["anchors"] == _expect(t, t, 6)[1]


def _scorer_polish(eng, z):
    """One ZMW polished through the scorer: AddRead, RefineConsensus, ConsensusQVs."""
    import pbccs_amd as P
    g = P.ArrowMultiReadMutationScorer(P.ArrowConfig(z["snr"]), z["draft"], engine=eng)
    added = [g.AddRead(r["seq"], r.get("strand", 0), r.get("ts", 0), r.get("te", len(z["draft"])), float("nan"))
             for r in z["reads"]]
    return added, P.RefineConsensus(g), g.Template(), P.ConsensusQVs(g)


def test_batch_beside_a_polish_on_the_same_engine(S):
    """As test_map_gpu.py's, except that the polish goes through the scorer.  The batch polish gives each workspace
    slot of a new engine a band pool with a 512 GB address range, and a range is never mapped twice in a process
    (DESIGN.md section 2); by the time this module runs, the whole suite in one process has used up the ranges a
    new pool may try.  The scorer's buffers are plain allocations."""
    from pbccs_amd import synth
    sparse, eng = S
    g = R.Lcg(53)
    pairs = []
    for n in (80, 200, 333, 450):
        t = g.seq(n)
        pairs.append((t, g.noisy(t, 15)))
    zmws = synth.make_zmws(3, 300, 6, seed=77)
    want = _check(S, pairs, 6, ranges=True)
    want_pol = [_scorer_polish(eng, z) for z in zmws]
    assert all(w[1][2] >= 0 and w[2] for w in want_pol)
    box = {}
    th = threading.Thread(target=lambda: box.setdefault("pol", [_scorer_polish(eng, z) for z in zmws]))
    th.start()
    got = [sparse.sparse_align_batch(pairs, 6, ranges=True, engine=eng) for _ in range(3)]
    th.join()
    assert all(g_ == want for g_ in got)
    assert box["pol"] == want_pol

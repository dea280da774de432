"""The fill kernels' operand path ("Operand path"): clamped unconditional loads of the previous
column, read bases taken from one load per chunk, plane addressing from group-uniform scalars.  Fills only, through
the scorer: AddRead result, flip-flop count and per-read LL against the restatement, at the band's edges, through
every kernel instantiation (PBCCS_FILL_FIRST_PATH sends short reads through the 64-lane and hybrid kernels) and at
the chunk boundaries of the 16- and 64-lane kernels.

Tolerance: the exact fills repeat the reference's FP64 operation order, so a per-read LL may differ from the
restatement's only by the device `log`'s last place -- 1e-12 relative and absolute, as tests/test_gpu_parity.py asserts
for the fills.  The exact kernels agree with each other bit for bit (`==`).
"""
import pytest

from oracle import oracle as O
from tests.test_gpu_parity import P, _close   # noqa: F401  (P: the module fixture)

pytestmark = pytest.mark.gpu

SNR = [10.0, 7.0, 5.0, 11.0]

# (name, environment): every exact instantiation of k_fill_coop a short read can be sent through
EXACT_PATHS = [
    ("16 lanes", {"PBCCS_FILL_FIRST_PATH": "1"}),
    ("64 lanes, 1 row per lane", {"PBCCS_FILL_FIRST_PATH": "2", "PBCCS_TALL_ROWS": "1"}),
    ("64 lanes, 2 rows per lane", {"PBCCS_FILL_FIRST_PATH": "2", "PBCCS_TALL_ROWS": "2"}),
    ("hybrid, 1 row per lane", {"PBCCS_FILL_FIRST_PATH": "3", "PBCCS_TALL_ROWS": "1", "PBCCS_HYBRID_ROWS": "64"}),
    ("hybrid, 2 rows per lane", {"PBCCS_FILL_FIRST_PATH": "3", "PBCCS_TALL_ROWS": "2", "PBCCS_HYBRID_ROWS": "64"}),
]


def _oracle_fills(tpl, reads):
    o = O.Scorer(tpl, SNR)
    res = [o.add_read(r["seq"], r.get("strand", 0), r.get("ts", 0), r.get("te", len(tpl)), float("nan")) for r in reads]
    info = [o.read_info(k) for k in range(len(reads))]
    return o, res, info


def _gpu_fills(P, tpl, reads, monkeypatch, env, muts=()):
    """AddRead results, flip-flop counts, the active reads' LLs and the scores of `muts`, filled under `env`."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    try:
        g = P.ArrowMultiReadMutationScorer(P.ArrowConfig(SNR), tpl)
        res = [g.AddRead(r["seq"], r.get("strand", 0), r.get("ts", 0), r.get("te", len(tpl)), float("nan"))
               for r in reads]
        flips, lls = g.NumFlipFlops(), g.BaselineScores()
        scores = g.ScoreMany([P.Mutation(t, s, b) for (t, s, b) in muts]) if muts else []
    finally:
        for k in env:
            monkeypatch.delenv(k)
    return res, flips, lls, scores


def _check_fills(got, ref):
    res, flips, lls, _ = got
    _, ores, info = ref
    assert res == ores
    active = [k for k, i in enumerate(info) if i["active"]]
    assert len(lls) == len(active)
    assert len(flips) == len(info)
    for k, x in zip(active, lls):
        y = info[k]["ll"]
        print("read", k, "ll", x, "oracle", y, "flipflops", flips[k], info[k]["flipflops"])
        assert flips[k] == info[k]["flipflops"], k
        assert _close(x, y, 1e-12, 1e-12), (k, x, y)


def _edge_cases():
    """Templates of 3-96 bp with 3-5 synthetic passes on both strands, plus reads of 1-100 bases on partial windows:
    i = 1, j = 1, i = I, row 0, the pinned last cell, and band begins of both parities (both planes)."""
    from pbccs_amd import synth
    cases = []
    for L in (3, 4, 5, 8, 17, 33, 64, 96):
        z = synth.make_zmws(1, L, 3 + L % 3, seed=100 + L)[0]
        cases.append((z["draft"], list(z["reads"])))
    z = synth.make_zmws(1, 96, 5, seed=7)[0]
    tpl = z["draft"]
    n = len(tpl)
    rc = {"A": "T", "C": "G", "G": "C", "T": "A"}
    rev = lambda s: "".join(rc[c] for c in reversed(s))   # noqa: E731
    extra = []
    for ts, te in ((0, 1), (0, 2), (1, 4), (n - 3, n), (n - 1, n), (5, 38), (6, 39), (0, n), (17, n - 16)):
        w = tpl[ts:te]
        extra.append({"seq": w, "strand": 0, "ts": ts, "te": te})                 # the window itself
        extra.append({"seq": rev(w), "strand": 1, "ts": ts, "te": te})            # on the reverse strand
        extra.append({"seq": w[:1] + w[2:], "strand": 0, "ts": ts, "te": te})     # a deletion: odd / even band begins
        extra.append({"seq": w[:1] + "A" + w[1:], "strand": 0, "ts": ts, "te": te})   # an insertion
    extra.append({"seq": (tpl + "ACGT")[:100], "strand": 0, "ts": 0, "te": n})     # 100 bases
    extra.append({"seq": tpl[0], "strand": 0, "ts": 0, "te": n})                    # one base over the whole template
    extra = [r for r in extra if len(r["seq"]) >= 1]
    cases.append((tpl, list(z["reads"]) + extra))
    return cases


def test_fill_edges_match_oracle(P, monkeypatch):
    for tpl, reads in _edge_cases():
        ref = _oracle_fills(tpl, reads)
        _check_fills(_gpu_fills(P, tpl, reads, monkeypatch, {}), ref)


@pytest.fixture(scope="module")
def short_zmws():
    """Short reads every kernel can take, with the restatement's fills: two ZMWs of the chunk-boundary set (their 16-lane
    fills run one and two chunks per column) and the 96 bp edge template with its partial windows."""
    from pbccs_amd import synth
    zs = [(z["draft"], list(z["reads"])) for z in (synth.make_zmws(1, 150, 4, seed=235)[0],
                                                    synth.make_zmws(1, 300, 4, seed=210)[0])]
    zs.append(_edge_cases()[-1])
    return [(tpl, reads, _oracle_fills(tpl, reads)) for tpl, reads in zs]


def test_every_exact_instantiation_agrees_bit_for_bit(P, short_zmws, monkeypatch):
    for tpl, reads, ref in short_zmws:
        muts = O.unique_mutations(tpl)[::3]
        outs = [_gpu_fills(P, tpl, reads, monkeypatch, env, muts) for _, env in EXACT_PATHS]
        _check_fills(outs[0], ref)
        for (name, _), got in zip(EXACT_PATHS[1:], outs[1:]):
            assert got[0] == outs[0][0], name          # AddRead results
            assert got[1] == outs[0][1], name          # flip-flops
            assert got[2] == outs[0][2], name          # LL bits
            assert got[3] == outs[0][3], name          # one round's mutation scores


@pytest.mark.parametrize("rows", ["1", "2"])
def test_short_reads_through_the_batch_tall_path_match_oracle(rows, monkeypatch):
    """The batch entry point with every read started on the 64-lane path: certified scan on (two rows per lane: the scan
    kernel; one row per lane has none and fills exactly) and off.  Records equal the restatement's."""
    import pbccs_amd
    from pbccs_amd import synth
    zs = synth.make_zmws(3, 150, 4, seed=235) + synth.make_zmws(2, 300, 4, seed=210)
    ref = [O.polish_zmw(z["draft"], z["reads"], z["snr"]) for z in zs]
    for scan in ("1", "0"):
        env = {"PBCCS_FILL_FIRST_PATH": "2", "PBCCS_TALL_ROWS": rows, "PBCCS_CERTIFIED_SCAN": scan}
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        try:
            eng = pbccs_amd.Engine(0)
            res = pbccs_amd.polish_zmws(zs, engine=eng)
            c = eng.counters()
        finally:
            for k in env:
                monkeypatch.delenv(k)
        # (the counter is the reads handed to the certified launch; at one row per lane that launch runs the exact kernel)
        assert (c["scan_reads"] > 0) == (scan == "1"), (scan, rows, c["scan_reads"])
        for r, e in zip(res, ref):
            assert r["add_read_results"] == e["add_read_results"]
            assert (r["n_tested"], r["n_applied"]) == (e["n_tested"], e["n_applied"])
            if e["converged"]:
                assert r["consensus"] == e["template"]
                assert max(abs(a - b) for a, b in zip(r["qvs"], e["qvs"])) <= 1
            assert _close(r["zg"], e["zg"], 1e-9) and _close(r["za"], e["za"], 1e-9)


# Chunk boundaries.  Seeds chosen on the CPU with the restatement's pass_log (a read's tallest column per pass):
#   make_zmws(1, 150, 4, seed=235): tallest columns 15 / 20 / 16 / 18 rows  -- 15 and 16: the 16-lane chunk exactly filled
#   make_zmws(1, 150, 4, seed=240): 17 / 16 / 28 / 18                       -- 17: one row into the second chunk
#   make_zmws(1, 2000, 10, seed=351): reads whose passes peak at 63 and 65 rows (the promotion to 64 lanes at 64 rows)
#                                     and one at 905 rows (eight 128-row chunks)
#   make_zmws(1, 2000, 10, seed=341): a pass peaking at 64 rows, another read at 627
#   make_zmws(1, 2000, 10, seed=674): a read whose passes peak at 34 and 129 rows (the second 128-row chunk of a column
#                                     holds one row; its columns reach that peak through 127 and 128 rows, which
#                                     pass_log does not list one by one) and a read at 808 rows (seven chunks)
CHUNK_SEEDS = [(150, 4, 235), (150, 4, 240), (2000, 10, 351), (2000, 10, 341), (2000, 10, 674)]


@pytest.mark.parametrize("length,passes,seed", CHUNK_SEEDS)
def test_fills_at_chunk_boundaries_match_oracle(P, monkeypatch, length, passes, seed):
    from pbccs_amd import synth
    z = synth.make_zmws(1, length, passes, seed=seed)[0]
    reads = list(z["reads"])
    _check_fills(_gpu_fills(P, z["draft"], reads, monkeypatch, {}), _oracle_fills(z["draft"], reads))

"""SparseAlign without a GPU: the plain Python restatement of the reference's rules (tests/sparse_restatement.py)
against the reference's own recorded outputs (tests/golden/sparse_align_ref.json), the six known answers of the
reference's tests/TestSparseAlign.cpp, the range recursion against its closed form, and the ABI's declarations."""
import glob
import json
import os
import re

import pytest

import sparse_restatement as R

ROOT = R.ROOT

# Seeded inputs on which the column set's "an entry already at this column keeps its old seed" rule decides the
# chain (found by searching seeds with chain_seeds(replace_same_column=True) as the counterfactual); frozen here and
# sent to the device by test_sparse_align_gpu.py.
SAME_COLUMN_CASES = [
    (5, {"kind": "copy", "n": 135, "err": 21, "ab": "AT", "seed": 5062}),
    (6, {"kind": "copy", "n": 126, "err": 29, "ab": "AC", "seed": 5522}),
]


def test_golden_file_is_complete_and_small():
    doc = json.load(open(R.GOLDEN))
    assert [c["name"] for c in doc["known_answers"]] == [
        "ExactAlign", "ExactPartial", "InsertAlign", "NoAlign", "SimpleAlign", "LongAlign"]
    seeded = doc["seeded"]
    assert len(seeded) >= 150
    assert {c["k"] for c in seeded} == {4, 5, 6, 8}
    tie_heavy = [c for c in seeded if c["spec"]["kind"] != "copy" or len(c["spec"].get("ab", "ACGT")) == 2]
    assert 2 * len(tie_heavy) >= len(seeded)
    assert {c["spec"]["p"] for c in seeded if c["spec"]["kind"] == "tandem"} == set(range(1, 8))
    assert {"suffix", "prefix", "unrelated", "short"} <= {c["spec"]["kind"] for c in seeded}
    for _, k, t, q, _, _ in R.golden_cases():
        assert len(t) <= 600 or len(q) <= 600 or k == 5   # LongAlign is the reference's own, about 1 kb
    for k in (4, 5, 6, 8):   # lengths K-1, K and K+1 on both sides
        lens = {(len(t), len(q)) for _, kk, t, q, _, _ in R.golden_cases() if kk == k}
        assert {(k - 1, k + 1), (k, k), (k + 1, k), (k + 1, k - 1), (k, k + 1)} <= lens
    others = [os.path.getsize(p) for p in glob.glob(os.path.join(ROOT, "tests", "golden", "*"))
              if os.path.abspath(p) != os.path.abspath(R.GOLDEN)]
    assert os.path.getsize(R.GOLDEN) <= max(others)


def test_restatement_equals_every_recorded_chain():
    cases = R.golden_cases()
    assert len(cases) >= 156
    for name, k, target, query, n_seeds, chain in cases:
        got_seeds, got_chain, _ = R.sparse_align_full(target, query, k)
        assert got_seeds == n_seeds, name
        assert got_chain == chain, name


def test_recorded_chains_increase_strictly_and_fit_the_bound():
    for name, k, target, query, _, chain in R.golden_cases():
        assert len(chain) <= max(0, min(len(target), len(query)) - k + 1), name
        for (h0, v0), (h1, v1) in zip(chain, chain[1:]):
            assert h0 < h1 and v0 < v1, name
        for h, v in chain:
            assert target[h:h + k] == query[v:v + k], name


def test_the_six_known_answers():
    """tests/TestSparseAlign.cpp's own assertions, on the recorded chains and on the restatement."""
    kat = {name: (k, t, q, chain) for name, k, t, q, _, chain in R.golden_cases()[:6]}
    for pick in (lambda k, t, q, chain: chain, lambda k, t, q, chain: R.sparse_align(t, q, k)):
        k, t, q, c = kat["ExactAlign"]
        c = pick(k, t, q, c)
        assert k == 5 and t == q and len(c) == len(t) - k + 1
        assert c[0] == (0, 0) and c[-1] == (len(t) - k, len(t) - k)
        k, t, q, c = kat["ExactPartial"]
        c = pick(k, t, q, c)
        assert len(c) == len(q) - k + 1 and c[0] == (34, 0) and c[-1] == (len(t) - k, len(q) - k)
        k, t, q, c = kat["InsertAlign"]
        c = pick(k, t, q, c)
        assert len(q) - len(t) == 38 and c[0] == (0, 0) and c[-1] == (len(t) - k, len(q) - k)
        k, t, q, c = kat["NoAlign"]
        assert pick(k, t, q, c) == []
        k, t, q, c = kat["SimpleAlign"]
        c = pick(k, t, q, c)
        assert c[0] == (0, 0) and c[-1] == (len(t) - k, len(q) - k)
        k, t, q, c = kat["LongAlign"]
        c = pick(k, t, q, c)
        assert c[0] == (0, 0) and c[-1][0] > 900 and c[-1][1] > 900


def test_where_we_define_instead_of_copying():
    assert R.sparse_align("ACGTACGTAC", "", 5) == []            # the reference dereferences the empty query
    assert R.sparse_align("ACGT", "ACGTACGT", 5) == []           # len1 < K
    assert R.sparse_align("AAAAAAAAAA", "AAAAAAAAAA", 4) == []   # homopolymer K-mers never seed


def test_same_column_cases_hit_the_rule_and_depend_on_it():
    for k, spec in SAME_COLUMN_CASES:
        t, q = R.make_pair(spec)
        seeds = R.find_seeds(t, q, k)
        trace = {}
        kept = R.chain_seeds(seeds, k, trace)
        assert trace["kept_old_seed"] > 0 and trace["kept_old_and_erased"] > 0
        assert R.chain_seeds(seeds, k, None, replace_same_column=True) != kept


def test_range_recursion_equals_the_closed_form():
    checked = 0
    for name, k, target, query, _, chain in R.golden_cases():
        lit = R.ranges_literal(chain, len(target), len(query))
        assert lit == R.ranges_closed_form(chain, len(target), len(query)), name
        checked += 1
        for h, v in chain:   # an anchored position: its anchor's row +- WIDTH, clamped
            assert lit[h] == (max(v - R.WIDTH, 0), min(v + R.WIDTH, len(query))), name
    assert checked >= 156
    # no anchors at all: every position inherits RangeUnion({}) stepped and clamped -> the inverted (I, 0)
    assert R.ranges_literal([], 7, 50) == [(50, 0)] * 7 == R.ranges_closed_form([], 7, 50)
    assert R.ranges_literal([], 0, 5) == [] == R.ranges_closed_form([], 0, 5)
    # one anchor in the middle: forward marks climb to I, reverse marks fall to 0, positions outside keep the
    # inverted half they inherit
    lit = R.ranges_literal([(100, 40)], 200, 60)
    assert lit == R.ranges_closed_form([(100, 40)], 200, 60)
    assert lit[100] == (10, 60) and lit[101] == (11, 60) and lit[99] == (9, 59)
    assert lit[0] == (0, 0) and lit[199] == (60, 60)
    assert R.cells_in_ranges([(50, 0), (3, 10)]) == 7


def test_rle_round_trip():
    for _, _, _, _, _, chain in R.golden_cases():
        assert R.rle_decode(R.rle_encode(chain)) == chain


# ---- the boundary, in the style of tests/test_abi_cpu.py ---------------------------------------------------------
def test_header_declares_and_lib_binds_the_sparse_symbols():
    from pbccs_amd import lib
    hdr = open(os.path.join(ROOT, "include", "pbccs_amd.h")).read()
    declared = set(re.findall(r"\b(pbccs_[a-z_]+)\s*\(", hdr))
    for name in ("pbccs_sparse_align_batch", "pbccs_sparse_align_stats_get"):
        assert name in declared, name
        assert name in lib.SIGNATURES, name
    for struct in ("pbccs_sparse_align_input", "pbccs_sparse_align_output", "pbccs_sparse_align_stats"):
        assert re.search(r"}\s*%s;" % struct, hdr), struct
    import ctypes
    assert [f for f, _ in lib.CSparseAlignOutput._fields_] == ["status", "n_anchors", "n_seeds", "score"]
    assert ctypes.sizeof(lib.CSparseAlignOutput) == 24 and ctypes.sizeof(lib.CSparseAlignInput) == 56
    import pbccs_amd
    assert callable(pbccs_amd.SparseAlign) and callable(pbccs_amd.sparse_align_batch)
    assert callable(pbccs_amd.sparse_align_stats)


def test_library_exports_the_sparse_symbols():
    from pbccs_amd import lib
    if not os.path.exists(lib.LIB_PATH):
        pytest.skip("libpbccs_amd.so not built (run __graft_entry__.build())")
    L = lib.load()
    assert hasattr(L, "pbccs_sparse_align_batch") and hasattr(L, "pbccs_sparse_align_stats_get")


"""The subread pileup on the GPU (pbccs_pileup_columns / pbccs_pileup_batch / pbccs_pileup_msa: k_pile_columns,
k_pile_reduce, k_pile_scan, k_pile_rows).  Expected values come from the Python restatement
(pileup_restatement), fed for the batch calls with the public, already pinned map_batch and align_batch results;
everything is integer arithmetic, so every array is compared for equality."""
import math
import random

import pytest

import pileup_restatement as R

pytestmark = pytest.mark.gpu

ARRAYS = ["counts", "ins_reads", "ins_bases", "slot_cov", "max_ins", "cov", "plurality", "ins_plurality",
          "plurality_sites", "cov_sum", "ec", "n_used"]
PER_READ = ["status", "n_match", "n_mismatch", "n_ins", "n_del"]
PLACEMENT = ["rc", "rb", "re", "tb", "te"]


@pytest.fixture(scope="module")
def P():
    import pbccs_amd
    from pbccs_amd import pileup
    eng = pbccs_amd.Engine(0)
    pileup.pileup_stats(eng, reset=True)
    return pileup, eng


def _same(got, want, what=""):
    for key in ARRAYS:
        assert got[key] == want[key], (what, key)
    assert len(got["reads"]) == len(want["reads"]), what
    for k, (g, w) in enumerate(zip(got["reads"], want["reads"])):
        for key in PER_READ + (PLACEMENT if w["status"] == "used" else []):
            assert g[key] == w[key], (what, k, key)
        assert R.same_concordance(g["concordance"], w["concordance"]), (what, k)
        assert math.isnan(g["concordance"]) == (g["status"] != "used")


def _text(rng, n, alphabet="ACGT"):
    return "".join(rng.choice(alphabet) for _ in range(n))


def _read(rng, tr, rc, L, tb=None, lead=None, alphabet="ACGT"):
    """A pileup read for transcript tr somewhere on a consensus of length L."""
    n_t = sum(c in "MRD" for c in tr)
    n_q = sum(c in "MRI" for c in tr)
    rb = rng.randrange(4) if lead is None else lead
    tb = rng.randrange(L - n_t + 1) if tb is None else tb
    return {"transcript": tr, "rc": rc, "rb": rb, "tb": tb, "te": tb + n_t,
            "seq": _text(rng, rb + n_q + rng.randrange(3), alphabet)}


def _transcript(rng, n, first=None, last=None):
    tr = [rng.choice("MMMMMRID") for _ in range(n)]
    if first:
        tr[0] = first
    if last:
        tr[-1] = last
    return "".join(tr)


def _spanning(rng, L, ins_every=None):
    """A transcript with exactly L consensus columns; ins_every: an insertion run of 1..3 at least that often."""
    tr, t = [], 0
    while t < L:
        c = rng.choice("MMMMMMRD" if ins_every else "MMMMMRID")
        tr.append(c)
        t += c != "I"
        if ins_every and t % ins_every == ins_every // 2 and c != "I":
            tr.append("I" * rng.randrange(1, 4))
    return "".join(tr)


# ------------------------------------------------------------------------------- hand-made transcripts (1)
@pytest.fixture(scope="module")
def hand_made():
    rng = random.Random(24)
    La, Lb, Lc = 260, 97, 300
    a = []
    for k, n in enumerate((1, 63, 64, 65, 127, 128, 129, 200)):   # every chunk boundary of the 64-lane walk
        a.append(_read(rng, _transcript(rng, n), k % 2, La))
        a.append(_read(rng, _transcript(rng, n, "I", "I"), (k + 1) % 2, La))
        a.append(_read(rng, _transcript(rng, n, "D", "D"), k % 2, La))
    a.append(_read(rng, "I" * 70, 1, La))                  # no consensus column
    a.append(_read(rng, "D" * 70, 0, La))                  # no read column
    a.append(_read(rng, "M" * 128, 1, La, tb=0, lead=0))   # exactly two full chunks
    a.append(_read(rng, "M" * 60 + "I" * 10 + "M" * 20, 0, La))       # a run across the chunk boundary
    a.append(_read(rng, "M" * 60 + "I" * 10 + "M" * 20, 1, La, alphabet="ACGTN"))
    a.append(_read(rng, _transcript(rng, 150), 0, La, alphabet="ACGTNacgtY"))   # characters outside ACGT
    # forward reads only, inside [10, 80): positions without coverage at both ends, a strand without reads; the
    # second read's insertion run is longer than a chunk
    b = [_read(rng, "M" * 30 + "D" * 5 + "M" * 20, 0, Lb, tb=10), _read(rng, "R" * 3 + "I" * 66 + "M" * 67, 0, Lb, tb=10)]
    c = [_read(rng, _transcript(rng, 150), 1, Lc, tb=100), _read(rng, "M" * 300, 1, Lc, tb=0),
         _read(rng, "R" * 3 + "I" * 130 + "M" * 67, 1, Lc, alphabet="ACGTN")]   # reverse only; a run over two chunks
    case = [(_text(rng, La), a), (_text(rng, Lb), b), ("", []), (_text(rng, Lc, "ACGTN"), c), ("ACGTA", [])]
    return case, [R.pileup(cons, reads) for cons, reads in case], [R.msa(cons, reads) for cons, reads in case]


def test_columns_on_hand_made_transcripts(P, hand_made):
    pileup, eng = P
    case, want, _ = hand_made
    before = pileup.pileup_stats(eng)
    got = pileup.pileup_columns(case, engine=eng)
    assert len(got) == len(case)
    for z, (g, w) in enumerate(zip(got, want)):
        _same(g, w, z)
    a, b, empty, c, e = got
    assert [r["status"] for r in a["reads"]][24:26] == ["empty_extent", "empty_extent"]
    assert a["reads"][1]["status"] == a["reads"][2]["status"] == "empty_extent"   # "I" and "D" alone
    empties = sum(r["status"] == "empty_extent" for w in want for r in w["reads"])
    assert 4 <= empties <= 5 and a["reads"][3]["status"] == "used"
    assert b["cov"][:10] == [0] * 10 and b["cov"][80:] == [0] * 17 and b["cov"][10] == 2 and b["n_used"] == [2, 0]
    assert b["plurality"][:10] == [255] * 10 and b["counts"][1] == [[0] * 6] * 97 and b["max_ins"][13] == 66
    assert c["n_used"] == [0, 3] and c["counts"][0] == [[0] * 6] * 300 and max(c["max_ins"]) == 130
    assert empty["ec"] == 0.0 and empty["cov"] == [] and empty["slot_cov"] == [0] and empty["plurality_sites"] == []
    assert e["cov"] == [0] * 5 and e["plurality"] == [255] * 5 and e["ec"] == 0.0 and e["n_used"] == [0, 0]
    assert sum(row[5] for s in (0, 1) for row in a["counts"][s]) > 0            # "other" was counted
    assert a["ec"] == a["cov_sum"] / 260 and a["cov_sum"] == sum(a["cov"])
    # each ZMW alone gives what it gave in the batch (an offset bug shows here)
    for z, zmw in enumerate(case):
        _same(pileup.pileup_columns([zmw], engine=eng)[0], got[z], z)
    st = pileup.pileup_stats(eng)
    assert st["skipped_empty_extent"] - before["skipped_empty_extent"] == 2 * empties
    # the batch: both kernels; alone, the two ZMWs without a used read launch the reduction only
    assert st["launches"] - before["launches"] == 2 + 2 * 3 + 2 and st["columns"] > before["columns"]
    assert st["slots"] - before["slots"] == 2 * (260 + 97 + 0 + 300 + 5 + 5)


# ------------------------------------------------------------------------------------- block boundaries (2)
@pytest.fixture(scope="module")
def boundaries():
    from pbccs_amd import pileup
    rng = random.Random(77)
    B = pileup.REDUCE_THREADS
    assert pileup.SCAN_THREADS == B   # one set of lengths puts L + 1 around both kernels' block size
    case = []
    for L in (B - 2, B - 1, B, 2 * B + 37):   # L + 1 one below, at and one above a block; two blocks and a part
        cons = _text(rng, L)
        reads = [_read(rng, _spanning(rng, L, ins_every=50), k % 2, L) for k in range(3)]
        reads.append(_read(rng, _spanning(rng, L - 7), 1, L, tb=3))
        reads.append(_read(rng, "I" * 5 + "M" * 9 + "I" * 4, 0, L, tb=L - 9))   # insertions at the last slot
        case.append((cons, reads))
    return case, [R.pileup(cons, reads) for cons, reads in case], [R.msa(cons, reads) for cons, reads in case]


def test_lengths_around_the_block_sizes(P, boundaries):
    pileup, eng = P
    case, want, _ = boundaries
    B = pileup.REDUCE_THREADS
    for z, (g, w) in enumerate(zip(pileup.pileup_columns(case, engine=eng), want)):
        _same(g, w, z)
        assert g["max_ins"][-1] == 4 and g["slot_cov"][-1] >= 4
    longest = want[-1]["max_ins"]
    assert all(any(longest[k * B:(k + 1) * B]) for k in range(3))   # an insertion in every block: first needs the carry


# ----------------------------------------------------------------------------------------- gapped rows (3)
def _check_rows(case, got, want, pile):
    for z, ((cons, reads), g, w, p) in enumerate(zip(case, got, want, pile)):
        assert g["width"] == w["width"] and g["col"] == w["col"], z
        assert g["rows"] == w["rows"], z
        assert g["width"] == len(cons) + sum(p["max_ins"])
        for r, row, pr in zip(reads, g["rows"], p["reads"]):
            assert len(row) == g["width"]
            if pr["status"] != "used":
                assert row.strip() == ""
                continue
            assert " " not in row.strip()
            assert row.replace("-", "").strip() == R.oriented(r["seq"], r["rc"])[pr["rb"]:pr["re"]]
        for pos in range(len(cons)):   # the rows' columns are the counts: ties the two outputs together
            for s in (0, 1):
                tally = [0] * 6
                for r, row, pr in zip(reads, g["rows"], p["reads"]):
                    ch = row[g["col"][pos]]
                    if pr["status"] == "used" and r["rc"] == s and ch != " ":
                        tally[4 if ch == "-" else R.code_of(ch)] += 1
                assert tally == p["counts"][s][pos], (z, pos, s)


def test_gapped_rows(P, hand_made, boundaries):
    pileup, eng = P
    for case, pile, want in (hand_made, boundaries):
        got = pileup.pileup_msa(case, engine=eng)
        _check_rows(case, got, want, pileup.pileup_columns(case, engine=eng))
        for z in (0, len(case) - 1):
            assert pileup.pileup_msa([case[z]], engine=eng)[0] == got[z]
    assert pileup.pileup_stats(eng)["launches"] > 0


# -------------------------------------------------------------------------------------------- refusals (4)
def test_refuses_transcripts_that_leave_their_extents(P):
    import pbccs_amd
    pileup, eng = P
    ok = {"transcript": "MMMM", "rc": 0, "rb": 0, "tb": 2, "te": 6, "seq": "ACGT"}
    cons = "ACGTACGTAC"
    launches = pileup.pileup_stats(eng)["launches"]
    for bad in ({"transcript": "MMXM"}, {"transcript": "MMM"}, {"te": 11, "transcript": "M" * 9, "seq": "ACGTACGTA"},
                {"rb": 1}, {"tb": -1, "te": 3}):
        for call in (pileup.pileup_columns, pileup.pileup_msa):
            with pytest.raises(pbccs_amd.PbccsError) as e:
                call([(cons, [ok]), (cons, [dict(ok, **bad)])], engine=eng)
            assert e.value.code == -1, bad
    assert pileup.pileup_stats(eng)["launches"] == launches   # refused before any device work
    assert pileup.pileup_columns([(cons, [ok])], engine=eng)[0]["cov"] == [0, 0, 1, 1, 1, 1, 0, 0, 0, 0]


# ---------------------------------------------------------------------------------- batch: ground truth (5)
def test_copies_of_the_consensus_through_the_batch(P):
    pileup, eng = P
    rng = random.Random(5)
    cons = _text(rng, 60)
    rev = lambda s: R.oriented(s, 1)   # noqa: E731
    g = pileup.pileup_batch([(cons, [cons, rev(cons), cons, None])], engine=eng)[0]
    assert [r["status"] for r in g["reads"]] == ["used", "used", "used", "unmapped"]
    for p, ch in enumerate(cons):
        hot = [1 if c == "ACGT".index(ch) else 0 for c in range(6)]
        assert g["counts"][0][p] == [2 * h for h in hot] and g["counts"][1][p] == hot
    assert [r["concordance"] for r in g["reads"][:3]] == [1.0] * 3 and math.isnan(g["reads"][3]["concordance"])
    assert g["ec"] == 3.0 and g["cov_sum"] == 180 and g["plurality_sites"] == [] and g["n_used"] == [2, 1]
    assert [r["rc"] for r in g["reads"][:3]] == [0, 1, 0] and g["ins_reads"] == [[0] * 61] * 2
    # three of four reads: a substitution at 30 and one inserted base before 45 that differs from both neighbours
    sub = next(c for c in "ACGT" if c not in cons[29:32])
    ins = next(c for c in "ACGT" if c not in cons[44:46])
    mut = cons[:30] + sub + cons[31:45] + ins + cons[45:]
    g = pileup.pileup_batch([(cons, [mut, rev(mut), mut, rev(cons)])], transcripts=True, engine=eng)[0]
    assert g["plurality_sites"] == [("sub", 30, cons[30], sub), ("ins", 45, cons[45], "+")]
    want_tr = "M" * 30 + "R" + "M" * 14 + "I" + "M" * 15
    assert [r["transcript"] for r in g["reads"]] == [want_tr, want_tr, want_tr, "M" * 60]
    assert g["counts"][0][30]["ACGT".index(sub)] == 2 and g["counts"][1][30]["ACGT".index(sub)] == 1
    assert g["counts"][1][30]["ACGT".index(cons[30])] == 1 and g["ins_reads"][0][45] == 2 and g["ins_reads"][1][45] == 1
    assert g["slot_cov"] == [4] * 61 and g["ins_plurality"][45] == 1 and sum(g["ins_plurality"]) == 1
    assert g["reads"][0]["concordance"] == 59 / 61 and g["cov_sum"] == 240 and g["ec"] == 4.0


# ---------------------------------------------------------------------------- batch against the restatement
def _expected(eng, zmws):
    """The restatement over map_batch's placements and align_batch's transcripts, all ZMWs in two device calls.
    Returns (results, transcripts per read)."""
    from pbccs_amd import align, mapping
    placed = mapping.map_batch([(c, [None if r is None else r["seq"] for r in reads]) for c, reads in zmws],
                               engine=eng)
    pairs, where = [], []
    for z, ((c, reads), pl) in enumerate(zip(zmws, placed)):
        for k, (r, p) in enumerate(zip(reads, pl)):
            if r is None or p is None:
                continue
            (rb, re_), (tb, te) = p["read"], p["tpl"]
            if re_ <= rb or te <= tb:
                continue
            pairs.append((c[tb:te], R.oriented(r["seq"], 1 if p["rc"] else 0)[rb:re_]))
            where.append((z, k))
    alns, _ = align.align_batch(pairs, align.NW, engine=eng) if pairs else ([], [])
    trs = [[None] * len(reads) for _, reads in zmws]
    for (z, k), a in zip(where, alns):
        trs[z][k] = a.Transcript()
    return [R.batch(c, reads, pl, tr) for (c, reads), pl, tr in zip(zmws, placed, trs)], trs


@pytest.fixture(scope="module")
def synthetic(P):
    from pbccs_amd import synth
    pileup, eng = P
    zs = synth.make_zmws(8, 300, 6, seed=1234)
    zmws = [(z["draft"], [{"seq": r["seq"]} for r in z["reads"]]) for z in zs]
    want, trs = _expected(eng, zmws)
    return zmws, want, trs, pileup.pileup_batch(zmws, transcripts=True, engine=eng)


def test_batch_equals_the_restatement(P, synthetic):
    zmws, want, trs, got = synthetic
    for z, (g, w) in enumerate(zip(got, want)):
        _same(g, w, z)
        assert g["n_used"] == [3, 3] and {r["status"] for r in g["reads"]} == {"used"}
        assert [r["transcript"] for r in g["reads"]] == trs[z]
        assert max(g["cov"]) == 6 and 4.0 < g["ec"] <= 6.0


def test_batch_equals_one_by_one_and_banded(P, synthetic):
    pileup, eng = P
    zmws, _, _, got = synthetic
    for z in (0, 5):
        _same(pileup.pileup_batch([zmws[z]], engine=eng)[0], got[z], z)
    for z, g in enumerate(pileup.pileup_batch(zmws, band=True, transcripts=True, engine=eng)):
        _same(g, got[z], ("band", z))
        assert [r["transcript"] for r in g["reads"]] == [r["transcript"] for r in got[z]["reads"]]
    import numpy as np
    for z, g in enumerate(pileup.pileup_batch(zmws[:3], arrays=True, engine=eng)):   # the same numbers as arrays
        assert g["counts"].shape == (2, len(zmws[z][0]), 6) and g["counts"].dtype == np.int32
        for key in ARRAYS[:8]:
            assert np.asarray(g[key]).tolist() == got[z][key], (z, key)
        assert g["plurality_sites"] == got[z]["plurality_sites"] and g["reads"][0]["re"] == got[z]["reads"][0]["re"]
    rows = pileup.pileup_batch(zmws[:2], msa=True, engine=eng)
    for z, g in enumerate(rows):
        _same(g, got[z], ("msa", z))
        assert "transcript" not in g["reads"][0]
        m = R.msa(zmws[z][0], [dict(seq=r["seq"], **{k: p[k] for k in ("transcript", "rc", "rb", "tb", "te")})
                               for r, p in zip(zmws[z][1], got[z]["reads"])])
        assert (g["width"], g["col"], g["rows"]) == (m["width"], m["col"], m["rows"])


# ------------------------------------------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def ccs_runs(P, tmp_path_factory):
    """Six 300-base ZMWs from a subread BAM with kinetics tracks, through ccs_batch plain, with the pileup, with the
    kinetics and with both."""
    from pbccs_amd import bamio, driver, kinetics, mapping, synth
    pileup, eng = P
    rng = random.Random(9)
    zs = synth.make_zmws(6, 300, 6, seed=4321)
    lines = []
    for hole, z in enumerate(zs):
        qs = 0
        for r in z["reads"]:
            n = len(r["seq"])
            lines.append(bamio.subread_sam_line("mvP", hole, qs, qs + n, r["seq"], z["snr"],
                                                ip=[rng.randrange(300) for _ in range(n)],
                                                pw=[rng.randrange(60) for _ in range(n)]))
            qs += n + 40
    p = tmp_path_factory.mktemp("pileup") / "subreads.bam"
    bamio.write_bam(str(p), "@HD\tVN:1.5\tSO:unknown\n", lines)
    chunks, _ = bamio.group_subread_bam(str(p))
    assert len(chunks) == 6
    runs = {"chunks": chunks, "plain": driver.ccs_batch(chunks, engine=eng),
            "pile": driver.ccs_batch(chunks, engine=eng, pileup=True)}
    mapping.map_stats(eng, reset=True)
    runs["kin"] = driver.ccs_batch(chunks, engine=eng, kinetics=True)
    runs["kin_jobs"] = mapping.map_stats(eng, reset=True)["jobs"]
    pileup.pileup_stats(eng, reset=True)
    kinetics.kinetics_stats(eng, reset=True)
    runs["both"] = driver.ccs_batch(chunks, engine=eng, kinetics=True, pileup=True)
    runs["both_jobs"] = mapping.map_stats(eng)["jobs"]
    runs["both_stats"] = (pileup.pileup_stats(eng), kinetics.kinetics_stats(eng))
    return runs


def _polished(res):
    return [z for z, r in enumerate(res) if r["status"] in ("Success", "PoorQuality")]


def test_ccs_batch_with_the_pileup(P, ccs_runs, tmp_path):
    from pbccs_amd import bamio, ccsio, driver
    pileup, eng = P
    chunks, plain, res = ccs_runs["chunks"], ccs_runs["plain"], ccs_runs["pile"]
    # with pileup=False the records are today's, field for field (through repr: NaN z-scores compare equal)
    assert repr(driver.ccs_batch(chunks, engine=eng, pileup=False)) == repr(plain)
    ok = _polished(res)
    assert len(ok) >= 4
    for z, (r, q) in enumerate(zip(res, plain)):
        assert repr({k: v for k, v in r.items() if k not in ("pileup", "ec")}) == repr(q)
        assert ("pileup" in r) == (z in ok) == ("ec" in r) and "pileup" not in q and "ec" not in q
    want, _ = _expected(eng, [(res[z]["consensus"], [r for r, a in zip(chunks[z]["reads"], res[z]["add_read_results"])
                                                     if a == 0]) for z in ok])
    sam = [ccsio.ccs_sam_record("mvP", chunks[z]["hole"], res[z], chunks[z]["snr"], pileup=True) for z in ok]
    out = tmp_path / "ccs.bam"
    bamio.write_ccs_bam(str(out), ["mvP"], sam)
    _, back = bamio.read_bam(str(out))
    assert back == sam
    for z, w, line in zip(ok, want, back):
        _same(res[z]["pileup"], w, z)
        assert res[z]["ec"] == w["ec"] and w["ec"] > 3.0
        last = line.split("\t")[-1]
        assert last == "ec:f:" + ccsio._f32(w["ec"])
        no_tag = ccsio.ccs_sam_record("mvP", chunks[z]["hole"], res[z], chunks[z]["snr"])
        assert line == no_tag + "\t" + last


def test_subread_alignment_records_round_trip(P, ccs_runs, tmp_path):
    from pbccs_amd import bamio, ccsio, driver
    pileup, eng = P
    chunks = ccs_runs["chunks"]
    res = driver.ccs_batch(chunks, engine=eng, pileup={"transcripts": True, "msa": True})
    ok = _polished(res)
    refs, lines, spans = [], [], []
    for z in ok:
        name = f"mvP/{chunks[z]['hole']}/ccs"
        refs.append((name, len(res[z]["consensus"])))
        pile = res[z]["pileup"]
        _same(pile, ccs_runs["pile"][z]["pileup"], z)   # the options add keys, they change none
        assert len(pile["rows"]) == len(pile["reads"]) and all(len(row) == pile["width"] for row in pile["rows"])
        reads = [r for r, a in zip(chunks[z]["reads"], res[z]["add_read_results"]) if a == 0]
        for r, pr in zip(reads, pile["reads"]):
            if pr["status"] != "used":
                continue
            lines.append(ccsio.subread_alignment_sam_record(name, r["name"], r["seq"], pr))
            spans.append((len(r["seq"]), pr["te"] - pr["tb"], pr))
    assert len(lines) >= 4 * 5
    p = tmp_path / "aligned.bam"
    bamio.write_aligned_bam(str(p), "@HD\tVN:1.5\tSO:unknown\n", refs, lines)
    header, back_refs, back = bamio.read_aligned_bam(str(p))
    assert back == lines and back_refs == refs and header.startswith("@HD")
    flags = set()
    for line, (n_read, n_ref, pr) in zip(back, spans):
        f = line.split("\t")
        ops = bamio._parse_cigar(f[5])
        assert sum(n for n, op in ops if "MIDNSHP=X"[op] in "IS=X") == n_read == len(f[9])
        assert sum(n for n, op in ops if "MIDNSHP=X"[op] in "D=X") == n_ref
        assert int(f[3]) == pr["tb"] + 1 and f[1] == ("16" if pr["rc"] else "0")
        assert f[11] == f"NM:i:{pr['n_mismatch'] + pr['n_ins'] + pr['n_del']}"
        assert f[12] == "mc:f:" + ccsio._f32(pr["concordance"])
        flags.add(f[1])
    assert flags == {"0", "16"}


def test_kinetics_and_pileup_share_one_placement(P, ccs_runs):
    kin_keys = [f"{s}_{t}{x}" for s in ("fwd", "rev") for t in ("ipd", "pw") for x in ("", "_mean", "_cov")] + ["fn", "rn"]
    chunks, both = ccs_runs["chunks"], ccs_runs["both"]
    ok = _polished(both)
    assert ok == _polished(ccs_runs["kin"]) == _polished(ccs_runs["pile"]) and len(ok) >= 4
    n_reads = 0
    for z in ok:
        for key in kin_keys:
            assert both[z][key] == ccs_runs["kin"][z][key], (z, key)
        assert repr(both[z]["pileup"]) == repr(ccs_runs["pile"][z]["pileup"]) and both[z]["ec"] == ccs_runs["pile"][z]["ec"]
        n_reads += sum(a == 0 for a in both[z]["add_read_results"])
    for z in set(range(len(both))) - set(ok):
        assert "pileup" not in both[z] and "fn" not in both[z]
    pst, kst = ccs_runs["both_stats"]
    # every read went through the placement stage once, and its transcript fed both features
    assert pst["placed"] == pst["shared"] == pst["reads"] == kst["reads"] == n_reads
    assert ccs_runs["both_jobs"] == ccs_runs["kin_jobs"] > 0

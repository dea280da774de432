"""Consensus kinetics on the GPU (pbccs_kinetics_pileup / pbccs_kinetics_batch: k_kin_columns, k_kin_reduce;
DESIGN.md §3.22).  Expected values come from the Python restatement (kinetics_restatement) fed with the public,
already pinned map_batch and align_batch results; every array is compared for equality."""
import random

import pytest

import kinetics_restatement as R

pytestmark = pytest.mark.gpu

KEYS = [f"{s}_{t}{x}" for s in ("fwd", "rev") for t in ("ipd", "pw") for x in ("", "_mean", "_cov")] + ["fn", "rn"]


@pytest.fixture(scope="module")
def K():
    import pbccs_amd
    from pbccs_amd import kinetics
    eng = pbccs_amd.Engine(0)
    kinetics.kinetics_stats(eng, reset=True)
    return kinetics, eng


def _same(got, want, what=""):
    for key in KEYS:
        assert got[key] == want[key], (what, key)


def _frames(rng, n):
    """Frames over the whole range, with both ends common."""
    return [rng.choice((0, 65535, rng.randrange(64), rng.randrange(1000), rng.randrange(65536))) for _ in range(n)]


def _read(rng, tr, rc, L, tb=None, lead=None):
    """A pileup read for transcript tr somewhere on a consensus of length L."""
    n_t = sum(c in "MRD" for c in tr)
    n_q = sum(c in "MRI" for c in tr)
    rb = rng.randrange(4) if lead is None else lead
    length = rb + n_q + rng.randrange(3)
    tb = rng.randrange(L - n_t + 1) if tb is None else tb
    return {"transcript": tr, "rc": rc, "rb": rb, "tb": tb, "te": tb + n_t, "len": length,
            "ip": _frames(rng, length), "pw": _frames(rng, length)}


def _transcript(rng, n, first=None, last=None):
    tr = [rng.choice("MMMMMRID") for _ in range(n)]
    if first:
        tr[0] = first
    if last:
        tr[-1] = last
    return "".join(tr)


# ------------------------------------------------------------------------------- pileup, hand-made transcripts
def _pileup_case():
    rng = random.Random(22)
    La, Lb, Lc = 260, 97, 300
    a = []
    for k, n in enumerate((1, 63, 64, 65, 127, 128, 129, 200)):   # every chunk boundary of the 64-lane walk
        a.append(_read(rng, _transcript(rng, n), k % 2, La))
        a.append(_read(rng, _transcript(rng, n, "I", "I"), (k + 1) % 2, La))
        a.append(_read(rng, _transcript(rng, n, "D", "D"), k % 2, La))
    a.append(_read(rng, "D" * 70, 0, La))                  # an empty query
    a.append(_read(rng, "I" * 70, 1, La))                  # an empty target extent
    a.append(_read(rng, "M" * 128, 1, La, tb=0, lead=0))   # exactly two full chunks
    nopw = _read(rng, _transcript(rng, 90), 0, La)
    nopw["pw"] = None                                      # a read without one track
    a.append(nopw)
    # forward reads only, inside [10, 80): positions without coverage at both ends, a strand without reads
    b = [_read(rng, "M" * 30 + "D" * 5 + "M" * 20, 0, Lb, tb=10), _read(rng, "R" * 3 + "I" * 66 + "M" * 67, 0, Lb, tb=10)]
    c = [_read(rng, _transcript(rng, 150), 1, Lc, tb=100), _read(rng, "M" * 300, 1, Lc, tb=0)]   # reverse only
    return [(La, a), (Lb, b), (0, []), (Lc, c), (5, [])]


def test_pileup_on_hand_made_transcripts(K):
    kinetics, eng = K
    case = _pileup_case()
    got = kinetics.kinetics_pileup(case, engine=eng)
    assert len(got) == len(case)
    for z, ((L, reads), g) in enumerate(zip(case, got)):
        want = R.pileup(L, reads)
        _same(g, want, z)
        assert len(g["fwd_ipd"]) == L and len(g["rev_pw_cov"]) == L
    a, b, _, c, e = got
    empty = 0
    for (L, reads), g in zip(case, got):   # a transcript without a target or without a query column is skipped
        want = ["used" if set(r["transcript"]) & set("MRD") and set(r["transcript"]) & set("MRI") else "empty_extent"
                for r in reads]
        assert g["read_status"] == want
        empty += want.count("empty_extent")
    assert a["read_status"][24:26] == ["empty_extent", "empty_extent"] and a["read_status"][3] == "used"
    assert b["fwd_ipd_cov"][:10] == [0] * 10 and b["fwd_ipd_cov"][80:] == [0] * 17 and b["fwd_ipd_cov"][10] == 2
    assert b["rn"] == 0 and b["rev_ipd_mean"] == [0] * 97 and b["rev_ipd"] == [0] * 97 and b["fn"] == 2
    assert c["fn"] == 0 and c["rn"] == 2
    assert e["fwd_ipd_cov"] == [0] * 5 and (e["fn"], e["rn"]) == (0, 0)
    assert a["fwd_pw_cov"] != a["fwd_ipd_cov"]             # the read without pw
    # each ZMW alone gives what it gave in the batch (an offset bug shows here)
    for z, (L, reads) in enumerate(case):
        _same(kinetics.kinetics_pileup([(L, reads)], engine=eng)[0], got[z], z)
    st = kinetics.kinetics_stats(eng)
    assert st["skipped_empty_extent"] == 2 * empty and st["launches"] >= 2 and st["columns"] > 0


def test_pileup_extremes(K):
    kinetics, eng = K
    n = 130
    reads = [{"transcript": "M" * n, "rc": rc, "rb": 0, "tb": 0, "te": n, "len": n, "ip": [65535] * n, "pw": [0] * n}
             for rc in (0, 1, 0, 1, 0)]
    g = kinetics.kinetics_pileup([(n, reads)], engine=eng)[0]
    assert g["fwd_ipd_mean"] == [65535] * n and g["fwd_ipd"] == [255] * n and g["fwd_ipd_cov"] == [3] * n
    assert g["rev_ipd_mean"] == [65535] * n and g["rev_pw_mean"] == [0] * n and g["rev_pw"] == [0] * n
    # rounding: {1, 2} -> 2, {1, 1, 2} -> 1
    one = [{"transcript": "M", "rc": 0, "rb": 0, "tb": 0, "te": 1, "len": 1, "ip": [v], "pw": [w]}
           for v, w in ((1, 1), (2, 1), (0, 2))]
    g = kinetics.kinetics_pileup([(1, one[:2]), (1, one)], engine=eng)
    assert g[0]["fwd_ipd_mean"] == [2] and g[1]["fwd_pw_mean"] == [1] and g[1]["fwd_ipd_mean"] == [1]


def test_pileup_refuses_transcripts_that_leave_their_extents(K):
    import pbccs_amd
    kinetics, eng = K
    ok = {"transcript": "MMMM", "rc": 0, "rb": 0, "tb": 2, "te": 6, "len": 4, "ip": [1] * 4, "pw": [1] * 4}
    for bad in ({"transcript": "MMXM"}, {"transcript": "MMM"}, {"te": 11, "transcript": "M" * 9, "len": 9,
                                                               "ip": [1] * 9, "pw": [1] * 9},
                {"rb": 1}, {"tb": -1, "te": 3}):
        with pytest.raises(pbccs_amd.PbccsError) as e:
            kinetics.kinetics_pileup([(10, [dict(ok, **bad)])], engine=eng)
        assert e.value.code == -1, bad
    assert kinetics.kinetics_pileup([(10, [ok])], engine=eng)[0]["fwd_ipd_cov"] == [0, 0, 1, 1, 1, 1, 0, 0, 0, 0]


# ------------------------------------------------------------------------------------- batch: ground truth
def test_forward_and_reverse_copies_through_the_batch(K):
    kinetics, eng = K
    rng = random.Random(5)
    cons = "".join(rng.choice("ACGT") for _ in range(40))
    n = len(cons)
    own = [10 + i for i in range(n)]                       # in the read's own coordinates
    reads = [{"seq": cons, "ip": own, "pw": [4] * n}, {"seq": R.revcomp(cons), "ip": own, "pw": [6] * n},
             {"seq": cons, "ip": own, "pw": [4] * n}, None]
    g = kinetics.kinetics_batch([(cons, reads)], engine=eng)[0]
    assert g["read_status"] == ["used", "used", "used", "unmapped"]
    assert g["fwd_ipd_mean"] == [10 + p for p in range(n)] and g["fwd_ipd_cov"] == [2] * n
    assert g["rev_ipd_mean"] == [10 + k for k in range(n)] and g["rev_ipd_cov"] == [1] * n
    assert g["fwd_pw_mean"] == [4] * n and g["rev_pw_mean"] == [6] * n
    assert g["fwd_ipd"] == [10 + p for p in range(n)] and (g["fn"], g["rn"]) == (2, 1)


# ---------------------------------------------------------------------------- batch against the restatement
def _tracked(zs, seed):
    rng = random.Random(seed)
    out = []
    for z in zs:
        out.append([{"seq": r["seq"], "ip": _frames(rng, len(r["seq"])), "pw": _frames(rng, len(r["seq"]))}
                    for r in z["reads"]])
    return out


def _expected(eng, zmws):
    """The restatement over map_batch's placements and align_batch's transcripts, all ZMWs in two device calls."""
    from pbccs_amd import align, mapping
    placed = mapping.map_batch([(c, [None if r is None else r["seq"] for r in reads]) for c, reads in zmws],
                               engine=eng)
    pairs, where = [], []
    for z, ((c, reads), pl) in enumerate(zip(zmws, placed)):
        ps, idx = R.pairs_for(c, reads, pl)
        pairs += ps
        where += [(z, k) for k in idx]
    alns, _ = align.align_batch(pairs, align.NW, engine=eng) if pairs else ([], [])
    trs = [[None] * len(reads) for _, reads in zmws]
    for (z, k), a in zip(where, alns):
        trs[z][k] = a.Transcript()
    return [R.batch(c, reads, pl, tr) for (c, reads), pl, tr in zip(zmws, placed, trs)]


@pytest.fixture(scope="module")
def synthetic(K):
    from pbccs_amd import synth
    kinetics, eng = K
    zs = synth.make_zmws(8, 300, 6, seed=1234)
    zmws = [(z["draft"], reads) for z, reads in zip(zs, _tracked(zs, 8))]
    return zmws, _expected(eng, zmws), kinetics.kinetics_batch(zmws, engine=eng)


def test_batch_equals_the_restatement(K, synthetic):
    zmws, want, got = synthetic
    for z, (g, w) in enumerate(zip(got, want)):
        _same(g, w, z)
        assert g["fn"] == 3 and g["rn"] == 3 and set(g["read_status"]) == {"used"}
        assert max(g["fwd_ipd_cov"]) == 3 and max(g["rev_pw_cov"]) == 3


def test_batch_equals_one_by_one_and_banded(K, synthetic):
    kinetics, eng = K
    zmws, _, got = synthetic
    for z in (0, 5):
        _same(kinetics.kinetics_batch([zmws[z]], engine=eng)[0], got[z], z)
    for z, g in enumerate(kinetics.kinetics_batch(zmws, band=True, engine=eng)):
        _same(g, got[z], ("band", z))


# ------------------------------------------------------------------------------------------------ end to end
def test_subread_bam_to_ccs_bam_with_kinetics(K, tmp_path):
    from pbccs_amd import bamio, ccsio, driver, synth
    kinetics, eng = K
    zs = synth.make_zmws(6, 300, 6, seed=4321)
    tracks = _tracked(zs, 9)
    lines = []
    for hole, (z, reads) in enumerate(zip(zs, tracks)):
        qs = 0
        for r in reads:
            lines.append(bamio.subread_sam_line("mvK", hole, qs, qs + len(r["seq"]), r["seq"], z["snr"], ip=r["ip"],
                                                pw=r["pw"]))
            qs += len(r["seq"]) + 40
    p = tmp_path / "subreads.bam"
    bamio.write_bam(str(p), "@HD\tVN:1.5\tSO:unknown\n", lines)
    chunks, _ = bamio.group_subread_bam(str(p))
    assert len(chunks) == 6 and all(r["ip"] == t["ip"] for c, ts in zip(chunks, tracks) for r, t in zip(c["reads"], ts))
    res = driver.ccs_batch(chunks, engine=eng, kinetics=True)
    plain = driver.ccs_batch(chunks, engine=eng)
    # with kinetics=False the records are today's, field for field (through repr: NaN z-scores compare equal)
    assert repr(driver.ccs_batch(chunks, engine=eng, kinetics=False)) == repr(plain)
    ok = [z for z, r in enumerate(res) if r["status"] in ("Success", "PoorQuality")]
    assert len(ok) >= 4
    extra = set(KEYS)
    for r, q in zip(res, plain):
        assert repr({k: v for k, v in r.items() if k not in extra}) == repr(q)
        assert not extra & set(q)
    want = _expected(eng, [(res[z]["consensus"], [r for r, a in zip(chunks[z]["reads"], res[z]["add_read_results"])
                                                  if a == 0]) for z in ok])
    sam = [ccsio.ccs_sam_record("mvK", chunks[z]["hole"], res[z], chunks[z]["snr"], kinetics=True) for z in ok]
    out = tmp_path / "ccs.bam"
    bamio.write_ccs_bam(str(out), ["mvK"], sam)
    _, back = bamio.read_bam(str(out))
    assert back == sam
    for z, w, line in zip(ok, want, back):
        _same(res[z], w, z)
        t = {x[:2]: x.split(":", 2)[2] for x in line.split("\t")[11:]}
        for tag, key in (("fi", "fwd_ipd"), ("fp", "fwd_pw"), ("ri", "rev_ipd"), ("rp", "rev_pw")):
            codes = [int(v) for v in t[tag].split(",")[1:]]
            assert t[tag].startswith("C") and codes == w[key]
            assert kinetics.codec_v1_decode(codes) == [R.decode(c) for c in w[key]]
        assert (int(t["fn"]), int(t["rn"])) == (w["fn"], w["rn"]) and w["fn"] + w["rn"] >= 3

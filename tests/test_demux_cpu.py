"""Barcode demultiplexing on the CPU: the restatement pinned to things it did not come from, the
call rules, the host-side refusals, the ABI mirrors against a stand-in that reads the C structs, and the SAM / BAM
tags."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import align_modes_restatement as AM
import demux_restatement as R
import pbccs_amd
from pbccs_amd import bamio, ccsio, demux, driver
from pbccs_amd import lib as L
from pbccs_amd.align import AlignParams, InvalidInputError, UnsupportedFeatureError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARAMS = [(3, -5, -4, -4), (1, -1, -1, -1), (4, -13, -7, -7)]


def rand_seq(rng, n, alphabet="ACGT"):
    return "".join(alphabet[k] for k in rng.integers(0, len(alphabet), n))


def small_cases():
    """(window, barcode): ties, homopolymers, a window shorter than the barcode, an empty window, raw bytes."""
    rng = np.random.default_rng(5)
    cases = [("", "ACGT"), ("A", "ACGT"), ("ACG", "ACGTACGT"), ("AAAAAAAA", "AAA"), ("AAAAAAAA", "A"),
             ("ACACACACAC", "CACA"), ("ACACACACAC", "ACAC"), ("TTTTACGTTTTT", "ACGT"), ("ACGTTTTTACGT", "ACGT"),
             ("acgtACGNacgt", "ACGT"), ("GGGG", "T"), ("GATTACA", "GATTACA"), ("CCCCCCCC", "CCCCCCCCCCCC")]
    for _ in range(40):
        cases.append((rand_seq(rng, int(rng.integers(0, 14)), "ACGTNa"), rand_seq(rng, int(rng.integers(1, 9)))))
    for _ in range(20):   # two letters: many equal-score paths
        cases.append((rand_seq(rng, int(rng.integers(1, 14)), "AC"), rand_seq(rng, int(rng.integers(1, 7)), "AC")))
    return cases


@pytest.mark.parametrize("params", PARAMS)
def test_semiglobal_equals_the_ends_free_restatement(params):
    for t, q in small_cases():
        _, score, ext = AM.align_ends(t, q, AM.SEMIGLOBAL, params)
        assert R.semiglobal(t, q, params) == (score, ext["target"]), (t, q)


def test_revcomp_is_the_ends_free_restatement_s():
    for s in ("ACGT", "AACCGGTTN", "acgtNM-", b"GATTACA"):
        assert R.revcomp(s) == AM.revcomp(s)


@pytest.mark.parametrize("params", PARAMS)
def test_end_scores_and_extents_equal_align_ends_on_windows(params):
    rng = np.random.default_rng(11)
    barcodes = [rand_seq(rng, k) for k in (1, 2, 5, 8, 8, 3)]
    for n in (0, 1, 4, 7, 8, 9, 15, 16, 17, 40):
        read = rand_seq(rng, n, "ACGTn")
        W = 8
        lead, trail = R.end_scores(read, barcodes, W, params)
        off = max(0, n - W)
        for b, s in enumerate(barcodes):
            assert lead[b] == AM.align_ends(read[:min(W, n)], s, AM.SEMIGLOBAL, params)[1]
            assert trail[b] == AM.align_ends(read[off:], AM.revcomp(s), AM.SEMIGLOBAL, params)[1]
        e = R.demux_one(read, barcodes, params, window=W)
        lx = AM.align_ends(read[:min(W, n)], barcodes[e["lead"]], AM.SEMIGLOBAL, params)[2]["target"]
        tx = AM.align_ends(read[off:], AM.revcomp(barcodes[e["trail"]]), AM.SEMIGLOBAL, params)[2]["target"]
        assert e["lead_extent"] == lx and e["trail_extent"] == (off + tx[0], off + tx[1])


@pytest.mark.parametrize("params", PARAMS)
def test_scores_np_equals_the_plain_form(params):
    rng = np.random.default_rng(3)
    barcodes = [rand_seq(rng, k) for k in (1, 2, 7, 8, 9, 16, 16, 5)] + ["AAAAAAAA", "ACACACAC"]
    reads = [rand_seq(rng, n, "ACGTNa") for n in (0, 1, 5, 12, 13, 23, 24, 25, 60, 60)] + ["A" * 30, "AC" * 20]
    S = R.scores_np(reads, barcodes, 12, params, chunk=3)
    for k, r in enumerate(reads):
        lead, trail = R.end_scores(r, barcodes, 12, params)
        assert S[k, 0].tolist() == lead and S[k, 1].tolist() == trail, r


def test_a_planted_exact_barcode_scores_match_times_length_with_exact_extents():
    rng = np.random.default_rng(8)
    barcodes = [rand_seq(rng, 16) for _ in range(12)]
    for i, j in ((0, 0), (3, 7), (11, 2)):
        pad_l, pad_r = rand_seq(rng, 3), rand_seq(rng, 5)
        insert = rand_seq(rng, 200)
        read = pad_l + barcodes[i] + insert + R.revcomp(barcodes[j]) + pad_r
        e = R.demux_one(read, barcodes, min_quality=demux.MIN_QUALITY)
        assert (e["lead"], e["trail"], e["called"]) == (i, j, True)
        assert e["pair"] == (min(i, j), max(i, j))
        assert e["best"] == ((i, 48), (j, 48)) and e["score"] == 96 and e["quality"] == 100
        assert e["lead_extent"] == (3, 19) and e["trail_extent"] == (3 + 16 + 200, 3 + 16 + 200 + 16)
        assert e["clip"] == (19, 219) and read[e["clip"][0]:e["clip"][1]] == insert and not e["overlap"]


def test_the_designs_agree_on_a_noise_free_symmetric_molecule():
    rng = np.random.default_rng(9)
    barcodes = [rand_seq(rng, 16) for _ in range(24)]
    for i in (0, 5, 23):
        read = barcodes[i] + rand_seq(rng, 150) + R.revcomp(barcodes[i])
        a = R.demux_one(read, barcodes, design="asymmetric")
        s = R.demux_one(read, barcodes, design="symmetric")
        for key in ("lead", "trail", "pair", "called", "score", "quality", "lead_extent", "trail_extent", "clip"):
            assert a[key] == s[key], key
        assert a["lead"] == a["trail"] == i


def test_duplicates_take_the_smallest_index_and_lead_by_zero():
    lens = [4, 4, 4, 4]
    c = R.call([5, 12, 12, 3], [7, 7, 2, 7], lens, 3)
    assert (c["lead"], c["trail"], c["score"], c["score_lead"]) == (1, 0, 19, 0)
    assert c["best"] == ((1, 12), (0, 7)) and c["second"] == (12, 7)
    s = R.call([5, 12, 12, 3], [7, 7, 7, 7], lens, 3, design="symmetric")
    assert (s["lead"], s["trail"], s["score"], s["score_lead"]) == (1, 1, 19, 0)
    assert R.call([5, 12, 12, 3], [7, 7, 2, 7], lens, 3, min_score_lead=1)["called"] is False


def test_one_barcode_has_no_second_and_an_unbounded_lead():
    for design in ("asymmetric", "symmetric"):
        c = R.call([9], [6], [4], 3, design=design, min_score_lead=10**6)
        assert c["second"] == (None, None) and c["score_lead"] == R.INT_MAX and c["called"]
        assert c["pair"] == (0, 0)


def test_quality_formula_and_its_clamps_and_the_gates():
    assert R.quality(96, 3, 16, 16) == 100 and R.quality(95, 3, 16, 16) == 98      # floor(9500 / 96) = 98
    assert R.quality(-1, 3, 16, 16) == 0 and R.quality(-500, 3, 16, 16) == 0 and R.quality(0, 3, 1, 1) == 0
    assert R.quality(10**6, 3, 16, 16) == 100
    assert R.quality(1, 3, 16, 16) == 1 and R.quality(47, 3, 8, 8) == 97           # floor(4700 / 48) = 97
    c = R.call([40, 10], [44, 8], [16, 16], 3, min_quality=87)
    assert c["quality"] == 87 and c["called"] and c["pair"] == (0, 0)               # floor(8400 / 96) = 87
    u = R.call([40, 10], [44, 8], [16, 16], 3, min_quality=88)
    assert not u["called"] and u["pair"] == (-1, -1)
    assert (u["lead"], u["trail"], u["score"], u["score_lead"], u["quality"]) == (0, 0, 84, 30, 87)   # still filled
    assert not R.call([40, 10], [44, 8], [16, 16], 3, min_score_lead=31)["called"]
    assert R.call([40, 10], [44, 8], [16, 16], 3, min_score_lead=30)["called"]


def test_overlapping_windows_set_overlap_and_drop_the_clip():
    bc = ["ACGTACGT", "TTTTGGGG"]
    read = "ACGTACGT"[:6]                      # one short read: both ends find their barcode in the same bases
    e = R.demux_one(read, bc, window=8)
    assert e["overlap"] and e["clip"] is None and e["lead_extent"][1] > e["trail_extent"][0]
    whole = bc[0] + R.revcomp(bc[1])           # windows 2 W - 1 and wider than the read: no insert, no overlap
    e = R.demux_one(whole, bc, window=15)
    assert (e["lead"], e["trail"]) == (0, 1) and e["clip"] == (8, 8) and not e["overlap"]
    e = R.demux_one("", bc, window=8)
    assert e["clip"] == (0, 0) and not e["overlap"] and e["best"] == ((0, -32), (0, -32)) and e["score_lead"] == 0


# ---- refusals: on the host, before an engine exists ---------------------------------------------------------------
def _no_engine(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("an engine or the library was touched")
    monkeypatch.setattr(pbccs_amd, "default_engine", boom)
    monkeypatch.setattr(demux, "load", boom)


@pytest.mark.parametrize("barcodes", [["ACGN"], ["acgt"], [""], ["A" * 65], [], ["ACGT", "AC-T"]])
def test_bad_barcode_sets_are_refused(monkeypatch, barcodes):
    _no_engine(monkeypatch)
    with pytest.raises(InvalidInputError):
        demux.demux_batch(["ACGT"], barcodes)
    with pytest.raises(InvalidInputError):
        demux.BarcodeSet(barcodes)


@pytest.mark.parametrize("kw", [{"params": AlignParams(0, -5, -4, -4)}, {"params": AlignParams(-1, -5, -4, -4)},
                                {"params": AlignParams(3, -5, 1, -4)}, {"params": AlignParams(3, -5, -4, 1)},
                                {"window": 0}, {"window": 1025}, {"window_mult": 17}, {"window_mult": 0},
                                {"design": "both"}, {"design": None},
                                {"params": AlignParams(2**20, -5, -4, -4), "window": 1024}])
def test_bad_options_are_refused(monkeypatch, kw):
    _no_engine(monkeypatch)
    with pytest.raises(InvalidInputError):
        demux.demux_batch(["ACGT"], ["A" * 64], **kw)
    with pytest.raises(InvalidInputError):
        driver.ccs_batch([], barcodes=dict(kw, barcodes=["A" * 64]))


def test_too_many_barcodes_are_refused(monkeypatch):
    _no_engine(monkeypatch)
    with pytest.raises(InvalidInputError):
        demux.BarcodeSet(["ACGT"] * 65536)
    assert len(demux.BarcodeSet(["ACGT"] * 65535)) == 65535


def test_barcode_set_from_fasta_keeps_names(tmp_path):
    p = tmp_path / "bc.fasta"
    p.write_text(">bc1001 first\nACGTACGT\nAC\n>bc1002\nTTTT\n")
    bs = demux.BarcodeSet.from_fasta(str(p))
    assert bs.seqs == ["ACGTACGTAC", "TTTT"] and bs.names == ["bc1001 first", "bc1002"] and bs.longest == 10
    assert bs.name(1) == "bc1002" and demux.BarcodeSet(["AC"]).name(0) == "0"


# ---- the ABI mirrors --------------------------------------------------------------------------------------------
class _FakeLib:
    """pbccs_demux_batch stand-in: reads the barcodes, options and reads through the ctypes layout of the C structs,
    answers by the restatement and writes every output array."""

    def pbccs_demux_batch(self, h, bc, opts, reads, n, out):
        bc, o, out = bc._obj, opts._obj, out._obj
        barcodes = [bc.seqs[k][:bc.lens[k]].decode() for k in range(bc.n)]
        B = bc.n
        for r in range(n):
            seq = ctypes.string_at(reads[r].seq, reads[r].len).decode("latin-1") if reads[r].len else ""
            lead, trail = R.end_scores(seq, barcodes, o.window, (o.match, o.mismatch, o.insert, o.delete_))
            e = R.demux_one(seq, barcodes, (o.match, o.mismatch, o.insert, o.delete_),
                            "symmetric" if o.design else "asymmetric", o.window, 3, o.min_quality, o.min_score_lead,
                            scores=(lead, trail))
            out.lead[r], out.trail[r], out.called[r] = e["lead"], e["trail"], int(e["called"])
            out.score[r], out.score_lead[r], out.quality[r] = e["score"], e["score_lead"], e["quality"]
            for k, v in enumerate(e["lead_extent"] + e["trail_extent"]):
                out.extents[4 * r + k] = v
            for k, v in enumerate(e["clip"] or (-1, -1)):
                out.clip[2 * r + k] = v
            out.overlap[r] = int(e["overlap"])
            for end in range(2):
                sec = e["second"][end]
                for k, v in enumerate((e["best"][end][1], e["best"][end][0], demux.INT_MIN if sec is None else sec)):
                    out.best[6 * r + 3 * end + k] = v
            if out.scores:
                for b in range(B):
                    out.scores[(2 * r) * B + b], out.scores[(2 * r + 1) * B + b] = lead[b], trail[b]
        return 0


class _Eng:
    _h = None


@pytest.mark.parametrize("design", ["asymmetric", "symmetric"])
def test_demux_batch_marshalling_round_trip(monkeypatch, design):
    monkeypatch.setattr(demux, "load", lambda: _FakeLib())
    rng = np.random.default_rng(4)
    barcodes = [rand_seq(rng, k) for k in (8, 8, 5, 1)]
    reads = ["", "A", barcodes[0] + rand_seq(rng, 30) + R.revcomp(barcodes[2]), rand_seq(rng, 12), b"ACGTnnACGT",
             barcodes[3]]
    kw = dict(params=AlignParams(2, -3, -2, -1), design=design, window=10, min_quality=50, min_score_lead=1)
    got, scores = demux.demux_batch(reads, barcodes, return_scores=True, engine=_Eng(), **kw)
    text = [r.decode() if isinstance(r, bytes) else r for r in reads]
    want = R.demux(text, barcodes, params=(2, -3, -2, -1), design=design, window=10, min_quality=50,
                   min_score_lead=1)
    assert got == want
    assert scores.shape == (len(reads), 2, 4) and scores.dtype == np.int32
    for r, s in zip(text, scores):
        assert (s[0].tolist(), s[1].tolist()) == R.end_scores(r, barcodes, 10, (2, -3, -2, -1))
    assert demux.demux_batch(reads, demux.BarcodeSet(barcodes), engine=_Eng(), **kw) == want
    assert demux.demux_batch([], barcodes, engine=_Eng()) == []


def test_the_ctypes_mirrors_have_the_header_s_layout(tmp_path):
    """sizeof and every offsetof of the demux structs, as a C compiler sees include/pbccs_amd.h."""
    structs = {"pbccs_demux_barcodes": L.CDemuxBarcodes, "pbccs_demux_options": L.CDemuxOptions,
               "pbccs_demux_read": L.CDemuxRead, "pbccs_demux_output": L.CDemuxOutput,
               "pbccs_demux_stats": L.CDemuxStats}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "pbccs_amd.h"', "int main(void) {"]
    for name, c in structs.items():
        lines.append(f'printf("{name} %zu\\n", sizeof({name}));')
        for f, _ in c._fields_:
            lines.append(f'printf("{name}.{f} %zu\\n", offsetof({name}, {f}));')
    lines += [f'printf("MIN_QUALITY %d\\n", PBCCS_DEMUX_MIN_QUALITY);', "return 0; }"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict(line.rsplit(" ", 1) for line in subprocess.check_output([str(exe)], text=True).splitlines())
    for name, c in structs.items():
        assert int(got[name]) == ctypes.sizeof(c)
        for f, _ in c._fields_:
            assert int(got[f"{name}.{f}"]) == getattr(c, f).offset, (name, f)
    assert int(got["MIN_QUALITY"]) == demux.MIN_QUALITY
    for sym in ("pbccs_demux_options_default", "pbccs_demux_batch", "pbccs_demux_stats_get", "pbccs_ccs_batch_demux"):
        assert sym in L.SIGNATURES


def test_the_measured_default_is_the_midpoint_on_record():
    import json
    with open(os.path.join(ROOT, "profiles", "demux.json")) as f:
        m = json.load(f)["min_quality"]
    assert m["free_reads"] >= 2000 and m["planted_reads"] >= 2000
    assert m["free_max_quality"] < m["planted_min_quality"]
    assert demux.MIN_QUALITY == m["min_quality_default"] == (m["free_max_quality"] + m["planted_min_quality"]) // 2


# ---- SAM / BAM ---------------------------------------------------------------------------------------------------
def _result(called=True, overlap=False):
    cons = "ACGTACGTAAGGCCTTAACCGGTTTGCATGCA"
    e = {"lead": 3, "trail": 1, "pair": (1, 3) if called else (-1, -1), "called": called, "score": 90,
         "score_lead": 40, "quality": 93, "lead_extent": (0, 8), "trail_extent": (24, 32),
         "clip": None if overlap else (8, 24), "overlap": overlap, "best": ((3, 45), (1, 45)), "second": (5, 5)}
    return {"consensus": cons, "qvs": list(range(10, 10 + len(cons))), "n_passes": 7, "predicted_accuracy": 0.999,
            "za": 1.5, "zscores": [0.5, -0.25], "add_read_results": [0, 0], "status_counts": [2, 0, 0, 0, 0],
            "ec": 6.5, "barcode": e}


def test_barcode_tags_follow_every_other_tag():
    res = _result()
    snr = (8.0, 9.0, 10.0, 11.0)
    plain = ccsio.ccs_sam_record("m", 7, res, snr, pileup=True)
    rec = ccsio.ccs_sam_record("m", 7, res, snr, pileup=True, barcode=True)
    assert rec == plain + "\tbc:B:S,1,3\tbq:i:93"
    assert ccsio.ccs_sam_record("m", 7, res, snr, barcode=False) == ccsio.ccs_sam_record("m", 7, res, snr)
    uncalled = _result(called=False)
    assert ccsio.ccs_sam_record("m", 7, uncalled, snr, barcode=True) == ccsio.ccs_sam_record("m", 7, uncalled, snr)
    assert ccsio.ccs_sam_record("m", 7, uncalled, snr, barcode="clip") == ccsio.ccs_sam_record("m", 7, uncalled, snr)


def test_clip_trims_seq_and_qual_and_refuses_the_per_base_tags():
    res = _result()
    snr = (8.0, 9.0, 10.0, 11.0)
    plain = ccsio.ccs_sam_record("m", 7, res, snr).split("\t")
    rec = ccsio.ccs_sam_record("m", 7, res, snr, barcode="clip").split("\t")
    assert rec[9] == res["consensus"][8:24] and rec[10] == plain[10][8:24]
    assert rec[:9] == plain[:9] and rec[11:] == plain[11:] + ["bc:B:S,1,3", "bq:i:93", "bx:B:i,8,8"]
    whole = ccsio.ccs_sam_record("m", 7, _result(overlap=True), snr, barcode="clip").split("\t")
    assert whole[9:11] == plain[9:11] and whole[-1] == "bx:B:i,0,0"
    for kw in ({"rich": True}, {"kinetics": True}, {"pileup": True}):
        with pytest.raises(UnsupportedFeatureError):
            ccsio.ccs_sam_record("m", 7, res, snr, barcode="clip", **kw)
    with pytest.raises(ValueError):
        ccsio.ccs_sam_record("m", 7, res, snr, barcode="trim")


def test_barcode_records_round_trip_through_bam(tmp_path):
    snr = (8.0, 9.0, 10.0, 11.0)
    lines = [ccsio.ccs_sam_record("m", 7, _result(), snr, barcode=True),
             ccsio.ccs_sam_record("m", 8, _result(), snr, barcode="clip"),
             ccsio.ccs_sam_record("m", 9, _result(called=False), snr, barcode=True)]
    path = str(tmp_path / "ccs.bam")
    bamio.write_ccs_bam(path, ["m"], lines)
    _, back = bamio.read_bam(path)
    assert back == lines

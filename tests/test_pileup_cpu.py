"""Host-side checks of the subread pileup: the restatement on hand-worked cases, cigar(), the
aligned BAM round trip, the records, and argument validation that raises before any engine exists."""
import math
import os
import random

import pytest

import pileup_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _read(tr, seq, rc=0, rb=0, tb=0):
    return {"transcript": tr, "seq": seq, "rc": rc, "rb": rb, "tb": tb, "te": tb + sum(c in "MRD" for c in tr)}


# ----------------------------------------------------------------------------------------- the restatement
def test_restatement_on_a_hand_worked_zmw():
    cons = "ACGT"
    reads = [_read("MMMM", "ACGT"),                      # the consensus itself
             _read("MRDM", "ATT"),                       # A, T over C, gap over G, T
             _read("RIIRM", "AGGGT", rc=1, tb=1),        # oriented ACCCT: A over C, CC inserted, C over G, T
             _read("III", "AAA"),                        # no consensus column: skipped
             None]
    g = R.pileup(cons, reads)
    assert [r["status"] for r in g["reads"]] == ["used", "used", "used", "empty_extent", "unmapped"]
    assert g["counts"][0] == [[2, 0, 0, 0, 0, 0], [0, 1, 0, 1, 0, 0], [0, 0, 1, 0, 1, 0], [0, 0, 0, 2, 0, 0]]
    assert g["counts"][1] == [[0, 0, 0, 0, 0, 0], [1, 0, 0, 0, 0, 0], [0, 1, 0, 0, 0, 0], [0, 0, 0, 1, 0, 0]]
    assert g["ins_reads"] == [[0, 0, 0, 0, 0], [0, 0, 1, 0, 0]] and g["ins_bases"] == [[0] * 5, [0, 0, 2, 0, 0]]
    assert g["slot_cov"] == [2, 3, 3, 3, 3] and g["max_ins"] == [0, 0, 2, 0, 0]
    assert g["cov"] == [2, 3, 3, 3] and g["cov_sum"] == 11 and g["ec"] == 2.75 and g["n_used"] == [2, 1]
    # position 1: A C T tie, the consensus's own C wins; position 2: C G gap tie, the consensus's own G wins
    assert g["plurality"] == [0, 1, 2, 3] and g["ins_plurality"] == [0] * 5 and g["plurality_sites"] == []
    assert [r["concordance"] for r in g["reads"][:3]] == [1.0, 0.5, 0.2] and math.isnan(g["reads"][3]["concordance"])
    third = g["reads"][2]
    assert (third["n_match"], third["n_mismatch"], third["n_ins"], third["n_del"], third["re"]) == (1, 2, 2, 0, 5)
    m = R.msa(cons, reads)
    assert m["width"] == 6 and m["col"] == [0, 1, 4, 5]
    assert m["rows"] == ["AC--GT", "AT---T", " ACCCT", "      ", "      "]


def test_restatement_plurality_ties_and_sites():
    # two reads disagree at position 1 (G against the consensus's C, and T): the lowest code of the tie wins
    g = R.pileup("ACA", [_read("MRM", "AGA"), _read("MRM", "ATA")])
    assert g["plurality"] == [0, 2, 0] and g["plurality_sites"] == [("sub", 1, "C", "G")]
    # a deletion and an insertion in two of three reads; N does not compete
    reads = [_read("MDM", "AA"), _read("MDIM", "AGA"), _read("MMIM", "ANGA")]
    g = R.pileup("ACA", reads)
    assert g["counts"][0][1] == [0, 0, 0, 0, 2, 1] and g["plurality"][1] == 4
    assert g["ins_reads"][0] == [0, 0, 2, 0] and g["ins_plurality"] == [0, 0, 1, 0]
    assert g["plurality_sites"] == [("del", 1, "C", "-"), ("ins", 2, "A", "+")]
    assert R.pileup("", [])["ec"] == 0.0 and R.pileup("AC", [])["plurality"] == [255, 255]
    # insertions at the ends: right-aligned before tb, left-aligned after te, no padding outside the extent
    m = R.msa("ACA", [_read("IIMMMI", "GGACAT"), _read("IMMM", "TACA"), _read("M", "C", tb=1)])
    assert m["rows"] == ["GGACAT", " TACA ", "   C  "] and m["col"] == [2, 3, 4]


def test_restatement_invariants_on_random_cases():
    rng = random.Random(7)
    for _ in range(200):
        L = rng.randrange(1, 30)
        cons = "".join(rng.choice("ACGT") for _ in range(L))
        reads = []
        for _ in range(rng.randrange(1, 6)):
            tb = rng.randrange(L)
            te = rng.randrange(tb + 1, L + 1)
            tr, need = [], te - tb
            while need:
                c = rng.choice("MMMRID")
                tr.append(c)
                need -= c in "MRD"
            tr += ["I"] * rng.randrange(3)
            rb = rng.randrange(3)
            nq = sum(c in "MRI" for c in tr)
            seq = "".join(rng.choice("ACGTN") for _ in range(rb + nq + rng.randrange(3)))
            reads.append(dict(_read("".join(tr), seq, rng.randrange(2), rb, tb)))
        m, g = R.msa(cons, reads), R.pileup(cons, reads)
        for r, row, pr in zip(reads, m["rows"], g["reads"]):
            assert len(row) == m["width"]
            if pr["status"] != "used":
                assert row.strip() == ""
                continue
            assert " " not in row.strip()
            assert row.replace("-", "").strip() == R.oriented(r["seq"], r["rc"])[r["rb"]:pr["re"]]
        for p in range(L):   # the columns of the rows are the counts
            for s in (0, 1):
                col = [row[m["col"][p]] for r, row, pr in zip(reads, m["rows"], g["reads"])
                       if pr["status"] == "used" and r["rc"] == s and row[m["col"][p]] != " "]
                want = [0] * 6
                for ch in col:
                    want[4 if ch == "-" else R.code_of(ch)] += 1
                assert want == g["counts"][s][p]


# ------------------------------------------------------------------------------------------------- cigar()
def test_cigar():
    from pbccs_amd import pileup
    assert pileup.cigar("MMRIIDM", 2, 10) == "2S2=1X2I1D1=2S"
    assert pileup.cigar("M", 0, 1) == "1=" and pileup.cigar("IIMMDD", 0, 4) == "2I2=2D"
    assert pileup.cigar("", 0, 0) == "" and pileup.cigar("", 3, 5) == "3S2S"
    rng = random.Random(1)
    for _ in range(50):
        tr = "".join(rng.choice("MRID") for _ in range(rng.randrange(1, 40)))
        rb, tail = rng.randrange(3), rng.randrange(3)
        n = rb + sum(c != "D" for c in tr) + tail
        assert pileup.cigar(tr, rb, n) == R.cigar(tr, rb, n)
    with pytest.raises(ValueError):
        pileup.cigar("MMX", 0, 3)
    with pytest.raises(ValueError):
        pileup.cigar("MMM", 0, 2)


# ------------------------------------------------------------------------------------------------- records
def _pile_read(tr, rc, rb, tb):
    d = {"status": "used", "transcript": tr, "rc": rc, "rb": rb, "tb": tb, "n_match": tr.count("M"),
         "n_mismatch": tr.count("R"), "n_ins": tr.count("I"), "n_del": tr.count("D")}
    d["concordance"] = d["n_match"] / len(tr)
    return d


def test_subread_alignment_record_and_aligned_bam_round_trip(tmp_path):
    from pbccs_amd import bamio, ccsio
    fwd = ccsio.subread_alignment_sam_record("m/7/ccs", "m/7/0_9", "TTACGTNAC", _pile_read("MMRIMDM", 0, 2, 4))
    assert fwd.split("\t") == ["m/7/0_9", "0", "m/7/ccs", "5", "255", "2S2=1X1I1=1D1=1S", "*", "0", "0", "TTACGTNAC",
                               "*", "NM:i:3", "mc:f:" + ccsio._f32(4 / 7)]
    rev = ccsio.subread_alignment_sam_record("m/7/ccs", "m/7/20_24", "AACX", _pile_read("MMMM", 1, 0, 0))
    assert rev.split("\t")[1:6] == ["16", "m/7/ccs", "1", "255", "4="] and rev.split("\t")[9] == "NGTT"
    other = ccsio.subread_alignment_sam_record("m/9/ccs", "m/9/0_3", "ACG", _pile_read("MDDM", 0, 1, 70000))
    with pytest.raises(ValueError):
        ccsio.subread_alignment_sam_record("m/7/ccs", "x", "ACG", {"status": "unmapped"})
    p = str(tmp_path / "aligned.bam")
    refs = [("m/7/ccs", 120), ("m/9/ccs", 80000)]
    offs = bamio.write_aligned_bam(p, "@HD\tVN:1.5\tSO:unknown\n", refs, [fwd, rev, other])
    assert len(offs) == 3 and offs[0] < offs[1] < offs[2]
    header, back_refs, lines = bamio.read_aligned_bam(p)
    assert header == "@HD\tVN:1.5\tSO:unknown\n" and back_refs == refs and lines == [fwd, rev, other]
    # the byte layout: refID, pos, bin from the alignment's end, the CIGAR words
    import struct
    rec = bamio.aligned_sam_to_bam_record(other, {"m/7/ccs": 0, "m/9/ccs": 1})
    ref, pos, _, mapq, bin_, ncig, flag, lseq = struct.unpack_from("<iiBBHHHI", rec, 4)
    assert (ref, pos, mapq, ncig, flag, lseq) == (1, 70000, 255, 4, 0, 3)
    assert bin_ == bamio._reg2bin(70000, 70004) == 4681 + (70000 >> 14)
    assert struct.unpack_from("<4I", rec, 36 + len("m/9/0_3") + 1) == (1 << 4 | 4, 1 << 4 | 7, 2 << 4 | 2, 1 << 4 | 7)
    with pytest.raises(ValueError):
        bamio.write_aligned_bam(p, "", [("other", 5)], [fwd])
    # the unaligned reader still reads the file's header and skips the dictionary
    assert bamio.read_bam(p)[0] == ""


def test_ccs_record_ec_tag_follows_every_other_tag():
    from pbccs_amd import ccsio
    res = {"qvs": [20, 30], "zscores": [0.5], "add_read_results": [0], "n_passes": 3, "predicted_accuracy": 0.99,
           "za": 0.1, "status_counts": [1, 0, 0, 0, 0], "consensus": "AC", "ec": 8.7}
    plain = ccsio.ccs_sam_record("m", 5, res, [5, 6, 7, 8])
    assert ccsio.ccs_sam_record("m", 5, res, [5, 6, 7, 8], pileup=False) == plain
    assert ccsio.ccs_sam_record("m", 5, res, [5, 6, 7, 8], pileup=True) == plain + "\tec:f:" + ccsio._f32(8.7)


# --------------------------------------------------------------------------------- validation, no engine
class _NoEngine:
    @property
    def _h(self):
        raise AssertionError("the engine was touched")


def test_arguments_are_refused_before_an_engine_exists():
    import pbccs_amd
    from pbccs_amd import driver, pileup
    ok = _read("MM", "AC")
    bad_inputs = [[("AC", [dict(ok, transcript=None)])], [("AC", [{"seq": "AC"}])], [("AC", ["MM"])],
                  [("AC", [dict(ok, tb="x")])], [("AC", [dict(ok, te=2**40)])], [(None, [])],
                  [("Aሴ", [])]]
    for bad in bad_inputs:
        for call in (pileup.pileup_columns, pileup.pileup_msa):
            with pytest.raises(pbccs_amd.PbccsError) as e:
                call(bad, engine=_NoEngine())
            assert e.value.code == -1
    for bad in ([("AC", [5])], [("AC", [{"seq": None}])], [(7, [])]):
        with pytest.raises(pbccs_amd.PbccsError) as e:
            pileup.pileup_batch(bad, engine=_NoEngine())
        assert e.value.code == -1
    with pytest.raises(ValueError):
        pileup.pileup_batch([("AC", ["AC"])], band="wide", engine=_NoEngine())
    for bad in ("yes", {"rows": True}, 3):
        with pytest.raises(ValueError):
            driver.ccs_batch([], engine=_NoEngine(), pileup=bad)


def test_header_bindings_and_exports():
    import pbccs_amd
    from pbccs_amd import lib
    hdr = open(os.path.join(ROOT, "include", "pbccs_amd.h")).read()
    for name in ("pbccs_pileup_options_default", "pbccs_pileup_columns", "pbccs_pileup_batch", "pbccs_pileup_msa",
                 "pbccs_pileup_stats_get"):
        assert name in lib.SIGNATURES and name + "(" in hdr, name
        if os.path.exists(lib.LIB_PATH):
            assert hasattr(lib.load(), name)
    for name in ("pileup_batch", "pileup_columns", "pileup_msa", "pileup_stats"):
        assert hasattr(pbccs_amd, name)
    import ctypes
    assert ctypes.sizeof(lib.CPileupRead) == 48 and ctypes.sizeof(lib.CPileupOutput) == 8 * 20 + 16
    assert ctypes.sizeof(lib.CPileupInput) == 56 and ctypes.sizeof(lib.CPileupStats) == 8 * 13

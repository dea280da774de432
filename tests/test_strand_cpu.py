"""Directional consensus, host side: the fixture's conditions re-derived with the CPU restatement,
the restatement's unit cases, the ABI mirrors and the record naming.  No GPU."""
import ctypes
import math
import os
import subprocess

import pytest

from oracle import oracle as O
from pbccs_amd import ccsio, lib
from tests import strand_common as C
from tests import strand_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INS, DEL, SUB = 0, 1, 2


# ---- the fixture ---------------------------------------------------------------------------------------------------
def test_fixture_is_what_the_generator_makes():
    fx = C.load_fixture()
    assert len(fx) >= 6 and len({z["seed"] for z in fx}) >= 3
    for z in fx:
        g = C.make_zmw(z["seed"], z["hetero"])
        for k in g:
            assert z[k] == g[k], (z["seed"], k)
        assert len(z["truth"]) == C.LENGTH and len(z["reads"]) == C.PASSES
        assert [r["strand"] for r in z["reads"]] == [0, 1] * (C.PASSES // 2)
        diff = [i for i in range(C.LENGTH) if z["truth"][i] != z["alt"][i]]
        assert diff == ([C.SITE] if z["hetero"] else [])
        if z["hetero"]:
            assert "ACGT".index(z["alt"][C.SITE]) == ("ACGT".index(z["truth"][C.SITE]) + 1) % 4
    # every heteroduplex ZMW is followed by the control of its seed: the same draft, the same forward reads
    for h, c in zip(fx[0::2], fx[1::2]):
        assert h["hetero"] and not c["hetero"] and h["seed"] == c["seed"] and h["draft"] == c["draft"]
        assert h["reads"][0::2] == c["reads"][0::2] and h["reads"][1::2] != c["reads"][1::2]


@pytest.mark.parametrize("idx", range(6))
def test_fixture_conditions_hold_on_the_cpu_restatement(idx):
    z = C.load_fixture()[idx]
    s, ref = C.oracle_polished(z)
    assert ref["converged"]                                                          # (a)
    assert s.template() == z["oracle_final"]
    strands = [r["strand"] for r in z["reads"]]
    sites, sums = C.oracle_sites(s, strands)
    assert [list(x) for x in sites] == z["oracle_sites"]                             # (b), as recorded
    if z["hetero"]:
        assert any(x[0] in (C.SITE, C.SITE + 1) for x in sites)
    else:
        assert sites == []
    for strand, want, key in ((0, z["truth"], "oracle_fwd_final"), (1, z["alt"], "oracle_rev_final")):   # (c)
        sub = C.single_strand(z, strand)
        e = O.polish_zmw(sub["draft"], sub["reads"], sub["snr"], qvs=False)
        assert e["converged"] and e["template"] == want == z[key]
    assert C.threshold_distance(sums) >= 1e-6                                         # (d)


# ---- the restatement's unit cases ----------------------------------------------------------------------------------
def test_sums_are_sequential_adds_in_read_order():
    per = [0.1, 1e16, 0.2, -1e16, 0.3, 0.4]
    got = R.strand_sums(per, [0, 1, 0, 1, 0, 1])
    assert got == ((0.1 + 0.2) + 0.3, (1e16 + -1e16) + 0.4, 3, 3)
    # order matters in floating point: the same reads in another order give another reverse sum
    assert R.strand_sums([1e16, 0.4, -1e16], [1, 1, 1])[1] != got[1]


def test_a_read_that_does_not_score_and_an_inactive_read_stay_out():
    per = [20.0, None, 20.0, -20.0, None, -20.0]   # read 1: outside the window, read 4: inactive
    assert R.strand_sums(per, [0, 0, 0, 1, 1, 1]) == (40.0, -40.0, 2, 2)
    assert R.qualifies((40.0, -40.0, 2, 2))
    assert not R.qualifies((40.0, -40.0, 2, 2), min_reads=3)


def test_min_reads_counts_each_strand():
    assert not R.qualifies((40.0, -40.0, 1, 5))
    assert not R.qualifies((40.0, -40.0, 5, 1))
    assert R.qualifies((40.0, -40.0, 1, 1), min_reads=1)
    assert R.qualifies((-40.0, 40.0, 2, 2))


def test_thresholds_are_strict_and_need_opposite_signs():
    assert not R.qualifies((12.5, -40.0, 3, 3)) and not R.qualifies((40.0, -12.5, 3, 3))
    assert R.qualifies((math.nextafter(12.5, 13), math.nextafter(-12.5, -13), 3, 3))
    assert not R.qualifies((40.0, 40.0, 3, 3)) and not R.qualifies((-40.0, -40.0, 3, 3))
    assert not R.qualifies((40.0, -1.0, 3, 3))


def test_a_nan_sum_never_qualifies():
    nan = float("nan")
    s = R.strand_sums([nan, 30.0, -30.0, -30.0], [0, 0, 1, 1])
    assert math.isnan(s[0]) and s[1:] == (-60.0, 2, 2)
    assert not R.qualifies(s) and not R.qualifies((40.0, nan, 2, 2)) and not R.qualifies((nan, nan, 2, 2))
    assert R.strand_sites([(SUB, 3, "A")], [s]) == []


def test_sites_report_the_largest_smaller_side_and_the_first_on_a_tie():
    muts = [(SUB, 4, "A"), (SUB, 4, "C"), (INS, 4, "G"), (DEL, 4, "-"), (SUB, 7, "T"), (SUB, 9, "A")]
    sums = [(30.0, -14.0, 2, 2),    # min 14
            (20.0, -20.0, 2, 2),    # min 20: the site's mutation
            (-20.0, 50.0, 2, 2),    # min 20 again: a tie, the first in enumeration order stays
            (90.0, -13.0, 2, 2),    # min 13
            (5.0, -40.0, 2, 2),     # does not qualify
            (-13.0, 13.0, 2, 2)]
    assert R.strand_sites(muts, sums) == [(4, SUB, "C", 20.0, -20.0), (9, SUB, "A", -13.0, 13.0)]
    assert R.strand_sites(muts, sums, min_score=25.0) == []
    assert R.strand_sites(muts, sums, min_score=13.5) == [(4, SUB, "C", 20.0, -20.0)]   # position 9 drops out
    assert R.strand_sites(muts[:1] + muts[2:], sums[:1] + sums[2:]) == [(4, INS, "G", -20.0, 50.0),
                                                                        (9, SUB, "A", -13.0, 13.0)]


# ---- the ABI ---------------------------------------------------------------------------------------------------------
def test_abi_structs_match_the_header(tmp_path):
    ofields = ["min_score", "min_reads", "min_sites", "directional"]
    rfields = ["n_sites", "cap", "position", "type", "base", "sum_fwd", "sum_rev", "split", "fwd", "rev"]
    xfields = ["repeats", "repeat_tested", "repeat_applied", "rich"]
    sfields = ["strand_screened", "strand_sites", "strand_split"]
    src = tmp_path / "sizes.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "pbccs_amd.h"\nint main(void) {\n'
                   'printf("%zu %zu %zu %zu", sizeof(pbccs_strand_options), sizeof(pbccs_strand_result), '
                   'sizeof(pbccs_polish_extras), sizeof(pbccs_strand_stats));\n' +
                   "".join(f'printf(" %zu", offsetof(pbccs_strand_options, {f}));\n' for f in ofields) +
                   "".join(f'printf(" %zu", offsetof(pbccs_strand_result, {f}));\n' for f in rfields) +
                   "".join(f'printf(" %zu", offsetof(pbccs_polish_extras, {f}));\n' for f in xfields) +
                   "".join(f'printf(" %zu", offsetof(pbccs_strand_stats, {f}));\n' for f in sfields) +
                   'printf(" %zu\\n", sizeof(pbccs_zmw_output));\nreturn 0; }\n')
    exe = str(tmp_path / "sizes")
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    want = [ctypes.sizeof(lib.CStrandOptions), ctypes.sizeof(lib.CStrandResult), ctypes.sizeof(lib.CPolishExtras),
            ctypes.sizeof(lib.CStrandStats)]
    want += [getattr(lib.CStrandOptions, f).offset for f in ofields]
    want += [getattr(lib.CStrandResult, f).offset for f in rfields]
    want += [getattr(lib.CPolishExtras, f).offset for f in xfields]
    want += [getattr(lib.CStrandStats, f).offset for f in sfields]
    want += [ctypes.sizeof(lib.CZmwOutput)]
    assert got == want
    assert [n for n, _ in lib.CStrandOptions._fields_] == ofields
    assert [n for n, _ in lib.CStrandResult._fields_] == rfields
    assert got[2] == 32 and got[-1] == 112   # the extras and the output record keep their layout


def test_library_exports_the_strand_calls_and_defaults():
    names = ("pbccs_strand_options_default", "pbccs_polish_batch_strand", "pbccs_ccs_batch_strand",
             "pbccs_scorer_strand_scores",
             "pbccs_scorer_strand_sites", "pbccs_strand_stats_get")
    hdr = open(os.path.join(ROOT, "include", "pbccs_amd.h")).read()
    L = lib.load()
    for name in names:
        assert name in lib.SIGNATURES and hasattr(L, name) and name in hdr, name
    o = lib.CStrandOptions(0.0, 0, 0, 7)
    L.pbccs_strand_options_default(ctypes.byref(o))
    assert (o.min_score, o.min_reads, o.min_sites, o.directional) == (12.5, 2, 1, 0)


def test_keywords_are_checked_before_any_device_work():
    import pbccs_amd
    from pbccs_amd import strand
    with pytest.raises(ValueError):
        strand.strand_options(True, "sometimes")
    with pytest.raises(ValueError):
        strand.strand_options({"min_scor": 3.0})
    o = strand.strand_options({"min_score": 9.0, "min_reads": 3, "min_sites": 2}, "discordant")
    assert (o.min_score, o.min_reads, o.min_sites, o.directional) == (9.0, 3, 2, 1)
    assert strand.strand_options(True, "always").directional == 2
    z = C.polish_inputs(C.load_fixture()[:1])
    with pytest.raises(ValueError):
        pbccs_amd.polish_windowed(z, strand_sites=True)
    with pytest.raises(ValueError):
        pbccs_amd.polish_windowed(z, directional="always")


def test_per_strand_record_names():
    res = {"status": "Success", "consensus": "ACGT", "qvs": [30, 40, 50, 60], "add_read_results": [0, -1, 0, -1],
           "zscores": [0.5, float("nan"), 1.0, float("nan")], "za": 0.4, "predicted_accuracy": 0.999, "n_passes": 2,
           "status_counts": [2, 0, 0, 0, 0]}
    snr = [10.0, 7.0, 5.0, 11.5]
    plain = ccsio.ccs_sam_record("m1", 7, res, snr)
    assert plain.split("\t")[0] == "m1/7/ccs" and plain == ccsio.ccs_sam_record("m1", 7, res, snr, strand=None)
    for strand in ("fwd", "rev"):
        line = ccsio.ccs_sam_record("m1", 7, res, snr, strand=strand)
        assert line.split("\t")[0] == f"m1/7/ccs/{strand}" and line.split("\t")[1:] == plain.split("\t")[1:]
        assert ccsio.ccs_fastq_record("m1", 7, res, strand=strand) == f"@m1/7/ccs/{strand}\nACGT\n+\n?IS]\n"
    assert ccsio.ccs_fastq_record("m1", 7, res) == "@m1/7/ccs\nACGT\n+\n?IS]\n"
    with pytest.raises(ValueError):
        ccsio.ccs_sam_record("m1", 7, res, snr, strand="both")


def test_settings_carry_the_reference_field():
    from pbccs_amd import ConsensusSettings
    from pbccs_amd import polish
    assert ConsensusSettings().directional is None
    assert polish._strand_keywords(False, None, ConsensusSettings()) is None
    assert polish._strand_keywords(False, None, ConsensusSettings(directional="always")).directional == 2
    assert polish._strand_keywords(False, "discordant", ConsensusSettings(directional="always")).directional == 1
    assert polish._strand_keywords(True, None, None).directional == 0

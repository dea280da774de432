"""Per-base rich consensus QVs, host side: the ABI mirrors, the Python reference computation on a
hand-worked example, the SAM / BAM tags and the feature-track helper.  No GPU."""
import ctypes
import math
import os
import subprocess

import pytest

from pbccs_amd import bamio, ccsio, lib, richqv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMPTY = 3077   # round(-10 log10(DBL_MIN)): what an empty sum gives in ConsensusQVs


def test_abi_structs_match_the_header(tmp_path):
    src = tmp_path / "sizes.c"
    fields = ["sub_qv", "ins_qv", "del_qv", "sub_tag", "ins_tag", "cap", "len"]
    xfields = ["repeats", "repeat_tested", "repeat_applied", "rich"]
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "pbccs_amd.h"\nint main(void) {\n'
                   'printf("%zu %zu", sizeof(pbccs_rich_qvs), sizeof(pbccs_polish_extras));\n' +
                   "".join(f'printf(" %zu", offsetof(pbccs_rich_qvs, {f}));\n' for f in fields) +
                   "".join(f'printf(" %zu", offsetof(pbccs_polish_extras, {f}));\n' for f in xfields) +
                   'printf(" %zu %zu\\n", sizeof(pbccs_zmw_output), sizeof(pbccs_quiver_result));\nreturn 0; }\n')
    exe = str(tmp_path / "sizes")
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    want = [ctypes.sizeof(lib.CRichQvs), ctypes.sizeof(lib.CPolishExtras)]
    want += [getattr(lib.CRichQvs, f).offset for f in fields]
    want += [getattr(lib.CPolishExtras, f).offset for f in xfields]
    want += [ctypes.sizeof(lib.CZmwOutput), ctypes.sizeof(lib.CQuiverResult)]   # no existing struct changed layout
    assert got == want
    assert got[:2] == [48, 32] and got[-2:] == [112, 56]
    assert [n for n, _ in lib.CRichQvs._fields_] == fields
    for name in ("pbccs_consensus_qvs_rich", "pbccs_quiver_consensus_qvs_rich", "pbccs_polish_windowed_ex"):
        assert name in lib.SIGNATURES
    for name in ("pbccs_polish_batch_ex2", "pbccs_quiver_polish_batch_ex2", "pbccs_ccs_batch_ex4"):
        assert name in lib.DIGIT_SIGNATURES
    hdr = open(os.path.join(ROOT, "include", "pbccs_amd.h")).read()
    for name in list(lib.DIGIT_SIGNATURES) + ["pbccs_rich_qvs", "pbccs_polish_extras"]:
        assert name in hdr, name


def test_library_exports_the_rich_calls():
    L = lib.load()
    for name in ("pbccs_consensus_qvs_rich", "pbccs_quiver_consensus_qvs_rich", "pbccs_polish_batch_ex2",
                 "pbccs_quiver_polish_batch_ex2", "pbccs_polish_windowed_ex", "pbccs_ccs_batch_ex4"):
        assert hasattr(L, name), name


def test_enumeration_order():
    tpl = "ACCGTTAG"
    assert richqv.unique_mutations(tpl, 0) == [(2, "C"), (2, "G"), (2, "T"), (0, "A"), (0, "C"), (0, "G"), (0, "T"),
                                               (1, "-")]
    assert richqv.unique_mutations(tpl, 2) == [(2, "A"), (2, "G"), (2, "T"), (0, "A"), (0, "G"), (0, "T")]
    assert richqv.unique_mutations(tpl, 3) == [(2, "A"), (2, "C"), (2, "T"), (0, "A"), (0, "G"), (0, "T"), (1, "-")]


def test_reference_on_a_hand_worked_example():
    """ACCGTTAG with every substitution at ln(1/27), every insertion at ln(1/297), every deletion at ln(1/999), so
    that S_sub = 3/27 = 1/9 (prob 1/10, QV 10), S_ins = 3/297 = 1/99 (prob 1/100, QV 20) and S_del = 1/999 (prob
    1/1000, QV 30).  Exceptions:
      position 0 has four insertions: S_ins = 4/297, prob 4/301, -10 log10 = 18.77 -> 19;
      positions 2 and 5 repeat the base before them: no deletion, the empty sum's 3077;
      position 3: the substitution to T scores +0.5 -- out of the sum, S_sub = 2/27, prob 2/29, 11.61 -> 12 -- yet it
        is the best substitution, so sub_tag is T;
      position 5: the insertion of G scores -1: S_ins = 2/297 + e^-1 = 0.374614, prob 0.272523, 5.65 -> 6, ins_tag G.
    Everywhere else the scores of a type tie and the first in enumeration order gives the tag.
    Overall: S = 1/9 + 1/99 + 1/999 = 0.122213, prob 0.108904, 9.63 -> 10; position 0: 0.125580, 0.111569, 9.52 -> 10;
    position 2: 0.121212, 0.108108, 9.66 -> 10; position 3: 2/27 + 1/99 + 1/999 = 0.085176, 0.078491, 11.05 -> 11;
    position 5: 1/9 + 0.374614 = 0.485725, 0.326928, 4.86 -> 5."""
    tpl = "ACCGTTAG"
    base = {2: math.log(1 / 27), 0: math.log(1 / 297), 1: math.log(1 / 999)}

    def score(p, t, b):
        if (p, t, b) == (3, 2, "T"):
            return 0.5
        if (p, t, b) == (5, 0, "G"):
            return -1.0
        return base[t]
    got = richqv.reference_rich_qvs(tpl, score)
    assert got == {
        "qvs": [10, 10, 10, 11, 10, 5, 10, 10],
        "sub_qv": [10, 10, 10, 12, 10, 10, 10, 10],
        "ins_qv": [19, 20, 20, 20, 20, 6, 20, 20],
        "del_qv": [30, 30, EMPTY, 30, 30, EMPTY, 30, 30],
        "sub_tag": "CAATAACA",
        "ins_tag": "ACAAAGAC",
    }
    assert richqv.sum_to_qv(0.0) == EMPTY
    assert richqv.probability_to_qv(10 ** -0.25) == 3 and richqv.probability_to_qv(10 ** -0.24) == 2   # halves go up


def _result():
    n = 13
    return {"status": "Success", "consensus": "ACGTTGCANACGT", "qvs": [30, 40, 93, 12, 0, 5, 60, 61, 62, 63, 70, 80, 90],
            "add_read_results": [0, 0, 3, 0], "zscores": [0.5, -1.25, float("nan"), 2.0], "za": 0.41666,
            "predicted_accuracy": 0.9987654, "n_passes": 3, "status_counts": [3, 0, 0, 1, 0],
            "sub_qv": [93, 94, 120] + [50] * (n - 3), "ins_qv": list(range(20, 20 + n)),
            "del_qv": [EMPTY, 31, EMPTY] + [45] * (n - 3), "sub_tag": "CAGACATGCTGAC", "ins_tag": "ACGTACGTACGTA"}


def test_sam_line_and_bam_round_trip(tmp_path):
    res = _result()
    snr = [10.0, 7.0, 5.0, 11.5]
    plain = ccsio.ccs_sam_record("m140905_42", 6251, res, snr)
    bare = {k: v for k, v in res.items() if k not in richqv.RICH_KEYS}
    assert plain == ccsio.ccs_sam_record("m140905_42", 6251, bare, snr)   # today's line, byte for byte
    assert plain.split("\t")[11:][-1].startswith("rs:B:i,") and "dq:Z:" not in plain
    rich = ccsio.ccs_sam_record("m140905_42", 6251, res, snr, rich=True)
    assert rich.startswith(plain + "\t")
    tags = rich[len(plain) + 1:].split("\t")
    assert [t[:5] for t in tags] == ["dq:Z:", "iq:Z:", "sq:Z:", "dt:Z:", "st:Z:"]
    # inverse naming: dq / dt are the insertion mutation's, iq the deletion's
    assert tags[0][5:] == "".join(chr(q + 33) for q in res["ins_qv"])
    assert tags[1][5:] == "~@~" + "N" * 10            # 3077 clips to 93 ('~'), 31 is '@', 45 is 'N'
    assert tags[2][5:] == "~~~" + "S" * 10            # 93, 94 and 120 all clip to 93
    assert tags[3][5:] == res["ins_tag"] and tags[4][5:] == res["sub_tag"]
    rec = bamio.sam_to_bam_record(rich, bin_=0)
    assert bamio.bam_record_to_sam(rec[4:]) == rich
    p = tmp_path / "ccs.bam"
    bamio.write_ccs_bam(str(p), ["m140905_42"], [rich, plain])
    _, lines = bamio.read_bam(str(p))
    assert lines == [rich, plain]


def test_feature_tracks_helper():
    res = _result()
    f = richqv.rich_feature_tracks(res, merge_qv=7)
    n = len(res["consensus"])
    assert f.Sequence == res["consensus"] and f.Length() == n
    assert f.InsQv == [93.0, 31.0, 93.0] + [45.0] * (n - 3)          # "this base is spurious": del_qv, clipped
    assert f.SubsQv == [93.0, 93.0, 93.0] + [50.0] * (n - 3)
    assert f.DelQv == [float(q) for q in res["ins_qv"]]              # "a base is missing before this one": ins_qv
    assert f.DelTag == [float(ord(c)) for c in res["ins_tag"]]
    assert f.MergeQv == [7.0] * n
    g = richqv.rich_feature_tracks({k: res[k] for k in richqv.RICH_KEYS}, consensus=res["consensus"])
    assert g.MergeQv == [0.0] * n and g.DelQv == f.DelQv
    with pytest.raises(ValueError):
        richqv.rich_feature_tracks(dict(res, sub_tag="AC"))

"""Arrow mutations of any width, the parts that need no GPU: the slipped-repeat fixture's claims re-derived from the
CPU restatement, the single-base gap g1 behind the GPU test's tolerance, the host-only 8-column rule and the ABI
structs of the new entry points."""
import ctypes
import os
import subprocess

import pytest

from pbccs_amd import Mutation, lib, wide_columns_needed
from tests import arrow_multibase_common as C
from tests.arrow_multibase_common import DEL, INS, SUB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G1 = 4.294581756880689e-08            # tests/test_arrow_multibase_gpu.py
EXCLUDED_CLASSES = {(INS, 0, 3)}


@pytest.mark.parametrize("k", range(4))
def test_fixture_claims_hold_on_the_cpu_restatement(k):
    """Each committed ZMW is what the generator gives for its seed; the CPU restatement's RefineConsensus converges
    on a template that is not the truth; one repeat candidate of that template gives the truth, whose refill
    likelihood summed over the reads is better by more than 0.04."""
    z = C.load_slips()[k]
    made = C.slip_zmw(z["seed"], z["unit_len"])
    assert (made["truth"], made["draft"], made["reads"]) == (z["truth"], z["draft"], z["reads"])
    assert 60 <= len(z["truth"]) <= 84 and len(z["reads"]) == 6
    assert abs(len(z["draft"]) - len(z["truth"])) == z["unit_len"]
    rec = C.qualify(made, z["unit_len"])
    assert rec is not None
    assert rec["oracle_final"] == z["oracle_final"] != z["truth"]
    assert (rec["oracle_n_tested"], rec["oracle_n_applied"]) == (z["oracle_n_tested"], z["oracle_n_applied"])
    assert rec["margin"] == pytest.approx(z["margin"], abs=1e-9) and rec["margin"] > 0.04
    # no single-base mutation of the stalled template is favourable: that is the stall
    s = C.oracle_on(z["oracle_final"], [dict(r, te=len(z["oracle_final"])) for r in z["reads"]])
    assert max(s.score(t, p, b, -12.5) for t, p, b in C.O.unique_mutations(z["oracle_final"])) <= 0.04


def test_fixture_has_both_repeat_lengths():
    assert sorted(z["unit_len"] for z in C.load_slips()) == [2, 2, 2, 3]


def test_g1_measurement_reproduces_the_constant():
    """Over every unique single-base mutation of the two 74-base ZMWs, per class of (type, distance to either
    template end): |ScoreMutation - refill| stays below 1e-6 everywhere but for insertions at position 0, and its
    largest value there is the constant the GPU test multiplies by 100."""
    g1 = 0.0
    for z in C.score_zmws():
        assert len(z["tpl"]) == 74
        per_class = C.g1_measure(z)
        assert {c for c, v in per_class.items() if v > 1e-6} == EXCLUDED_CLASSES
        assert all(v > 1.0 for c, v in per_class.items() if c in EXCLUDED_CLASSES)
        g1 = max(g1, max(v for c, v in per_class.items() if c not in EXCLUDED_CLASSES))
    assert g1 == pytest.approx(G1, rel=1e-6)


def cols(m, strand, ts, te):
    return wide_columns_needed(m, strand, ts, te)


def test_column_rule_accepts_and_rejects():
    """1 + |bases| columns in the middle of a window (2 for a deletion); to the window's end (ExtendAlpha) or
    start (ExtendBeta) in the edge cases; on the reverse strand the window is mirrored; a read the mutation
    misses needs none."""
    # middle of the window [0, 64)
    assert cols(Mutation(INS, 30, "A"), 0, 0, 64) == 2
    assert cols(Mutation(INS, 30, "ACGTACG"), 0, 0, 64) == 8
    assert cols(Mutation(SUB, 30, "ACGT"), 0, 0, 64) == 5
    assert cols(Mutation(DEL, 30, "-", end=36), 0, 0, 64) == 2
    # at the beginning: oe + ld + 1
    assert cols(Mutation(INS, 2, "AC"), 0, 0, 64) == 5
    assert cols(Mutation(INS, 1, "ACGTACG"), 0, 0, 64) == 9        # refused
    assert cols(Mutation(SUB, 1, "ACG"), 0, 0, 64) == 5
    assert cols(Mutation(DEL, 2, "-", end=5), 0, 0, 64) == 3
    # at the end: Jv - (os - 1) + 1
    assert cols(Mutation(SUB, 60, "ACGT"), 0, 0, 64) == 6
    assert cols(Mutation(INS, 62, "ACG"), 0, 0, 64) == 4           # end == J - 2 is still the middle
    assert cols(Mutation(INS, 63, "ACG"), 0, 0, 64) == 6
    assert cols(Mutation(INS, 63, "ACGTACG"), 0, 0, 64) == 10      # refused
    assert cols(Mutation(DEL, 59, "-", end=63), 0, 0, 64) == 3
    # the reverse strand mirrors the window: the template's end is the read's beginning
    assert cols(Mutation(INS, 62, "ACG"), 1, 0, 64) == cols(Mutation(INS, 2, "ACG"), 0, 0, 64) == 6
    assert cols(Mutation(SUB, 1, "ACG"), 1, 0, 64) == cols(Mutation(SUB, 60, "ACG"), 0, 0, 64)
    # a partial window [5, 58): coordinates are the window's, overhangs are clipped to it
    assert cols(Mutation(INS, 7, "AC"), 0, 5, 58) == 5
    assert cols(Mutation(SUB, 3, "ACGT"), 0, 5, 58) == cols(Mutation(SUB, 5, "GT"), 0, 5, 58) == 3
    assert cols(Mutation(DEL, 56, "-", end=62), 0, 5, 58) == cols(Mutation(DEL, 56, "-", end=58), 0, 5, 58)
    # reads the mutation misses
    assert cols(Mutation(SUB, 60, "AC"), 0, 5, 58) == -1
    assert cols(Mutation(INS, 59, "AC"), 0, 5, 58) == -1
    assert cols(Mutation(INS, 58, "AC"), 0, 5, 58) > 0            # an insertion at the window's end is scored
    # tiny windows take the whole refill (no extension buffer); an emptied window is refused
    assert cols(Mutation(SUB, 1, "AC"), 0, 0, 4) == 0
    assert cols(Mutation(DEL, 0, "-", end=4), 0, 0, 4) == -2
    # invalid mutations
    for bad in (Mutation(INS, 30, "ACGTACGT"), Mutation(SUB, 30, "AN"), Mutation(SUB, 30, "AC", end=35)):
        with pytest.raises(lib.PbccsError):
            cols(bad, 0, 0, 64)


def test_abi_struct_sizes_match_the_header(tmp_path):
    """pbccs_counters gained a field at its end and the new calls take pbccs_mutation_ex / pbccs_repeat_options:
    the ctypes mirrors in pbccs_amd/lib.py have the header's sizes and the new field's offset."""
    src = tmp_path / "sizes.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "pbccs_amd.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(pbccs_counters), '
                   'offsetof(pbccs_counters, repeat_skipped_ckpt), sizeof(pbccs_mutation_ex), '
                   'sizeof(pbccs_repeat_options), sizeof(pbccs_zmw_input), sizeof(pbccs_zmw_output)); return 0; }\n')
    exe = str(tmp_path / "sizes")
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [ctypes.sizeof(lib.CCounters), lib.CCounters.repeat_skipped_ckpt.offset,
                   ctypes.sizeof(lib.CMutationEx), ctypes.sizeof(lib.CRepeatOptions), ctypes.sizeof(lib.CZmwInput),
                   ctypes.sizeof(lib.CZmwOutput)]
    for name in ("pbccs_scorer_score_many_ex", "pbccs_scorer_scores_ex", "pbccs_scorer_is_favorable_ex",
                 "pbccs_scorer_apply_mutations_ex", "pbccs_refine_repeats", "pbccs_polish_batch_ex",
                 "pbccs_wide_columns_needed"):
        assert name in lib.SIGNATURES and hasattr(lib.load(), name)

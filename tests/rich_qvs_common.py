"""Shared inputs of the rich-QV tests: the single-scorer Arrow fixture, the oracle-side reference
computation, and the comparison rules.  Not a test module."""
import math

from pbccs_amd import richqv

SNR = (10.0, 7.0, 5.0, 11.0)
# 56 bases: a homopolymer (TTTT at 3..6), a dinucleotide repeat (ACACACA at 8..14), first base A, last base G
TPL = "ACGTTTTGACACACAGTCCATGGATTACGCTAGCTAAGGCTTACGATCGGATCCAG"
HOMOPOLYMER = (3, 7)   # [begin, end) of the T run


def revcomp(s):
    return s[::-1].translate(str.maketrans("ACGT", "TGCA"))


def arrow_reads():
    """Five reads on both strands: a deletion, a substitution (reverse), a partial window with an insertion, a read
    three bases longer than the template (reverse), and an exact pass."""
    t = TPL
    longer = t[:20] + "G" + t[20:33] + "T" + t[33:47] + "A" + t[47:]
    assert len(longer) == len(t) + 3
    return [
        {"seq": t[:30] + t[31:], "strand": 0, "ts": 0, "te": len(t)},
        {"seq": revcomp(t[:17] + "A" + t[18:]), "strand": 1, "ts": 0, "te": len(t)},
        {"seq": t[8:25] + "C" + t[25:44], "strand": 0, "ts": 8, "te": 44},
        {"seq": revcomp(longer), "strand": 1, "ts": 0, "te": len(t)},
        {"seq": t, "strand": 0, "ts": 0, "te": len(t)},
    ]


def oracle_rich(tpl, score):
    """The definition over an oracle scorer: score(type, start, base) -> the full sum of one mutation.  Returns
    (reference dict, per position {type: sorted scores}) -- the second for the near-tie rule of the tags."""
    by_pos = []

    def at(p, t, b):
        s = score(t, p, b)
        by_pos[p].setdefault(t, []).append(s)
        return s
    for _ in tpl:
        by_pos.append({})
    ref = richqv.reference_rich_qvs(tpl, at)
    return ref, by_pos


def near_tie(scores, eps=1e-6):
    """The two best scores of one type lie within eps of each other (the tag is then not compared)."""
    s = sorted(scores, reverse=True)
    return len(s) > 1 and s[0] - s[1] <= eps


def empty_sum_qv():
    """What a type with nothing below 0 gets: ProbabilityToQV(0) = round(-10 log10(DBL_MIN))."""
    return richqv.sum_to_qv(0.0)


def assert_typed_close(got, ref, keys=("sub_qv", "ins_qv", "del_qv"), tol=1):
    """Typed QVs within `tol` of the reference (the project's QV tolerance); exactly equal where the
    reference's partial sum is empty."""
    for k in keys:
        assert len(got[k]) == len(ref[k]), k
        for p, (a, b) in enumerate(zip(got[k], ref[k])):
            if b == empty_sum_qv():
                assert a == b, (k, p, a, b)
            else:
                assert abs(a - b) <= tol, (k, p, a, b)


def tag_mismatches(got, ref, by_pos):
    """(positions compared and differing, positions skipped for a near-tie) over both tags."""
    bad, skipped = [], set()
    for key, t in (("sub_tag", 2), ("ins_tag", 0)):
        for p in range(len(ref[key])):
            if near_tie(by_pos[p].get(t, [])):
                skipped.add(p)
            elif got[key][p] != ref[key][p]:
                bad.append((key, p, got[key][p], ref[key][p]))
    return bad, skipped


assert math.isfinite(empty_sum_qv())

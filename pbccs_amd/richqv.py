"""Per-base rich consensus QVs: ConsensusQVs' sum of a position taken apart by mutation type.

For position p of the final template, over the mutations UniqueSingleBaseMutationEnumerator lists there (the
substitutions to the other three bases, the insertions of every base but tpl[p-1], the deletion when
tpl[p] != tpl[p-1]) with their full scores s(m):

  sub_qv / ins_qv / del_qv = ProbabilityToQV(1 - 1 / (1 + S)), S = the sum of e^s(m) over the substitutions /
      insertions / deletion with s(m) < 0, in enumeration order (raw and unclipped; an empty sum gives the value it
      gives in ConsensusQVs);
  sub_tag / ins_tag = the base of the substitution / insertion with the largest s(m) (scores >= 0 count, the first
      in enumeration order wins a tie; 'N' only when none was enumerated).

Names follow the mutation type.  File formats name by error type, the inverse: PacBio's DeletionQV / DeletionTag
(dq / dt, "a base is missing before this one") are ins_qv / ins_tag, InsertionQV (iq, "this base is spurious") is
del_qv, and sq / st are sub_qv / sub_tag.
"""
import ctypes
import math

from . import lib as L

RICH_KEYS = ("sub_qv", "ins_qv", "del_qv", "sub_tag", "ins_tag")
DBL_MIN = 2.2250738585072014e-308
_BASES = "ACGT"


def unique_mutations(tpl, p):
    """UniqueSingleBaseMutationEnumerator(tpl).Mutations(p, p + 1) (MutationEnumerator.cpp:120-145) as
    (type, base) pairs in its order; type 0 insertion, 1 deletion, 2 substitution; the deletion's base is '-'."""
    prev = tpl[p - 1] if p > 0 else "-"
    out = [(2, b) for b in _BASES if b != tpl[p]]
    out += [(0, b) for b in _BASES if b != prev]
    if tpl[p] != prev:
        out.append((1, "-"))
    return out


def probability_to_qv(prob):
    """ProbabilityToQV (Consensus-inl.hpp:130-138)."""
    if prob == 0.0:
        prob = DBL_MIN
    v = -10.0 * math.log10(prob)   # >= 0: std::round rounds its halves up
    f = math.floor(v)
    return int(f) + (1 if v - f >= 0.5 else 0)


def sum_to_qv(s):
    return probability_to_qv(1.0 - 1.0 / (1.0 + s))


def reference_rich_qvs(tpl, score):
    """The definition above, computed in Python: score(p, type, base) -> s(m).  Returns the dict ConsensusRichQVs
    returns, "qvs" included (ConsensusQVs' own sum, over all of the position's mutations in enumeration order)."""
    out = {"qvs": [], "sub_qv": [], "ins_qv": [], "del_qv": [], "sub_tag": "", "ins_tag": ""}
    for p in range(len(tpl)):
        total = 0.0
        part = {0: 0.0, 1: 0.0, 2: 0.0}
        best = {0: None, 2: None}
        for t, b in unique_mutations(tpl, p):
            s = score(p, t, b)
            if s < 0.0:
                e = math.exp(s)
                total += e
                part[t] += e
            if t != 1 and (best[t] is None or s > best[t][0]):
                best[t] = (s, b)
        out["qvs"].append(sum_to_qv(total))
        out["sub_qv"].append(sum_to_qv(part[2]))
        out["ins_qv"].append(sum_to_qv(part[0]))
        out["del_qv"].append(sum_to_qv(part[1]))
        out["sub_tag"] += best[2][1] if best[2] else "N"
        out["ins_tag"] += best[0][1] if best[0] else "N"
    return out


class RichBuffers:
    """A pbccs_rich_qvs array for n ZMWs and the buffers it points at (caps[i] entries for ZMW i)."""

    def __init__(self, caps):
        n = len(caps)
        self.arr = (L.CRichQvs * max(1, n))()
        self._keep = []
        for i, cap in enumerate(caps):
            cap = max(1, int(cap))
            qv = [(ctypes.c_int * cap)() for _ in range(3)]
            tag = [ctypes.create_string_buffer(cap) for _ in range(2)]
            self._keep.append((qv, tag))
            r = self.arr[i]
            r.sub_qv, r.ins_qv, r.del_qv = qv
            r.sub_tag = ctypes.cast(tag[0], ctypes.POINTER(ctypes.c_char))
            r.ins_tag = ctypes.cast(tag[1], ctypes.POINTER(ctypes.c_char))
            r.cap = cap
            r.len = 0

    def record(self, i):
        """The five rich keys of ZMW i (empty where nothing was written)."""
        qv, tag = self._keep[i]
        n = self.arr[i].len
        if n < 0:
            raise L.PbccsError(-5, "rich QVs outgrew their buffers")
        return {"sub_qv": list(qv[0][:n]), "ins_qv": list(qv[1][:n]), "del_qv": list(qv[2][:n]),
                "sub_tag": tag[0].raw[:n].decode(), "ins_tag": tag[1].raw[:n].decode()}

    def extras(self, repeats=None, tested=None, applied=None):
        x = L.CPolishExtras()
        if repeats is not None:
            x.repeats = ctypes.pointer(repeats)
            x.repeat_tested = tested
            x.repeat_applied = applied
        x.rich = self.arr
        self._extras = (x, repeats)
        return x


def ConsensusRichQVs(mms):
    """ConsensusQVs with the per-base rich QVs beside it: {"qvs", "sub_qv", "ins_qv", "del_qv", "sub_tag",
    "ins_tag"} for an Arrow or a Quiver scorer (pbccs_consensus_qvs_rich / pbccs_quiver_consensus_qvs_rich: the same
    sweep as ConsensusQVs, then k_qv_rich / k_qqv_rich).  "qvs" is ConsensusQVs(mms), bit for bit.  Naming is by
    mutation type; see the module docstring for the file formats' inverse naming."""
    from . import quiver
    cap = mms.TemplateLength()
    rb = RichBuffers([cap])
    out = (ctypes.c_int * max(1, cap))()
    n = ctypes.c_int()
    fn = (L.load().pbccs_quiver_consensus_qvs_rich if isinstance(mms, quiver.QuiverMultiReadMutationScorer)
          else L.load().pbccs_consensus_qvs_rich)
    L.check(fn(mms._h, out, rb.arr, ctypes.byref(n)))
    res = {"qvs": list(out[: n.value])}
    res.update(rb.record(0))
    return res


def rich_feature_tracks(record, merge_qv=0.0, consensus=None):
    """The five QvSequenceFeatures tracks of a rich record (a polish record made with rich_qvs=True, or
    ConsensusRichQVs' dict with `consensus` given): InsQv = del_qv (this base is spurious), SubsQv = sub_qv,
    DelQv / DelTag = ins_qv / ins_tag (a base is missing before this one), MergeQv = the constant passed.  The QVs
    are clipped to [0, 93] as QVsToASCII clips them."""
    from .quiver import QvSequenceFeatures
    seq = record["consensus"] if consensus is None else consensus
    n = len(seq)
    for k in RICH_KEYS:
        if len(record[k]) != n:
            raise ValueError(f"rich track {k} has {len(record[k])} entries for {n} bases")

    def clip(v):
        return [float(min(max(0, q), 93)) for q in v]
    return QvSequenceFeatures(seq, ins_qv=clip(record["del_qv"]), subs_qv=clip(record["sub_qv"]),
                              del_qv=clip(record["ins_qv"]), del_tag=list(record["ins_tag"]),
                              merge_qv=[float(merge_qv)] * n)

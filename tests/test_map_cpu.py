"""MapToDraft's rules, restated in plain Python and pinned against the oracle (no GPU): what
SparsePoa::OrientAndAddRead + FindConsensus report for a read on a graph that holds only the draft, i.e.
oracle.sparse_poa([draft, draft, read], min_coverage=2)'s third summary.  Then the driver's host path
(driver.zmw_input(..., mapper=)) over an oracle-backed POA.

tests/test_map_gpu.py imports the restatement and the case builders from here."""
import random

import pytest

from pbccs_amd import driver

MATCH, MISMATCH, INSERT, DELETE = 3, -5, -4, -4   # DefaultPoaConfig(LOCAL)
_COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}


def revcomp(s):
    return "".join(_COMP[c] for c in reversed(s))


def local_extents(draft, read):
    """(score, (i0, i1), (j0, j1)).  Column j has consumed j draft bases, row i has consumed i read bases; column 0
    and row 0 are Start cells of score 0.  Candidates Start, diagonal, Delete (left), Extra (up), a later one only
    when strictly greater; every cell carries the Start cell its path left from.  End cell: columns in order, the
    column's first maximal row, a later column only when strictly greater."""
    n_i = len(read)
    prev_s = [0] * (n_i + 1)
    prev_o = [(i, 0) for i in range(n_i + 1)]
    best, end, origin = 0, (0, 0), (0, 0)
    for j in range(1, len(draft) + 1):
        cur_s, cur_o = [0] * (n_i + 1), [(0, j)] * (n_i + 1)
        b = draft[j - 1]
        for i in range(1, n_i + 1):
            s, o = 0, (i, j)
            c = prev_s[i - 1] + (MATCH if read[i - 1] == b else MISMATCH)
            if c > s:
                s, o = c, prev_o[i - 1]
            c = prev_s[i] + DELETE
            if c > s:
                s, o = c, prev_o[i]
            c = cur_s[i - 1] + INSERT
            if c > s:
                s, o = c, cur_o[i - 1]
            cur_s[i], cur_o[i] = s, o
        m = max(cur_s)
        if m > best:
            i = cur_s.index(m)
            best, end, origin = m, (i, j), cur_o[i]
        prev_s, prev_o = cur_s, cur_o
    if best == 0:
        return 0, (0, 0), (0, 0)
    return best, (origin[0], end[0]), (origin[1], end[1])


def map_restated(draft, reads, min_score_to_add=0.0):
    """mapping.map_to_draft's contract: per read None (not mapped) or {"rc", "read", "tpl", "score"}."""
    out = []
    for r in reads:
        if not r:
            out.append(None)
            continue
        fwd, rev = local_extents(draft, r), local_extents(draft, revcomp(r))
        if fwd[0] >= rev[0] and fwd[0] >= min_score_to_add:
            rc, a = False, fwd
        elif rev[0] >= fwd[0] and rev[0] >= min_score_to_add:
            rc, a = True, rev
        else:
            out.append(None)
            continue
        out.append({"rc": rc, "read": a[1], "tpl": a[2], "score": a[0]})
    return out


def summary_of(m):
    return None if m is None else {"rc": m["rc"], "read": tuple(m["read"]), "tpl": tuple(m["tpl"])}


def oracle_map(draft, read):
    """The yardstick: (consensus, summary of the read) of a SparsePoa that holds the draft twice, then the read."""
    from oracle import oracle as O
    r = O.sparse_poa([draft, draft, read], min_coverage=2)
    assert r["keys"][2] == 2, r["keys"]
    return r["consensus"], r["summaries"][2]


def noisy(rng, s, ins=0.10, dele=0.06, sub=0.03, alphabet="ACGT"):
    out = []
    for c in s:
        while rng.random() < ins:
            out.append(rng.choice(alphabet))
        x = rng.random()
        if x < dele:
            continue
        out.append(rng.choice([a for a in alphabet if a != c]) if x < dele + sub and len(alphabet) > 1 else c)
    return "".join(out) or s[:1]


def seeded_cases(n=120, seed=20240, lo=30, hi=160):
    """(draft, read): a noisy copy of a window of the draft with random flanks, on either strand.  Every second case
    is tie-heavy: a homopolymer or dinucleotide draft, or a two-letter alphabet."""
    rng = random.Random(seed)
    cases = []
    for k in range(n):
        length = rng.randint(lo, hi)
        alphabet = "ACGT"
        if k % 2 == 0:
            draft = "".join(rng.choice("ACGT") for _ in range(length))
        elif k % 6 == 1:
            draft = rng.choice("ACGT") * length
        elif k % 6 == 3:
            a, b = rng.sample("ACGT", 2)
            draft = (a + b) * (length // 2 + 1)
            draft = draft[:length]
        else:
            alphabet = "".join(rng.sample("ACGT", 2))
            draft = "".join(rng.choice(alphabet) for _ in range(length))
        b = rng.randint(0, length // 3)
        e = rng.randint(max(b + 1, 2 * length // 3), length)
        read = noisy(rng, draft[b:e], alphabet=alphabet)
        read = ("".join(rng.choice("ACGT") for _ in range(rng.randint(0, 12))) + read +
                "".join(rng.choice("ACGT") for _ in range(rng.randint(0, 12))))
        if rng.random() < 0.5:
            read = revcomp(read)
        cases.append((draft, read))
    return cases


def edge_cases():
    rng = random.Random(7)
    d = "".join(rng.choice("ACGT") for _ in range(90))
    half = "".join(rng.choice("ACGT") for _ in range(40))
    return [
        ("AAAAAAAAAAAAAAAAAAAAAAAAAAAAAA", "CCCCCCCCCCCC"),      # no matching base on either strand: A/T vs C/G
        (d, d[37]),                                             # a 1-base read
        (d, d),                                                 # read == draft
        (half + revcomp(half), half[10:] + revcomp(half)[:25]),  # a draft that is its own reverse complement
        (d, revcomp(d)),                                        # read == rc(draft)
        ("ACGTTGCA" + "G" * 60 + "TGACCATG", "G" * 25),          # a read inside a homopolymer
        (d, "TTTTTTTTTT" + d[20:70] + "CACACACACA"),            # unaligned flanks
    ]


_CASES = seeded_cases() + edge_cases()


def test_restatement_equals_the_oracle_on_every_case():
    dropped = 0
    for draft, read in _CASES:
        css, exp = oracle_map(draft, read)
        if css != draft:
            dropped += 1
            continue
        got = summary_of(map_restated(draft, [read])[0])
        assert got == exp, (draft, read, got, exp)
    assert dropped == 0   # the set drops none: a drop is a failure


def test_no_matching_base_is_mapped_with_empty_extents():
    draft, read = edge_cases()[0]
    assert map_restated(draft, [read]) == [{"rc": False, "read": (0, 0), "tpl": (0, 0), "score": 0}]
    assert map_restated(draft, [read, "", None], min_score_to_add=1.0) == [None, None, None]


class OraclePoa:
    """The SparsePoa surface driver.poa_inputs takes, over oracle.sparse_poa."""

    def __init__(self):
        self.reads = []

    def orient_and_add_read(self, seq):
        from oracle import oracle as O
        key = O.sparse_poa(self.reads + [seq])["keys"][-1]
        if key >= 0:
            self.reads.append(seq)
        return key

    def find_consensus(self, min_coverage):
        from oracle import oracle as O
        r = O.sparse_poa(self.reads, min_coverage=min_coverage)
        return r["consensus"], dict(enumerate(r["summaries"]))


def host_chunk(seed=5, length=120, passes=7):
    """One ZMW as raw subreads: noisy passes on alternating strands, the last one partial, plus one read of twice
    the median length (FilterReads drops it: None, last)."""
    rng = random.Random(seed)
    tpl = "".join(rng.choice("ACGT") for _ in range(length))
    reads = []
    for p in range(passes):
        s = noisy(rng, tpl, 0.04, 0.03, 0.01)
        reads.append({"seq": revcomp(s) if p % 2 else s, "flags": driver.FULL_PASS})
    reads[-1] = {"seq": reads[-1]["seq"][: length // 2], "flags": driver.ADAPTER_BEFORE}
    reads.insert(2, {"seq": noisy(rng, tpl + tpl + tpl[:20], 0.04, 0.03, 0.01), "flags": driver.FULL_PASS})
    return {"snr": [9.0, 8.0, 7.0, 10.0], "reads": reads}


@pytest.mark.parametrize("cap", [3, 5])
def test_driver_host_path_maps_the_reads_past_the_cap(cap):
    chunk = host_chunk()
    order = driver.filter_reads(chunk["reads"], 10)
    assert order[-1] is None and len(order) == len(chunk["reads"])
    status, base = driver.zmw_input(chunk, OraclePoa(), max_poa_coverage=cap)
    assert status is None and len(base["reads"]) == cap          # today's output: the reads stop at the cap
    assert driver.zmw_input(chunk, OraclePoa(), max_poa_coverage=cap, mapper=None) == (status, base)
    status, zmw = driver.zmw_input(chunk, OraclePoa(), max_poa_coverage=cap, mapper=map_restated)
    assert status is None and zmw["draft"] == base["draft"]
    assert len(zmw["reads"]) == len(order)                       # one entry per read of FilterReads' order
    assert zmw["reads"][:cap] == base["reads"]
    assert zmw["reads"][-1]["seq"] is None                       # the dropped read is a placeholder
    for r, got in zip(order[cap:-1], zmw["reads"][cap:-1]):
        m = map_restated(zmw["draft"], [r["seq"]])[0]
        assert got == driver.extract_mapped_read(r, m, 10)
        assert got["seq"] == r["seq"][m["read"][0]:m["read"][1]] and (got["ts"], got["te"]) == m["tpl"]
        assert got["te"] - got["ts"] > len(zmw["draft"]) // 3    # a real window, not a placeholder
    # no cap, or a cap no read lies past: the mapper is never called
    def never(draft, reads):
        raise AssertionError("mapper called")
    assert driver.zmw_input(chunk, OraclePoa(), mapper=never) == driver.zmw_input(chunk, OraclePoa())

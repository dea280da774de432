"""The banded POA fill's rules as tests/poa_band_restatement.py states them, checked without a
device: the ranges on unbranched graphs against tests/sparse_restatement.py, the ranges on hand-made branching
graphs against values worked out by hand from RangeFinder.cpp:71-165, and the containment property on seeded pairs."""
import poa_band_restatement as B
import sparse_restatement as R

BIG = B.INT_MAX // 2


def test_unbranched_graphs_give_the_linear_ranges():
    g = R.Lcg(7)
    pairs = []
    for n, err in ((40, 5), (150, 10), (333, 15), (600, 8)):
        t = g.seq(n)
        pairs.append((t, g.noisy(t, err)))
    t = g.seq(200)
    pairs.append((t, t[60:140]))            # positions before the first and after the last anchor
    pairs.append((g.seq(90), g.seq(70)))    # unrelated: few anchors or none
    pairs.append((g.seq(50), "A" * 30))     # no seeds at all: every position is (len2, 0)
    pairs.append((g.seq(80), g.seq(12)))    # I < WIDTH
    for t, q in pairs:
        chain = R.sparse_align(t, q, B.K)
        graph = B.chain_graph(t)
        css = list(range(2, 2 + len(t)))
        got = B.ranges_literal(graph, css, chain, len(q))
        assert [got[v] for v in css] == R.ranges_literal(chain, len(t), len(q)), (len(t), len(q))
    assert B.ranges_literal(B.chain_graph("ACGTAC"), list(range(2, 8)), [], 30)[4] == (30, 0)


# ^ = 0, $ = 1; the consensus path 2..8; a bubble 3 -> 9 -> 5 around vertex 4; a side branch ^ -> 10 -> $
_BASES = "^$ACGTACGTC"
_EDGES = [(0, 2), (2, 3), (3, 4), (4, 5), (5, 6), (6, 7), (7, 8), (8, 1), (3, 9), (9, 5), (0, 10), (10, 1)]
_CSS = [2, 3, 4, 5, 6, 7, 8]


def test_branching_graph_read_of_60():
    """Anchors at consensus positions 2 and 3 (vertices 4 and 5), read rows 50 and 51, I = 60.
    direct(4) = [20, min(80, 60)) and direct(5) = [21, 60): the upper clamp of the direct range.
    Forward marks: ^ is RangeUnion({}) = (BIG, -BIG); 2 = next(^) = (min(BIG + 1, 60), -BIG + 1) = (60, -BIG + 1);
    3 = (60, -BIG + 2); 9 = next(3) = (60, -BIG + 3); 6 = next(21, 60) = (22, min(61, 60)) -- next's clamp; 7 = (23, 60);
    8 = (24, 60); 10 = (60, -BIG + 1); $ = hull(next(8), next(10)) = (25, 60).
    Reverse marks: $ is (BIG, -BIG); 8 = prev($) = (BIG - 1, max(-BIG - 1, 0)) = (BIG - 1, 0) -- prev's clamp; 7 =
    (BIG - 2, 0); 6 = (BIG - 3, 0); 9 = prev(5) = (20, 59); 3 = hull(prev(4), prev(9)) = hull((19, 59), (19, 58)) = (19, 59);
    2 = (18, 58); 10 = prev($) = (BIG - 1, 0); ^ = hull(prev(2), prev(10)) = hull((17, 57), (BIG - 2, 0)) = (17, 57)."""
    graph = B.Graph(_BASES, _EDGES)
    got = B.ranges_literal(graph, _CSS, [(2, 50), (3, 51)], 60)
    assert got == {0: (17, 57), 2: (18, 58), 3: (19, 59), 4: (20, 60), 5: (21, 60), 9: (20, 59),
                   6: (22, 60), 7: (23, 60), 8: (24, 60),
                   10: (60, 0),          # no anchored ancestor or descendant: the inverted interval
                   1: (25, 60)}
    # the bands: closed above, so row I exists where E == I; the inverted interval is an empty column
    assert list(B.band_rows(got[4], 60)) == list(range(20, 61))
    assert list(B.band_rows(got[9], 60)) == list(range(20, 60))
    assert list(B.band_rows(got[10], 60)) == []
    # before the first anchor only the reverse mark is real, after the last only the forward one
    assert got[2] == (18, 58) and got[8] == (24, 60)


def test_branching_graph_read_of_10_clips_both_ends():
    """The same graph, anchors (2, 1) and (3, 2), I = 10 < WIDTH: direct(4) = [max(1 - 30, 0), min(31, 10)) = [0, 10)
    and direct(5) = [0, 10).  Forward: 6 = (1, 10), 7 = (2, 10), 8 = (3, 10), $ = hull((4, 10), (10, -BIG + 2));
    2 = (10, -BIG + 1), 3 = (10, -BIG + 2), 9 = (10, -BIG + 3), 10 = (10, -BIG + 1).  Reverse: 9 = prev(0, 10) =
    (max(-1, 0), 9) = (0, 9) -- prev's clamp on Begin; 3 = hull(prev(0, 10), prev(0, 9)) = (0, 9); 2 = (0, 8); ^ =
    hull((0, 7), (BIG - 2, 0)) = (0, 7); 8, 7, 6 = (BIG - 1, 0), (BIG - 2, 0), (BIG - 3, 0)."""
    graph = B.Graph(_BASES, _EDGES)
    got = B.ranges_literal(graph, _CSS, [(2, 1), (3, 2)], 10)
    assert got == {0: (0, 7), 2: (0, 8), 3: (0, 9), 4: (0, 10), 5: (0, 10), 9: (0, 9), 6: (1, 10), 7: (2, 10),
                   8: (3, 10), 10: (10, 0), 1: (4, 10)}
    assert list(B.band_rows(got[8], 10)) == list(range(3, 11))


def test_empty_columns_offer_nothing():
    """A fill under the ranges above: the side branch's column is empty, so vertex 10 never carries a step, and a
    cell next to it loses nothing but that candidate."""
    graph = B.Graph(_BASES, _EDGES)
    read = "TTTTTTTTTTTTTTTTTTTTACGTACGT" + "C" * 32       # rows 21..28 spell the consensus path
    assert len(read) == 60
    ranges = B.ranges_literal(graph, _CSS, [(2, 50), (3, 51)], 60)
    score, steps, cells = B.fill_and_trace(graph, read, ranges)
    assert all(v != 10 for v, _, _ in steps)
    assert B.inside(cells, ranges, 60)
    full_score, full_steps, full_cells = B.fill_and_trace(graph, read, None)
    assert full_score >= score
    # a band that holds nothing but row 0 of ^ still ends: the Start move closes every walk
    assert steps[0] == (B.EXIT, B.END_MOVE, 60) and steps[-1][1] == B.START_MOVE


def _pairs():
    """Read 1 against the chain of read 0: 150 to 600 bases, 5 to 15% errors, both strands."""
    out = []
    for k, (n, err) in enumerate(((150, 5), (150, 15), (220, 10), (300, 8), (300, 15), (380, 12), (450, 6), (450, 15),
                                  (520, 10), (600, 5), (600, 12), (600, 15))):
        g = R.Lcg(9100 + k)
        t = g.seq(n)
        r0, r1 = g.noisy(t, err), g.noisy(t, err)
        rc = k % 2 == 1
        given = R.revcomp(r1) if rc else r1          # the read as the instrument gives it
        out.append((r0, given, rc))
    return out


def test_containment_on_seeded_pairs():
    contained = 0
    pairs = _pairs()
    for r0, given, rc in pairs:
        q = R.revcomp(given) if rc else given
        graph = B.chain_graph(r0)
        css = list(range(2, 2 + len(r0)))
        chain = R.sparse_align(r0, q, B.K)
        assert chain, "a related pair has anchors"
        ranges = B.ranges_literal(graph, css, chain, len(q))
        full_score, full_steps, full_cells = B.fill_and_trace(graph, q, None)
        if not B.inside(full_cells, ranges, len(q)):
            continue
        contained += 1
        score, steps, _ = B.fill_and_trace(graph, q, ranges)
        assert (score, steps) == (full_score, full_steps), (len(r0), len(q), rc)
    assert contained >= 0.9 * len(pairs), "vacuous: %d of %d walks lie inside their bands" % (contained, len(pairs))

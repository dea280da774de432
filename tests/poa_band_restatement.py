"""A plain Python restatement of the banded POA fill's rules, shared by tests/test_poa_band_cpu.py
and tests/test_poa_band_gpu.py; it is not a test itself.

  * graph_from_dot: the graph (ids, bases, edges) a handle's GraphViz text describes;
  * ranges_literal: SdpRangeFinder::InitRangeFinder (RangeFinder.cpp:71-165) on that graph, from the consensus
    path and the anchors, with std::map-like dictionaries and the two recursions written as the reference writes them;
  * fill_and_trace: one LOCAL read against the graph, column by column and row by row as makeAlignmentColumn /
    makeAlignmentColumnForExit / tracebackAndThread's walk do it, a cell existing only inside its vertex's range
    (B <= i <= min(E, I)); with ranges=None every range is full, which is the reference's own fill.

Nothing here is shaped like the device code: dictionaries of rows, no prefix maxima, no column program."""
import re

INT_MAX = 2 ** 31 - 1
WIDTH = 30
K = 6
MATCH, MISMATCH, INSERT, DELETE = 3, -5, -4, -4
ENTER, EXIT = 0, 1
START_MOVE, END_MOVE, MATCH_MOVE, MISMATCH_MOVE, DELETE_MOVE, EXTRA_MOVE = 1, 2, 3, 4, 5, 6
EMPTY = (INT_MAX // 2, -(INT_MAX // 2))     # RangeUnion({})


class Graph:
    """Vertices 0..n-1 (^ = 0, $ = 1) with their bases; edges as (u, v) pairs."""

    def __init__(self, bases, edges):
        self.bases = list(bases)
        self.n = len(self.bases)
        self.preds = [[] for _ in range(self.n)]
        self.succs = [[] for _ in range(self.n)]
        for u, v in edges:
            self.preds[v].append(u)
            self.succs[u].append(v)
        for v in range(self.n):
            self.preds[v].sort()      # in-edges are visited by ascending source (PoaGraphImpl.hpp:130-143)
            self.succs[v].sort()

    def topological(self):
        """Some topological order of all vertices (Kahn's; which one does not matter to any rule)."""
        indeg = [len(p) for p in self.preds]
        ready = [v for v in range(self.n) if indeg[v] == 0]
        order = []
        while ready:
            v = ready.pop()
            order.append(v)
            for w in self.succs[v]:
                indeg[w] -= 1
                if indeg[w] == 0:
                    ready.append(w)
        assert len(order) == self.n, "the graph has a cycle"
        return order


_NODE = re.compile(r'^(\d+)\[shape=Mrecord,.* label="\{ (?:\{ \d+ \| )?(.) ')
_EDGE = re.compile(r"^(\d+)->(\d+) ;")


def graph_from_dot(text):
    bases, edges = {}, []
    for line in text.splitlines():
        m = _NODE.match(line)
        if m:
            bases[int(m.group(1))] = m.group(2)
            continue
        m = _EDGE.match(line)
        if m:
            edges.append((int(m.group(1)), int(m.group(2))))
    assert sorted(bases) == list(range(len(bases)))
    return Graph([bases[v] for v in range(len(bases))], edges)


def chain_graph(seq):
    """^ -> seq[0] -> ... -> seq[-1] -> $, numbered as AddFirstRead numbers it."""
    n = len(seq)
    edges = [(ENTER, 2)] + [(2 + k, 3 + k) for k in range(n - 1)] + [(1 + n, EXIT)]
    return Graph("^$" + seq, edges)


def _next(iv, upper):
    return (min(iv[0] + 1, upper), min(iv[1] + 1, upper))


def _prev(iv, lower=0):
    return (max(iv[0] - 1, lower), max(iv[1] - 1, lower))


def _union(ivs):
    b, e = EMPTY
    for x in ivs:
        b, e = min(b, x[0]), max(e, x[1])
    return (b, e)


def ranges_literal(graph, css_path, anchors, read_len):
    """{vertex: (B, E)} for every vertex, $ included."""
    by_css_pos = dict(anchors)
    order = graph.topological()
    direct = {v: None for v in order}
    for pos, v in enumerate(css_path):
        if pos in by_css_pos:
            q = by_css_pos[pos]
            direct[v] = (max(q - WIDTH, 0), min(q + WIDTH, read_len))
    fwd, rev = {}, {}
    for v in order:
        fwd[v] = direct[v] if direct[v] is not None else _union([_next(fwd[u], read_len) for u in graph.preds[v]])
    for v in reversed(order):
        rev[v] = direct[v] if direct[v] is not None else _union([_prev(rev[w], 0) for w in graph.succs[v]])
    return {v: _union([fwd[v], rev[v]]) for v in order}


def band_rows(rng, read_len):
    """The rows a column holds: B <= i <= min(E, I)."""
    return range(rng[0], min(rng[1], read_len) + 1)


def fill_and_trace(graph, read, ranges=None):
    """(exit score, steps, cells): steps as [(vertex, move, row of the visited cell)] from the End move into $ down
    to the Start move, cells the set of (vertex, row) the walk stood on or took a candidate from."""
    I = len(read)
    score, move = {}, {}
    for v in graph.topological():
        if v == EXIT:
            continue
        rows = band_rows(ranges[v], I) if ranges is not None else range(0, I + 1)
        sc, mv = {}, {}
        for i in rows:
            best, how, frm = 0, START_MOVE, ENTER      # LOCAL; row 0 is 0 by Start (or ^'s own 0)
            if i > 0:
                is_match = read[i - 1] == graph.bases[v]
                for u in graph.preds[v]:
                    if i - 1 in score[u]:
                        cand = score[u][i - 1] + (MATCH if is_match else MISMATCH)
                        if cand > best:
                            best, how, frm = cand, (MATCH_MOVE if is_match else MISMATCH_MOVE), u
                    if i in score[u]:
                        cand = score[u][i] + DELETE
                        if cand > best:
                            best, how, frm = cand, DELETE_MOVE, u
                if i - 1 in sc:
                    cand = sc[i - 1] + INSERT
                    if cand > best:
                        best, how, frm = cand, EXTRA_MOVE, v
            sc[i], mv[i] = best, (how, frm)
        score[v], move[v] = sc, mv
    # $: each column's first maximal existing row, the maximum over the columns by ascending vertex id, strict '>'
    best, best_v, best_row = None, None, None
    for u in range(graph.n):
        if u == EXIT or not score[u]:
            continue
        row = max(sorted(score[u]), key=lambda i: (score[u][i], -i))
        if best is None or score[u][row] > best:
            best, best_v, best_row = score[u][row], u, row
    steps = [(EXIT, END_MOVE, I)]
    cells = set()
    v, i = best_v, best_row
    while not (v == ENTER and i == 0):
        cells.add((v, i))
        how, frm = move[v][i]
        steps.append((v, how, i))
        if how == START_MOVE:
            v, i = ENTER, 0
        elif how == DELETE_MOVE:
            cells.add((frm, i))
            v = frm
        else:
            cells.add((frm, i - 1))
            v, i = frm, i - 1
    return best, steps, cells


def inside(cells, ranges, read_len):
    """Every cell of a walk exists under the ranges."""
    return all(v == ENTER and i == 0 or i in band_rows(ranges[v], read_len) for v, i in cells)

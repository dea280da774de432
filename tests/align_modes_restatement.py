"""The ends-free alignment rules, cell by cell in plain Python: what k_align_fill_ends and
k_align_trace_ends must equal in transcript, score and extents.  They are the reference POA's rules
(PoaGraphImpl.cpp:178-352) on a graph that holds the target as one unbranched path.

Query on rows i = 0..I, target on columns j = 0..J, params = (Match, Mismatch, Insert, Delete).
  borders   S(0, j) = 0 (Start); column 0: SEMIGLOBAL S(i, 0) = i * Insert (Extra), LOCAL 0 (Start)
  cell      in this order, a later one only when strictly greater: (LOCAL) Start 0; diagonal; Delete
            S(i, j-1) + Delete; Extra S(i-1, j) + Insert
  end cell  SEMIGLOBAL: row I, the smallest j holding the row's maximum; LOCAL: the maximum over all cells,
            the smallest j, then the smallest i
  walk      back to the first Start cell (i0, j0); M / R diagonal, D Delete, I Extra

align_ends is the plain form.  align_ends_np computes the same rows with numpy for the larger shapes of the GPU
tests; tests/test_align_modes_cpu.py pins it to the plain form on small inputs."""
import numpy as np

GLOBAL, SEMIGLOBAL, LOCAL = 0, 1, 2
DIAG, DELETE, EXTRA, START = 0, 1, 2, 3

_COMP = bytearray([127]) * 256
for _a, _b in zip(b"ACGTacgtNMnm-\x00\x01\x02\x03", b"TGCAtgcaMNmn-\x03\x02\x01\x00"):
    _COMP[_a] = _b
_COMP = bytes(_COMP)


def _bytes(s):
    return s if isinstance(s, bytes) else s.encode("latin-1")


def revcomp(s):
    """Sequence.cpp's ComplementArray (N <-> M, every other byte 127), reversed."""
    out = _bytes(s)[::-1].translate(_COMP)
    return out if isinstance(s, bytes) else out.decode("latin-1")


def fill(target, query, mode, params):
    """(S, mv): scores and moves, (I + 1) x (J + 1) lists."""
    t, q = _bytes(target), _bytes(query)
    match, mismatch, ins, dele = params
    I, J = len(q), len(t)
    S = [[0] * (J + 1) for _ in range(I + 1)]
    mv = [[START] * (J + 1) for _ in range(I + 1)]
    for i in range(1, I + 1):
        if mode == SEMIGLOBAL:
            S[i][0] = i * ins
            mv[i][0] = EXTRA
        for j in range(1, J + 1):
            best, move = None, None
            if mode == LOCAL:
                best, move = 0, START
            c = S[i - 1][j - 1] + (match if q[i - 1] == t[j - 1] else mismatch)
            if best is None or c > best:
                best, move = c, DIAG
            c = S[i][j - 1] + dele
            if c > best:
                best, move = c, DELETE
            c = S[i - 1][j] + ins
            if c > best:
                best, move = c, EXTRA
            S[i][j], mv[i][j] = best, move
    return S, mv


def end_cell(S, mode):
    I, J = len(S) - 1, len(S[0]) - 1
    if mode == SEMIGLOBAL:
        bj = 0
        for j in range(1, J + 1):
            if S[I][j] > S[I][bj]:
                bj = j
        return I, bj
    bi = bj = 0
    for j in range(J + 1):          # columns in order, a later one only when strictly greater
        for i in range(I + 1):      # the first maximal row
            if S[i][j] > S[bi][bj]:
                bi, bj = i, j
    return bi, bj


def walk(target, query, mv, i, j):
    """(transcript, i0, j0) from the end cell (i, j) back to the first Start cell."""
    t, q = _bytes(target), _bytes(query)
    out = []
    while mv[i][j] != START:
        m = mv[i][j]
        if m == DIAG:
            out.append("M" if q[i - 1] == t[j - 1] else "R")
            i, j = i - 1, j - 1
        elif m == DELETE:
            out.append("D")
            j -= 1
        else:
            out.append("I")
            i -= 1
    return "".join(reversed(out)), i, j


def _one(target, query, mode, params, filler):
    S, mv = filler(target, query, mode, params)
    i1, j1 = end_cell(S, mode)
    tr, i0, j0 = walk(target, query, mv, i1, j1)
    return tr, int(S[i1][j1]), {"target": (j0, j1), "query": (i0, i1), "rc": False}


def _both(target, query, mode, params, both_strands, filler):
    fwd = _one(target, query, mode, params, filler)
    if not both_strands:
        return fwd
    rev = _one(target, revcomp(query), mode, params, filler)
    if fwd[1] >= rev[1]:            # SparsePoa.cpp:112-132 without the threshold
        return fwd
    rev[2]["rc"] = True
    return rev


def align_ends(target, query, mode, params=(0, -1, -1, -1), both_strands=False):
    """(transcript, score, extent) by the plain rules."""
    return _both(target, query, mode, params, both_strands, fill)


def fill_np(target, query, mode, params):
    """fill, one numpy row at a time.  A row's Delete chain is a running maximum: with x(j) the best of the
    candidates that do not come from the left, S(i, j) = max over k <= j of x(k) + (j - k) * Delete.  The move
    is the first candidate, in the rule's order, that equals the cell."""
    t = np.frombuffer(_bytes(target), dtype=np.uint8)
    q = np.frombuffer(_bytes(query), dtype=np.uint8)
    match, mismatch, ins, dele = params
    I, J = len(q), len(t)
    S = np.zeros((I + 1, J + 1), dtype=np.int64)
    mv = np.full((I + 1, J + 1), START, dtype=np.uint8)
    ramp = np.arange(J + 1, dtype=np.int64) * dele
    for i in range(1, I + 1):
        x = np.empty(J + 1, dtype=np.int64)
        x[0] = i * ins if mode == SEMIGLOBAL else 0
        diag = S[i - 1, :-1] + np.where(t == q[i - 1], match, mismatch)
        extra = S[i - 1, 1:] + ins
        x[1:] = np.maximum(diag, extra)
        if mode == LOCAL:
            x[1:] = np.maximum(x[1:], 0)
        row = np.maximum.accumulate(x - ramp) + ramp
        S[i] = row
        dl = row[:-1] + dele
        m = np.where(diag == row[1:], DIAG, np.where(dl == row[1:], DELETE, EXTRA))
        if mode == LOCAL:
            m = np.where(row[1:] == 0, START, m)
        else:
            mv[i, 0] = EXTRA
        mv[i, 1:] = m
    return S, mv


def _end_cell_np(S, mode):
    if mode == SEMIGLOBAL:
        return S.shape[0] - 1, int(np.argmax(S[-1]))      # argmax: the first maximum
    mx = S.max()
    j = int(np.argmax((S == mx).any(axis=0)))
    return int(np.argmax(S[:, j] == mx)), j


def _one_np(target, query, mode, params):
    S, mv = fill_np(target, query, mode, params)
    i1, j1 = _end_cell_np(S, mode)
    tr, i0, j0 = walk(target, query, mv, i1, j1)
    return tr, int(S[i1, j1]), {"target": (j0, j1), "query": (i0, i1), "rc": False}


def align_ends_np(target, query, mode, params=(0, -1, -1, -1), both_strands=False):
    """align_ends through fill_np."""
    fwd = _one_np(target, query, mode, params)
    if not both_strands:
        return fwd
    rev = _one_np(target, revcomp(query), mode, params)
    if fwd[1] >= rev[1]:
        return fwd
    rev[2]["rc"] = True
    return rev


def global_score(target, query, params):
    """Needleman-Wunsch score of the two whole sequences (ties do not matter to a score)."""
    t, q = _bytes(target), _bytes(query)
    match, mismatch, ins, dele = params
    prev = [j * dele for j in range(len(t) + 1)]
    for i in range(1, len(q) + 1):
        cur = [i * ins] + [0] * len(t)
        for j in range(1, len(t) + 1):
            cur[j] = max(prev[j - 1] + (match if q[i - 1] == t[j - 1] else mismatch), cur[j - 1] + dele,
                         prev[j] + ins)
        prev = cur
    return prev[len(t)]

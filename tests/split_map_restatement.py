"""The split-mapping rule in plain Python: a read is placed on a draft as a chain of LOCAL
segments, on either strand, at a jump penalty.  No GPU, no library; tests/test_split_map_cpu.py pins it to
test_map_cpu.local_extents and to planted cases, tests/test_split_map_gpu.py pins the kernels to it.

Rows are the read as given for both orientations; orientation 0 has the draft on the columns, orientation 1 its
reverse complement.  G(i) is the best chain that ends at or before row i, less the jump penalty; it is the Start
value of every cell of row i + 1."""

MATCH, MISMATCH, INSERT, DELETE = 3, -5, -4, -4   # map::kMatch / kMismatch / kInsert / kDelete
_COMP = {"A": "T", "C": "G", "G": "C", "T": "A", "a": "t", "c": "g", "g": "c", "t": "a",
         "N": "M", "M": "N", "n": "m", "m": "n", "-": "-"}


def complement_columns(draft):
    """rc(draft) with map_kernels.hip's complement(): N <-> M, anything unknown matches nothing."""
    return [_COMP.get(c, "\x7f") for c in reversed(draft)]


def split_rows(draft, read, jump_penalty):
    """The row records: G[i] and R[i] = (score, o, j, start cell) for i = 1..I (R[0] is None)."""
    n_i, n_j = len(read), len(draft)
    cols = (list(draft), complement_columns(draft))
    G = [0] * (n_i + 1)
    R = [None] * (n_i + 1)
    prev_s = [[0] * (n_j + 1) for _ in range(2)]
    prev_o = [[(0, j) for j in range(n_j + 1)] for _ in range(2)]
    for i in range(1, n_i + 1):
        g = G[i - 1]
        b = read[i - 1]
        best = None
        for o in range(2):
            col, ps, po = cols[o], prev_s[o], prev_o[o]
            cur_s, cur_o = [g] * (n_j + 1), [(i, 0)] * (n_j + 1)
            for j in range(1, n_j + 1):
                s, st = g, (i, j)                                   # Start
                c = ps[j - 1] + (MATCH if b == col[j - 1] else MISMATCH)
                if c > s:
                    s, st = c, po[j - 1]                            # diagonal
                c = cur_s[j - 1] + DELETE
                if c > s:
                    s, st = c, cur_o[j - 1]                         # Delete (left)
                c = ps[j] + INSERT
                if c > s:
                    s, st = c, po[j]                                # Extra (up)
                cur_s[j], cur_o[j] = s, st
                if best is None or s > best[0]:                     # o = 0 first, then the smaller j
                    best = (s, o, j, st)
            prev_s[o], prev_o[o] = cur_s, cur_o
        R[i] = best
        G[i] = best[0] - jump_penalty if best[0] - jump_penalty > g else g
    return G, R


def split_map(draft, read, jump_penalty, max_segments=8):
    """None for no read or a chain score of 0, else {"score", "n_segments", "truncated", "segments": [{"rc", "read",
    "tpl", "score"}]}: the last max_segments segments of the chain in read order, extents on the read as given and
    on the draft."""
    if not read:
        return None
    n_j = len(draft)
    G, R = split_rows(draft, read, jump_penalty)
    end, score = 0, 0
    for i in range(1, len(read) + 1):
        if R[i][0] > score:
            end, score = i, R[i][0]
    if score == 0:
        return None
    segs = []
    r = end
    while True:
        h, o, j1, (i0, j0) = R[r]
        g = G[i0 - 1] if i0 > 0 else 0
        segs.append({"rc": bool(o), "read": (i0, r), "tpl": (n_j - j1, n_j - j0) if o else (j0, j1), "score": h - g})
        if g == 0:
            break
        r = G.index(g)            # the smallest row with G(r) = g
    segs.reverse()
    return {"score": score, "n_segments": len(segs), "truncated": len(segs) > max_segments,
            "segments": segs[-max_segments:]}


def split_map_restated(draft, reads, jump_penalty, max_segments=8):
    """mapping.split_map_to_draft's contract."""
    return [split_map(draft, r, jump_penalty, max_segments) for r in reads]


def accept_split(res, read_len, min_length):
    """The driver's acceptance rule for a read FilterReads dropped: not truncated, at least two segments,
    consecutive segments on alternating strands, at least two segments whose read extent reaches min_length."""
    if res is None or res["truncated"] or len(res["segments"]) < 2:
        return False
    segs = res["segments"]
    if any(a["rc"] == b["rc"] for a, b in zip(segs, segs[1:])):
        return False
    return sum(1 for s in segs if s["read"][1] - s["read"][0] >= min_length) >= 2

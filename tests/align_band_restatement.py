"""The banded fill of the pairwise aligners, restated: tests/test_align_cpu.py's ref_align / ref_affine with every
cell outside the band dead.  The query is on rows i, the target on columns j; the band of
half-width w holds the diagonals lo <= j - i <= hi, lo = min(0, J - I) - w, hi = max(0, J - I) + w.  A dead cell's
value is forced (NW: -2^30; affine: -FLT_MAX in both states), border cells included; a live cell is computed from
its three neighbours exactly as in the full restatement, every affine sum one numpy.float32 add.  The traceback is
the full restatement's, over the banded matrices; where it would read a dead cell the transcript is None (the score is
still the banded fill's)."""
import numpy as np

from tests.test_align_cpu import (AFFINE_DEFAULT, F32, IUPAC_DEFAULT, NEG, NW_DEFAULT, WalkLeavesMatrix, match_score)

NW_DEAD = -(1 << 30)


def band_of(I, J, w):
    delta = J - I
    return min(0, delta) - w, max(0, delta) + w


def smax1(a, b):   # std::max on scalars: a unless a < b
    return b if a < b else a


def banded_align(target, query, w, params=NW_DEFAULT):
    """(transcript, Score(I, J)) of the NW fill inside the band; transcript None where the walk leaves the band."""
    match, mismatch, insert, delete = params
    I, J = len(query), len(target)
    lo, hi = band_of(I, J, w)
    live = lambda i, j: lo <= j - i <= hi
    S = [[NW_DEAD] * (J + 1) for _ in range(I + 1)]
    for i in range(I + 1):
        if live(i, 0):
            S[i][0] = i * insert
    for j in range(J + 1):
        if live(0, j):
            S[0][j] = j * delete
    for i in range(1, I + 1):
        for j in range(max(1, i + lo), min(J, i + hi) + 1):
            S[i][j] = max(S[i - 1][j - 1] + (match if query[i - 1] == target[j - 1] else mismatch),
                          max(S[i - 1][j] + insert, S[i][j - 1] + delete))
    tr = []
    i, j = I, J
    while i > 0 or j > 0:
        if not live(i, j):
            return None, S[I][J]
        if i == 0:
            move = 2
        elif j == 0:
            move = 1
        else:
            a = S[i - 1][j - 1] + (match if query[i - 1] == target[j - 1] else mismatch)
            b = S[i - 1][j] + insert
            c = S[i][j - 1] + delete
            move = 0 if (a >= b and a >= c) else (1 if b >= c else 2)   # ArgMax3
        if move == 0:
            i, j = i - 1, j - 1
            tr.append("M" if query[i] == target[j] else "R")
        elif move == 1:
            i -= 1
            tr.append("I")
        else:
            j -= 1
            tr.append("D")
    return "".join(reversed(tr)), S[I][J]


def banded_affine(target, query, w, params=AFFINE_DEFAULT, iupac=False):
    """(transcript, max(M, GAP)(I, J) as numpy.float32) of the affine fill inside the band."""
    p = tuple(F32(x) for x in params)
    open_, ext = p[2], p[3]
    I, J = len(query), len(target)
    lo, hi = band_of(I, J, w)
    live = lambda i, j: lo <= j - i <= hi
    with np.errstate(over="ignore", invalid="ignore"):
        M = [[NEG] * (J + 1) for _ in range(I + 1)]
        G = [[NEG] * (J + 1) for _ in range(I + 1)]
        M[0][0] = F32(0)
        for i in range(1, I + 1):
            if live(i, 0):
                G[i][0] = F32(open_ + F32(F32(i - 1) * ext))
        for j in range(1, J + 1):
            if live(0, j):
                G[0][j] = F32(open_ + F32(F32(j - 1) * ext))
        for i in range(1, I + 1):
            for j in range(max(1, i + lo), min(J, i + hi) + 1):
                sc = match_score(target[j - 1], query[i - 1], p, iupac)
                M[i][j] = F32(smax1(M[i - 1][j - 1], G[i - 1][j - 1]) + sc)
                G[i][j] = smax1(smax1(F32(M[i][j - 1] + open_), F32(G[i][j - 1] + ext)),
                                smax1(F32(M[i - 1][j] + open_), F32(G[i - 1][j] + ext)))
        tr = []
        i, j = I, J
        in_m = bool(M[I][J] >= G[I][J])
        score = F32(M[I][J] if M[I][J] >= G[I][J] else G[I][J])
        while i > 0 or j > 0:
            if not live(i, j):
                return None, score
            if in_m:
                if i == 0 or j == 0:
                    raise WalkLeavesMatrix()
                prev_m = bool(M[i - 1][j - 1] >= G[i - 1][j - 1])
                i, j = i - 1, j - 1
                tr.append("M" if query[i] == target[j] else "R")
            else:
                s = [F32(M[i][j - 1] + open_) if j > 0 else NEG, F32(G[i][j - 1] + ext) if j > 0 else NEG,
                     F32(M[i - 1][j] + open_) if i > 0 else NEG, F32(G[i - 1][j] + ext) if i > 0 else NEG]
                arg = 0
                for k in range(1, 4):   # std::max_element: the first maximum
                    if s[arg] < s[k]:
                        arg = k
                prev_m = arg in (0, 2)
                if arg < 2:
                    if j == 0:
                        raise WalkLeavesMatrix()
                    j -= 1
                    tr.append("D")
                else:
                    if i == 0:
                        raise WalkLeavesMatrix()
                    i -= 1
                    tr.append("I")
            in_m = prev_m
    return "".join(reversed(tr)), score


def banded(kind, target, query, w, params=None):
    """The banded restatement by kind (0 NW, 1 affine, 2 IUPAC-aware affine): (transcript, score)."""
    if kind == 0:
        return banded_align(target, query, w, tuple(params) if params else NW_DEFAULT)
    return banded_affine(target, query, w, tuple(params) if params else (AFFINE_DEFAULT if kind == 1 else IUPAC_DEFAULT),
                         kind == 2)


def block_indel_pair(k, seed=1):
    """A 120-base target and its copy with k bases inserted at one place and k other bases deleted 40 further on:
    I == J, and the optimal path runs k diagonals off the main one for 40 columns."""
    import random
    rng = random.Random(seed * 1000 + k)
    target = "".join(rng.choice("ACGT") for _ in range(120))
    ins = "".join(rng.choice("ACGT") for _ in range(k))
    query = target[:30] + ins + target[30:70] + target[70 + k:]
    assert len(query) == len(target)
    return target, query


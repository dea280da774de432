"""The certified band of the pairwise aligners, host side: the exported certificate
(pbccs_align_band_bound, pbccs_align_band_widen; no engine, no GPU) against the banded restatement
(tests/align_band_restatement.py) and the full restatement of tests/test_align_cpu.py.

Wherever the certificate holds for a banded score, the banded transcript and score are the full fill's; the
certificate is sharp on a block indel; the widened half-width certifies."""
import itertools
import math
import random

import pytest

from tests.align_band_restatement import banded, block_indel_pair
from tests.test_align_cpu import ref

NW, AFFINE, IUPAC = 0, 1, 2
# (kind, values, the parameter conditions hold): one non-dyadic set, two sets that cannot be certified
PARAM_SETS = [
    (NW, None, True),
    (NW, (2, -1, -2, -2), True),
    (NW, (1, 0, -1, -1), True),
    (NW, (0, -3, 1, -1), True),                         # one positive gap score, but Insert + Delete <= s+
    (NW, (0, -1, 1, 1), False),                         # a positive gap pair pays
    (AFFINE, None, True),
    (AFFINE, (1.0, -1.0, -2.0, 0.25, 0.0), True),      # 2 g+ = 0.5 <= 1
    (AFFINE, (0.3, -1.1, -2.7, -0.4, -0.6), True),     # not dyadic: E > 0
    (AFFINE, (0.0, -1.0, 0.5, -0.5, 0.0), False),      # 2 g+ = 1 > 0
    (IUPAC, None, True),
    (IUPAC, (0.0, -1.0, -1.0, -0.5, 0.5), True),       # s+ is the partial match score
]


def params_of(kind, values):
    import pbccs_amd as P
    if values is None:
        return None
    if kind == NW:
        return P.AlignConfig(P.AlignParams(*values))
    return P.AffineAlignmentParams(*values)


def conditions_hold(kind, values):
    """The parameter conditions of the certificate, restated."""
    if kind == NW:
        m, x, i, d = values or (0, -1, -1, -1)
        return i + d <= max(m, x)
    m, x, o, e, p = values or ((0.0, -1.0, -1.0, -0.5, 0.0) if kind == AFFINE else (0.0, -1.0, -1.0, -0.5, -0.25))
    sp = max(m, x, p) if kind == IUPAC else max(m, x)
    return 2 * max(o, e) <= sp


def tiny_pairs():
    rng = random.Random(2718)
    pairs = [("A" * j, "A" * i) for i in range(10) for j in range(10)]
    ac = ["".join(s) for n in range(4) for s in itertools.product("AC", repeat=n)]
    pairs += [(t, q) for t in ac for q in ac]
    for alphabet, count in (("AC", 120), ("ACGTRYSWKMN", 160)):
        for _ in range(count):
            pairs.append(("".join(rng.choice(alphabet) for _ in range(rng.randint(0, 9))),
                          "".join(rng.choice(alphabet) for _ in range(rng.randint(0, 9)))))
    return pairs


def same_score(kind, a, b):
    if kind == NW:
        return a == b
    if float(a) == 0.0 and float(b) == 0.0:   # a numerically zero score is exempt from sign
        return True
    return float(a).hex() == float(b).hex()


def test_parameter_sets_are_what_they_claim():
    for kind, values, ok in PARAM_SETS:
        assert conditions_hold(kind, values) == ok, (kind, values)
    assert sum(1 for _, _, ok in PARAM_SETS if not ok) >= 2


@pytest.mark.parametrize("kind,values", [(k, v) for k, v, _ in PARAM_SETS])
def test_certified_band_equals_full_exhaustive_tiny(kind, values):
    from pbccs_amd import align as A
    n_cert = n_not = n_dead = 0
    for t, q in tiny_pairs():
        I, J = len(q), len(t)
        full = None
        for w in range(max(I, J) + 2):
            u, e, ok = A.align_band_bound(kind, I, J, w, params_of(kind, values))
            assert ok == conditions_hold(kind, values), (kind, values, I, J, w)
            assert e >= 0.0 and (e == 0.0 or values == (0.3, -1.1, -2.7, -0.4, -0.6))
            if not ok:
                n_dead += 1
                continue
            btr, bs = banded(kind, t, q, w, values)   # btr None: the walk read a dead cell
            if not float(bs) > u + e:
                n_not += 1
                continue
            n_cert += 1
            if full is None:
                full = ref(kind, t, q, values)
            assert btr is not None, (kind, values, t, q, w)
            assert btr == full[0], (kind, values, t, q, w)
            assert same_score(kind, bs, full[1]), (kind, values, t, q, w, bs, full[1])
    if conditions_hold(kind, values):
        assert n_cert > 1000 and n_not > 50 and n_dead == 0
    else:
        assert n_cert == 0 and n_not == 0 and n_dead > 1000


@pytest.mark.parametrize("k", (1, 5, 12))
def test_certificate_is_sharp_on_a_block_indel(k):
    """Default NW, I == J == 120: the optimal path runs on diagonal -k, the band's edge at w = k."""
    from pbccs_amd import align as A
    t, q = block_indel_pair(k)
    tr, score = ref(NW, t, q)
    assert score == -2 * k and len(t) == len(q) == 120      # a condition on the input
    btr, bs = banded(NW, t, q, k)
    u, e, ok = A.align_band_bound(NW, 120, 120, k)
    assert ok and e == 0.0 and u == -2 * (k + 1)
    assert bs > u and (btr, bs) == (tr, score)
    # one narrower: the band cannot hold the path, and whatever it scores is not certified
    _, bs1 = banded(NW, t, q, k - 1)
    u1, _, _ = A.align_band_bound(NW, 120, 120, k - 1)
    assert u1 == -2 * k and bs1 <= score and not bs1 > u1
    assert A.align_band_widen(NW, 120, 120, bs1) >= k
    assert A.align_band_widen(NW, 120, 120, score) == k


def test_widened_band_certifies():
    """w2 from a first attempt's score: the smallest certifying width, and the banded fill at w2 is the full one."""
    from pbccs_amd import align as A
    rng = random.Random(99)
    n_second = 0
    for kind, values, ok in PARAM_SETS:
        if not ok:
            assert A.align_band_widen(kind, 30, 33, -5.0, params_of(kind, values)) == -1
            continue
        for _ in range(12):
            q = "".join(rng.choice("ACGT") for _ in range(rng.randint(20, 40)))
            t = list(q)
            for _ in range(rng.randint(0, 6)):
                pos = rng.randrange(len(t))
                if rng.random() < 0.5:
                    del t[pos]
                else:
                    t.insert(pos, rng.choice("ACGT"))
            t = "".join(t) or "A"
            I, J = len(q), len(t)
            _, s1 = banded(kind, t, q, 0, values)
            u0, e0, _ = A.align_band_bound(kind, I, J, 0, params_of(kind, values))
            if float(s1) > u0 + e0:
                continue
            n_second += 1
            w2 = A.align_band_widen(kind, I, J, float(s1), params_of(kind, values))
            assert 0 < w2 <= max(I, J)
            u, e, _ = A.align_band_bound(kind, I, J, w2, params_of(kind, values))
            assert float(s1) > u + e
            u1, e1, _ = A.align_band_bound(kind, I, J, w2 - 1, params_of(kind, values))
            assert not float(s1) > u1 + e1
            btr, bs = banded(kind, t, q, w2, values)
            assert float(bs) >= float(s1) and float(bs) > u + e   # certified by construction
            full = ref(kind, t, q, values)
            assert btr == full[0] and same_score(kind, bs, full[1])
    assert n_second >= 20


def test_bound_edges():
    from pbccs_amd import align as A
    # no path can leave a band that holds the whole matrix
    u, e, ok = A.align_band_bound(NW, 5, 9, 9)
    assert u == -math.inf and e == 0.0 and ok
    # the dead-cell value's range: (I + J + 1) max|param| <= 2^30
    import pbccs_amd as P
    big = P.AlignConfig(P.AlignParams(0, -(1 << 20), -(1 << 20), -(1 << 20)))
    assert A.align_band_bound(NW, 500, 500, 3, big)[2] is True
    assert A.align_band_bound(NW, 512, 512, 3, big)[2] is False
    # the defaults are exact in float32 for any length the aligner takes; a non-dyadic set is not
    assert A.align_band_bound(AFFINE, 50000, 50000, 10)[1] == 0.0
    _, e, ok = A.align_band_bound(AFFINE, 1000, 1000, 10, P.AffineAlignmentParams(0.3, -1.1, -2.7, -0.4, -0.6))
    n, B, u24 = 2000, 2001 * 2.7, 2.0 ** -24
    assert ok and n * u24 * B <= e <= 1.01 * n * u24 * B / (1 - n * u24) + 1e-9

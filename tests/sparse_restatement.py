"""A plain Python restatement of the reference's SparseAlign<K> (include/pacbio/ccs/SparseAlignment.h FindSeeds,
src/ChainSeeds.cpp ChainSeeds with matchReward 3) and of SdpRangeFinder::InitRangeFinder on a graph that holds only
the draft, plus the seeded generator the recorded cases of tests/golden/sparse_align_ref.json were drawn from.
Shared by tests/test_sparse_align_cpu.py and tests/test_sparse_align_gpu.py; it is not a test itself.

The two sweep sets and the column set are kept as sorted Python lists and walked exactly as ChainSeeds.cpp walks
its std::sets; nothing here is shaped like the device code."""
import bisect
import json
import os
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "sparse_align_ref.json")
MATCH_REWARD = 3
WIDTH = 30
INT_MAX = 2 ** 31 - 1
_COMP = {"A": "T", "C": "G", "G": "C", "T": "A"}


def revcomp(s):
    return "".join(_COMP[c] for c in reversed(s))


def find_seeds(target, query, k):
    """Seeds (h, v) in (v, h) order: every target position holding the query's K-mer at v, homopolymers skipped."""
    if len(target) < k or len(query) < k:
        return []
    index = {}
    for i in range(len(target) - k + 1):
        index.setdefault(target[i:i + k], []).append(i)
    seeds = []
    for j in range(len(query) + 1 - k):
        kmer = query[j:j + k]
        if kmer == kmer[0] * k:
            continue
        for i in index.get(kmer, ()):
            seeds.append((i, j))
    return seeds


def link_score(a, b, k):
    fwd = min(a[0] - b[0], a[1] - b[1])
    indels = abs((a[0] - a[1]) - (b[0] - b[1]))
    matches = k - max(0, k - fwd)
    mismatches = fwd - matches
    return MATCH_REWARD * matches - indels - mismatches


def visible_left(seeds, k):
    """ComputeVisibilityLeft: for each seed the sweep set's upper_bound under the (diagonal, h) order."""
    n = len(seeds)
    order = sorted(range(n), key=lambda t: (seeds[t][0], seeds[t][1]))
    visible = [None] * n
    sweep = []   # sorted (d, h, index)
    rem = 0
    a = 0
    while a < n:
        col = seeds[order[a]][0]
        b = a
        while b < n and seeds[order[b]][0] == col:
            s = order[b]
            h, v = seeds[s]
            at = bisect.bisect_right(sweep, (h - v, h, n))
            if at < len(sweep):
                visible[s] = sweep[at][2]
            b += 1
        for s in order[a:b]:
            h, v = seeds[s]
            bisect.insort(sweep, (h - v, h, s))
        while rem < n and seeds[order[rem]][0] + k < col:
            h, v = seeds[order[rem]]
            sweep.pop(bisect.bisect_left(sweep, (h - v, h, order[rem])))
            rem += 1
        a = b
    return visible


def chain_seeds(seeds, k, trace=None, replace_same_column=False):
    """ChainSeeds: (chain as a list of (h, v), best chain score or None).  trace, when a dict, counts how often
    the column set found a lower entry at the leaving seed's own column and kept its seed (std::set::insert does
    not replace).  replace_same_column=True is what ChainSeeds does NOT do; it serves only to find inputs on which
    that rule decides the chain."""
    n = len(seeds)
    scores = [k] * n
    visible = visible_left(seeds, k)
    order = sorted(range(n), key=lambda t: (seeds[t][1], seeds[t][0]))
    pred = [None] * n
    sweep = []        # sorted (d, h, index)
    columns = []      # sorted column keys
    col_seed = {}     # column -> seed index
    best_score, best_end = None, None
    rem = 0

    def z(t):
        return scores[t] + seeds[t][0] + seeds[t][1]

    a = 0
    while a < n:
        row = seeds[order[a]][1]
        b = a
        while b < n and seeds[order[b]][1] == row:
            s = order[b]
            h, v = seeds[s]
            cand_score, cand = None, None
            at = bisect.bisect_left(columns, h)
            if at > 0:
                t = col_seed[columns[at - 1]]
                cand_score, cand = scores[t] + link_score(seeds[s], seeds[t], k), t
            at = bisect.bisect_left(sweep, (h - v, h, -1))
            if at > 0:
                t = sweep[at - 1][2]
                sc = scores[t] + link_score(seeds[s], seeds[t], k)
                if cand is None or sc > cand_score:
                    cand_score, cand = sc, t
            t = visible[s]
            if t is not None:
                sc = scores[t] + link_score(seeds[s], seeds[t], k)
                if cand is None or sc > cand_score:
                    cand_score, cand = sc, t
            if cand is not None and cand_score > 0:
                scores[s] = cand_score
                pred[s] = cand
                if best_score is None or cand_score > best_score:
                    best_score, best_end = cand_score, s
            b += 1
        for s in order[a:b]:
            h, v = seeds[s]
            bisect.insort(sweep, (h - v, h, s))
        while rem < n and seeds[order[rem]][1] + k < row:
            t = order[rem]
            h, v = seeds[t]
            col = h + k
            if col not in col_seed or z(col_seed[col]) < z(t):
                if col not in col_seed:
                    col_seed[col] = t
                    bisect.insort(columns, col)
                elif replace_same_column:
                    col_seed[col] = t
                elif trace is not None:
                    trace["kept_old_seed"] = trace.get("kept_old_seed", 0) + 1
                at = bisect.bisect_right(columns, col)
                erased = 0
                while at < len(columns) and z(col_seed[columns[at]]) < z(t):
                    del col_seed[columns[at]]
                    columns.pop(at)
                    erased += 1
                if trace is not None and erased and col_seed[col] != t:
                    trace["kept_old_and_erased"] = trace.get("kept_old_and_erased", 0) + 1
            sweep.pop(bisect.bisect_left(sweep, (h - v, h, t)))
            rem += 1
        a = b
    chain = []
    t = best_end
    while t is not None:
        chain.append(seeds[t])
        t = pred[t]
    chain.reverse()
    return chain, best_score


def sparse_align(target, query, k, trace=None):
    if not query:
        return []
    return chain_seeds(find_seeds(target, query, k), k, trace)[0]


def sparse_align_full(target, query, k):
    """(n_seeds, chain, score): score 0 for an empty chain."""
    seeds = find_seeds(target, query, k) if query else []
    chain, score = chain_seeds(seeds, k)
    return len(seeds), chain, (score if chain else 0)


# ---- alignable ranges on a linear draft ------------------------------------------------------------------------
def ranges_literal(chain, len1, len2):
    """InitRangeFinder's two recursions on ^ -> d_0 .. d_{J-1} -> $, literally."""
    direct = {}
    for h, v in chain:
        direct[h] = (max(v - WIDTH, 0), min(v + WIDTH, len2))
    empty = (INT_MAX // 2, -(INT_MAX // 2))
    fwd = [None] * len1
    prev = empty
    for p in range(len1):
        prev = fwd[p] = direct[p] if p in direct else (min(prev[0] + 1, len2), min(prev[1] + 1, len2))
    rev = [None] * len1
    nxt = empty
    for p in range(len1 - 1, -1, -1):
        nxt = rev[p] = direct[p] if p in direct else (max(nxt[0] - 1, 0), max(nxt[1] - 1, 0))
    return [(min(f[0], r[0]), max(f[1], r[1])) for f, r in zip(fwd, rev)]


def ranges_closed_form(chain, len1, len2):
    """The same from the nearest anchor on each side (what the device computes)."""
    big = INT_MAX // 2
    hs = [h for h, _ in chain]
    out = []
    for p in range(len1):
        at = bisect.bisect_right(hs, p)      # anchors with h <= p
        if at > 0 and hs[at - 1] == p:
            v = chain[at - 1][1]
            out.append((max(v - WIDTH, 0), min(v + WIDTH, len2)))
            continue
        if at > 0:
            h, v = chain[at - 1]
            f = (min(max(v - WIDTH, 0) + (p - h), len2), min(min(v + WIDTH, len2) + (p - h), len2))
        else:
            f = (min(big + p + 1, len2), min(-big + p + 1, len2))
        if at < len(chain):
            h, v = chain[at]
            r = (max(max(v - WIDTH, 0) - (h - p), 0), max(min(v + WIDTH, len2) - (h - p), 0))
        else:
            r = (max(big - (len1 - p), 0), max(-big - (len1 - p), 0))
        out.append((min(f[0], r[0]), max(f[1], r[1])))
    return out


def cells_in_ranges(ranges):
    return sum(max(0, e - b) for b, e in ranges)


# ---- the seeded generator behind the recorded cases ------------------------------------------------------------
class Lcg:
    """Knuth's 64-bit LCG; the upper bits only.  Written out so that the cases do not depend on a library."""

    def __init__(self, seed):
        self.x = (seed * 2862933555777941757 + 3037000493) & (2 ** 64 - 1)

    def below(self, n):
        self.x = (self.x * 6364136223846793005 + 1442695040888963407) & (2 ** 64 - 1)
        return (self.x >> 33) % n

    def seq(self, n, alphabet="ACGT"):
        return "".join(alphabet[self.below(len(alphabet))] for _ in range(n))

    def noisy(self, s, pct, alphabet="ACGT"):
        out = []
        for c in s:
            r = self.below(300)
            if r < pct:           # substitution
                out.append(alphabet[self.below(len(alphabet))])
            elif r < 2 * pct:     # deletion
                continue
            elif r < 3 * pct:     # insertion
                out.append(c)
                out.append(alphabet[self.below(len(alphabet))])
            else:
                out.append(c)
        return "".join(out)


def make_pair(spec):
    """spec: {"kind", "seed", "n", ...} -> (target, query)."""
    g = Lcg(spec["seed"])
    kind, n = spec["kind"], spec["n"]
    ab = spec.get("ab", "ACGT")
    if kind == "copy":            # random target, noisy copy at err percent
        t = g.seq(n, ab)
        return t, g.noisy(t, spec["err"], ab)
    if kind == "tandem":          # a period-p repeat and a noisy copy of it
        unit = g.seq(spec["p"], ab)
        while spec["p"] > 1 and unit == unit[0] * spec["p"]:
            unit = g.seq(spec["p"], ab)
        t = (unit * (n // spec["p"] + 1))[:n]
        return t, g.noisy(t, spec["err"], ab)
    if kind == "suffix":
        t = g.seq(n, ab)
        return t, t[n - spec["m"]:]
    if kind == "prefix":
        t = g.seq(n, ab)
        return t, t[:spec["m"]]
    if kind == "unrelated":
        return g.seq(n, ab), g.seq(spec["m"], ab)
    if kind == "short":           # lengths around K on either side
        t = g.seq(n, ab)
        return t, (t + g.seq(8, ab))[:spec["m"]]
    raise ValueError(kind)


def rle_encode(chain):
    """Runs along diagonals: flat [h, v, run, h, v, run, ...]."""
    out = []
    for h, v in chain:
        if out and out[-3] + out[-1] == h and out[-2] + out[-1] == v:
            out[-1] += 1
        else:
            out += [h, v, 1]
    return out


def rle_decode(flat):
    chain = []
    for a in range(0, len(flat), 3):
        h, v, run = flat[a:a + 3]
        chain += [(h + r, v + r) for r in range(run)]
    return chain


def pair_crc(target, query):
    return zlib.crc32((target + "/" + query).encode())


_cases = None


def golden_cases():
    """[(name, k, target, query, n_seeds, chain)] of every recorded case; loaded once and shared."""
    global _cases
    if _cases is None:
        doc = json.load(open(GOLDEN))
        cases = []
        for c in doc["known_answers"]:
            cases.append((c["name"], c["k"], c["target"], c["query"], c["n_seeds"], rle_decode(c["chain"])))
        for c in doc["seeded"]:
            t, q = make_pair(c["spec"])
            assert pair_crc(t, q) == c["crc"], c["spec"]
            name = "%s-%d-k%d" % (c["spec"]["kind"], c["spec"]["seed"], c["k"])
            cases.append((name, c["k"], t, q, c["n_seeds"], rle_decode(c["chain"])))
        _cases = cases
    return _cases

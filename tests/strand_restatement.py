"""The strand-discordance screen's two rules, stated literally in Python over per-read score lists.

A per-read entry is the read's Scores(m, .) term, or None for a read that does not enter the sums: an inactive read,
or one that does not score the mutation (ReadScoresMutation).  Reads come in AddRead order; strands are 0 (forward)
and 1 (reverse).
"""

DEFAULT_MIN_SCORE = 12.5
DEFAULT_MIN_READS = 2


def strand_sums(per_read, strands):
    """k_strand_sums for one mutation: (sum_fwd, sum_rev, n_fwd, n_rev); sequential adds in read order, no break."""
    sum_f = sum_r = 0.0
    n_f = n_r = 0
    for v, s in zip(per_read, strands):
        if v is None:
            continue
        if s == 0:
            sum_f += v
            n_f += 1
        else:
            sum_r += v
            n_r += 1
    return sum_f, sum_r, n_f, n_r


def qualifies(sums, min_score=DEFAULT_MIN_SCORE, min_reads=DEFAULT_MIN_READS):
    """A mutation qualifies when both strands have min_reads scoring reads and one sum lies above min_score while
    the other lies below -min_score.  A NaN sum compares false."""
    sum_f, sum_r, n_f, n_r = sums
    if n_f < min_reads or n_r < min_reads:
        return False
    return (sum_f > min_score and sum_r < -min_score) or (sum_r > min_score and sum_f < -min_score)


def strand_sites(mutations, sums, min_score=DEFAULT_MIN_SCORE, min_reads=DEFAULT_MIN_READS):
    """k_strand_sites: mutations = [(type, pos, base)] in enumeration order (grouped by position), sums = their
    strand_sums.  One (pos, type, base, sum_fwd, sum_rev) per discordant position, in template order: the
    qualifying mutation with the largest min(|sum_fwd|, |sum_rev|), the first in enumeration order on a tie."""
    best = {}
    order = []
    for (t, p, b), s in zip(mutations, sums):
        if not qualifies(s, min_score, min_reads):
            continue
        v = min(abs(s[0]), abs(s[1]))
        if p not in best:
            order.append(p)
            best[p] = (v, (p, t, b, s[0], s[1]))
        elif v > best[p][0]:
            best[p] = (v, (p, t, b, s[0], s[1]))
    return [best[p][1] for p in sorted(order)]

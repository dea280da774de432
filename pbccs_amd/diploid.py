"""Diploid site calling (ConsensusCore Arrow/Diploid.cpp:94-241, Quiver/Diploid.cpp): DiploidSite and
IsSiteHeterozygous as the reference's SWIG binding exposes them, and the scorers' SiteScores / DiploidSites.

A site's scores are an (n_reads, 9) float32 matrix: columns Scores(Substitution(p, ACGT)), Scores(Insertion(p,
ACGT)), Scores(Deletion(p)), the order LENGTH_DIFFS assumes.  IsSiteHeterozygous is host-only; the scorers'
calls build the site tensor on the GPU and screen every site there."""
import ctypes

import numpy as np

from . import lib as _lib_mod
from .lib import load

MUTATIONS_PER_SITE = 9
LENGTH_DIFFS = (0, 0, 0, 0, 1, 1, 1, 1, -1)


class DiploidSite:
    """ConsensusCore::DiploidSite (Diploid.hpp): the two alleles as column indices, the log Bayes factor and
    each read's allele (0 or 1).  Position is the template position when a scorer's DiploidSites made it."""

    def __init__(self, Allele0, Allele1, LogBayesFactor, AlleleForRead, Position=None):
        self.Allele0 = Allele0
        self.Allele1 = Allele1
        self.LogBayesFactor = LogBayesFactor
        self.AlleleForRead = list(AlleleForRead)
        self.Position = Position

    def __repr__(self):
        return (f"DiploidSite(Allele0={self.Allele0}, Allele1={self.Allele1}, LogBayesFactor={self.LogBayesFactor!r}, "
                f"AlleleForRead={self.AlleleForRead}, Position={self.Position})")

    def __eq__(self, o):
        return (self.Position, self.Allele0, self.Allele1, self.LogBayesFactor, self.AlleleForRead) == \
               (o.Position, o.Allele0, o.Allele1, o.LogBayesFactor, o.AlleleForRead)


def IsSiteHeterozygous(site_scores, log_prior_ratio):
    """DiploidSite* IsSiteHeterozygous(const float*, int dim1, int dim2, float logPriorRatio): None when the site
    is not heterozygous, else its DiploidSite.  site_scores: a 2-D float32 array (reads x 9)."""
    m = np.ascontiguousarray(site_scores, dtype=np.float32)
    if m.ndim != 2:
        raise ValueError("site_scores must be a 2-D array")
    is_het = ctypes.c_int()
    site = _lib_mod.CDiploidSite()
    afr = (ctypes.c_int * max(1, m.shape[0]))()
    _lib_mod.check(load().pbccs_is_site_heterozygous(
        m.ctypes.data_as(_lib_mod.PF), m.shape[0], m.shape[1], float(log_prior_ratio), ctypes.byref(is_het),
        ctypes.byref(site), afr))
    if not is_het.value:
        return None
    return DiploidSite(site.allele0, site.allele1, site.log_bayes_factor, afr[: m.shape[0]])


def site_scores(fn, handle, n_reads, tpl_len, begin, end):
    """The (sites, reads, 9) float32 tensor of [begin, end) through one of the *_site_scores calls."""
    if end is None:
        end = tpl_len
    begin, end = int(begin), int(end)
    cap = max(0, end - begin) * n_reads * MUTATIONS_PER_SITE
    out = np.zeros(max(1, cap), dtype=np.float32)
    n = ctypes.c_longlong()
    _lib_mod.check(fn(handle, begin, end, out.ctypes.data_as(_lib_mod.PF), cap, ctypes.byref(n)))
    return out[: n.value].reshape(end - begin, n_reads, MUTATIONS_PER_SITE)


def diploid_sites(fn, handle, n_reads, tpl_len, log_prior_ratio, begin, end, host_all, cap=None):
    """The heterozygous sites of [begin, end) through one of the *_diploid_sites calls, ascending by Position."""
    if end is None:
        end = tpl_len
    begin, end = int(begin), int(end)
    if cap is None:
        cap = max(1, end - begin)
    sites = (_lib_mod.CDiploidSite * max(1, cap))()
    afr = (ctypes.c_int * max(1, cap * n_reads))()
    n = ctypes.c_int()
    _lib_mod.check(fn(handle, begin, end, float(log_prior_ratio), 1 if host_all else 0, sites, cap, ctypes.byref(n),
                      afr))
    return [DiploidSite(sites[k].allele0, sites[k].allele1, sites[k].log_bayes_factor,
                        afr[k * n_reads: (k + 1) * n_reads], sites[k].position) for k in range(n.value)]

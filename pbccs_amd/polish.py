"""Batched ccs polish driver: pbccs' Consensus<>() from the scorer setup on (Consensus.h:436-552).

The POA draft, FilterReads and ExtractMappedRead (Consensus.h:223-325, 352-390) run before the boundary
(pbccs_amd.driver): it takes a draft plus mapped, extent-clipped reads per ZMW, exactly what Consensus.h
hands to ArrowMultiReadMutationScorer.  Thousands of ZMWs go to the GPU per call; results come back in input order.
"""
import ctypes
import math

from . import lib as L


class ConsensusSettings:
    """ConsensusSettings (include/pacbio/ccs/Consensus.h:86-111, defaults src/Consensus.cpp:46-54)."""

    def __init__(self, min_passes=3, min_length=10, min_zscore=-5.0, max_drop_fraction=0.34,
                 min_predicted_accuracy=0.90, score_diff=12.5, max_iterations=40, mutation_separation=10,
                 mutation_neighborhood=20, zmws_per_batch=0, directional=None):
        self.min_passes = min_passes
        self.min_length = min_length
        self.min_zscore = min_zscore
        self.max_drop_fraction = max_drop_fraction
        self.min_predicted_accuracy = min_predicted_accuracy
        self.score_diff = score_diff
        self.max_iterations = max_iterations
        self.mutation_separation = mutation_separation
        self.mutation_neighborhood = mutation_neighborhood
        self.zmws_per_batch = zmws_per_batch
        # ConsensusSettings::Directional (Consensus.h:94; the reference's option is commented out): None,
        # "discordant" or "always" -- what polish_zmws / polish_stream / driver.ccs_batch do when their own
        # `directional` keyword is not given
        self.directional = directional

    def _c(self):
        o = L.CPolishOptions()
        o.min_passes = self.min_passes
        o.min_length = self.min_length
        o.min_zscore = self.min_zscore
        o.max_drop_fraction = self.max_drop_fraction
        o.min_predicted_accuracy = self.min_predicted_accuracy
        o.score_diff = self.score_diff
        o.refine = L.CRefineOptions(self.max_iterations, self.mutation_separation, self.mutation_neighborhood)
        o.zmws_per_batch = self.zmws_per_batch
        return o


class _Marshalled:
    """pbccs_zmw_input / pbccs_zmw_output arrays for a list of ZMW dicts; the output buffers stay owned here."""

    def __init__(self, zmws):
        n = len(zmws)
        self.zmws = zmws
        self._ins = (L.CZmwInput * max(1, n))()
        self._outs = (L.CZmwOutput * max(1, n))()
        self._keep = []
        for i, z in enumerate(zmws):
            reads = z["reads"]
            nr = len(reads)
            draft = z["draft"].encode()
            # a read with no sequence is a placeholder the driver skipped (pbccs_amd.driver): not added, counted
            # in the drop fraction's denominator only
            seqs = (ctypes.c_char_p * max(1, nr))(*[None if r["seq"] is None else r["seq"].encode() for r in reads])
            lens = (ctypes.c_int * max(1, nr))(*[0 if r["seq"] is None else len(r["seq"]) for r in reads])
            strands = (ctypes.c_int * max(1, nr))(*[int(r.get("strand", 0)) for r in reads])
            ts = (ctypes.c_int * max(1, nr))(*[int(r.get("ts", 0)) for r in reads])
            te = (ctypes.c_int * max(1, nr))(*[int(r.get("te", len(z["draft"]))) for r in reads])
            fp = (ctypes.c_ubyte * max(1, nr))(*[1 if r.get("full_pass", True) else 0 for r in reads])
            cap = 2 * len(draft) + 64
            cons = ctypes.create_string_buffer(cap)
            qv = (ctypes.c_int * cap)()
            arr = (ctypes.c_int * max(1, nr))()
            zs = (ctypes.c_double * max(1, nr))()
            self._keep.append((draft, seqs, lens, strands, ts, te, fp, cons, qv, arr, zs))
            self._ins[i].draft = draft
            self._ins[i].draft_len = len(draft)
            for k in range(4):
                self._ins[i].snr[k] = float(z["snr"][k])
            self._ins[i].n_reads = nr
            self._ins[i].seqs = seqs
            self._ins[i].lens = lens
            self._ins[i].strands = strands
            self._ins[i].tstarts = ts
            self._ins[i].tends = te
            self._ins[i].full_pass = fp
            self._outs[i].consensus = ctypes.cast(cons, ctypes.c_char_p)
            self._outs[i].consensus_cap = cap
            self._outs[i].qvs = qv
            self._outs[i].add_read_results = arr
            self._outs[i].zscores = zs

    def results(self):
        from . import ZMW_STATUS
        res = []
        for i, z in enumerate(self.zmws):
            o = self._outs[i]
            nr = len(z["reads"])
            keep = self._keep[i]
            ln = max(0, o.consensus_len)
            ok = o.status in (0, 6)
            res.append({
                "status": ZMW_STATUS[o.status], "status_code": o.status,
                "consensus": keep[7].raw[:ln].decode() if ok else "",
                "qvs": list(keep[8][:ln]) if ok else [],
                "add_read_results": list(keep[9][:nr]), "zscores": list(keep[10][:nr]),
                "zg": o.zg, "za": o.za, "predicted_accuracy": o.predicted_accuracy, "n_tested": o.n_tested,
                "n_applied": o.n_applied, "n_passes": o.n_passes, "status_counts": list(o.status_counts),
            })
        return res


class PreparedBatch(_Marshalled):
    """ZMWs copied to HBM (pbccs_batch_create); polish() runs the hot path once (pbccs_batch_polish)."""

    def __init__(self, zmws, settings=None, engine=None):
        from . import default_engine
        import time
        self._lib = L.load()
        self.engine = engine or default_engine()
        self.settings = settings or ConsensusSettings()
        t0 = time.perf_counter()
        super().__init__(zmws)
        t1 = time.perf_counter()
        n = len(zmws)
        self._opts = self.settings._c()
        h = ctypes.c_void_p()
        L.check(L.load().pbccs_batch_create(self.engine._h, self._ins, n, ctypes.byref(self._opts), ctypes.byref(h)))
        self._h = h
        self.marshal_s = t1 - t0                     # Python dicts -> the boundary's C structs
        self.create_s = time.perf_counter() - t1     # pbccs_batch_create (per-ZMW setup + upload)

    def polish(self):
        L.check(L.load().pbccs_batch_polish(self._h, self._outs))

    def close(self):
        if getattr(self, "_h", None):
            self._lib.pbccs_batch_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()


def polish_many(batches):
    """Polish several PreparedBatches of one engine concurrently (pbccs_batch_polish_many)."""
    if not batches:
        return
    n = len(batches)
    hs = (ctypes.c_void_p * n)(*[b._h.value for b in batches])
    outs = (ctypes.POINTER(L.CZmwOutput) * n)(*[ctypes.cast(b._outs, ctypes.POINTER(L.CZmwOutput)) for b in batches])
    L.check(batches[0]._lib.pbccs_batch_polish_many(hs, n, outs))


def _rich_buffers(m):
    """RichBuffers for the ZMWs of a _Marshalled, each as large as the ZMW's consensus buffer."""
    from .richqv import RichBuffers
    return RichBuffers([o.consensus_cap for o in m._outs[:len(m.zmws)]])


def _add_rich(res, rb):
    """The five rich keys into the records; empty for a ZMW without a consensus."""
    for i, r in enumerate(res):
        r.update(rb.record(i))
    return res


def _polish_repeats(zmws, settings, engine, repeats, one_batch, rich_qvs=False, strand=None):
    """pbccs_polish_batch_ex: RefineConsensus, RefineRepeats(repeat_length, min_repeat_elements), ConsensusQVs per
    ZMW; the records gain n_repeat_tested / n_repeat_applied.  rich_qvs (with or without
    repeats): pbccs_polish_batch_ex2 with one pbccs_rich_qvs per ZMW.  strand (a pbccs_strand_options):
    pbccs_polish_batch_strand; the records gain strand_sites and, when split, fwd / rev."""
    from . import default_engine
    engine = engine or default_engine()
    settings = settings or ConsensusSettings()
    m = _Marshalled(zmws)
    n = len(zmws)
    opts = settings._c()
    if one_batch and opts.zmws_per_batch <= 0:
        opts.zmws_per_batch = max(1, n)   # polish_zmws: one device batch
    ro = rt = ra = None
    if repeats is not None:
        repeat_length, min_repeat_elements = repeats
        ro = L.CRepeatOptions(int(repeat_length), int(min_repeat_elements), 1, 10, 20)
        rt = (ctypes.c_longlong * max(1, n))()
        ra = (ctypes.c_longlong * max(1, n))()
    if strand is not None:
        from .strand import SiteBuffers
        x = L.CPolishExtras()
        if rich_qvs:
            rb = _rich_buffers(m)
            x = rb.extras(ro, rt, ra)
        elif ro is not None:
            x.repeats = ctypes.pointer(ro)
            x.repeat_tested = rt
            x.repeat_applied = ra
        sb = SiteBuffers([o.consensus_cap for o in m._outs[:n]], [len(z["reads"]) for z in zmws])
        L.check(L.load().pbccs_polish_batch_strand(engine._h, m._ins, n, ctypes.byref(opts), ctypes.byref(x),
                                                   ctypes.byref(strand), sb.arr, m._outs))
    elif rich_qvs:
        rb = _rich_buffers(m)
        x = rb.extras(ro, rt, ra)
        L.check(L.load().pbccs_polish_batch_ex2(engine._h, m._ins, n, ctypes.byref(opts), ctypes.byref(x), m._outs))
    else:
        L.check(L.load().pbccs_polish_batch_ex(engine._h, m._ins, n, ctypes.byref(opts), ctypes.byref(ro), rt, ra,
                                               m._outs))
    res = m.results()
    if repeats is not None:
        for i, r in enumerate(res):
            r["n_repeat_tested"] = rt[i]
            r["n_repeat_applied"] = ra[i]
    if strand is not None:
        for i, r in enumerate(res):
            r["strand_sites"] = sb.sites(i)
            r.update(sb.sub_records(i))
    return _add_rich(res, rb) if rich_qvs else res


def _strand_keywords(strand_sites, directional, settings=None):
    """The pbccs_strand_options of the batch keywords, or None when neither is given (settings.directional stands
    in for a `directional` that is not given)."""
    if directional is None and settings is not None:
        directional = getattr(settings, "directional", None)
    if not strand_sites and directional is None:
        return None
    from .strand import strand_options
    return strand_options(strand_sites, directional)


def polish_zmws(zmws, settings=None, engine=None, repeats=None, rich_qvs=False, strand_sites=False, directional=None):
    """Polish ZMWs on the GPU (upload, hot path, download).

    zmws: list of dicts {draft, snr (4), reads: [{seq, strand, ts, te, full_pass?}]}.
    Returns one dict per ZMW: status, consensus, qvs, add_read_results, zscores, zg, za, predicted_accuracy,
    n_tested, n_applied, n_passes, status_counts.
    repeats=(repeat_length, min_repeat_elements): RefineRepeats between RefineConsensus and ConsensusQVs
    (pbccs_polish_batch_ex); the records then also hold n_repeat_tested and n_repeat_applied.
    rich_qvs=True: the records also hold sub_qv, ins_qv, del_qv, sub_tag and ins_tag, the per-base rich QVs of the
    final template (pbccs_polish_batch_ex2; named by mutation type, see pbccs_amd.richqv).
    strand_sites=True (or a dict with any of min_score, min_reads, min_sites): the records also hold strand_sites,
    the StrandSite(pos, type, base, sum_fwd, sum_rev) list of the strand-discordance screen on the final template
    (pbccs_polish_batch_strand).  directional="discordant" | "always": the ZMWs with sites / all
    ZMWs are polished once more per strand, and their records hold "fwd" and "rev" sub-records, each what this
    call returns for the ZMW with only that strand's reads (per-read entries indexed like the joint record's, -1 /
    NaN for the other strand's reads).  Every other field is what the call without the keywords returns.
    """
    strand = _strand_keywords(strand_sites, directional, settings)
    if repeats is not None or rich_qvs or strand is not None:
        return _polish_repeats(zmws, settings, engine, repeats, True, rich_qvs, strand)
    b = PreparedBatch(zmws, settings, engine)
    try:
        b.polish()
        return b.results()
    finally:
        b.close()


WINDOW_FALLBACK = {0: None, 1: "window status", 2: "no join", 3: "predicted accuracy"}


def window_options(window=2000, overlap=200, guard=8, k=6):
    """pbccs_window_options; ValueError unless window > overlap >= 2 guard, guard >= 1 and 4 <= k <= 8."""
    window, overlap, guard, k = int(window), int(overlap), int(guard), int(k)
    if not (window > overlap and overlap >= 2 * guard and guard >= 1 and 4 <= k <= 8):
        raise ValueError("window options: need window > overlap >= 2 guard, guard >= 1, 4 <= k <= 8")
    return L.CWindowOptions(window, overlap, guard, k)


def window_plan(draft_len, window=2000, overlap=200):
    """The windows [(begin, end)] of a draft (pbccs_window_plan; host only, no device)."""
    wo = L.CWindowOptions(int(window), int(overlap), 1, 8)
    nw = ctypes.c_int()
    rc = L.load().pbccs_window_plan(int(draft_len), ctypes.byref(wo), None, 0, ctypes.byref(nw))
    if rc not in (L.PBCCS_OK, -5):
        L.check(rc)
    b = (ctypes.c_int * (2 * max(1, nw.value)))()
    L.check(L.load().pbccs_window_plan(int(draft_len), ctypes.byref(wo), b, nw.value, ctypes.byref(nw)))
    return [(b[2 * i], b[2 * i + 1]) for i in range(nw.value)]


def window_join(transcript_a, bounds_a, transcript_b, bounds_b, guard=8):
    """The join of two neighbouring windows from their draft-to-consensus transcripts (pbccs_window_join; host
    only): (p, cut_a, cut_b), or None when no candidate has 2 guard neighbouring M around it in both."""
    found, p, ca, cb = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    ta, tb = transcript_a.encode(), transcript_b.encode()
    L.check(L.load().pbccs_window_join(ta, len(ta), int(bounds_a[0]), int(bounds_a[1]), tb, len(tb), int(bounds_b[0]),
                                       int(bounds_b[1]), int(guard), ctypes.byref(found), ctypes.byref(p),
                                       ctypes.byref(ca), ctypes.byref(cb)))
    return (p.value, ca.value, cb.value) if found.value else None


def window_slices(zmws, window=2000, overlap=200, k=6, min_length=10, engine=None):
    """Where every read is cut at the window boundaries (pbccs_window_slices; the chains and the cuts run on the
    GPU).  Per ZMW: {"windows": [(begin, end)], "slices": per window a list with one entry per read -- None for a
    placeholder, else (begin, end, ts', te') with [begin, end) in the read's forward text --, "unanchored_reads"}."""
    from . import default_engine
    engine = engine or default_engine()
    wo = L.CWindowOptions(int(window), int(overlap), 1, int(k))
    m = _Marshalled(zmws)
    n = len(zmws)
    nw = (ctypes.c_int * max(1, n))()
    un = (ctypes.c_int * max(1, n))()
    need = ctypes.c_longlong()
    rc = L.load().pbccs_window_slices(engine._h, m._ins, n, ctypes.byref(wo), int(min_length), nw, None, 0,
                                      ctypes.byref(need), un)
    if rc not in (L.PBCCS_OK, -5):
        L.check(rc)
    buf = (ctypes.c_int * max(1, need.value))()
    L.check(L.load().pbccs_window_slices(engine._h, m._ins, n, ctypes.byref(wo), int(min_length), nw, buf, need.value,
                                         ctypes.byref(need), un))
    flat = list(buf[:need.value])
    out, at = [], 0
    for z, zm in enumerate(zmws):
        nr = len(zm["reads"])
        rows = []
        for _ in range(nw[z]):
            rows.append([None if flat[at + 4 * r] < 0 else tuple(flat[at + 4 * r:at + 4 * r + 4]) for r in range(nr)])
            at += 4 * nr
        out.append({"windows": window_plan(len(zm["draft"]), window, overlap), "slices": rows,
                    "unanchored_reads": un[z]})
    return out


def polish_windowed(zmws, settings=None, window=2000, overlap=200, guard=8, k=6, engine=None, rich_qvs=False,
                    strand_sites=False, directional=None):
    """Polish ZMWs with long drafts as overlapping windows (pbccs_polish_windowed).

    Results as polish_zmws plus "windowed" (the draft had more than one window), "fallback" (0, or the reason code
    the ZMW was polished whole for; WINDOW_FALLBACK names them), "unanchored_reads" and "windows": per window
    begin, end, join (the draft position it is joined to the next window at, -1 for none), cut_begin / cut_end
    (its piece of its own consensus), status, n_tested, n_applied.
    rich_qvs=True: the five rich keys too (pbccs_polish_windowed_ex); the stitched arrays are the same pieces of the
    windows' arrays as the stitched qvs.
    strand_sites / directional: not supported on windows; ValueError when given."""
    if strand_sites or directional is not None:
        raise ValueError("the strand screen and the directional polish do not run on the windowed polish")
    from . import default_engine
    engine = engine or default_engine()
    settings = settings or ConsensusSettings()
    wo = window_options(window, overlap, guard, k)
    m = _Marshalled(zmws)
    n = len(zmws)
    opts = settings._c()
    info = (L.CWindowInfo * max(1, n))()
    recs = []
    for i, z in enumerate(zmws):
        cap = len(window_plan(len(z["draft"]), window, overlap))
        recs.append((L.CWindowRecord * cap)())
        info[i].windows = recs[-1]
        info[i].windows_cap = cap
    if rich_qvs:
        rb = _rich_buffers(m)
        x = rb.extras()
        L.check(L.load().pbccs_polish_windowed_ex(engine._h, m._ins, n, ctypes.byref(opts), ctypes.byref(wo),
                                                  ctypes.byref(x), m._outs, info))
    else:
        L.check(L.load().pbccs_polish_windowed(engine._h, m._ins, n, ctypes.byref(opts), ctypes.byref(wo), m._outs,
                                               info))
    res = m.results()
    if rich_qvs:
        _add_rich(res, rb)
    for i, r in enumerate(res):
        r["windowed"] = info[i].n_windows > 1
        r["fallback"] = info[i].fallback
        r["unanchored_reads"] = info[i].unanchored_reads
        r["windows"] = [{"begin": w.begin, "end": w.end, "join": w.join, "cut_begin": w.cut_begin,
                         "cut_end": w.cut_end, "status": w.status, "n_tested": w.n_tested, "n_applied": w.n_applied}
                        for w in recs[i][:info[i].n_windows]]
    return res


def window_stats(engine=None, reset=False):
    """The windowed polish's work since the last reset (pbccs_window_stats_get)."""
    from . import default_engine
    engine = engine or default_engine()
    s = L.CWindowStats()
    L.check(L.load().pbccs_window_stats_get(engine._h, ctypes.byref(s), 1 if reset else 0))
    return {"zmws": s.zmws, "windows": s.windows, "fallbacks": list(s.fallbacks), "unanchored_reads": s.unanchored_reads,
            "cut_tasks": s.cut_tasks, "joints": s.joints, "launches": s.launches, "slices_ms": s.slices_ms,
            "polish_ms": s.polish_ms, "join_ms": s.join_ms, "fallback_ms": s.fallback_ms}


def plan_batches(zmws, budget_bytes, max_per_batch=2000, max_len_ratio=1.5):
    """The work queue's batch plan (pbccs_plan_batches; host only, no device).

    Returns (batches, est): batches = lists of ZMW indices, largest estimated band footprint first;
    est = per-ZMW estimated FP64 band bytes.
    """
    m = _Marshalled(zmws)
    n = len(zmws)
    order = (ctypes.c_int * max(1, n))()
    start = (ctypes.c_int * (n + 1))()
    est = (ctypes.c_double * max(1, n))()
    nb = ctypes.c_int()
    L.check(L.load().pbccs_plan_batches(m._ins, n, float(budget_bytes), int(max_per_batch), float(max_len_ratio),
                                        order, start, est, ctypes.byref(nb)))
    return [list(order[start[b]:start[b + 1]]) for b in range(nb.value)], list(est[:n])


def polish_stream(zmws, settings=None, engine=None, repeats=None, rich_qvs=False, strand_sites=False,
                  directional=None):
    """Polish a stream of heterogeneous ZMWs (pbccs_polish_batch): bucketed by length and pass count into
    memory-sized device batches that the engine's workspace slots pull largest-first from one queue, like
    ccs's ZMW work queue (src/main/ccs.cpp:222-262).  Results in input order, as polish_zmws(); `repeats`,
    `rich_qvs`, `strand_sites` and `directional` as there."""
    strand = _strand_keywords(strand_sites, directional, settings)
    if repeats is not None or rich_qvs or strand is not None:
        return _polish_repeats(zmws, settings, engine, repeats, False, rich_qvs, strand)
    from . import default_engine
    engine = engine or default_engine()
    settings = settings or ConsensusSettings()
    m = _Marshalled(zmws)
    opts = settings._c()
    L.check(L.load().pbccs_polish_batch(engine._h, m._ins, len(zmws), ctypes.byref(opts), m._outs))
    return m.results()

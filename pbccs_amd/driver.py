"""Per-ZMW driver steps on the host side of the boundary: FilterReads, the POA
step's bookkeeping and ExtractMappedRead of include/pacbio/ccs/Consensus.h, turning one ZMW's raw
subreads into the pbccs_zmw_input the GPU polish takes.

    chunk (subreads + SNR) --FilterReads--> ordered reads --POA--> draft + per-read extents
        --ExtractMappedRead--> mapped, extent-clipped reads --> polish boundary (pbccs_batch_*)

The POA itself is pluggable (`poa`: a callable with the SparsePoa contract, below).  The boundary keeps
the reference's bookkeeping: reads the POA did not take and reads ExtractMappedRead rejected are passed as
placeholders (no sequence), so they count in the drop fraction's denominator exactly as Consensus.h's
`nReads = readKeys.size()` does (:441-482).

Parity: no reference test exercises FilterReads / ExtractMappedRead directly; this restatement follows
the cited lines (float32 arithmetic where the reference uses float) and is checked by tests/test_driver.py
against hand-derived expectations -- parity unpinned by reference fixtures.
"""
import numpy as np

ADAPTER_BEFORE = 1
ADAPTER_AFTER = 2
FULL_PASS = ADAPTER_BEFORE | ADAPTER_AFTER


def _full(read):
    f = read.get("flags", FULL_PASS)
    return bool(f & ADAPTER_BEFORE) and bool(f & ADAPTER_AFTER)


def _median(lengths):
    """Median<size_t> (Consensus.h:213-221): the middle element, or 0.5 * (sum of the two middle ones) as
    double, returned as float."""
    v = sorted(lengths)
    n = len(v)
    if n % 2 == 1:
        return np.float32(v[n // 2])
    return np.float32(0.5 * (v[n // 2 - 1] + v[n // 2]))


def filter_reads(reads, min_length):
    """FilterReads (include/pacbio/ccs/Consensus.h:223-292).

    reads: dicts with "seq" and "flags" (LocalContextFlags; default a full pass).  Returns the reads in the
    reference's priority order -- full passes first by closeness of their length to the median full-pass
    length, then the others by the same closeness -- with None for reads of at least twice the median
    length, which sort last.  An empty list when no read can be used (median shorter than min_length)."""
    if not reads:
        return []
    longest = 0
    lengths = []
    for r in reads:
        longest = max(longest, len(r["seq"]))
        if _full(r):
            lengths.append(len(r["seq"]))
    median = np.float32(longest) if not lengths else _median(lengths)
    max_len = 2 * int(median)                 # 2 * static_cast<size_t>(median)
    if median < np.float32(min_length):
        return []
    results = [r if len(r["seq"]) < max_len else None for r in reads]

    def lex(r):
        with np.errstate(divide="ignore", invalid="ignore"):
            l = np.float32(len(r["seq"]))
            v = min(l / median, median / l)   # float arithmetic (:271-272)
        return (v, np.float32(0.0)) if _full(r) else (np.float32(0.0), v)

    # std::stable_sort with "lhs > rhs", nullptr last (:281-289): non-null reads by descending key, ties
    # in input order; Python's sort is stable, so sort on the negated key
    kept = [r for r in results if r is not None]
    kept.sort(key=lambda r: tuple(-x for x in lex(r)))
    return kept + [None] * (len(results) - len(kept))


def extract_mapped_read(read, summary, min_length):
    """ExtractMappedRead (Consensus.h:294-325).  summary: {"rc": bool, "read": (l, r), "tpl": (l, r)}
    (PoaAlignmentSummary: ReverseComplementedRead, ExtentOnRead, ExtentOnConsensus).  Returns the mapped
    read as the polish boundary takes it, or None when the extent on the read is shorter than min_length.
    Quirk: the substring is taken from the read as given, even when the POA
    added it reverse-complemented and the extent is in the reverse complement's coordinates."""
    rs, re_ = summary["read"]
    ts, te = summary["tpl"]
    if rs > re_ or re_ - rs < min_length:
        return None
    return {"seq": read["seq"][rs:re_], "strand": 1 if summary["rc"] else 0, "ts": int(ts), "te": int(te),
            "full_pass": _full(read)}


def poa_inputs(reads, poa, max_poa_coverage=None):
    """PoaConsensus (Consensus.h:352-390): feed the filtered reads to the POA in order (None -> key -1) until
    max_poa_coverage reads were added, then take the consensus with minCoverage = 1 below 5 reads, else
    (cov + 1) / 2 - 1.

    poa: an object with the SparsePoa surface -- orient_and_add_read(seq) -> key (>= 0, or -1 when the read
    could not be added) and find_consensus(min_coverage) -> (sequence, summaries by key).
    Returns (draft, read_keys, summaries)."""
    keys = []
    cov = 0
    for r in reads:
        key = -1 if r is None else poa.orient_and_add_read(r["seq"])
        keys.append(key)
        if key >= 0:
            cov += 1
            if max_poa_coverage is not None and cov >= max_poa_coverage:
                break
    min_cov = 1 if cov < 5 else (cov + 1) // 2 - 1
    draft, summaries = poa.find_consensus(min_cov)
    return draft, keys, summaries


_PLACEHOLDER = {"seq": None, "strand": 0, "ts": 0, "te": 0, "full_pass": False}


def _past_cap(rest, summaries, min_length):
    """The entries of FilterReads' order the maxPoaCov stop never reached, with the summary ({"rc", "read",
    "tpl"}, or None) the mapping onto the finished draft gave each.  A dropped read (None) and an unmapped one
    become placeholders, as reads the POA rejected do."""
    out = []
    for r, sm in zip(rest, summaries):
        mr = extract_mapped_read(r, sm, min_length) if r is not None and sm is not None else None
        out.append(mr if mr is not None else dict(_PLACEHOLDER))
    return out


def dropped_reads(reads, min_length):
    """(index, read) of the reads filter_reads sets to None (at least twice the median full-pass length), in input
    order: the k-th None of filter_reads' order stands for the k-th of them."""
    order = filter_reads(reads, min_length)
    kept = {id(r) for r in order if r is not None}
    return [(k, r) for k, r in enumerate(reads) if id(r) not in kept] if order else []


def split_options(split_long_reads):
    """(jump_penalty or None, max_segments) of the split_long_reads keyword: True, or a dict with any of
    "jump_penalty" and "max_segments"."""
    opts = {} if split_long_reads is True else split_long_reads
    if not isinstance(opts, dict) or set(opts) - {"jump_penalty", "max_segments"}:
        raise ValueError('split_long_reads: False, True, or a dict with any of "jump_penalty", "max_segments"')
    return opts.get("jump_penalty"), int(opts.get("max_segments", 8))


def split_read(read, chain, min_length):
    """A read FilterReads dropped and its split mapping (mapping.split_map_to_draft's entry) -> the polish reads of
    a missed-adapter read, or None when it is not accepted as one.  Accepted: not truncated, at least two segments,
    consecutive segments on alternating strands, at least two segments of min_length read bases.  Each such segment
    becomes {"seq", "strand", "ts", "te", "full_pass", "segment"} in read order, its sequence cut from the read as
    given in the read's own coordinates (no Appendix A.15 quirk).  Interior segments are full passes; the first
    needs the read's ADAPTER_BEFORE, the last its ADAPTER_AFTER."""
    if chain is None or chain["truncated"] or len(chain["segments"]) < 2:
        return None
    segs = chain["segments"]
    if any(a["rc"] == b["rc"] for a, b in zip(segs, segs[1:])):
        return None
    flags = read.get("flags", FULL_PASS)
    out = []
    for k, sg in enumerate(segs):
        b, e = sg["read"]
        if e - b < min_length:
            continue
        full = (k > 0 or bool(flags & ADAPTER_BEFORE)) and (k + 1 < len(segs) or bool(flags & ADAPTER_AFTER))
        out.append({"seq": read["seq"][b:e], "strand": 1 if sg["rc"] else 0, "ts": int(sg["tpl"][0]),
                    "te": int(sg["tpl"][1]), "full_pass": full, "segment": dict(sg)})
    return out if len(out) >= 2 else None


def _apply_splits(zmw, slots, dropped, chains, min_length):
    """Replaces, in place, the placeholder of every accepted missed-adapter read by its segments' polish reads.
    slots: positions in zmw["reads"] of the dropped reads' placeholders, in order; dropped: dropped_reads();
    chains: one split mapping per dropped read.  Records the accepted reads in zmw["split_reads"] ("segments": the
    ones that became reads, "n_segments": the chain's count)."""
    reads, split = [], []
    at = {pos: k for k, pos in enumerate(slots)}
    for pos, r in enumerate(zmw["reads"]):
        k = at.get(pos)
        got = split_read(dropped[k][1], chains[k], min_length) if k is not None and k < len(dropped) else None
        if got is None:
            reads.append(r)
            continue
        split.append({"subread": dropped[k][0], "first": len(reads), "n_segments": chains[k]["n_segments"],
                      "segments": [g.pop("segment") for g in got]})
        reads += got
    zmw["reads"] = reads
    zmw["split_reads"] = split
    zmw["n_missed_adapters"] = sum(s["n_segments"] - 1 for s in split)


def zmw_input(chunk, poa, min_length=10, max_poa_coverage=None, mapper=None, split_mapper=None):
    """One ZMW's subreads -> the polish boundary's ZMW dict, or (status, None) when the ZMW ends before the
    scorer: NoSubreads (Consensus.h:414-420) or TooShort (:427-434).

    chunk: {"snr": 4 floats, "reads": [{"seq", "flags"}]}.  Returns (None, zmw) on success, where zmw is
    {"draft", "snr", "reads"} and reads holds one entry per POA key in order: the mapped read, or a
    placeholder {"seq": None} for a read the POA or ExtractMappedRead skipped.
    mapper (optional, a callable with mapping.map_to_draft's contract): the reads past max_poa_coverage are
    placed on the draft with it and follow the POA's reads, one entry per read of FilterReads' order.
    split_mapper (optional, a callable (draft, reads) with mapping.split_map_to_draft's results): every read
    FilterReads dropped is split-mapped onto the draft, and one accepted as a missed-adapter read (split_read) has
    its placeholder replaced in place by its segments' reads; zmw then also holds "split_reads" ([{"subread",
    "first", "segments"}], first being the position of its first read) and "n_missed_adapters"."""
    reads = filter_reads(chunk["reads"], min_length)
    if not reads or all(r is None for r in reads):
        return "NoSubreads", None
    draft, keys, summaries = poa_inputs(reads, poa, max_poa_coverage)
    if len(draft) < min_length:
        return "TooShort", None
    out = []
    for i, key in enumerate(keys):
        mr = extract_mapped_read(reads[i], summaries[key], min_length) if key >= 0 else None
        out.append(mr if mr is not None else {"seq": None, "strand": 0, "ts": 0, "te": 0, "full_pass": False})
    if mapper is not None:
        rest = reads[len(keys):]
        summ = iter(mapper(draft, [r["seq"] for r in rest if r is not None]) if any(r is not None for r in rest) else [])
        out += _past_cap(rest, [None if r is None else next(summ) for r in rest], min_length)
    zmw = {"draft": draft, "snr": list(chunk["snr"]), "reads": out}
    if split_mapper is not None:
        dropped = dropped_reads(chunk["reads"], min_length)
        slots = [i for i, r in enumerate(reads[:len(out)]) if r is None]
        _apply_splits(zmw, slots, dropped, split_mapper(draft, [r["seq"] for _, r in dropped]) if slots else [],
                      min_length)
    return None, zmw


def zmw_inputs_batch(chunks, min_length=10, max_poa_coverage=None, engine=None, map_past_cap=False,
                     banded_poa=False, split_long_reads=False):
    """zmw_input for many ZMWs at once, with the POA of all of them on the GPU in one pbccs_poa_batch
    (every ZMW adds its next subread in the same device round).  Returns [(status, zmw)] as zmw_input.
    map_past_cap: the reads past max_poa_coverage of all ZMWs are placed on their drafts in one pbccs_map_batch.
    banded_poa: the POA fills inside SdpRangeFinder's ranges (poa.poa_batch(banded=True)).
    split_long_reads (False, True, or {"jump_penalty", "max_segments"}): the reads FilterReads dropped of all ZMWs
    are split-mapped onto their drafts in one pbccs_split_map_batch, as zmw_input's split_mapper."""
    from . import poa as _poa
    filtered = [filter_reads(c["reads"], min_length) for c in chunks]
    idx = [z for z, rs in enumerate(filtered) if rs and not all(r is None for r in rs)]
    out = [("NoSubreads", None)] * len(chunks)
    res = _poa.poa_batch([[None if r is None else r["seq"] for r in filtered[z]] for z in idx],
                         max_coverage=max_poa_coverage, engine=engine, banded=banded_poa)
    past = {}
    if map_past_cap:
        from . import mapping as _mapping
        todo = [(z, r) for z, r in zip(idx, res) if len(r["consensus"]) >= max(1, min_length) and -2 in r["keys"]]
        got = _mapping.map_batch([(r["consensus"], [None if x is None else x["seq"]
                                                    for x in filtered[z][r["keys"].index(-2):]]) for z, r in todo],
                                 engine=engine)
        past = {z: g for (z, _), g in zip(todo, got)}
    for z, r in zip(idx, res):
        draft = r["consensus"]
        if len(draft) < min_length:
            out[z] = ("TooShort", None)
            continue
        reads = []
        for i, key in enumerate(r["keys"]):
            if key == -2:
                # past maxPoaCov: Consensus.h's loop stopped before this read
                if z in past:
                    reads += _past_cap(filtered[z][i:], past[z], min_length)
                break
            mr = extract_mapped_read(filtered[z][i], r["summaries"][key], min_length) if key >= 0 else None
            reads.append(mr if mr is not None else {"seq": None, "strand": 0, "ts": 0, "te": 0, "full_pass": False})
        out[z] = (None, {"draft": draft, "snr": list(chunks[z]["snr"]), "reads": reads})
    if split_long_reads:
        from . import mapping as _mapping
        jump, max_seg = split_options(split_long_reads)
        todo = []
        for z in idx:
            if out[z][1] is None:
                continue
            slots = [i for i, r in enumerate(filtered[z][:len(out[z][1]["reads"])]) if r is None]
            dropped = dropped_reads(chunks[z]["reads"], min_length)
            # a read or draft the mapper cannot take (map::kMaxLen) stays the placeholder it is
            ok = len(out[z][1]["draft"]) <= 65535
            todo.append((z, slots, dropped, [r["seq"] if ok and len(r["seq"]) <= 65535 else None for _, r in dropped]
                         if slots else []))
        got = _mapping.split_map_batch([(out[z][1]["draft"], seqs) for z, _, _, seqs in todo], jump, max_seg,
                                       engine=engine)
        for (z, slots, dropped, _), chains in zip(todo, got):
            _apply_splits(out[z][1], slots, dropped, chains, min_length)
    return out


def ccs_batch(chunks, settings=None, engine=None, max_poa_coverage=None, map_past_cap=False, banded_poa=False,
              polish_window=None, rich_qvs=False, kinetics=False, strand_sites=False, directional=None,
              pileup=False, split_long_reads=False, barcodes=None):
    """Consensus.h's per-ZMW driver for many ZMWs in one native call (pbccs_ccs_batch): FilterReads,
    the GPU POA, TooShort, ExtractMappedRead and the GPU polish, with no Python between the stages.
    chunks: [{"snr", "reads": [{"seq", "flags"?}]}].  Returns per ZMW the polish result dict (as
    polish_zmws) plus "draft"; add_read_results / zscores hold one entry per input subread, in the
    chunk's read order: -1 / NaN for a read that never reached AddRead (dropped by FilterReads, not added
    by the POA, rejected by ExtractMappedRead, past the maxPoaCov stop, or the ZMW ended earlier).
    "add_order" lists the subread indices in AddRead order (FilterReads' stable order, Consensus.h:281):
    the order of ZScores() and of the ccs.bam zs tag.
    map_past_cap (pbccs_ccs_batch_ex): the reads past the maxPoaCov stop are placed on the draft on the GPU
    (mapping.map_to_draft's aligner) and reach AddRead like the POA's reads, in FilterReads' order.
    banded_poa (pbccs_ccs_batch_ex2): the draft's alignments are filled inside SdpRangeFinder's ranges
    (poa.poa_batch(banded=True)); everything after the draft is unchanged.
    polish_window (pbccs_ccs_batch_ex3): None, or the windowed polish's options as a dict with any of window,
    overlap, guard, k (polish.polish_windowed's defaults for the rest): drafts longer than window + overlap are
    polished in overlapping windows and stitched.  The results then also carry "n_windows", "windowed" and
    "fallback" (polish.WINDOW_FALLBACK names the codes).
    rich_qvs (pbccs_ccs_batch_ex4): the results also carry sub_qv, ins_qv, del_qv, sub_tag and ins_tag, the per-base
    rich QVs of the consensus (pbccs_amd.richqv), as polish_zmws(..., rich_qvs=True) gives them.
    kinetics (pbccs_kinetics_batch, after the native call): every ZMW that ended Success or PoorQuality also
    carries the consensus kinetics of pbccs_amd.kinetics -- fwd_ipd, fwd_pw, rev_ipd, rev_pw
    (CodecV1 codes), the same names with _mean and _cov, fn and rn -- from its final consensus and those subreads,
    whole and with their "ip" / "pw" tracks, whose add_read_results entry is SUCCESS.  A chunk whose reads carry
    no tracks raises before any device work.
    strand_sites / directional (pbccs_ccs_batch_strand): as polish_zmws' keywords -- the results also
    carry strand_sites and, for the ZMWs polished once more per strand, the "fwd" and "rev" sub-records, their
    add_read_results / zscores indexed by input subread like the joint record's.  Not with polish_window (ValueError).
    pileup (pbccs_pileup_batch, after the native call): True, or a dict with any of "msa", "transcripts", "arrays"
    (booleans) and "band": every ZMW that ended Success or PoorQuality also carries "pileup", what pbccs_amd.pileup.pileup_batch
    returns for its final consensus and the subreads whose add_read_results entry is SUCCESS (with
    "msa" the gapped rows too, with "transcripts" each read's transcript, with "arrays" numpy arrays instead of nested
    lists, which is much cheaper for large calls), and "ec", the effective coverage.  The
    pileup's arrays run in the consensus's direction for both strands, unlike the kinetics arrays.  With kinetics
    and pileup together the reads are placed and aligned once, in one native call for both.
    split_long_reads (pbccs_ccs_batch_split): False, True, or a dict with any of "jump_penalty" and
    "max_segments".  Every subread FilterReads dropped for its length is split-mapped onto the draft; one that is a
    chain of at least two segments on alternating strands (not truncated, two of them at least min_length long) is
    taken for a read fused across a missed adapter, and its segments reach AddRead in its place, last, in read order.
    The results then also carry "split_reads": [{"subread", "segments": [{"rc", "read", "tpl", "score", "full_pass",
    "add_read_result", "zscore"}]}] and "n_missed_adapters" (the sum of the chains' segments - 1); the subread's
    own add_read_results / zscores entries stay -1 / NaN (so kinetics and pileup leave it out), and "add_order"
    repeats its index once per added segment.  Not with polish_window, strand_sites or directional (ValueError).
    barcodes (pbccs_ccs_batch_demux, or pbccs_demux_batch after the native call of the other options; DESIGN.md
    §3.27): None, a demux.BarcodeSet, or a dict with "barcodes" and any of demux.demux_batch's keywords (params,
    design, window, window_mult, min_quality, min_score_lead).  Every ZMW that ended Success also carries "barcode",
    what demux.demux_batch returns for its consensus; all of them are demultiplexed in one native call.  A bad set
    or option raises before any device work.
    Raises on a draft longer than its buffer (PBCCS_ERANGE).

    Marshalling is flat, as poa.poa_batch's: every subread in one buffer behind one pointer table, every
    output in shared arrays, the per-ZMW structs written column-wise through numpy views (per-ZMW ctypes
    arrays were ~3 s of Python per 10,000 ZMWs, half the ccs stage's wall time)."""
    import ctypes
    from . import ZMW_STATUS, default_engine
    from . import lib as L
    from .polish import ConsensusSettings
    from .quiver import _struct_dtype
    strand = None
    split = None
    if split_long_reads:
        if polish_window is not None or strand_sites or directional is not None:
            raise ValueError("split_long_reads does not run with polish_window, strand_sites or directional")
        split = split_options(split_long_reads)
    if directional is None and settings is not None:
        directional = getattr(settings, "directional", None)
    if strand_sites or directional is not None:
        if polish_window is not None:
            raise ValueError("the strand screen and the directional polish do not run on the windowed polish")
        from .strand import strand_options
        strand = strand_options(strand_sites, directional)
    if kinetics:   # before any engine is touched
        for z, c in enumerate(chunks):
            if c["reads"] and not any(r.get("ip") is not None or r.get("pw") is not None for r in c["reads"]):
                raise ValueError(f"ccs_batch(kinetics=True): the reads of chunk {z} carry no ip / pw tracks")
    pile_opts = None
    if pileup:   # before any engine is touched
        pile_opts = {} if pileup is True else pileup
        if not isinstance(pile_opts, dict) or set(pile_opts) - {"msa", "transcripts", "band", "arrays"}:
            raise ValueError('ccs_batch(pileup=...): True, or a dict with any of "msa", "transcripts", "band", "arrays"')
    demux_spec = demux_native = None
    if barcodes is not None:   # before any engine is touched
        from .demux import demux_options
        demux_spec = demux_options(barcodes)
    eng = engine or default_engine()
    settings = settings or ConsensusSettings()
    n = len(chunks)
    counts = np.fromiter((len(c["reads"]) for c in chunks), dtype=np.int64, count=n)
    flat = [r for c in chunks for r in c["reads"]]
    nr_all = len(flat)
    seqs = [r["seq"] for r in flat]
    joined = "".join(seqs).encode()   # one encode: per-read lengths in characters are bytes for ACGT text
    lens = np.fromiter(map(len, seqs), dtype=np.int32, count=nr_all)
    if len(joined) != int(lens.sum()):   # non-ASCII text: lengths in bytes, read by read
        enc = [s.encode() for s in seqs]
        joined = b"".join(enc)
        lens = np.fromiter(map(len, enc), dtype=np.int32, count=nr_all)
    flags = np.fromiter((int(r.get("flags", FULL_PASS)) for r in flat), dtype=np.uint8, count=nr_all)
    bases = np.zeros(nr_all + 1, dtype=np.int64)
    np.cumsum(lens, out=bases[1:])
    blob = np.frombuffer(joined, dtype=np.uint8) if joined else np.zeros(1, dtype=np.uint8)   # read-only view
    ptrs = (blob.ctypes.data + bases[:-1]).astype(np.uint64)
    first = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(counts, out=first[1:])
    f0 = first[:-1]
    # a POA consensus never exceeds the bases of the reads it was built from: per-ZMW capacity read bases + 64
    caps = bases[first[1:]] - bases[f0] + 64
    cstart = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(caps, out=cstart[1:])
    cons = np.zeros(max(1, int(cstart[-1])), dtype=np.uint8)     # calloc'd: pages past a draft's length untouched
    draft = np.zeros(max(1, int(cstart[-1])), dtype=np.uint8)
    qv = np.zeros(max(1, int(cstart[-1])), dtype=np.int32)
    arr = np.zeros(max(1, nr_all), dtype=np.int32)
    zs = np.zeros(max(1, nr_all), dtype=np.float64)
    order = np.zeros(max(1, nr_all), dtype=np.int32)
    ins = np.zeros(max(1, n), dtype=_struct_dtype(L.CCcsInput))
    outs = np.zeros(max(1, n), dtype=_struct_dtype(L.CCcsOutput))
    if n:
        ins["snr"][:n] = np.array([[float(v) for v in c["snr"][:4]] for c in chunks], dtype=np.float64)
        ins["n_subreads"][:n] = counts
        ins["seqs"][:n] = ptrs.ctypes.data + 8 * f0
        ins["lens"][:n] = lens.ctypes.data + 4 * f0
        ins["flags"][:n] = flags.ctypes.data + f0
        pol = outs["polish"]
        pol["consensus"][:n] = cons.ctypes.data + cstart[:-1]
        pol["consensus_cap"][:n] = caps
        pol["qvs"][:n] = qv.ctypes.data + 4 * cstart[:-1]
        pol["add_read_results"][:n] = arr.ctypes.data + 4 * f0
        pol["zscores"][:n] = zs.ctypes.data + 8 * f0
        outs["draft"][:n] = draft.ctypes.data + cstart[:-1]
        outs["draft_cap"][:n] = caps
        outs["add_order"][:n] = order.ctypes.data + 4 * f0
    opts = settings._c()
    mc = 2**62 if max_poa_coverage is None else int(max_poa_coverage)
    winfo = None
    rich = None
    sb = None
    if rich_qvs:   # one pbccs_rich_qvs per ZMW over shared arrays laid out like qv
        total = max(1, int(cstart[-1]))
        rich_qv = np.zeros((3, total), dtype=np.int32)
        rich_tag = np.zeros((2, total), dtype=np.uint8)
        rich = np.zeros(max(1, n), dtype=_struct_dtype(L.CRichQvs))
        if n:
            for row, key in enumerate(("sub_qv", "ins_qv", "del_qv")):
                rich[key][:n] = rich_qv[row].ctypes.data + 4 * cstart[:-1]
            for row, key in enumerate(("sub_tag", "ins_tag")):
                rich[key][:n] = rich_tag[row].ctypes.data + cstart[:-1]
            rich["cap"][:n] = caps
        x = L.CPolishExtras()
        x.rich = ctypes.cast(rich.ctypes.data, ctypes.POINTER(L.CRichQvs))
    if split is not None:
        x = x if rich_qvs else L.CPolishExtras()
        jump, max_seg = split
        if not 1 <= max_seg <= 64 or (jump is not None and jump < 0):
            raise ValueError("split_long_reads: jump_penalty >= 0 and 1 <= max_segments <= 64")
        so = L.CSplitOptions(-1 if jump is None else int(jump), max_seg)
        scap = counts * max_seg                        # segments per ZMW: every subread split max_seg ways
        sfirst = np.zeros(n + 1, dtype=np.int64)
        np.cumsum(scap, out=sfirst[1:])
        stot = max(1, int(sfirst[-1]))
        s_sub, s_seg = np.zeros(stot, dtype=np.int32), np.zeros(6 * stot, dtype=np.int32)
        s_full, s_arr = np.zeros(stot, dtype=np.uint8), np.zeros(stot, dtype=np.int32)
        s_zs, s_order = np.zeros(stot, dtype=np.float64), np.zeros(stot + max(1, nr_all), dtype=np.int32)
        souts = np.zeros(max(1, n), dtype=_struct_dtype(L.CCcsSplitOutput))
        if n:
            s0 = sfirst[:-1]
            souts["cap"][:n] = scap
            souts["subread"][:n] = s_sub.ctypes.data + 4 * s0
            souts["segments"][:n] = s_seg.ctypes.data + 24 * s0
            souts["full_pass"][:n] = s_full.ctypes.data + s0
            souts["add_read_results"][:n] = s_arr.ctypes.data + 4 * s0
            souts["zscores"][:n] = s_zs.ctypes.data + 8 * s0
            souts["add_order"][:n] = s_order.ctypes.data + 4 * (s0 + f0)
        co = L.CCcsOptions(mc, 1 if map_past_cap else 0)
        po = L.CPoaOptions(mc, -1, 1 if banded_poa else 0)
        L.check(L.load().pbccs_ccs_batch_split(eng._h, ctypes.cast(ins.ctypes.data, ctypes.POINTER(L.CCcsInput)), n,
                                               ctypes.byref(co), ctypes.byref(po), ctypes.byref(opts), ctypes.byref(x),
                                               ctypes.byref(so),
                                               ctypes.cast(souts.ctypes.data, ctypes.POINTER(L.CCcsSplitOutput)),
                                               ctypes.cast(outs.ctypes.data, ctypes.POINTER(L.CCcsOutput))))
    elif strand is not None:
        from .strand import SiteBuffers
        x = x if rich_qvs else L.CPolishExtras()
        sb = SiteBuffers(caps.tolist(), counts.tolist())
        co = L.CCcsOptions(mc, 1 if map_past_cap else 0)
        po = L.CPoaOptions(mc, -1, 1 if banded_poa else 0)
        L.check(L.load().pbccs_ccs_batch_strand(eng._h, ctypes.cast(ins.ctypes.data, ctypes.POINTER(L.CCcsInput)), n,
                                                ctypes.byref(co), ctypes.byref(po), ctypes.byref(opts), ctypes.byref(x),
                                                ctypes.byref(strand), sb.arr,
                                                ctypes.cast(outs.ctypes.data, ctypes.POINTER(L.CCcsOutput))))
    elif rich_qvs:
        wo = None
        if polish_window is not None:
            from .polish import window_options
            wo = window_options(**dict(polish_window))
            winfo = (L.CWindowInfo * max(1, n))()
        co = L.CCcsOptions(mc, 1 if map_past_cap else 0)
        po = L.CPoaOptions(mc, -1, 1 if banded_poa else 0)
        L.check(L.load().pbccs_ccs_batch_ex4(eng._h, ctypes.cast(ins.ctypes.data, ctypes.POINTER(L.CCcsInput)), n,
                                             ctypes.byref(co), ctypes.byref(po),
                                             ctypes.byref(wo) if wo is not None else None, ctypes.byref(opts),
                                             ctypes.byref(x), ctypes.cast(outs.ctypes.data, ctypes.POINTER(L.CCcsOutput)),
                                             winfo))
    elif polish_window is not None:
        from .polish import window_options
        wo = window_options(**dict(polish_window))
        winfo = (L.CWindowInfo * max(1, n))()
        co = L.CCcsOptions(mc, 1 if map_past_cap else 0)
        po = L.CPoaOptions(mc, -1, 1 if banded_poa else 0)
        L.check(L.load().pbccs_ccs_batch_ex3(eng._h, ctypes.cast(ins.ctypes.data, ctypes.POINTER(L.CCcsInput)), n,
                                             ctypes.byref(co), ctypes.byref(po), ctypes.byref(wo), ctypes.byref(opts),
                                             ctypes.cast(outs.ctypes.data, ctypes.POINTER(L.CCcsOutput)), winfo))
    elif banded_poa:
        co = L.CCcsOptions(mc, 1 if map_past_cap else 0)
        po = L.CPoaOptions(mc, -1, 1)
        L.check(L.load().pbccs_ccs_batch_ex2(eng._h, ctypes.cast(ins.ctypes.data, ctypes.POINTER(L.CCcsInput)), n,
                                             ctypes.byref(co), ctypes.byref(po), ctypes.byref(opts),
                                             ctypes.cast(outs.ctypes.data, ctypes.POINTER(L.CCcsOutput))))
    elif map_past_cap:
        co = L.CCcsOptions(mc, 1)
        L.check(L.load().pbccs_ccs_batch_ex(eng._h, ctypes.cast(ins.ctypes.data, ctypes.POINTER(L.CCcsInput)), n,
                                            ctypes.byref(co), ctypes.byref(opts),
                                            ctypes.cast(outs.ctypes.data, ctypes.POINTER(L.CCcsOutput))))
    elif demux_spec is not None:   # the plain call and the demultiplexing of its Success consensuses, natively
        from . import demux as _demux
        dout, darrs = _demux._outputs(n)
        dmask = np.zeros(max(1, n), dtype=np.int32)
        bset, keep = demux_spec[0]._c()
        L.check(L.load().pbccs_ccs_batch_demux(eng._h, ctypes.cast(ins.ctypes.data, ctypes.POINTER(L.CCcsInput)), n,
                                               mc, ctypes.byref(opts), ctypes.byref(bset),
                                               ctypes.byref(demux_spec[2]),
                                               ctypes.cast(outs.ctypes.data, ctypes.POINTER(L.CCcsOutput)),
                                               ctypes.byref(dout),
                                               ctypes.cast(dmask.ctypes.data, ctypes.POINTER(ctypes.c_int))))
        del keep
        demux_native = (_demux._entries(n, darrs), dmask.tolist())
    else:
        L.check(L.load().pbccs_ccs_batch(eng._h, ctypes.cast(ins.ctypes.data, ctypes.POINTER(L.CCcsInput)), n, mc,
                                         ctypes.byref(opts),
                                         ctypes.cast(outs.ctypes.data, ctypes.POINTER(L.CCcsOutput))))
    del blob, joined, ptrs, lens, flags   # the inputs lived until the call returned
    pol = outs["polish"]
    status, clen = pol["status"][:n].tolist(), pol["consensus_len"][:n].tolist()
    zg, za, pacc = pol["zg"][:n].tolist(), pol["za"][:n].tolist(), pol["predicted_accuracy"][:n].tolist()
    ntest, nappl, npass = pol["n_tested"][:n].tolist(), pol["n_applied"][:n].tolist(), pol["n_passes"][:n].tolist()
    scounts, dlen = pol["status_counts"][:n].tolist(), outs["draft_len"][:n].tolist()
    cs, fs, cnt = cstart.tolist(), first.tolist(), counts.tolist()
    arr_l, zs_l, order_l = arr.tolist(), zs.tolist(), order.tolist()
    res = []
    for z in range(n):
        st, c, f, nr = status[z], cs[z], fs[z], cnt[z]
        ok = st in (0, 6)
        ln = max(0, clen[z]) if ok else 0
        res.append({"status": ZMW_STATUS[st], "status_code": st,
                    "consensus": cons[c:c + ln].tobytes().decode() if ok else "",
                    "qvs": qv[c:c + ln].tolist() if ok else [],
                    "draft": draft[c:c + max(0, dlen[z])].tobytes().decode(),
                    "add_read_results": arr_l[f:f + nr], "zscores": zs_l[f:f + nr],
                    "polished": st not in (1, 2),   # NoSubreads / TooShort end before the polish
                    "add_order": [k for k in order_l[f:f + nr] if k >= 0],
                    "zg": zg[z], "za": za[z], "predicted_accuracy": pacc[z], "n_tested": ntest[z],
                    "n_applied": nappl[z], "n_passes": npass[z], "status_counts": scounts[z]})
        if winfo is not None:
            res[-1].update(n_windows=winfo[z].n_windows, windowed=winfo[z].n_windows > 1, fallback=winfo[z].fallback)
        if rich is not None:
            rl = int(rich["len"][z])
            if rl < 0:
                raise L.PbccsError(-5, "rich QVs outgrew their buffers")
            res[-1].update(sub_qv=rich_qv[0, c:c + rl].tolist(), ins_qv=rich_qv[1, c:c + rl].tolist(),
                           del_qv=rich_qv[2, c:c + rl].tolist(), sub_tag=rich_tag[0, c:c + rl].tobytes().decode(),
                           ins_tag=rich_tag[1, c:c + rl].tobytes().decode())
        if sb is not None:
            res[-1]["strand_sites"] = sb.sites(z)
            res[-1].update(sb.sub_records(z))
        if split is not None:
            s0, ns = int(sfirst[z]), int(souts["n_segments"][z])
            by_sub = {}
            for g in range(s0, s0 + ns):
                sg = s_seg[6 * g:6 * g + 6].tolist()
                by_sub.setdefault(int(s_sub[g]), []).append(
                    {"rc": bool(sg[0]), "read": (sg[1], sg[2]), "tpl": (sg[3], sg[4]), "score": sg[5],
                     "full_pass": bool(s_full[g]), "add_read_result": int(s_arr[g]), "zscore": float(s_zs[g])})
            res[-1]["split_reads"] = [{"subread": k, "segments": v} for k, v in by_sub.items()]
            res[-1]["n_missed_adapters"] = int(souts["n_missed_adapters"][z])
            a0 = s0 + f
            res[-1]["add_order"] = s_order[a0:a0 + int(souts["n_added"][z])].tolist()
    if kinetics or pile_opts is not None:
        todo = [z for z in range(n) if res[z]["status_code"] in (0, 6) and res[z]["consensus"]]
        zin = [(res[z]["consensus"],
                [{"seq": r["seq"], "ip": r.get("ip"), "pw": r.get("pw")}
                 for r, a in zip(chunks[z]["reads"], res[z]["add_read_results"]) if a == 0])
               for z in todo]
        if pile_opts is None:
            from .kinetics import kinetics_batch
            got, piles = kinetics_batch(zin, engine=eng), None
        else:   # one run of the placement and alignment stage for both
            from .pileup import _batch
            piles, got = _batch(zin, pile_opts.get("band"), bool(pile_opts.get("transcripts")),
                                bool(pile_opts.get("msa")), eng, bool(kinetics), bool(pile_opts.get("arrays")))
        if got is not None:
            for z, g in zip(todo, got):
                g.pop("read_status")
                res[z].update(g)
        if piles is not None:
            for z, g in zip(todo, piles):
                res[z]["pileup"] = g
                res[z]["ec"] = g["ec"]
    if demux_native is not None:
        for z in range(n):
            if demux_native[1][z]:
                res[z]["barcode"] = demux_native[0][z]
    elif demux_spec is not None:   # beside the other options: one more native call, after theirs
        from .demux import demux_batch
        todo = [z for z in range(n) if res[z]["status_code"] == 0 and res[z]["consensus"]]
        got = demux_batch([res[z]["consensus"] for z in todo], demux_spec[0], engine=eng, **demux_spec[1])
        for z, g in zip(todo, got):
            res[z]["barcode"] = g
    return res

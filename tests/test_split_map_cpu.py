"""Split mapping, host side (no GPU): tests/split_map_restatement.py pinned to things it did not
come from -- test_map_cpu.local_extents when the jump penalty forbids a second segment, planted noise-free fused
reads, the score identity -- then the driver's host path over an oracle-backed POA and the ABI mirrors.

tests/test_split_map_gpu.py imports the case builders from here."""
import ctypes
import os
import random
import subprocess

import pytest

from pbccs_amd import driver, lib, synth
from split_map_restatement import accept_split, split_map, split_map_restated
from test_map_cpu import OraclePoa, edge_cases, host_chunk, local_extents, noisy, revcomp, seeded_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ADAPTER = synth.ADAPTER
P_TEST = 20   # small enough that chance matches chain: many short segments, ties and jumps on small cases


def rand_seq(rng, n, alphabet="ACGT"):
    return "".join(rng.choice(alphabet) for _ in range(n))


def planted_cases(length=80, seed=11):
    """(draft, read, jump penalty, [(rc, read extent, draft extent)]): noise-free fused reads of a draft X."""
    x = rand_seq(random.Random(seed), length)
    a, n = len(ADAPTER), length
    return [
        (x, x, 150, [(False, (0, n), (0, n))]),
        (x, revcomp(x), 150, [(True, (0, n), (0, n))]),
        (x, x + ADAPTER + revcomp(x), 150, [(False, (0, n), (0, n)), (True, (n + a, 2 * n + a), (0, n))]),
        (x, x + ADAPTER + revcomp(x) + ADAPTER + x, 150,
         [(False, (0, n), (0, n)), (True, (n + a, 2 * n + a), (0, n)), (False, (2 * n + 2 * a, 3 * n + 2 * a), (0, n))]),
    ]


def fused_cases(seed=77):
    """(draft, read): fused reads of 2 to 4 noisy passes at the synth error rates, on drafts that take the register
    path of every columns-per-lane value and the row-buffer path."""
    import numpy as np
    rng = np.random.Generator(np.random.PCG64(seed))
    out = []
    for passes, length in ((2, 100), (3, 130), (4, 90), (2, 300), (3, 600)):
        z = synth.make_zmw(rng, length, 1)
        f = synth.make_fused_read(rng, z["truth"], passes, first_strand=passes % 2)
        out.append((z["draft"], f["seq"]))
    return out


def tie_cases(seed=5):
    """Tie-heavy pairs: homopolymer, dinucleotide and two-letter drafts against reads of the same letters."""
    rng = random.Random(seed)
    out = []
    for n in (40, 70, 150):
        out.append(("A" * n, "A" * (n // 2) + "T" * (n // 3) + "A" * 7))
        out.append((("AC" * n)[:n], ("AC" * 9) + ("GT" * 11) + "CACA" + ("TG" * 6)))
        d = rand_seq(rng, n, "AG")
        out.append((d, noisy(rng, d[5:], alphabet="AG") + noisy(rng, revcomp(d), alphabet="CT")[: n // 2]))
    return out


def identity_holds(res, jump):
    return res["score"] == sum(s["score"] for s in res["segments"]) - jump * (len(res["segments"]) - 1)


_PINNED = seeded_cases() + edge_cases()


def test_one_segment_equals_the_best_local_alignment_when_a_jump_never_pays():
    for draft, read in _PINNED:
        want = max(local_extents(draft, read)[0], local_extents(draft, revcomp(read))[0])
        got = split_map(draft, read, 3 * len(read) + 1)
        if want == 0:
            assert got is None
            continue
        assert got["n_segments"] == 1 and len(got["segments"]) == 1 and not got["truncated"], (draft, read, got)
        assert got["score"] == got["segments"][0]["score"] == want, (draft, read, got, want)


def test_single_segment_extents_are_the_local_alignments():
    # the forward orientation is MapToDraft's own alignment, extents included, whenever it is the larger one
    n = 0
    for draft, read in _PINNED:
        fwd, rev = local_extents(draft, read), local_extents(draft, revcomp(read))
        if fwd[0] <= rev[0]:
            continue
        seg = split_map(draft, read, 3 * len(read) + 1)["segments"][0]
        assert (seg["rc"], seg["read"], seg["tpl"]) == (False, fwd[1], fwd[2])
        n += 1
    assert n > 30


def test_planted_fused_reads_come_back_with_their_extents_and_strands():
    for draft, read, jump, want in planted_cases():
        got = split_map(draft, read, jump)
        assert [(s["rc"], s["read"], s["tpl"]) for s in got["segments"]] == want, (read, got)
        assert [s["score"] for s in got["segments"]] == [3 * len(draft)] * len(want)
        assert got["score"] == 3 * len(draft) * len(want) - jump * (len(want) - 1) and not got["truncated"]


def test_no_matching_base_gives_no_segment():
    draft, read = edge_cases()[0]
    assert split_map_restated(draft, [read, "", None], 0) == [None, None, None]


def test_score_identity_on_every_case():
    chained = 0
    cases = _PINNED + tie_cases() + fused_cases()[:3] + [(d, r) for d, r, _, _ in planted_cases()]
    for draft, read in cases:
        for jump in (0, P_TEST, 150):
            got = split_map(draft, read, jump, max_segments=1 << 16)
            if got is None:
                continue
            assert not got["truncated"] and got["n_segments"] == len(got["segments"])
            assert identity_holds(got, jump), (draft, read, jump, got)
            ends = [s["read"] for s in got["segments"]]
            assert all(a[1] <= b[0] for a, b in zip(ends, ends[1:]))   # chained along the read
            chained += len(ends) > 1
    assert chained > 50


def test_truncation_keeps_the_last_segments_and_the_true_count():
    draft, read, jump, want = planted_cases()[3]
    got = split_map(draft, read, jump, max_segments=2)
    assert got["truncated"] and got["n_segments"] == 3
    assert [(s["rc"], s["read"], s["tpl"]) for s in got["segments"]] == want[1:]
    assert not accept_split(got, len(read), 10)


def fused_host_chunk():
    """test_map_cpu.host_chunk() with its double-length read rebuilt as a fused pair of passes."""
    chunk = host_chunk()
    rng = random.Random(99)
    tpl_like = chunk["reads"][0]["seq"]
    fused = (noisy(rng, tpl_like, 0.02, 0.02, 0.01) + ADAPTER + revcomp(noisy(rng, tpl_like, 0.02, 0.02, 0.01)))
    chunk["reads"][2] = {"seq": fused, "flags": driver.ADAPTER_BEFORE}
    return chunk


def test_driver_host_path_recovers_the_fused_pair():
    chunk = fused_host_chunk()
    base_status, base = driver.zmw_input(chunk, OraclePoa())
    assert base_status is None and base["reads"][-1]["seq"] is None and set(base) == {"draft", "snr", "reads"}
    assert driver.dropped_reads(chunk["reads"], 10) == [(2, chunk["reads"][2])]
    status, zmw = driver.zmw_input(chunk, OraclePoa(),
                                   split_mapper=lambda d, rs: split_map_restated(d, rs, 150))
    assert status is None and zmw["draft"] == base["draft"]
    assert zmw["reads"][:-2] == base["reads"][:-1] and len(zmw["reads"]) == len(base["reads"]) + 1
    a, b = zmw["reads"][-2:]
    chain = split_map(zmw["draft"], chunk["reads"][2]["seq"], 150)
    assert accept_split(chain, len(chunk["reads"][2]["seq"]), 10)
    s0, s1 = chain["segments"]
    seq = chunk["reads"][2]["seq"]
    assert a == {"seq": seq[s0["read"][0]:s0["read"][1]], "strand": int(s0["rc"]), "ts": s0["tpl"][0],
                 "te": s0["tpl"][1], "full_pass": True}    # the read's ADAPTER_BEFORE and the missed adapter
    assert b == {"seq": seq[s1["read"][0]:s1["read"][1]], "strand": int(s1["rc"]), "ts": s1["tpl"][0],
                 "te": s1["tpl"][1], "full_pass": False}   # no ADAPTER_AFTER on the read
    # the first pass is a noisy copy of the chunk's first subread: it lies on the strand the POA gave that one
    first = next(r for r in base["reads"] if r["seq"] and r["seq"] in chunk["reads"][0]["seq"])
    assert a["strand"] != b["strand"] and a["strand"] == first["strand"]
    assert min(len(a["seq"]), len(b["seq"])) > 100 and a["te"] - a["ts"] > 100 and b["te"] - b["ts"] > 100
    assert zmw["split_reads"] == [{"subread": 2, "first": len(base["reads"]) - 1, "n_segments": 2,
                                   "segments": [s0, s1]}]
    assert zmw["n_missed_adapters"] == 1
    # a read that is no fused pair stays the one placeholder: host_chunk's own long read is three forward copies
    plain = host_chunk()
    status, kept = driver.zmw_input(plain, OraclePoa(), split_mapper=lambda d, rs: split_map_restated(d, rs, 150))
    assert kept["reads"] == driver.zmw_input(plain, OraclePoa())[1]["reads"] and kept["split_reads"] == []


def test_keyword_off_is_todays_zmw_input():
    chunk = fused_host_chunk()
    got = driver.zmw_input(chunk, OraclePoa())
    assert got == driver.zmw_input(chunk, OraclePoa(), split_mapper=None)
    status, zmw = got
    order = driver.filter_reads(chunk["reads"], 10)
    assert list(zmw) == ["draft", "snr", "reads"] and len(zmw["reads"]) == len(order)
    assert [list(r) for r in zmw["reads"]] == [["seq", "strand", "ts", "te", "full_pass"]] * len(order)
    # the record of the parent commit, byte for byte (its repr's SHA-256)
    import hashlib
    assert hashlib.sha256(repr(driver.zmw_input(host_chunk(), OraclePoa())).encode()).hexdigest() == _TODAY


_TODAY = "0d7e99f9e5b760a172fd5484cde08fe3ebc1c493a72cc0ff94a4682b2851c6b7"


def test_split_options_and_refusals():
    assert driver.split_options(True) == (None, 8)
    assert driver.split_options({"jump_penalty": 90, "max_segments": 4}) == (90, 4)
    with pytest.raises(ValueError):
        driver.split_options({"penalty": 3})
    for kw in ({"polish_window": {}}, {"strand_sites": True}, {"directional": {}}):
        with pytest.raises(ValueError):
            driver.ccs_batch([], split_long_reads=True, **kw)


def test_abi_structs_match_the_header(tmp_path):
    names = {"pbccs_split_map_output": lib.CSplitMapOutput, "pbccs_split_map_stats": lib.CSplitMapStats,
             "pbccs_split_options": lib.CSplitOptions, "pbccs_ccs_split_output": lib.CCcsSplitOutput}
    body = "".join(f'printf("%zu ", sizeof({n}));\n' +
                   "".join(f'printf("%zu ", offsetof({n}, {f}));\n' for f, _ in c._fields_) for n, c in names.items())
    # no existing struct changed layout
    old = {"pbccs_map_input": lib.CMapInput, "pbccs_map_output": lib.CMapOutput, "pbccs_map_stats": lib.CMapStats,
           "pbccs_ccs_options": lib.CCcsOptions, "pbccs_ccs_output": lib.CCcsOutput}
    body += "".join(f'printf("%zu ", sizeof({n}));\n' for n in old)
    src = tmp_path / "sizes.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "pbccs_amd.h"\nint main(void) {\n' + body +
                   'printf("%d %d\\n", PBCCS_SPLIT_JUMP_PENALTY, PBCCS_SPLIT_MAX_SEGMENTS);\nreturn 0; }\n')
    exe = str(tmp_path / "sizes")
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe])
    got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    want = []
    for c in names.values():
        want += [ctypes.sizeof(c)] + [getattr(c, f).offset for f, _ in c._fields_]
    want += [ctypes.sizeof(c) for c in old.values()]
    from pbccs_amd import mapping
    assert got == want + [mapping.SPLIT_JUMP_PENALTY, 8]
    assert ctypes.sizeof(lib.CSplitMapOutput) == 32 and ctypes.sizeof(lib.CSplitMapStats) == 40
    for name in ("pbccs_split_map_batch", "pbccs_split_map_stats_get", "pbccs_ccs_batch_split",
                 "pbccs_split_options_default"):
        assert name in lib.SIGNATURES

"""Consensus kinetics without a device: the CodecV1 codec, hand-worked cases for the Python
restatement the GPU tests compare against, the BAM tags in and out, and the host validation."""
import random

import pytest

import kinetics_restatement as R

_RNG = random.Random(5)
CONS = "".join(_RNG.choice("ACGT") for _ in range(40))


# ------------------------------------------------------------------------------------------------- codec
def test_decode_is_strictly_increasing():
    from pbccs_amd import kinetics
    d = kinetics.codec_v1_decode(range(256))
    assert d[0] == 0 and d[63] == 63 and d[64] == 64 and d[127] == 190 and d[128] == 192 and d[191] == 444
    assert d[192] == 448 and d[255] == 952
    assert all(a < b for a, b in zip(d, d[1:]))
    assert d == R.REPRESENTABLE


def test_encode_inverts_decode():
    from pbccs_amd import kinetics
    codes = list(range(256))
    assert kinetics.codec_v1_encode(kinetics.codec_v1_decode(codes)) == codes
    assert [R.encode(R.decode(c)) for c in codes] == codes


# frames -> code, by hand: group 0 is the frame itself; group 1 (64..190, step 2) is 64 + (f - 64) / 2; group 2
# (192..444, step 4) is 128 + (f - 192) / 4; group 3 (448..952, step 8) is 192 + (f - 448) / 8.  65 lies between
# 64 and 66 (-> 66 = code 65); 191 between 190 and 192 (-> 192 = code 128); 194 between 192 and 196 (-> 196 = code
# 129); 446 between 444 and 448 (-> 448 = code 192); 447 is nearest to 448; 452 between 448 and 456 (-> 456 = 193).
HAND = [(0, 0), (63, 63), (64, 64), (65, 65), (66, 65), (190, 127), (191, 128), (192, 128), (194, 129), (444, 191),
        (446, 192), (447, 192), (448, 192), (452, 193), (952, 255), (953, 255), (65535, 255)]


def test_encode_by_hand():
    from pbccs_amd import kinetics
    assert kinetics.codec_v1_encode([f for f, _ in HAND]) == [c for _, c in HAND]
    assert [R.encode(f) for f, _ in HAND] == [c for _, c in HAND]


def test_encode_agrees_with_the_search_everywhere():
    from pbccs_amd import kinetics
    frames = list(range(0, 1100)) + [4096, 65535]
    assert kinetics.codec_v1_encode(frames) == [R.encode(f) for f in frames]


# ------------------------------------------------------------------------------- the restatement, by hand
def _copy(rc, extra=None):
    """An exact copy of CONS as a read of the given strand with ip[i] = 10 + i in the read's own coordinates."""
    n = len(CONS)
    r = {"transcript": "M" * n, "rc": rc, "rb": 0, "tb": 0, "te": n, "len": n, "ip": [10 + i for i in range(n)],
         "pw": [3] * n}
    r.update(extra or {})
    return r


def test_forward_and_reverse_copies():
    n = len(CONS)
    got = R.pileup(n, [_copy(0), _copy(1), _copy(0)])
    assert got["fwd_ipd_mean"] == [10 + p for p in range(n)]
    assert got["rev_ipd_mean"] == [10 + k for k in range(n)]   # in reverse-strand order
    assert got["fwd_ipd_cov"] == [2] * n and got["rev_ipd_cov"] == [1] * n
    assert got["fwd_pw_mean"] == [3] * n and got["rev_pw"] == [3] * n
    assert (got["fn"], got["rn"]) == (2, 1)


def test_single_deletion_and_single_insertion():
    n = len(CONS)
    # read A lacks consensus base 17 (a D column), read B has one extra base after its 25th (an I column)
    a = {"transcript": "M" * 17 + "D" + "M" * (n - 18), "rc": 0, "rb": 0, "tb": 0, "te": n, "len": n - 1,
         "ip": [100] * (n - 1), "pw": [7] * (n - 1)}
    b = {"transcript": "M" * 25 + "I" + "M" * (n - 25), "rc": 0, "rb": 0, "tb": 0, "te": n, "len": n + 1,
         "ip": [100] * 25 + [9999] + [100] * (n - 25), "pw": [7] * (n + 1)}
    got = R.pileup(n, [a, b])
    assert got["fwd_ipd_cov"] == [2] * 17 + [1] + [2] * (n - 18)
    assert got["fwd_ipd_mean"] == [100] * n            # the inserted base's 9999 reaches no position
    assert got["fwd_pw_mean"] == [7] * n
    assert got["rev_ipd_cov"] == [0] * n and got["rev_ipd_mean"] == [0] * n and got["rn"] == 0
    assert got["fn"] == 2


def test_rounding_halves_up():
    def one(values):
        reads = [{"transcript": "M", "rc": 0, "rb": 0, "tb": 0, "te": 1, "len": 1, "ip": [v], "pw": [v]}
                 for v in values]
        return R.pileup(1, reads)["fwd_ipd_mean"][0]
    assert one([1, 2]) == 2        # 1.5 -> 2
    assert one([1, 1, 2]) == 1     # 1.33 -> 1
    assert one([]) == 0


def test_saturation():
    reads = [{"transcript": "MM", "rc": 0, "rb": 0, "tb": 0, "te": 2, "len": 2, "ip": [65535, 65535],
              "pw": [65535, 0]} for _ in range(5)]
    got = R.pileup(2, reads)
    assert got["fwd_ipd_mean"] == [65535, 65535] and got["fwd_ipd"] == [255, 255]
    assert got["fwd_pw_mean"] == [65535, 0] and got["fwd_pw"] == [255, 0]


def test_missing_track_is_not_counted():
    n = len(CONS)
    got = R.pileup(n, [_copy(0), _copy(0, {"pw": None})])
    assert got["fwd_ipd_cov"] == [2] * n and got["fwd_pw_cov"] == [1] * n and got["fn"] == 2


# ------------------------------------------------------------------------------------------ BAM round trip
def test_subread_bam_round_trip(tmp_path):
    from pbccs_amd import bamio, kinetics
    seq = CONS[:12]
    ip = [0, 1, 63, 64, 65, 191, 500, 952, 953, 2000, 65535, 7]
    pw = list(range(12))
    lines = [bamio.subread_sam_line("m", 7, 0, 12, seq, [8, 8, 8, 8], ip=ip, pw=pw),
             bamio.subread_sam_line("m", 7, 20, 32, seq, [8, 8, 8, 8], ip=ip, pw=pw, kinetics_codec=True),
             bamio.subread_sam_line("m", 7, 40, 52, seq, [8, 8, 8, 8]),
             bamio.subread_sam_line("m", 7, 60, 72, seq, [8, 8, 8, 8], ip=ip)]
    assert "\tip:B:S,0,1,63," in lines[0] and "\tip:B:C,0,1,63,64,65,128," in lines[1]
    path = str(tmp_path / "s.bam")
    bamio.write_bam(path, "@HD\tVN:1.5\n", lines)
    recs = bamio.read_subread_bam(path)
    assert recs[0]["ip"] == ip and recs[0]["pw"] == pw                      # B:S: frames as they are
    lossy = kinetics.codec_v1_decode(kinetics.codec_v1_encode(ip))
    assert recs[1]["ip"] == lossy and recs[1]["pw"] == pw                   # B:C: decoded frames
    assert lossy == [0, 1, 63, 64, 66, 192, 504, 952, 952, 952, 952, 7]
    assert "ip" not in recs[2] and "pw" not in recs[2]
    assert recs[3]["ip"] == ip and "pw" not in recs[3]
    chunks, _ = bamio.group_subread_bam(path)
    reads = chunks[0]["reads"]
    assert [r.get("ip") for r in reads] == [ip, lossy, None, ip]
    assert [r.get("pw") for r in reads] == [pw, pw, None, None]
    with pytest.raises(ValueError):
        bamio.subread_sam_line("m", 7, 0, 12, seq, [8, 8, 8, 8], ip=ip[:-1])


def _result(n):
    return {"consensus": CONS[:n], "qvs": [20] * n, "zscores": [0.5, -0.25], "add_read_results": [0, 0],
            "n_passes": 2, "predicted_accuracy": 0.999, "za": 0.1, "status_counts": [2, 0, 0, 0, 0],
            "sub_qv": [30] * n, "ins_qv": [31] * n, "del_qv": [32] * n, "sub_tag": "A" * n, "ins_tag": "C" * n,
            "fwd_ipd": list(range(n)), "fwd_pw": [255] * n, "fn": 3, "rev_ipd": [64] * n,
            "rev_pw": list(range(n, 0, -1)), "rn": 2}


def test_ccs_record_keeps_the_six_tags():
    from pbccs_amd import bamio, ccsio
    n = 9
    res = _result(n)
    plain = ccsio.ccs_sam_record("m", 11, res, [8, 9, 10, 11])
    assert ccsio.ccs_sam_record("m", 11, res, [8, 9, 10, 11], kinetics=False) == plain
    assert not any(t[:2] in ("fi", "fp", "fn", "ri", "rp", "rn") for t in plain.split("\t")[11:])
    kin = ccsio.ccs_sam_record("m", 11, res, [8, 9, 10, 11], kinetics=True)
    assert kin.startswith(plain + "\t")
    six = kin[len(plain) + 1:].split("\t")
    assert six == ["fi:B:C," + ",".join(map(str, range(n))), "fp:B:C" + ",255" * n, "fn:i:3",
                   "ri:B:C" + ",64" * n, "rp:B:C," + ",".join(map(str, range(n, 0, -1))), "rn:i:2"]
    back = bamio.bam_record_to_sam(bamio.sam_to_bam_record(kin, bin_=0)[4:])
    assert back == kin
    both = ccsio.ccs_sam_record("m", 11, res, [8, 9, 10, 11], rich=True, kinetics=True)
    names = [t[:2] for t in both.split("\t")[11:]]
    assert names[-11:] == ["dq", "iq", "sq", "dt", "st", "fi", "fp", "fn", "ri", "rp", "rn"]


# ------------------------------------------------------------------------------------------------ errors
@pytest.fixture
def no_engine(monkeypatch):
    """Any attempt to reach an engine fails the test."""
    import pbccs_amd

    def boom(*a, **k):
        raise AssertionError("the engine was touched")
    monkeypatch.setattr(pbccs_amd, "default_engine", boom)
    monkeypatch.setattr(pbccs_amd, "Engine", boom)


def test_track_length_mismatch_is_refused_on_the_host(no_engine):
    import pbccs_amd
    from pbccs_amd import kinetics
    read = {"seq": CONS, "ip": [1] * (len(CONS) - 1), "pw": [1] * len(CONS)}
    with pytest.raises(pbccs_amd.PbccsError) as e:
        kinetics.kinetics_batch([(CONS, [read])])
    assert e.value.code == -1 and "ip track" in str(e.value)
    with pytest.raises(pbccs_amd.PbccsError) as e:
        kinetics.kinetics_pileup([(len(CONS), [_copy(0, {"pw": [3] * 5})])])
    assert e.value.code == -1 and "pw track" in str(e.value)
    with pytest.raises(pbccs_amd.PbccsError):
        kinetics.kinetics_batch([(CONS, [{"seq": CONS, "ip": [70000] * len(CONS)}])])


def test_chunk_without_tracks_is_refused_on_the_host(no_engine):
    from pbccs_amd import driver
    chunk = {"snr": [8, 8, 8, 8], "reads": [{"seq": CONS, "flags": 3} for _ in range(3)]}
    with pytest.raises(ValueError, match="carry no ip / pw tracks"):
        driver.ccs_batch([chunk], kinetics=True)

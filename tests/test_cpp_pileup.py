"""The C++ facade's PacBio::CCS::ConsensusPileup and PileupCigar (include/pbccs_amd/Pileup.hpp):
tests/cpp/pileup_driver.cpp compiles, links and runs PileupCigar on the host (CPU tests), and gives the Python
call's arrays on the device (gpu test)."""
import os
import subprocess

import pytest

import pileup_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "pileup_driver.cpp")
BIN = os.path.join(ROOT, "tests", "cpp", "_build", "pileup_driver")
LIBDIR = os.path.join(ROOT, "pbccs_amd", "_lib")


def _build():
    os.makedirs(os.path.dirname(BIN), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-I" + os.path.join(ROOT, "include"), SRC, "-L" + LIBDIR,
                           "-lpbccs_amd", "-Wl,-rpath," + LIBDIR, "-o", BIN])


def _run(args, text):
    return subprocess.run([BIN] + args, input=text, capture_output=True, text=True, check=True).stdout.split("\n")[:-1]


def test_pileup_facade_driver_compiles_and_links():
    if not os.path.exists(os.path.join(LIBDIR, "libpbccs_amd.so")):
        pytest.skip("library not built")
    _build()
    assert os.path.exists(BIN)


def test_facade_cigar_is_the_restatement():
    if not os.path.exists(os.path.join(LIBDIR, "libpbccs_amd.so")):
        pytest.skip("library not built")
    _build()
    cases = [("M", 0, 1), ("MMRIIDM", 2, 10), ("IIMMDD", 0, 4), ("DMRRI", 3, 7), ("M" * 70 + "I" * 3, 1, 80)]
    got = _run(["cigar"], "".join(f"{t} {rb} {n}\n" for t, rb, n in cases))
    assert got == [R.cigar(*c) for c in cases]
    assert got[1] == "2S2=1X2I1D1=2S"


@pytest.mark.gpu
def test_pileup_facade_gives_the_python_arrays():
    import pbccs_amd
    from pbccs_amd import pileup, synth
    _build()
    z = synth.make_zmws(1, 200, 4, seed=55)[0]
    reads = [r["seq"] for r in z["reads"]]
    want = pileup.pileup_batch([(z["draft"], reads)], transcripts=True, engine=pbccs_amd.Engine(0))[0]
    flat = lambda rows: [v for row in rows for v in row]   # noqa: E731
    for args in ([], ["band"]):
        got = _run(args, z["draft"] + "\n" + "".join(s + "\n" for s in reads))
        ints = [[int(x) for x in line.split()] for line in got[:12]]
        assert ints[0] == [want["cov_sum"]] + want["n_used"] and want["n_used"] == [2, 2]
        assert ints[1] == flat(want["counts"][0]) and ints[2] == flat(want["counts"][1])
        assert ints[3:5] == want["ins_reads"] and ints[5:7] == want["ins_bases"]
        assert ints[7:12] == [want[k] for k in ("slot_cov", "max_ins", "cov", "plurality", "ins_plurality")]
        for k, r in enumerate(want["reads"]):
            assert [int(x) for x in got[12 + 2 * k].split()] == [0] + [r[key] for key in (
                "n_match", "n_mismatch", "n_ins", "n_del", "rc", "rb", "re", "tb", "te")]
            assert got[13 + 2 * k] == r["transcript"] and r["status"] == "used"
    assert want["cov_sum"] > 3 * len(z["draft"])

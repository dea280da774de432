"""The C++ facade's PacBio::CCS::ConsensusKinetics and CodecV1 functions (include/pbccs_amd/Kinetics.hpp):
tests/cpp/kinetics_driver.cpp compiles, links and runs the codec on the host (CPU tests), and gives the Python
call's arrays on the device (gpu test)."""
import os
import random
import subprocess

import pytest

import kinetics_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "kinetics_driver.cpp")
BIN = os.path.join(ROOT, "tests", "cpp", "_build", "kinetics_driver")
LIBDIR = os.path.join(ROOT, "pbccs_amd", "_lib")


def _build():
    os.makedirs(os.path.dirname(BIN), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-I" + os.path.join(ROOT, "include"), SRC, "-L" + LIBDIR,
                           "-lpbccs_amd", "-Wl,-rpath," + LIBDIR, "-o", BIN])


def _lines(args, text):
    out = subprocess.run([BIN] + args, input=text, capture_output=True, text=True, check=True).stdout
    return [[int(x) for x in line.split()] for line in out.split("\n")[:-1]]


def test_kinetics_facade_driver_compiles_and_links():
    if not os.path.exists(os.path.join(LIBDIR, "libpbccs_amd.so")):
        pytest.skip("library not built")
    _build()
    assert os.path.exists(BIN)


def test_facade_codec_is_the_restatement():
    if not os.path.exists(os.path.join(LIBDIR, "libpbccs_amd.so")):
        pytest.skip("library not built")
    _build()
    frames = list(range(1000)) + [4000, 65535]
    codes, decoded = _lines(["codec"], " ".join(map(str, frames)) + "\n")
    assert codes == [R.encode(f) for f in frames]
    assert decoded == R.REPRESENTABLE


@pytest.mark.gpu
def test_kinetics_facade_gives_the_python_arrays():
    import pbccs_amd
    from pbccs_amd import kinetics, synth
    _build()
    rng = random.Random(3)
    z = synth.make_zmws(1, 200, 4, seed=55)[0]
    reads = [{"seq": r["seq"], "ip": [rng.randrange(1200) for _ in r["seq"]],
              "pw": [rng.randrange(70) for _ in r["seq"]]} for r in z["reads"]]
    reads[1]["pw"] = None
    text = z["draft"] + "\n" + "".join(
        r["seq"] + "\n" + " ".join(map(str, r["ip"])) + "\n" + ("-" if r["pw"] is None else " ".join(map(str, r["pw"])))
        + "\n" for r in reads)
    want = kinetics.kinetics_batch([(z["draft"], reads)], engine=pbccs_amd.Engine(0))[0]
    for args in ([], ["band"]):
        got = _lines(args, text)
        assert got[0] == [want["fn"], want["rn"]] and want["fn"] == 2 and want["rn"] == 2
        keys = [f"{s}_{t}{x}" for s in ("fwd", "rev") for x in ("", "_mean", "_cov") for t in ("ipd", "pw")]
        assert got[1:13] == [want[k] for k in keys]
        assert got[13] == [0, 0, 0, 0]
    assert want["rev_pw_cov"] != want["rev_ipd_cov"]

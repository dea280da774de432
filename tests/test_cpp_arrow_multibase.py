"""The Arrow half of the C++ facade's multi-base surface (include/pbccs_amd/ConsensusCore.hpp):
tests/cpp/arrow_multibase_driver.cpp scores a wide mutation with the Arrow scorer's Score / FastScore / Scores,
runs RefineConsensus and RefineRepeats on one slipped-repeat ZMW of tests/golden/arrow_repeat_slips.json and applies
a wide mutation.  Its outcome must equal the Python scorer's.  The CPU test compiles and links it."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "arrow_multibase_driver.cpp")
BIN = os.path.join(ROOT, "tests", "cpp", "_build", "arrow_multibase_driver")
LIBDIR = os.path.join(ROOT, "pbccs_amd", "_lib")


def _build():
    os.makedirs(os.path.dirname(BIN), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-I" + os.path.join(ROOT, "include"), SRC, "-L" + LIBDIR,
                           "-lpbccs_amd", "-Wl,-rpath," + LIBDIR, "-o", BIN])


def test_arrow_multibase_facade_driver_compiles_and_links():
    _build()
    assert os.path.exists(BIN)


@pytest.mark.gpu
def test_arrow_multibase_facade_driver():
    import pbccs_amd as P
    from tests import arrow_multibase_common as C
    _build()
    z = C.load_slips()[0]
    wide = P.Mutation(P.INSERTION, 33, "GCA")
    lines = [" ".join([z["draft"]] + [repr(float(x)) for x in z["snr"]] + [str(z["unit_len"])]),
             f"{wide.type} {wide.start} {wide.end} {wide.new_bases}"]
    lines += [f"{r['strand']} {r['ts']} {r['te']} {r['seq']}" for r in z["reads"]]
    out = subprocess.run([BIN], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    got = [ln.split() for ln in out.stdout.strip().split("\n")]
    s = P.ArrowMultiReadMutationScorer(P.ArrowConfig(z["snr"]), z["draft"])
    for r in z["reads"]:
        s.AddRead(r["seq"], r["strand"], r["ts"], r["te"])
    want = [s.Score(wide, wide=True), s.FastScore(wide, wide=True)] + s.Scores(wide, wide=True)
    assert got[0][0] == "score" and [float.fromhex(x) for x in got[0][1:]] == want
    conv, nt, na = P.RefineConsensus(s)
    assert got[1] == ["refine", str(int(conv)), str(nt), str(na), s.Template()] and s.Template() == z["oracle_final"]
    for k in (2, 3):
        rc, rt, ra = P.RefineRepeats(s, z["unit_len"])
        assert got[k] == ["repeats", str(int(rc)), str(rt), str(ra), s.Template()]
    assert got[2][3] == "1" and got[3][1:4] == ["1", got[2][2], "0"] and s.Template() == z["truth"]
    s.ApplyMutations([wide], wide=True)
    assert got[4] == ["applied", s.Template()]

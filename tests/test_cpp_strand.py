"""StrandSites / StrandScores of the C++ facade (include/pbccs_amd/ConsensusCore.hpp):
tests/cpp/strand_driver.cpp polishes the fixture's ZMWs through an Arrow scorer and prints the screen's sites.  Its
outcome must equal the Python scorer's.  The CPU test compiles and links it."""
import os
import subprocess

import pytest

from tests import strand_common as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "strand_driver.cpp")
BIN = os.path.join(ROOT, "tests", "cpp", "_build", "strand_driver")
LIBDIR = os.path.join(ROOT, "pbccs_amd", "_lib")


def _build():
    os.makedirs(os.path.dirname(BIN), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-I" + os.path.join(ROOT, "include"), SRC, "-L" + LIBDIR,
                           "-lpbccs_amd", "-Wl,-rpath," + LIBDIR, "-o", BIN])


def test_strand_facade_driver_compiles_and_links():
    _build()
    assert os.path.exists(BIN)


@pytest.mark.gpu
@pytest.mark.parametrize("idx", [0, 1, 2])
def test_strand_facade_driver(idx):
    import pbccs_amd as P
    _build()
    z = C.load_fixture()[idx]
    lines = [" ".join([z["draft"]] + [repr(float(x)) for x in z["snr"]] + [repr(C.MIN_ZSCORE)])]
    lines += [f"{r['strand']} {r['ts']} {r['te']} {r['seq']}" for r in z["reads"]]
    out = subprocess.run([BIN], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    rows = [ln.split() for ln in out.stdout.strip().split("\n")]
    s = P.ArrowMultiReadMutationScorer(P.ArrowConfig(z["snr"]), z["draft"])
    for r in z["reads"]:
        s.AddRead(r["seq"], r["strand"], r["ts"], r["te"], C.MIN_ZSCORE)
    assert P.RefineConsensus(s)[0]
    assert rows[0] == ["template", s.Template()]
    want = s.StrandSites()
    got = [(int(r[1]), int(r[2]), r[3], float.fromhex(r[4]), float.fromhex(r[5])) for r in rows if r[0] == "site"]
    assert got == [tuple(w) for w in want]
    assert [tuple(g[:3]) for g in got] == [tuple(w[:3]) for w in z["oracle_sites"]]
    if want:
        w = want[0]
        sums = s.StrandScores([P.Mutation(w.type, w.pos, w.base)])[0]
        r = [r for r in rows if r[0] == "sums"][0]
        assert (float.fromhex(r[1]), float.fromhex(r[2]), int(r[3]), int(r[4])) == tuple(sums)
        assert (sums.sum_fwd, sums.sum_rev) == (w.sum_fwd, w.sum_rev)
    else:
        assert not [r for r in rows if r[0] == "sums"]

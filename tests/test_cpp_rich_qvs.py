"""ConsensusRichQVs of the C++ facade (include/pbccs_amd/ConsensusCore.hpp, Quiver.hpp):
tests/cpp/rich_qvs_driver.cpp builds an Arrow scorer on the single-scorer fixture of tests/rich_qvs_common.py and
prints ConsensusQVs and the rich struct.  Its outcome must equal the Python scorer's.  The CPU test compiles and
links it, and compiles the Quiver overload."""
import os
import subprocess

import pytest

import rich_qvs_common as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "rich_qvs_driver.cpp")
BIN = os.path.join(ROOT, "tests", "cpp", "_build", "rich_qvs_driver")
LIBDIR = os.path.join(ROOT, "pbccs_amd", "_lib")


def _build():
    os.makedirs(os.path.dirname(BIN), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-I" + os.path.join(ROOT, "include"), SRC, "-L" + LIBDIR,
                           "-lpbccs_amd", "-Wl,-rpath," + LIBDIR, "-o", BIN])


def test_rich_qvs_facade_driver_compiles_and_links():
    _build()
    assert os.path.exists(BIN)


def test_quiver_overload_compiles(tmp_path):
    src = tmp_path / "q.cpp"
    src.write_text('#include <pbccs_amd/Quiver.hpp>\n'
                   'ConsensusCore::RichConsensusQVs f(ConsensusCore::AbstractMultiReadMutationScorer& s)\n'
                   '{ return ConsensusCore::ConsensusRichQVs(s); }\n')
    subprocess.check_call(["g++", "-std=c++17", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), str(src)])


@pytest.mark.gpu
def test_rich_qvs_facade_driver():
    import pbccs_amd as P
    _build()
    reads = C.arrow_reads()
    lines = [" ".join([C.TPL] + [repr(float(x)) for x in C.SNR])]
    lines += [f"{r['strand']} {r['ts']} {r['te']} {r['seq']}" for r in reads]
    out = subprocess.run([BIN], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    got = {ln.split()[0]: ln.split()[1:] for ln in out.stdout.strip().split("\n")}
    s = P.ArrowMultiReadMutationScorer(P.ArrowConfig(C.SNR), C.TPL)
    for r in reads:
        s.AddRead(r["seq"], r["strand"], r["ts"], r["te"])
    want = P.ConsensusRichQVs(s)
    assert [int(x) for x in got["plain"]] == P.ConsensusQVs(s) == want["qvs"]
    for k in ("qvs", "sub_qv", "ins_qv", "del_qv"):
        assert [int(x) for x in got[k]] == want[k], k
    assert got["sub_tag"] == [want["sub_tag"]] and got["ins_tag"] == [want["ins_tag"]]

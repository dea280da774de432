"""The multi-base half of the C++ facade (include/pbccs_amd/Quiver.hpp): tests/cpp/quiver_multibase_driver.cpp is a
ConsensusCore caller written against the facade only.  It checks the reference's enumerator and bounds known
answers itself (TestMutationEnumerator.cpp:107-137, TestMultiReadMutationScorer.cpp:545-595, each of the four
recursor types) and runs RefineRepeats on the seeded repeat-count draft of tests/test_quiver_multibase_gpu.py, whose
outcome must equal the test-side loop over the CPU restatement.  The CPU test compiles and links it."""
import os
import subprocess

import pytest

from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "quiver_multibase_driver.cpp")
BIN = os.path.join(ROOT, "tests", "cpp", "_build", "quiver_multibase_driver")
LIBDIR = os.path.join(ROOT, "pbccs_amd", "_lib")


def _build():
    os.makedirs(os.path.dirname(BIN), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-I" + os.path.join(ROOT, "include"), SRC, "-L" + LIBDIR,
                           "-lpbccs_amd", "-Wl,-rpath," + LIBDIR, "-o", BIN])


def test_multibase_facade_driver_compiles_and_links():
    _build()
    assert os.path.exists(BIN)


@pytest.mark.gpu
def test_multibase_facade_driver(tmp_path):
    from tests.test_quiver_multibase_gpu import PARAMS2, _oracle_on, _oracle_refine_repeats, _repeat_case
    _build()
    draft, truth, reads, _ = _repeat_case(7)
    lines = [" ".join(repr(float(x)) for x in O.qv_params(PARAMS2)), draft, str(len(reads))]
    for r in reads:
        f = r["features"]
        tracks = [",".join(repr(float(ord(x)) if isinstance(x, str) else float(x)) for x in f[k])
                  for k in ("ins", "subs", "del", "del_tag", "merge")]
        lines.append(f"{r['strand']} {r['ts']} {r['te']} {r['seq']} " + " ".join(tracks))
    lines.append("1 2")
    case = tmp_path / "case5.txt"
    case.write_text("\n".join(lines) + "\n")
    out = subprocess.run([BIN, str(case)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    got = out.stdout.split("\n")
    assert got[0] == "enumerator ok" and got[1] == "bounds ok"
    base = _oracle_on(truth, reads, [(0, len(truth))] * len(reads)).baseline()
    for line, iters in zip(got[2:4], (1, 2)):
        w = line.split()
        conv, nt, na, tpl = _oracle_refine_repeats(draft, reads, 2, 3, iters)
        assert w[:6] == ["repeat", str(iters), str(int(conv)), str(nt), str(na), tpl]
        assert tpl == truth and float.fromhex(w[6]) == base

"""The diploid half of the C++ facades (include/pbccs_amd/ConsensusCore.hpp, Quiver.hpp): tests/cpp/diploid_driver.cpp
is a ConsensusCore caller written against the facades only.  The CPU test compiles and links it and runs its
host-only known answers of IsSiteHeterozygous; the GPU test runs it on the Quiver seed-7 case of
tests/test_diploid_cpu.py, where it must print the sites the Python path reports (floats compared through
float.hex)."""
import os
import subprocess

import pytest

from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "diploid_driver.cpp")
BIN = os.path.join(ROOT, "tests", "cpp", "_build", "diploid_driver")
LIBDIR = os.path.join(ROOT, "pbccs_amd", "_lib")


def _build():
    os.makedirs(os.path.dirname(BIN), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-I" + os.path.join(ROOT, "include"), SRC, "-L" + LIBDIR,
                           "-lpbccs_amd", "-Wl,-rpath," + LIBDIR, "-o", BIN])


def test_diploid_facade_driver_compiles_links_and_knows_the_answers():
    _build()
    out = subprocess.run([BIN], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.split("\n")[0] == "known answers ok"


@pytest.mark.gpu
def test_diploid_facade_driver(tmp_path):
    import pbccs_amd as P
    from tests.test_diploid_cpu import CASES, PRIORS, make_case
    from tests.test_quiver_gpu import PARAMS2, GpuQuiver
    _build()
    tpl, reads = make_case("quiver", CASES[0])
    lines = [" ".join(repr(float(x)) for x in O.qv_params(PARAMS2)), tpl, str(len(reads))]
    for r in reads:
        f = r["features"]
        tracks = [",".join(repr(float(ord(x)) if isinstance(x, str) else float(x)) for x in f[k])
                  for k in ("ins", "subs", "del", "del_tag", "merge")]
        lines.append(f"{r['strand']} {r['ts']} {r['te']} {r['seq']} " + " ".join(tracks))
    lines += [repr(p) for p in PRIORS]
    case = tmp_path / "diploid_case.txt"
    case.write_text("\n".join(lines) + "\n")
    out = subprocess.run([BIN, str(case)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    got = [w.split() for w in out.stdout.split("\n") if w.startswith("site ")]
    g = GpuQuiver(tpl, PARAMS2)
    for r in reads:
        g.add_read(r["seq"], r["strand"], r["ts"], r["te"], r["features"])
    exp = []
    for prior in PRIORS:
        for d in g.s.DiploidSites(prior):
            exp.append((float(prior), d.Position, d.Allele0, d.Allele1, float(d.LogBayesFactor).hex(),
                        "".join(str(a) for a in d.AlleleForRead)))
    assert len(exp) > 0
    assert [(float.fromhex(w[1]), int(w[2]), int(w[3]), int(w[4]), float.fromhex(w[5]).hex(), w[6]) for w in got] == exp

"""The C++ facade's AlignEnds (include/pbccs_amd/Align.hpp): tests/cpp/align_modes_driver.cpp compiles and links
against the header and the library, throws the refusals without a device, and on the GPU aligns one pair SEMIGLOBAL
and LOCAL to the restatement's transcript, score and extents."""
import os
import subprocess

import pytest

from tests import align_modes_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "align_modes_driver.cpp")
BIN = os.path.join(ROOT, "tests", "cpp", "_build", "align_modes_driver")
LIBDIR = os.path.join(ROOT, "pbccs_amd", "_lib")


def build_driver():
    os.makedirs(os.path.dirname(BIN), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"), SRC,
                           "-L" + LIBDIR, "-lpbccs_amd", "-Wl,-rpath," + LIBDIR, "-o", BIN])
    return BIN


def test_modes_driver_compiles_links_and_refuses():
    out = subprocess.run([build_driver()], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.split("\n")[0] == "modes host ok"


@pytest.mark.gpu
def test_one_pair_of_each_mode_equals_the_restatement():
    target = "TTGACCA" + "GATTACAGATTACCA" + "CCGTAGT"
    query = "GG" + "GATTACGATTTACCA" + "AC"
    params = (3, -5, -4, -4)
    out = subprocess.run([build_driver(), target, query] + [str(v) for v in params], capture_output=True, text=True,
                         timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.split("\n")
    for line, mode in zip(lines, (R.SEMIGLOBAL, R.LOCAL)):
        tr, score, ext = R.align_ends(target, query, mode, params)
        (tb, te), (qb, qe) = ext["target"], ext["query"]
        assert line == f"{mode} {tr}. {score} {tb} {te} {qb} {qe} 0", (mode, line)

"""The C++ facade's BandOptions (include/pbccs_amd/Align.hpp): tests/cpp/align_band_driver.cpp compiles and links
against the header and the library, knows the certificate's host-side answers without a device, and on the GPU aligns
the block-indel pair banded and full to the same alignment."""
import os
import subprocess

import pytest

from tests.align_band_restatement import block_indel_pair
from tests.test_align_cpu import ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "align_band_driver.cpp")
BIN = os.path.join(ROOT, "tests", "cpp", "_build", "align_band_driver")
LIBDIR = os.path.join(ROOT, "pbccs_amd", "_lib")


def build_driver():
    os.makedirs(os.path.dirname(BIN), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(ROOT, "include"), SRC,
                           "-L" + LIBDIR, "-lpbccs_amd", "-Wl,-rpath," + LIBDIR, "-o", BIN])
    return BIN


def test_band_driver_compiles_links_and_knows_the_host_answers():
    out = subprocess.run([build_driver()], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.split("\n")[0] == "band host ok"


@pytest.mark.gpu
@pytest.mark.parametrize("k", (5, 12))
def test_block_indel_pair_banded_equals_full(k):
    t, q = block_indel_pair(k)
    tr, score = ref(0, t, q)
    out = subprocess.run([build_driver(), str(k), t, q], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.split("\n")
    assert lines[0] == f"nw {tr}. {score} attempts 1 2 banded 1 1" and lines[1] == "equal ok"

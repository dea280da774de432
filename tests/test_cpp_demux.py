"""The C++ facade's PacBio::CCS::BarcodeDemux (include/pbccs_amd/Demux.hpp): tests/cpp/demux_driver.cpp compiles,
links and refuses on the host (CPU tests) and reproduces two restatement cases (gpu test)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "demux_driver.cpp")
BIN = os.path.join(ROOT, "tests", "cpp", "_build", "demux_driver")
LIBDIR = os.path.join(ROOT, "pbccs_amd", "_lib")


def _build():
    os.makedirs(os.path.dirname(BIN), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-I" + os.path.join(ROOT, "include"), SRC, "-L" + LIBDIR,
                           "-lpbccs_amd", "-Wl,-rpath," + LIBDIR, "-o", BIN])


def test_demux_facade_driver_compiles_links_and_refuses_on_the_host():
    if not os.path.exists(os.path.join(LIBDIR, "libpbccs_amd.so")):
        pytest.skip("library not built")
    _build()
    assert subprocess.run([BIN], capture_output=True, text=True, check=True).stdout.strip() == "demux host ok"


def _run(params, design, window, min_quality, min_score_lead, barcodes, reads):
    head = " ".join(str(v) for v in list(params) + [1 if design == "symmetric" else 0, window, min_quality,
                                                    min_score_lead])
    text = "\n".join([head, " ".join(barcodes)] + [r or "-" for r in reads]) + "\n"
    out = subprocess.run([BIN, "run"], input=text, capture_output=True, text=True, check=True).stdout
    res = []
    for line in out.strip().splitlines():
        v = [int(x) for x in line.split()]
        sec = lambda s: None if s == -2**31 else s  # noqa: E731
        res.append({"lead": v[0], "trail": v[1], "called": bool(v[2]),
                    "pair": (min(v[0], v[1]), max(v[0], v[1])) if v[2] else (-1, -1), "score": v[3],
                    "score_lead": v[4], "quality": v[5], "lead_extent": (v[6], v[7]), "trail_extent": (v[8], v[9]),
                    "clip": None if v[12] else (v[10], v[11]), "overlap": bool(v[12]),
                    "best": ((v[14], v[13]), (v[17], v[16])), "second": (sec(v[15]), sec(v[18]))})
    return res


@pytest.mark.gpu
def test_demux_facade_reproduces_the_restatement():
    import numpy as np
    import demux_restatement as R
    _build()
    rng = np.random.default_rng(31)
    seq = lambda n: "".join("ACGT"[k] for k in rng.integers(0, 4, n))  # noqa: E731
    barcodes = [seq(16) for _ in range(70)] + [seq(7)]
    reads = [barcodes[4] + seq(150) + R.revcomp(barcodes[69]), seq(200), "", barcodes[70] + seq(3),
             barcodes[9][:15] + seq(90) + R.revcomp(barcodes[9])]
    assert _run((3, -5, -4, -4), "asymmetric", 0, 74, 0, barcodes, reads) == R.demux(reads, barcodes, min_quality=74)
    assert _run((1, -1, -1, -1), "symmetric", 20, 10, 1, barcodes, reads) == R.demux(
        reads, barcodes, params=(1, -1, -1, -1), design="symmetric", window=20, min_quality=10, min_score_lead=1)

"""The C++ facade's PacBio::CCS::MapToDraft (include/pbccs_amd/SparsePoa.hpp): tests/cpp/map_driver.cpp compiles and
links (CPU test) and reports the oracle's summaries on three of the edge cases (gpu test)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "map_driver.cpp")
BIN = os.path.join(ROOT, "tests", "cpp", "_build", "map_driver")
LIBDIR = os.path.join(ROOT, "pbccs_amd", "_lib")


def _build():
    os.makedirs(os.path.dirname(BIN), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-I" + os.path.join(ROOT, "include"), SRC, "-L" + LIBDIR,
                           "-lpbccs_amd", "-Wl,-rpath," + LIBDIR, "-o", BIN])


def test_map_facade_driver_compiles_and_links():
    if not os.path.exists(os.path.join(LIBDIR, "libpbccs_amd.so")):
        pytest.skip("library not built")
    _build()
    assert os.path.exists(BIN)


def _run(min_score, draft, reads):
    out = subprocess.run([BIN], input="\n".join([str(min_score), draft] + reads) + "\n", capture_output=True,
                         text=True, check=True).stdout
    return [tuple(int(x) for x in line.split()) for line in out.strip().splitlines()]


@pytest.mark.gpu
def test_map_facade_matches_the_oracle_on_edge_cases():
    from test_map_cpu import edge_cases, local_extents, oracle_map
    _build()
    cases = edge_cases()
    for draft, read in (cases[0], cases[4], cases[6]):   # no matching base, read == rc(draft), unaligned flanks
        css, s = oracle_map(draft, read)
        assert css == draft
        (mapped, rc, rb, re_, tb, te, score), = _run(0, draft, [read])
        assert mapped == 1 and (bool(rc), (rb, re_), (tb, te)) == (s["rc"], s["read"], s["tpl"])
    # the mapped flag: a 10-base exact copy scores 30
    draft, _ = cases[6]
    got = _run(30.5, draft, [draft[5:15], draft[5:16]])
    assert [g[0] for g in got] == [0, 1] and got[0][1:] == (0, 0, 0, 0, 0, 0)
    assert got[1][1:] == (0, 0, 11, 5, 16, 33) and local_extents(draft, draft[5:16])[0] == 33

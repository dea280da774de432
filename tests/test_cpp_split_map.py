"""The C++ facade's PacBio::CCS::SplitMapToDraft (include/pbccs_amd/SparsePoa.hpp): tests/cpp/split_map_driver.cpp
compiles and links (CPU test) and reproduces two restatement cases (gpu test)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "split_map_driver.cpp")
BIN = os.path.join(ROOT, "tests", "cpp", "_build", "split_map_driver")
LIBDIR = os.path.join(ROOT, "pbccs_amd", "_lib")


def _build():
    os.makedirs(os.path.dirname(BIN), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-I" + os.path.join(ROOT, "include"), SRC, "-L" + LIBDIR,
                           "-lpbccs_amd", "-Wl,-rpath," + LIBDIR, "-o", BIN])


def test_split_map_facade_driver_compiles_and_links():
    if not os.path.exists(os.path.join(LIBDIR, "libpbccs_amd.so")):
        pytest.skip("library not built")
    _build()
    assert os.path.exists(BIN)


def _run(jump, max_segments, draft, reads):
    out = subprocess.run([BIN], input="\n".join([f"{jump} {max_segments}", draft] + reads) + "\n",
                         capture_output=True, text=True, check=True).stdout
    rows = [tuple(int(x) for x in line.split()) for line in out.strip().splitlines()]
    res = []
    while rows:
        count, truncated, score = rows.pop(0)
        segs = [rows.pop(0) for _ in range(min(count, max_segments))]
        res.append(None if count == 0 else {
            "score": score, "n_segments": count, "truncated": bool(truncated),
            "segments": [{"rc": bool(s[0]), "read": (s[1], s[2]), "tpl": (s[3], s[4]), "score": s[5]} for s in segs]})
    return res


@pytest.mark.gpu
def test_split_map_facade_reproduces_the_restatement():
    from split_map_restatement import split_map
    from test_split_map_cpu import planted_cases
    _build()
    draft, three, jump, _ = planted_cases()[3]        # X A rc(X) A X
    _, pair, _, _ = planted_cases()[2]                # X A rc(X)
    assert _run(jump, 8, draft, [three, pair]) == [split_map(draft, three, jump), split_map(draft, pair, jump)]
    assert _run(jump, 2, draft, [three]) == [split_map(draft, three, jump, 2)]

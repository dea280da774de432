#!/usr/bin/env python3
"""Writes tests/golden/align_kats.json: the known answers of ConsensusCore's pairwise-alignment unit tests.

Usage: make_align_golden.py PATH/TO/ConsensusCore/src/Tests/TestPairwiseAlignment.cpp [OUT.json]

Only values are taken from the file -- input strings, expected aligned strings, transcripts, counts and position
arrays -- of the Representation, GlobalAlignment, TargetPositionsInQuery, AffineAlignment (Basic, LargeGap) and
Iupac tests.  The AlignLinear cases are left out (the project has no AlignLinear); of LinearAlignmentTests only
the two input strings and the parameters of its one Align call are kept ("align_peer": inputs without an
expectation)."""
import json
import os
import re
import sys

STR = r'"((?:[^"\\]|\\.)*)"'


def test_bodies(text):
    """{(suite, name): body} of every TEST(...) { ... } block (bodies have balanced braces)."""
    out = {}
    for m in re.finditer(r"TEST\((\w+),\s*(\w+)\)\s*\{", text):
        depth, k = 1, m.end()
        while depth:
            depth += {"{": 1, "}": -1}.get(text[k], 0)
            k += 1
        out[(m.group(1), m.group(2))] = text[m.end():k - 1]
    return out


def literals(body):
    """{name: value} of every `const char* name = "..." "..." ...;` (adjacent literals concatenated)."""
    out = {}
    for m in re.finditer(r"const\s+char\s*\*\s*(\w+)\s*=\s*\\?\s*((?:" + STR + r"\s*)+);", body):
        out[m.group(1)] = "".join(re.findall(STR, m.group(2)))
    return out


def value(tok, names):
    tok = tok.strip()
    m = re.fullmatch(STR, tok)
    if m:
        return m.group(1)
    if tok in names:
        return names[tok]
    m = re.fullmatch(r"(\d+\.?\d*)\s*/\s*(\d+\.?\d*)", tok)
    if m:
        return float(m.group(1)) / float(m.group(2))
    return float(tok) if "." in tok else int(tok)


def cases(body):
    """The alignments a test body makes, in order, each with the expectations that follow it."""
    names = literals(body)
    out = []
    arg = r"(" + STR + r"|\w+)"
    for stmt in body.split(";"):
        m = re.search(r"PairwiseAlignment\s+\w+\(\s*" + arg + r"\s*,\s*" + arg + r"\s*\)", stmt)
        if m:
            out.append({"call": "PairwiseAlignment", "target": value(m.group(1), names),
                        "query": value(m.group(3), names), "expect": {}})
            continue
        m = re.search(r"=\s*(Align|AlignAffine|AlignAffineIupac)\(\s*" + arg + r"\s*,\s*" + arg + r"\s*\)", stmt)
        if m:
            out.append({"call": m.group(1), "target": value(m.group(2), names), "query": value(m.group(4), names),
                        "expect": {}})
            continue
        m = re.search(r"(?:EXPECT|ASSERT)_(?:FLOAT_)?EQ\((.+),\s*\w+(?:->|\.)(\w+)\(\)\s*\)", stmt, re.S)
        if m and out:
            out[-1]["expect"][m.group(2)] = value(m.group(1), names)
    return out


def positions(body):
    arrays = {}
    out = []
    for blk in re.findall(r"\{((?:[^{}]|\{[^{}]*\})*)\}", body):
        arrays = {m.group(1): [int(x) for x in m.group(2).split(",")]
                  for m in re.finditer(r"int\s+(\w+)\[\]\s*=\s*\{([^}]*)\}", blk)}
        for m in re.finditer(r"TargetToQueryPositions\(" + STR + r"\),\s*ElementsAreArray\((\w+)\)", blk):
            out.append({"transcript": m.group(1), "expected": arrays[m.group(2)]})
    return out


def main(argv):
    src = argv[1]
    dst = argv[2] if len(argv) > 2 else os.path.join(os.path.dirname(os.path.abspath(__file__)), "align_kats.json")
    tests = test_bodies(open(src).read())
    strip = lambda cs: [{k: v for k, v in c.items() if k != "call"} for c in cs]   # noqa: E731
    large = cases(tests[("AffineAlignmentTests", "LargeGapTest")])
    linear = tests[("LinearAlignmentTests", "BasicTest")]
    peer = literals(linear)
    pm = re.search(r"AlignParams\s+\w+\(\s*(-?\d+)\s*,\s*(-?\d+)\s*,\s*(-?\d+)\s*,\s*(-?\d+)\s*\)", linear)
    doc = {
        "source": "ConsensusCore/src/Tests/TestPairwiseAlignment.cpp",
        "representation": strip(cases(tests[("PairwiseAlignmentTests", "RepresentationTests")])),
        "align": strip(cases(tests[("PairwiseAlignmentTests", "GlobalAlignmentTests")])),
        "target_to_query_positions": positions(tests[("PairwiseAlignmentTests", "TargetPositionsInQueryTest")]),
        "affine": strip(cases(tests[("AffineAlignmentTests", "BasicTests")])),
        "affine_large_gap": strip(large)[0],
        "iupac": strip(cases(tests[("IupacAlignmentTests", "BasicTest")])),
        "align_peer": {"target": peer["ref"], "query": peer["read"], "params": [int(x) for x in pm.groups()]},
    }
    with open(dst, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{dst}: " + ", ".join(f"{k} {len(v) if isinstance(v, list) else 1}" for k, v in doc.items() if k != "source"))


if __name__ == "__main__":
    main(sys.argv)

"""What csrc/gen/ap2_jacgen.cpp does to the shooting node's statement order, on the host (no GPU).

On the device sin and cos expand to a branch, which cuts the straight-line node code into basic
blocks; the generator therefore moves a sin / cos of a leaf, with the leaf's load, to the top of the
shooting node's body, where nothing is live yet.  That move must not change the operation graph:
the generator's report keeps the operation counts of the node kinds, the Radau node's body is the
committed one byte for byte, and the shooting body holds no sin / cos below its first other
statement."""
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from awebox_amd import build as B
from awebox_amd import problem as pb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "awebox_amd", "csrc")

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++ to build the generator")


@pytest.fixture(scope="module")
def generated(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("jacgen")
    exe = str(tmp / "ap2_jacgen")
    subprocess.run(["g++", "-O1", "-std=c++17", os.path.join(CSRC, "gen", "ap2_jacgen.cpp"), "-o", exe], check=True)
    np.savetxt(str(tmp / "consts.txt"), pb.build_constants(pb.Ap2Config()).consts)
    out = subprocess.run([exe, str(tmp / "consts.txt"), str(tmp / "gen.hpp")], check=True, capture_output=True,
                         text=True)
    return json.loads(out.stdout), open(str(tmp / "gen.hpp")).read()


def _body(header, name):
    i = header.index("{\n", header.index("void " + name + "(")) + 2
    return header[i:header.index("\n}\n", i) + 1]


def _statements(body):
    return [ln.strip() for ln in body.split("\n") if ln.strip().startswith(("const double v", "tan[", "val["))]


def test_operation_counts_are_those_of_the_node_model(generated):
    report, _ = generated
    s, r = report["shooting"], report["radau"]
    assert (s["flops"], s["transcendental"], s["tangents"]) == (5042, 52, 347)
    assert (r["flops"], r["transcendental"], r["tangents"]) == (5014, 47, 317)


def test_radau_body_is_the_committed_one(generated):
    _, header = generated
    assert _body(header, "ap2_node_radau") == _body(open(B.GEN_HEADER).read(), "ap2_node_radau")


def test_shooting_body_has_its_branching_calls_at_the_top(generated):
    _, header = generated
    st = _statements(_body(header, "ap2_node_shoot"))
    trig = [i for i, s in enumerate(st) if re.search(r"= ::(sin|cos)\(", s)]
    assert trig, "the shooting node's path constraint takes a cosine"
    leaf = re.compile(r"const double v\d+ = (th\[\d+\]|in\(\d+\)|cst\[\d+\]);")
    head = 0
    while head < len(st) and (leaf.match(st[head]) or head in trig):
        head += 1
    assert all(i < head for i in trig), (trig, head)
    # every statement still follows the definitions of what it reads
    seen = set()
    for s in st:
        m = re.match(r"const double (v\d+) = (.*);", s)
        rhs = m.group(2) if m else s.split("=", 1)[1]
        assert set(re.findall(r"\bv\d+\b", rhs)) <= seen, s
        if m:
            seen.add(m.group(1))

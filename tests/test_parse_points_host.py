"""The line routine of ops/hip/parse_points.h (pp_line) under the host
compiler, through tools_dev/points_host_check.cpp: class and extracted
elements per line against json.loads + Aggregator.write, then the same
pools once more under AddressSanitizer + UBSan (a stand-alone program)."""

import os
import shutil
import subprocess

import pytest

from points_pool import (MUST_PUNT, QUERIES, SKIP_DROP, line, required_pool,
                         truth_line)

from dragnet_amd.points import fast_reduce_spec

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SANITIZE = ["-O1", "-g", "-fsanitize=address,undefined",
            "-fno-sanitize-recover=all"]


def _build(out_dir, flags):
    cxx = shutil.which("c++") or shutil.which("g++") or \
        shutil.which("clang++")
    assert cxx, "a host C++ compiler is part of the build contract"
    exe = str(out_dir / "points_host_check")
    subprocess.run(
        [cxx, "-std=c++17"] + flags +
        ["-I", os.path.join(REPO, "dragnet_amd", "ops", "hip"),
         os.path.join(REPO, "tools_dev", "points_host_check.cpp"),
         "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module", params=[["-O2"], SANITIZE],
                ids=["plain", "sanitized"])
def checker(request, tmp_path_factory):
    return _build(tmp_path_factory.mktemp("phc"), request.param)


def _hex(b):
    return b.hex() or "-"


def ask(exe, lines):
    """The checker's answers for `lines` under QUERIES, parsed:
    ("skip",), ("punt",), ("drop", mi) or ("taken", mi, key, value)."""
    req = []
    for q in QUERIES:
        req.append("metric")
        for name, kind, step in fast_reduce_spec(q):
            req.append("col %d %r %s" % (kind, step, _hex(name.encode())))
    req += ["line " + _hex(text) for text in lines]
    res = subprocess.run([exe], input="\n".join(req) + "\n",
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-4000:]
    out = []
    for ans in res.stdout.split("\n")[:-1]:
        w = ans.split(" ")
        if w[0] == "taken":
            key = tuple(int(e[2:]) if e[0] == "i" else
                        bytes.fromhex(e[2:].strip("-")).decode("utf-8")
                        for e in w[3:])
            out.append(("taken", int(w[1]), key, int(w[2])))
        else:
            out.append((w[0],) + tuple(int(x) for x in w[1:]))
    assert len(out) == len(lines)
    return out


@pytest.mark.parametrize("mi", [0, 1, 2])
def test_required_shape_is_never_punted(checker, mi):
    lines = required_pool(mi)
    for text, got in zip(lines, ask(checker, lines)):
        want = truth_line(text)
        assert got == want, text
        if got[0] == "taken":  # int against str: == does not tell True from 1
            assert [type(e) for e in got[2]] == [type(e) for e in want[2]]


def test_must_punt(checker):
    lines = [text for _id, text, _runs in MUST_PUNT]
    lines.append(line(2, [("x", '"%s"' % ("y" * (1 << 18)))]))  # PP_MAX_LINE
    assert ask(checker, lines) == [("punt",)] * len(lines)


def test_skip_and_drop(checker):
    got = ask(checker, [text for text, _cls, _mi in SKIP_DROP])
    for (text, cls, mi), g in zip(SKIP_DROP, got):
        assert g == ((cls,) if cls != "drop" else (cls, mi)), text
        assert g == truth_line(text), text

"""ops/hip/dbl2dec.h under the host compiler, through
tools_dev/dbl2dec_host_check.cpp: dn_js_number of every corpus double
against the independent Number::toString of numeric_cases.py and, for the
golden pairs, against V8's recorded strings; once plain, once under
AddressSanitizer + UBSan (a stand-alone program)."""

import os
import shutil
import struct
import subprocess

import pytest

from dbl2dec_corpus import corpora, golden_pairs
from numeric_cases import js_tostring

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SANITIZE = ["-O1", "-g", "-fsanitize=address,undefined",
            "-fno-sanitize-recover=all"]
CORPORA = corpora()


@pytest.fixture(scope="module", params=[["-O2"], SANITIZE],
                ids=["plain", "sanitized"])
def checker(request, tmp_path_factory):
    cxx = shutil.which("c++") or shutil.which("g++") or \
        shutil.which("clang++")
    assert cxx, "a host C++ compiler is part of the build contract"
    exe = str(tmp_path_factory.mktemp("d2d") / "dbl2dec_host_check")
    subprocess.run(
        [cxx, "-std=c++17"] + request.param +
        ["-I", os.path.join(REPO, "dragnet_amd", "ops", "hip"),
         os.path.join(REPO, "tools_dev", "dbl2dec_host_check.cpp"),
         "-o", exe], check=True)
    return exe


def render(exe, xs):
    inp = "".join(struct.pack(">d", x).hex() + "\n" for x in xs)
    res = subprocess.run([exe], input=inp, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    return res.stdout.split("\n")[:-1]


@pytest.mark.parametrize("name", sorted(CORPORA))
def test_js_number(checker, name):
    xs = CORPORA[name]
    got = render(checker, xs)
    assert len(got) == len(xs)
    for x, g in zip(xs, got):
        assert g == js_tostring(x), x.hex()
    if name == "golden":
        assert got == [s for _x, s in golden_pairs()]

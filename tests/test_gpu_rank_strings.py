"""
rank_strings (ops/hip/rank_strings.h): the rank of every dictionary string
in byte order on the GPU, against Python's sorted() over the bytes.

All tests here require an MI355X (pytest -m gpu).
"""

import numpy as np
import pytest

from dragnet_amd import merge
from dragnet_amd.query import query_load

pytestmark = pytest.mark.gpu

POOL = ["x" * n for n in range(18)] + [
    '"', "\\", 'say "hi"\\', "".join(map(chr, range(0x20))) + "\x7f",
    "é", "z", "Z", "a", "ab", "a\u0000", "€uro", "\U0001F600", "a\U0010FFFFb",
    "éé€€\U0001F600", "abcdefgé", "0123456789abcde€-"]
FIXED = [b"", b"a", b"a\0", b"a\0\0", b"a\0b", b"ab", b"abcdefg",
         b"abcdefgh", b"abcdefg\0", b"\x80", b"\x7f"]


def ops():
    from dragnet_amd.ops import load_ops
    return load_ops(required=True)


def dictionary(kind, G):
    """G distinct byte strings, in no string order."""
    rng = np.random.default_rng(G)
    if kind == "bytes":  # the sign flip, zeros, "", the chunk edges
        alphabet = np.frombuffer(b"\x00\x01\x7f\x80\xffa", np.uint8)
        items = list(dict.fromkeys(
            alphabet[rng.integers(0, 6, rng.integers(0, 21))].tobytes()
            for _ in range(4 * G + 8)))
    elif kind == "pool":
        items = [(POOL[i % len(POOL)] +
                  ("" if i < len(POOL) else str(i))).encode()
                 for i in range(G)]
    else:  # one group above the finish cutoff for seven rounds
        items = [b"p" * 50 + str(i).encode() for i in range(G)]
    items = items[:G]
    assert len(items) == G
    return [items[i] for i in rng.permutation(G)]


def want(items):
    rank = np.empty(len(items), np.int64)
    rank[sorted(range(len(items)), key=items.__getitem__)] = \
        np.arange(len(items))
    return rank.tolist()


def run_op(items, offs=None, lead=0):
    import torch
    raw = b"L" * lead + b"".join(items)
    if offs is None:
        offs = np.cumsum([0] + [len(b) for b in items])
    blob = torch.from_numpy(np.frombuffer(raw, np.uint8).copy()).cuda()[lead:]
    rank, twice = ops().rank_strings(
        blob, torch.from_numpy(np.asarray(offs, np.int64)).cuda())
    return rank.tolist(), twice


@pytest.mark.parametrize("kind", ["bytes", "pool", "prefix"])
@pytest.mark.parametrize("G", [1, 2, 64, 65, 2048, 2049, 5000])
def test_op_equals_sorted(kind, G):
    items = dictionary(kind, G)
    assert run_op(items) == (want(items), False)


@pytest.mark.parametrize("case", ["cutoff", "cutoff+1", "multi-tile",
                                  "fixed0", "fixed1", "fixed2", "fixed3"])
def test_ties(case):
    if case.startswith("cutoff"):  # the two sides of the finish cutoff
        n = ops().RANK_FINISH_MAX + (case == "cutoff+1")
        items = [b"12345678%d" % i for i in range(n)]
    elif case == "multi-tile":  # a later round whose group column varies
        items = [b"fifteen bytes..%d" % i for i in range(2100)] + \
            [b"fifteen", b"fif"] + \
            [b"another fifteen%d" % i for i in range(70)]
    else:
        order = np.random.default_rng(int(case[-1])).permutation(len(FIXED))
        items = [FIXED[i] for i in order]
    assert run_op(items) == (want(items), False)


@pytest.mark.parametrize("items", [
    [b"b", b"a", b"c", b"a"],                                   # round 0
    [b"q" * 28 + b"%02d" % (i % 99) for i in range(100)],       # a later one
    [b"q" * 28 + b"%02d" % (i % 9) for i in range(10)],         # the finish
], ids=["round0", "later", "finish"])
def test_duplicates(monkeypatch, items):
    assert run_op(items)[1]
    strings = [b.decode() for b in items]
    monkeypatch.setenv("DRAGNET_RANK_GPU", "1")
    assert merge.rank_strings(strings) is None
    q = query_load(breakdown_specs="a")
    uniq = np.array([[i, merge._EL_STR] for i in range(len(items))])
    sums = np.arange(1.0, len(items) + 1)
    host = merge.render_points(q, uniq, sums, strings)
    monkeypatch.setenv("DRAGNET_RENDER_GPU", "1")
    assert merge.render_points(q, uniq, sums, strings) == host


def test_op_errors_alignment_and_empty():
    for offs in ([0, 3, 2, 4], [1, 2, 4], [0, 2, 5]):
        with pytest.raises(RuntimeError, match="does not ascend"):
            run_op([b"abcd"], offs=offs)
    items = dictionary("bytes", 300)
    assert run_op(items, lead=1) == (want(items), False)
    rank, twice = run_op([])
    assert rank == [] and not twice


def test_seam_equals_host(monkeypatch):
    import torch
    items = dictionary("pool", 1000)
    strings = [b.decode() for b in items]
    host = merge.rank_strings(strings)
    assert isinstance(host, np.ndarray) and host.tolist() == want(items)
    q = query_load(breakdown_specs="a,b")
    uniq = np.array([[i, (i * 7) % 1000, 5] for i in range(1000)])
    sums = np.arange(1000.0)
    dicts = [strings[:600], strings[400:]]
    parts = [(np.array([[i % len(d), (i * 3) % len(d)] for i in range(700)]),
              np.full(700, 5), np.arange(700.0) % 6) for d in dicts]
    wire = [(np.frombuffer(b, np.uint8).copy(), o)
            for b, o in map(merge._strings_blob, dicts)]
    out = {}
    for mode in ("0", "1"):
        for var in ("UNIFY", "MERGE", "RENDER", "RANK"):
            monkeypatch.setenv("DRAGNET_%s_GPU" % var, mode)
        out[mode] = (merge.render_points(q, uniq, sums, strings),
                     merge.reaggregate_points(q, parts, wire))
    assert out["1"] == out["0"]
    blob, offs = merge._strings_blob(strings)
    pair = (torch.from_numpy(np.frombuffer(blob, np.uint8).copy()).cuda(),
            torch.from_numpy(offs).cuda())
    dev = merge.rank_strings(pair)
    assert dev.is_cuda and dev.tolist() == host.tolist()

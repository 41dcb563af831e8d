"""
render_points (ops/hip/render_points.h): the merged rows as NDJSON point
lines on the GPU, against the host definition: merge._decode_rows,
Aggregator.points() and output.point_json per point, which is pure
json.dumps and uses neither the kernels nor the C++ serializer.

All tests here require an MI355X (pytest -m gpu).
"""

import numpy as np
import pytest

from dragnet_amd import merge
from dragnet_amd.output import point_json
from dragnet_amd.points import Aggregator
from dragnet_amd.query import query_load

pytestmark = pytest.mark.gpu

PLAIN = {1: "a", 2: "a,b", 8: "a,b,c,d,e,f,g,h"}
MIXED = "p,ts[date,field=time],lat[aggr=lquantize,step=10]"
QUANT = "p,ts[date,field=time],lat[aggr=quantize]"

# lengths 0 to 17, the escapes, every control byte, 2-, 3- and 4-byte
# sequences, prefixes and orders that differ from first-seen order
POOL = ["x" * n for n in range(18)] + [
    '"', "\\", 'say "hi"\\', "".join(map(chr, range(0x20))) + "\x7f",
    "é", "z", "Z", "a", "ab", "a\u0000", "€uro", "\U0001F600", "a\U0010FFFFb",
    "éé€€\U0001F600", "abcdefgé", "0123456789abcde€-"]


def encoded(spec, table):
    """(query, uniq, sums, strings) of a table {key tuple: value}: the
    rows in np.unique's order, string codes in first-seen order."""
    q = query_load(breakdown_specs=spec)
    agg = Aggregator(q)
    agg.table.update(table)
    codes, tags, vals, strings = merge._encode_table(agg, len(q.breakdowns))
    uniq, sums = merge._group_host(
        np.concatenate([codes, tags[:, None]], axis=1), vals)
    return q, uniq, sums, strings


def check(monkeypatch, spec, table, refused=False):
    q, uniq, sums, strings = encoded(spec, table)
    want = "".join(point_json(p) + "\n" for p in merge._decode_rows(
        q, uniq, sums, strings).points()).encode()
    got = merge._render_device(q, uniq, sums, strings, None)
    assert got is None if refused else got == want
    monkeypatch.setenv("DRAGNET_RENDER_GPU", "1")
    assert merge.render_points(q, uniq, sums, strings) == want
    return want


def string_key(i, nk):
    first = POOL[i % len(POOL)] + ("" if i < len(POOL) else str(i))
    return (first,) + tuple(POOL[(i * (j + 2) + j) % len(POOL)]
                            for j in range(1, nk))


@pytest.mark.parametrize("nk", [1, 2, 8])
@pytest.mark.parametrize("g", [1, 255, 256, 257, 1000])
def test_string_tables(monkeypatch, g, nk):
    check(monkeypatch, PLAIN[nk],
          {string_key(i, nk): i * 7 + 1 for i in range(g)})


@pytest.mark.parametrize("spec", [MIXED, QUANT])
@pytest.mark.parametrize("g", [1, 257, 1000])
def test_mixed_tables(monkeypatch, spec, g):
    # negative dates; ordinals -1 to 63, the most a quantize column holds
    check(monkeypatch, spec,
          {(POOL[i % 5 + 20], (i - g // 2) * 86400000, i % 65 - 1): i
           for i in range(g)})


def test_order_and_ties(monkeypatch):
    names = ["a", "ab", "a\u0000", "Z", "z", "é", ""]
    want = check(monkeypatch, 'x"y é,b\\c',
                 {(s, t): 1 for s in names for t in reversed(names)})
    assert want.startswith(b'{"fields":{"x\\"y \\u00e9":"","b\\\\c":""}')
    check(monkeypatch, "ts[date,field=time],a",
          {(d, s): 2 for d in (5, -86400000, 0, -1) for s in ("b", "a")})


@pytest.mark.parametrize("v", [0, 1, 2**53 - 1, 2**53, 2**62, -3, -0.0])
def test_values(monkeypatch, v):
    check(monkeypatch, "a", {("k",): v, ("l",): 1})


def test_oversize_tiles(monkeypatch):
    # 5000 control bytes escape to 30002: beside 255 other strings that
    # is more than the escape kernel's output stage, and two such lines
    # in a tile are more than the emit kernel's
    big = "\x01" * 5000
    table = {("key-%012d" % i, big if i % 100 == 0 else "s"): i
             for i in range(300)}
    table[(big, big)] = 9
    check(monkeypatch, "a,b", table)


@pytest.mark.parametrize("spec,table", [
    ("a", {("k",): 0.5}), ("a", {("k",): float("nan")}),
    ("a", {("k",): float("inf")}), ("a", {("k",): 2.0**63}),
    (QUANT, {("p", 0, 64): 1, ("p", 0, 63): 1}),
    (MIXED, {("p", 0, 2**62): 1, ("p", 0, -5): 1}),
    ("a", {(1.5,): 1}), ("a", {("k",): 1, (3,): 2})])
def test_refusals_take_the_host_path(monkeypatch, spec, table):
    check(monkeypatch, spec, table, refused=True)


def wire(strings):
    blob, offs = merge._strings_blob(strings)
    return np.frombuffer(blob, np.uint8).copy(), offs


def raw_op(rows, strings, order=None):
    import torch

    from dragnet_amd.ops import load_ops
    blob, offs = strings
    segs = [b'{"fields":{"a":', b'},"value":', b"}\n"]

    def dev(a, dtype):
        return torch.from_numpy(np.array(a, dtype=dtype)).cuda()

    return load_ops(required=True).render_points(
        dev(rows, np.int64), dev(np.ones(len(rows)), np.float64),
        None if order is None else dev(order, np.int32),
        dev(np.frombuffer(blob, np.uint8), np.uint8), dev(offs, np.int64),
        [0], [0], dev(np.frombuffer(b"".join(segs), np.uint8), np.uint8),
        dev(np.cumsum([0] + [len(s) for s in segs]), np.int64))


def test_op_refuses_and_raises():
    two = (b"abcd", np.array([0, 2, 4]))
    text, line_off, refused = raw_op([[1, 1], [0, 1]], two, order=[1, 0])
    assert not refused and line_off.tolist() == [0, 32, 64]
    assert bytes(text.cpu().numpy()) == \
        b'{"fields":{"a":"ab"},"value":1}\n{"fields":{"a":"cd"},"value":1}\n'
    assert raw_op([[0, merge._EL_F64]], two)[2]
    with pytest.raises(RuntimeError, match="outside the dictionary"):
        raw_op([[0, 1], [2, 1]], two)
    with pytest.raises(RuntimeError, match="ill-formed UTF-8"):
        raw_op([[0, 1]], (b"ab\xed\xa0\x80", np.array([0, 5])))
    with pytest.raises(RuntimeError, match="order entry"):
        raw_op([[0, 1], [1, 1]], two, order=[0, 2])
    with pytest.raises(RuntimeError, match="none of INT, STR and F64"):
        raw_op([[0, 3]], two)


def test_empty(monkeypatch):
    monkeypatch.setenv("DRAGNET_RENDER_GPU", "1")
    q = query_load(breakdown_specs="a")
    assert merge.render_points(q, np.zeros((0, 2), np.int64),
                               np.zeros(0), []) == b""
    assert raw_op(np.zeros((0, 2)), wire([]))[0].numel() == 0


def test_reaggregate_points_device_equals_host(monkeypatch):
    q = query_load(breakdown_specs="a,b")
    dicts = [["x", "é", "z"], ["z", "x\n", "é"], ["q", "x"]]
    parts = [(np.array([[i % len(d), (i + 1) % len(d)] for i in range(40)]),
              np.full(40, 5), np.arange(40.0) % 6) for d in dicts]
    out = {}
    for mode in ("1", "0"):
        for var in ("UNIFY", "MERGE", "RENDER"):
            monkeypatch.setenv("DRAGNET_%s_GPU" % var, mode)
        out[mode] = merge.reaggregate_points(
            q, parts, [wire(d) for d in dicts])
    assert out["1"] == out["0"] == "".join(
        point_json(p) + "\n"
        for p in merge.reaggregate(q, parts, dicts).points()).encode()

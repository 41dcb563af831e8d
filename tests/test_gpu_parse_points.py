"""merge.parse_points / merge.reduce_points (ops/hip/parse_points.h)
against the pure-Python loop of cmd_index_read (points_pool.truth): the
device result plus the oracle over its punts equals the truth in tables
(with key and value types), ninputs and ndropped_nonnumeric."""

import io

import pytest

from points_pool import (MUST_PUNT, QUERIES, SKIP_DROP, line, required_pool,
                         same, truth, truth_line)

from dragnet_amd import merge
from dragnet_amd.points import Aggregator, reduce_tagged_stream

pytestmark = pytest.mark.gpu

CLS = {"skip": merge.PARSE_SKIP, "drop": merge.PARSE_DROP,
       "taken": merge.PARSE_TAKEN, "punt": merge.PARSE_PUNT}


def classes(data):
    return merge.parse_points(data, QUERIES)[3].cpu().tolist()


def oracle(aggs, punted):
    """The per-line Python path over the punted lines, added into aggs."""
    for a, b in zip(aggs, truth(b"\n".join(punted))):
        a.ninputs += b.ninputs
        a.ndropped_nonnumeric += b.ndropped_nonnumeric
        for k, v in b.table.items():
            a.table[k] = a.table.get(k, 0) + v
    return aggs


def reduced(data):
    """reduce_points, then the oracle over what it punted."""
    aggs = [Aggregator(q) for q in QUERIES]
    punted = merge.reduce_points(data, aggs, QUERIES)
    assert punted is not None
    return oracle(aggs, punted)


@pytest.mark.parametrize("mi", [0, 1, 2])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 1000])
def test_tile_edges(n, mi):
    pool = required_pool(mi)
    data = b"\n".join(pool[i % len(pool)] for i in range(n)) + b"\n"
    cls = classes(data)
    assert len(cls) == n and merge.PARSE_PUNT not in cls
    assert merge.PARSE_TAKEN in cls
    same(reduced(data), truth(data))


def _long(nbytes):
    return line(1, [("req.method", '"%s"' % ("m" * nbytes))])


# one line of 60 KB among short ones: the first tile of 256 lines does not
# fit the stage and is parsed from global memory, every pool and the skip
# and drop lines in it; the second tile is staged again
WIDE = [_long(60000)] + required_pool(0) + required_pool(1) + \
    required_pool(2) + [text for text, _cls, _mi in SKIP_DROP]
WIDE += required_pool(1)[:1] * (256 - len(WIDE)) + required_pool(0)

STAGING = {
    "beyond-the-stage": (b"\n".join(WIDE) + b"\n",
                         [truth_line(text)[0] for text in WIDE]),
    # PP_MAX_LINE: the line is punted, its neighbours are not
    "over-max-line": (b"\n".join(
        [required_pool(1)[0], _long(1 << 18), required_pool(1)[1]]) + b"\n",
        ["taken", "punt", "taken"]),
    "no-trailing-newline": (b"\n".join(required_pool(1)[:3]),
                            ["taken"] * 3),
    "crlf": (b"\r\n".join(required_pool(1)[:3]) + b"\r\n", ["taken"] * 3),
    "blank-lines": (b"\n\n  \n" + required_pool(2)[0] + b"\n\t\r\n\n",
                    ["skip", "skip", "skip", "taken", "skip", "skip"]),
    "empty": (b"", []),
    "one-newline": (b"\n", ["skip"]),
}


@pytest.mark.parametrize("case", sorted(STAGING))
def test_staging_edges(case):
    data, want = STAGING[case]
    cls = classes(data)
    assert cls == [CLS[w] for w in want]
    same(reduced(data), truth(data))


@pytest.mark.parametrize("case", MUST_PUNT, ids=[c[0] for c in MUST_PUNT])
def test_must_punt(case):
    _id, text, truth_runs = case
    data = required_pool(1)[0] + b"\n" + text + b"\n"
    assert classes(data) == [merge.PARSE_TAKEN, merge.PARSE_PUNT]
    tables, counters, punted, _cls = merge.parse_points(data, QUERIES)
    assert punted == [text] and counters.sum() == 1
    if truth_runs:
        same(reduced(data), truth(data))


def test_skip_and_drop():
    data = b"\n".join(text for text, _cls, _mi in SKIP_DROP) + b"\n"
    _tables, counters, _punted, cls = merge.parse_points(data, QUERIES)
    assert cls.cpu().tolist() == [CLS[c] for _t, c, _mi in SKIP_DROP]
    drops = sum(1 for _t, c, _mi in SKIP_DROP if c == "drop")
    assert counters.tolist() == [[drops, drops], [0, 0], [0, 0]]
    same(reduced(data), truth(data))


def test_span_form():
    data = b"\n".join([
        line(0, [("a", '"xé"'), ("t", "true"), ("lat", "1"),
                 ("ts", "1")]),
        line(1, [("res.statusCode", "-17")], spaced=True),
        line(0, [("a", "null"), ("t", "5"), ("lat", "1"), ("ts", "1")]),
        line(1, [("req.method", '""'), ("res.statusCode", "false")]),
    ]) + b"\n"
    tables, _counters, punted, _cls = merge.parse_points(data, QUERIES)
    text, start, length = tables[0].strings
    raw = text.cpu().numpy().tobytes()
    assert raw == data + b"undefined"
    start, length = start.tolist(), length.tolist()
    spans = [raw[a:a + n].decode("utf-8") for a, n in zip(start, length)]
    assert spans == ["xé", "true", "undefined", "-17", "null", "",
                     "false"]
    inside = [a for a in start if a < len(data)]
    assert inside == sorted(inside) and punted == []
    assert tables[0].codes.tolist() == [[0, 1, 1, 0], [4, 5, 1, 0]]
    assert tables[1].codes.tolist() == [[2, 3], [5, 6]]
    assert tables[0].tagpack.tolist() == [0b0101, 0b0001]
    assert tables[1].vals.tolist() == [1.0, 1.0]


def test_inexact_chunk_goes_to_the_host_whole(monkeypatch):
    big = line(1, [("req.method", '"GET"')], value=2 ** 52)
    data = big + b"\n" + required_pool(1)[0] + b"\n" + big + b"\n"
    aggs = [Aggregator(q) for q in QUERIES]
    assert merge.reduce_points(data, aggs, QUERIES) is None
    assert all(a.ninputs == 0 and not a.table for a in aggs)
    monkeypatch.setenv("DRAGNET_PARSE_GPU", "1")
    assert reduce_tagged_stream(io.BytesIO(data), aggs, QUERIES) == []
    same(aggs, truth(data))


def test_policy(monkeypatch):
    data = b"\n".join(required_pool(0) + required_pool(1) +
                      [MUST_PUNT[0][1], MUST_PUNT[2][1]]) + b"\n"
    got = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("DRAGNET_PARSE_GPU", mode)
        aggs = [Aggregator(q) for q in QUERIES]
        punted = reduce_tagged_stream(io.BytesIO(data), aggs, QUERIES)
        assert MUST_PUNT[0][1] in punted and MUST_PUNT[2][1] in punted
        got[mode] = oracle(aggs, punted)  # the host punts 1e999, say
    same(got["1"], got["0"])
    same(got["1"], truth(data))

"""Host-side decode of a GPU extraction snapshot (engine/decode.py):
hand-built snapshots, no GPU and no extension (CPU-only)."""

import os

import numpy as np

from dragnet_amd.engine import decode
from dragnet_amd.engine import plan as planmod
from dragnet_amd.query import query_load

P = planmod


def code(tag, val):
    return (tag << 30) | val


def snapshot(nm=1, strings=(), numbers=(), rows=(), counters=None):
    """A `host` dict: `strings` (raw in-record bytes, in id order),
    `numbers`, and per metric a list of (codes, value) rows."""
    cnt = np.zeros(decode.C_GLOBAL_N + nm * decode.CM_N, dtype=np.int64)
    for slot, v in (counters or {}).items():
        cnt[slot] = v
    host = {"cnt": cnt, "n_str": len(strings), "n_num": len(numbers),
            "aggs": []}
    if strings:
        lens = [len(s) for s in strings]
        # payloads sit in 8-byte granules, as the device stores them
        offs = np.cumsum([0] + [(n + 7) & ~7 for n in lens[:-1]])
        blob = np.zeros(int(offs[-1]) + lens[-1], dtype=np.uint8)
        for o, s in zip(offs, strings):
            blob[o:o + len(s)] = np.frombuffer(s, dtype=np.uint8)
        host.update(str_off=offs.astype(np.int32),
                    str_len=np.array(lens, dtype=np.int32), blob=blob)
    if numbers:
        host["numbers"] = np.array(numbers, dtype=np.float64)
    for m in range(nm):
        mrows = rows[m] if rows else []
        keys = np.full((len(mrows), planmod.MAX_KEY), planmod.EMPTY_CODE,
                       dtype=np.uint32)
        for i, (codes, _v) in enumerate(mrows):
            keys[i, :len(codes)] = codes
        # the device tensors are int32: the host sees the same bits
        host["aggs"].append((keys.view(np.int32), np.array(
            [v for _c, v in mrows], dtype=np.float64)))
    return host


def test_key_codes_of_every_tag():
    q2 = query_load(breakdown_specs="a,b")
    qb = query_load(breakdown_specs="latency[aggr=quantize]")
    cplan = planmod.compile_plan([q2, qb])
    strings = [b"GET", b"[1,\"x\"]", b"[1,", b"caf\\u00e9"]
    numbers = [200.0, 2.0 ** 53 - 1, 2.0 ** 53, 0.25, 1e9]
    sp = [code(P.TAG_SPECIAL, v) for v in (
        P.SPECIAL_NULL, P.SPECIAL_UNDEF, P.SPECIAL_TRUE, P.SPECIAL_FALSE,
        P.SPECIAL_OBJECT, P.SPECIAL_ARRAY)]
    rows_a = [
        ([code(P.TAG_STR, 0), code(P.TAG_NUM, 0)], 3.0),
        ([code(P.TAG_STR, 3), code(P.TAG_NUM, 1)], 2.5),
        ([code(P.TAG_NUM, 2), code(P.TAG_NUM, 3)], 1.0),
        ([sp[0], sp[1]], 4.0),
        ([sp[2], sp[3]], 5.0),
        ([sp[4], sp[5]], 6.0),
        ([code(P.TAG_SPECIAL, P.SPECIAL_ARRJSON | (1 << 3)),
          code(P.TAG_SPECIAL, P.SPECIAL_ARRJSON | (2 << 3))], 7.0),
    ]
    rows_b = [
        ([code(P.TAG_ORD, P.ORD_BIAS + 5)], 2.0),
        ([code(P.TAG_ORD, P.ORD_BIAS - 1)], 1.5),
        ([code(P.TAG_NUM, 4)], 1.0),
    ]
    host = snapshot(2, strings, numbers, [rows_a, rows_b], {
        decode.C_GLOBAL_N + decode.CM_AGG_IN: 29,
        decode.C_GLOBAL_N + decode.CM_N + decode.CM_AGG_IN: 5,
        decode.C_GLOBAL_N + decode.CM_N + decode.CM_NONNUMERIC: 2})
    aggs, _stages = decode.decode_snapshot(host, [q2, qb], cplan)

    dstrings = ["GET", '[1,"x"]', "[1,", "café"]
    dnumbers = np.array(numbers)
    for agg, q, rows in ((aggs[0], q2, rows_a), (aggs[1], qb, rows_b)):
        want = {planmod.decode_key(c, q, dstrings, dnumbers): v
                for c, v in rows}
        assert len(want) == len(rows)
        assert agg.table == want
    # spot checks of what decode_key gives, so that the loop above cannot
    # agree with itself on nonsense
    t = aggs[0].table
    assert t[("GET", "200")] == 3 and type(t[("GET", "200")]) is int
    assert t[("café", "9007199254740991")] == 2.5
    assert type(t[("café", "9007199254740991")]) is float
    assert t[("9007199254740992", "0.25")] == 1
    assert t[("null", "undefined")] == 4
    assert t[("true", "false")] == 5
    assert t[("[object Object]", "<array>")] == 6
    assert t[("1,x", "[1,")] == 7  # valid array JSON / payload as it is
    assert aggs[1].table == {(5,): 2, (-1,): 1.5, (1000000000,): 1}
    assert aggs[0].ninputs == 29 and aggs[0].ndropped_nonnumeric == 0
    assert aggs[1].ninputs == 5 and aggs[1].ndropped_nonnumeric == 2


def test_duplicate_string_ids_merge():
    """Two lanes interning a string at the same moment can both insert
    it: two ids, identical bytes.  Rows that differ only in that id are
    one group."""
    q = query_load(breakdown_specs="a,b")
    host = snapshot(1, [b"/index.html", b"/about", b"/index.html"], [404.0],
                    [[([code(P.TAG_STR, 0), code(P.TAG_NUM, 0)], 3.0),
                      ([code(P.TAG_STR, 1), code(P.TAG_NUM, 0)], 1.0),
                      ([code(P.TAG_STR, 2), code(P.TAG_NUM, 0)], 4.5)]])
    strings, numbers = decode.decode_dicts(host)
    assert strings == ["/index.html", "/about", "/index.html"]
    assert numbers.tolist() == [404.0]
    aggs, _stages = decode.decode_snapshot(
        host, [q], planmod.compile_plan([q]))
    assert aggs[0].table == {("/index.html", "404"): 7.5,
                             ("/about", "404"): 1}


def test_decode_json_string():
    d = decode.decode_json_string
    assert d("plain café".encode("utf-8")) == "plain café"
    assert d(b"caf\\u00e9 \\n \\\"q\\\"") == "café \n \"q\""
    assert d(b"\\ud83d\\ude00") == "\U0001F600"
    assert d(b"bad \\x escape") == "bad \\x escape"
    assert d(b"ab\xff\xfecd") == "ab��cd"


def _oracle_counters(stages, nm=1):
    """The device counter array that would give the oracle's stages."""
    cnt = np.zeros(decode.C_GLOBAL_N + nm * decode.CM_N, dtype=np.int64)
    mc = cnt[decode.C_GLOBAL_N:]
    by = dict(stages)
    cnt[decode.C_LINES] = by["json parser"]["ninputs"]
    cnt[decode.C_PARSED] = by["json parser"]["noutputs"]
    cnt[decode.C_INVALID_JSON] = by["json parser"]["invalid json"]
    mc[decode.CM_FILTER_IN] = by["json parser"]["noutputs"]
    if "Datasource filter" in by:
        cnt[decode.C_DS_FILTERED] = by["Datasource filter"]["nfilteredout"]
        cnt[decode.C_DS_FAILEDEVAL] = by["Datasource filter"]["nfailedeval"]
        mc[decode.CM_FILTER_IN] = by["Datasource filter"]["noutputs"]
    if "User filter" in by:
        mc[decode.CM_FILTERED] = by["User filter"]["nfilteredout"]
        mc[decode.CM_FAILEDEVAL] = by["User filter"]["nfailedeval"]
    if "Datetime parser" in by:
        mc[decode.CM_UNDEF] = by["Datetime parser"]["undef"]
        mc[decode.CM_BADDATE] = by["Datetime parser"]["baddate"]
    if "Time filter" in by:
        mc[decode.CM_TIME_OUT] = by["Time filter"]["nfilteredout"]
    mc[decode.CM_AGG_IN] = by["Aggregator"]["ninputs"]
    mc[decode.CM_NONNUMERIC] = by["Aggregator"]["nonnumeric"]
    return cnt


def test_counter_stages_against_oracle(fixture_tree):
    from dragnet_amd.engine.cpu import CpuEngine
    files = sorted(os.path.join(root, n)
                   for root, _dirs, names in os.walk(fixture_tree)
                   for n in names)
    dated = dict(
        breakdown_specs="ts[date,field=time,aggr=lquantize,step=3600],"
                        "latency[aggr=quantize]",
        time_after="2014-05-02T06:00:00", time_before="2014-05-04")
    cases = [
        (query_load(**dated), None,
         ["json parser", "SkinnerAdapterStream", "Datetime parser",
          "Time filter", "Aggregator"]),
        (query_load(filter={"eq": ["req.method", "GET"]}, **dated),
         {"ne": ["operation", "getjoberrors"]},
         ["json parser", "SkinnerAdapterStream", "Datasource filter",
          "User filter", "Datetime parser", "Time filter", "Aggregator"]),
    ]
    for q, ds_filter, names in cases:
        res = CpuEngine().scan(files, [q], ds_filter=ds_filter,
                               time_field="time")
        want = [(n, dict(c)) for n, c in res.stages]
        assert [n for n, _c in want] == names
        by = dict(want)
        assert by["json parser"]["invalid json"] == 2
        assert by["Time filter"]["nfilteredout"]
        if ds_filter is None:
            assert by["Datetime parser"]["undef"] == 1
            assert by["Datetime parser"]["baddate"] == 1
        else:
            assert by["Datasource filter"]["nfilteredout"]
            assert by["User filter"]["nfilteredout"]
        assert by["Aggregator"]["noutputs"] > 0
        by["Aggregator"]["noutputs"] = 0  # the caller patches it
        cplan = planmod.compile_plan([q], ds_filter=ds_filter,
                                     time_field="time")
        got = decode.counter_stages(_oracle_counters(want), cplan, [q])
        assert got == want


def test_empty_snapshot():
    qs = [query_load(breakdown_specs="a,b"),
          query_load(breakdown_specs="latency[aggr=quantize]")]
    host = snapshot(2)
    assert host["n_str"] == host["n_num"] == 0
    strings, numbers = decode.decode_dicts(host)
    assert strings == [] and numbers.shape == (0,)
    aggs, stages = decode.decode_snapshot(
        host, qs, planmod.compile_plan(qs))
    assert [a.table for a in aggs] == [{}, {}]
    assert [(a.ninputs, a.ndropped_nonnumeric) for a in aggs] == [(0, 0)] * 2
    assert [n for n, _c in stages] == [
        "json parser", "SkinnerAdapterStream", "Aggregator"]
    assert all(v == 0 for _n, c in stages for v in c.values())

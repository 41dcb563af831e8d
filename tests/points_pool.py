"""Tagged point lines for the parse_points tests (test_parse_points_host,
test_gpu_parse_points) and their truth: json.loads plus Aggregator.write,
the loop of cli.cmd_index_read, which uses neither the kernels nor the
C++ reducer.  Values are integers, so sums have no order."""

import json

from dragnet_amd.points import Aggregator
from dragnet_amd.query import query_load

# the query sets of test_points_fast.py
QUERIES = [
    query_load(breakdown_specs="a,t[date,field=time],"
                               "lat[aggr=quantize],"
                               "ts[aggr=lquantize,step=60]"),
    query_load(breakdown_specs="req.method,res.statusCode"),
    query_load(),  # zero breakdowns
]

STRINGS = ["abcdefghijklmnopq"[:n] for n in range(18)] + [
    "é", "€", "\U0001F600", "xéy€\U0001F600z", "\x7f"]


def line(mi, items, value=1, spaced=False, value_first=False):
    """One point line.  items is a list of (name, json text) pairs, so a
    name may come twice; spaced is json.dumps' default separators."""
    comma, colon = (", ", ": ") if spaced else (",", ":")
    pairs = [("__dn_metric", json.dumps(mi))] + list(items)
    fields = '"fields"%s{%s}' % (colon, comma.join(
        json.dumps(k, ensure_ascii=False) + colon + v for k, v in pairs))
    val = '"value"%s%s' % (colon, json.dumps(value))
    return ("{%s}" % comma.join(
        [val, fields] if value_first else [fields, val])).encode("utf-8")


def _s(x):
    return json.dumps(x, ensure_ascii=False)


def required_pool(mi):
    """Lines in the required shape for metric mi: every one is TAKEN or
    DROPPED, none may be punted."""
    out = []
    if mi == 0:
        dates = ["1400000000", "-86400", "1400000000.9", "-1.5e3", "0",
                 "true", "null", '"soon"']
        # 17 digits and 1e23 take dn_dec2dbl's slow path
        lats = ["0", "1", "26", "3.5", "1e3", "0.25", "-7", "1024",
                "9007199254740992", "null", "true", "1e999",
                "12345678901234567e-3", "1e23", "0.0001e311", "9.9e307"]
        tss = ["61", "-61.5", "0", "600", "59.999", "-0", "1.2e2"]
        plains = [_s(s) for s in STRINGS] + [
            "true", "false", "null", "7", "-3", "1099511627776"]
        for i, a in enumerate(plains):
            items = [("a", a), ("t", dates[i % len(dates)]),
                     ("lat", lats[i % len(lats)]),
                     ("ts", tss[i % len(tss)])]
            if i % 5 == 1:
                items.pop(i % 4)                        # a missing field
            if i % 7 == 2:
                items.insert(0, ("a", '"first"'))       # the last one wins
            if i % 9 == 3:
                items.append(("junk", _s(STRINGS[i % len(STRINGS)])))
            out.append(line(0, items, value=1 + i % 5, spaced=i % 2 == 1,
                            value_first=i % 3 == 2))
    elif mi == 1:
        codes = ["200", "-17", '"200"', "null", "false", "9007199254740992"]
        for i, s in enumerate(STRINGS):
            items = [("req.method", _s(s)),
                     ("res.statusCode", codes[i % len(codes)])]
            if i % 4 == 3:
                items.pop(i % 2)
            out.append(line(1, items, value=2 + i % 3, spaced=i % 2 == 0,
                            value_first=i % 5 == 4))
    else:
        for i in range(6):
            out.append(line(2, [("unrelated", _s(STRINGS[3 * i]))][:i % 2],
                            value=i, spaced=i % 2 == 1,
                            value_first=i % 3 == 1))
    return out


_M0 = [("a", '"k"'), ("t", "1"), ("lat", "1"), ("ts", "1")]


def _m0(**over):
    return [(k, over.get(k, v)) for k, v in _M0]


# One line per item of the issue's "must punt" list: (id, line, whether
# the truth can run it; a missing value is a KeyError in cmd_index_read).
MUST_PUNT = [
    ("escape", line(0, _m0(a='"x\\ny"')), True),
    ("escape-in-name", line(0, _M0 + [("b\\u0061", "1")]), True),
    ("nested", line(0, _m0(a='{"z":1}')), True),
    ("array", line(0, _m0(a='[1,"b"]')), True),
    ("dup-fields", b'{"fields":{"__dn_metric":2},"fields":{"__dn_metric":2},'
                   b'"value":1}', True),
    ("dup-value", b'{"fields":{"__dn_metric":2},"value":1,"value":2}', True),
    ("other-key", b'{"fields":{"__dn_metric":2},"value":1,"extra":1}', True),
    ("no-value", b'{"fields":{"__dn_metric":2}}', False),
    ("value-float", line(2, [], value=2.5), True),
    ("value-negative", line(2, [], value=-1), True),
    ("value-2^53", line(2, [], value=2 ** 53), True),
    ("value-string", b'{"fields":{"__dn_metric":2},"value":"1"}', False),
    ("plain-float", line(0, _m0(a="2.5")), True),
    ("plain-exponent", line(0, _m0(a="1e2")), True),
    ("plain-float-before-drop", line(0, _m0(lat="null", a="2.5")), True),
    ("plain-minus-zero", line(0, _m0(a="-0")), True),
    ("plain-big-int", line(0, _m0(a="9007199254740993")), True),
    ("20-digits", line(0, _m0(lat="1.2345678901234567890")), True),
    ("lquantize-2^62", line(0, _m0(ts="1e300")), True),
    ("near-overflow", line(0, _m0(lat="1.7e308")), True),
    ("trailing", line(0, _M0) + b" x", True),
    ("bad-utf8", line(0, _m0(a='"\\u00e9"')).replace(b"\\u00e9", b"\xe9"),
     True),
    ("surrogate", line(0, _m0(a='"Z"')).replace(b"Z", b"\xed\xa0\x80"),
     False),
    ("bucket-string", line(0, _m0(lat='"26"')), True),
    ("metric-bool", line(True, _M0), True),
]

# (line, class, metric): what is neither taken nor punted
SKIP_DROP = [
    (b'{"fields":{"a":"x"},"value":1}', "skip", None),
    (b'{"fields":{"__dn_metric":1.5,"a":"x"},"value":1}', "skip", None),
    (b'{"fields":{"__dn_metric":3,"a":"x"},"value":1}', "skip", None),
    (b'{"fields":{"__dn_metric":-1,"a":"x"},"value":1}', "skip", None),
    (b'{"fields":{"__dn_metric":"0"},"value":1}', "skip", None),
    (b'{"fields":{"__dn_metric":123456789012345678901},"value":1}', "skip",
     None),
    (b"{}", "skip", None),
    (b'{"value":1}', "skip", None),
    (b"   \t", "skip", None),
    (line(0, _m0(lat="null")), "drop", 0),
    (line(0, _m0(lat="true")), "drop", 0),
    (line(0, _m0(ts="false")), "drop", 0),
    (line(0, _M0[:3]), "drop", 0),                   # ts missing
    (line(0, _m0(lat="1e999")), "drop", 0),          # infinity
    (line(0, _m0(lat="null", ts='"x"')), "drop", 0),  # drops before ts
]


def truth_line(text, queries=QUERIES):
    """What cmd_index_read does with one line: ("skip",), ("drop", mi) or
    ("taken", mi, key tuple, value)."""
    text = text.strip()
    if not text:
        return ("skip",)
    try:
        p = json.loads(text)
    except ValueError:
        return ("skip",)
    mi = p.get("fields", {}).get("__dn_metric")
    if not isinstance(mi, int) or not 0 <= mi < len(queries):
        return ("skip",)
    agg = Aggregator(queries[mi])
    if not agg.write(p):
        return ("drop", int(mi))
    (key, value), = agg.table.items()
    return ("taken", int(mi), key, value)


def truth(data, queries=QUERIES):
    """py_reduce of test_points_fast.py."""
    aggs = [Aggregator(q) for q in queries]
    for text in data.split(b"\n"):
        got = truth_line(text, queries)
        if got[0] != "skip":
            aggs[got[1]].write(json.loads(text))
    return aggs


def same(got, want):
    """Tables with key and value types, ninputs, ndropped_nonnumeric."""
    for i, (a, b) in enumerate(zip(got, want)):
        assert a.ninputs == b.ninputs, i
        assert a.ndropped_nonnumeric == b.ndropped_nonnumeric, i
        assert a.table == b.table, (i, a.table, b.table)
        typed = lambda t: sorted(  # noqa: E731
            (repr(k), [type(e) for e in k], type(v)) for k, v in t.items())
        assert typed(a.table) == typed(b.table), i

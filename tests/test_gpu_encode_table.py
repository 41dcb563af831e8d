"""
encode_table (ops/hip/encode_table.h): one metric of a scan's extraction
to the merge's wire form on the GPU, against the host definition:
decode.decode_snapshot on the same arrays.  The device table goes
through merge.reaggregate and must give the reference Aggregator's table
exactly.  The snapshots are synthetic, so no scan is needed but for the
seam test.

All tests here require an MI355X (pytest -m gpu).
"""

import numpy as np
import pytest

from dragnet_amd import merge
from dragnet_amd.engine import decode
from dragnet_amd.engine import plan as P
from dragnet_amd.query import query_load

pytestmark = pytest.mark.gpu

PLAIN = {1: "a", 2: "a,b", 8: "a,b,c,d,e,f,g,h"}
MIXED = "p,ts[date,field=time],lat[aggr=lquantize,step=10]"
S, N, O, X = P.TAG_STR << 30, P.TAG_NUM << 30, P.TAG_ORD << 30, \
    P.TAG_SPECIAL << 30


def snapshot(rows, strings=(), numbers=(), pad=0, spare=5):
    """(host dict for decode_snapshot, the same as extract_all's device
    dict) of rows [(codes, count)], with `spare` garbage entries beyond
    every count and `pad` bytes in front of the first string."""
    import torch
    n, n_str, n_num = len(rows), len(strings), len(numbers)
    keys = np.full((n + spare, 8), 0xFFFFFFFF, dtype=np.uint32)
    counts = np.full(n + spare, np.nan)
    for i, (codes, v) in enumerate(rows):
        keys[i, :len(codes)] = codes
        counts[i] = v
    lens = [len(s) for s in strings]
    off = np.full(n_str + spare, 0xFFFFFF00, dtype=np.uint32)
    ln = np.full(n_str + spare, 77, dtype=np.uint32)
    off[:n_str] = pad + np.concatenate([[0], np.cumsum(lens)])[:n_str]
    ln[:n_str] = lens
    blob = np.frombuffer(b"#" * pad + b"".join(strings) + b"@" * 40,
                         dtype=np.uint8).copy()
    used = pad + sum(lens)  # the last string ends exactly there
    nums = np.concatenate([np.asarray(numbers, dtype=np.float64),
                           np.full(spare, 7.25)])
    host = {"cnt": np.zeros(decode.C_GLOBAL_N + decode.CM_N, np.int64),
            "n_str": n_str, "n_num": n_num, "str_off": off[:n_str],
            "str_len": ln[:n_str], "blob": blob[:used],
            "numbers": nums[:n_num], "aggs": [(keys[:n], counts[:n])]}

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a)).cuda()

    def i32(a):
        return dev(np.asarray(a, dtype=np.uint32).view(np.int32))

    return host, {
        "aggs": [(i32(keys), dev(counts), i32([n]))], "str_off": i32(off),
        "str_len": i32(ln), "n_str": i32([n_str]), "blob": dev(blob),
        "used": i32([used]), "numbers": dev(nums), "n_num": i32([n_num])}


def typed(table):
    """Keys and values with their types; a key number beyond int64
    travels as a float (merge._encode_table) and compares as one."""
    def el(e):
        if isinstance(e, str) or (type(e) is int and -2**63 <= e < 2**63):
            return e
        return ("f64", float(e))
    return {tuple(map(el, k)): (v, type(v)) for k, v in table.items()}


def raw_op(dev, q):
    from dragnet_amd.ops import load_ops
    k, c, n = dev["aggs"][0]
    return load_ops(required=True).encode_table(
        k, c, n, dev["str_off"], dev["str_len"], dev["n_str"], dev["blob"],
        dev["used"], dev["numbers"], dev["n_num"], merge.col_kinds(q))


def check(spec, rows, strings=(), numbers=(), exceptions=None, **kw):
    """Device table == host table; the structure of the wire form; with
    `exceptions`, the (kind, id) pairs that must come back as such."""
    import torch
    q = query_load(breakdown_specs=spec)
    nk = len(q.breakdowns)
    host, dev = snapshot(rows, strings, numbers, **kw)
    want = decode.decode_snapshot(
        host, [q], P.compile_plan([q], time_field="time"))[0][0]
    w = merge.encode_table(dev, q)
    blob, offs = w.strings
    for t, dtype, shape in [(w.codes, torch.int64, (len(rows), nk)),
                            (w.tagpack, torch.int64, (len(rows),)),
                            (w.vals, torch.float64, (len(rows),)),
                            (blob, torch.uint8, None),
                            (offs, torch.int64, None)]:
        assert t.is_cuda and t.dtype == dtype
        assert shape is None or tuple(t.shape) == shape
    offs_h, n_dict = offs.cpu().numpy(), offs.numel() - 1
    assert offs_h[0] == 0 and offs_h[-1] == blob.numel()
    assert (np.diff(offs_h) >= 0).all()
    kinds = merge.col_kinds(q)
    used = {int(c[j]) for c, _v in rows for j in range(nk)
            if c[j] >> 30 in (P.TAG_STR, P.TAG_SPECIAL)
            or (c[j] >> 30 == P.TAG_NUM and kinds[j] == 0)}
    assert n_dict <= len(used)
    codes_h, tags_h = w.codes.cpu().numpy(), w.tagpack.cpu().numpy()
    for j in range(nk):
        is_str = ((tags_h >> (2 * j)) & 3) == merge._EL_STR
        assert ((codes_h[is_str, j] >= 0)
                & (codes_h[is_str, j] < n_dict)).all()
    got = merge.reaggregate(q, [(w.codes, w.tagpack, w.vals)], [w.strings])
    assert typed(got.table) == typed(want.table)
    if exceptions is not None:
        out = raw_op(dev, q)
        assert list(zip(out[5].tolist(), out[6].tolist())) == exceptions


@pytest.mark.parametrize("nk", [1, 2, 8])
@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 777])
def test_shapes(n, nk):
    """Row tiles are 256: one short, exact, one over, several blocks."""
    strings = [b"s%d" % i for i in range(300)]  # two string tiles
    numbers = [float(i) for i in range(10)] + [0.5]
    pool = ([S | i for i in range(0, 300, 7)] + [N | i for i in range(11)]
            + [X | c for c in range(6)])
    rows = [([pool[(5 * i + 3 * j) % len(pool)] for j in range(nk)], i + 1)
            for i in range(n)]
    check(PLAIN[nk], rows, strings, numbers)


@pytest.mark.parametrize("pad", [0, 5])
def test_strings(pad):
    """Lengths round the 8- and 16-byte units, an offset at every residue
    mod 16 (sixteen 17-byte strings), one string beyond the LDS stage, an
    unreferenced id in between, UTF-8 as Python decides it, a backslash."""
    from dragnet_amd.ops import load_ops
    stage = load_ops(required=True).ENC_STAGE_BYTES
    good = [b"x" * k for k in (0, 1, 7, 8, 9, 15, 16, 17)]
    good += [bytes([97 + k]) * 17 for k in range(16)]
    good += ["é".encode(), "€uro".encode(), "a😀b".encode(),
             b"y" * (stage + 5), b"tail"]
    bad = [b"\xc0\x80", b"\xed\xa0\x80", b"\xf4\x90\x80\x80", b"\x80",
           b"ab\xe2\x82", b"abcdefgh\xc3", b"a\\u0041", b"q\\"]
    strings = good[:10] + [b"UNREFERENCED"] + bad + good[10:]
    skip = 10
    rows = [([S | i], i + 1) for i in range(len(strings)) if i != skip]
    exc = [(0, i) for i in range(skip + 1, skip + 1 + len(bad))]
    check("a", rows, strings, pad=pad, exceptions=exc)
    # the same strings 300 ids apart: tiles with one string each
    far = [b"-"] * (300 * len(strings))
    far[::300] = strings
    check("a", [([S | 300 * i], 2) for i in range(len(strings))
                if i != skip], far, pad=pad)


def test_numbers():
    """Plain column: digits below 2^53, everything else an exception.
    Date column: truncation.  Bucketized column: ordinals, and numbers
    as int64 or, from 2^63 up, as f64 bits."""
    plain = [0.0, -0.0, 1.0, -1.0, 999.0, 2.0**53 - 1, -(2.0**53 - 1),
             1234567890123456.0, 2.0**53, 0.5, 1e21, float("nan"),
             float("inf"), -2.5]
    ints = [1399.75, -7.9, 2.0**62, -2.0**62, 2.0**63, -2.0**63, -2.0**64]
    numbers = plain + ints
    rows = []
    for i in range(len(plain)):
        for j, x in enumerate(ints):
            o = (0, P.ORD_BIAS, 2**30 - 1)[(i + j) % 3]
            rows.append(([N | i, N | (len(plain) + j % 2), O | o], 1))
            rows.append(([N | i, S | 0, N | (len(plain) + j)], 3))
    assert merge.col_kinds(query_load(breakdown_specs=MIXED)) == [0, 1, 2]
    check(MIXED, rows, [b"2014"], numbers,
          exceptions=[(2, i) for i in range(8, len(plain))])


def test_specials_and_collisions():
    """The six constants and an array's text; null beside "null", two
    ids of one string, 5 beside "5", "a" beside its escape: each pair is
    one key, its counts summed."""
    strings = [b"null", b"dup", b"dup", b"5", b'[1,null,"x",[2]]', b"a",
               b"\\u0061", b"[1,"]
    rows = [([X | c, S | 1], 1) for c in range(6)]
    rows += [([S | 0, S | 2], 10), ([S | 3, S | 1], 20), ([N | 0, S | 2], 40),
             ([X | (P.SPECIAL_ARRJSON | 4 << 3), S | 5], 80),
             ([X | (P.SPECIAL_ARRJSON | 7 << 3), S | 6], 160),
             ([X | (P.SPECIAL_ARRJSON | 4 << 3), S | 6], 320)]
    check("a,b", rows, strings, [5.0],
          exceptions=[(0, 6), (1, 4), (1, 7)])


@pytest.mark.parametrize("spec,rows,strings,numbers,match", [
    ("a", [([S | 3], 1)], [b"x", b"y", b"z"], [], "beyond the dictionary"),
    ("a", [([N | 1], 1)], [], [1.0], "beyond the dictionary"),
    (MIXED, [([S | 0, S | 0, S | 0], 1)], [b"x"], [], "tag"),
    ("a", [([O | 5], 1)], [], [], "tag"),
    ("a", [([X | 7], 1)], [], [], "tag"),
])
def test_bad_input_raises(spec, rows, strings, numbers, match):
    q = query_load(breakdown_specs=spec)
    _host, dev = snapshot(rows, strings, numbers)
    with pytest.raises(RuntimeError, match=match):
        raw_op(dev, q)


def test_span_beyond_used_raises():
    q = query_load(breakdown_specs="a")
    _host, dev = snapshot([([S | 0], 1), ([S | 1], 1)], [b"abc", b"defg"])
    dev["used"] -= 1  # the blob tensor is longer: only `used` bounds it
    with pytest.raises(RuntimeError, match="used payload"):
        raw_op(dev, q)


@pytest.mark.parametrize("x", [float("nan"), float("-inf")])
@pytest.mark.parametrize("col", [1, 2])
def test_refusal_takes_the_host_path(x, col):
    """Where the host's int() raises, the kernels refuse."""
    q = query_load(breakdown_specs=MIXED)
    codes = [S | 0, N | 1, O | 4]
    codes[col] = N | 0
    _host, dev = snapshot([(codes, 1)], [b"s"], [x, 3.0])
    assert raw_op(dev, q)[-1] is True
    assert merge.encode_table(dev, q) is None


def test_seam_real_scan(monkeypatch):
    """One small scan: extract_wire under DRAGNET_ENCODE_GPU=1 against
    the decoded snapshot encoded on the host, both through reaggregate;
    under =0 extract_wire declines."""
    from dragnet_amd.engine.gpu import GpuEngine, _ScanContext
    recs = b"".join(
        b'{"time":"2014-05-0%dT0%d:00:00Z","m":%s,"lat":%d,"c":%s}\n'
        % (1 + i % 3, i % 7, [b'"GET"', b'"P\\u0055T"', b"null", b"17",
                              b"[1,2]", b"2.5", b'"caf\xc3\xa9"'][i % 7],
           i * 37 % 500, [b"200", b"true", b'"200"'][i % 3])
        for i in range(300))
    qs = [query_load(breakdown_specs="m,c"),
          query_load(breakdown_specs="ts[date,field=time],"
                     "lat[aggr=lquantize,step=100],m")]
    ctx = _ScanContext(GpuEngine(), P.compile_plan(qs, time_field="time"),
                       agg_slots=1 << 12, dict_slots=1 << 12,
                       dict_data_cap=1 << 20, dense=False)
    ctx.feed(recs)
    ctx.flush()
    h = ctx.extract_async(qs)
    monkeypatch.setenv("DRAGNET_ENCODE_GPU", "0")
    assert ctx.extract_wire(qs, h) is None
    aggs, _stages = ctx.decode_extracted(h, qs)
    monkeypatch.setenv("DRAGNET_ENCODE_GPU", "1")
    wires = ctx.extract_wire(qs, h)
    for q, agg, w in zip(qs, aggs, wires):
        assert len(agg.table) > 5 and w.codes.is_cuda
        assert (w.ninputs, w.ndropped_nonnumeric) == \
            (agg.ninputs, agg.ndropped_nonnumeric)
        hw = merge.encode_table(agg, q)
        want = merge.reaggregate(q, [(hw.codes, hw.tagpack, hw.vals)],
                                 [hw.strings])
        got = merge.reaggregate(q, [(w.codes, w.tagpack, w.vals)],
                                [w.strings])
        assert typed(got.table) == typed(want.table) == typed(agg.table)

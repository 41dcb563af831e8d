"""
format_numbers (ops/hip/format_numbers.h over dbl2dec.h): f64 values to
their JavaScript strings on the GPU, against the independent
Number::toString of numeric_cases.py, the host seam, and, through
merge.encode_table, the dictionary the host loop builds.  All comparisons
are exact.

All tests here require an MI355X (pytest -m gpu).
"""

import numpy as np
import pytest

from dbl2dec_corpus import corpora
from numeric_cases import js_tostring

from dragnet_amd import merge

pytestmark = pytest.mark.gpu

CORPUS = [x for _name, xs in sorted(corpora().items()) for x in xs]
LONGEST = [-1.2345678901234567e-308, -1.2345678901234567e-6]  # 24, 25 bytes


def expect(xs):
    strings = [js_tostring(x).encode() for x in xs]
    return b"".join(strings), np.cumsum([0] + [len(s) for s in strings])


def run_op(xs, variant=0):
    import torch

    from dragnet_amd.ops import load_ops
    text, offs = load_ops(required=True).format_numbers(
        torch.tensor(xs, dtype=torch.float64).cuda(), variant)
    assert text.dtype == torch.uint8 and offs.dtype == torch.int64
    return text.cpu().numpy().tobytes(), offs.cpu().numpy()


def check(xs, variant=0):
    text, offs = run_op(xs, variant)
    want_text, want_offs = expect(xs)
    assert offs.tolist() == want_offs.tolist()
    assert text == want_text


def test_corpus():
    check(CORPUS)


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 2048, 2049, 5000])
def test_tile_and_scan_edges(n):
    """Tiles are 256 numbers, scan blocks 2048."""
    step = max(len(CORPUS) // max(n, 1), 1)
    check(CORPUS[::step][:n])


@pytest.mark.parametrize("x", LONGEST + [0.0])
def test_stage_bounds(x):
    """A whole tile of the longest string (the stage's bound) or of the
    shortest (ragged 16-byte units everywhere), between mixed tiles."""
    check(CORPUS[:300] + [x] * 600 + CORPUS[300:500])


@pytest.mark.parametrize("variant", [1, 2, 3])
def test_measurement_variants(variant):
    check(CORPUS[:3000] + LONGEST * 300, variant)


@pytest.mark.parametrize("on_device", [False, True])
def test_seam_equals_host(on_device, monkeypatch):
    import torch
    xs = np.array(CORPUS[::7] + LONGEST * 200)
    monkeypatch.setenv("DRAGNET_FORMAT_GPU", "0")
    want_blob, want_offs = merge.format_numbers(xs)
    assert want_blob.tobytes() == expect(xs.tolist())[0]
    monkeypatch.setenv("DRAGNET_FORMAT_GPU", "1")
    blob, offs = merge.format_numbers(
        torch.from_numpy(xs).cuda() if on_device else xs)
    assert blob.is_cuda and offs.is_cuda
    assert blob.cpu().numpy().tobytes() == want_blob.tobytes()
    assert offs.cpu().numpy().tolist() == want_offs.tolist()


def test_encode_table_dictionary(monkeypatch):
    """A plain column of fractional and large numbers beside escaped
    strings and arrays: the wire table with the numbers formatted on the
    device is the one the host loop gives, exceptions in their order."""
    from dragnet_amd.engine import plan as P
    from dragnet_amd.engine.gpu import GpuEngine, _ScanContext
    from dragnet_amd.query import query_load
    values = [b"2.5", b"0.1", b"1234.5678", b"9007199254740992",
              b"9007199254740994", b"1e21", b"1e-7", b"123456789012345680000",
              b"-0.000001", b"17", b'"GET"', b'"P\\u0055T"', b"[1,2]",
              b'"caf\\u00e9"', b"[0.5]", b"null"]
    recs = b"".join(
        b'{"m":%s,"c":%s}\n' % (values[i % len(values)] if i % 3 else
                                b"%d.%03d" % (i, i * 7 % 1000),
                                [b"200", b"0.25", b'"2\\u0030"'][i % 3])
        for i in range(400))
    qs = [query_load(breakdown_specs="m,c")]
    ctx = _ScanContext(GpuEngine(), P.compile_plan(qs, time_field="time"),
                       agg_slots=1 << 12, dict_slots=1 << 12,
                       dict_data_cap=1 << 20, dense=False)
    ctx.feed(recs)
    ctx.flush()
    h = ctx.extract_async(qs)
    monkeypatch.setenv("DRAGNET_ENCODE_GPU", "1")
    wires = []
    for mode in "01":
        monkeypatch.setenv("DRAGNET_FORMAT_GPU", mode)
        wires.append(ctx.extract_wire(qs, h)[0])
    host, dev = wires
    assert host.codes.shape[0] > 150
    for a, b in [(host.codes, dev.codes), (host.tagpack, dev.tagpack),
                 (host.vals, dev.vals), (host.strings[0], dev.strings[0]),
                 (host.strings[1], dev.strings[1])]:
        assert a.dtype == b.dtype and a.cpu().tolist() == b.cpu().tolist()
    blob = bytes(dev.strings[0].cpu().tolist())
    for s in (b"1e+21", b"1e-7", b"9007199254740992", b"-0.000001", b"PUT",
              b"1,2", b"123456789012345680000"):
        assert s in blob

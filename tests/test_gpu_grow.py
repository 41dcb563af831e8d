"""
Growable GPU scans: input that cannot be read twice (byte source, FIFO)
— or any scan under DRAGNET_GROW=1 — grows its aggregation tables and
dictionaries in place between kernel launches (ops/hip/scan_rehash.h,
engine/capacity.py) instead of restarting.  Every comparison against
the CPU oracle is exact.

All tests here require an MI355X (pytest -m gpu).
"""

import os
import threading

import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engines():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from dragnet_amd.engine.cpu import CpuEngine
    from dragnet_amd.engine.gpu import GpuEngine
    return CpuEngine(), GpuEngine()


@pytest.fixture(scope="module")
def lines50k():
    """The input of test_gpu_engine.test_overflow_regrow."""
    from dragnet_amd.tools.mktestdata import generate_lines
    return list(generate_lines(50_000, seed=11))


@pytest.fixture
def small_tables(monkeypatch):
    """Tiny first-guess sizes and a 64-record floor: small inputs make
    populated tables grow several times."""
    monkeypatch.setenv("DRAGNET_AGG_SLOTS", "128")
    monkeypatch.setenv("DRAGNET_DICT_SLOTS", "128")
    monkeypatch.setenv("DRAGNET_DICT_DATA_MB", "1")
    monkeypatch.setenv("DRAGNET_GROW_MIN_RECORDS", "64")


def pieces(blob, size):
    """A generator over blob: it cannot be read a second time."""
    for at in range(0, len(blob), size):
        yield blob[at:at + size]


def q(spec, **kw):
    from dragnet_amd.query import query_load
    return query_load(breakdown_specs=spec, **kw)


def assert_same(cpu_res, gpu_res):
    assert len(cpu_res.aggregators) == len(gpu_res.aggregators)
    for ca, ga in zip(cpu_res.aggregators, gpu_res.aggregators):
        assert ga.points() == ca.points()
        assert ga.ninputs == ca.ninputs
        assert ga.ndropped_nonnumeric == ca.ndropped_nonnumeric
    assert dict(gpu_res.stages)["json parser"] == \
        dict(cpu_res.stages)["json parser"]


def growths(res):
    s = res.gpu_stats
    return sum(s["agg"]) + s["sdict"] + s["sdata"] + s["ndict"]


# 1
def test_generator_byte_source(engines, lines50k, small_tables):
    """A generator overflows tiny tables many times over: the scan
    neither fails nor restarts, populated tables are rehashed more than
    once, and the result is the oracle's."""
    cpu, gpu = engines
    blob = b"".join(lines50k)
    qs = [q("req.url,req.method")]
    c = cpu.scan([], qs, byte_source=pieces(blob, 1 << 20))
    g = gpu.scan([], qs, byte_source=pieces(blob, 1 << 20))
    assert_same(c, g)
    assert len(g.aggregators[0].points()) == 2000
    assert g.gpu_stats["restarts"] == 0
    assert g.gpu_stats["agg"][0] >= 2
    assert g.gpu_stats["sdict"] >= 2


# 2
@pytest.fixture(scope="module")
def kng_blob():
    recs = []
    for i in range(30_000):
        recs.append(b'{"k":"%s","n":%d,"g":%d}\n' % (
            (b"key-%06d-" % i).ljust(80, b"x"), 3 * i + 1, i % 7))
    return b"".join(recs)


@pytest.mark.parametrize("spec,must_grow,must_not", [
    ("k", ["sdict", "sdata"], ["ndict"]),
    ("n", ["ndict"], ["sdict", "sdata"]),
    ("g", [], ["agg", "sdict", "sdata", "ndict"]),
])
def test_each_structure_alone(engines, kng_blob, small_tables, spec,
                              must_grow, must_not):
    """Unique 80-byte strings (2.4 MB of payload in a 1 MB buffer),
    unique numbers, or seven groups: only what fills up grows."""
    cpu, gpu = engines
    qs = [q(spec)]
    c = cpu.scan([], qs, byte_source=pieces(kng_blob, 1 << 19))
    g = gpu.scan([], qs, byte_source=pieces(kng_blob, 1 << 19))
    assert_same(c, g)
    st = dict(g.gpu_stats)
    st["agg"] = st["agg"][0]
    assert st["restarts"] == 0
    for name in must_grow:
        assert st[name] >= 1, (name, st)
    for name in must_not:
        assert st[name] == 0, (name, st)


# 3
def test_ids_survive_growth(engines, lines50k, monkeypatch):
    """Growth moves every entry and keeps every id: the decoded
    aggregate and both dictionaries, in id order, are the same before
    and after, and the scan carries on into the grown tables."""
    import numpy as np

    cpu, gpu = engines
    from dragnet_amd.engine import plan as planmod
    from dragnet_amd.engine.gpu import _ScanContext
    monkeypatch.setenv("DRAGNET_GROW_MIN_RECORDS", "64")
    lines = lines50k[:6000]
    qs = [q("req.url,res.statusCode")]
    ctx = _ScanContext(gpu, planmod.compile_plan(qs), agg_slots=1 << 13,
                       dict_slots=1 << 13, dict_data_cap=1 << 20,
                       growable=True)
    ctx.feed(b"".join(lines[:3000]))

    def snapshot():
        h = ctx.extract_async(qs)
        aggs, _stages = ctx.decode_extracted(h, qs)
        strings, numbers = ctx._decode_dicts(h)
        return dict(aggs[0].table), strings, numbers

    table0, strings0, numbers0 = snapshot()
    # (the string list may name a string twice: two lanes interning it
    # at the same moment can both insert it; decode merges such groups)
    assert len(table0) > 1000 and len(set(strings0)) > 400
    assert len(set(numbers0.tolist())) == 7
    sizes0 = dict(ctx.planner.size)
    for name in ctx.planner.names:
        ctx.grow(name, 4 * sizes0[name])
    assert ctx.agg_slots == 4 << 13 and ctx.dict_slots == 4 << 13
    table1, strings1, numbers1 = snapshot()
    assert table1 == table0
    assert strings1 == strings0
    assert np.array_equal(numbers1, numbers0)

    ctx.feed(b"".join(lines[3000:]))
    ctx.flush()
    aggs, stages = ctx.finalize(qs)
    assert not ctx.overflowed()
    c = cpu.scan([], qs, byte_source=[b"".join(lines)])
    assert aggs[0].points() == c.aggregators[0].points()
    assert aggs[0].ninputs == c.aggregators[0].ninputs
    assert dict(stages)["json parser"] == dict(c.stages)["json parser"]

    # reset() works on the grown state: a fresh scan of the whole input
    ctx.reset()
    ctx.feed(b"".join(lines))
    ctx.flush()
    aggs, _stages = ctx.finalize(qs)
    assert aggs[0].points() == c.aggregators[0].points()


# 4
def test_several_metrics(engines, lines50k, small_tables):
    """Each metric's table grows on its own."""
    cpu, gpu = engines
    blob = b"".join(lines50k[:20_000])
    qs = [q("req.url"), q("host")]
    c = cpu.scan([], qs, byte_source=pieces(blob, 1 << 20))
    g = gpu.scan([], qs, byte_source=pieces(blob, 1 << 20))
    assert_same(c, g)
    assert g.gpu_stats["restarts"] == 0
    assert g.gpu_stats["agg"][0] >= 1
    assert g.gpu_stats["agg"][1] == 0


# 5
def test_buckets_dates_and_drops(engines, fixture_tree, small_tables):
    """Bucketized columns, a date breakdown and a time filter over the
    fixture tree (invalid JSON, a bad date, a missing time field): every
    drop is counted once, whatever sub-range it falls into."""
    cpu, gpu = engines
    files = []
    for root, _dirs, names in os.walk(fixture_tree):
        for n in sorted(names):
            files.append(os.path.join(root, n))
    files.sort()
    blob = b"".join(open(p, "rb").read() for p in files)
    from dragnet_amd.query import query_load
    qs = [query_load(
        breakdown_specs="ts[date,field=time,aggr=lquantize,step=3600],"
                        "latency[aggr=quantize]",
        time_after="2014-05-02T06:00:00", time_before="2014-05-04")]
    c = cpu.scan([], qs, time_field="time",
                 byte_source=pieces(blob, 4096))
    g = gpu.scan([], qs, time_field="time",
                 byte_source=pieces(blob, 4096))
    assert_same(c, g)
    assert [s for s in g.stages if s[0] != "Aggregator"] == \
        [s for s in c.stages if s[0] != "Aggregator"]
    names = [s[0] for s in g.stages]
    assert "Datetime parser" in names and "Time filter" in names
    assert dict(g.stages)["json parser"]["invalid json"] == 2
    assert g.gpu_stats["restarts"] == 0
    assert g.gpu_stats["agg"][0] >= 1


# 6
def test_sub_range_edges(engines, lines50k, small_tables):
    """Record counts that are no multiple of the block or the floor,
    empty lines, a chunk that ends in a one-record sub-range, and
    partial lines carried from chunk to chunk."""
    cpu, gpu = engines
    lines = list(lines50k[:1357])
    for at in (0, 63, 64, 65, 700, 1300):
        lines.insert(at, b"\n")
    n = len(lines)
    assert n % 64 and n % 256
    blob = b"".join(lines)
    qs = [q("req.method,res.statusCode")]
    c = cpu.scan([], qs, byte_source=[blob])
    assert dict(c.stages)["json parser"]["invalid json"] == 6

    # tiny chunks: every cut falls inside a record
    g = gpu.scan([], qs, byte_source=pieces(blob, 997))
    assert_same(c, g)
    # two chunks, cut inside a record so that the second holds 5 * 64 + 1
    # lines: with 28 groups in a 128-slot table a sub-range is one floor
    # of 64 records, so the chunk ends in a sub-range of one
    cut = len(b"".join(lines[:n - 321])) + 5
    g = gpu.scan([], qs, byte_source=iter([blob[:cut], blob[cut:]]))
    assert_same(c, g)
    assert g.gpu_stats["restarts"] == 0


# 7
def test_skinner_integer_weights(engines, lines50k, small_tables):
    """json-skinner points carry integer weights: the weighted sums are
    exact after the tables holding them were rehashed."""
    cpu, gpu = engines
    from dragnet_amd.output import point_json
    base = cpu.scan([], [q("req.url,res.statusCode")],
                    byte_source=[b"".join(lines50k[:20_000])]
                    ).aggregators[0].points()
    blob = b"".join((point_json(p) + "\n").encode()
                    for _ in range(3) for p in base)
    qs = [q("req.url")]
    c = cpu.scan([], qs, data_format="json-skinner",
                 byte_source=pieces(blob, 1 << 18))
    g = gpu.scan([], qs, data_format="json-skinner",
                 byte_source=pieces(blob, 1 << 18))
    assert_same(c, g)
    pts = g.aggregators[0].points()
    assert len(pts) == 500
    assert all(isinstance(p["value"], int) for p in pts)
    assert sum(p["value"] for p in pts) == 3 * 20_000
    assert g.gpu_stats["restarts"] == 0
    assert g.gpu_stats["agg"][0] >= 1 and g.gpu_stats["sdict"] >= 1


# 8
def test_fifo_in_file_list(engines, lines50k, small_tables, tmp_path,
                           monkeypatch):
    """A FIFO among the files cannot be reopened: the scan is growable
    and runs once."""
    cpu, _gpu = engines
    from dragnet_amd.engine.gpu import GpuEngine
    # several chunks through the ping-pong route
    monkeypatch.setenv("DRAGNET_CHUNK_MB", "1")
    blob = b"".join(lines50k[:20_000])
    fifo = str(tmp_path / "pipe.ndjson")
    os.mkfifo(fifo)

    def writer():
        with open(fifo, "wb") as f:
            f.write(blob)

    t = threading.Thread(target=writer, daemon=True)
    t.start()
    qs = [q("req.url")]
    g = GpuEngine().scan([fifo], qs)
    t.join(timeout=10)
    assert not t.is_alive()
    c = cpu.scan([], qs, byte_source=[blob])
    assert_same(c, g)
    assert g.gpu_stats["restarts"] == 0
    assert g.gpu_stats["agg"][0] >= 1


# 9
def test_grow_knob_on_regular_file(engines, lines50k, tmp_path,
                                   monkeypatch):
    """DRAGNET_GROW=1 opts a regular-file scan in (the input and sizes
    of test_overflow_regrow); without it the scan restarts as before."""
    cpu, gpu = engines
    path = tmp_path / "many.ndjson"
    path.write_bytes(b"".join(lines50k))
    monkeypatch.setenv("DRAGNET_AGG_SLOTS", "128")
    monkeypatch.setenv("DRAGNET_DICT_SLOTS", "128")
    monkeypatch.setenv("DRAGNET_DICT_DATA_MB", "1")
    qs = [q("req.url")]
    c = cpu.scan([str(path)], qs)

    monkeypatch.setenv("DRAGNET_GROW", "1")
    g = gpu.scan([str(path)], qs)
    assert_same(c, g)
    assert g.gpu_stats["restarts"] == 0
    assert growths(g) >= 1

    monkeypatch.delenv("DRAGNET_GROW")
    g = gpu.scan([str(path)], qs)
    assert_same(c, g)
    assert g.gpu_stats["restarts"] >= 1
    assert growths(g) == 0


# 10
def test_low_cardinality_plans_no_growth(engines, lines50k, monkeypatch):
    """Default sizes, four groups: nothing grows."""
    cpu, gpu = engines
    for name in ("DRAGNET_AGG_SLOTS", "DRAGNET_DICT_SLOTS",
                 "DRAGNET_DICT_DATA_MB", "DRAGNET_GROW_MIN_RECORDS",
                 "DRAGNET_GROW"):
        monkeypatch.delenv(name, raising=False)
    blob = b"".join(lines50k[:20_000])
    qs = [q("req.method")]
    c = cpu.scan([], qs, byte_source=pieces(blob, 1 << 20))
    g = gpu.scan([], qs, byte_source=pieces(blob, 1 << 20))
    assert_same(c, g)
    assert g.gpu_stats == {"restarts": 0, "agg": [0], "sdict": 0,
                           "sdata": 0, "ndict": 0}


def _small_context(gpu, qs, **kw):
    from dragnet_amd.engine import plan as planmod
    from dragnet_amd.engine.gpu import _ScanContext
    return _ScanContext(gpu, planmod.compile_plan(qs), agg_slots=128,
                        dict_slots=128, dict_data_cap=4096, **kw)


def _values(aggs):
    return [{tuple(sorted(p["fields"].items())): p["value"]
             for p in a.points()} for a in aggs]


# 11
def test_state_sizes_and_rejected_growth(engines, monkeypatch):
    """The state reports its sizes under the planner's names; a growth
    it rejects (a host-side argument check) changes nothing, and the
    context scans and grows as if it had not been asked."""
    from dragnet_amd.tools.mktestdata import generate_lines
    cpu, gpu = engines
    monkeypatch.setenv("DRAGNET_GROW_MIN_RECORDS", "64")
    qs = [q("req.method,res.statusCode"), q("host")]
    ctx = _small_context(gpu, qs, growable=True)
    st = ctx.state
    sizes0 = {"agg0": 128, "agg1": 128, "sdict": 128, "sdata": 4096,
              "ndict": 128}
    assert st.sizes() == sizes0
    assert list(st.sizes()) == ctx.planner.names
    assert st.sizes() == ctx.planner.size

    for call, text in (
            (lambda: st.grow_agg(0, 128), "a table may only grow"),
            (lambda: st.grow_agg(0, 64), "a table may only grow"),
            (lambda: st.grow_sdict(192), "must be a power of two"),
            (lambda: st.grow_sdata(4096), "buffer may only grow"),
            (lambda: st.grow_agg(2, 256), "no such metric")):
        with pytest.raises(RuntimeError, match=text):
            call()
    assert st.sizes() == sizes0

    blob = b"".join(generate_lines(200, seed=11))
    want = cpu.scan([], qs, byte_source=[blob])
    ctx.feed(blob)
    aggs, _stages = ctx.finalize(qs)
    assert not ctx.overflowed()
    assert [a.points() for a in aggs] == \
        [a.points() for a in want.aggregators]
    once = _values(aggs)
    sizes1 = st.sizes()

    ctx.grow("agg1", 512)
    assert st.sizes() == dict(sizes1, agg1=512) == ctx.planner.size
    ctx.feed(blob)
    aggs, _stages = ctx.finalize(qs)
    assert not ctx.overflowed()
    assert _values(aggs) == [{k: 2 * v for k, v in m.items()}
                             for m in once]


# 12
def test_dense_state_does_not_grow(engines):
    from dragnet_amd.tools.mktestdata import generate_lines
    cpu, gpu = engines
    qs = [q("req.method,res.statusCode")]
    ctx = _small_context(gpu, qs, dense=True)
    assert ctx.dense
    with pytest.raises(RuntimeError, match="dense tables do not grow"):
        ctx.state.grow_agg(0, 256)
    blob = b"".join(generate_lines(200, seed=11))
    ctx.feed(blob)
    aggs, _stages = ctx.finalize(qs)
    assert not ctx.overflowed()
    assert aggs[0].points() == \
        cpu.scan([], qs, byte_source=[blob]).aggregators[0].points()

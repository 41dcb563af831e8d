"""
Index queries answered from columnar sidecars on the GPU (pytest -m
gpu): dict_intern_kernel + coded_query_kernel over the merged sidecars
of a tree must give exactly what the per-file SQLite path gives — the
same points, the same `Index List` / `Index Result Aggregator` counters.
Row weights are integer counts, so sums are exact and outputs are
compared byte for byte.
"""

import os

import pytest

from dragnet_amd.index import IndexSink
from dragnet_amd.index import columnar as C

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def require_gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def sidecar_delta(fn):
    """(result of fn(), how many files / launches took the sidecar
    path meanwhile, how many files went the other way)."""
    before = dict(C.STATS)
    rv = fn()
    return rv, {k: C.STATS[k] - before[k] for k in before}


def tree_files(idx, suffix):
    out = []
    for d, _dirs, names in os.walk(idx):
        out += [os.path.join(d, n) for n in names if n.endswith(suffix)]
    return sorted(out)


# ---- CLI parity: the trees and query cases of test_gpu_cli's
# test_cli_query_index_gpu_path and ..._gpu_columnar_bounds ----

def tree_one(dn, fixture_tree, idx):
    one = os.path.join(fixture_tree, "2014", "05-01", "one.log")
    assert dn("datasource-add", "input", "--path=" + one,
              "--index-path=" + idx, "--time-field=time").code == 0
    assert dn("metric-add", "input", "m", "-b",
              "host,operation,req.method,latency[aggr=quantize]").code == 0
    return [(), ("-b", "operation"),
            ("-f", '{ "eq": [ "req.method", "GET" ] }',
             "-b", "host,operation"),
            ("-b", "host,latency[aggr=quantize]")]


def tree_bounds(dn, fixture_tree, idx):
    assert dn("datasource-add", "input", "--path=" + fixture_tree,
              "--index-path=" + idx, "--time-field=time",
              "--time-format=%Y/%m-%d").code == 0
    assert dn("metric-add", "input", "m", "-b",
              "ts[date,field=time,aggr=lquantize,step=3600],"
              "host,req.method,latency[aggr=quantize]").code == 0
    return [("-b", "host", "--after", "2014-05-01",
             "--before", "2014-05-03"),
            ("-b", "req.method,latency[aggr=quantize]",
             "--after", "2014-05-02", "--before", "2014-05-05"),
            ("-b", "ts[date,field=time,aggr=lquantize,step=3600],host",
             "--after", "2014-05-02", "--before", "2014-05-03"),
            ("-b", "host,req.method")]


@pytest.mark.parametrize("interval", ["day", "hour"])
@pytest.mark.parametrize("tree", [tree_one, tree_bounds])
def test_cli_query_sidecars_equal_sqlite(dn, fixture_tree, tmp_path,
                                         monkeypatch, tree, interval):
    idx = str(tmp_path / "idx")
    monkeypatch.setenv("DRAGNET_ENGINE", "gpu")
    monkeypatch.setenv("DRAGNET_INDEX_COLUMNAR", "1")
    cases = tree(dn, fixture_tree, idx)
    r = dn("build", "--interval=" + interval, "input")
    assert r.code == 0, r.err
    nfiles = len(tree_files(idx, ".sqlite"))
    assert len(tree_files(idx, ".dncol")) == nfiles > 0
    for case in cases:
        argv = ["query", "--counters", "--interval=" + interval, *case,
                "input"]
        monkeypatch.setenv("DRAGNET_INDEX_GPU", "0")
        sql, d0 = sidecar_delta(lambda: dn(*argv))
        monkeypatch.setenv("DRAGNET_INDEX_GPU", "1")
        gpu, d1 = sidecar_delta(lambda: dn(*argv))
        assert sql.code == 0 and gpu.code == 0, (case, gpu.err)
        assert gpu.out == sql.out, case
        assert gpu.err == sql.err, case
        # the sidecar path served every file the query found, in one
        # launch; SQLite served them all before
        assert d0["sidecar_files"] == 0 and d0["other_files"] > 0
        assert d1["sidecar_files"] == d0["other_files"], case
        assert d1["other_files"] == 0 and d1["sidecar_launches"] == 1


# ---- a synthetic tree, straight through IndexSink and the writer ----

SEG_ROWS = [0, 1, 63, 64, 65, 257]
METHODS = ["GET", "PUT", "DEL"]
LATS = [0, 1, 2, 4, 64, 1024]
METRIC = {"name": "m", "filter": None, "breakdowns": [
    {"name": "host", "field": "host"},
    {"name": "method", "field": "method"},
    {"name": "lat", "field": "lat", "aggr": "quantize"}]}


def hosts_of(k):
    """File k's hosts: "m" is in every file, behind k others that sort
    before it, so its local dictionary code is k (0 in the 1-row file,
    which holds nothing else)."""
    return ["m"] + ["a%d" % j for j in range(k)] + ["z%d" % k]


def write_file(path, k, nrows, host_of=None, sidecar=True):
    sink = IndexSink(path, [METRIC])
    hosts = hosts_of(k)
    for i in range(nrows):
        host = hosts[i % len(hosts)]
        sink.write_point({"fields": {
            "__dn_metric": 0,
            "host": host_of(i) if host_of else host,
            "method": METHODS[(i + k) % 3],
            "lat": LATS[(i // 3 + k) % len(LATS)]}, "value": 1 + i % 4})
    sink.flush()
    if sidecar:
        C.write_sidecar(path)


@pytest.fixture(scope="module")
def gpu_engine():
    import torch
    if not torch.cuda.is_available():  # module scope: set up before
        pytest.skip("no GPU")          # require_gpu gets to skip
    from dragnet_amd.engine.gpu import GpuEngine
    return GpuEngine()


def datasource(idx, engine):
    from dragnet_amd.config import Datasource
    from dragnet_amd.datasource.file import FileDatasource
    ds = Datasource(name="t", backend="file", path="/dev/null",
                    index_path=idx, time_field="time")
    return FileDatasource(ds, engine=engine)


@pytest.fixture(scope="module")
def seg_tree(tmp_path_factory):
    idx = str(tmp_path_factory.mktemp("segidx"))
    for k, nrows in enumerate(SEG_ROWS):
        write_file(os.path.join(idx, "by_day", "2014-05-%02d.sqlite"
                                % (k + 1)), k, nrows)
    return idx


@pytest.fixture(scope="module")
def k7_tree(tmp_path_factory):
    """seg_tree's files without their sidecars: every file goes through
    the per-file K7 query."""
    idx = str(tmp_path_factory.mktemp("k7idx"))
    for k, nrows in enumerate(SEG_ROWS):
        write_file(os.path.join(idx, "by_day", "2014-05-%02d.sqlite"
                                % (k + 1)), k, nrows, sidecar=False)
    return idx


def ask(fd, monkeypatch, mode, **kw):
    """(points, stages, sidecar tally) of one query under a policy."""
    from dragnet_amd.query import query_load
    monkeypatch.setenv("DRAGNET_INDEX_GPU", mode)
    res, delta = sidecar_delta(
        lambda: fd.query(query_load(**kw), interval="day"))
    assert not res.errors
    return res.aggregators[0].points(), dict(res.stages), delta


SEG_QUERIES = {
    "none": dict(),
    "one_string": dict(breakdown_specs="host"),
    "strings_and_bucket": dict(
        breakdown_specs="host,method,lat[aggr=quantize]"),
    "eq": dict(filter={"eq": ["method", "GET"]}, breakdown_specs="host"),
    "lt": dict(filter={"lt": ["lat", 64]}, breakdown_specs="method"),
}


def check_segment_edges(fd, monkeypatch, name, served):
    """Mode 1 against mode 0 for one SEG_QUERIES entry; `served` is the
    tally that mode 1 must leave."""
    kw = SEG_QUERIES[name]
    want, wstages, d0 = ask(fd, monkeypatch, "0", **kw)
    got, gstages, d1 = ask(fd, monkeypatch, "1", **kw)
    assert d0["sidecar_files"] == 0
    assert d1 == served
    assert got == want
    assert sum(p["value"] for p in got) > 0
    assert gstages["Index List"] == wstages["Index List"]
    assert gstages["Index Result Aggregator"] == \
        wstages["Index Result Aggregator"]
    if name == "none":
        # one partial row per file, the empty file's included
        assert gstages["Index List"]["ninputs"] == len(SEG_ROWS)
    if name == "one_string":
        assert any(p["fields"]["host"] == "m" for p in got)
        assert gstages["Index List"]["ninputs"] > len(got)


@pytest.mark.parametrize("name", sorted(SEG_QUERIES))
def test_segment_edges(seg_tree, gpu_engine, monkeypatch, name):
    """Files of 0, 1, 63, 64, 65 and 257 rows: segments that end inside,
    at and just past a wave; the same group key in several files; one
    string at a different local code in every file."""
    check_segment_edges(
        datasource(seg_tree, gpu_engine), monkeypatch, name,
        {"sidecar_files": len(SEG_ROWS), "sidecar_launches": 1,
         "other_files": 0})


@pytest.mark.parametrize("name", sorted(SEG_QUERIES))
def test_segment_edges_k7(k7_tree, gpu_engine, monkeypatch, name):
    """The same files through the per-file K7 query: no rows (no
    launch), one row, and rows that end inside a wave."""
    check_segment_edges(
        datasource(k7_tree, gpu_engine), monkeypatch, name,
        {"sidecar_files": 0, "sidecar_launches": 0,
         "other_files": len(SEG_ROWS)})


def test_auto_mode_counts_rows_from_headers(seg_tree, gpu_engine,
                                            monkeypatch):
    fd = datasource(seg_tree, gpu_engine)
    kw = SEG_QUERIES["one_string"]
    want, _s, _d = ask(fd, monkeypatch, "0", **kw)
    monkeypatch.delenv("DRAGNET_INDEX_COLUMNAR_ROWS", raising=False)
    total = sum(SEG_ROWS)
    for rows, taken in ((None, False), (total + 1, False), (total, True)):
        if rows is not None:
            monkeypatch.setenv("DRAGNET_INDEX_COLUMNAR_ROWS", str(rows))
        got, _s, d = ask(fd, monkeypatch, "auto", **kw)
        assert got == want
        assert d["sidecar_files"] == (len(SEG_ROWS) if taken else 0)


# ---- fallbacks ----

@pytest.fixture(scope="module")
def backslash_tree(tmp_path_factory):
    idx = str(tmp_path_factory.mktemp("bsidx"))
    for k in range(3):
        write_file(
            os.path.join(idx, "by_day", "2014-05-%02d.sqlite" % (k + 1)),
            k, 20,
            host_of=(lambda i: "c:\\dir%d" % (i % 3)) if k == 1 else None)
    return idx


def test_backslash_in_needed_column_goes_to_sqlite(backslash_tree,
                                                   gpu_engine, monkeypatch):
    fd = datasource(backslash_tree, gpu_engine)
    want, _s, _d = ask(fd, monkeypatch, "0", breakdown_specs="host")
    got, _s, d = ask(fd, monkeypatch, "1", breakdown_specs="host")
    assert got == want
    assert d["sidecar_files"] == 0 and d["other_files"] == 3
    assert any("\\" in p["fields"]["host"] for p in got)


def test_backslash_in_other_column_keeps_sidecar_path(backslash_tree,
                                                      gpu_engine,
                                                      monkeypatch):
    fd = datasource(backslash_tree, gpu_engine)
    kw = dict(breakdown_specs="method,lat[aggr=quantize]")
    want, _s, _d = ask(fd, monkeypatch, "0", **kw)
    got, _s, d = ask(fd, monkeypatch, "1", **kw)
    assert got == want
    assert d["sidecar_files"] == 3 and d["other_files"] == 0


def test_stale_sidecar_file_goes_to_sqlite(tmp_path, gpu_engine,
                                           monkeypatch):
    idx = str(tmp_path / "idx")
    files = [os.path.join(idx, "by_day", "2014-05-%02d.sqlite" % (k + 1))
             for k in range(3)]
    for k, f in enumerate(files):
        write_file(f, k, 30)
    st = os.stat(files[1])
    os.utime(files[1], ns=(st.st_atime_ns, st.st_mtime_ns + 10 ** 9))
    fd = datasource(idx, gpu_engine)
    kw = dict(breakdown_specs="host,method")
    want, wst, _d = ask(fd, monkeypatch, "0", **kw)
    got, gst, d = ask(fd, monkeypatch, "1", **kw)
    assert got == want
    assert gst["Index List"] == wst["Index List"]
    assert d == {"sidecar_files": 2, "sidecar_launches": 1,
                 "other_files": 1}


def test_max_key_breakdowns_served_without_sidecars(tmp_path, gpu_engine,
                                                    monkeypatch):
    from dragnet_amd.engine.plan import MAX_KEY
    names = ["c%d" % i for i in range(MAX_KEY)]
    metric = {"name": "m", "filter": None, "breakdowns": [
        {"name": n, "field": n} for n in names]}
    idx = str(tmp_path / "idx")
    for k in range(2):
        f = os.path.join(idx, "by_day", "2014-05-%02d.sqlite" % (k + 1))
        sink = IndexSink(f, [metric])
        for i in range(10):
            fields = {n: "v%d" % ((i + j + k) % 3)
                      for j, n in enumerate(names)}
            sink.write_point({"fields": dict(fields, __dn_metric=0),
                              "value": i + 1})
        sink.flush()
        C.write_sidecar(f)
    fd = datasource(idx, gpu_engine)
    full = dict(breakdown_specs=",".join(names))
    want, _s, _d = ask(fd, monkeypatch, "0", **full)
    got, _s, d = ask(fd, monkeypatch, "1", **full)
    assert got == want
    assert d["sidecar_files"] == 0 and d["other_files"] == 2
    # one breakdown fewer leaves room for the file column
    less = dict(breakdown_specs=",".join(names[:-1]))
    want, _s, _d = ask(fd, monkeypatch, "0", **less)
    got, _s, d = ask(fd, monkeypatch, "1", **less)
    assert got == want
    assert d["sidecar_files"] == 2


# ---- overflow retry ----

def test_overflow_retries_with_larger_tables(seg_tree, gpu_engine,
                                             monkeypatch):
    """One aggregation slot — the fewest the state accepts — and far
    more groups: the query retries with 8x tables until they fit."""
    fd = datasource(seg_tree, gpu_engine)
    kw = SEG_QUERIES["strings_and_bucket"]
    want, _s, _d = ask(fd, monkeypatch, "0", **kw)
    assert len(want) > 8
    monkeypatch.setenv("DRAGNET_AGG_SLOTS", "1")
    before = dict(gpu_engine.coded_stats)
    got, _s, d = ask(fd, monkeypatch, "1", **kw)
    assert got == want
    assert d["sidecar_files"] == len(SEG_ROWS)
    assert gpu_engine.coded_stats["retries"] - before["retries"] >= 2
    assert gpu_engine.coded_stats["launches"] - before["launches"] == 1


def test_k7_overflow_retries_once(k7_tree, gpu_engine, monkeypatch):
    """Two aggregation slots and three groups in every file of 63 rows
    and more: those files overflow, and their one retry, at 16 slots,
    holds them."""
    from dragnet_amd.engine import colquery
    fd = datasource(k7_tree, gpu_engine)
    kw = dict(breakdown_specs="method")
    want, _s, _d = ask(fd, monkeypatch, "0", **kw)
    assert len(want) == len(METHODS) == 3
    slots = []

    class Counting(colquery._ScanContext):
        def __init__(self, eng, cplan, agg_slots, *rest, **kwargs):
            slots.append(agg_slots)
            super().__init__(eng, cplan, agg_slots, *rest, **kwargs)

    monkeypatch.setattr(colquery, "_ScanContext", Counting)
    monkeypatch.setenv("DRAGNET_AGG_SLOTS", "2")
    got, _s, d = ask(fd, monkeypatch, "1", **kw)
    assert got == want
    assert d["sidecar_files"] == 0 and d["other_files"] == len(SEG_ROWS)
    # a first attempt per file; a second for the four with three groups
    assert sorted(slots) == [2] * len(SEG_ROWS) + [16] * 4


# ---- malformed calls are rejected before any launch ----

def test_columnar_query_rejects_malformed_input(gpu_engine):
    import torch
    from dragnet_amd.engine import colquery
    from dragnet_amd.query import query_load
    dev = gpu_engine.device
    cplan = colquery.column_plan(query_load(breakdown_specs="host"), None)
    nf = len(cplan.field_sigs)
    state = colquery._ScanContext(gpu_engine, cplan, 16, 16, 8 << 20,
                                  dense=False).state
    none = [torch.empty(0)] * nf
    descs = gpu_engine.ops.col_descs_host([0] * nf, none, none, none).to(dev)
    blob = torch.zeros(16, dtype=torch.uint8, device=dev)
    values = torch.ones(4, dtype=torch.float64, device=dev)
    short = torch.zeros(3, dtype=torch.float64, device=dev)
    with pytest.raises(RuntimeError, match="column shorter than nrows"):
        state.columnar_query(descs, blob, values, 4, [short])
    with pytest.raises(RuntimeError, match="col_descs does not match"):
        state.columnar_query(descs[:-8], blob, values, 4, [])
    torch.cuda.synchronize(dev)
    assert int(state.counters.sum().item()) == 0  # no row was counted

"""
Columnar index sidecars on the host (dragnet_amd/index/columnar.py):
the format's round trip, the reader's validation, the tree merge, the
opt-in switches and the tool.  No GPU: the CPU engine never reads a
sidecar, so with one present `dn query` must not change at all.
"""

import json
import os
import struct

import numpy as np
import pytest

from dragnet_amd.index import IndexSink
from dragnet_amd.index import columnar as C
from dragnet_amd.query import QueryConfig

STRINGS = ["", "héllo 世界", "back\\slash", "plain", "plain"]
INTS = [-5, 2 ** 31 + 7, 3, -(2 ** 33), 2 ** 40]

METRICS = [
    {"name": "total", "filter": None, "breakdowns": []},
    {"name": "strs", "filter": None, "breakdowns": [
        {"name": "host", "field": "host"},
        {"name": "req.method", "field": "req.method"}]},
    {"name": "nums", "filter": None, "breakdowns": [
        {"name": "lat", "field": "lat", "aggr": "lquantize", "step": 1},
        {"name": "host", "field": "host"}]},
]


def make_index(path, nrows, shift=0):
    """An index file straight through IndexSink: nrows rows per metric.
    Only `host` ever holds a backslash."""
    sink = IndexSink(str(path), METRICS)
    for i in range(nrows):
        j = i + shift
        sink.write_point({"fields": {"__dn_metric": 0}, "value": i + 1})
        sink.write_point({"fields": {
            "__dn_metric": 1, "host": STRINGS[j % len(STRINGS)],
            "req.method": ["GET", "PUT", "GET"][j % 3]}, "value": i + 2})
        sink.write_point({"fields": {
            "__dn_metric": 2, "lat": INTS[j % len(INTS)],
            "host": "h%d" % (j % 7)}, "value": 3})
    sink.flush()
    return str(path)


def assert_same_table(got, want):
    kinds, cols, vals = got
    kinds2, cols2, vals2 = want
    assert kinds == kinds2
    assert vals.dtype == np.float64 and np.array_equal(vals, vals2)
    for k, a, b in zip(kinds, cols, cols2):
        if k == "n":
            assert np.array_equal(a, b)
        else:
            assert a[0] == b[0]
            assert np.array_equal(a[1], b[1])
            assert np.array_equal(a[2], b[2])


# ---- round trip ----

@pytest.mark.parametrize("native", [True, False])
@pytest.mark.parametrize("nrows", [0, 1, 65])
def test_round_trip_equals_read_columns(tmp_path, nrows, native):
    """Sidecar -> decode through the dictionary == _csink.read_columns
    on the same file, whichever extractor fed the writer."""
    from dragnet_amd.index import _csink  # noqa: F401  (the reference)
    f = make_index(tmp_path / "x.sqlite", nrows)
    side = C.write_sidecar(f, native=native)
    assert side == f + ".dncol"
    assert not [n for n in os.listdir(str(tmp_path)) if ".dncol." in n]
    sc = C.open_sidecar(f, full=True)
    assert sc is not None
    assert [m["id"] for m in sc.metrics] == [0, 1, 2]
    assert sc.config["version"] == "2.0.0"
    for ent in sc.metrics:
        assert ent["nrows"] == nrows
        assert ent["label"] == METRICS[ent["id"]]["name"]
        assert ent["params"] == METRICS[ent["id"]]["breakdowns"]
        assert_same_table(sc.table(ent["id"]),
                          C.read_table(f, ent, native=True))
    if nrows == 65:
        # negative and > 2^31 integers survive as exact doubles
        lat = sc.column(2, "lat")
        assert set(lat.tolist()) == set(float(v) for v in INTS)
        codes, values = sc.column(1, "host")
        assert sorted(values) == sorted(
            set(s.encode("utf-8") for s in STRINGS))
        assert len(codes) == 65


def test_has_backslash_only_where_there_is_one(tmp_path):
    f = make_index(tmp_path / "x.sqlite", 65)
    C.write_sidecar(f)
    sc = C.open_sidecar(f)
    assert sc.column_info(1, "host")["has_backslash"] is True
    assert sc.column_info(1, "req.method")["has_backslash"] is False
    assert sc.column_info(2, "host")["has_backslash"] is False


def test_writers_agree_byte_for_byte(tmp_path):
    """The writer does not depend on which extractor fed it."""
    f = make_index(tmp_path / "x.sqlite", 65)
    a = open(C.write_sidecar(f, native=True), "rb").read()
    b = open(C.write_sidecar(f, native=False), "rb").read()
    assert a == b


# ---- validation ----

def split_sidecar(path):
    data = open(path, "rb").read()
    version, hlen = struct.unpack("<II", data[8:16])
    header = json.loads(data[16:16 + hlen].decode("utf-8"))
    base = (16 + hlen + 63) & ~63
    return data, header, base


def rewrite_header(path, mutate):
    data, header, base = split_sidecar(path)
    mutate(header)
    raw = json.dumps(header, separators=(",", ":")).encode("utf-8")
    out = C.MAGIC + struct.pack("<II", C.VERSION, len(raw)) + raw
    out += b"\0" * (((len(out) + 63) & ~63) - len(out))
    open(path, "wb").write(out + data[base:])


def poke_u32(path, section, index, value):
    data, _header, base = split_sidecar(path)
    at = base + section[0] + 4 * index
    open(path, "wb").write(
        data[:at] + struct.pack("<I", value) + data[at + 4:])


def strs_column(header, name="host"):
    """The first metric's column of that name."""
    for m in header["metrics"]:
        names = [p["name"] for p in json.loads(m["params"])]
        if name in names:
            return m["columns"][names.index(name)]
    raise KeyError(name)


def damage_truncated(side, index):
    data = open(side, "rb").read()
    open(side, "wb").write(data[:len(data) - 70])


def damage_truncated_header(side, index):
    open(side, "wb").write(open(side, "rb").read()[:11])


def damage_magic(side, index):
    data = open(side, "rb").read()
    open(side, "wb").write(b"X" + data[1:])


def damage_version(side, index):
    data = open(side, "rb").read()
    open(side, "wb").write(
        data[:8] + struct.pack("<I", C.VERSION + 1) + data[12:])


def damage_offset_past_eof(side, index):
    size = os.path.getsize(side)

    def mutate(h):
        strs_column(h)["codes"][0] = size
    rewrite_header(side, mutate)


def damage_code_equals_ndict(side, index):
    _d, header, _b = split_sidecar(side)
    col = strs_column(header)
    poke_u32(side, col["codes"], 0, col["ndict"])


def damage_dict_span(side, index):
    _d, header, _b = split_sidecar(side)
    col = strs_column(header)
    poke_u32(side, col["len"], col["ndict"] - 1, 1 << 20)


def damage_sqlite_mtime(side, index):
    st = os.stat(index)
    os.utime(index, ns=(st.st_atime_ns, st.st_mtime_ns + 1000000000))


def damage_sqlite_size(side, index):
    # as if the index file had been a byte shorter when stamped
    def mutate(h):
        h["sqlite_size"] -= 1
    rewrite_header(side, mutate)


DAMAGES = [damage_truncated, damage_truncated_header, damage_magic,
           damage_version, damage_offset_past_eof,
           damage_code_equals_ndict, damage_dict_span,
           damage_sqlite_mtime, damage_sqlite_size]


@pytest.mark.parametrize("damage", DAMAGES,
                         ids=[d.__name__[7:] for d in DAMAGES])
def test_damaged_sidecar_is_unusable_not_an_error(tmp_path, damage):
    f = make_index(tmp_path / "x.sqlite", 65)
    side = C.write_sidecar(f)
    assert C.open_sidecar(f, full=True) is not None
    damage(side, f)
    assert C.open_sidecar(f, full=True) is None
    # what a query does: open by the header, check columns as they load
    sc = C.open_sidecar(f)
    if sc is not None:
        q = QueryConfig(breakdowns=[{"name": "host"},
                                    {"name": "req.method"}])
        groups, errors = C.group_sidecars([sc], q)
        assert not errors
        launches, rejected = C.merge_group(
            groups[0][1], C.needed_columns(q, groups[0][0]))
        assert launches == [] and rejected == [sc]


CLI_QUERIES = [(), ("-b", "host"),
               ("-f", '{ "eq": [ "req.method", "GET" ] }',
                "-b", "host,operation"),
               ("-b", "operation,latency[aggr=quantize]")]


def cli_tree(dn, fixture_tree, idx, interval=None):
    one = os.path.join(fixture_tree, "2014", "05-01", "one.log")
    assert dn("datasource-add", "input", "--path=" + one,
              "--index-path=" + idx, "--time-field=time").code == 0
    assert dn("metric-add", "input", "m", "-b",
              "host,operation,req.method,latency[aggr=quantize]").code == 0
    extra = ("--interval=" + interval,) if interval else ()
    r = dn("build", *extra, "input")
    assert r.code == 0, r.err
    return extra


def tree_files(idx, suffix):
    out = []
    for d, _dirs, names in os.walk(idx):
        out += [os.path.join(d, n) for n in names if n.endswith(suffix)]
    return sorted(out)


def run_queries(dn, extra):
    out = []
    for case in CLI_QUERIES:
        r = dn("query", "--counters", *extra, *case, "input")
        assert r.code == 0, r.err
        out.append((r.out, r.err))
    return out


@pytest.mark.parametrize("damage", DAMAGES,
                         ids=[d.__name__[7:] for d in DAMAGES])
def test_query_output_with_damaged_sidecar(dn, fixture_tree, tmp_path,
                                           damage):
    """`dn query` prints the same with a damaged sidecar as with none."""
    idx = str(tmp_path / "idx")
    extra = cli_tree(dn, fixture_tree, idx)
    assert tree_files(idx, ".dncol") == []
    want = run_queries(dn, extra)
    from dragnet_amd.tools import index_columnar
    index_columnar.refresh(idx)
    for f in tree_files(idx, ".sqlite"):
        side = f + ".dncol"
        damage(side, f)
        assert C.open_sidecar(f, full=True) is None
    assert run_queries(dn, extra) == want


# ---- tree merge ----

def test_tree_merge(tmp_path):
    """Three sidecars with partly overlapping dictionaries, and an empty
    file between them."""
    metrics = [METRICS[1]]
    rows = {
        "a": [("x", "GET", 1), ("y", "PUT", 2), ("x", "PUT", 3)],
        "b": [],
        "c": [("z", "GET", 4), ("y", "GET", 5)],
        "d": [("y", "DEL", 6), ("w", "PUT", 7), ("x", "GET", 8),
              ("z", "PUT", 9)],
    }
    sidecars = []
    for name in sorted(rows):
        f = str(tmp_path / (name + ".sqlite"))
        sink = IndexSink(f, metrics)
        for host, method, v in rows[name]:
            sink.write_point({"fields": {
                "__dn_metric": 0, "host": host, "req.method": method},
                "value": v})
        sink.flush()
        C.write_sidecar(f)
        sidecars.append(C.open_sidecar(f))
    # the same string sits at different local codes
    local = [sc.column(0, "host")[1] for sc in sidecars]
    assert local[0].index(b"y") != local[3].index(b"y")

    q = QueryConfig(breakdowns=[{"name": "host"}, {"name": "req.method"}])
    groups, errors = C.group_sidecars(sidecars, q)
    assert errors == [] and len(groups) == 1
    found, members = groups[0]
    assert C.total_rows(members) == 9
    needed = C.needed_columns(q, found)
    assert needed == ["host", "req.method"]
    launches, rejected = C.merge_group(members, needed)
    assert rejected == [] and len(launches) == 1
    mg = launches[0]
    assert mg.members == sidecars
    assert mg.seg_start.dtype == np.uint32
    assert mg.seg_start.tolist() == [0, 3, 3, 5, 9]
    assert mg.nrows == 9
    # equal strings, equal global codes: the dictionary has no repeats
    assert len(set(mg.dict_values)) == len(mg.dict_values)
    blob, doff, dlen = mg.dictionary()
    words = [blob[o:o + n] for o, n in zip(doff.tolist(), dlen.tolist())]
    assert words == mg.dict_values
    got = [(words[h].decode(), words[m].decode(), v)
           for h, m, v in zip(mg.codes["host"].tolist(),
                              mg.codes["req.method"].tolist(),
                              mg.values.tolist())]
    # per file, rows in the file's own stored order
    for i, sc in enumerate(sidecars):
        a, b = mg.seg_start[i], mg.seg_start[i + 1]
        _k, cols, vals = sc.table(0)
        mine = []
        for r in range(len(vals)):
            cell = [c[0][c[1][r]:c[1][r] + c[2][r]].decode() for c in cols]
            mine.append((cell[0], cell[1], vals[r]))
        assert got[a:b] == mine
        assert sorted(mine) == sorted(
            (h, m, float(v)) for h, m, v in rows["abcd"[i]])
    assert mg.has_backslash == {"host": False, "req.method": False}

    # only the needed column is loaded
    q1 = QueryConfig(breakdowns=[{"name": "req.method"}])
    (found1, members1), = C.group_sidecars(sidecars, q1)[0]
    (mg1,), _ = C.merge_group(members1, C.needed_columns(q1, found1))
    assert list(mg1.codes) == ["req.method"] and mg1.nums == {}

    # a launch limit splits at file boundaries
    parts, rejected = C.merge_group(members, needed, max_rows=5)
    assert rejected == []
    assert [p.seg_start.tolist() for p in parts] == [[0, 3, 3, 5], [0, 4]]
    assert [len(p.members) for p in parts] == [3, 1]


def test_group_by_serving_metric(tmp_path):
    """Files whose serving metric differs land in different groups; a
    file no metric of which serves the query is an error."""
    def one_metric(name, metric, fields):
        sink = IndexSink(str(tmp_path / name), [metric])
        sink.write_point({"fields": dict(fields, __dn_metric=0),
                          "value": 1})
        sink.flush()
        return sink.filename

    fa = make_index(tmp_path / "a.sqlite", 3)
    fb = one_metric("b.sqlite", METRICS[2], {"lat": 3, "host": "h"})
    fc = one_metric("c.sqlite", METRICS[0], {})
    scs = []
    for f in (fa, fb, fc):
        C.write_sidecar(f)
        scs.append(C.open_sidecar(f))
    q = QueryConfig(breakdowns=[{"name": "host"}])
    groups, errors = C.group_sidecars(scs, q)
    assert [[sc.index_file for sc, _f in m] for _f, m in groups] == \
        [[fa], [fb]]
    assert [(sc.index_file, msg) for sc, msg in errors] == \
        [(fc, "no metrics available to serve query")]


# ---- opt-in, tool ----

@pytest.mark.parametrize("interval", ["all", "day", "hour"])
def test_build_writes_sidecars_only_when_asked(dn, fixture_tree, tmp_path,
                                               monkeypatch, interval):
    monkeypatch.delenv("DRAGNET_INDEX_COLUMNAR", raising=False)
    idx = str(tmp_path / "idx")
    cli_tree(dn, fixture_tree, idx, interval)
    assert tree_files(idx, ".dncol") == []
    listing = tree_files(idx, "")
    assert listing

    monkeypatch.setenv("DRAGNET_INDEX_COLUMNAR", "1")
    r = dn("build", "--interval=" + interval, "input")
    assert r.code == 0, r.err
    index_files = [f for f in tree_files(idx, "")
                   if not f.endswith(".dncol")]
    assert index_files == listing
    assert tree_files(idx, ".dncol") == [f + ".dncol" for f in listing]
    for f in listing:
        assert C.open_sidecar(f, full=True) is not None


def test_build_columnar_argument(fixture_tree, tmp_path, monkeypatch):
    from dragnet_amd.config import Datasource
    from dragnet_amd.datasource.file import FileDatasource
    from dragnet_amd.engine.cpu import CpuEngine
    monkeypatch.delenv("DRAGNET_INDEX_COLUMNAR", raising=False)
    one = os.path.join(fixture_tree, "2014", "05-01", "one.log")
    metrics = [{"name": "m", "filter": None, "breakdowns": [
        {"name": "host", "field": "host"}]}]
    for flag in (False, True):
        idx = str(tmp_path / ("idx%d" % flag))
        ds = Datasource(name="t", backend="file", path=one,
                        index_path=idx, time_field="time")
        files = FileDatasource(ds, engine=CpuEngine()).build(
            metrics, interval="day", columnar=flag)
        assert files
        assert tree_files(idx, ".dncol") == \
            ([f + ".dncol" for f in sorted(files)] if flag else [])


def test_partitioned_write_covers_owned_files_only(tmp_path):
    from dragnet_amd.datasource.file import write_index
    metrics = [{"name": "m", "filter": None, "breakdowns": [
        {"name": "host", "field": "host"}]}]
    points = [{"fields": {"__dn_metric": 0, "host": "h%d" % d,
                          "__dn_ts": 1398902400 + 86400 * d}, "value": 1}
              for d in range(5)]
    idx = str(tmp_path / "idx")
    world = 2
    owned = {}
    for rank in range(world):
        before = set(tree_files(idx, ".dncol"))
        written = write_index(idx, metrics, "day", points,
                              partition=(rank, world), columnar=True)
        owned[rank] = set(tree_files(idx, ".dncol")) - before
        assert owned[rank] == set(
            f + ".dncol" for i, f in enumerate(sorted(written))
            if i % world == rank)
    assert len(owned[0]) == 3 and len(owned[1]) == 2


def test_tool_is_idempotent_and_force_rewrites(dn, fixture_tree, tmp_path,
                                               capsys):
    from dragnet_amd.tools import index_columnar
    idx = str(tmp_path / "idx")
    cli_tree(dn, fixture_tree, idx)
    files = tree_files(idx, ".sqlite")
    assert index_columnar.main([idx]) == 0
    sides = tree_files(idx, ".dncol")
    assert sides == [f + ".dncol" for f in files]
    assert capsys.readouterr().out == "".join(
        "wrote %s\n" % s for s in sides)
    ids = [(os.stat(s).st_ino, os.stat(s).st_mtime_ns) for s in sides]

    assert index_columnar.main([idx]) == 0
    assert capsys.readouterr().out == "".join(
        "fresh %s\n" % s for s in sides)
    assert [(os.stat(s).st_ino, os.stat(s).st_mtime_ns)
            for s in sides] == ids

    # a stale one is refreshed, the others left alone
    st = os.stat(files[0])
    os.utime(files[0], ns=(st.st_atime_ns, st.st_mtime_ns + 10 ** 9))
    assert index_columnar.refresh(idx) == (1, len(files) - 1)
    assert C.open_sidecar(files[0], full=True) is not None

    content = [open(s, "rb").read() for s in sides]
    assert index_columnar.main(["--force", idx]) == 0
    assert capsys.readouterr().out == "".join(
        "wrote %s\n" % s for s in sides)
    assert [open(s, "rb").read() for s in sides] == content
    assert index_columnar.main([]) == 2


# ---- the CPU engine never reads sidecars ----

@pytest.mark.parametrize("interval", ["day", "hour"])
def test_cpu_engine_ignores_sidecars(dn, fixture_tree, tmp_path,
                                     monkeypatch, interval):
    monkeypatch.setenv("DRAGNET_ENGINE", "cpu")
    idx = str(tmp_path / "idx")
    extra = cli_tree(dn, fixture_tree, idx, interval)
    want = run_queries(dn, extra)
    from dragnet_amd.tools import index_columnar
    nwrote, _ = index_columnar.refresh(idx)
    assert nwrote == len(tree_files(idx, ".sqlite")) > 0
    before = dict(C.STATS)
    for mode in ("auto", "1", "0"):
        monkeypatch.setenv("DRAGNET_INDEX_GPU", mode)
        assert run_queries(dn, extra) == want
    assert C.STATS["sidecar_files"] == before["sidecar_files"]
    assert C.STATS["sidecar_launches"] == before["sidecar_launches"]


# ---- datasource routing, with a stand-in for the GPU engine ----

class StandInEngine(object):
    """Answers coded_query on the host, row by row, from the merged
    columns: what the kernels must compute."""
    name = "gpu"

    def __init__(self):
        self.launches = []

    def coded_query(self, query, filt, params, kinds, mg):
        from dragnet_amd import krill
        from dragnet_amd.points import Aggregator
        pred = krill.create_predicate(filt) if filt is not None else None
        self.launches.append([sc.index_file for sc in mg.members])
        parts = []
        for i in range(len(mg.members)):
            agg = Aggregator(query)
            for r in range(mg.seg_start[i], mg.seg_start[i + 1]):
                f = {n: a[r] for n, a in mg.nums.items()}
                f.update((n, mg.dict_values[a[r]].decode("utf-8"))
                         for n, a in mg.codes.items())
                nested = dict(f)  # the filter plucks dotted paths
                for n, v in f.items():
                    if "." in n:
                        head, tail = n.split(".", 1)
                        nested.setdefault(head, {})[tail] = v
                if pred is None or pred.eval(nested):
                    agg.write({"fields": f, "value": int(mg.values[r])})
            parts.append(agg)
        return parts


def test_query_routes_sidecar_files_through_one_launch(tmp_path,
                                                       monkeypatch):
    from dragnet_amd.config import Datasource
    from dragnet_amd.datasource.file import FileDatasource
    from dragnet_amd.query import query_load
    idx = str(tmp_path / "idx")
    files = [os.path.join(idx, "by_day", "2014-05-%02d.sqlite" % (k + 1))
             for k in range(4)]
    for k, f in enumerate(files):
        make_index(f, [0, 5, 65, 33][k], shift=k)
        if k != 3:
            C.write_sidecar(f)  # the last file has none
    st = os.stat(files[1])       # and the second one's is stale
    os.utime(files[1], ns=(st.st_atime_ns, st.st_mtime_ns + 10 ** 9))
    eng = StandInEngine()
    ds = Datasource(name="t", backend="file", path="/dev/null",
                    index_path=idx, time_field="time")
    fd = FileDatasource(ds, engine=eng)
    monkeypatch.delenv("DRAGNET_INDEX_COLUMNAR_ROWS", raising=False)

    def ask(mode, **kw):
        monkeypatch.setenv("DRAGNET_INDEX_GPU", mode)
        del eng.launches[:]
        res = fd.query(query_load(**kw), interval="day")
        assert not res.errors
        return (res.aggregators[0].points(), res.stages,
                [list(x) for x in eng.launches], res.sidecar_files)

    for kw in (dict(), dict(breakdown_specs="req.method"),
               dict(filter={"eq": ["req.method", "GET"]},
                    breakdown_specs="req.method"),
               dict(filter={"ge": ["lat", 3]},
                    breakdown_specs="lat[aggr=lquantize,step=1]")):
        want, wstages, launches, served = ask("0", **kw)
        assert launches == [] and served == []
        # auto: SQLite below the row threshold (and by default)
        assert ask("auto", **kw)[2] == []
        monkeypatch.setenv("DRAGNET_INDEX_COLUMNAR_ROWS", "1000")
        assert ask("auto", **kw)[2] == []
        monkeypatch.setenv("DRAGNET_INDEX_COLUMNAR_ROWS", "65")
        got, gstages, launches, served = ask("auto", **kw)
        assert launches == [[files[0], files[2]]]
        assert served == [files[0], files[2]]
        assert got == want
        assert gstages == wstages
        monkeypatch.delenv("DRAGNET_INDEX_COLUMNAR_ROWS")

    # a needed column with a backslash: no launch at all
    got, _s, launches, _f = ask("0", breakdown_specs="host")
    monkeypatch.setenv("DRAGNET_INDEX_COLUMNAR_ROWS", "0")
    assert ask("auto", breakdown_specs="host") == (got, _s, [], [])

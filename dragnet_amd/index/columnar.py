"""
Columnar index sidecars: a dictionary-coded cache of an index file's
metric tables, and the host-side merge of a tree's sidecars into one
launch for the GPU engine (GpuEngine.coded_query, engine/colquery.py).
numpy only: neither torch nor a GPU is needed here.

A sidecar for index file F is F.dncol.  It holds exactly what
_csink.read_columns returns for each metric table of F — built from the
FINISHED SQLite file, so TEXT-affinity coercions and NULL -> "" hold by
construction — with every string column dictionary-coded.  The .sqlite
file stays the index; the sidecar is optional, and a missing, stale or
damaged one only means that SQLite serves that file.

Layout (little-endian; docs/DESIGN.md):

    "DNCOLIX1" | u32 version | u32 header length | UTF-8 JSON header
    sections, each aligned to 64 bytes; the header names every section
    as [offset, length], offsets counted from the first 64-byte
    boundary after the header

    'n' column   f64[nrows]
    's' column   u32 codes[nrows], u32 off[ndict], u32 len[ndict], and
                 the byte blob of the ndict distinct values
    value        f64[nrows]

The header also carries the SQLite file's size and st_mtime_ns at the
time of writing (the freshness stamp), the dragnet_config rows and the
dragnet_metrics rows.

Reading validates on the host, before any byte reaches the device:
magic, version, stamp, every section inside the file and of its array's
length (open_sidecar); every dictionary span inside its blob and every
code below ndict (when a column is loaded).  A failure is logged at
info and reported as "no usable sidecar", never raised to the caller of
a query.
"""

import json
import os
import sqlite3
import struct

import numpy as np

from .query import (IndexError_, check_version, column_kinds, find_metric,
                    metric_entry)
from .sink import sqlite3_escape

MAGIC = b"DNCOLIX1"
VERSION = 1
SUFFIX = ".dncol"
ALIGN = 64
FILE_COLUMN = "__dn_file"  # the reserved trailing breakdown of a launch

# per-launch limits of the device side: u32 rows, u32 dictionary offsets
MAX_ROWS = (1 << 32) - 1
MAX_DICT_BYTES = (1 << 32) - 1

# Process-wide tally of how index queries were served, for tests and
# diagnostics: files and launches that took the sidecar path, files
# that SQLite (or the per-file extract path) served.
STATS = {"sidecar_files": 0, "sidecar_launches": 0, "other_files": 0}


class SidecarError(Exception):
    """This sidecar cannot be used (the reason is the message)."""


def _log():
    from ..log import get_logger
    return get_logger().child("index-columnar")


def sidecar_path(index_file):
    return index_file + SUFFIX


def is_sidecar_name(name):
    """A sidecar, or the temporary file one is written through."""
    return name.endswith(SUFFIX) or (SUFFIX + ".") in name


def enabled_by_env():
    return os.environ.get("DRAGNET_INDEX_COLUMNAR") == "1"


def _align(n):
    return (n + ALIGN - 1) & ~(ALIGN - 1)


# ---- extraction out of the finished SQLite file ----

def _csink_or_none():
    try:
        from . import _csink
        return _csink
    except ImportError:
        return None


def _py_read_columns(path, table, names, kinds):
    """read_columns without the native reader: the same (cols, vals)
    shape.  CAST gives what sqlite3_column_text / _double coerce to."""
    exprs = ["CAST(%s AS %s)" % (n, "REAL" if k == "n" else "TEXT")
             for n, k in zip(names, kinds)]
    sql = "SELECT %s from %s" % (
        ", ".join(exprs + ["CAST(value AS REAL)"]), table)
    db = sqlite3.connect("file:%s?mode=ro" % path, uri=True)
    db.text_factory = bytes
    try:
        rows = db.execute(sql).fetchall()
    finally:
        db.close()
    cols = []
    for ci, k in enumerate(kinds):
        if k == "n":
            cols.append(np.array([r[ci] or 0.0 for r in rows],
                                 dtype=np.float64))
        else:
            vals = [r[ci] or b"" for r in rows]
            lens = np.array([len(v) for v in vals], dtype=np.uint32)
            offs = np.zeros(len(vals), dtype=np.uint32)
            if len(vals):
                offs[1:] = np.cumsum(lens[:-1], dtype=np.uint64)
            cols.append((b"".join(vals), offs, lens))
    vals = np.array([r[-1] or 0.0 for r in rows], dtype=np.float64)
    return cols, vals


def read_table(path, met, native=None):
    """(kinds, cols, vals) of one metric table, as _csink.read_columns
    returns them; native=False forces the pure-Python extractor."""
    params = met["params"]
    kinds = column_kinds(params)
    names = [sqlite3_escape(p["name"]) for p in params]
    table = "dragnet_index_%d" % met["id"]
    cs = _csink_or_none() if native in (None, True) else None
    if cs is None:
        cols, vals = _py_read_columns(path, table, names, kinds)
    else:
        sql = "SELECT %s from %s" % (", ".join(names + ["value"]), table)
        cols, vals = cs.read_columns(path, sql, kinds)
    return kinds, cols, vals


def read_catalog(path):
    """(config rows as [key, value] pairs, dragnet_metrics rows as
    [id, label, filter, params]) of an index file."""
    db = sqlite3.connect("file:%s?mode=ro" % path, uri=True)
    try:
        config = [list(r) for r in db.execute(
            "SELECT key, value FROM dragnet_config")]
        metrics = [list(r) for r in db.execute(
            "SELECT id, label, filter, params FROM dragnet_metrics "
            "ORDER BY id")]
    finally:
        db.close()
    return config, metrics


# ---- dictionary coding ----

_CHUNK = 1 << 18


def dict_encode(blob, offs, lens):
    """(codes u32[nrows], distinct values as a sorted list of bytes)."""
    n = len(offs)
    if n == 0:
        return np.zeros(0, dtype=np.uint32), []
    maxlen = int(lens.max())
    if maxlen == 0:
        return np.zeros(n, dtype=np.uint32), [b""]
    if b"\0" in blob or maxlen > 256:
        # fixed-width byte strings drop trailing NULs: code row by row
        mv = memoryview(blob)
        rows = [bytes(mv[o:o + ln])
                for o, ln in zip(offs.tolist(), lens.tolist())]
        values = sorted(set(rows))
        where = {v: i for i, v in enumerate(values)}
        return np.array([where[r] for r in rows], dtype=np.uint32), values
    arr = np.frombuffer(blob, dtype=np.uint8)
    span = np.arange(maxlen, dtype=np.int64)
    fixed = []
    for a in range(0, n, _CHUNK):
        o = offs[a:a + _CHUNK].astype(np.int64)[:, None]
        ln = lens[a:a + _CHUNK].astype(np.int64)[:, None]
        idx = np.minimum(o + span, len(arr) - 1)
        mat = np.where(span < ln, arr[idx], 0).astype(np.uint8)
        fixed.append(np.ascontiguousarray(mat).view("S%d" % maxlen)[:, 0])
    distinct = np.unique(np.concatenate([np.unique(f) for f in fixed]))
    codes = np.concatenate([np.searchsorted(distinct, f) for f in fixed])
    return codes.astype(np.uint32), [bytes(v) for v in distinct]


# ---- writing ----

def encode_sidecar(stamp, config, metric_rows, tables):
    """The bytes of a sidecar.  tables: per metric row, (kinds, cols,
    vals) as read_table returns them — whichever extractor fed it."""
    sections = []
    pos = [0]

    def add(data):
        data = bytes(data)
        at = pos[0]
        sections.append((at, data))
        pos[0] = _align(at + len(data))
        return [at, len(data)]

    metrics = []
    for (mid, label, filt, params), (kinds, cols, vals) in zip(
            metric_rows, tables):
        nrows = int(len(vals))
        columns = []
        for k, c in zip(kinds, cols):
            if k == "n":
                columns.append({"kind": "n", "data": add(
                    np.ascontiguousarray(c, dtype="<f8").tobytes())})
                continue
            codes, values = dict_encode(c[0], np.asarray(c[1]),
                                        np.asarray(c[2]))
            dlen = np.array([len(v) for v in values], dtype="<u4")
            doff = np.zeros(len(values), dtype="<u4")
            if len(values):
                doff[1:] = np.cumsum(dlen[:-1], dtype=np.uint64)
            columns.append({
                "kind": "s",
                "codes": add(codes.astype("<u4").tobytes()),
                "off": add(doff.tobytes()),
                "len": add(dlen.tobytes()),
                "blob": add(b"".join(values)),
                "ndict": len(values),
                "has_backslash": any(b"\\" in v for v in values),
            })
        metrics.append({
            "id": mid, "label": label, "filter": filt, "params": params,
            "nrows": nrows, "columns": columns,
            "value": add(np.ascontiguousarray(vals, dtype="<f8").tobytes()),
        })
    header = json.dumps({
        "sqlite_size": stamp[0], "sqlite_mtime_ns": stamp[1],
        "config": config, "metrics": metrics,
    }, separators=(",", ":")).encode("utf-8")
    out = bytearray(MAGIC + struct.pack("<II", VERSION, len(header))
                    + header)
    base = _align(len(out))
    out.extend(b"\0" * (base - len(out)))
    for at, data in sections:
        out.extend(b"\0" * (base + at - len(out)))
        out.extend(data)
    return bytes(out)


def write_sidecar(index_file, native=None):
    """Build index_file's sidecar from the finished SQLite file; write
    to <sidecar>.<pid>, then rename into place.  Returns its path."""
    st = os.stat(index_file)
    config, metric_rows = read_catalog(index_file)
    tables = [read_table(index_file,
                         metric_entry(mid, label, filt, params), native)
              for mid, label, filt, params in metric_rows]
    data = encode_sidecar((st.st_size, st.st_mtime_ns), config,
                          metric_rows, tables)
    path = sidecar_path(index_file)
    tmp = "%s.%d" % (path, os.getpid())
    with open(tmp, "wb") as f:
        f.write(data)
    os.replace(tmp, path)
    return path


# ---- reading ----

class Sidecar(object):
    """An opened, header-validated sidecar.  metrics holds
    IndexQuerier.metrics entries, each with "nrows" added."""

    def __init__(self, index_file, path, header, base, size):
        self.index_file = index_file
        self.path = path
        self.config = dict((k, v) for k, v in header["config"])
        self.metrics = []
        self._layout = {}
        self._base = base
        for m in header["metrics"]:
            ent = metric_entry(m["id"], m["label"], m["filter"],
                               m["params"])
            ent["nrows"] = int(m["nrows"])
            self.metrics.append(ent)
            self._layout[m["id"]] = m
        self._check_sections(size)

    def _check_sections(self, size):
        def sect(s, count, item):
            off, ln = int(s[0]), int(s[1])
            if off < 0 or ln < 0 or self._base + off + ln > size:
                raise SidecarError("section past the end of the file")
            if count is not None and ln != count * item:
                raise SidecarError("section of the wrong length")

        for ent in self.metrics:
            m = self._layout[ent["id"]]
            nrows = ent["nrows"]
            kinds = column_kinds(ent["params"])
            if nrows < 0 or len(m["columns"]) != len(kinds):
                raise SidecarError("columns do not match the params")
            sect(m["value"], nrows, 8)
            for k, c in zip(kinds, m["columns"]):
                if c["kind"] != k:
                    raise SidecarError("column of the wrong kind")
                if k == "n":
                    sect(c["data"], nrows, 8)
                    continue
                ndict = int(c["ndict"])
                if ndict < 0:
                    raise SidecarError("negative dictionary size")
                sect(c["codes"], nrows, 4)
                sect(c["off"], ndict, 4)
                sect(c["len"], ndict, 4)
                sect(c["blob"], None, 1)

    def metric(self, mid):
        for ent in self.metrics:
            if ent["id"] == mid:
                return ent
        raise SidecarError("no such metric")

    def _read(self, s, dtype):
        item = np.dtype(dtype).itemsize
        with open(self.path, "rb") as f:
            a = np.fromfile(f, dtype=dtype, count=int(s[1]) // item,
                            offset=self._base + int(s[0]))
        if a.size * item != int(s[1]):
            raise SidecarError("short read")
        return a

    def values(self, mid):
        return self._read(self._layout[mid]["value"], "<f8")

    def column_info(self, mid, name):
        ent = self.metric(mid)
        for p, c in zip(ent["params"], self._layout[mid]["columns"]):
            if p["name"] == name:
                return c
        raise SidecarError("no such column")

    def column(self, mid, name):
        """An 'n' column -> f64[nrows]; an 's' column -> (codes
        u32[nrows], distinct values as a list of bytes), with every
        dictionary span and every code checked."""
        c = self.column_info(mid, name)
        if c["kind"] == "n":
            return self._read(c["data"], "<f8")
        codes = self._read(c["codes"], "<u4")
        doff = self._read(c["off"], "<u4").astype(np.int64)
        dlen = self._read(c["len"], "<u4").astype(np.int64)
        blob = self._read(c["blob"], np.uint8).tobytes()
        if len(doff) and int((doff + dlen).max()) > len(blob):
            raise SidecarError("dictionary span past the blob")
        if len(codes) and int(codes.max()) >= len(doff):
            raise SidecarError("code past the dictionary")
        values = [blob[o:o + ln] for o, ln in zip(doff.tolist(),
                                                   dlen.tolist())]
        return codes, values

    def table(self, mid):
        """(kinds, cols, vals) decoded back to read_columns' shape
        (tests, diagnostics)."""
        ent = self.metric(mid)
        kinds = column_kinds(ent["params"])
        cols = []
        for p, k in zip(ent["params"], kinds):
            c = self.column(mid, p["name"])
            if k == "n":
                cols.append(c)
                continue
            codes, values = c
            lens = np.array([len(v) for v in values],
                            dtype=np.uint32)[codes]
            offs = np.zeros(len(codes), dtype=np.uint32)
            if len(codes):
                offs[1:] = np.cumsum(lens[:-1], dtype=np.uint64)
            cols.append((b"".join(values[c_] for c_ in codes.tolist()),
                         offs, lens))
        return kinds, cols, self.values(mid)


def open_sidecar(index_file, st=None, full=False):
    """The usable sidecar of index_file, or None (reason logged at
    info).  full=True also loads and checks every column."""
    path = sidecar_path(index_file)
    try:
        with open(path, "rb") as f:
            size = os.fstat(f.fileno()).st_size
            head = f.read(16)
            if len(head) < 16 or head[:8] != MAGIC:
                raise SidecarError("bad magic")
            version, hlen = struct.unpack("<II", head[8:])
            if version != VERSION:
                raise SidecarError("unsupported version %d" % version)
            if 16 + hlen > size:
                raise SidecarError("header past the end of the file")
            header = json.loads(f.read(hlen).decode("utf-8"))
        if st is None:
            st = os.stat(index_file)
        if (header["sqlite_size"] != st.st_size
                or header["sqlite_mtime_ns"] != st.st_mtime_ns):
            raise SidecarError("stale: the index file has changed")
        sc = Sidecar(index_file, path, header, _align(16 + hlen), size)
        if full:
            for ent in sc.metrics:
                sc.table(ent["id"])
        return sc
    except FileNotFoundError:
        return None
    except (SidecarError, OSError, ValueError, KeyError, TypeError,
            IndexError, AttributeError, OverflowError) as e:
        _log().info("sidecar not usable", path=path, reason=str(e))
        return None


# ---- tree merge ----

class Merged(object):
    """One launch: the needed columns of `members` (Sidecars, in file
    order) concatenated.

    params / kinds   the served metric's, as columnar_query takes them
    datefield, ignore_filter   of find_metric, equal for every member
    seg_start        u32[nfiles + 1] first row of each member
    values           f64[nrows]
    nums             {column name: f64[nrows]}
    codes            {column name: u32[nrows]} into the launch dictionary
    dict_values      the launch dictionary: distinct bytes, code order
    has_backslash    {string column name: bool}
    """

    def __init__(self):
        self.members = []
        self.nums = {}
        self.codes = {}
        self.dict_values = []
        self.has_backslash = {}

    @property
    def nrows(self):
        return int(self.seg_start[-1])

    def dictionary(self):
        """(blob bytes, u32 off[ndict], u32 len[ndict])."""
        dlen = np.array([len(v) for v in self.dict_values],
                        dtype=np.uint32)
        doff = np.zeros(len(dlen), dtype=np.uint32)
        if len(dlen):
            doff[1:] = np.cumsum(dlen[:-1], dtype=np.uint64)
        return b"".join(self.dict_values), doff, dlen


def needed_columns(query, found):
    """Names of the metric columns a query reads: its breakdowns'
    source columns, its filter's fields (unless the metric's own filter
    already applied it) and the date column of a time-bounded query."""
    names = [b.get("field", b["name"]) for b in query.breakdowns]
    if query.filter is not None and not found["ignore_filter"]:
        from .. import krill
        names += list(krill.create_predicate(query.filter).fields())
    if found["datefield"]:
        names.append(found["datefield"])
    have = set(p["name"] for p in found["params"])
    out = []
    for n in names:
        if n in have and n not in out:
            out.append(n)
    return out


def group_sidecars(sidecars, query):
    """Group sidecars (file order kept) by the metric that serves the
    query -> (groups, errors).  groups: list of (found, [(sidecar,
    found)...]) keyed by (params, datefield, ignore_filter); errors:
    [(sidecar, message)] for files no metric of which serves it."""
    groups = {}
    errors = []
    for sc in sidecars:
        try:
            check_version(sc.config)
            found = find_metric(sc.metrics, query)
        except IndexError_ as e:
            errors.append((sc, str(e)))
            continue
        key = (json.dumps(found["params"], sort_keys=True),
               found["datefield"], found["ignore_filter"])
        groups.setdefault(key, (found, []))[1].append((sc, found))
    return list(groups.values()), errors


def merge_group(members, needed, max_rows=MAX_ROWS,
                max_dict_bytes=MAX_DICT_BYTES):
    """Merge one group's members [(sidecar, found)] into launches ->
    (list of Merged, rejected sidecars).  A member whose columns fail
    their checks, or that alone exceeds a launch, is rejected (SQLite
    serves it).  Launches split at file boundaries."""
    launches = []
    rejected = []
    cur = None
    parts = None
    where = None
    nbytes = 0

    def close():
        if cur is None or not cur.members:
            return
        rows = [len(v) for v in parts["value"]]
        cur.seg_start = np.zeros(len(rows) + 1, dtype=np.uint32)
        cur.seg_start[1:] = np.cumsum(rows, dtype=np.uint64)
        cur.values = np.concatenate(parts["value"])
        for n in needed:
            arrs = parts[n]
            if n in cur.has_backslash:
                cur.codes[n] = np.concatenate(arrs).astype(np.uint32)
            else:
                cur.nums[n] = np.concatenate(arrs)
        launches.append(cur)

    for sc, found in members:
        mid = found["id"]
        try:
            kinds = dict(zip((p["name"] for p in found["params"]),
                             column_kinds(found["params"])))
            loaded = {n: sc.column(mid, n) for n in needed}
            vals = sc.values(mid)
            infos = {n: sc.column_info(mid, n) for n in needed}
        except (SidecarError, OSError, ValueError, KeyError) as e:
            _log().info("sidecar not usable", path=sc.path, reason=str(e))
            rejected.append(sc)
            continue
        add_bytes = sum(sum(len(v) for v in loaded[n][1])
                        for n in needed if kinds[n] == "s")
        if len(vals) > max_rows or add_bytes > max_dict_bytes:
            rejected.append(sc)
            continue
        if cur is not None and (
                sum(len(v) for v in parts["value"]) + len(vals) > max_rows
                or nbytes + add_bytes > max_dict_bytes):
            close()
            cur = None
        if cur is None:
            cur = Merged()
            cur.params = found["params"]
            cur.kinds = column_kinds(found["params"])
            cur.datefield = found["datefield"]
            cur.ignore_filter = found["ignore_filter"]
            cur.has_backslash = {n: False for n in needed
                                 if kinds[n] == "s"}
            parts = {n: [] for n in needed}
            parts["value"] = []
            where = {}
            nbytes = 0
        cur.members.append(sc)
        parts["value"].append(vals)
        nbytes += add_bytes
        for n in needed:
            if kinds[n] == "n":
                parts[n].append(loaded[n])
                continue
            codes, values = loaded[n]
            # the launch dictionary: a dict over the DISTINCT values
            remap = np.zeros(len(values), dtype=np.uint32)
            for i, v in enumerate(values):
                g = where.get(v)
                if g is None:
                    g = where[v] = len(cur.dict_values)
                    cur.dict_values.append(v)
                remap[i] = g
            parts[n].append(remap[codes] if len(codes)
                            else np.zeros(0, dtype=np.uint32))
            if infos[n].get("has_backslash") or any(
                    b"\\" in v for v in values):
                cur.has_backslash[n] = True
    close()
    return launches, rejected


def total_rows(members):
    """Rows the launch would read, known from the headers alone."""
    return sum(sc.metric(found["id"])["nrows"] for sc, found in members)

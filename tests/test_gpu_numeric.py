"""
Numeric fidelity of the HIP scan (pytest -m gpu): JSON number parse
(K1), ToNumber coercion and relational filters (K2), ISO date parse
(K3) and bucketing (K4) against IEEE / ECMAScript truth.

Every record is {"id": "<k>", "n": <literal>} under breakdown `id,n`,
so each literal lands in its own group and a mismatch names it.  Every
test asserts two things:

  (a) GPU == CPU oracle: points, ninputs, nonnumeric drops and the
      json parser stage, exactly;
  (b) GPU == independent truth computed here without the package: the
      key of literal L is the JS string of float(L) (Python float() is
      correctly rounded; numeric_cases.js_tostring is pinned against
      V8 by test_numeric_cpu.py).  Shortest-repr strings are unique
      per double, so string equality is bit equality (+-0 both "0").

Literals of more than 19 significant digits are held to (b'): the
device keeps 19 digits, so the result is float(L) or one of its two
neighbours — the one divergence that stays documented.
"""

import datetime
import json
import math

import pytest

import numeric_cases as nc
from numeric_cases import (EPOCH, civil_ms, date_cases, geometry_records,
                           string_cases)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engines():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from dragnet_amd.engine.cpu import CpuEngine
    from dragnet_amd.engine.gpu import GpuEngine
    return CpuEngine(), GpuEngine()


def q(**kw):
    from dragnet_amd.query import query_load
    return query_load(**kw)


def assert_same(c, g, loose_ids=()):
    """(a).  Records named in loose_ids carry a literal of more than
    19 significant digits: both engines must still group them (same
    ids on both sides), but their keys are compared under (b') by the
    caller, not with the oracle."""
    def strict(points):
        return [p for p in points if p["fields"].get("id") not in loose_ids]

    def ids(points):
        return sorted(p["fields"]["id"] for p in points
                      if p["fields"].get("id") in loose_ids)

    for ca, ga in zip(c.aggregators, g.aggregators):
        assert strict(ga.points()) == strict(ca.points())
        assert ids(ga.points()) == ids(ca.points())
        assert ga.ninputs == ca.ninputs
        assert ga.ndropped_nonnumeric == ca.ndropped_nonnumeric
    assert dict(g.stages)["json parser"] == dict(c.stages)["json parser"]


def scan_both(engines, tmp_path, data, queries, loose_ids=(), **kw):
    cpu, gpu = engines
    path = tmp_path / "num.ndjson"
    path.write_bytes(data)
    qs = queries if isinstance(queries, list) else [queries]
    c = cpu.scan([str(path)], qs, **kw)
    g = gpu.scan([str(path)], qs, **kw)
    assert_same(c, g, loose_ids)
    return c, g


def by_id(agg, field="n"):
    out = {}
    for p in agg.points():
        assert p["value"] == 1, p
        assert p["fields"]["id"] not in out
        out[p["fields"]["id"]] = p["fields"][field]
    return out


def loose_ids_of(lits):
    return {str(i) for i, lit in enumerate(lits) if nc.sig_digits(lit) > 19}


def number_lines(lits):
    return b"".join(('{"id": "%d", "n": %s}\n' % (i, lit)).encode()
                    for i, lit in enumerate(lits))


def check_literal_truth(got, lits):
    """(b) / (b'): got maps record id -> decoded key of `n`."""
    bad = []
    for i, lit in enumerate(lits):
        key = got.get(str(i))
        x = float(lit)
        if nc.sig_digits(lit) <= 19:
            ok = key == nc.js_tostring(x)
        else:
            ok = key in {nc.js_tostring(y) for y in nc.neighbours(x)}
        if not ok:
            bad.append((lit, key, nc.js_tostring(x)))
    assert not bad, "%d wrong, first: %r" % (len(bad), bad[:10])
    assert len(got) == len(lits)


@pytest.fixture(scope="module")
def class_corpus():
    """The eight literal classes (400 each) + specials + ties."""
    by_class = nc.literal_classes()
    assert len(by_class) == 8 and all(
        len(v) == 400 for v in by_class.values())
    lits = sum(by_class.values(), []) + nc.special_literals()
    assert len(lits) <= 4000
    return lits


# ---- literal classes -------------------------------------------------

def test_literal_classes_linear(engines, tmp_path, class_corpus):
    _c, g = scan_both(engines, tmp_path, number_lines(class_corpus),
                      q(breakdown_specs="id,n"),
                      loose_ids=loose_ids_of(class_corpus))
    check_literal_truth(by_id(g.aggregators[0]), class_corpus)


def test_literal_classes_per_class(engines, tmp_path):
    """Same corpus grouped by value alone: a wrong last bit also shows
    as a different number of distinct groups than distinct doubles."""
    by_class = nc.literal_classes()
    for name, lits in by_class.items():
        _c, g = scan_both(engines, tmp_path, number_lines(lits),
                          q(breakdown_specs="n"))
        want = {}
        for lit in lits:
            k = nc.truth_key(lit)
            want[k] = want.get(k, 0) + 1
        got = {p["fields"]["n"]: p["value"]
               for p in g.aggregators[0].points()}
        assert got == want, name


def test_infinity_literals_drop_under_a_bucketizer(engines, tmp_path):
    """1e400 parses to Infinity (the oracle groups it so); under
    quantize/lquantize it is a nonnumeric drop, not a bucket."""
    lits = ["1e400", "-1e400", "1.7976931348623159e308", "1e300", "5"]
    for spec in ("id,n[aggr=quantize]", "id,n[aggr=lquantize,step=10]"):
        c, g = scan_both(engines, tmp_path, number_lines(lits),
                         q(breakdown_specs=spec))
        assert g.aggregators[0].ndropped_nonnumeric == 3
        assert sorted(by_id(g.aggregators[0])) == ["3", "4"]


# ---- SWAR digit-run geometry -----------------------------------------

def test_digit_run_geometry(engines, tmp_path):
    recs = geometry_records()
    assert len(recs) <= 4000 * 2
    half = len(recs) // 2
    for part in (recs[:half], recs[half:]):
        assert len(part) <= 4000
        data = "".join(ln + "\n" for ln, _ in part).encode()
        loose = {json.loads(ln.split(', "p"')[0] + "}")["id"]
                 for ln, lit in part
                 if lit is not None and nc.sig_digits(lit) > 19}
        _c, g = scan_both(engines, tmp_path, data,
                          q(breakdown_specs="id,n"), loose_ids=loose)
        got = by_id(g.aggregators[0])
        ninvalid = sum(1 for _ln, lit in part if lit is None)
        st = dict(g.stages)["json parser"]
        assert st["invalid json"] == ninvalid
        bad = []
        for ln, lit in part:
            rid = json.loads(ln.split(', "p"')[0] + "}")["id"]
            if lit is None:
                assert rid not in got, ln
                continue
            x = float(lit)
            if nc.sig_digits(lit) <= 19:
                ok = got.get(rid) == nc.js_tostring(x)
            else:
                ok = got.get(rid) in {nc.js_tostring(y)
                                      for y in nc.neighbours(x)}
            if not ok:
                bad.append((ln, got.get(rid), nc.js_tostring(x)))
        assert not bad, "%d wrong, first: %r" % (len(bad), bad[:10])


@pytest.mark.parametrize("newline", [True, False])
@pytest.mark.parametrize("last", [
    '{"id": "2", "n": 99999999}', '{"id": "2", "n": 1234567.8901234567}',
    '{"id": "2", "n": 12345678', "99999999", "1234567890123456",
    "0.00000001234", "-1e5", "1e", "12."])
def test_last_record_of_the_file(engines, tmp_path, last, newline):
    """A digit run that ends at the last byte of the input: with and
    without the trailing newline, as an object field and as a bare
    top-level number (the run then stops at the record end, not at a
    terminator byte)."""
    lits = ["1.5", "0.30000000000000004"]
    data = number_lines(lits) + last.encode() + (b"\n" if newline else b"")
    _c, g = scan_both(engines, tmp_path, data, q(breakdown_specs="id,n"))
    got = {p["fields"]["id"]: p["fields"]["n"]
           for p in g.aggregators[0].points()}
    assert got["0"] == "1.5" and got["1"] == "0.30000000000000004"
    try:
        rec = json.loads(last)
    except ValueError:
        rec = None
    st = dict(g.stages)["json parser"]
    assert st["invalid json"] == (1 if rec is None else 0)
    if isinstance(rec, dict):
        assert got["2"] == nc.js_tostring(float(rec["n"]))
    elif rec is not None:
        assert got["undefined"] == "undefined"


# ---- byte sources ----------------------------------------------------

def test_literal_classes_wave_transposed(engines, tmp_path, class_corpus):
    """scan_kernel_x instantiates parse_json_number over XBytesT."""
    cpu, gpu = engines
    from dragnet_amd.engine import plan as planmod
    from dragnet_amd.engine.gpu import _ScanContext
    pool = number_lines(class_corpus)
    path = tmp_path / "xp.ndjson"
    path.write_bytes(pool)
    query = q(breakdown_specs="id,n")
    exp = cpu.scan([str(path)], [query])
    cplan = planmod.compile_plan([query])
    ctx = _ScanContext(gpu, cplan, agg_slots=1 << 15,
                       dict_slots=1 << 15, dict_data_cap=8 << 20)
    ctx.stage_xpose(pool)
    ctx.reset()
    ctx.scan_xpose()
    aggs, stages = ctx.finalize([query])
    loose = loose_ids_of(class_corpus)
    assert [p for p in aggs[0].points()
            if p["fields"]["id"] not in loose] == \
        [p for p in exp.aggregators[0].points()
         if p["fields"]["id"] not in loose]
    assert aggs[0].ninputs == exp.aggregators[0].ninputs
    assert dict(stages)["json parser"] == dict(exp.stages)["json parser"]
    check_literal_truth(by_id(aggs[0]), class_corpus)


def test_literal_classes_lds_staged(engines, tmp_path, class_corpus,
                                    monkeypatch):
    """DRAGNET_LDS_STAGE parses from the block's LDS tile (Bytes with a
    bias) instead of the global chunk."""
    monkeypatch.setenv("DRAGNET_LDS_STAGE", "1")
    _c, g = scan_both(engines, tmp_path, number_lines(class_corpus),
                      q(breakdown_specs="id,n"),
                      loose_ids=loose_ids_of(class_corpus))
    check_literal_truth(by_id(g.aggregators[0]), class_corpus)


# ---- js_to_number ----------------------------------------------------

def string_lines(cases):
    return b"".join(('{"id": "%d", "s": %s}\n' % (i, raw)).encode()
                    for i, (raw, _v) in enumerate(cases))


def finite(v):
    return v == v and abs(v) != math.inf


def test_string_coercion_under_bucketizers(engines, tmp_path):
    cases = string_cases()
    assert len(cases) <= 4000
    for raw, _v in cases:
        json.loads(raw)  # the corpus itself is valid JSON
    qs = [q(breakdown_specs="id,s[aggr=lquantize,step=1]"),
          q(breakdown_specs="id,s[aggr=quantize]")]
    _c, g = scan_both(engines, tmp_path, string_lines(cases), qs)
    ndrop = sum(1 for _r, v in cases if not finite(v))
    lq, p2 = by_id(g.aggregators[0], "s"), by_id(g.aggregators[1], "s")
    assert g.aggregators[0].ndropped_nonnumeric == ndrop
    assert g.aggregators[1].ndropped_nonnumeric == ndrop
    bad = []
    for i, (raw, v) in enumerate(cases):
        rid = str(i)
        if not finite(v):
            if rid in lq or rid in p2:
                bad.append((raw, "not dropped", lq.get(rid)))
            continue
        want_lq = math.floor(v)
        want_p2 = 0 if v < 1 else 2 ** (math.frexp(v)[1] - 1)
        if lq.get(rid) != want_lq or p2.get(rid) != want_p2:
            bad.append((raw, lq.get(rid), want_lq, p2.get(rid), want_p2))
    assert not bad, "%d wrong, first: %r" % (len(bad), bad[:10])


def test_string_coercion_under_numeric_filters(engines, tmp_path):
    cases = string_cases()
    filters = [("ge", 0), ("lt", 0), ("eq", 26), ("eq", 0), ("ne", 12),
               ("le", 12), ("gt", 1e17), ("eq", 18446744073709551616),
               ("lt", 1e-13), ("eq", math.inf), ("le", -math.inf)]
    ops = {"lt": lambda a, b: a < b, "le": lambda a, b: a <= b,
           "gt": lambda a, b: a > b, "ge": lambda a, b: a >= b,
           "eq": lambda a, b: a == b, "ne": lambda a, b: a != b}
    data = string_lines(cases)
    for op, const in filters:
        if const in (math.inf, -math.inf):
            # JSON filters carry no Infinity literal: a numeric string
            # constant compares numerically against string fields only
            # when both are strings -> lexical; skip non-JSON constants
            continue
        _c, g = scan_both(engines, tmp_path, data,
                          q(filter={op: ["s", const]},
                            breakdown_specs="id"))
        got = {p["fields"]["id"] for p in g.aggregators[0].points()}
        want = {str(i) for i, (_r, v) in enumerate(cases)
                if ops[op](v, float(const))}
        assert got == want, (op, const, sorted(got ^ want)[:10])


# ---- bucket boundaries (K4) ------------------------------------------

def test_quantize_boundaries(engines, tmp_path):
    vals = []
    for k in list(range(-2, 66)) + [100, 255, 256, 511, 512, 1000, 1022,
                                    1023]:
        v = 2.0 ** k
        vals += [v, math.nextafter(v, 0.0), math.nextafter(v, math.inf)]
    vals += [1.0, 0.9999999999999999, 0.0, -0.0, -1.0, -2.5, -1e300,
             5e-324, 1.7976931348623157e308, 3.0, 1e15, 1e16, 1e22]
    lits = [repr(v) for v in vals] + ["-0", "1", "2", "4294967296"]
    assert all(math.isfinite(float(x)) for x in lits)
    _c, g = scan_both(engines, tmp_path, number_lines(lits),
                      q(breakdown_specs="id,n[aggr=quantize]"))
    got = by_id(g.aggregators[0])
    assert g.aggregators[0].ndropped_nonnumeric == 0
    bad = []
    for i, lit in enumerate(lits):
        v = float(lit)
        want = 0 if v < 1 else 2 ** (math.frexp(v)[1] - 1)
        if got.get(str(i)) != want:
            bad.append((lit, got.get(str(i)), want))
    assert not bad, bad[:10]


@pytest.mark.parametrize("step", [1, 7, 10, 1000])
def test_lquantize_boundaries(engines, tmp_path, step):
    """floor(v/step), not truncation, below zero; ordinals either side
    of the +-2^29 packed-ordinal escape, +-2^53, +-2^63 and +-1e300
    (far outside any integer type)."""
    vals = []
    ks = list(range(0, 6)) + [99, 2 ** 29 - 1, 2 ** 29, 2 ** 29 + 1,
                              2 ** 31, 2 ** 32, 2 ** 53, 2 ** 63, 2 ** 64]
    for k in ks:
        for sgn in (1, -1):
            v = float(sgn * k * step)
            vals += [v, math.nextafter(v, -math.inf),
                     math.nextafter(v, math.inf)]
    vals += [1e300, -1e300, 1.7976931348623157e308,
             -1.7976931348623157e308, 0.5, -0.5, -0.0, 5e-324, -5e-324,
             step - 1e-9, -(step - 1e-9), 2.5 * step, -2.5 * step]
    lits = [repr(v) for v in vals]
    _c, g = scan_both(
        engines, tmp_path, number_lines(lits),
        q(breakdown_specs="id,n[aggr=lquantize,step=%d]" % step))
    got = by_id(g.aggregators[0])
    assert g.aggregators[0].ndropped_nonnumeric == 0
    bad = []
    for i, lit in enumerate(lits):
        want = math.floor(float(lit) / step) * step
        if got.get(str(i)) != want:
            bad.append((lit, got.get(str(i)), want))
    assert not bad, bad[:10]


# ---- filter boundaries (K2) ------------------------------------------

PY_OPS = {"lt": lambda a, b: a < b, "le": lambda a, b: a <= b,
          "gt": lambda a, b: a > b, "ge": lambda a, b: a >= b,
          "eq": lambda a, b: a == b, "ne": lambda a, b: a != b}


@pytest.mark.parametrize("const", [0.3, 0.1, 9007199254740992, 1e21, -0.0])
def test_filter_boundaries(engines, tmp_path, const):
    """Each relational op at the constant itself and both neighbouring
    doubles, written shortest and with 20 digits, as numbers and as
    numeric strings."""
    c = float(const)
    lits = []
    for v in (c, math.nextafter(c, -math.inf), math.nextafter(c, math.inf)):
        lits += [repr(v), "%.19e" % v]
    if c == 0:
        lits += ["0", "-0", "0.0", "0e999"]
    rows = [(lit, lit) for lit in lits] + \
           [('"%s"' % lit, lit) for lit in lits]
    data = b"".join(('{"id": "%d", "n": %s}\n' % (i, raw)).encode()
                    for i, (raw, _l) in enumerate(rows))
    ops = sorted(PY_OPS)
    qs = [q(filter={op: ["n", const]}, breakdown_specs="id")
          for op in ops]
    _c, g = scan_both(engines, tmp_path, data, qs)
    for op, agg in zip(ops, g.aggregators):
        got = {p["fields"]["id"] for p in agg.points()}
        want = {str(i) for i, (_raw, lit) in enumerate(rows)
                if PY_OPS[op](float(lit), c)}
        assert got == want, (op, const, sorted(got ^ want))


# ---- dates (K3) ------------------------------------------------------

def date_lines(cases):
    return b"".join(
        ('{"id": "%d", "time": %s}\n' % (i, json.dumps(s))).encode()
        for i, (s, _ms) in enumerate(cases))


def test_date_table_is_self_consistent():
    """The independent truth agrees with a few hand-computed instants
    (runs without touching either engine)."""
    assert civil_ms(1970, 1, 1) == 0
    assert civil_ms(2014, 5, 1, 12, 34, 56, 789) == 1398947696789
    assert civil_ms(2000, 2, 29) == 951782400000
    assert civil_ms(1900, 2, 29) is None and civil_ms(2100, 2, 29) is None
    assert civil_ms(0, 1, 1) == -62167219200000
    assert civil_ms(2014, 5, 1, 24) == civil_ms(2014, 5, 2)


def test_date_parse_table(engines, tmp_path):
    cases = date_cases()
    assert len(cases) <= 4000
    c, g = scan_both(
        engines, tmp_path, date_lines(cases),
        q(breakdown_specs="id,ts[date,field=time,aggr=lquantize,step=1]"))
    assert dict(g.stages)["Datetime parser"] == \
        dict(c.stages)["Datetime parser"]
    nbad = sum(1 for _s, ms in cases if ms is None)
    assert dict(g.stages)["Datetime parser"]["baddate"] == nbad
    got = by_id(g.aggregators[0], "ts")
    bad = []
    for i, (s, ms) in enumerate(cases):
        want = None if ms is None else ms // 1000  # floor, also < 0
        if got.get(str(i)) != want:
            bad.append((s, got.get(str(i)), want))
    assert not bad, "%d wrong, first: %r" % (len(bad), bad[:10])


def iso(ms):
    d = EPOCH + datetime.timedelta(milliseconds=ms)
    return d.strftime("%Y-%m-%dT%H:%M:%S.") + "%03dZ" % (ms % 1000)


def test_time_bounds_at_the_instant(engines, tmp_path):
    """time_after / time_before exactly on, and 1 ms either side of, a
    record's instant.  Bounds are whole seconds after a ceil
    (ge ceil(after), lt ceil(before)); records carry floor(ms/1000)."""
    T = civil_ms(2014, 5, 1, 12, 34, 56)
    recs = [T + k * 500 for k in range(-4, 5)] + [T - 1, T + 1, T + 999]
    data = b"".join(('{"id": "%d", "time": "%s"}\n' % (i, iso(ms))).encode()
                    for i, ms in enumerate(recs))
    edges = [T - 1, T, T + 1]
    for a in edges:
        for b in [e for e in edges if e >= a] + [T + 1001]:
            _c, g = scan_both(
                engines, tmp_path, data,
                q(breakdown_specs="id", time_after=iso(a),
                  time_before=iso(b)),
                time_field="time")
            lo, hi = -(-a // 1000), -(-b // 1000)
            want = {str(i) for i, ms in enumerate(recs)
                    if lo <= ms // 1000 < hi}
            got = {p["fields"]["id"] for p in g.aggregators[0].points()}
            assert got == want, (iso(a), iso(b))

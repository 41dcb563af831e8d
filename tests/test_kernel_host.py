"""
The scan kernel's record semantics on the CPU (no GPU).

dragnet_amd/ops/hip/scan_text.h and scan_record.h are plain C++17 as
well as device code; tools_dev/kernel_host_check.cpp compiles them with
the host compiler and answers one request per line.  Every test here
is a differential between that program and an independent truth, and
holds for each byte source the kernels instantiate: Bytes and the
wave-transposed XBytesT<5|6|7> (the checker lays the record out exactly
as the host engine sizes it, so the sanitizer build at the end also
checks the "may read past end into the padding" contract).

The corpora are the GPU differentials' own (numeric_cases.py,
test_gpu_fuzz.py generators); those tests keep running on the device.
"""

import functools
import json
import os
import random
import shutil
import subprocess

import pytest

import numeric_cases as nc
import test_gpu_fuzz as fz

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCES = ["bytes", "x5", "x6", "x7"]
MASK64 = (1 << 64) - 1
SENTINEL_SIG = "%016x" % 1

source = pytest.mark.parametrize("src", SOURCES)


# ---- building and driving the checker --------------------------------

def _build(out_dir, name, flags):
    cxx = shutil.which("c++") or shutil.which("g++") or \
        shutil.which("clang++")
    assert cxx, "a host C++ compiler is part of the build contract"
    exe = str(out_dir / name)
    subprocess.run(
        [cxx, "-std=c++17"] + flags +
        ["-I", os.path.join(REPO, "dragnet_amd", "ops", "hip"),
         os.path.join(REPO, "tools_dev", "kernel_host_check.cpp"),
         "-o", exe], check=True)
    return exe


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("khc"), "kernel_host_check",
                  ["-O2"])


_answers = {}


def ask(exe, src, requests, key=None):
    """Answer lines for the request lines; a named corpus is run once
    per (program, byte source)."""
    if key is not None and (exe, src, key) in _answers:
        return _answers[(exe, src, key)]
    res = subprocess.run([exe, src], input="".join(
        r + "\n" for r in requests), capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-4000:]
    out = res.stdout.split("\n")[:-1]
    if key is not None:
        _answers[(exe, src, key)] = out
    return out


def hx(b):
    if isinstance(b, str):
        b = b.encode("utf-8")
    return b.hex() or "-"


# ---- numbers ---------------------------------------------------------

@functools.lru_cache(None)
def number_literals():
    lits = nc.special_literals() + sum(nc.literal_classes().values(), [])
    lits += [lit for _ln, lit in nc.geometry_records() if lit is not None]
    return list(dict.fromkeys(lits))


GRAMMAR_REJECTS = ["01", "1.", ".5", "-", "+1", "1e", "1e+", "0x10", "1_0"]


def number_requests():
    return ["number " + hx(lit)
            for lit in number_literals() + GRAMMAR_REJECTS]


@source
def test_json_numbers(checker, src):
    lits = number_literals()
    assert len(lits) > 8 * 400  # the classes, specials, digit-run shapes
    out = ask(checker, src, number_requests(), "number")
    assert len(out) == len(lits) + len(GRAMMAR_REJECTS)
    bad = []
    for lit, ans in zip(lits, out):
        status, bits, used = ans.split()
        x = float(lit)
        if nc.sig_digits(lit) <= 19:
            ok = bits == nc.double_to_bits(x)
        else:  # the one documented divergence: 19 digits are kept
            ok = nc.bits_to_double(bits) in nc.neighbours(x)
        if status != "ok" or int(used) != len(lit) or not ok:
            bad.append((lit, ans, nc.double_to_bits(x)))
    assert not bad, "%d wrong, first: %r" % (len(bad), bad[:10])
    for lit, ans in zip(GRAMMAR_REJECTS, out[len(lits):]):
        assert ans.split()[0] == "invalid", (lit, ans)


# ---- ToNumber --------------------------------------------------------

@functools.lru_cache(None)
def string_cases():
    return nc.string_cases()


def tonumber_requests():
    return ["tonumber " + hx(raw[1:-1]) for raw, _v in string_cases()]


@source
def test_to_number(checker, src):
    cases = string_cases()
    out = ask(checker, src, tonumber_requests(), "tonumber")
    assert len(out) == len(cases) >= 1000
    bad = []
    for (raw, want), bits in zip(cases, out):
        got = nc.bits_to_double(bits)
        if want != want:
            ok = got != got
        else:
            ok = bits == nc.double_to_bits(want)
        if not ok:
            bad.append((raw, got, want))
    assert not bad, "%d wrong, first: %r" % (len(bad), bad[:10])


# ---- dates -----------------------------------------------------------

@functools.lru_cache(None)
def date_cases():
    return nc.date_cases()


def date_requests():
    return ["date " + hx(json.dumps(s)[1:-1]) for s, _ms in date_cases()]


@source
def test_dates(checker, src):
    cases = date_cases()
    out = ask(checker, src, date_requests(), "date")
    assert len(out) == len(cases) >= 1600
    bad = [(s, ans, ms) for (s, ms), ans in zip(cases, out)
           if ans != ("invalid" if ms is None else "ok %d" % ms)]
    assert not bad, "%d wrong, first: %r" % (len(bad), bad[:10])


# ---- key signatures --------------------------------------------------

KEY_ALPHABET = [chr(c) for c in range(0x20, 0x7F) if chr(c) not in '"\\.']


@functools.lru_cache(None)
def key_paths():
    """Component lists: every length 0..40 alone and after an 8-byte
    component, then seeded random paths of 1-6 components."""
    rng = random.Random(4242)

    def comp(n):
        return "".join(rng.choice(KEY_ALPHABET) for _ in range(n))

    paths = [[comp(n)] for n in range(41)]
    paths += [[comp(8), comp(n)] for n in range(41)]
    for _ in range(400):
        paths.append([comp(rng.randrange(41))
                      for _ in range(rng.randrange(1, 7))])
    return paths


@source
def test_key_signatures(checker, src):
    from dragnet_amd.engine import plan
    paths = key_paths()
    seen = {len(c) for p in paths for c in p}
    assert seen == set(range(41))
    req = []
    for comps in paths:
        dotted = ".".join(comps)
        req.append("keysig 1 " + hx(dotted))  # skinner: dots split
        req.append("keysig 0 " + " ".join(hx(c) for c in comps))  # nested
        req.append("keysig 0 " + hx(dotted))  # json: one literal key
    out = ask(checker, src, req)
    assert len(out) == 3 * len(paths)
    for i, comps in enumerate(paths):
        dotted = ".".join(comps)
        want = "%016x" % plan.path_sig(dotted)
        assert out[3 * i] == want, (dotted, "dot_splits")
        assert out[3 * i + 1] == want, (dotted, "chained")
        assert out[3 * i + 2] == "%016x" % plan.lit_sig(dotted), dotted


# ---- records ---------------------------------------------------------

def plan_requests(cplan, dot_splits=0):
    """plan.compile_plan's arrays as the checker's text protocol."""
    nodes, bounds = cplan.programs
    return [
        "plan %d %d %016x %016x" % (
            dot_splits, len(cplan.field_sigs),
            cplan.sig_bloom & MASK64, cplan.fields_parent_sig & MASK64),
        "field_sigs " + " ".join("%016x" % int(s)
                                 for s in cplan.field_sigs),
        "prog_nodes " + " ".join(str(int(x)) for x in nodes.ravel()),
        "prog_bounds " + " ".join(str(int(x)) for x in bounds.ravel()),
        "const_meta " + " ".join(str(int(x))
                                 for x in cplan.const_meta.ravel()),
        "const_dvals " + " ".join(nc.double_to_bits(float(x))
                                  for x in cplan.const_dvals),
        "const_bytes " + hx(bytes(cplan.const_bytes)),
    ]


FIELDS = fz.KEYS + ["res.b"]  # KEYS already holds a.b and req.a


@functools.lru_cache(None)
def record_plan():
    """(queries, compiled plan): every fuzz key as a breakdown plus the
    filters of a few seeded rand_query draws."""
    from dragnet_amd.engine import plan
    from dragnet_amd.query import query_load
    qs = [query_load(breakdown_specs=",".join(FIELDS[:6])),
          query_load(breakdown_specs=",".join(FIELDS[6:]))]
    rng = random.Random(31)
    while sum(1 for q in qs if q.filter) < 8:
        q = fz.rand_query(rng)
        if q.filter:
            qs.append(q)
    cplan = plan.compile_plan(qs)
    assert {p for p, _raw in cplan.fields.paths} == set(FIELDS)
    return qs, cplan


@functools.lru_cache(None)
def record_lines():
    lines = []
    for seed in range(1000, 1004):
        rng = random.Random(seed)
        lines += [fz.rand_line(rng) for _ in range(2000)]
    return lines


def record_requests():
    return plan_requests(record_plan()[1]) + \
        ["record " + hx(ln) for ln in record_lines()]


TYPE_CODE = {type(None): 1, dict: 6, list: 7}  # common.h FieldType


def slot_matches(tok, want, line):
    """One captured slot against the oracle's value for its path."""
    from dragnet_amd import krill
    from dragnet_amd.scan_cpu import parse_json_line
    if want is krill.MISSING:
        return tok == "0"
    if want is None or isinstance(want, bool):
        return tok == {None: "1", False: "2", True: "3"}[want]
    if isinstance(want, (int, float)):
        return tok == "4:" + nc.double_to_bits(float(want))
    t, off, ln = (int(x) for x in tok.split(":"))
    span = line[off:off + ln]
    if isinstance(want, str):
        return t == 5 and json.loads(b'"' + span + b'"') == want
    return t == TYPE_CODE[type(want)] and \
        parse_json_line(span.decode("utf-8")) == want


def top_type_of(rec):
    if isinstance(rec, bool):
        return 3 if rec else 2
    if isinstance(rec, (int, float)):
        return 4
    return 5 if isinstance(rec, str) else TYPE_CODE[type(rec)]


@functools.lru_cache(None)
def record_truth():
    """Per line: None if the oracle rejects it, else (record, wanted
    value per physical slot, wanted result per program)."""
    from dragnet_amd import krill
    from dragnet_amd.scan_cpu import parse_json_line
    qs, cplan = record_plan()
    preds = [None] + [krill.create_predicate(q.filter) if q.filter
                      else None for q in qs]
    paths = [p for p, _raw in cplan.fields.paths]
    truth = []
    for line in record_lines():
        try:
            if not line:
                raise ValueError("empty line")
            rec = parse_json_line(line.decode("utf-8"))
        except ValueError:
            truth.append(None)
            continue
        slots = [krill.MISSING] * len(cplan.field_sigs)
        for i, p in enumerate(paths):
            slots[i] = krill.pluck(rec, p)  # nested path
            if cplan.comp_slot[i] >= 0:     # top-level literal "a.b" key
                slots[cplan.comp_slot[i]] = rec[p] if (
                    isinstance(rec, dict) and p in rec) else krill.MISSING
        results = []
        for pred in preds:
            try:
                results.append(1 if pred is None or pred.eval(rec) else 0)
            except Exception:  # the oracle's FilterStage: nfailedeval
                results.append(-1)
        truth.append((rec, slots, results))
    return truth


@source
def test_records(checker, src):
    lines, truth = record_lines(), record_truth()
    out = ask(checker, src, record_requests(), "record")
    assert len(out) == len(lines) == 8000
    nvalid = sum(1 for t in truth if t is not None)
    assert 5000 < nvalid < 7600  # both outcomes well represented
    compared = 0
    bad = []
    for line, want, ans in zip(lines, truth, out):
        compared += 1
        if want is None:
            if ans != "0":
                bad.append((line, "accepted"))
            continue
        rec, slots, results = want
        head, _, progs = ans.partition(" ;")
        toks = head.split()
        if toks[0] != "1":
            bad.append((line, "rejected"))
        elif int(toks[1]) != top_type_of(rec):
            bad.append((line, "top_type", toks[1]))
        elif not all(slot_matches(t, w, line)
                     for t, w in zip(toks[2:], slots)) or \
                len(toks) - 2 != len(slots):
            bad.append((line, "slots", toks[2:]))
        elif [int(x) for x in progs.split()] != results:
            bad.append((line, "programs", progs, results))
    assert not bad, "%d wrong, first: %r" % (len(bad), bad[:5])
    assert compared == len(lines)  # the envelope holds: nothing skipped


# ---- envelope pins (mirror test_gpu_envelope.py) ---------------------

def one_field_plan(name, dot_splits=0):
    from dragnet_amd.engine import plan
    from dragnet_amd.query import query_load
    fmt = "json-skinner" if dot_splits else "json"
    return plan_requests(plan.compile_plan(
        [query_load(breakdown_specs=name)], data_format=fmt), dot_splits)


@source
def test_depth_64_accepted_65_invalid(checker, src):
    def nested(depth, val):
        return ("{\"k\":" * depth) + json.dumps(val) + ("}" * depth)

    req = one_field_plan("a") + [
        "record " + hx(nested(63, {"a": "x"})),   # 64 levels with the leaf
        "record " + hx(nested(64, {"a": "x"})),
        "record " + hx("[" * 64 + "]" * 64),
        "record " + hx("[" * 65 + "]" * 65)]
    out = ask(checker, src, req)
    assert [o.split()[0] for o in out] == ["1", "0", "1", "0"]


@source
def test_escaped_key_is_the_sentinel_and_captures_nothing(checker, src):
    req = ["keysig 0 " + hx("\\u0061bc"), "keysig 1 " + hx("\\u0061bc"),
           "keysig 0 " + hx("abc")]
    req += one_field_plan("abc") + [
        "record " + hx('{"\\u0061bc": "v1"}'),
        "record " + hx('{"abc": "v2"}')]
    out = ask(checker, src, req)
    from dragnet_amd.engine import plan
    assert out[0] == out[1] == SENTINEL_SIG
    assert out[2] == "%016x" % plan.path_sig("abc")
    # valid object, slot "abc": missing / the 2-byte string at offset 9
    assert out[3].split(" ;")[0] == "1 6 0"
    assert out[4].split(" ;")[0] == "1 6 5:9:2"


@source
def test_raw_control_character_is_invalid(checker, src):
    req = one_field_plan("a") + [
        "record " + hx(b'{"a": "x\x01y"}'),
        "record " + hx(b'{"a": "x\ty"}'),
        "record " + hx(b'{"a\x1f": 1}'),
        "record " + hx(b'{"a": "x\\u0001y"}'),   # escaped: fine
        "keysig 0 " + hx(b"a\x01b")]
    out = ask(checker, src, req)
    assert [o.split()[0] for o in out] == ["0", "0", "0", "1", "invalid"]


# ---- the same corpora under AddressSanitizer + UBSan -----------------

SANITIZE = ["-O1", "-g", "-fsanitize=address,undefined",
            "-fno-sanitize-recover=all"]


@pytest.fixture(scope="module")
def checker_sanitized(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("khc_san"),
                  "kernel_host_check_san", SANITIZE)


@source
def test_sanitizer_build_agrees(checker, checker_sanitized, src):
    """A stand-alone program, run directly: exact-size buffers put the
    sanitizer's red zone right behind the padding the engine promises."""
    for key, make in (("record", record_requests),
                      ("number", number_requests),
                      ("tonumber", tonumber_requests),
                      ("date", date_requests)):
        req = make()
        plain = ask(checker, src, req, key)
        assert ask(checker_sanitized, src, req) == plain, key
        assert len(plain) > 1000

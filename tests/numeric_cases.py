"""
Shared helpers for the numeric-fidelity tests (test_numeric_cpu.py,
test_kernel_host.py on the CPU, test_gpu_numeric.py on the device): an
ECMAScript Number::toString written independently of
dragnet_amd.points, and the corpora with their truths — seeded number
literals, digit-run geometry, ToNumber strings and ISO-8601 dates.

Nothing here imports the package under test: the helpers are the
INDEPENDENT truth the engines are compared with.  The formatter itself
is pinned against V8 by tests/golden/numeric/js_number_tostring.json.
"""

import calendar
import datetime
import json
import math
import os
import random
import struct
from decimal import Decimal

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)),
                      "golden", "numeric", "js_number_tostring.json")


def load_golden():
    with open(GOLDEN) as f:
        return json.load(f)


def bits_to_double(h):
    return struct.unpack(">d", bytes.fromhex(h))[0]


def double_to_bits(x):
    return struct.pack(">d", x).hex()


def js_tostring(x):
    """ECMAScript Number::toString(x) for a Python float, built on
    Decimal(repr(x)): repr yields the shortest round-trip digits (the
    k, s of the spec), Decimal.as_tuple() hands them over with the
    exponent, and the spec's four layout rules do the rest."""
    if x != x:
        return "NaN"
    if x == 0:
        return "0"
    if x in (math.inf, -math.inf):
        return "Infinity" if x > 0 else "-Infinity"
    sign, digs, exp = Decimal(repr(abs(x))).as_tuple()
    s = "".join(map(str, digs)).lstrip("0")
    stripped = s.rstrip("0")
    exp += len(s) - len(stripped)
    s = stripped
    k = len(s)
    n = k + exp  # value = 0.s * 10^n  (spec: s * 10^(n-k))
    neg = "-" if x < 0 else ""
    if k <= n <= 21:
        return neg + s + "0" * (n - k)
    if 0 < n <= 21:
        return neg + s[:n] + "." + s[n:]
    if -6 < n <= 0:
        return neg + "0." + "0" * (-n) + s
    e = n - 1
    tail = ("e+" if e >= 0 else "e-") + str(abs(e))
    return neg + (s if k == 1 else s[0] + "." + s[1:]) + tail


def truth_key(lit):
    """The group key a JSON number literal must decode to: the JS
    string of its correctly rounded binary64 (Python float() is
    correctly rounded)."""
    return js_tostring(float(lit))


def sig_digits(lit):
    """Significant decimal digits in a literal's mantissa: leading and
    trailing zeros carry no information (dropping a trailing zero past
    the 19th digit loses nothing)."""
    m = lit.lstrip("+-").lower().partition("e")[0].replace(".", "")
    return len(m.strip("0"))


def neighbours(x):
    return {math.nextafter(x, -math.inf), x, math.nextafter(x, math.inf)}


# ---- literal classes (the issue's table), 400 each, seeded ----

def literal_classes(per_class=400, seed=20260):
    rng = random.Random(seed)
    cls = {}
    cls["repr_1e6"] = [repr(rng.uniform(-1e6, 1e6))
                       for _ in range(per_class)]
    cls["repr_unit"] = [repr(rng.uniform(0, 1)) for _ in range(per_class)]
    cls["d16_small_exp"] = [
        "%d.%de%d" % (rng.randrange(1, 10),
                      rng.randrange(10 ** 14, 10 ** 15),
                      rng.randrange(-5, 6))
        for _ in range(per_class)]
    cls["d15_exp30"] = [
        "%d.%de%d" % (rng.randrange(1, 10),
                      rng.randrange(10 ** 13, 10 ** 14),
                      rng.randrange(-30, 31))
        for _ in range(per_class)]
    cls["d6_bigexp"] = [
        "%d.%05de%s%d" % (rng.randrange(1, 10), rng.randrange(10 ** 5),
                          rng.choice("+-"), rng.randrange(23, 61))
        for _ in range(per_class)]
    cls["d3_exp22"] = [
        "%d.%02de%d" % (rng.randrange(1, 10), rng.randrange(100),
                        rng.randrange(-22, 23))
        for _ in range(per_class)]
    cls["leading_zero"] = [
        "0." + "0" * rng.randrange(1, 12)
        + str(rng.randrange(10 ** 14, 10 ** 15))
        for _ in range(per_class)]
    cls["d6_e308"] = [
        "%d.%05de308" % (1, rng.randrange(79770))
        for _ in range(per_class)]
    return cls


def tie_literals(seed=53):
    """Integers exactly half-way between two doubles, +-1 either side."""
    rng = random.Random(seed)
    ties = [2 ** 53 + 1]
    for bits_ in (56, 58, 60, 62, 63):  # 17..19 digits
        ulp = 1 << (bits_ - 52)
        base = rng.randrange(1 << (bits_ - 1), 1 << bits_) // ulp * ulp
        ties.append(base + ulp // 2)
    ties += [10 ** 16 + 1, 10 ** 17 + 8, 10 ** 18 + 64]
    out = []
    for t in ties:
        out += [str(t - 1), str(t), str(t + 1), "-" + str(t)]
    return out


SPECIALS = [
    "1e23", "8.5e-22", "8.84e-22", "5e-324", "4.9e-324",
    "2.4703282292062327e-324", "2.4703282292062328e-324",
    "2.2250738585072011e-308", "2.2250738585072014e-308",
    "1.7976931348623157e308", "1.7976931348623159e308",
    "1.7976931348623158e308", "1e400", "-1e400", "1e309", "1e-400",
    "-0", "-0.0", "0", "0.0", "0e999", "0.0e-999", "0E+5", "-0e999",
    "0.000000000000012345678", "0.0000000000000000001234",
    "1234567890123456789", "9223372036854775807",
    "9999999999999999999", "12345678901234567890",
    "18446744073709551615", "18446744073709551616",
    "99999999999999999999", "10000000000000000000",
    "1E5", "1e+5", "1.5E-7", "123456789012345680000", "1e21", "1e-7",
    "0.000001", "100", "1.0", "1.10", "120e-1",
] + ["0." + "0" * z + "1234" for z in range(26)]


def special_literals():
    return SPECIALS + tie_literals()


# ---- SWAR digit-run geometry ----

TERMS = [",", "}", " ", "e5", ".5"]


def geometry_records():
    """Digit runs of every length 1..24 as the integer part and as the
    fraction part, at every byte alignment 0..7 (a preceding string
    value pads the record), followed by each terminator; digits all
    '9' and '1' followed by zeros.  Returns [(line, literal|None)]:
    None where the text is not a JSON number (fraction run + '.5')."""
    recs = []
    k = 0
    for part in ("int", "frac"):
        for n in range(1, 25):
            for run in ("9" * n, "1" + "0" * (n - 1)):
                for align in range(8):
                    for term in TERMS:
                        lit = run if part == "int" else "3." + run
                        valid = True
                        if term in ("e5", ".5"):
                            lit += term
                            valid = not (part == "frac" and term == ".5")
                        if term == ",":
                            tail = ', "z": 1}'
                        elif term == " ":
                            tail = " }"
                        else:
                            tail = "}"
                        line = '{"id": "%d", "p": "%s", "n": %s%s' % (
                            k, "x" * align, lit, tail)
                        recs.append((line, lit if valid else None))
                        k += 1
    return recs


# ---- js_to_number strings ----

# (raw JSON text of the string value, Number(value) per ECMAScript)
_NAN = float("nan")
ESCAPED_SPELLINGS = [
    ('"\\t12"', 12.0), ('"12\\n"', 12.0), ('"\\u002012"', 12.0),
    ('"\\r\\n 12 \\t\\f"', 12.0), ('"\\u000b12\\u000C"', 12.0),
    ('"\\u00a012\\ufeff"', 12.0), ('"\\u2003 12\\u2028"', 12.0),
    ('"12\\\\t"', _NAN),       # 12 + backslash + t: no whitespace
    ('"12\\\\\\t"', _NAN),     # 12 + backslash + TAB: inner backslash
    ('"\\\\t12"', _NAN), ('"1\\t2"', _NAN), ('"\\u00412"', _NAN),
    ('"\\t"', 0.0), ('"\\u0020\\n"', 0.0), ('"12\\u001c"', _NAN),
    ('"12\\u0085"', _NAN), ('"\\b12"', _NAN),
]


def string_cases():
    """[(raw JSON string text, truth double)]: the V8-recorded table,
    the escaped-whitespace spellings, and the 17-digit / leading-zero
    literal classes spelled as strings — plain, and scaled by an
    exponent so the value is an integer beyond 2^53 where a
    step-1 lquantize shows every bit."""
    cases = []
    for s, want in load_golden()["tonumber"]:
        v = _NAN if want == "NaN" else bits_to_double(want)
        cases.append((json.dumps(s), v))
    cases += ESCAPED_SPELLINGS
    cls = literal_classes(per_class=150, seed=77)
    for lit in cls["repr_1e6"] + cls["repr_unit"] + cls["leading_zero"]:
        cases.append(('"%s"' % lit, float(lit)))
    for lit in cls["d16_small_exp"]:
        m = lit.partition("e")[0]
        for e in (17, 18):
            cases.append(('"%se%d"' % (m, e), float("%se%d" % (m, e))))
    for lit in cls["leading_zero"]:
        frac = lit[2:]
        s = "%se%d" % (lit, len(frac) + 3)
        cases.append(('" %s"' % s, float(s)))
    for t in tie_literals():
        cases.append(('"%s"' % t, float(t)))
    return cases


# ---- ISO-8601 dates ----

EPOCH = datetime.datetime(1970, 1, 1)


def civil_ms(y, mo, d, hh=0, mi=0, ss=0, ms=0, tz_min=0):
    """Epoch ms by datetime arithmetic, or None if a component is out
    of range (ES5 rules: hour 24 only as 24:00:00.000).  Year 0 does
    not exist in datetime: shift by one 400-year Gregorian cycle."""
    shift = 0
    if y < 1:
        y += 400
        shift = 146097
    if not (1 <= mo <= 12) or not (1 <= d <= calendar.monthrange(y, mo)[1]):
        return None
    if hh > 24 or mi > 59 or ss > 59 or (hh == 24 and (mi or ss or ms)):
        return None
    days = (datetime.datetime(y, mo, d) - EPOCH).days - shift
    return (((days * 24 + hh) * 60 + mi) * 60 + ss) * 1000 + ms \
        - tz_min * 60000


def date_cases():
    """[(string, epoch ms | None)]."""
    out = []
    for y in (1900, 2000, 2016, 2100):
        for mo in range(0, 14):
            last = calendar.monthrange(y, mo)[1] if 1 <= mo <= 12 else 31
            days = range(0, last + 2) if 1 <= mo <= 12 else (1, 15)
            for d in days:
                out.append(("%04d-%02d-%02dT06:07:08.009Z" % (y, mo, d),
                            civil_ms(y, mo, d, 6, 7, 8, 9)))
    base = (2014, 5, 1)
    for hh in (0, 23, 24, 25):
        for mi in (0, 59, 60):
            for ss in (0, 59, 60):
                out.append(("2014-05-01T%02d:%02d:%02dZ" % (hh, mi, ss),
                            civil_ms(*base, hh, mi, ss)))
    out.append(("2014-05-01T24:00:00.000Z", civil_ms(*base, 24)))
    out.append(("2014-05-01T24:00:00.001Z", None))
    out.append(("2014-12-31T24:00:00", civil_ms(2015, 1, 1)))
    digits = "7891234567"
    for n in range(0, 11):
        frac = digits[:n]
        want = civil_ms(*base, 12, 34, 56, int((frac + "000")[:3])) \
            if 1 <= n <= 9 else None
        out.append(("2014-05-01T12:34:56.%sZ" % frac, want))
    out.append(("2014-05-01T12:34:56.9999", civil_ms(*base, 12, 34, 56, 999)))
    t = civil_ms(*base, 12, 34, 56, 789)
    for zone, tzm in (("Z", 0), ("+05:30", 330), ("+0530", 330),
                      ("-00:00", 0), ("", 0), ("-08:00", -480),
                      ("+14:00", 840)):
        out.append(("2014-05-01T12:34:56.789" + zone, t - tzm * 60000))
        out.append(("2014-05-01T12:34" + zone,
                    civil_ms(*base, 12, 34) - tzm * 60000))
    out += [
        ("2014-05-01Z", None), ("2014-05-01+05:30", None),
        ("2014-05Z", None), ("2014Z", None),
        ("2014-05-01T12:34:56+5:30", None), ("2014-05-01T12:34:56+05", None),
        ("2014-05-01T12:34:56 Z", None),
        ("2014", civil_ms(2014, 1, 1)), ("2014-05", civil_ms(2014, 5, 1)),
        ("2014-05-01", civil_ms(*base)),
        ("2014-05-01 12:34:56", civil_ms(*base, 12, 34, 56)),
        ("2014-05-01T12:34:56", civil_ms(*base, 12, 34, 56)),
        ("2014-05-01t12:34:56Z", None), ("2014-05-01T12:34:56z", None),
        ("2014-05-01T12", None), ("2014-05-01T12:3", None),
        ("2014-5-01", None), ("14-05-01", None), ("20140501", None),
        ("2014-05-01T", None), ("", None), ("   ", None),
        (" 2014-05-01T12:34:56Z", civil_ms(*base, 12, 34, 56)),
        ("2014-05-01T12:34:56Z ", civil_ms(*base, 12, 34, 56)),
        ("\t2014-05-01T12:34:56Z\t", civil_ms(*base, 12, 34, 56)),
        (" \t 2014-05-01 \n", civil_ms(*base)),
        ("\\t2014-05-01", None),   # a literal backslash, not a tab
        ("2014-05-01\\", None),
        ("0000-01-01T00:00:00Z", civil_ms(0, 1, 1)),
        ("0000-02-29T00:00:00Z", civil_ms(0, 2, 29)),
        ("0000-12-31T23:59:59.999Z", civil_ms(0, 12, 31, 23, 59, 59, 999)),
        ("1969-12-31T23:59:59.500Z", -500),
        ("1969-12-31T23:59:59.999Z", -1), ("1969-12-31T23:59:59Z", -1000),
        ("1969-12-31T23:59:58.001Z", -1999),
        ("1969-07-20T20:17:40Z", civil_ms(1969, 7, 20, 20, 17, 40)),
        ("1970-01-01T00:00:00.000Z", 0), ("1970-01-01T00:00:00.999Z", 999),
        ("9999-12-31T23:59:59.999Z",
         civil_ms(9999, 12, 31, 23, 59, 59, 999)),
        ("1970-01-01T00:00:00+00:01", -60000),
    ]
    return out

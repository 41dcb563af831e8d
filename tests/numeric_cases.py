"""
Shared helpers for the numeric-fidelity tests (test_numeric_cpu.py,
test_gpu_numeric.py): an ECMAScript Number::toString written
independently of dragnet_amd.points, and the seeded literal corpora.

Nothing here imports the package under test: the helpers are the
INDEPENDENT truth the engines are compared with.  The formatter itself
is pinned against V8 by tests/golden/numeric/js_number_tostring.json.
"""

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

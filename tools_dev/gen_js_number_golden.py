#!/usr/bin/env python3
"""
Regenerate tests/golden/numeric/js_number_tostring.json by asking a
local `node` (V8) for ground truth:

  "tostring":  [[<16 hex digits of a binary64>, String(x)], ...]
  "tonumber":  [[<string s>, <16 hex digits of Number(s)> | "NaN"], ...]

The double list is seeded and covers integers up to and beyond 2^53,
both sides of the 1e21 and 1e-6/1e-7 notation switches, subnormals, the
largest double, negatives, -0 and 17-digit values.  ECMAScript
Number::toString and StringToNumber have not changed since ES1/ES5, so
any node version yields the same file.  Tests only READ the fixture.

    python tools_dev/gen_js_number_golden.py
"""

import json
import math
import os
import random
import struct
import subprocess

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..",
                   "tests", "golden", "numeric",
                   "js_number_tostring.json")

NODE_SRC = r"""
const inp = JSON.parse(require('fs').readFileSync(0, 'utf8'));
const ts = inp.bits.map(h => {
  const x = Buffer.from(h, 'hex').readDoubleBE(0);
  return [h, String(x)];
});
const tn = inp.strings.map(s => {
  const x = Number(s);
  if (x !== x) return [s, 'NaN'];
  const b = Buffer.alloc(8); b.writeDoubleBE(x, 0);
  return [s, b.toString('hex')];
});
process.stdout.write(JSON.stringify({tostring: ts, tonumber: tn}));
"""

# the ToNumber table of tests/test_gpu_numeric.py (string operands)
TONUMBER_STRINGS = [
    "26", " 26 ", "2.6e1", ".5", "5.", "+5", "-.5e1", "1e", "e5", ".",
    "", "   ",
    "0x1a", "0X1A", "0x", "-0x10", "+0x10", "0x10000000000000001",
    "0x1_0", "1_0", "0xffffffffffffffffffff", "0x20000000000001",
    "0x20000000000003", "0x8000000000000400", "0x8000000000000401",
    "0x8000000000000c00",
    "Infinity", "-Infinity", "+Infinity", "infinity", "1e400", "0e999",
    "-1e400", "007", "1e-400", "-0", "0.0",
    "\t12", "12\n", " 12",
    "9007199254740993", "0.1234567890123456", "123456.78901234567",
    "0.000000000000012345678", "0.0000000000000000001234",
    "1.7976931348623157e308", "1.7976931348623159e308", "5e-324",
    "2.4703282292062327e-324", "2.4703282292062328e-324",
    "12345678901234567890", "1e23", "8.5e-22", "nan", "NaN", "1e5x",
    "1 2", "--1", "1e+", "1e-", "1.e3", ".e3",
]


def bits(x):
    return struct.pack(">d", x).hex()


def doubles():
    rng = random.Random(20141)
    out = [0.0, -0.0, 1.0, -1.0, 0.5, 0.1, 0.3, 1e21, 1e-6, 1e-7,
           5e-324, 2.2250738585072014e-308, 2.225073858507201e-308,
           1.7976931348623157e308, 123456789012345680000.0, 1e16,
           0.00001, 1e22, 1e23, 1.5e-7, 1.5e-6, 123.456, 100.0,
           float(2 ** 53), float(2 ** 53 + 2), float(2 ** 63),
           float(2 ** 64), 4294967296.0, 0.000001234]
    for x in (1e21, 1e-6, 1e-7, float(2 ** 53), 1.0, 1e20):
        out += [math.nextafter(x, 0.0), math.nextafter(x, math.inf)]
    for _ in range(40):   # integers below 2^53
        out.append(float(rng.randrange(1, 2 ** 53)))
    for _ in range(40):   # integers beyond 2^53
        out.append(float(rng.randrange(2 ** 53, 2 ** 80)))
    for _ in range(40):   # around the 1e21 switch
        out.append(rng.uniform(1e19, 1e23))
    for _ in range(40):   # around the 1e-6 / 1e-7 switch
        out.append(10 ** rng.uniform(-9, -4))
    for _ in range(30):   # subnormals
        out.append(struct.unpack(
            ">d", struct.pack(">Q", rng.randrange(1, 1 << 52)))[0])
    for _ in range(60):   # 17-digit shortest forms
        out.append(rng.uniform(-1e6, 1e6))
    for _ in range(30):
        out.append(rng.uniform(0, 1))
    for _ in range(60):   # the whole exponent range, both signs
        v = struct.unpack(">d", struct.pack(
            ">Q", rng.randrange(1 << 52, 0x7FF << 52)))[0]
        out.append(v if rng.random() < 0.5 else -v)
    seen, uniq = set(), []
    for x in out:
        b = bits(x)
        if b not in seen:
            seen.add(b)
            uniq.append(b)
    return uniq


def main():
    inp = json.dumps({"bits": doubles(), "strings": TONUMBER_STRINGS})
    res = subprocess.run(["node", "-e", NODE_SRC], input=inp,
                         capture_output=True, text=True, check=True)
    data = json.loads(res.stdout)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        f.write('{"tostring": [\n')
        f.write(",\n".join(json.dumps(r) for r in data["tostring"]))
        f.write('\n],\n"tonumber": [\n')
        f.write(",\n".join(json.dumps(r) for r in data["tonumber"]))
        f.write("\n]}\n")
    print("%d doubles, %d strings -> %s"
          % (len(data["tostring"]), len(data["tonumber"]), OUT))


if __name__ == "__main__":
    main()

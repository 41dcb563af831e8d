"""The doubles the number-formatting tests print (test_dbl2dec_host.py on
the CPU, test_gpu_format_numbers.py on the device), by corpus name, as
lists of floats.  Truth is numeric_cases.js_tostring; the golden pairs
carry V8's own strings besides."""

import math
import random
import struct

from numeric_cases import (bits_to_double, literal_classes, load_golden,
                           neighbours, special_literals)


def golden_pairs():
    return [(bits_to_double(h), s) for h, s in load_golden()["tostring"]]


def corpora():
    rng = random.Random(1707)
    out = {"golden": [x for x, _s in golden_pairs()]}
    lits = special_literals() + [lit for c in literal_classes().values()
                                 for lit in c]
    out["literals"] = [float(lit) for lit in lits]
    # asymmetric intervals and subnormals: every power of two
    out["pow2"] = sorted(y for e in range(-1074, 1024)
                         for y in neighbours(math.ldexp(1.0, e)))
    # the layout switches at 1e21 and 1e-6 / 1e-7, 17-digit outputs
    out["pow10"] = sorted(y for e in range(-323, 309)
                          for y in neighbours(float("1e%d" % e)))
    out["edges"] = [2.0 ** 53 - 1, 2.0 ** 53, 2.0 ** 53 + 2,
                    1.7976931348623157e308, 5e-324, math.nan, math.inf,
                    -math.inf, 0.0, -0.0, -1.2345678901234567e-308,
                    -1.2345678901234567e-6]
    rand = []
    while len(rand) < 40000:  # 20000 patterns and their negations
        x = struct.unpack("<d", struct.pack("<Q", rng.getrandbits(64)))[0]
        if math.isfinite(x):
            rand += [x, -x]
    out["random"] = rand
    return out

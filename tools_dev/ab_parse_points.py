"""A/B of points.reduce_tagged_stream over synthetic tagged point streams:
the C++ reducer (DRAGNET_PARSE_GPU=0) against the parse_points path
(DRAGNET_PARSE_GPU=1), and the op alone with the text already on the
device.  Prints one line per cell; profiles/r16_parse_points.md.

    python tools_dev/ab_parse_points.py [lines ...]
"""
import io
import json
import os
import random
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dragnet_amd import merge  # noqa: E402
from dragnet_amd.ops import load_ops  # noqa: E402
from dragnet_amd.points import Aggregator, reduce_tagged_stream  # noqa: E402
from dragnet_amd.query import query_load  # noqa: E402

QUERIES = [query_load(breakdown_specs="req.method,res.statusCode,host"),
           query_load(breakdown_specs="lat[aggr=quantize],host")]


def stream(n, card, seed=5):
    rng = random.Random(seed)
    out = []
    for _ in range(n):
        h = "host-%06d" % rng.randrange(card)
        if rng.random() < 0.5:
            f = {"__dn_metric": 0, "req.method": rng.choice(["GET", "PUT"]),
                 "res.statusCode": rng.choice([200, 204, 404, 500]),
                 "host": h}
        else:
            f = {"__dn_metric": 1, "lat": rng.randrange(1, 4096), "host": h}
        out.append(json.dumps({"fields": f, "value": rng.randrange(1, 9)},
                              separators=(",", ":")))
    return ("\n".join(out) + "\n").encode()


def median_ms(fn, reps=7):
    fn()
    fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def whole(data, mode):
    os.environ["DRAGNET_PARSE_GPU"] = mode
    aggs = [Aggregator(q) for q in QUERIES]
    assert reduce_tagged_stream(io.BytesIO(data), aggs, QUERIES) == []
    return aggs


def main():
    ops = load_ops(required=True)
    specs = merge._parse_specs(QUERIES)
    for n in [int(a) for a in sys.argv[1:]] or [10000, 100000, 1000000]:
        for card in (10, n // 10):
            data = stream(n, max(card, 1))
            a, b = whole(data, "0"), whole(data, "1")
            assert all(x.table == y.table and x.ninputs == y.ninputs
                       for x, y in zip(a, b))
            text = merge._parse_upload(data, torch.device("cuda", 0))
            host = median_ms(lambda: whole(data, "0"))
            dev = median_ms(lambda: whole(data, "1"))
            op = median_ms(lambda: ops.parse_points(text, len(data), *specs))
            print("lines %8d  distinct hosts %7d  bytes %10d  host %9.2f ms  "
                  "device %9.2f ms  op alone %8.3f ms" %
                  (n, card, len(data), host, dev, op), flush=True)


if __name__ == "__main__":
    main()

"""A/B of the two ways to the JavaScript strings of f64 values
(dragnet_amd.merge.format_numbers), on one GPU:

    host      plan.number_key per value and _strings_blob, the result
              uploaded, which merge._encode_device needs on the device
    device    one ops.format_numbers call; nothing leaves the device

for n in {1e3, 1e4, 1e5, 1e6} numbers of three classes (two-decimal
latencies round(uniform(0, 1e4), 2); uniform(0, 1); random finite bit
patterns), with the input resident on the device (the host path pays the
D2H copy) and with the input in host memory (the device path pays the
upload).  Then the two design choices of ops/hip/format_numbers.h, the op
alone at the largest size on the last two classes: the decimal form parked
between the passes against converted twice, the power table where the
linker puts it against staged in LDS per block.  Then merge.encode_table
end to end on a snapshot whose plain column holds 1e5 and 1e6 distinct
fractional numbers, with DRAGNET_FORMAT_GPU at 0 and at 1.

    python tools_dev/ab_format_numbers.py [--reps 3] [--sizes 1000,...]
                                          [--out FILE]

The paths are alternated in one process; the device path is warmed up once
per shape; every timed region ends after a device synchronise.  Reports
median (min..max) in ms and prints markdown; the bytes of the two paths
are compared in every cell.
"""

import argparse
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from dragnet_amd import merge as D  # noqa: E402
from dragnet_amd.engine import decode  # noqa: E402
from dragnet_amd.engine import plan as P  # noqa: E402
from dragnet_amd.query import query_load  # noqa: E402

KINDS = ("latency .2f", "uniform(0,1)", "random bits")
VARIANTS = ((0, "parked, linker-placed table"), (1, "recomputed"),
            (2, "parked, LDS table"), (3, "recomputed, LDS table"))


def make_numbers(n, kind, seed):
    rng = np.random.default_rng(seed)
    if kind == "latency .2f":
        return np.round(rng.uniform(0, 1e4, n), 2)
    if kind == "uniform(0,1)":
        return rng.uniform(0, 1, n)
    bits = rng.integers(0, 1 << 63, 2 * n + 64, dtype=np.int64) \
        | (rng.integers(0, 2, 2 * n + 64, dtype=np.int64) << 63)
    x = bits.view(np.float64)
    return x[np.isfinite(x)][:n].copy()


def seam(mode, values):
    import torch
    os.environ["DRAGNET_FORMAT_GPU"] = mode
    blob, offs = D.format_numbers(values)
    return torch.as_tensor(blob).cuda(), torch.as_tensor(offs).cuda()


def make_snapshot(n, seed):
    """(query, extract_all-shaped dict): n rows of one plain column, row i
    keyed by number id i, the numbers n distinct three-decimal latencies
    in random order."""
    import torch
    x = np.round(np.arange(n) * 0.01 + 0.005, 3)
    np.random.default_rng(seed).shuffle(x)
    keys = np.zeros((n, 8), dtype=np.uint32)
    keys[:, 0] = (P.TAG_NUM << 30) | np.arange(n, dtype=np.uint32)

    def i32(a):
        return torch.from_numpy(
            np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).cuda()

    snap = {"cnt": torch.zeros(decode.C_GLOBAL_N + decode.CM_N,
                               dtype=torch.int64).cuda(),
            "aggs": [(i32(keys), torch.ones(n).double().cuda(), i32([n]))],
            "str_off": i32([0]), "str_len": i32([0]), "n_str": i32([0]),
            "blob": torch.zeros(16, dtype=torch.uint8).cuda(),
            "used": i32([0]), "numbers": torch.from_numpy(x).cuda(),
            "n_num": i32([n])}
    return query_load(breakdown_specs="c0"), snap


def encode(mode, q, snap):
    os.environ["DRAGNET_FORMAT_GPU"] = mode
    return D.encode_table(snap, q)


def timed(fn, *args):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn(*args)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def fmt(ts):
    ms = [t * 1e3 for t in ts]
    return "%.2f (%.2f..%.2f)" % (statistics.median(ms), min(ms), max(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--sizes", default="1000,10000,100000,1000000")
    ap.add_argument("--encode-sizes", default="100000,1000000")
    ap.add_argument("--out")
    args = ap.parse_args()

    import torch
    assert torch.cuda.is_available(), "this measurement needs a GPU"
    from dragnet_amd.ops import load_ops
    ops = load_ops(required=True)
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    sizes = [int(s) for s in args.sizes.split(",") if s]
    wins = {n: True for n in sizes}
    say("| numbers | n | input | text MB | host ms | device ms |")
    say("|---|---|---|---|---|---|")
    for kind in KINDS:
        for n in sizes:
            x = make_numbers(n, kind, seed=n % 997)
            for where, values in (("resident", torch.from_numpy(x).cuda()),
                                  ("uploaded", x)):
                _t, got = timed(seam, "1", values)  # warm-up
                th, td = [], []
                for _rep in range(args.reps):
                    t, want = timed(seam, "0", values)
                    th.append(t)
                    t, got = timed(seam, "1", values)
                    td.append(t)
                assert torch.equal(got[0], want[0]) and \
                    torch.equal(got[1], want[1]), "the two paths differ"
                if statistics.median(td) >= statistics.median(th):
                    wins[n] = False
                say("| %s | %d | %s | %.2f | %s | %s |" % (
                    kind, n, where, got[0].numel() / 1e6, fmt(th), fmt(td)))
    say()
    threshold = None
    for n in sorted(sizes, reverse=True):
        if not wins[n]:
            break
        threshold = n
    say("Smallest measured n from which the device median beats the host "
        "median for every class and both input places, and at every larger "
        "measured n: %s" % ("none" if threshold is None else threshold))
    say()
    say("| numbers | n | variant | op ms |")
    say("|---|---|---|---|")
    n = max(sizes)
    for kind in KINDS[1:]:
        x = torch.from_numpy(make_numbers(n, kind, seed=7)).cuda()
        want = ops.format_numbers(x, 0)
        ts = {v: [] for v, _name in VARIANTS}
        for v, _name in VARIANTS:  # warm-up
            assert torch.equal(ops.format_numbers(x, v)[0], want[0])
        for _rep in range(5 * args.reps):
            for v, _name in VARIANTS:
                ts[v].append(timed(ops.format_numbers, x, v)[0])
        for v, name in VARIANTS:
            say("| %s | %d | %s | %s |" % (kind, n, name, fmt(ts[v])))
    say()
    say("| distinct fractional numbers | FORMAT_GPU=0 ms | FORMAT_GPU=1 ms |")
    say("|---|---|---|")
    for n in [int(s) for s in args.encode_sizes.split(",") if s]:
        q, snap = make_snapshot(n, seed=n % 991)
        _t, got = timed(encode, "1", q, snap)  # warm-up
        th, td = [], []
        for _rep in range(args.reps):
            t, want = timed(encode, "0", q, snap)
            th.append(t)
            t, got = timed(encode, "1", q, snap)
            td.append(t)
        for a, b in zip((got.codes, got.tagpack, got.vals) + got.strings,
                        (want.codes, want.tagpack, want.vals) + want.strings):
            assert torch.equal(a, b), "the two wire tables differ"
        say("| %d | %s | %s |" % (n, fmt(th), fmt(td)))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

"""A/B of the two ways to split a rank's rows by destination rank
(dragnet_amd.merge.partition_rows), on one GPU:

    host     remap table D2H + numpy remap, hash, stable argsort, gather,
             then the upload of the send buffer   (DRAGNET_PARTITION_GPU=0)
    device   upload of what is on the host + the partition_rows kernels (=1)

for n in {1e5, 1e6, 8e6} rows, nk in {2, 8}, world 8, rows that spread
evenly over the ranks and rows that all go to one.  Column 0 is
string-tagged and goes through a remap table of 65536 entries; the other
codes are integers.  Each case is measured twice: with the input (codes,
tags, values, remap) starting on the device and starting on the host,
which is where _encode_table leaves it today.

    python tools_dev/ab_partition_rows.py [--reps 3] [--sizes 100000,...]
                                          [--out FILE]

The paths are alternated in one process.  Every timed region ends with
the send buffer and the counts on the device, after a device synchronise.
The device path is warmed up once per shape.  At 8e6 rows the host path
is timed twice at most.  Reports median (min..max) in ms and prints
markdown; the results are compared for equality in every cell.
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

WORLD = 8
REMAP = 1 << 16


def make_table(n, nk, skew, seed):
    rng = np.random.default_rng(seed)
    remap = rng.permutation(REMAP).astype(np.int64)
    if skew:  # one row, repeated: one destination
        codes = np.tile(rng.integers(0, REMAP, size=(1, nk)), (n, 1))
    else:
        codes = rng.integers(0, REMAP, size=(n, nk))
    tags = np.full(n, D._EL_STR, dtype=np.int64)
    vals = rng.integers(1, 1001, size=n).astype(np.float64)
    return codes.astype(np.int64), tags, vals, remap


def host_path(table):
    import torch
    wire, counts = D._partition_host(*table, WORLD)
    return (torch.from_numpy(wire.reshape(-1)).cuda(),
            torch.from_numpy(counts).cuda())


def device_path(table):
    wire, counts = D._partition_device(*table, WORLD, None)
    return wire.reshape(-1), counts


def timed(fn, table):
    import torch
    t0 = time.perf_counter()
    out = fn(table)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def fmt(ts):
    ms = [t * 1e3 for t in ts]
    return "%.1f (%.1f..%.1f)" % (statistics.median(ms), min(ms), max(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--sizes", default="100000,1000000,8000000")
    ap.add_argument("--out")
    args = ap.parse_args()

    import torch
    assert torch.cuda.is_available(), "this measurement needs a GPU"

    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say("| nk | rows | destinations | host ms, input on device | device ms, "
        "input on device | host ms, input on host | device ms, input on "
        "host |")
    say("|---|---|---|---|---|---|---|")
    sizes = [int(s) for s in args.sizes.split(",") if s]
    wins = {n: True for n in sizes}
    losses = []
    for nk in (2, 8):
        for n in sizes:
            for skew in (False, True):
                table_h = make_table(n, nk, skew, seed=n % 997 + nk)
                table_d = tuple(torch.from_numpy(a).cuda() for a in table_h)
                host_reps = min(args.reps, 2) if n > 2000000 else args.reps
                cols = []
                for where, table in (("device", table_d), ("host", table_h)):
                    _t, got = timed(device_path, table)  # warm-up
                    th, td = [], []
                    for rep in range(args.reps):
                        if rep < host_reps:
                            t, want = timed(host_path, table)
                            th.append(t)
                        t, got = timed(device_path, table)
                        td.append(t)
                    assert torch.equal(got[0], want[0])
                    assert torch.equal(got[1], want[1])
                    cols += [fmt(th), fmt(td)]
                    if statistics.median(td) >= statistics.median(th):
                        wins[n] = False
                        losses.append((nk, n, skew, where))
                say("| %d | %d | %s | %s |" % (
                    nk, n, "one" if skew else "all %d" % WORLD,
                    " | ".join(cols)))
                del table_d, got, want
    say()
    threshold = None
    for n in sorted(sizes, reverse=True):
        if not wins[n]:
            break
        threshold = n
    say("Smallest measured n from which the device path's median beats "
        "the host path's in both starting positions, at both widths and "
        "both spreads, and at every larger n: %s"
        % ("none" if threshold is None else threshold))
    say("Cells (nk, rows, one destination, input on) where the device "
        "path's median is not ahead: %s" % (losses or "none"))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

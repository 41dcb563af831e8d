"""A/B of the two ways to the rank of every dictionary string in byte order
(dragnet_amd.merge.rank_strings), on one GPU:

    host      merge._rank_host on the (blob, offs) pair resident on the
              device: the D2H copy of the dictionary, G bytes slices, the
              set, one sorted(); plus the upload of the ranks, which
              _render_device needs on the device: what runs today
    device    merge._rank_device: one ops.rank_strings call on the same
              pair; the ranks stay on the device

for G in {1e4, 1e5, 1e6} strings and four dictionaries: the three of
ab_render_points.py (8-byte ASCII, 64-byte ASCII, 20 non-ASCII characters)
and one with a long shared prefix (48 constant bytes, then 8 digits).

    python tools_dev/ab_rank_strings.py [--reps 3] [--sizes 10000,...]
                                        [--finish-max 0,8,...] [--out FILE]

The paths are alternated in one process; the device path is warmed up once
per shape; every timed region ends after a device synchronise.  Reports
median (min..max) in ms and prints markdown; the ranks of the two paths
are compared in every cell.  At the largest size the op is also timed with
each --finish-max value in place of RANK_FINISH_MAX (0: global rounds to
the end), for the choice of that constant.
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

KINDS = ("8-byte ASCII", "64-byte ASCII", "non-ASCII", "48-byte prefix")
GATED = KINDS[:3]


def make_strings(G, kind, seed):
    if kind == "non-ASCII":
        strings = ["".join("é€"[(i >> b) & 1] for b in range(20))
                   for i in range(G)]
    elif kind == "48-byte prefix":
        strings = ["p" * 48 + "%08d" % i for i in range(G)]
    else:
        pad = "x" * (0 if kind == "8-byte ASCII" else 56)
        strings = ["%08d" % i + pad for i in range(G)]
    perm = np.random.default_rng(seed).permutation(G)
    return [strings[i] for i in perm]


def host_path(pair):
    import torch
    rank = D._rank_host(pair)
    return torch.from_numpy(rank).to(pair[0].device)


def device_path(pair):
    return D._rank_device(pair, None)


def timed(fn, *args):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn(*args)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def fmt(ts):
    ms = [t * 1e3 for t in ts]
    return "%.1f (%.1f..%.1f)" % (statistics.median(ms), min(ms), max(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--sizes", default="10000,100000,1000000")
    ap.add_argument("--finish-max", default="0,8,64,512,4096")
    ap.add_argument("--out")
    args = ap.parse_args()

    import torch
    assert torch.cuda.is_available(), "this measurement needs a GPU"
    from dragnet_amd.ops import load_ops
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    ops = load_ops(required=True)
    cutoffs = [int(s) for s in args.finish_max.split(",") if s]
    sweep = []
    say("RANK_FINISH_MAX = %d" % ops.RANK_FINISH_MAX)
    say()
    say("| strings | G | blob MB | host ms | device ms |")
    say("|---|---|---|---|---|")
    sizes = [int(s) for s in args.sizes.split(",") if s]
    wins = {n: True for n in sizes}
    gate = []
    for kind in KINDS:
        for G in sizes:
            strings = make_strings(G, kind, seed=G % 997)
            blob, offs = D._strings_blob(strings)
            del strings
            pair = (torch.from_numpy(
                        np.frombuffer(blob, dtype=np.uint8).copy()).cuda(),
                    torch.from_numpy(offs).cuda())
            _t, got = timed(device_path, pair)  # warm-up
            th, td = [], []
            for _rep in range(args.reps):
                t, want = timed(host_path, pair)
                th.append(t)
                t, got = timed(device_path, pair)
                td.append(t)
            assert got is not None and torch.equal(got, want), \
                "device ranks differ from the host's"
            if kind in GATED:
                if statistics.median(td) >= statistics.median(th):
                    wins[G] = False
                if G == 1000000:
                    gate.append((kind, statistics.median(td) * 1e3,
                                 min(th) * 1e3))
            say("| %s | %d | %.1f | %s | %s |" % (
                kind, G, len(blob) / 1e6, fmt(th), fmt(td)))
            if G == max(sizes):  # the cutoff of the finish kernel
                for cut in cutoffs:
                    ops.rank_strings(*pair, finish_max=cut)  # warm-up
                    ts = [timed(ops.rank_strings, pair[0], pair[1], cut)
                          for _rep in range(args.reps)]
                    assert torch.equal(ts[-1][1][0], want)
                    sweep.append("| %s | %d | %d | %s |" % (
                        kind, G, cut, fmt([t for t, _out in ts])))
            del pair, got, want
    say()
    say("| strings | G | finish_max | device ms |")
    say("|---|---|---|---|")
    for row in sweep:
        say(row)
    say()
    threshold = None
    for G in sorted(sizes, reverse=True):
        if not wins[G]:
            break
        threshold = G
    say("Smallest measured G from which the device median beats the host "
        "median for each of the three gated dictionaries, and at every "
        "larger measured G: %s" % ("none" if threshold is None else threshold))
    for kind, dev, host_min in gate:
        say("Gate at 1e6, %s: device median %.1f ms, host minimum %.1f ms: "
            "%s" % (kind, dev, host_min,
                    "met" if dev < host_min else "MISSED"))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

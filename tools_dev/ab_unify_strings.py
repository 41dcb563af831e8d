"""A/B of the two ways to build the global string dictionary and the
per-rank remap tables (dragnet_amd.merge.unify_dictionaries), on
one GPU:

    host     blob D2H + _decode_strings + the dict loop (DRAGNET_UNIFY_GPU=0)
    device   unify_strings on the blobs + decode of the G firsts        (=1)

for n in {1e3, 1e4, 1e5, 1e6, 8e6} strings in 8 dictionaries of n / 8,
in three duplication patterns (all distinct; n / 8 distinct, each present
in every dictionary; 25 distinct) and two lengths (6..10 and 56..72
bytes, ASCII, a common prefix and the distinguishing characters last, as
in urls).  Each case is measured twice: with the blobs starting on the
device (the RCCL case: the host path pays the download) and starting on
the host (the gloo case: the device path pays the upload).

    python tools_dev/ab_unify_strings.py [--reps 3] [--sizes 1000,...]
                                         [--out FILE]

The paths are alternated in one process.  Every timed region ends with
gstrings in host memory and the remap tables where the next step takes
them (host arrays / device tensors), after a device synchronise.  The
device path is warmed up once per shape; the host path is Python alone.
At 8e6 strings the host path is timed twice at most.  Reports median
(min..max) in ms and prints markdown; the results are compared for
equality in every cell.
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
ALPHABET = np.frombuffer(
    b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789-_",
    dtype=np.uint8)


def make_dicts(n, pattern, lo, hi, seed):
    """WORLD (blob, offs) pairs of n / WORLD strings each.  String id k
    is lo + k % (hi - lo + 1) bytes: 'x' filler, then k in 4 characters."""
    rng = np.random.default_rng(seed)
    per = n // WORLD
    if pattern == "distinct":
        ids = rng.permutation(per * WORLD)
    elif pattern == "segments":
        ids = np.concatenate([rng.permutation(per) for _ in range(WORLD)])
    else:
        ids = rng.integers(0, 25, size=per * WORLD)
    length = lo + ids % (hi - lo + 1)
    end = np.cumsum(length)
    blob = np.full(int(end[-1]), ord("x"), dtype=np.uint8)
    for d in range(4):
        blob[end - 1 - d] = ALPHABET[(ids >> (6 * d)) & 63]
    dicts = []
    for r in range(WORLD):
        a, b = r * per, (r + 1) * per
        b0 = int(end[a - 1]) if a else 0
        offs = np.concatenate([[0], end[a:b] - b0]).astype(np.int64)
        dicts.append((blob[b0:int(end[b - 1])].copy(), offs))
    return dicts


def timed(fn, dicts):
    import torch
    t0 = time.perf_counter()
    out = fn(dicts)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def device_path(dicts):
    return D._unify_device(dicts, None)


def fmt(ts):
    ms = [t * 1e3 for t in ts]
    return "%.1f (%.1f..%.1f)" % (statistics.median(ms), min(ms), max(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--sizes", default="1000,10000,100000,1000000,8000000")
    ap.add_argument("--out")
    args = ap.parse_args()

    import torch
    assert torch.cuda.is_available(), "this measurement needs a GPU"

    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say("| bytes | strings | distinct | host ms, blobs on device | device "
        "ms, blobs on device | host ms, blobs on host | device ms, blobs "
        "on host |")
    say("|---|---|---|---|---|---|---|")
    sizes = [int(s) for s in args.sizes.split(",") if s]
    wins = {n: True for n in sizes}
    losses = []
    for lo, hi in ((6, 10), (56, 72)):
        for n in sizes:
            for pattern in ("distinct", "segments", "few"):
                dicts_h = make_dicts(n, pattern, lo, hi, seed=n % 997 + lo)
                dicts_d = [(torch.from_numpy(b).cuda(),
                            torch.from_numpy(o).cuda()) for b, o in dicts_h]
                host_reps = min(args.reps, 2) if n > 2000000 else args.reps
                cols = []
                for where, dicts in (("device", dicts_d), ("host", dicts_h)):
                    _t, got = timed(device_path, dicts)  # warm-up
                    th, td = [], []
                    for rep in range(args.reps):
                        if rep < host_reps:
                            t, want = timed(D._unify_host, dicts)
                            th.append(t)
                        t, got = timed(device_path, dicts)
                        td.append(t)
                    assert got[0] == want[0]
                    for g, w in zip(got[1], want[1]):
                        assert np.array_equal(g.cpu().numpy(), w)
                    cols += [fmt(th), fmt(td)]
                    if statistics.median(td) >= statistics.median(th):
                        wins[n] = False
                        losses.append((lo, n, pattern, where))
                say("| %d..%d | %d | %d | %s |" % (
                    lo, hi, n // WORLD * WORLD, len(want[0]),
                    " | ".join(cols)))
                del dicts_d, got, want
    say()
    threshold = None
    for n in sorted(sizes, reverse=True):
        if not wins[n]:
            break
        threshold = n
    say("Smallest measured n from which the device path's median beats "
        "the host path's in both starting positions, at every pattern and "
        "length measured, and at every larger n: %s"
        % ("none" if threshold is None else threshold))
    say("Cells (bytes from, strings, pattern, blobs on) where the device "
        "path's median is not ahead: %s" % (losses or "none"))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

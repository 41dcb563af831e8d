"""A/B of the ways to re-aggregate merged tables (the grouping step of
dragnet_amd.merge.reaggregate), on one GPU:

    host     np.unique(axis=0) + np.bincount      (DRAGNET_MERGE_GPU=0)
    parent   merge_rows(sort=False), the copy of the g distinct rows and
             np.lexsort on the host: the device path as it was before
             the sort kernels, written out below
    device   merge_rows(sort=True): grouped and ordered on the device,
             only sorted rows cross to the host                    (=1)

for n in {1e4, 1e5, 1e6, 8e6} rows of nk in {2, 8} key columns at low
(25 groups), medium (n/8) and all-distinct cardinality, integer weights
(so the device result is exact and is the one a merge would use).  Each
case is measured twice: with the rows starting on the device (the RCCL
case: the host path pays the download, the device path brings back only
the distinct rows) and starting on the host (the gloo case: the device
path pays the upload).

    python tools_dev/ab_merge_rows.py [--reps 3] [--sizes 10000,...]
                                      [--out FILE]

The paths are alternated in one process.  Every timed region ends
with the result in host memory, which follows a device synchronise.
The device paths are warmed up once per shape; the host path is numpy
alone.  At 8e6 rows the host path is timed twice at most (it takes many
seconds).  Reports median (min..max) in ms and prints markdown; all
three results are compared for equality in every case.  "passes" is the
number of 8-bit digits that vary over the distinct rows: the radix
passes the sort takes.
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


def make_rows(n, nk, groups, seed):
    """(codes [n, nk], tagpack [n], vals [n]) drawn from `groups`
    distinct key rows (groups == n: a permutation, all distinct)."""
    rng = np.random.default_rng(seed)
    pool = rng.integers(0, 1 << 40, size=(groups, nk), dtype=np.int64)
    pool[:, 0] = np.arange(groups)  # distinct for certain
    pick = rng.permutation(n) if groups == n else \
        rng.integers(0, groups, size=n)
    return (np.ascontiguousarray(pool[pick]), np.zeros(n, dtype=np.int64),
            rng.integers(1, 1001, size=n).astype(np.float64))


def timed(fn, part, nk):
    t0 = time.perf_counter()
    out = fn([part], None, nk)
    return time.perf_counter() - t0, out


def device_path(parts, remaps, nk):
    out = D._group_rows_device(parts, remaps, nk, None)
    assert out is not None, "integer weights must be exact"
    return out


def parent_device_path(parts, remaps, nk):
    """merge._group_rows_device before merge_rows had sort=."""
    import torch

    from dragnet_amd.ops import load_ops
    ops = load_ops(required=True)
    codes, tags, vals = parts[0]

    def up(a, dtype):
        return torch.as_tensor(a).to(device="cuda", dtype=dtype)

    rows = torch.cat([up(codes, torch.int64).reshape(-1, nk),
                      up(tags, torch.int64).reshape(-1, 1)], dim=1)
    uniq, sums, exact = ops.merge_rows(rows, up(vals, torch.float64), nk)
    assert exact, "integer weights must be exact"
    uniq = uniq.cpu().numpy()
    sums = sums.cpu().numpy()
    order = np.lexsort(uniq.T[::-1])
    return uniq[order], sums[order]


def passes(uniq):
    """Digits that vary over the rows: what sort_span_kernel finds."""
    diff = np.bitwise_or.reduce(uniq, axis=0) ^ \
        np.bitwise_and.reduce(uniq, axis=0)
    return sum(int(((int(d) >> (8 * b)) & 0xff) != 0)
               for d in diff.view(np.uint64) for b in range(8))


def fmt(ts):
    ms = [t * 1e3 for t in ts]
    return "%.1f (%.1f..%.1f)" % (statistics.median(ms), min(ms), max(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--sizes", default="10000,100000,1000000,8000000")
    ap.add_argument("--out")
    args = ap.parse_args()

    import torch
    assert torch.cuda.is_available(), "this measurement needs a GPU"

    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say("| nk | rows | groups | passes | host ms, rows on device | parent ms, "
        "rows on device | device ms, rows on device | host ms, rows on "
        "host | parent ms, rows on host | device ms, rows on host |")
    say("|---|---|---|---|---|---|---|---|---|---|")
    sizes = [int(s) for s in args.sizes.split(",") if s]
    wins = {n: True for n in sizes}
    behind_parent = []
    for nk in (2, 8):
        for n in sizes:
            for groups in (25, max(n // 8, 1), n):
                part_h = make_rows(n, nk, groups, seed=nk * 1000 + groups % 997)
                part_d = tuple(torch.from_numpy(a).cuda() for a in part_h)
                host_reps = min(args.reps, 2) if n > 2000000 else args.reps
                cols = []
                for part in (part_d, part_h):
                    _t, got = timed(device_path, part, nk)  # warm-up
                    _t, old = timed(parent_device_path, part, nk)
                    th, tp, td = [], [], []
                    for rep in range(args.reps):
                        if rep < host_reps:
                            t, want = timed(D._group_rows_host, part, nk)
                            th.append(t)
                        t, old = timed(parent_device_path, part, nk)
                        tp.append(t)
                        t, got = timed(device_path, part, nk)
                        td.append(t)
                    for other in (got, old):
                        assert np.array_equal(other[0], want[0])
                        assert np.array_equal(other[1], want[1])
                    cols += [fmt(th), fmt(tp), fmt(td)]
                    if statistics.median(td) >= statistics.median(th):
                        wins[n] = False
                    if statistics.median(td) >= statistics.median(tp):
                        behind_parent.append((nk, n, want[0].shape[0]))
                say("| %d | %d | %d | %d | %s |" % (
                    nk, n, want[0].shape[0], passes(want[0]),
                    " | ".join(cols)))
                del part_d
    say()
    threshold = None
    for n in sorted(sizes, reverse=True):
        if not wins[n]:
            break
        threshold = n
    say("Smallest measured n from which the device path's median beats "
        "the host path's in both starting positions, at every "
        "cardinality and nk measured, and at every larger n: %s"
        % ("none" if threshold is None else threshold))
    say("Cases (nk, rows, groups; either starting position) where the "
        "device path's median is not ahead of the parent's device path: "
        "%s" % (sorted(set(behind_parent)) or "none"))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

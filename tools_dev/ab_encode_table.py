"""A/B of the two ways from a scan's extraction snapshot on the device to
the wire form of one table on the device (dragnet_amd.merge.encode_table),
on one GPU:

    host     D2H of the snapshot + decode.decode_snapshot + _encode_table
             + _strings_blob + the upload of the five arrays
    device   the encode_table kernels on the snapshot where it lies, and
             the host rendering of the exceptions   (DRAGNET_ENCODE_GPU=1)

for n in {1e4, 1e5, 1e6, 8e6} rows, nk in {1, 8}, and three tables:
all-string (plain columns, ids into a dictionary of min(n, 65536)
strings of 12..28 bytes), all-ordinal (bucketized columns) and the
all-string table with 1 % of its dictionary strings escaped.  The
snapshots are synthetic: no scan runs.

    python tools_dev/ab_encode_table.py [--reps 3] [--sizes 10000,...]
                                        [--host-max ROWS] [--out FILE]

The paths are alternated in one process.  Every timed region ends with
the wire table on the device, after a device synchronise.  The device
path is warmed up once per shape.  The host path is per-row Python: it is
timed once from 1e6 rows and not at all beyond --host-max rows (the cell
then says so).  Reports median (min..max) in ms and prints markdown; up
to 1e5 rows the two tables are put through reaggregate and compared.
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

KINDS = ("all-string", "all-ordinal", "1 % exceptions")


def make_snapshot(n, nk, kind, seed):
    """(query, extract_all-shaped dict of device tensors)."""
    import torch
    rng = np.random.default_rng(seed)
    n_str = min(n, 1 << 16)
    keys = np.zeros((n, 8), dtype=np.uint32)
    if kind == "all-ordinal":
        spec = ",".join("c%d[aggr=lquantize,step=10]" % j for j in range(nk))
        keys[:, :nk] = (P.TAG_ORD << 30) | rng.integers(
            0, 1 << 20, size=(n, nk)).astype(np.uint32)
    else:
        spec = ",".join("c%d" % j for j in range(nk))
        keys[:, :nk] = (P.TAG_STR << 30) | rng.integers(
            0, n_str, size=(n, nk)).astype(np.uint32)
    strings = []
    for i in range(n_str):
        s = b"%08d" % i + b"x" * int(rng.integers(4, 21))
        if kind == "1 % exceptions" and i % 100 == 0:
            s = s[:6] + b"\\u0041" + s[12:]
        strings.append(s)
    lens = np.array([len(s) for s in strings], dtype=np.uint32)
    off = (np.cumsum(lens) - lens).astype(np.uint32)
    blob = np.frombuffer(b"".join(strings), dtype=np.uint8).copy()

    def i32(a):
        return torch.from_numpy(
            np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).cuda()

    snap = {"cnt": torch.zeros(decode.C_GLOBAL_N + decode.CM_N,
                               dtype=torch.int64).cuda(),
            "aggs": [(i32(keys), torch.from_numpy(rng.integers(
                1, 1001, size=n).astype(np.float64)).cuda(), i32([n]))],
            "str_off": i32(off), "str_len": i32(lens), "n_str": i32([n_str]),
            "blob": torch.from_numpy(blob).cuda(),
            "used": i32([blob.size]), "numbers": torch.zeros(1).double().cuda(),
            "n_num": i32([0])}
    return query_load(breakdown_specs=spec), snap


def host_path(q, snap, cplan):
    """What the sharded datasource does today, from the same snapshot."""
    import torch
    k, c, n = snap["aggs"][0]
    n = int(n.item())
    n_str = int(snap["n_str"].item())
    used = int(snap["used"].item())
    host = {"cnt": snap["cnt"].cpu().numpy(), "n_str": n_str, "n_num": 0,
            "str_off": snap["str_off"][:n_str].cpu().numpy(),
            "str_len": snap["str_len"][:n_str].cpu().numpy(),
            "blob": snap["blob"][:used].cpu().numpy(),
            "aggs": [(k[:n].cpu().numpy(), c[:n].cpu().numpy())]}
    agg = decode.decode_snapshot(host, [q], cplan)[0][0]
    w = D.encode_table(agg, q)
    up = [torch.from_numpy(np.ascontiguousarray(a)).cuda()
          for a in (w.codes, w.tagpack, w.vals) + w.strings]
    return D.WireTable(up[0], up[1], up[2], (up[3], up[4]))


def device_path(q, snap, cplan):
    return D.encode_table(snap, q)


def timed(fn, *args):
    import torch
    t0 = time.perf_counter()
    out = fn(*args)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def fmt(ts):
    if not ts:
        return "not run"
    ms = [t * 1e3 for t in ts]
    return "%.1f (%.1f..%.1f)" % (statistics.median(ms), min(ms), max(ms))


def table_of(q, w):
    return D.reaggregate(q, [(w.codes, w.tagpack, w.vals)], [w.strings]).table


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--sizes", default="10000,100000,1000000,8000000")
    ap.add_argument("--host-max", type=int, default=8000000)
    ap.add_argument("--out")
    args = ap.parse_args()

    import torch
    assert torch.cuda.is_available(), "this measurement needs a GPU"
    os.environ["DRAGNET_MERGE_GPU"] = os.environ["DRAGNET_UNIFY_GPU"] = "0"

    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say("| table | nk | rows | host ms | device ms |")
    say("|---|---|---|---|---|")
    sizes = [int(s) for s in args.sizes.split(",") if s]
    wins = {n: True for n in sizes}
    losses, unmeasured = [], []
    for kind in KINDS:
        for nk in (1, 8):
            for n in sizes:
                q, snap = make_snapshot(n, nk, kind, seed=n % 997 + nk)
                cplan = P.compile_plan([q])
                host_reps = 0 if n > args.host_max else \
                    1 if n >= 1000000 else args.reps
                _t, got = timed(device_path, q, snap, cplan)  # warm-up
                th, td = [], []
                for rep in range(args.reps):
                    if rep < host_reps:
                        t, want = timed(host_path, q, snap, cplan)
                        th.append(t)
                    t, got = timed(device_path, q, snap, cplan)
                    td.append(t)
                if th and n <= 100000:
                    assert table_of(q, got) == table_of(q, want)
                if not th:
                    unmeasured.append((kind, nk, n))
                elif statistics.median(td) >= statistics.median(th):
                    wins[n] = False
                    losses.append((kind, nk, n))
                say("| %s | %d | %d | %s | %s |" % (kind, nk, n, fmt(th),
                                                    fmt(td)))
                del snap, got
    say()
    threshold = None
    for n in sorted(sizes, reverse=True):
        if not wins[n]:
            break
        if not any(u[2] == n for u in unmeasured):
            threshold = n
    say("Smallest measured n from which the device path's median beats the "
        "host path's for every table and both widths, and at every larger "
        "measured n: %s" % ("none" if threshold is None else threshold))
    say("Cells (table, nk, rows) where the device path's median is not "
        "ahead: %s" % (losses or "none"))
    say("Cells whose host path was not run: %s" % (unmeasured or "none"))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

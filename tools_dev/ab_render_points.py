"""A/B of the two ways from a merged table (distinct rows, sums, global
dictionary) to the NDJSON point lines `dn scan --points` prints
(dragnet_amd.merge.render_points), on one GPU:

    host      merge._decode_rows + Aggregator.points() + output.output_points
              through the native serializer: what runs today
    device    merge._render_device: string ranks on the host, the rank
              gather, sort_rows and the render_points kernels, the text
              copied to the host; with the rows, sums and dictionary
              resident on the device, and with them on the host (uploads
              inside the timed region)

for g in {1e4, 1e5, 1e6} distinct rows, nk in {1, 8} string columns, and
three dictionaries: 8-byte ASCII strings, 64-byte ASCII strings and
strings of 20 non-ASCII characters (2- and 3-byte sequences).  With nk = 1
the dictionary has g strings; with nk = 8 it has min(g, 65536).

    python tools_dev/ab_render_points.py [--reps 3] [--sizes 10000,...]
                                         [--host-max ROWS] [--out FILE]

The paths are alternated in one process.  Every timed region ends with
the bytes on the host, after a device synchronise.  The device paths are
warmed up once per shape.  The host path is per-row Python: it is timed
once from 1e6 rows and not at all beyond --host-max rows.  Reports median
(min..max) in ms and prints markdown; wherever the host path ran, its
bytes and the device's are compared.
"""

import argparse
import io
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from dragnet_amd import merge as D  # noqa: E402
from dragnet_amd import output  # noqa: E402
from dragnet_amd.query import query_load  # noqa: E402

KINDS = ("8-byte ASCII", "64-byte ASCII", "non-ASCII")


def make_table(g, nk, kind, seed):
    """(query, uniq [g, nk + 1], sums [g], strings list of str)."""
    rng = np.random.default_rng(seed)
    n_str = g if nk == 1 else min(g, 1 << 16)
    if kind == "non-ASCII":
        strings = ["".join("é€"[(i >> b) & 1] for b in range(20))
                   for i in range(n_str)]
    else:
        pad = "x" * (0 if kind == "8-byte ASCII" else 56)
        strings = ["%08d" % i + pad for i in range(n_str)]
    perm = rng.permutation(n_str)  # codes in no string order
    strings = [strings[i] for i in perm]
    codes = rng.integers(0, n_str, size=(g, nk))
    codes[:, 0] = np.arange(g) % n_str
    if nk > 1:
        codes[:, 1] = np.arange(g) // n_str  # (col 0, col 1): distinct
    tp = sum(D._EL_STR << (2 * j) for j in range(nk))
    uniq = np.concatenate(
        [codes, np.full((g, 1), tp)], axis=1).astype(np.int64)
    sums = rng.integers(1, 100001, size=g).astype(np.float64)
    spec = ",".join("c%d" % j for j in range(nk))
    return query_load(breakdown_specs=spec), uniq, sums, strings


def host_path(q, uniq, sums, strings):
    out = io.TextIOWrapper(io.BytesIO())
    output.output_points(D._decode_rows(q, uniq, sums, strings).points(), out)
    out.flush()
    return out.buffer.getvalue()


def device_path(q, uniq, sums, strings):
    got = D._render_device(q, uniq, sums, strings, None)
    assert got is not None, "the device path refused the table"
    return got


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--sizes", default="10000,100000,1000000")
    ap.add_argument("--host-max", type=int, default=1000000)
    ap.add_argument("--out")
    args = ap.parse_args()

    import torch
    assert torch.cuda.is_available(), "this measurement needs a GPU"
    os.environ.pop("DRAGNET_PY_POINTS", None)  # the native serializer

    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    say("| strings | nk | rows | text MB | host ms | device ms, resident | "
        "device ms, input on the host |")
    say("|---|---|---|---|---|---|---|")
    sizes = [int(s) for s in args.sizes.split(",") if s]
    wins = {n: True for n in sizes}
    losses, unmeasured = [], []
    for kind in KINDS:
        for nk in (1, 8):
            for g in sizes:
                q, uniq, sums, strings = make_table(g, nk, kind,
                                                    seed=g % 997 + nk)
                blob, offs = D._strings_blob(strings)
                blob = np.frombuffer(blob, dtype=np.uint8).copy()
                on_host = (uniq, sums, (blob, offs))
                resident = (torch.from_numpy(uniq).cuda(),
                            torch.from_numpy(sums).cuda(),
                            (torch.from_numpy(blob).cuda(),
                             torch.from_numpy(offs).cuda()))
                host_reps = 0 if g > args.host_max else \
                    1 if g >= 1000000 else args.reps
                _t, got = timed(device_path, q, *resident)  # warm-up
                th, tr, tu = [], [], []
                for rep in range(args.reps):
                    if rep < host_reps:
                        t, want = timed(host_path, q, uniq, sums, strings)
                        th.append(t)
                    t, got = timed(device_path, q, *resident)
                    tr.append(t)
                    t, got_up = timed(device_path, q, *on_host)
                    tu.append(t)
                assert got == got_up
                if th:
                    assert got == want, "device bytes differ from the host's"
                else:
                    unmeasured.append((kind, nk, g))
                if th and max(statistics.median(tr), statistics.median(tu)) \
                        >= statistics.median(th):
                    wins[g] = False
                    losses.append((kind, nk, g))
                say("| %s | %d | %d | %.1f | %s | %s | %s |" % (
                    kind, nk, g, len(got) / 1e6, fmt(th), fmt(tr), fmt(tu)))
                del resident, got, got_up
    say()
    threshold = None
    for g in sorted(sizes, reverse=True):
        if not wins[g]:
            break
        if not any(u[2] == g for u in unmeasured):
            threshold = g
    say("Smallest measured g from which both device medians beat the host "
        "path's for every dictionary and both widths, and at every larger "
        "measured g: %s" % ("none" if threshold is None else threshold))
    say("Cells (strings, nk, rows) where a device median is not ahead: %s"
        % (losses or "none"))
    say("Cells whose host path was not run: %s" % (unmeasured or "none"))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

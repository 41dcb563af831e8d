"""
Measurements for in-place table growth (profiles/r06_grow_in_place.md).

    python tools_dev/diag_grow.py rehash
        cost of one growth: a populated 2^20-slot aggregation table,
        string dictionary and number dictionary rehashed to 2^22, and a
        256 MB payload buffer moved to 1 GB; HIP events around the
        binding call (needs this tree's extension)

    python tools_dev/diag_grow.py bytesource [--mb 1024] [--runs 5]
        wall time of a byte_source= scan of a bench pool at default
        table sizes, flagship filter + two-field breakdown.  Uses only
        GpuEngine.scan, so DN_TREE=<checkout of another commit> times
        that commit with the same script.

    python tools_dev/diag_grow.py restart [--mb 2048] [--runs 3]
        a regular-file scan that overflows its (tiny) tables: restart
        (default) against DRAGNET_GROW=1

Each prints one JSON line.
"""

import argparse
import json
import os
import statistics
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
TREE = os.environ.get("DN_TREE") or os.path.dirname(HERE)
sys.path.insert(0, TREE)


def spread(xs):
    return {"median": round(statistics.median(xs), 4),
            "min": round(min(xs), 4), "max": round(max(xs), 4),
            "runs": [round(x, 4) for x in xs]}


def flagship():
    from dragnet_amd.query import query_load
    return query_load(filter={"eq": ["req.method", "GET"]},
                      breakdown_specs="req.method,res.statusCode")


def pool(mb):
    import bench  # the tree's bench.py: seeded mktestdata-shaped pool
    buf, nrec = bench.build_pool(mb, seed=1000, workers=min(
        16, len(os.sched_getaffinity(0))))
    return bytes(buf), nrec


def cmd_rehash(_args):
    blob = b"".join(b'{"k":"key-%07d","n":%d}\n' % (i, 7 * i + 3)
                    for i in range(600_000))
    import torch
    from dragnet_amd.engine import plan as planmod
    from dragnet_amd.engine.gpu import GpuEngine, _ScanContext
    from dragnet_amd.query import query_load
    os.environ["DRAGNET_GROW_MIN_RECORDS"] = "65536"
    eng = GpuEngine()
    qs = [query_load(breakdown_specs="k,n")]
    out = {"what": "rehash", "entries": 600_000}
    times = {}
    for rep in range(3):
        ctx = _ScanContext(eng, planmod.compile_plan(qs), 1 << 20, 1 << 20,
                           256 << 20, growable=True)
        # populate in one unplanned launch (57% load), so that every
        # structure still has its first size when it is timed
        planner, ctx.planner = ctx.planner, None
        ctx.feed(blob)
        ctx.planner = planner
        occ = ctx.state.occupancy().cpu().tolist()
        assert not ctx.overflowed(), occ
        assert occ[0] == occ[1] == occ[3] == 600_000, occ
        for name, new in (("agg0", 1 << 22), ("sdict", 1 << 22),
                          ("ndict", 1 << 22), ("sdata", 1 << 30)):
            torch.cuda.synchronize()
            e0 = torch.cuda.Event(enable_timing=True)
            e1 = torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            ctx.grow(name, new)  # allocation + zeroing + rehash
            e1.record()
            torch.cuda.synchronize()
            times.setdefault(name, []).append(
                (e0.elapsed_time(e1), (time.perf_counter() - t0) * 1e3))
        assert ctx.state.occupancy().cpu().tolist() == occ
        assert not ctx.overflowed()
        del ctx
    for name, ts in times.items():
        out[name + "_ms_events"] = spread([t[0] for t in ts])
        out[name + "_ms_wall"] = spread([t[1] for t in ts])
    print(json.dumps(out))


def cmd_bytesource(args):
    buf, nrec = pool(args.mb)
    from dragnet_amd.engine.gpu import GpuEngine
    eng = GpuEngine()
    qs = [flagship()]
    step = 8 << 20

    def source():
        for at in range(0, len(buf), step):
            yield buf[at:at + step]

    eng.scan([], qs, byte_source=source())  # warm-up
    secs = []
    stats = None
    for _ in range(args.runs):
        t0 = time.perf_counter()
        res = eng.scan([], qs, byte_source=source())
        secs.append(time.perf_counter() - t0)
        stats = getattr(res, "gpu_stats", None)
    print(json.dumps({"what": "bytesource", "tree": TREE, "mb": args.mb,
                      "records": nrec, "seconds": spread(secs),
                      "gb_per_s": round(len(buf) / 1e9 /
                                        statistics.median(secs), 3),
                      "gpu_stats": stats}))


def cmd_restart(args):
    buf, nrec = pool(args.mb)
    from dragnet_amd.engine.gpu import GpuEngine
    from dragnet_amd.query import query_load
    os.environ.update(DRAGNET_AGG_SLOTS="128", DRAGNET_DICT_SLOTS="128",
                      DRAGNET_DICT_DATA_MB="1")
    qs = [query_load(breakdown_specs="req.url")]
    out = {"what": "restart-vs-grow", "mb": args.mb, "records": nrec}
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "corpus.ndjson")
        with open(path, "wb") as f:
            f.write(buf)
        del buf
        points = None
        for mode in ("restart", "grow"):
            os.environ["DRAGNET_GROW"] = "1" if mode == "grow" else "0"
            eng = GpuEngine()
            eng.scan([path], qs)  # warm-up (page cache, pinned buffers)
            secs = []
            for _ in range(args.runs):
                t0 = time.perf_counter()
                res = eng.scan([path], qs)
                secs.append(time.perf_counter() - t0)
            out[mode] = {"seconds": spread(secs),
                         "gpu_stats": res.gpu_stats}
            pts = res.aggregators[0].points()
            assert points is None or pts == points
            points = pts
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["rehash", "bytesource", "restart"])
    ap.add_argument("--mb", type=int, default=None)
    ap.add_argument("--runs", type=int, default=None)
    args = ap.parse_args()
    if args.mb is None:
        args.mb = 2048 if args.what == "restart" else 1024
    if args.runs is None:
        args.runs = 3 if args.what == "restart" else 5
    {"rehash": cmd_rehash, "bytesource": cmd_bytesource,
     "restart": cmd_restart}[args.what](args)


if __name__ == "__main__":
    main()

"""A/B of the three ways to answer an index query on the GPU engine:

    sqlite    per-file SQLite WHERE + GROUP BY      (DRAGNET_INDEX_GPU=0)
    k7        per-file extract + columnar_query     (=1, no sidecars)
    sidecar   merged columnar sidecars, one launch  (=1, sidecars)

over a dense muskie-style metric (host x method x operation x status x
caller x latency bucket) of 50k, 500k and 2M rows in one index file,
and the 2M rows as a 24-file hourly tree; query = eq filter + 2-field
breakdown, the one of profiles/r02_k7.md.

    python tools_dev/ab_columnar_index.py [--reps 5] [--sizes 50000,...]
           [--cli-reps 3] [--out FILE]
    python tools_dev/ab_columnar_index.py --kernels-only DIR
        (builds nothing: runs the sidecar path over a tree that a
         previous run left in DIR; for a kernel-trace profiler run)

The three are alternated in one process, warm; each timed region ends
with the result on the host, which follows a device synchronise.
Reports median and spread (min..max) in ms, the sidecar path's split
(read headers / load + merge / H2D / kernels / decode), `dn query` wall
time per path, sidecar vs .sqlite bytes and the cost of writing the
sidecars.  Prints markdown.
"""

import argparse
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from dragnet_amd.index import IndexSink  # noqa: E402
from dragnet_amd.index import columnar  # noqa: E402

METRIC = {"name": "requests", "filter": None, "breakdowns": [
    {"name": "host", "field": "host"},
    {"name": "req.method", "field": "req.method"},
    {"name": "operation", "field": "operation"},
    {"name": "res.statusCode", "field": "res.statusCode"},
    {"name": "req.caller", "field": "req.caller"},
    {"name": "latency", "field": "latency", "aggr": "quantize"}]}
RADIX = [64, 4, 16, 8, 32, 20]
FILTER = {"eq": ["req.method", "GET"]}
BREAKDOWNS = "host,operation"


def columns(lo, hi):
    """Rows lo..hi of the dense enumeration, as the sink buffers them."""
    i = np.arange(lo, hi, dtype=np.int64)
    digits = []
    for r in RADIX:
        digits.append(i % r)
        i = i // r
    hosts = np.array(["host%02d.example.com" % k for k in range(64)])
    methods = np.array(["GET", "PUT", "HEAD", "DELETE"])
    ops = np.array(["op_%s" % chr(97 + k) * 3 for k in range(16)])
    status = np.array(["200", "204", "301", "400", "403", "404", "500",
                       "503"])
    callers = np.array(["caller-%03d" % k for k in range(32)])
    lat = np.where(digits[5] == 0, 0, 1 << np.maximum(digits[5] - 1, 0))
    return [hosts[digits[0]].tolist(), methods[digits[1]].tolist(),
            ops[digits[2]].tolist(), status[digits[3]].tolist(),
            callers[digits[4]].tolist(), lat.tolist()], \
        (1 + (np.arange(lo, hi) % 7)).tolist()


def write_index_file(path, lo, hi):
    sink = IndexSink(path, [METRIC])
    sink._cols[0], sink._vals[0] = columns(lo, hi)
    sink.flush()


def build_tree(root, nrows, nfiles):
    """-> (index root, interval)."""
    if nfiles == 1:
        write_index_file(
            os.path.join(root, "by_day", "2014-05-01.sqlite"), 0, nrows)
        return root, "day"
    per = (nrows + nfiles - 1) // nfiles
    for h in range(nfiles):
        write_index_file(
            os.path.join(root, "by_hour", "2014-05-01-%02d.sqlite" % h),
            h * per, min(nrows, (h + 1) * per))
    return root, "hour"


def tree_bytes(root, suffix):
    n = 0
    for d, _dirs, names in os.walk(root):
        n += sum(os.path.getsize(os.path.join(d, f)) for f in names
                 if f.endswith(suffix))
    return n


def fmt(ts):
    ms = [t * 1e3 for t in ts]
    return "%.1f (%.1f..%.1f)" % (statistics.median(ms), min(ms), max(ms))


def datasource(root, engine):
    from dragnet_amd.config import Datasource
    from dragnet_amd.datasource.file import FileDatasource
    ds = Datasource(name="ab", backend="file", path="/dev/null",
                    index_path=root, time_field="time")
    return FileDatasource(ds, engine=engine)


def the_query():
    from dragnet_amd.query import query_load
    return query_load(filter=FILTER, breakdown_specs=BREAKDOWNS)


def run_paths(fd, interval, reps):
    """Alternate the three paths; -> {path: [seconds]}, points equal."""
    real_open = columnar.open_sidecar
    times = {"sqlite": [], "k7": [], "sidecar": []}
    points = {}
    for rep in range(reps + 1):  # the first round warms up
        for path in ("sqlite", "k7", "sidecar"):
            os.environ["DRAGNET_INDEX_GPU"] = "0" if path == "sqlite" \
                else "1"
            columnar.open_sidecar = (lambda *a, **k: None) \
                if path == "k7" else real_open
            before = columnar.STATS["sidecar_files"]
            t0 = time.perf_counter()
            res = fd.query(the_query(), interval=interval)
            pts = res.aggregators[0].points()
            dt = time.perf_counter() - t0
            took = columnar.STATS["sidecar_files"] > before
            assert took == (path == "sidecar"), path
            points[path] = pts
            if rep:
                times[path].append(dt)
    columnar.open_sidecar = real_open
    assert points["k7"] == points["sqlite"] == points["sidecar"]
    return times


def sidecar_split(fd, interval, reps):
    """The sidecar path's phases, by hand: -> {phase: [seconds]}."""
    from dragnet_amd import krill
    q = the_query()
    out = {}
    for rep in range(reps + 1):
        t = {}
        t0 = time.perf_counter()
        paths = [p for p, _ in fd._find_index_files(q, interval)]
        scs = [columnar.open_sidecar(p) for p in paths]
        (found, members), = columnar.group_sidecars(scs, q)[0]
        t["read headers"] = time.perf_counter() - t0
        t0 = time.perf_counter()
        (mg,), _rej = columnar.merge_group(
            members, columnar.needed_columns(q, found))
        t["load + merge"] = time.perf_counter() - t0
        filt = krill.filter_and(q.filter, None)
        fd.engine().coded_query(q, filt, mg.params, mg.kinds, mg,
                                timings=t)
        if rep:
            for k, v in t.items():
                out.setdefault(k, []).append(v)
    return out


def cli_times(root, interval, reps, engine="gpu"):
    cfg = os.path.join(root, "dn_config.json")
    env = dict(os.environ, DRAGNET_CONFIG=cfg, DRAGNET_ENGINE=engine,
               PYTHONPATH=REPO)
    dn = [sys.executable, "-m", "dragnet_amd.cli"]
    subprocess.run(dn + ["datasource-add", "ab", "--path=/dev/null",
                         "--index-path=" + root, "--time-field=time"],
                   env=env, check=True)
    import json
    argv = dn + ["query", "--interval=" + interval, "-f",
                 json.dumps(FILTER), "-b", BREAKDOWNS, "ab"]
    # "0" never creates the engine; "auto" creates it (to learn that
    # it is a GPU engine) whichever way the row threshold then decides,
    # so auto-to-SQLite is what the sidecar path has to beat in a CLI
    never = str(1 << 62)
    paths = (("sqlite", "0", never), ("auto-sqlite", "auto", never),
             ("sidecar", "auto", "0"))
    out = {name: [] for name, _m, _r in paths}
    outputs = {}
    for _ in range(reps):
        for name, mode, rows in paths:
            t0 = time.perf_counter()
            r = subprocess.run(
                argv, env=dict(env, DRAGNET_INDEX_GPU=mode,
                               DRAGNET_INDEX_COLUMNAR_ROWS=rows),
                capture_output=True, check=True, timeout=300)
            out[name].append(time.perf_counter() - t0)
            outputs[name] = r.stdout
    assert outputs["sqlite"] == outputs["sidecar"] == outputs["auto-sqlite"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cli-reps", type=int, default=3)
    ap.add_argument("--sizes", default="50000,500000,2000000")
    ap.add_argument("--hourly", type=int, default=2000000,
                    help="rows of the 24-file hourly tree (0: none)")
    ap.add_argument("--keep", help="leave the last tree in this directory")
    ap.add_argument("--kernels-only", metavar="DIR")
    ap.add_argument("--out")
    args = ap.parse_args()

    from dragnet_amd.engine.gpu import GpuEngine
    eng = GpuEngine()

    if args.kernels_only:
        fd = datasource(args.kernels_only, eng)
        interval = "hour" if os.path.isdir(
            os.path.join(args.kernels_only, "by_hour")) else "day"
        os.environ["DRAGNET_INDEX_GPU"] = "1"
        for _ in range(args.reps):
            fd.query(the_query(), interval=interval)
        return

    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    cases = [(int(n), 1) for n in args.sizes.split(",") if n]
    if args.hourly:
        cases.append((args.hourly, 24))
    say("| rows | files | SQLite ms | K7 forced ms | sidecar ms | "
        "sidecar/SQLite | .sqlite MB | .dncol MB | write sidecars ms |")
    say("|---|---|---|---|---|---|---|---|---|")
    splits, clis = [], []
    for nrows, nfiles in cases:
        keep = args.keep if (nrows, nfiles) == cases[-1] else None
        tmp = None if keep else tempfile.TemporaryDirectory()
        root = keep or tmp.name
        root, interval = build_tree(root, nrows, nfiles)
        from dragnet_amd.tools import index_columnar
        t0 = time.perf_counter()
        index_columnar.refresh(root)
        t_side = time.perf_counter() - t0
        fd = datasource(root, eng)
        times = run_paths(fd, interval, args.reps)
        med = {k: statistics.median(v) for k, v in times.items()}
        say("| %d | %d | %s | %s | %s | %.2fx | %.1f | %.1f | %.0f |" % (
            nrows, nfiles, fmt(times["sqlite"]), fmt(times["k7"]),
            fmt(times["sidecar"]), med["sidecar"] / med["sqlite"],
            tree_bytes(root, ".sqlite") / 1e6,
            tree_bytes(root, ".dncol") / 1e6, t_side * 1e3))
        splits.append((nrows, nfiles,
                       sidecar_split(fd, interval, args.reps)))
        if args.cli_reps:
            clis.append((nrows, nfiles,
                         cli_times(root, interval, args.cli_reps)))
        if tmp is not None:
            tmp.cleanup()
    say()
    say("Sidecar path split, ms, median (min..max):")
    say()
    phases = ["read headers", "load + merge", "h2d", "kernels", "decode"]
    say("| rows | files | " + " | ".join(phases) + " |")
    say("|---|---|" + "---|" * len(phases))
    for nrows, nfiles, sp in splits:
        say("| %d | %d | %s |" % (nrows, nfiles, " | ".join(
            fmt(sp[p]) for p in phases)))
    if clis:
        say()
        say("`dn query` wall time, ms, median (min..max):")
        say()
        say("| rows | files | SQLite (`=0`, no engine) | SQLite (`auto`, "
            "engine created) | sidecar (`auto`) |")
        say("|---|---|---|---|---|")
        for nrows, nfiles, c in clis:
            say("| %d | %d | %s | %s | %s |" % (
                nrows, nfiles, fmt(c["sqlite"]), fmt(c["auto-sqlite"]),
                fmt(c["sidecar"])))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

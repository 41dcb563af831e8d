#!/usr/bin/env python3
"""
dragnet_amd flagship benchmark — the driver contract.

Measures the headline metric from BASELINE.json: NDJSON records/sec
(whole node) + GB/s for a `dn scan` with a krill filter and a 2-field
breakdown (req.method, res.statusCode) over synthetic muskie-shaped
NDJSON (the tools/mktestdata record shape), scanned by the fused
MI355X CDNA4 kernel with data-parallel fan-out over N GPUs and an
RCCL merge of per-GPU partial aggregates each step.

One "step" = one complete scan job over this rank's resident pool:
async H2D staging of the pool, device newline index, fused scan
kernel, table extraction + decode, cross-rank aggregate merge.
Per-GPU work is fixed as N grows (weak scaling).

    python bench.py --gpus N --steps K --warmup W [--mb MB]
                    [--dump-outputs DIR] [--full]

A plain run sets up, warms up, times the K steps and prints the one
JSON result line.  --dump-outputs DIR also writes the aggregate the
last timed step returned as DIR/<name>.npy; the pool is seeded, so two
builds run with the same arguments scan identical bytes and their
dumps compare output for output.  --full is where measurements beyond
the headline figure belong; none exist today, so it changes nothing.

For N>1 launch via torch.distributed.run with --nproc-per-node N
(reads RANK/LOCAL_RANK/WORLD_SIZE/MASTER_* from the env).
"""

import argparse
import json
import multiprocessing
import os
import sys
import time


def log(msg):
    if int(os.environ.get("RANK", 0)) == 0:
        sys.stderr.write("[bench] %s\n" % msg)
        sys.stderr.flush()


SLAB_MB = 64


def build_slab(job):
    """One pool slab: at least `target` bytes of synthetic NDJSON
    (mktestdata shape) from its own seed."""
    target, seed = job
    from dragnet_amd.tools.mktestdata import generate_lines
    out = []
    total = 0
    nrec = 0
    # open-ended generator so the record count adapts to actual line size
    gen = generate_lines(1 << 62, seed=seed)
    for line in gen:
        out.append(line)
        total += len(line)
        nrec += 1
        if total >= target:
            break
    return b"".join(out), nrec


def build_pool(mb, seed, workers=1):
    """Generate ~mb MB of synthetic NDJSON (mktestdata shape).

    The pool is a run of SLAB_MB slabs, slab i seeded (seed, i), so its
    bytes depend on (mb, seed) alone and not on `workers`.  The
    generator is pure Python, about a minute per GB on one core, so
    the independent slabs are generated in parallel.  Workers are
    forked: call this before anything initialises the GPU."""
    target = mb * 1024 * 1024
    nslab = max(1, -(-mb // SLAB_MB))
    jobs = [(-(-target // nslab), (seed << 16) + i)
            for i in range(nslab)]
    workers = max(1, min(workers, nslab))
    if workers == 1:
        slabs = [build_slab(j) for j in jobs]
    else:
        with multiprocessing.get_context("fork").Pool(workers) as mp:
            slabs = mp.map(build_slab, jobs, chunksize=1)
    return b"".join(s for s, _ in slabs), sum(n for _, n in slabs)


def dump_outputs(dirname, result):
    """Write the aggregate a caller of the timed path receives — the
    sorted points of the last timed step — as float64 .npy arrays:
    point_values[i] is point i's count, point_keys[i] the UTF-8 code
    units of its canonical-JSON `fields`, zero-padded to a common
    width."""
    import numpy as np
    points = result.points()
    keys = [json.dumps(p["fields"], sort_keys=True,
                       separators=(",", ":")).encode("utf-8")
            for p in points]
    width = max([len(k) for k in keys] + [1])
    karr = np.zeros((len(keys), width), dtype=np.float64)
    for i, k in enumerate(keys):
        karr[i, :len(k)] = np.frombuffer(k, dtype=np.uint8)
    varr = np.array([p["value"] for p in points], dtype=np.float64)
    assert karr.nbytes + varr.nbytes <= 64 << 20, \
        "aggregate too large to dump whole"
    os.makedirs(dirname, exist_ok=True)
    np.save(os.path.join(dirname, "point_keys.npy"), karr)
    np.save(os.path.join(dirname, "point_values.npy"), varr)
    log("dumped %d points to %s" % (len(points), dirname))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--mb", type=int,
                    default=int(os.environ.get("DRAGNET_BENCH_MB", 1024)),
                    help="per-GPU NDJSON pool size (MB; swept 256->512"
                         "->1024->2048: 1024 is +2.6%% over 512, 2048 "
                         "flat — fewer pass boundaries)")
    ap.add_argument("--device-resident", action="store_true",
                    help="skip per-step H2D (data already in HBM): "
                         "measures kernel-side scan throughput")
    ap.add_argument("--passes", type=int, default=0,
                    help="full pool passes per step (0 = auto-size so "
                         "a step is ~150 ms of GPU work)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write the last timed "
                         "step's aggregate as DIR/<name>.npy (rank 0)")
    ap.add_argument("--full", action="store_true",
                    help="also run every measurement beyond the "
                         "headline figure (none today)")
    args = ap.parse_args()
    assert args.steps >= 1, "--steps must be at least 1"

    rank = int(os.environ.get("RANK", 0))
    world = int(os.environ.get("WORLD_SIZE", 1))
    local_rank = int(os.environ.get("LOCAL_RANK", 0))

    # Self-launch: `python bench.py --gpus N` (no torchrun) re-execs
    # under torch.distributed.run with one rank per GPU, so the driver
    # measures N GPUs however it invokes us.
    if args.gpus > 1 and world == 1:
        import socket
        import subprocess
        s = socket.socket()
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
        s.close()
        cmd = [sys.executable, "-m", "torch.distributed.run",
               "--nnodes=1", "--nproc-per-node", str(args.gpus),
               "--master-addr", "127.0.0.1",
               "--master-port", str(port),
               os.path.abspath(__file__)] + sys.argv[1:]
        log("self-launching %d ranks via torch.distributed.run"
            % args.gpus)
        sys.exit(subprocess.call(cmd))

    # the pool first: its generator forks workers, which must not
    # inherit an initialised GPU runtime
    log("generating %d MB pool per GPU ..." % args.mb)
    t0 = time.time()
    ncpu = len(os.sched_getaffinity(0))
    pool, nrec = build_pool(args.mb, seed=1000 + rank,
                            workers=max(1, min(16, ncpu) // world))
    pool_bytes = len(pool)
    log("pool: %d records, %.1f MB in %.1fs" % (
        nrec, pool_bytes / 1e6, time.time() - t0))

    import torch
    assert torch.cuda.is_available(), "bench needs a GPU"

    # backend override for plumbing rehearsals on a single GPU
    # (DRAGNET_BENCH_BACKEND=gloo shares cuda:0 across ranks and
    # merges through CPU tensors; production N>1 uses RCCL)
    backend = os.environ.get("DRAGNET_BENCH_BACKEND", "nccl")
    ngpu = torch.cuda.device_count()
    dev_index = local_rank if backend == "nccl" else local_rank % ngpu
    torch.cuda.set_device(dev_index)

    dist = None
    if world > 1:
        import torch.distributed as torch_dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29601")
        # keep stdout pure for the one-JSON-line contract: the gloo /
        # RCCL init banners printf to fd 1, so route fd 1 to stderr
        # around init
        sys.stdout.flush()
        saved_fd1 = os.dup(1)
        os.dup2(2, 1)
        try:
            torch_dist.init_process_group(backend, rank=rank,
                                          world_size=world)
        finally:
            sys.stdout.flush()
            os.dup2(saved_fd1, 1)
            os.close(saved_fd1)
        dist = torch_dist

    from dragnet_amd.distributed import merge_tables_tensor
    from dragnet_amd.engine import plan as planmod
    from dragnet_amd.engine.gpu import GpuEngine, _ScanContext
    from dragnet_amd.query import query_load

    query = query_load(
        filter={"eq": ["req.method", "GET"]},
        breakdown_specs="req.method,res.statusCode")

    eng = GpuEngine(device=torch.device("cuda", dev_index))
    cplan = planmod.compile_plan([query])
    eng.chunk_bytes = pool_bytes  # single-chunk pool
    ctx = _ScanContext(eng, cplan,
                       agg_slots=1 << 16, dict_slots=1 << 16,
                       dict_data_cap=32 << 20)
    ctx.stage_resident(pool)
    device = eng.device

    xpose = (args.device_resident
             and os.environ.get("DRAGNET_XPOSE") == "1")
    if xpose:
        log("staging wave-transposed pool ...")
        ctx.stage_xpose(pool)
    if args.device_resident and not xpose:
        ctx.scan_resident()  # prime HBM once

    # hipGraph replay pays on the device-resident path (one launch per
    # step); captured H2D memcpy nodes serialize against the kernels
    # and HURT the streaming path (35 vs 47 GB/s measured), so graphs
    # stay off when copies are in the loop.
    # hipGraph replay pays on the linear device-resident path; it
    # measured -6% on the wave-transposed path (single kernel + fused
    # reset already) so xpose runs ungraphed.
    graph = None
    if (args.device_resident and not xpose
            and os.environ.get("DRAGNET_NO_GRAPH") != "1"):
        graph = ctx.make_graph(h2d=False)
        log("hipGraph capture: %s"
            % ("ok" if graph is not None else "unavailable"))

    # Software pipeline: each step enqueues its scan + extraction and
    # then decodes the PREVIOUS step's snapshot on the host while this
    # step's copies/kernels run (decode syncs only on the snapshot's
    # event, on a dedicated D2H stream).  drain() decodes the last
    # pending handle, so a timed region of K steps + one drain does
    # exactly K scans and K decodes — no work leaves the clock.
    pending = [None]

    def do_merge(agg):
        if dist is not None:
            return merge_tables_tensor(
                agg, query,
                device if backend == "nccl" else torch.device("cpu"))
        return agg

    # Multi-pass steps: one step = `passes` full scans of the pool
    # accumulated into ONE aggregate job (reset + P scans + 1 extract),
    # sized so the timed region is seconds of observable GPU work, not
    # 0.1 s.
    passes = args.passes
    if passes <= 0:
        # ~150 ms/step at the measured ~53 GB/s streaming rate
        passes = max(1, 8192 // max(args.mb, 1))

    def step():
        if graph is not None:
            for _ in range(passes):
                graph.replay()
        elif xpose:
            ctx.reset()
            for _ in range(passes):
                ctx.scan_xpose()
        else:
            ctx.reset()
            for _ in range(passes):
                ctx.scan_resident(h2d=not args.device_resident)
        ex = ctx.extract_async([query])
        merged = None
        if pending[0] is not None:
            aggs, _stages = ctx.decode_extracted(pending[0], [query])
            merged = do_merge(aggs[0])
        pending[0] = ex
        return merged

    def drain():
        if pending[0] is None:
            return None
        aggs, _stages = ctx.decode_extracted(pending[0], [query])
        pending[0] = None
        return do_merge(aggs[0])

    # warmup
    for _ in range(args.warmup):
        step()
    result = drain()
    assert int(ctx.counters[1].item()) == 0, "invalid JSON in pool?!"

    # timed region
    if dist is not None:
        dist.barrier()
    torch.cuda.synchronize(device)
    t_start = time.time()
    for _ in range(args.steps):
        r = step()
        if r is not None:
            result = r
    result = drain()
    torch.cuda.synchronize(device)
    if dist is not None:
        dist.barrier()
    elapsed = time.time() - t_start

    # max over ranks
    if dist is not None:
        red_dev = device if backend == "nccl" else torch.device("cpu")
        t = torch.tensor([elapsed], dtype=torch.float64, device=red_dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())

    total_records = nrec * passes * args.steps * world
    total_bytes = pool_bytes * passes * args.steps * world
    recs_per_sec = total_records / elapsed
    gb_per_sec = total_bytes / elapsed / 1e9
    ms_per_step = elapsed / args.steps * 1000.0

    # sanity: the scan actually matched records
    matched = sum(p["value"] for p in result.points())
    assert matched > 0, "no records matched the filter"

    if rank == 0 and args.dump_outputs:
        dump_outputs(args.dump_outputs, result)

    if rank == 0:
        out = {
            "metric": "NDJSON records/sec (whole node), krill filter "
                      "+ 2-field breakdown (req.method,res.statusCode)",
            "value": round(recs_per_sec, 1),
            "unit": "records/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(ms_per_step, 3),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "uint8",
            "data": "synthetic (mktestdata muskie-shaped NDJSON, "
                    "random-generated, %d MB/GPU %s pool, "
                    "%d passes/step)"
                    % (args.mb,
                       "device-resident wave-transposed" if xpose
                       else "device-resident" if args.device_resident
                       else "host-staged", passes),
            "gb_per_sec": round(gb_per_sec, 3),
            "config": {
                "model": "dn scan: filter eq(req.method,GET) + "
                         "breakdown req.method,res.statusCode",
                "global_batch": nrec * world,
                "seq_len": int(pool_bytes / max(nrec, 1)),
                "parallelism": "dp%d" % world,
            },
        }
        print(json.dumps(out))
    if dist is not None:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()

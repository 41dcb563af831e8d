"""
Multi-GPU data parallelism: shard the input across ranks, merge partial
aggregates over RCCL/xGMI.

The reference's distributed path is Manta map/reduce — one map task per
input object emitting skinner points, one reduce re-aggregating them
(reference lib/datasource-manta.js:202-219).  Here the same shape runs
as one process per GPU under torch.distributed (backend "nccl" IS RCCL
on ROCm; "gloo" for CPU tests):

  * shard assignment: round-robin over the file list (the analog of
    addJobKey fan-out, lib/datasource-manta.js:549-559)
  * merge: per-rank aggregate tables are exchanged as DENSE TENSORS and
    re-aggregated — correctness rests on points merging associatively/
    commutatively (proved by the x3 idempotence test)

The merge (C1+C2 of SURVEY.md §2c) is fully tensor-typed — no object
serialization crosses the wire.  This module does the collectives; what
happens to the gathered tensors needs no process group and is merge.py
(reaggregate, unify_dictionaries and the wire form they read):

  C2 dictionary exchange: each rank's string dictionary travels as a
     UTF-8 byte blob + offset tensor (_gather_dictionaries).
  C1 table exchange: each rank's table travels as an int64 key-code
     matrix, a tag column and an f64 value vector.  Payloads are
     typically <= MBs, so the latency-optimal direct all_gather beats
     ring algorithms on xGMI's 7 p2p links (SURVEY.md §5 topology
     note); every rank re-aggregates the union (allreduce semantics).
  Pathological cardinality (> _PARTITION_ROWS local rows): hash-
     partition the keys with all_to_all_single so each rank owns and
     merges one key range (reduce-scatter shape), then all_gather the
     merged partitions.
"""

import os

import numpy as np

# _rebuild_table: not called here, importable beside _encode_table, its inverse
from .merge import (_EL_STR, WireTable, _encode_table,  # noqa: F401
                    _group_rows, _np, _rebuild_table, _strings_blob,
                    encode_table, partition_rows, reaggregate,
                    reaggregate_points,
                    unify_dictionaries)

_PARTITION_ROWS = 1 << 20  # switch to hash-partition all_to_all above


def dist_env():
    """(rank, world_size, local_rank) from torchrun env, or (0,1,0)."""
    return (int(os.environ.get("RANK", 0)),
            int(os.environ.get("WORLD_SIZE", 1)),
            int(os.environ.get("LOCAL_RANK", 0)))


def init_process_group(backend=None):
    import torch
    import torch.distributed as dist
    if dist.is_initialized():
        return dist
    rank, world, local = dist_env()
    if world == 1:
        return None
    if backend is None:
        # DRAGNET_DIST_BACKEND=gloo lets N ranks rehearse on one GPU
        # (RCCL refuses duplicate devices); production defaults to
        # RCCL when CUDA/HIP devices are visible
        backend = os.environ.get("DRAGNET_DIST_BACKEND") or \
            ("nccl" if torch.cuda.is_available() else "gloo")
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29517")
    if backend == "nccl":
        torch.cuda.set_device(local)
    dist.init_process_group(backend=backend, rank=rank,
                            world_size=world)
    return dist


def shard_files(files, rank, world):
    """Round-robin shard assignment (deterministic across ranks)."""
    return [f for i, f in enumerate(files) if i % world == rank]


def _coll_device(group=None):
    """Device collectives must use: CUDA for RCCL, CPU for gloo."""
    import torch
    import torch.distributed as dist
    if dist.get_backend(group) == "nccl":
        return torch.device("cuda", torch.cuda.current_device())
    return torch.device("cpu")


# ---- collectives -------------------------------------------------------

def _all_gather_padded(t, sizes, device, group):
    """all_gather a variable-length 1-D tensor: pad to the global max
    (>=1 so zero-length never reaches RCCL), return per-rank tensors
    trimmed to their true sizes."""
    import torch
    import torch.distributed as dist
    world = dist.get_world_size(group)
    maxn = max(max(sizes), 1)
    padded = torch.zeros(maxn, dtype=t.dtype, device=device)
    if t.numel():
        padded[:t.numel()] = t
    bufs = [torch.empty(maxn, dtype=t.dtype, device=device)
            for _ in range(world)]
    dist.all_gather(bufs, padded, group=group)
    return [b[:sizes[r]] for r, b in enumerate(bufs)]


def _to_device(arr, dtype, device):
    import torch
    if torch.is_tensor(arr):  # a device wire table: no upload
        return arr.contiguous().to(device=device, dtype=dtype)
    return torch.from_numpy(np.ascontiguousarray(arr)).to(
        device=device, dtype=dtype)


def _gather_dictionaries(blob, soffs, ns_strs, ns_blob, device, group):
    """all_gather the ranks' dictionaries in wire form, given every
    rank's string and byte counts: one (blob, offs) pair per rank."""
    import torch
    g_soffs = _all_gather_padded(_to_device(soffs, torch.int64, device),
                                 list(ns_strs + 1), device, group)
    g_blob = _all_gather_padded(_to_device(blob, torch.uint8, device),
                                list(ns_blob), device, group)
    return list(zip(g_blob, g_soffs))


def merge_tables_tensor(agg, query, device=None, group=None,
                        as_points=False):
    """Dense RCCL merge of one aggregation table (C1+C2); every rank
    returns the fully-merged Aggregator (allreduce semantics).  See
    module docstring for the wire format; no object serialization.
    agg is this rank's Aggregator, encoded here on the host, or its
    WireTable (merge.encode_table): one on the device is neither
    encoded nor uploaded.  With as_points every rank returns the merged
    table's points as NDJSON bytes instead (merge.reaggregate_points):
    no Aggregator is built, so no counters travel with it."""
    import torch
    import torch.distributed as dist

    if device is None:
        device = _coll_device(group)
    nk = len(query.breakdowns)
    if not isinstance(agg, WireTable):
        agg = encode_table(agg, query)
    codes, tagpack, vals = agg.codes, agg.tagpack, agg.vals
    blob, soffs = agg.strings

    world = dist.get_world_size(group)
    meta = torch.tensor([codes.shape[0], len(soffs) - 1, len(blob)],
                        dtype=torch.int64, device=device)
    metas = [torch.empty(3, dtype=torch.int64, device=device)
             for _ in range(world)]
    dist.all_gather(metas, meta, group=group)
    ns_rows, ns_strs, ns_blob = torch.stack(metas).cpu().numpy().T
    # path choice is COLLECTIVE (computed from the gathered sizes, so
    # every rank takes the same branch): pathological cardinality goes
    # through the hash-partition reduce-scatter shape instead of
    # shipping every row everywhere
    if int(ns_rows.max()) > _PARTITION_ROWS:
        dicts = _gather_dictionaries(blob, soffs, ns_strs, ns_blob, device,
                                     group)
        merged = _merge_partitioned(query, codes, tagpack, vals, dicts,
                                    device, group, as_points)
    else:
        g_codes = _all_gather_padded(
            _to_device(codes.reshape(-1), torch.int64, device),
            list(ns_rows * nk), device, group)
        g_tags = _all_gather_padded(
            _to_device(tagpack, torch.int64, device), list(ns_rows),
            device, group)
        g_vals = _all_gather_padded(
            _to_device(vals, torch.float64, device), list(ns_rows),
            device, group)
        dicts = _gather_dictionaries(blob, soffs, ns_strs, ns_blob, device,
                                     group)
        # C2 + C1: the gathered blobs, offsets, codes, tags and values
        # go to reaggregate as they are; unify_dictionaries decodes the
        # strings it needs
        parts = [(g_codes[r].reshape(int(ns_rows[r]), nk), g_tags[r],
                  g_vals[r]) for r in range(world)]
        merged = (reaggregate_points if as_points else reaggregate)(
            query, parts, dicts, device=device)
    if as_points:
        return merged
    merged.ninputs = agg.ninputs  # per-rank; callers sum via counters
    merged.ndropped_nonnumeric = agg.ndropped_nonnumeric
    return merged


def _merge_partitioned(query, codes, tagpack, vals, dicts, device, group,
                       as_points=False):
    """Pathological-cardinality path: hash-partition key rows across
    ranks with all_to_all_single (reduce-scatter shape — each rank
    merges one key range), then all_gather the merged partitions so
    every rank still ends with the full table.

    Strings cannot be hashed consistently pre-unification, so the
    global dictionary is built FIRST from the gathered `dicts` (strings
    are few relative to rows in any realistic pathological-cardinality
    table), then rows are partitioned on their remapped codes."""
    import torch
    import torch.distributed as dist

    world = dist.get_world_size(group)
    rank = dist.get_rank(group)
    nk = len(query.breakdowns)

    # C2 first: unify dictionaries globally
    gstrings, remaps = unify_dictionaries(dicts, device)

    # remap, hash each row to its rank, group by rank (merge.py: host or
    # GPU, same bits); remaps[rank] goes in where the unify left it
    wire, counts = partition_rows(codes, tagpack, vals, remaps[rank], world,
                                  device)
    if torch.is_tensor(wire):
        send = wire.reshape(-1).to(device)
        in_counts = (counts * (nk + 2)).to(device)
    else:
        send = _to_device(wire.reshape(-1), torch.int64, device)
        in_counts = torch.from_numpy(counts * (nk + 2)).to(device)
    out_counts = torch.empty_like(in_counts)
    dist.all_to_all_single(out_counts, in_counts, group=group)
    recv = torch.empty(int(out_counts.sum().item()), dtype=torch.int64,
                       device=device)
    dist.all_to_all_single(
        recv, send, list(out_counts.cpu().numpy()),
        list(in_counts.cpu().numpy()), group=group)

    def split(flat):
        """[n * (nk + 2)] i64 wire rows -> (codes, tagpack, vals)."""
        m = flat.reshape(-1, nk + 2)
        return (m[:, :nk], m[:, nk],
                m[:, nk + 1].contiguous().view(torch.float64))

    # merge my partition (codes are global already: no segments, no
    # remap), then share the merged partitions
    uniq, sums = _group_rows([split(recv)], None, nk, device)
    out = np.concatenate([uniq, sums.view(np.int64)[:, None]], axis=1)

    sz = torch.tensor([out.shape[0] * (nk + 2)], dtype=torch.int64,
                      device=device)
    szs = [torch.empty(1, dtype=torch.int64, device=device)
           for _ in range(world)]
    dist.all_gather(szs, sz, group=group)
    szs = [int(s.item()) for s in szs]
    parts = _all_gather_padded(
        _to_device(out.reshape(-1), torch.int64, device), szs, device,
        group)
    # every partition is in global codes: each rank's "dictionary" is
    # the global one and its remap the identity
    return (reaggregate_points if as_points else reaggregate)(
        query, [split(p) for p in parts], [gstrings] * world, device=device)


def merge_aggregators(aggs, queries, device=None, group=None):
    """Dense merge of every query's table; every rank returns the
    fully-merged [Aggregator, ...]."""
    return [merge_tables_tensor(a, q, device=device, group=group)
            for a, q in zip(aggs, queries)]


def merge_points_object(aggs, queries, group=None):
    """Rank-0 merge view (legacy name): dense tensor merge under the
    hood; returns merged [Aggregator, ...] on rank 0, None elsewhere."""
    import torch.distributed as dist
    merged = merge_aggregators(aggs, queries, group=group)
    return merged if dist.get_rank(group) == 0 else None


def merge_counter_stages(stages, group=None):
    """Sum per-stage counters across ranks (for --counters output).

    Every rank runs the identical pipeline, so the stage list shape
    and per-stage counter keys are identical everywhere; the values
    ride in one int64 tensor through all_reduce(SUM) — no object
    serialization.  Every rank returns the merged stages."""
    import torch
    import torch.distributed as dist
    device = _coll_device(group)
    vals = []
    for _name, c in stages:
        vals.extend(int(c[k]) for k in c)
    t = torch.tensor(vals or [0], dtype=torch.int64, device=device)
    dist.all_reduce(t, op=dist.ReduceOp.SUM, group=group)
    flat = t.cpu().numpy()
    out = []
    i = 0
    for name, c in stages:
        merged = {}
        for k in c:
            merged[k] = int(flat[i])
            i += 1
        out.append((name, merged))
    return out

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
serialization crosses the wire:

  C2 dictionary unification: each rank's string dictionary travels as a
     UTF-8 byte blob + offset tensor; every rank builds the global
     dictionary and remaps its peers' string codes into it
     (unify_dictionaries: a dict loop on the host, or the
     unify_strings kernels, ops/hip/unify_strings.h, on the gathered
     blobs where they lie; DRAGNET_UNIFY_GPU chooses).
  C1 table exchange: each rank's table flattens to an int64 key-code
     matrix [n, nk] (per-element tag: int / string-id / f64-bits packed
     into a companion column) and an f64 value vector.  Payloads are
     typically <= MBs, so the latency-optimal direct all_gather beats
     ring algorithms on xGMI's 7 p2p links (SURVEY.md §5 topology
     note); every rank re-aggregates the union (allreduce semantics):
     reaggregate() groups the rows and sums their values, on the host
     via np.unique + bincount or on the GPU with the merge_rows kernels
     (ops/hip/merge_rows.h; DRAGNET_MERGE_GPU chooses).
  Pathological cardinality (> _PARTITION_ROWS local rows): hash-
     partition the keys with all_to_all_single so each rank owns and
     merges one key range (reduce-scatter shape), then all_gather the
     merged partitions.
"""

import os

import numpy as np

from .points import Aggregator

# per-element tag values in the packed tag column
_EL_INT = 0   # int64 payload (ordinals, dates, integral counts)
_EL_STR = 1   # payload = index into the rank's string dictionary
_EL_F64 = 2   # payload = IEEE-754 bits of a float key element

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


# ---- dense table encode/decode ----------------------------------------

def _encode_table(agg, nk):
    """Flatten an Aggregator's table to dense arrays:
    (codes i64 [n, nk], tagpack i64 [n], vals f64 [n], strings list).
    Key elements are int (ordinal/date), str, or (defensively) float;
    strings are dictionary-encoded per rank (C2 unifies them)."""
    n = len(agg.table)
    codes = np.zeros((n, nk), dtype=np.int64)
    tagpack = np.zeros(n, dtype=np.int64)
    vals = np.empty(n, dtype=np.float64)
    strings = []
    sidx = {}
    for i, (k, v) in enumerate(agg.table.items()):
        vals[i] = v
        tp = 0
        for j, el in enumerate(k):
            if isinstance(el, str):
                si = sidx.get(el)
                if si is None:
                    si = sidx[el] = len(strings)
                    strings.append(el)
                codes[i, j] = si
                tp |= _EL_STR << (2 * j)
            elif isinstance(el, float) and not el.is_integer():
                codes[i, j] = np.float64(el).view(np.int64)
                tp |= _EL_F64 << (2 * j)
            else:
                iv = int(el)
                if -(1 << 63) <= iv < (1 << 63):
                    codes[i, j] = iv
                else:
                    # lquantize ordinals of absurd magnitudes exceed
                    # int64: ship as f64 bits (JS-float key semantics
                    # — the reference's ordinals are floats there
                    # anyway); every rank rebuilds the same float key
                    codes[i, j] = np.float64(float(iv)).view(np.int64)
                    tp |= _EL_F64 << (2 * j)
        tagpack[i] = tp
    return codes, tagpack, vals, strings


def _strings_blob(strings):
    bs = [s.encode("utf-8") for s in strings]
    offs = np.zeros(len(bs) + 1, dtype=np.int64)
    if bs:
        np.cumsum([len(b) for b in bs], out=offs[1:])
    return b"".join(bs), offs


def _decode_strings(blob_bytes, offs):
    return [blob_bytes[offs[i]:offs[i + 1]].decode("utf-8")
            for i in range(len(offs) - 1)]


def _group_host(X, vals):
    """Group identical rows of X [n, w] and sum vals over each group:
    (uniq [g, w] in np.unique's order, sums f64 [g])."""
    uniq, inv = np.unique(X, axis=0, return_inverse=True)
    sums = np.bincount(inv, weights=vals, minlength=uniq.shape[0])
    return uniq, sums


def _scalar_table(query, vals):
    """The table of a query without breakdowns: one scalar sum."""
    merged = Aggregator(query)
    if vals.size:
        total = float(vals.sum())
        merged.table[()] = int(total) if total.is_integer() else total
    return merged


def _decode_rows(query, uniq, sums, strings):
    """Decode each UNIQUE key row [codes..., tagpack] to the
    Aggregator's canonical Python tuple once, in row order."""
    merged = Aggregator(query)
    nk = len(query.breakdowns)
    for r in range(uniq.shape[0]):
        tp = int(uniq[r, nk])
        key = []
        for j in range(nk):
            tag = (tp >> (2 * j)) & 3
            c = int(uniq[r, j])
            if tag == _EL_STR:
                key.append(strings[c])
            elif tag == _EL_F64:
                key.append(float(np.int64(c).view(np.float64)))
            else:
                key.append(c)
        v = float(sums[r])
        merged.table[tuple(key)] = int(v) if v.is_integer() else v
    return merged


def _rebuild_table(query, codes, tagpack, vals, strings):
    """Vectorized host re-aggregation of one dense table: group
    identical key rows with np.unique and sum values with bincount
    (_group_host), then decode the unique rows (_decode_rows).  The
    per-row Python of _encode_table and of the decode loop is what it
    was; vectorising either is a separate piece of work."""
    if len(query.breakdowns) == 0:
        return _scalar_table(query, vals)
    X = np.concatenate([codes, tagpack[:, None]], axis=1)
    return _decode_rows(query, *_group_host(X, vals), strings)


# ---- re-aggregation of gathered tables ---------------------------------

MERGE_GPU_ROWS_DEFAULT = float("inf")


def _env_merge_gpu_rows():
    """Total rows from which DRAGNET_MERGE_GPU=auto groups on the GPU
    (DRAGNET_MERGE_GPU_ROWS).  profiles/r08_merge_rows.md measured no
    size that wins at every cardinality, hence the default of infinity:
    auto mode never selects it, DRAGNET_MERGE_GPU=1 does.  With the
    rows ordered on the device (profiles/r09_sort_rows.md) the same
    rule gives 10000; the default is unchanged so far."""
    v = os.environ.get("DRAGNET_MERGE_GPU_ROWS")
    if v is None:
        return MERGE_GPU_ROWS_DEFAULT
    try:
        return int(v)
    except ValueError:
        return float("inf")


def _merge_on_gpu(n_rows, nk):
    """Path choice of the row grouping (DRAGNET_MERGE_GPU): "0" always
    the host; "1" the GPU whenever one is visible; "auto" the GPU from
    DRAGNET_MERGE_GPU_ROWS rows up.  A table without breakdowns is a
    scalar sum and an empty one is nothing: both stay on the host."""
    mode = os.environ.get("DRAGNET_MERGE_GPU", "auto")
    if mode == "0" or nk < 1 or n_rows == 0:
        return False
    if mode != "1" and n_rows < _env_merge_gpu_rows():
        return False
    import torch
    return torch.cuda.is_available()


def _np(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def _group_rows_host(parts, remaps, nk):
    """Remap (numpy fancy indexing), concatenate, group: the reference
    the device path must equal bit for bit."""
    all_rows, all_vals = [], []
    for r, (codes, tags, vals) in enumerate(parts):
        rt = _np(tags).astype(np.int64, copy=False)
        rc = _np(codes).reshape(rt.shape[0], nk).astype(np.int64,
                                                        copy=True)
        if remaps is not None:
            remap = _np(remaps[r])  # a device slice after a GPU unify
            for j in range(nk):
                is_str = ((rt >> (2 * j)) & 3) == _EL_STR
                if is_str.any():
                    rc[is_str, j] = remap[rc[is_str, j]]
        all_rows.append(np.concatenate([rc, rt[:, None]], axis=1))
        all_vals.append(_np(vals).astype(np.float64, copy=False))
    return _group_host(np.concatenate(all_rows), np.concatenate(all_vals))


def _group_rows_device(parts, remaps, nk, device):
    """One merge_rows call over the parts as segments; the remap runs
    inside the kernel.  Parts already on the GPU are never copied to
    the host; only the distinct rows and their sums come back, already
    in np.unique's order (lexicographic over the columns left to right,
    as signed int64: the radix sort of ops/hip/sort_rows.h, behind
    merge_rows' sort=True).  None when the kernel reports sums that
    depend on the order of its adds."""
    import torch

    from .ops import load_ops
    ops = load_ops(required=True)  # a missing extension is an error
    if device is None or torch.device(device).type != "cuda":
        on_gpu = [p[0].device for p in parts
                  if torch.is_tensor(p[0]) and p[0].is_cuda]
        device = on_gpu[0] if on_gpu else torch.device(
            "cuda", torch.cuda.current_device())

    def up(a, dtype):
        return torch.as_tensor(a).to(device=device, dtype=dtype)

    rows = torch.cat([
        torch.cat([up(codes, torch.int64).reshape(-1, nk),
                   up(tags, torch.int64).reshape(-1, 1)], dim=1)
        for codes, tags, _vals in parts])
    vals = torch.cat([up(v, torch.float64) for _c, _t, v in parts])
    kw = {}
    if remaps is not None:
        def offsets(sizes):
            return torch.from_numpy(
                np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64))
        if any(torch.is_tensor(m) for m in remaps):  # after a GPU unify
            remap = torch.cat([up(m, torch.int64) for m in remaps])
        else:
            remap = up(np.concatenate(remaps), torch.int64)
        kw = dict(
            seg_start=offsets([int(_t.shape[0]) for _c, _t, _v in parts]),
            remap=remap,
            remap_off=offsets([len(m) for m in remaps]))
    uniq, sums, exact = ops.merge_rows(rows, vals, nk, sort=True, **kw)
    if not exact:
        return None
    return uniq.cpu().numpy(), sums.cpu().numpy()


def _group_rows(parts, remaps, nk, device=None):
    """Group the rows [codes..., tagpack] of all parts and sum their
    values: (uniq [g, nk + 1], sums [g]) in np.unique's order.  remaps
    is one int64 table per part for its string-tagged codes, or None.

    The result is bit-identical whichever path runs.  Device f64 adds
    come in no fixed order, and only sums of non-negative integers that
    stay below 2^53 are independent of the order, so the kernel reports
    anything else (a fractional, negative, NaN or infinite weight, a
    value or a sum at or beyond 2^53) and the host path then answers."""
    n_rows = sum(int(p[1].shape[0]) for p in parts)
    out = None
    if _merge_on_gpu(n_rows, nk):
        out = _group_rows_device(parts, remaps, nk, device)
    if out is None:
        out = _group_rows_host(parts, remaps, nk)
    return out


# ---- dictionary unification (C2) ----------------------------------------

UNIFY_GPU_STRINGS_DEFAULT = float("inf")


def _env_unify_gpu_strings():
    """Total strings from which DRAGNET_UNIFY_GPU=auto unifies on the
    GPU (DRAGNET_UNIFY_GPU_STRINGS).  The default is infinity: auto mode
    never selects it, DRAGNET_UNIFY_GPU=1 does
    (profiles/r10_unify_strings.md)."""
    v = os.environ.get("DRAGNET_UNIFY_GPU_STRINGS")
    if v is None:
        return UNIFY_GPU_STRINGS_DEFAULT
    try:
        return int(v)
    except ValueError:
        return float("inf")


def _is_blob_pair(d):
    return isinstance(d, tuple) and len(d) == 2 and hasattr(d[0], "dtype")


def _unify_on_gpu(dicts, n_strings):
    """Path choice of the dictionary unification (DRAGNET_UNIFY_GPU),
    with DRAGNET_MERGE_GPU's meaning: "0" always the host; "1" the GPU
    whenever one is visible; "auto" the GPU from
    DRAGNET_UNIFY_GPU_STRINGS strings up.  Dictionaries that arrive as
    Python strings are on the host already and stay there."""
    mode = os.environ.get("DRAGNET_UNIFY_GPU", "auto")
    if mode == "0" or n_strings == 0:
        return False
    if not all(_is_blob_pair(d) for d in dicts):
        return False
    if mode != "1" and n_strings < _env_unify_gpu_strings():
        return False
    import torch
    return torch.cuda.is_available()


def _unify_host(dicts):
    """The dict loop: the reference the device path must equal."""
    gdict = {}
    gstrings = []
    remaps = []
    for d in dicts:
        rstr = _decode_strings(_np(d[0]).tobytes(), _np(d[1])) \
            if _is_blob_pair(d) else d
        remap = np.empty(len(rstr), dtype=np.int64)
        for i, s in enumerate(rstr):
            gi = gdict.get(s)
            if gi is None:
                gi = gdict[s] = len(gstrings)
                gstrings.append(s)
            remap[i] = gi
        remaps.append(remap)
    return gstrings, remaps


def _unify_device(dicts, device):
    """One unify_strings call (ops/hip/unify_strings.h) over the blobs
    as one blob.  Blobs already on the GPU are never copied to the host;
    the remap tables stay on the device, and only the bytes of the G
    first occurrences come back, to be decoded into gstrings."""
    import torch

    from .ops import load_ops
    ops = load_ops(required=True)  # a missing extension is an error
    if device is None or torch.device(device).type != "cuda":
        on_gpu = [d[0].device for d in dicts
                  if torch.is_tensor(d[0]) and d[0].is_cuda]
        device = on_gpu[0] if on_gpu else torch.device(
            "cuda", torch.cuda.current_device())

    def up(a, dtype):
        return torch.as_tensor(a).to(device=device, dtype=dtype)

    blobs = [up(b, torch.uint8).reshape(-1) for b, _o in dicts]
    offs = [up(o, torch.int64).reshape(-1) for _b, o in dicts]
    bases = np.concatenate(
        [[0], np.cumsum([int(b.numel()) for b in blobs])])
    counts = np.concatenate(
        [[0], np.cumsum([max(int(o.numel()) - 1, 0) for o in offs])])
    blob = torch.cat(blobs)
    start = torch.cat([o[:-1] + int(bases[r]) for r, o in enumerate(offs)])
    length = torch.cat([o[1:] - o[:-1] for o in offs])
    remap, first = ops.unify_strings(blob, start, length)
    remaps = [remap[int(counts[r]):int(counts[r + 1])]
              for r in range(len(dicts))]
    # the G distinct strings, packed in id order, are all that crosses
    flen = length[first]
    fend = torch.cumsum(flen, 0)
    shift = start[first] - (fend - flen)  # source minus packed position
    goffs = np.concatenate([[0], fend.cpu().numpy()])
    nbytes = int(goffs[-1])
    packed = blob[torch.repeat_interleave(shift, flen, output_size=nbytes)
                  + torch.arange(nbytes, device=device)]
    return _decode_strings(packed.cpu().numpy().tobytes(), goffs), remaps


def unify_dictionaries(dicts, device=None):
    """C2: one global dictionary out of the per-rank ones.  Each entry
    of dicts is a list of str, or the wire form (blob uint8 [bytes],
    offs int64 [n_r + 1]), numpy or torch on any device.  Returns
    (gstrings, remaps): the distinct strings, first seen first in rank
    order, and per rank the int64 table from its codes to indices of
    gstrings.  On the host this is a dict loop over the decoded strings;
    on the GPU (DRAGNET_UNIFY_GPU, wire-form entries only) the
    unify_strings kernels number the spans where the gather left them,
    the remaps stay device tensors for merge_rows, and only the distinct
    strings are decoded.  Both give the same result."""
    n_strings = sum(max(len(d[1]) - 1, 0) if _is_blob_pair(d) else len(d)
                    for d in dicts)
    if _unify_on_gpu(dicts, n_strings):
        return _unify_device(dicts, device)
    return _unify_host(dicts)


def reaggregate(query, parts, strings_per_part, device=None):
    """The step after the gather; needs no process group.  parts is
    one (codes [n_r, nk], tagpack [n_r], vals [n_r]) per rank, numpy or
    torch on any device, with string codes in that rank's dictionary
    strings_per_part[r]: a list of str or a (blob, offs) pair.  Builds
    the global dictionary (first seen first, in rank order) and the
    per-rank remap tables (unify_dictionaries: host or GPU, same
    result); remaps, groups and sums the rows (_group_rows: likewise),
    and decodes the distinct rows into the merged Aggregator, in
    np.unique's row order."""
    nk = len(query.breakdowns)
    if nk == 0:
        vals = [_np(v).astype(np.float64, copy=False)
                for _c, _t, v in parts]
        return _scalar_table(
            query, np.concatenate(vals) if vals else np.zeros(0))
    gstrings, remaps = unify_dictionaries(strings_per_part, device)
    uniq, sums = _group_rows(parts, remaps, nk, device)
    return _decode_rows(query, uniq, sums, gstrings)


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


def merge_tables_tensor(agg, query, device=None, group=None):
    """Dense RCCL merge of one aggregation table (C1+C2); every rank
    returns the fully-merged Aggregator (allreduce semantics).  See
    module docstring for the wire format; no object serialization."""
    import torch
    import torch.distributed as dist

    if device is None:
        device = _coll_device(group)
    nk = len(query.breakdowns)
    codes, tagpack, vals, strings = _encode_table(agg, nk)
    blob, soffs = _strings_blob(strings)

    world = dist.get_world_size(group)
    meta = torch.tensor([codes.shape[0], len(strings), len(blob)],
                        dtype=torch.int64, device=device)
    metas = [torch.empty(3, dtype=torch.int64, device=device)
             for _ in range(world)]
    dist.all_gather(metas, meta, group=group)
    metas = torch.stack(metas).cpu().numpy()
    ns_rows = metas[:, 0]
    ns_strs = metas[:, 1]
    ns_blob = metas[:, 2]
    # path choice is COLLECTIVE (computed from the gathered sizes, so
    # every rank takes the same branch): pathological cardinality goes
    # through the hash-partition reduce-scatter shape instead of
    # shipping every row everywhere
    if int(ns_rows.max()) > _PARTITION_ROWS:
        return _merge_partitioned(query, codes, tagpack, vals, strings,
                                  device, group, agg)

    def dev(arr, dtype):
        t = torch.from_numpy(np.ascontiguousarray(arr))
        return t.to(device=device, dtype=dtype)

    g_codes = _all_gather_padded(
        dev(codes.reshape(-1), torch.int64), list(ns_rows * nk),
        device, group)
    g_tags = _all_gather_padded(
        dev(tagpack, torch.int64), list(ns_rows), device, group)
    g_vals = _all_gather_padded(
        dev(vals, torch.float64), list(ns_rows), device, group)
    g_soffs = _all_gather_padded(
        dev(soffs, torch.int64), list(ns_strs + 1), device, group)
    g_blob = _all_gather_padded(
        dev(np.frombuffer(blob, dtype=np.uint8).copy(), torch.uint8),
        list(ns_blob), device, group)

    # C2 + C1: the gathered blobs, offsets, codes, tags and values go
    # to reaggregate as they are; unify_dictionaries decodes the strings
    # it needs
    strings_per_part = []
    parts = []
    for r in range(world):
        strings_per_part.append((g_blob[r], g_soffs[r]))
        parts.append((g_codes[r].reshape(int(ns_rows[r]), nk),
                      g_tags[r], g_vals[r]))
    merged = reaggregate(query, parts, strings_per_part, device=device)
    merged.ninputs = agg.ninputs  # per-rank; callers sum via counters
    merged.ndropped_nonnumeric = agg.ndropped_nonnumeric
    return merged


def _merge_partitioned(query, codes, tagpack, vals, strings, device,
                       group, agg):
    """Pathological-cardinality path: hash-partition key rows across
    ranks with all_to_all_single (reduce-scatter shape — each rank
    merges one key range), then all_gather the merged partitions so
    every rank still ends with the full table.

    Strings cannot be hashed consistently pre-unification, so the
    global dictionary is built FIRST (strings are few relative to
    rows in any realistic pathological-cardinality table), then rows
    are partitioned on their remapped codes.
    """
    import torch
    import torch.distributed as dist

    world = dist.get_world_size(group)
    rank = dist.get_rank(group)
    nk = len(query.breakdowns)

    # C2 first: unify dictionaries globally
    blob, soffs = _strings_blob(strings)
    meta = torch.tensor([len(strings), len(blob)], dtype=torch.int64,
                        device=device)
    metas = [torch.empty(2, dtype=torch.int64, device=device)
             for _ in range(world)]
    dist.all_gather(metas, meta, group=group)
    metas = torch.stack(metas).cpu().numpy()

    def dev(arr, dtype):
        return torch.from_numpy(np.ascontiguousarray(arr)).to(
            device=device, dtype=dtype)

    g_soffs = _all_gather_padded(dev(soffs, torch.int64),
                                 list(metas[:, 0] + 1), device, group)
    g_blob = _all_gather_padded(
        dev(np.frombuffer(blob, dtype=np.uint8).copy(), torch.uint8),
        list(metas[:, 1]), device, group)
    gstrings, remaps = unify_dictionaries(
        [(g_blob[r], g_soffs[r]) for r in range(world)], device)
    my_remap = _np(remaps[rank])
    for j in range(nk):
        is_str = ((tagpack >> (2 * j)) & 3) == _EL_STR
        if is_str.any():
            codes[is_str, j] = my_remap[codes[is_str, j]]

    # partition rows by key hash
    h = np.zeros(codes.shape[0], dtype=np.uint64)
    for j in range(nk):
        cj = np.ascontiguousarray(codes[:, j]).view(np.uint64)
        h = (h ^ cj) * np.uint64(0x100000001B3)
    h ^= tagpack.view(np.uint64)
    part = (h % np.uint64(world)).astype(np.int64)
    order = np.argsort(part, kind="stable")
    counts = np.bincount(part, minlength=world)

    row = np.concatenate(
        [codes, tagpack[:, None], vals.view(np.int64)[:, None]],
        axis=1)[order]  # [n, nk+2] i64 rows, grouped by target rank
    send = dev(row.reshape(-1), torch.int64)
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
    parts = _all_gather_padded(dev(out.reshape(-1), torch.int64), szs,
                               device, group)
    # every partition is in global codes: each rank's "dictionary" is
    # the global one and its remap the identity
    merged = reaggregate(query, [split(p) for p in parts],
                         [gstrings] * world, device=device)
    merged.ninputs = agg.ninputs
    merged.ndropped_nonnumeric = agg.ndropped_nonnumeric
    return merged


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

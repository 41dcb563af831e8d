"""
Index queries over stored columns on the GPU (ops/hip/scan_columns.h):
the host half of GpuEngine.columnar_query (K7: one index file's columns,
extracted out of SQLite) and GpuEngine.coded_query (the merged,
dictionary-coded columnar sidecars of a launch group).  Both compile the
same kernel plan, map its slots to columns, upload them, and run one
launch-finalize loop that retries with larger tables on overflow.
"""

import time

import numpy as np

from . import plan as planmod
from .gpu import _ScanContext, first_guess_slots

# ColDesc kinds (scan_columns.h)
COL_NUM, COL_STR, COL_CODED = 1, 2, 3


def column_plan(query, filt, extra=()):
    """The kernel plan of an index query over stored columns; `extra`
    breakdowns follow the query's own."""
    from ..query import QueryConfig

    # kernel plan: each breakdown reads the column keyed by its
    # FIELD name — the reference's deserializeRow reads
    # row[escape(field.field)] (lib/index-query.js:395-400), so a
    # renamed date breakdown (field != name) reads a column that
    # was never selected -> undefined -> dropped by the
    # bucketizer.  Stored columns are keyed by NAME, so mapping
    # the kernel slot by field reproduces exactly that; the
    # caller's query does the date/bucket decode.
    kq_bds = []
    for b in query.breakdowns:
        src = b.get("field", b["name"])
        nb = {"name": src, "field": src}
        if "aggr" in b:
            nb["aggr"] = b["aggr"]
            if "step" in b:
                nb["step"] = b["step"]
        kq_bds.append(nb)
    kq = QueryConfig(filter=None, breakdowns=kq_bds + list(extra),
                     allow_reserved=True)
    return planmod.compile_plan([kq], ds_filter=filt)


def _uploader(eng):
    """up(array, view=None): the array (viewed as dtype `view`) as a
    device tensor."""
    def up(arr, view=None):
        arr = np.ascontiguousarray(arr)
        return eng.torch.from_numpy(
            arr.view(view) if view else arr).to(eng.device)
    return up


def upload_columns(eng, cplan, params, kinds, number, string):
    """Upload the columns that the plan's slots read.  A slot reads the
    column of its name; companion slots, and any slot without a column,
    stay missing.  number(name, ci) -> the f64 array of numeric column
    ci; string(name, ci) -> (ColDesc kind, u32 soff array, u32 slen
    array or None).  -> (device descriptor array, the device tensors it
    points into)."""
    up = _uploader(eng)
    by_name = {p["name"]: i for i, p in enumerate(params)}
    nf = len(cplan.field_sigs)
    slot_kinds = [0] * nf
    nums, soffs, slens = ([eng.torch.empty(0)] * nf for _ in range(3))
    keep = []
    for si, (path, _raw) in enumerate(cplan.fields.paths):
        ci = by_name.get(path)
        if ci is None:
            continue
        if kinds[ci] == "n":
            slot_kinds[si] = COL_NUM
            nums[si] = up(number(path, ci))
            keep.append(nums[si])
        else:
            slot_kinds[si], off, length = string(path, ci)
            soffs[si] = up(off, np.int32)
            keep.append(soffs[si])
            if length is not None:
                slens[si] = up(length, np.int32)
                keep.append(slens[si])
    descs = eng.ops.col_descs_host(slot_kinds, nums, soffs, slens)
    return descs.to(eng.device), keep


def run_query(eng, cplan, decode_query, dict_cap, attempts, launch, error,
              tally=None):
    """launch(state) on fresh tables, finalize; on overflow again with
    8x the slots and 4x the string payload, `attempts` times in all
    (each retry counted in tally["retries"]), then RuntimeError(error).
    -> the Aggregator."""
    agg_slots, dict_slots = first_guess_slots()
    for _ in range(attempts):
        ctx = _ScanContext(eng, cplan, agg_slots, dict_slots,
                           min(dict_cap, 0xFFFFFFFF), dense=False)
        launch(ctx.state)
        aggs, _stages = ctx.finalize([decode_query])
        if not ctx.overflowed():
            return aggs[0]
        if tally is not None:
            tally["retries"] += 1
        agg_slots *= 8
        dict_slots *= 8
        dict_cap *= 4
    raise RuntimeError(error)


def columnar_query(eng, query, filt, params, kinds, cols, vals):
    """GpuEngine.columnar_query."""
    up = _uploader(eng)
    cplan = column_plan(query, filt)
    # one blob for every string column, each at its bias
    biases, blobs, bias = {}, [], 0
    for ci, c in enumerate(cols):
        if kinds[ci] == "s":
            biases[ci] = bias
            blobs.append(c[0])
            bias += len(c[0])
    blob = b"".join(blobs) or b"\0"
    blob_t = up(np.frombuffer(blob, dtype=np.uint8).copy())
    descs, keep = upload_columns(
        eng, cplan, params, kinds, lambda _name, ci: cols[ci],
        lambda _name, ci: (
            COL_STR, cols[ci][1].astype(np.uint32) + np.uint32(biases[ci]),
            cols[ci][2]))
    vals_t = up(vals)
    nrows = int(vals.shape[0])
    return run_query(
        eng, cplan, query, max(len(blob) * 2 + (1 << 20), 8 << 20), 2,
        lambda state: state.columnar_query(descs, blob_t, vals_t, nrows,
                                           keep),
        "columnar query overflowed after retry")


def coded_query(eng, query, filt, params, kinds, merged, timings=None):
    """GpuEngine.coded_query."""
    from ..index.columnar import FILE_COLUMN
    from ..points import Aggregator
    from ..query import QueryConfig
    clock = [time.perf_counter()]

    def mark(phase):
        if timings is None:
            return
        eng.torch.cuda.synchronize(eng.device)
        now = time.perf_counter()
        timings[phase] = timings.get(phase, 0.0) + now - clock[0]
        clock[0] = now

    # the file ordinal rides in a reserved trailing breakdown; the
    # decode query carries it too, so decode needs no change
    file_bd = {"name": FILE_COLUMN, "field": FILE_COLUMN,
               "aggr": "lquantize", "step": 1}
    cplan = column_plan(query, filt, extra=[file_bd])
    dq = QueryConfig(
        filter=None,
        breakdowns=[dict(b) for b in query.breakdowns] + [file_bd],
        allow_reserved=True)

    up = _uploader(eng)
    # (the file column's slot has no column: it stays missing)
    descs, keep = upload_columns(
        eng, cplan, params, kinds, lambda name, _ci: merged.nums[name],
        lambda name, _ci: (COL_CODED, merged.codes[name], None))
    blob, doff, dlen = merged.dictionary()
    # 16 bytes of slack: the text layer reads 8-byte words
    blob_t = up(np.frombuffer(blob + b"\0" * 16, dtype=np.uint8).copy())
    doff_t = up(doff, np.int32)
    dlen_t = up(dlen, np.int32)
    seg_t = up(merged.seg_start, np.int32)
    vals_t = up(merged.values)
    mark("h2d")

    def launch(state):
        state.coded_query(descs, blob_t, doff_t, dlen_t, seg_t, vals_t,
                          merged.nrows, keep)
        mark("kernels")

    agg = run_query(
        eng, cplan, dq,
        max(len(blob) * 2 + 8 * len(doff) + (1 << 20), 8 << 20), 4, launch,
        "coded query overflowed after retries", tally=eng.coded_stats)
    eng.coded_stats["launches"] += 1

    # split by file ordinal and strip it
    parts = [Aggregator(query) for _ in merged.members]
    for key, v in agg.table.items():
        t = parts[key[-1]].table
        t[key[:-1]] = t.get(key[:-1], 0) + v
    mark("decode")
    return parts

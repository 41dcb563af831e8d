"""
Host-side decode of a GPU scan's extraction snapshot: numpy in, the
canonical aggregate representation of the CPU oracle (points.Aggregator
and the pipeline counter stages) out.  No torch, no GPU: engine/gpu.py
copies the snapshot to the host and hands it over as a plain dict,

    cnt      int64 counters (slots below)
    n_str, n_num   ids handed out by the string / number dictionary
    str_off, str_len, blob   per string id, its span in the payload
                   bytes (needed only where n_str > 0)
    numbers  float64 per number id (needed only where n_num > 0)
    aggs     per metric (keys uint32-or-int32 [n, MAX_KEY], counts
             float64 [n]): the ready rows of its table
"""

import json

import numpy as np

from ..points import Aggregator
from . import plan as planmod

# device counter slots (ops/hip/common.h CounterSlot)
(C_LINES, C_INVALID_JSON, C_PARSED, C_DS_FILTERED, C_DS_FAILEDEVAL,
 C_OVERFLOW) = range(6)
C_GLOBAL_N = 8
CM_N = 8
(CM_FILTER_IN, CM_FILTERED, CM_FAILEDEVAL, CM_UNDEF, CM_BADDATE,
 CM_TIME_OUT, CM_AGG_IN, CM_NONNUMERIC) = range(8)


def decode_snapshot(host, queries, cplan):
    """-> (one Aggregator per query, counter stages)."""
    cnt = host["cnt"]
    strings, numbers = decode_dicts(host)
    aggs = []
    for m, q in enumerate(queries):
        k, c = host["aggs"][m]
        k = k.astype(np.uint32)
        agg = Aggregator(q)
        mc = cnt[C_GLOBAL_N + m * CM_N:
                 C_GLOBAL_N + (m + 1) * CM_N]
        agg.ninputs = int(mc[CM_AGG_IN])
        agg.ndropped_nonnumeric = int(mc[CM_NONNUMERIC])
        nk = len(q.breakdowns)
        for i in range(k.shape[0]):
            key = planmod.decode_key(k[i, :nk], q, strings, numbers)
            v = c[i]
            v = int(v) if float(v).is_integer() else float(v)
            # two ids may name one string (decode_dicts): such rows merge
            agg.table[key] = agg.table.get(key, 0) + v
        aggs.append(agg)

    stages = counter_stages(cnt, cplan, queries)
    for name, c in stages:
        if name == "Aggregator":
            c["noutputs"] = aggs[0].noutputs()
    return aggs, stages


def decode_dicts(host):
    """The dictionaries in id order: (strings list, numbers array).
    The list may name a string twice: two lanes interning it at the
    same moment can both insert it."""
    n_str = host["n_str"]
    strings = []
    if n_str:
        off = host["str_off"].astype(np.uint32)
        ln = host["str_len"].astype(np.uint32)
        blob = host["blob"].tobytes()
        for i in range(n_str):
            raw = blob[off[i]:off[i] + ln[i]]
            strings.append(decode_json_string(raw))
    numbers = np.zeros(0)
    if host["n_num"]:
        numbers = host["numbers"]
    return strings, numbers


def counter_stages(cnt, cp, queries):
    """Reconstruct the reference pipeline counter stages from the
    device counters (mirrors scan_cpu.ScanPipeline.counter_stages)."""
    parsed = int(cnt[C_PARSED])
    stages = [("json parser", {
        "ninputs": int(cnt[C_LINES]), "noutputs": parsed,
        "invalid json": int(cnt[C_INVALID_JSON])})]
    if cp.data_format == "json":
        stages.append(("SkinnerAdapterStream",
                       {"ninputs": parsed, "noutputs": parsed}))
    # program 0 is the ds filter; OP_TRUE means "no filter"
    progs, bounds = cp.programs
    if progs[bounds[0][0]][0] != planmod.OP_TRUE:
        out, err = int(cnt[C_DS_FILTERED]), int(cnt[C_DS_FAILEDEVAL])
        stages.append(("Datasource filter", {
            "ninputs": parsed, "noutputs": parsed - out - err,
            "nfilteredout": out, "nfailedeval": err}))
    # metric 0's pipeline (what the CLI displays for scans)
    q = queries[0]
    mc = cnt[C_GLOBAL_N:C_GLOBAL_N + CM_N]
    n = int(mc[CM_FILTER_IN])
    if q.filter is not None:
        out = n - int(mc[CM_FILTERED]) - int(mc[CM_FAILEDEVAL])
        stages.append(("User filter", {
            "ninputs": n, "noutputs": out,
            "nfilteredout": int(mc[CM_FILTERED]),
            "nfailedeval": int(mc[CM_FAILEDEVAL])}))
        n = out
    m0 = cp.metrics[0][0]
    if m0[planmod.M_NSYNTH] > 0:  # has synthetic requirements
        out = n - int(mc[CM_UNDEF]) - int(mc[CM_BADDATE])
        stages.append(("Datetime parser", {
            "ninputs": n, "noutputs": out,
            "undef": int(mc[CM_UNDEF]),
            "baddate": int(mc[CM_BADDATE])}))
        n = out
    if m0[planmod.M_HAS_TF]:  # time filter
        stages.append(("Time filter", {
            "ninputs": n, "noutputs": n - int(mc[CM_TIME_OUT]),
            "nfilteredout": int(mc[CM_TIME_OUT]),
            "nfailedeval": 0}))
    stages.append(("Aggregator", {
        "ninputs": int(mc[CM_AGG_IN]),
        "noutputs": 0,  # patched by caller if needed
        "nonnumeric": int(mc[CM_NONNUMERIC])}))
    return stages


def decode_json_string(raw):
    """Decode raw in-record string bytes (may contain JSON escapes)
    to the same Python string json.loads would produce."""
    try:
        s = raw.decode("utf-8")
    except UnicodeDecodeError:
        return raw.decode("utf-8", "replace")
    if "\\" in s:
        try:
            return json.loads('"' + s + '"')
        except ValueError:
            return s
    return s

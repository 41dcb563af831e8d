"""
The step after the multi-GPU gather: re-aggregate the ranks' tables.
Nothing here needs a process group; distributed.py does the collectives
and hands the gathered tensors to reaggregate().

  wire form: a rank's table is an int64 key-code matrix [n, nk], a tag
     column (2 bits per element: int / string-id / f64-bits) and an f64
     value vector (_encode_table); its string dictionary is a UTF-8 byte
     blob + offset array (_strings_blob).  The dictionary may name one
     string twice (two scan ids of one string, the constant null beside
     a literal "null", "a" beside "\\u0061") and the table may hold one
     key in two rows: every consumer unifies the dictionaries and
     regroups the rows first (reaggregate, _merge_partitioned).
  encode_table: an Aggregator to that form row by row on the host, or a
     scan's extraction snapshot to it on the device, where it lies: the
     encode_table kernels (ops/hip/encode_table.h); a WireTable either
     way.  DRAGNET_ENCODE_GPU chooses (encode_on_gpu).
  format_numbers: the key strings of the fractional and large numbers
     that export hands back, plan.number_key per value on the host or the
     format_numbers kernels (ops/hip/format_numbers.h) on the device;
     DRAGNET_FORMAT_GPU chooses.
  C2 unify_dictionaries: the global dictionary, first seen first in rank
     order, and per rank the table from its codes to global ones:
     FirstSeen on the host, or the unify_strings kernels
     (ops/hip/unify_strings.h) on the gathered blobs where they lie.
  C1 _group_rows: remap the string codes, group identical rows and sum
     their values: np.unique + bincount on the host, or the merge_rows
     kernels (ops/hip/merge_rows.h, ordered by sort_rows.h).
  partition_rows: the high-cardinality merge sends each row to the rank
     its hash names; remap, hash and a stable split by destination:
     numpy on the host, or the partition_rows kernels
     (ops/hip/partition_rows.h) with the remap table where unify left it.
  render_points: the receiving end.  The distinct rows, their sums and
     the global dictionary to the NDJSON point lines `dn scan --points`
     prints: _decode_rows, Aggregator.points() and output.point_json per
     row on the host, or, in the order sort_rows gives, the render_points
     kernels (ops/hip/render_points.h), no row becoming a Python object.
     reaggregate_points is reaggregate with that in place of
     _decode_rows; DRAGNET_RENDER_GPU chooses.
  rank_strings: what orders those lines by string, the rank of every
     dictionary string in byte order: one sorted() over the bytes on the
     host, or the rank_strings kernels (ops/hip/rank_strings.h) on the
     dictionary where it lies; DRAGNET_RANK_GPU chooses.
  parse_points / reduce_points: the reduce side.  Tagged NDJSON point
     lines (dn index-read's input) to rows by the parse_points kernels
     (ops/hip/parse_points.h), their string elements spans into the
     uploaded text, which unify_strings and merge_rows take as they are;
     what the device punts stays with the C++ reducer
     (points.reduce_tagged_stream; DRAGNET_PARSE_GPU chooses).
  DRAGNET_UNIFY_GPU, DRAGNET_MERGE_GPU and DRAGNET_PARTITION_GPU choose
  (_use_gpu); the host and device paths give the same bits.
"""

import os

import numpy as np

from .points import Aggregator

# per-element tag values in the packed tag column
_EL_INT = 0   # int64 payload (ordinals, dates, integral counts)
_EL_STR = 1   # payload = index into the rank's string dictionary
_EL_F64 = 2   # payload = IEEE-754 bits of a float key element


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


class WireTable(object):
    """One rank's table of one query in wire form: codes [n, nk],
    tagpack [n], vals [n] and the dictionary (blob, offs), numpy or
    torch on any device, with the scan's ninputs and
    ndropped_nonnumeric for that query."""

    __slots__ = ("codes", "tagpack", "vals", "strings", "ninputs",
                 "ndropped_nonnumeric")

    def __init__(self, codes, tagpack, vals, strings, ninputs=0,
                 ndropped_nonnumeric=0):
        self.codes, self.tagpack, self.vals = codes, tagpack, vals
        self.strings = strings
        self.ninputs = ninputs
        self.ndropped_nonnumeric = ndropped_nonnumeric


def col_kinds(query):
    """Per breakdown, what ops/hip/encode_table.h needs of it: 2 for a
    bucketized column, 1 for a date column without bucketizer, else 0."""
    return [2 if query.bucketizers.get(b["name"]) is not None
            else 1 if "date" in b else 0 for b in query.breakdowns]


def encode_on_gpu(n_rows, nk):
    """Path choice of the wire-form export: _use_gpu over
    DRAGNET_ENCODE_GPU and DRAGNET_ENCODE_GPU_ROWS rows of one table
    (infinity by default: profiles/r13_encode_table.md).  A table
    without breakdowns is a scalar and stays on the host."""
    return nk >= 1 and _use_gpu("DRAGNET_ENCODE_GPU",
                                "DRAGNET_ENCODE_GPU_ROWS", n_rows)


def _encode_device(snap, metric, query):
    """The encode_table kernels (ops/hip/encode_table.h) on metric
    `metric` of an extraction snapshot (ScanState.extract_all's dict of
    device tensors): (codes, tagpack, vals, (blob, offs)) on the
    device, row i being extraction row i, or None where the kernels
    refuse (NaN or an infinity in an integer column: the host path
    raises there).  The device renders plain strings, integral numbers
    and the constants; the E exceptions it hands back (escaped or
    ill-formed strings, array texts, other numbers) are rendered here,
    once per distinct value, and appended to the dictionary in the order
    their codes assume: strings and array texts by the host path's own
    functions, the numbers by format_numbers."""
    import torch

    from .engine.decode import decode_json_string
    from .engine.plan import array_key
    from .ops import load_ops
    ops = load_ops(required=True)  # a missing extension is an error
    keys, counts, n = snap["aggs"][metric]
    (codes, tagpack, vals, blob, offs, exc_kind, _exc_id, exc_blob,
     exc_offs, refused) = ops.encode_table(
        keys, counts, n, snap["str_off"], snap["str_len"], snap["n_str"],
        snap["blob"], snap["used"], snap["numbers"], snap["n_num"],
        col_kinds(query))
    if refused:
        return None
    if exc_kind.numel():
        # ordered by (kind, id): strings and array texts, then the numbers
        kinds = exc_kind.cpu().tolist()
        head = len(kinds) - kinds.count(2)
        at = exc_offs[:head + 1].cpu().tolist()
        raw = exc_blob[:at[head]].cpu().numpy().tobytes()
        extra = []
        for kind, a, b in zip(kinds, at, at[1:]):
            s = decode_json_string(raw[a:b])
            if kind == 1:
                s = array_key(s)
            extra.append(s.encode("utf-8"))
        # the tail is 8 bytes a number; format_numbers keeps it on the
        # device where DRAGNET_FORMAT_GPU says so
        nums = exc_blob[at[head]:].clone().view(torch.float64)
        num_blob, num_offs = format_numbers(nums, blob.device)
        ends = np.cumsum([len(e) for e in extra]).astype(np.int64)
        dev = blob.device
        parts = [blob, torch.from_numpy(np.frombuffer(
            b"".join(extra), dtype=np.uint8).copy()).to(dev),
            torch.as_tensor(num_blob).to(dev)]
        mid = offs[-1] + (int(ends[-1]) if head else 0)
        offs = torch.cat([offs, offs[-1] + torch.from_numpy(ends).to(dev),
                          mid + torch.as_tensor(num_offs).to(dev)[1:]])
        blob = torch.cat(parts)
    return codes, tagpack, vals, (blob, offs)


def format_numbers(values, device=None):
    """The key strings of numbers in a plain column, JS String(number),
    as a dictionary in wire form: (blob uint8, offs int64 [n + 1]) for
    f64 `values`, numpy or torch on any device.  On the host it is
    plan.number_key per value and _strings_blob (numpy out), which is
    the definition; on the GPU the format_numbers kernels
    (ops/hip/format_numbers.h) give the same bytes and nothing leaves
    the device.  DRAGNET_FORMAT_GPU and DRAGNET_FORMAT_GPU_NUMBERS
    numbers choose (_use_gpu; infinity by default:
    profiles/r17_format_numbers.md)."""
    n = int(np.prod(values.shape))
    if _use_gpu("DRAGNET_FORMAT_GPU", "DRAGNET_FORMAT_GPU_NUMBERS", n):
        import torch

        from .ops import load_ops
        ops = load_ops(required=True)  # a missing extension is an error
        device, up = _work_device(device, [values])
        return ops.format_numbers(
            up(values, torch.float64).reshape(-1).contiguous())
    from .engine.plan import number_key
    blob, offs = _strings_blob(
        [number_key(v) for v in _np(values).reshape(-1).astype(np.float64)])
    return np.frombuffer(blob, dtype=np.uint8).copy(), offs


def encode_table(source, query, metric=0):
    """A table to the wire form, a WireTable.  An Aggregator goes
    through the host form, _encode_table and _strings_blob (numpy
    out).  An extraction snapshot (ScanState.extract_all's dict) goes
    through the encode_table kernels for its metric `metric` (device
    tensors out) and never becomes Python objects; None where the
    kernels refuse, and the caller decodes the snapshot on the host.
    Callers choose by encode_on_gpu.  Both describe the same table: the
    device form keeps the extraction's rows and may name one string
    twice, which every consumer unifies and regroups."""
    nk = len(query.breakdowns)
    if isinstance(source, Aggregator):
        codes, tagpack, vals, strings = _encode_table(source, nk)
        blob, offs = _strings_blob(strings)
        return WireTable(codes, tagpack, vals,
                         (np.frombuffer(blob, dtype=np.uint8).copy(), offs),
                         source.ninputs, source.ndropped_nonnumeric)
    out = _encode_device(source, metric, query)
    return None if out is None else WireTable(*out)


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


# ---- what the host and device paths share ------------------------------

def _use_gpu(mode_var, threshold_var, count):
    """The path policy of the device steps.  Mode "0": never the GPU;
    "1": whenever one is visible; anything else ("auto", the default):
    from `threshold_var` items up, where unset or unparsable means
    infinity: auto then never selects it.  No items: the host."""
    mode = os.environ.get(mode_var, "auto")
    if mode == "0" or count == 0:
        return False
    if mode != "1":
        try:
            threshold = int(os.environ[threshold_var])
        except (KeyError, ValueError):
            threshold = float("inf")
        if count < threshold:
            return False
    import torch
    return torch.cuda.is_available()


def _np(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def _work_device(device, inputs):
    """(device, up): the CUDA device a device step works on (`device`
    if it is one, else that of the first input already on a GPU, else
    the current one) and up(a, dtype), which puts an array or tensor
    there.  Inputs already on it are not copied."""
    import torch
    if device is None or torch.device(device).type != "cuda":
        on_gpu = [t.device for t in inputs
                  if torch.is_tensor(t) and t.is_cuda]
        device = on_gpu[0] if on_gpu else torch.device(
            "cuda", torch.cuda.current_device())

    def up(a, dtype):
        return torch.as_tensor(a).to(device=device, dtype=dtype)

    return device, up


class FirstSeen:
    """Numbers byte strings in order of first occurrence: the host form
    of ops/hip/unify_strings.h.  `values` is the running dictionary."""

    def __init__(self):
        self.values = []
        self._where = {}

    def ids(self, items):
        """int64 ids of items (bytes each); the unseen ones are appended
        to the dictionary in order."""
        where, values = self._where, self.values
        out = np.empty(len(items), dtype=np.int64)
        for i, v in enumerate(items):
            g = where.get(v)
            if g is None:
                g = where[v] = len(values)
                values.append(v)
            out[i] = g
        return out


# ---- row grouping (C1) ---------------------------------------------------

def _merge_on_gpu(n_rows, nk):
    """Path choice of the row grouping: _use_gpu over DRAGNET_MERGE_GPU
    and DRAGNET_MERGE_GPU_ROWS total rows.  profiles/r08_merge_rows.md
    measured no size that wins at every cardinality, hence infinity;
    with the rows ordered on the device (profiles/r09_sort_rows.md) the
    same rule gives 10000, and the default is unchanged so far.  A table
    without breakdowns is a scalar sum and stays on the host."""
    return nk >= 1 and _use_gpu("DRAGNET_MERGE_GPU",
                                "DRAGNET_MERGE_GPU_ROWS", n_rows)


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


def _group_rows_device(parts, remaps, nk, device, keep=False):
    """One merge_rows call over the parts as segments; the remap runs
    inside the kernel.  Parts already on the GPU are never copied to
    the host; only the distinct rows and their sums come back, already
    in np.unique's order (lexicographic over the columns left to right,
    as signed int64: the radix sort of ops/hip/sort_rows.h, behind
    merge_rows' sort=True); with keep they stay device tensors, for
    render_points.  None when the kernel reports sums that depend on
    the order of its adds."""
    import torch

    from .ops import load_ops
    ops = load_ops(required=True)  # a missing extension is an error
    device, up = _work_device(device, [p[0] for p in parts])
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
    if keep:
        return uniq, sums
    return uniq.cpu().numpy(), sums.cpu().numpy()


def _group_rows(parts, remaps, nk, device=None, keep=False):
    """Group the rows [codes..., tagpack] of all parts and sum their
    values: (uniq [g, nk + 1], sums [g]) in np.unique's order.  remaps
    is one int64 table per part for its string-tagged codes, or None.

    The result is bit-identical whichever path runs.  Device f64 adds
    come in no fixed order, and only sums of non-negative integers that
    stay below 2^53 are independent of the order, so the kernel reports
    anything else (a fractional, negative, NaN or infinite weight, a
    value or a sum at or beyond 2^53) and the host path then answers.
    With keep the device path leaves both on the device."""
    n_rows = sum(int(p[1].shape[0]) for p in parts)
    out = None
    if _merge_on_gpu(n_rows, nk):
        out = _group_rows_device(parts, remaps, nk, device, keep)
    if out is None:
        out = _group_rows_host(parts, remaps, nk)
    return out


# ---- dictionary unification (C2) ----------------------------------------

def _is_blob_pair(d):
    return isinstance(d, tuple) and len(d) == 2 and hasattr(d[0], "dtype")


def _unify_on_gpu(dicts, n_strings):
    """Path choice of the dictionary unification: _use_gpu over
    DRAGNET_UNIFY_GPU and DRAGNET_UNIFY_GPU_STRINGS total strings
    (infinity by default: profiles/r10_unify_strings.md).  Dictionaries
    that arrive as Python strings are on the host already and stay
    there."""
    return all(_is_blob_pair(d) for d in dicts) and _use_gpu(
        "DRAGNET_UNIFY_GPU", "DRAGNET_UNIFY_GPU_STRINGS", n_strings)


def _unify_host(dicts, as_blob=False):
    """FirstSeen over the strings' UTF-8 bytes (the encoding is
    one-to-one): the reference the device path must equal.  Wire-form
    entries are sliced, not decoded; only the distinct strings are, and
    with as_blob not even those: they come back as (blob, offs)."""
    seen = FirstSeen()
    remaps = []
    for d in dicts:
        if _is_blob_pair(d):
            blob, offs = _np(d[0]).tobytes(), _np(d[1]).tolist()
            items = [blob[a:b] for a, b in zip(offs, offs[1:])]
        else:
            items = [s.encode("utf-8") for s in d]
        remaps.append(seen.ids(items))
    if as_blob:
        offs = np.zeros(len(seen.values) + 1, dtype=np.int64)
        np.cumsum([len(b) for b in seen.values], out=offs[1:])
        blob = np.frombuffer(b"".join(seen.values), dtype=np.uint8).copy()
        return (blob, offs), remaps
    return [b.decode("utf-8") for b in seen.values], remaps


def _unify_device(dicts, device, as_blob=False):
    """One unify_strings call (ops/hip/unify_strings.h) over the blobs
    as one blob.  Blobs already on the GPU are never copied to the host;
    the remap tables stay on the device, and only the bytes of the G
    first occurrences come back, to be decoded into gstrings; with
    as_blob they stay where they are packed, as (blob, offs)."""
    import torch

    from .ops import load_ops
    ops = load_ops(required=True)  # a missing extension is an error
    device, up = _work_device(device, [d[0] for d in dicts])
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
    if as_blob:
        return (packed, torch.cat([fend.new_zeros(1), fend])), remaps
    return _decode_strings(packed.cpu().numpy().tobytes(), goffs), remaps


def unify_dictionaries(dicts, device=None):
    """C2: one global dictionary out of the per-rank ones.  Each entry
    of dicts is a list of str, or the wire form (blob uint8 [bytes],
    offs int64 [n_r + 1]), numpy or torch on any device.  Returns
    (gstrings, remaps): the distinct strings, first seen first in rank
    order, and per rank the int64 table from its codes to indices of
    gstrings.  On the host this is FirstSeen over the strings' bytes;
    on the GPU (DRAGNET_UNIFY_GPU, wire-form entries only) the
    unify_strings kernels number the spans where the gather left them
    and the remaps stay device tensors for merge_rows.  Either way only
    the distinct strings are decoded, and both give the same result."""
    return _unify(dicts, device)


def _unify(dicts, device, as_blob=False):
    """unify_dictionaries; with as_blob the distinct strings come back
    in wire form, (blob, offs), where the path that ran leaves them."""
    n_strings = sum(max(len(d[1]) - 1, 0) if _is_blob_pair(d) else len(d)
                    for d in dicts)
    if _unify_on_gpu(dicts, n_strings):
        return _unify_device(dicts, device, as_blob)
    return _unify_host(dicts, as_blob)


# ---- partition by destination rank ---------------------------------------

_PARTITION_MAX_WORLD = 256  # ops/hip/partition_rows.h: a thread per bin


def _partition_host(codes, tagpack, vals, remap, world):
    """Remap, hash, stable argsort by hash % world: the reference the
    device path must equal bit for bit."""
    tagpack = _np(tagpack).astype(np.int64, copy=False)
    codes = _np(codes).astype(np.int64, copy=True)  # the caller's stay
    vals = _np(vals).astype(np.float64, copy=False)
    nk = codes.shape[1]
    if remap is not None:
        remap = _np(remap)  # a device slice after a GPU unify
        for j in range(nk):
            is_str = ((tagpack >> (2 * j)) & 3) == _EL_STR
            if is_str.any():
                codes[is_str, j] = remap[codes[is_str, j]]
    h = np.zeros(codes.shape[0], dtype=np.uint64)
    for j in range(nk):
        cj = np.ascontiguousarray(codes[:, j]).view(np.uint64)
        h = (h ^ cj) * np.uint64(0x100000001B3)
    h ^= tagpack.view(np.uint64)
    part = (h % np.uint64(world)).astype(np.int64)
    order = np.argsort(part, kind="stable")
    counts = np.bincount(part, minlength=world)
    wire = np.concatenate(
        [codes, tagpack[:, None], vals.view(np.int64)[:, None]],
        axis=1)[order]
    return wire, counts


def _partition_device(codes, tagpack, vals, remap, world, device):
    """One partition_rows call; the remap table is used where it lies
    and the wire rows and counts stay on the device."""
    import torch

    from .ops import load_ops
    ops = load_ops(required=True)  # a missing extension is an error
    device, up = _work_device(device, [codes, remap])
    rows = torch.cat([up(codes, torch.int64),
                      up(tagpack, torch.int64).reshape(-1, 1)], dim=1)
    return ops.partition_rows(
        rows, up(vals, torch.float64), rows.shape[1] - 1, world,
        remap=None if remap is None else up(remap, torch.int64))


def partition_rows(codes, tagpack, vals, remap, world, device=None):
    """Split one rank's table by the rank that will merge each row.
    codes [n, nk], tagpack [n] and vals [n] are numpy or torch on any
    device; remap is the int64 table of this rank's string-tagged codes
    (unify_dictionaries), numpy or a device tensor, or None.  Row i,
    after the remap, goes to rank hash(row i) % world.  Returns (wire
    int64 [n, nk + 2], counts int64 [world]): the remapped codes, the
    tag pack and the bits of the value of every row, grouped by
    destination in rank order, input order kept within a group, and
    the rows per destination.

    The host path (numpy arrays out) is the stable argsort; the device
    path (tensors on the GPU out) is the partition_rows kernels.
    DRAGNET_PARTITION_GPU and DRAGNET_PARTITION_GPU_ROWS choose
    (_use_gpu; infinity by default: profiles/r12_partition_rows.md);
    more than 256 ranks, or a table without breakdowns, stay on the
    host.  Both give the same bits."""
    n, nk = codes.shape
    if nk >= 1 and world <= _PARTITION_MAX_WORLD and _use_gpu(
            "DRAGNET_PARTITION_GPU", "DRAGNET_PARTITION_GPU_ROWS", n):
        return _partition_device(codes, tagpack, vals, remap, world, device)
    return _partition_host(codes, tagpack, vals, remap, world)


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


# ---- the receiving end: rows to point lines -------------------------------

def _points_bytes(agg):
    """An Aggregator's points as NDJSON, json.dumps per point: what
    output.output_points writes."""
    from .output import point_json
    return "".join(point_json(p) + "\n" for p in agg.points()).encode()


def _render_host(query, uniq, sums, strings):
    """_decode_rows, Aggregator.points() and output.point_json per row:
    the definition the device path must equal byte for byte."""
    if _is_blob_pair(strings):
        strings = _decode_strings(_np(strings[0]).tobytes(),
                                  _np(strings[1]).tolist())
    return _points_bytes(_decode_rows(query, _np(uniq), _np(sums), strings))


def _rank_host(strings):
    """The ranks on the host: the G byte strings as slices, a set to see
    whether one occurs twice, one C-level sort.  The reference the device
    path must equal."""
    if _is_blob_pair(strings):
        raw, at = _np(strings[0]).tobytes(), _np(strings[1]).tolist()
        items = [raw[a:b] for a, b in zip(at, at[1:])]
    else:
        items = [s.encode("utf-8") for s in strings]
    n_str = len(items)
    if len(set(items)) != n_str:
        return None
    rank = np.empty(n_str, dtype=np.int64)
    rank[sorted(range(n_str), key=items.__getitem__)] = np.arange(n_str)
    return rank


def _rank_device(strings, device):
    """One rank_strings call (ops/hip/rank_strings.h) on the dictionary
    where it lies; the ranks stay on the device."""
    import torch

    from .ops import load_ops
    ops = load_ops(required=True)  # a missing extension is an error
    if not _is_blob_pair(strings):
        blob, offs = _strings_blob(strings)
        strings = np.frombuffer(blob, dtype=np.uint8).copy(), offs
    device, up = _work_device(device, list(strings))
    rank, twice = ops.rank_strings(
        up(strings[0], torch.uint8).reshape(-1).contiguous(),
        up(strings[1], torch.int64).reshape(-1).contiguous())
    return None if twice else rank


def rank_strings(strings, device=None):
    """The rank of every dictionary string in byte order, which for UTF-8
    is code point order, Aggregator.points()'s: int64 [G], rank[i] = the
    number of strings smaller than string i; None when a string occurs
    twice.  strings is a list of str or a (blob, offs) pair, numpy or
    torch on any device.  On the host (_rank_host) the result is numpy;
    on the GPU (_rank_device, the rank_strings kernels) no dictionary
    byte leaves the device and the ranks stay there.
    DRAGNET_RANK_GPU and DRAGNET_RANK_GPU_STRINGS strings choose
    (_use_gpu; infinity by default: profiles/r15_rank_strings.md)."""
    n_str = max(len(strings[1]) - 1, 0) if _is_blob_pair(strings) \
        else len(strings)
    if _use_gpu("DRAGNET_RANK_GPU", "DRAGNET_RANK_GPU_STRINGS", n_str):
        return _rank_device(strings, device)
    return _rank_host(strings)


def _render_device(query, uniq, sums, strings, device):
    """The render_points kernels (ops/hip/render_points.h) on the rows
    where they lie: the NDJSON bytes, or None where the table is one
    only the host renders (rows of different tag packs, an F64 tag,
    numbers beyond int64, a fractional sum, two breakdowns of one name,
    one string twice in the dictionary).

    Line order is Aggregator.points()'s: integers by value, strings by
    code point, which is UTF-8 byte order.  rank_strings gives the rank
    of each dictionary string in that order, on the host or by the
    rank_strings kernels; a device gather puts the ranks in place of the
    codes of the string columns and sort_rows orders those nk columns."""
    import json

    import torch

    from .ops import load_ops
    from .points import fast_reduce_spec
    ops = load_ops(required=True)  # a missing extension is an error
    nk = len(query.breakdowns)
    spec = fast_reduce_spec(query)
    names = [name for name, _kind, _step in spec]
    if len(set(names)) != nk:
        return None
    device, up = _work_device(device, [uniq, sums])
    rows = up(uniq, torch.int64).contiguous()
    tags = rows[:, nk]
    tp = int(tags[0])
    if bool((tags != tp).any()):
        return None
    el = [(tp >> (2 * j)) & 3 for j in range(nk)]
    if any(e not in (_EL_INT, _EL_STR) for e in el):
        return None
    keys = rows[:, :nk].contiguous()
    if _EL_STR in el:
        if _is_blob_pair(strings):
            blob, offs = strings
        else:
            blob, offs = _strings_blob(strings)
            blob = np.frombuffer(blob, dtype=np.uint8).copy()
        n_str = max(len(offs) - 1, 0)
        rank = rank_strings((blob, offs), device)
        if rank is None:
            return None
        if n_str:  # none: every code is out of range, and the op says so
            rank = up(rank, torch.int64)
            for j in range(nk):
                if el[j] == _EL_STR:  # a bad code is the op's to report
                    keys[:, j] = rank[keys[:, j].clamp(0, n_str - 1)]
    else:
        blob, offs = np.zeros(0, np.uint8), np.zeros(1, np.int64)
    order = ops.sort_rows(keys)
    segs = ['{"fields":{' + json.dumps(names[0]) + ":"]
    segs += ["," + json.dumps(name) + ":" for name in names[1:]]
    segs += ['},"value":', "}\n"]
    segs = [t.encode() for t in segs]
    seg_offs = np.concatenate([[0], np.cumsum([len(t) for t in segs])])
    text, _line_off, refused = ops.render_points(
        rows, up(sums, torch.float64).contiguous(), order,
        up(blob, torch.uint8).reshape(-1).contiguous(),
        up(offs, torch.int64).reshape(-1).contiguous(),
        [kind for _name, kind, _step in spec],
        [int(step) for _name, _kind, step in spec],
        up(np.frombuffer(b"".join(segs), dtype=np.uint8).copy(), torch.uint8),
        up(seg_offs, torch.int64))
    return None if refused else text.cpu().numpy().tobytes()


def render_points(query, uniq, sums, strings, device=None):
    """The receiving end's one seam: distinct rows uniq [g, nk + 1]
    (key codes, then the tag pack) and their sums [g] as _group_rows
    returns them, numpy or torch on any device, and the dictionary the
    string codes index, a list of str or a (blob, offs) pair, to the
    NDJSON bytes output_points(agg.points()) writes for the Aggregator
    _decode_rows builds from them.

    The host path builds exactly that (_render_host); the device path is
    the render_points kernels (_render_device) and gives the same bytes,
    or hands a table it cannot render to the host path whole.
    DRAGNET_RENDER_GPU and DRAGNET_RENDER_GPU_ROWS distinct rows choose
    (_use_gpu; infinity by default: profiles/r14_render_points.md).  A
    table without breakdowns is one scalar and stays on the host."""
    nk = len(query.breakdowns)
    g = int(uniq.shape[0])
    out = None
    if nk >= 1 and _use_gpu("DRAGNET_RENDER_GPU", "DRAGNET_RENDER_GPU_ROWS",
                            g):
        out = _render_device(query, uniq, sums, strings, device)
    if out is None:
        out = _render_host(query, uniq, sums, strings)
    return out


def reaggregate_points(query, parts, strings_per_part, device=None):
    """reaggregate with render_points in place of _decode_rows: the
    merged table as NDJSON bytes, one point per line, in
    Aggregator.points()'s order.  Where the group step and the render
    step both run on the device the distinct rows and their sums stay
    there between them, and the global dictionary stays in wire form
    wherever unify_dictionaries left it."""
    nk = len(query.breakdowns)
    if nk == 0:
        vals = [_np(v).astype(np.float64, copy=False)
                for _c, _t, v in parts]
        return _points_bytes(_scalar_table(
            query, np.concatenate(vals) if vals else np.zeros(0)))
    gstrings, remaps = _unify(strings_per_part, device, as_blob=True)
    uniq, sums = _group_rows(parts, remaps, nk, device, keep=True)
    return render_points(query, uniq, sums, gstrings, device)


# ---- the reduce side: point lines back to rows ----------------------------

# caps of ops/hip/parse_points.h; beyond them the op is not called
_PARSE_MAX_METRICS = 8
_PARSE_MAX_KEY = 8
_PARSE_NAME_BYTES = 2048
_PARSE_TAIL = b"undefined"
PARSE_SKIP, PARSE_DROP, PARSE_TAKEN, PARSE_PUNT = 0, 1, 2, 3


def _parse_specs(queries):
    """The metrics' columns as ops.parse_points takes them, (ncols,
    kinds, steps, names, name_offs), or None where its caps do not hold:
    too many metrics or columns, too many name bytes, or an lquantize
    step that is zero or not a double (the device divides doubles)."""
    from .points import fast_reduce_spec
    if not 1 <= len(queries) <= _PARSE_MAX_METRICS:
        return None
    ncols, kinds, steps, names = [], [], [], []
    for q in queries:
        spec = fast_reduce_spec(q)
        if len(spec) > _PARSE_MAX_KEY:
            return None
        ncols.append(len(spec))
        for name, kind, step in spec:
            if kind == 3:
                exact = q.bucketizers[name].step
                if exact == 0 or step != exact:
                    return None
            try:
                names.append(name.encode("utf-8"))
            except UnicodeEncodeError:
                return None
            kinds.append(kind)
            steps.append(step)
    offs = [0]
    for n in names:
        offs.append(offs[-1] + len(n))
    if offs[-1] > _PARSE_NAME_BYTES:
        return None
    return ncols, kinds, steps, b"".join(names), offs


_parse_pinned = None  # the upload's staging buffer, grown as needed


def _parse_upload(data, device):
    """`data` and the tail as one uint8 tensor on the device, through a
    pinned host buffer that is kept between calls (a 64 MiB chunk per
    call is the stream's rhythm).  The copy has landed on return."""
    global _parse_pinned
    import torch
    n = len(data) + len(_PARSE_TAIL)
    if _parse_pinned is None or _parse_pinned.numel() < n:
        _parse_pinned = torch.empty(max(n, 1 << 16), dtype=torch.uint8,
                                    pin_memory=True)
    stage = _parse_pinned.numpy()
    stage[:len(data)] = np.frombuffer(data, dtype=np.uint8)
    stage[len(data):n] = np.frombuffer(_PARSE_TAIL, dtype=np.uint8)
    return _parse_pinned[:n].to(device)


def parse_points(data, queries, device=None):
    """The parse_points kernels (ops/hip/parse_points.h) over `data`,
    tagged NDJSON point lines as `dn index-scan` writes them: uploads
    the bytes with the constant `undefined` behind them and returns
    (tables, counters, punted, classes), or None where the op's caps do
    not hold (_parse_specs; 2^31 bytes).  tables: per metric a WireTable
    of the taken lines in line order, on the device, whose dictionary
    is the span form (text, start, length): a string element indexes
    the spans, which point into the uploaded text, one numbering for
    all metrics.  counters: int64 [M, 2] on the host, ninputs and
    nonnumeric.  punted: the lines left to the host reducer, as bytes.
    classes: uint8 per line on the device (PARSE_*)."""
    from .ops import load_ops
    ops = load_ops(required=True)  # a missing extension is an error
    specs = _parse_specs(queries)
    if specs is None or len(data) >= (1 << 31) - len(_PARSE_TAIL):
        return None
    device, _up = _work_device(device, [])
    text = _parse_upload(data, device)
    (metric, rows, span_start, span_len, vals, counters, punts,
     classes) = ops.parse_points(text, len(data), *specs)
    counters = counters.cpu().numpy()
    kmax = rows.shape[1] - 1
    tables = []
    for m, nk in enumerate(specs[0]):
        if len(specs[0]) == 1:
            mine, mvals = rows, vals
        else:
            mask = metric == m
            mine, mvals = rows[mask], vals[mask]
        tables.append(WireTable(
            mine[:, :nk], mine[:, kmax], mvals,
            (text, span_start, span_len),
            int(counters[m, 0]), int(counters[m, 1])))
    punted = [bytes(data[a:b]) for a, b in punts.cpu().tolist()]
    return tables, counters, punted, classes


def reduce_points(data, aggs, queries, device=None):
    """One chunk of a tagged point stream into `aggs`, on the device:
    parse_points, one unify_strings call over all spans, merge_rows per
    metric with the remap in place (a metric without breakdowns is an
    int64 sum), _decode_rows over the distinct rows with only the
    distinct strings decoded, and the result added into aggs exactly as
    points.reduce_tagged_stream's run() does.  Returns the punted lines,
    for the host reducer; None, with nothing committed, where the op's
    caps do not hold or merge_rows reports sums that are not exact (a
    sum at or beyond 2^53): the whole chunk is the host reducer's."""
    import torch

    from .ops import load_ops
    ops = load_ops(required=True)  # a missing extension is an error
    parsed = parse_points(data, queries, device)
    if parsed is None:
        return None
    tables, _counters, punted, _classes = parsed
    text, span_start, span_len = tables[0].strings
    strings, remap = [], None
    if span_start.numel():
        remap, first = ops.unify_strings(text, span_start, span_len)
        end = len(data)  # the distinct strings, from the host's copy
        strings = [
            (data[a:a + n] if a < end else _PARSE_TAIL).decode("utf-8")
            for a, n in zip(span_start[first].cpu().tolist(),
                            span_len[first].cpu().tolist())]
    else:
        remap = torch.zeros(0, dtype=torch.int64, device=text.device)
    merged = []
    for q, wt in zip(queries, tables):
        nk = len(q.breakdowns)
        n = int(wt.vals.shape[0])
        if n == 0:
            merged.append(None)
        elif nk == 0:
            # below 2^62 the f64 total tells that the int64 one is exact
            if float(wt.vals.sum()) >= 2.0 ** 62:
                return None
            merged.append({(): int(wt.vals.to(torch.int64).sum())})
        else:
            rows = torch.cat([wt.codes, wt.tagpack.reshape(-1, 1)],
                             dim=1).contiguous()
            uniq, sums, exact = ops.merge_rows(
                rows, wt.vals.contiguous(), nk,
                seg_start=torch.tensor([0, n]), remap=remap,
                remap_off=torch.tensor([0, int(remap.numel())]))
            if not exact:
                return None
            merged.append(_decode_rows(q, uniq.cpu().numpy(),
                                       sums.cpu().numpy(), strings).table)
    for agg, wt, t in zip(aggs, tables, merged):
        agg.ninputs += wt.ninputs
        agg.ndropped_nonnumeric += wt.ndropped_nonnumeric
        tab = agg.table
        for k, v in (t or {}).items():
            tab[k] = tab.get(k, 0) + v
    return punted

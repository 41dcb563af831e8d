"""
MI355X GPU scan engine — host orchestration.

Streams NDJSON bytes through the fused CDNA4 scan kernel
(ops/hip/scan_kernels.hip): chunked reads into pinned host buffers,
async H2D on the current HIP stream, torch-side newline indexing, one
fused kernel launch per chunk, then table/dictionary extraction and
host-side decode (engine/decode.py) into the same canonical aggregate
representation the CPU oracle produces (points.Aggregator) — so every
downstream consumer (formatters, index sink, RCCL merge) is
engine-agnostic.  File scans take their chunks from the host-only
framer in engine/chunks.py.  The tables, dictionaries and counters
belong to the extension's ScanState, which allocates and grows them.
Index queries over stored columns (ops/hip/scan_columns.h) are driven
from engine/colquery.py.

Capacity handling: the hash tables and dictionaries are sized up front,
as a first guess.  A scan of regular files restarts on overflow
(C_OVERFLOW counter) with 8x the capacity (aggregation is a pure
function of the input, so a restart is correct).  A scan that cannot
be read twice (byte source, pipe, device) — or any scan under
DRAGNET_GROW=1 — is growable instead: engine/capacity.py plans every
launch so that nothing can overflow, and a structure that is about to
fill is rehashed into a larger one on the device between two launches
(ScanState.grow_*); nothing is lost or read again.
"""

import os
import stat
from types import SimpleNamespace

import numpy as np

from . import capacity, decode, xpose
from . import plan as planmod
from .chunks import _pad, choose_chunk_bytes, frame_files
from .decode import (  # noqa: F401  (the counter slots, for importers)
    C_DS_FAILEDEVAL, C_DS_FILTERED, C_GLOBAL_N, C_INVALID_JSON, C_LINES,
    C_OVERFLOW, C_PARSED, CM_AGG_IN, CM_BADDATE, CM_FAILEDEVAL,
    CM_FILTER_IN, CM_FILTERED, CM_N, CM_NONNUMERIC, CM_TIME_OUT, CM_UNDEF)
from .xpose import _build_xpose_layout  # noqa: F401  (its earlier home)


def _env_int(name, default):
    try:
        return int(os.environ.get(name, default))
    except ValueError:
        return default


def first_guess_slots():
    """(aggregation, dictionary) table slots a scan or an index query
    starts with; an overflow multiplies them."""
    return (_env_int("DRAGNET_AGG_SLOTS", 1 << 20),
            _env_int("DRAGNET_DICT_SLOTS", 1 << 20))


def _is_regular(path):
    """A path that cannot be stat'ed counts as not regular."""
    try:
        return stat.S_ISREG(os.stat(path).st_mode)
    except OSError:
        return False


class GpuEngine(object):
    name = "gpu"

    def __init__(self, device=None):
        import torch
        self.torch = torch
        if not torch.cuda.is_available():
            raise RuntimeError("no GPU visible (torch.cuda unavailable)")
        from ..ops import load_ops
        self.ops = load_ops(required=True)
        self.device = device if device is not None else \
            torch.device("cuda", torch.cuda.current_device())
        self.chunk_bytes = _env_int("DRAGNET_CHUNK_MB", 256) * 1024 * 1024
        # coded_query's tally: launch groups answered, overflow retries
        self.coded_stats = {"launches": 0, "retries": 0}
        # chunk addressing is uint32 on-device: offsets/positions must
        # fit 4 GiB per chunk (arbitrarily large INPUTS stream through
        # many chunks; only a single RECORD larger than the chunk is
        # rejected, at scan time)
        if self.chunk_bytes > (3 << 30):
            raise ValueError(
                "DRAGNET_CHUNK_MB too large: device chunk addressing "
                "is 32-bit (max 3072 MB per chunk)")

    # ---- public engine interface ----

    def scan(self, files, queries, ds_filter=None, time_field=None,
             data_format="json", byte_source=None):
        from ..datasource.file import ScanResult

        cplan = planmod.compile_plan(
            queries, ds_filter=ds_filter, time_field=time_field,
            data_format=data_format)

        agg_slots, dict_slots = first_guess_slots()
        dict_data = _env_int("DRAGNET_DICT_DATA_MB", 256) * 1024 * 1024

        # Input that cannot be read twice cannot restart: it scans once,
        # growable, and never risks the dense directory (its capacity
        # bounds key cardinality).  DRAGNET_GROW=1 opts regular files in.
        if (byte_source is not None or _env_int("DRAGNET_GROW", 0) == 1
                or not all(_is_regular(p) for p in files)):
            ctx = _ScanContext(self, cplan, agg_slots, dict_slots,
                               dict_data, dense=False, growable=True)
            if byte_source is not None:
                for chunk in byte_source:
                    ctx.feed(chunk)
                ctx.flush()
            else:
                ctx.scan_files(files)
            if ctx.overflowed():
                # safety net (a pathological probe chain): never a
                # partial aggregate
                raise RuntimeError(
                    "table overflow on non-restartable byte source")
            aggs, stages = ctx.finalize(queries)
            return ScanResult(aggs, stages, gpu_stats=dict(
                ctx.planner.grow_counts(), restarts=0))

        dense = None
        nogrow = {"agg": [0] * len(queries), "sdict": 0, "sdata": 0,
                  "ndict": 0}
        for attempt in range(4):
            ctx = _ScanContext(self, cplan, agg_slots, dict_slots,
                               dict_data, dense=dense)
            ctx.scan_files(files)
            if ctx.overflowed():
                from ..log import get_logger
                if ctx.dense:
                    # dense directory overflowed (high cardinality):
                    # restart on the atomic hash path at full size
                    get_logger().child("gpu-engine").warn(
                        "dense directory overflow; restarting on the "
                        "hash path", agg_slots=agg_slots)
                    dense = False
                    continue
                get_logger().child("gpu-engine").warn(
                    "aggregation table overflow; restarting scan",
                    agg_slots=agg_slots * 8, dict_slots=dict_slots * 8)
                dense = False
                agg_slots *= 8
                dict_slots *= 8
                dict_data *= 4
                continue
            aggs, stages = ctx.finalize(queries)
            return ScanResult(aggs, stages,
                              gpu_stats=dict(nogrow, restarts=attempt))
        raise RuntimeError("aggregation tables overflowed after retries")

    def columnar_query(self, query, filt, params, kinds, cols, vals):
        """K7: evaluate `query` over one index metric's typed columns
        on-device (columnar_query_kernel) — no NDJSON round trip
        (reference lib/index-query.js:303-338 semantics; VERDICT r1
        #6).

        query:  the effective QueryConfig (drives decode: date and
                bucket canonicalization)
        filt:   combined query ∧ time-bounds krill filter (or None)
        params: the metric's param dicts (column name order)
        kinds:  'n'/'s' per column (matches read_columns)
        cols:   per column f64 numpy array or (blob, offs, lens)
        vals:   f64 numpy array of row weights
        """
        from . import colquery
        return colquery.columnar_query(self, query, filt, params, kinds,
                                       cols, vals)

    def coded_query(self, query, filt, params, kinds, merged,
                    timings=None):
        """Evaluate `query` over the merged, dictionary-coded sidecar
        columns of a whole launch group in one pass (dict_intern_kernel
        + coded_query_kernel, ops/hip/scan_columns.h).

        query, filt, params, kinds: as columnar_query takes them
        merged: index.columnar.Merged — the needed columns of the
                group's files concatenated, string columns as codes
                into one launch dictionary, seg_start row offsets
        timings: a dict to receive the seconds spent in "h2d", "kernels"
                (tables allocated, both kernels run) and "decode"; each
                phase then ends in a device synchronise (measurement
                only)

        Returns one Aggregator per file of the group, in order: that
        file's partial result, as its own SQLite GROUP BY would give.
        """
        from . import colquery
        return colquery.coded_query(self, query, filt, params, kinds,
                                    merged, timings)


class _ScanContext(object):
    def __init__(self, eng, cplan, agg_slots, dict_slots, dict_data_cap,
                 dense=None, growable=False):
        torch = eng.torch
        if growable:
            dense = False  # the dense directory does not grow
        self.eng = eng
        self.t = torch
        self.cplan = cplan
        dev = eng.device
        # Dense-accumulation mode (default on): the aggregate table is
        # a small slot directory, per-workgroup counts go to a dense
        # partial matrix, and the MFMA f64 column-sum reduce folds it
        # before extraction.  High cardinality overflows
        # the directory and the engine restarts with dense off (the
        # atomic hash path).
        if dense is None:
            dense = _env_int("DRAGNET_DENSE", 1) == 1
        self.dense = dense
        if dense:
            agg_slots = _env_int("DRAGNET_DENSE_SLOTS", 8192)

        def dev_i32(np_arr):
            return torch.from_numpy(
                np.ascontiguousarray(np_arr.astype(np.int32))).to(dev)

        def dev_f64(np_arr):
            return torch.from_numpy(
                np.ascontiguousarray(np_arr.astype(np.float64))).to(dev)

        # plan buffers and scalars, by name
        progs, bounds = cplan.programs
        metrics, sreq = cplan.metrics
        bds, steps = cplan.breakdown_descs
        plan = dict(
            field_sigs=torch.from_numpy(
                cplan.field_sigs.view(np.int64)).to(dev),
            comp_slot=torch.from_numpy(cplan.comp_slot).to(dev),
            nf_match=cplan.nf_match,
            sig_bloom=cplan.sig_bloom,
            fields_parent_sig=cplan.fields_parent_sig,
            prog_nodes=dev_i32(progs),
            prog_bounds=dev_i32(bounds),
            const_meta=dev_i32(cplan.const_meta),
            const_dvals=dev_f64(cplan.const_dvals),
            const_bytes=torch.from_numpy(
                np.ascontiguousarray(cplan.const_bytes)).to(dev),
            synth_slots=dev_i32(cplan.synthetic),
            n_synth=cplan.n_synth,
            metric_rows=dev_i32(metrics),
            synth_req=dev_i32(sreq),
            bd_rows=dev_i32(bds),
            bd_steps=dev_f64(steps),
            value_slot=cplan.value_slot,
            fields_slot=cplan.fields_slot,
            skinner=cplan.data_format == "json-skinner",
        )

        # The bound extension object allocates and owns the tables,
        # dictionaries and counters (the kernel descriptors point into
        # its tensors) and caches the launch knobs (DRAGNET_MIN_WAVES /
        # XGRAN / LDS_STAGE) as of now.
        self.state = eng.ops.ScanState(
            plan=plan, agg_slots=agg_slots, dict_slots=dict_slots,
            dict_data_bytes=dict_data_cap, dense=dense)

        # Growable scans: every launch goes through the planner, which
        # books occupancy against the state's sizes
        self.planner = None
        if growable:
            nm, s_cols, n_cols = capacity.plan_shape(metrics, bds)
            sizes = self.state.sizes()
            self.planner = capacity.CapacityPlanner(
                nm, s_cols, n_cols,
                dict(sizes, agg=[sizes["agg%d" % m] for m in range(nm)]))

        # chunk buffers + newline index, all modes (_ensure_buffers)
        self._pinned = self._dev_data = None
        self._pos = self._nlines = self._segs = None
        # feed/flush: the one pinned buffer, copies on the current stream
        self._partial = b""
        self._copy_ev = None  # guards pinned-buffer reuse across chunks
        self._fin_stream = None  # lazy: D2H lane for pipelined decode
        # staging state of one mode each, created by the method named:
        self._files = None  # _ensure_file_staging: ping-pong buffers
        self._pool = None   # stage_resident: slices + pass ping-pong
        self._x = None      # stage_xpose: ScanState.scan_xpose's arguments

    @property
    def counters(self):
        return self.state.counters

    @property
    def agg_slots(self):
        """Slots of the largest aggregation table."""
        return max(v for k, v in self.state.sizes().items()
                   if k.startswith("agg"))

    @property
    def dict_slots(self):
        sizes = self.state.sizes()
        return max(sizes["sdict"], sizes["ndict"])

    # ---- chunk feeding ----

    def feed(self, chunk):
        """Consume a byte chunk (records split on newlines; partial
        trailing line carried to the next chunk)."""
        data = self._partial + chunk
        cut = data.rfind(b"\n")
        if cut < 0:
            self._partial = data
            return
        self._partial = data[cut + 1:]
        self._run(data[:cut + 1])

    def flush(self):
        if self._partial:
            self._run(self._partial + b"\n")
            self._partial = b""

    def _ensure_buffers(self, padded):
        torch = self.t
        dev = self.eng.device
        if self._pinned is not None and self._pinned.numel() >= padded:
            return
        cap = max(padded, self.eng.chunk_bytes + (1 << 20))
        cap = (cap + 15) & ~15
        self._pinned = torch.empty(cap, dtype=torch.uint8, pin_memory=True)
        self._dev_data = torch.empty(cap, dtype=torch.uint8, device=dev)
        # worst case: every byte is a newline
        self._pos = torch.empty(cap + 2, dtype=torch.int32, device=dev)
        self._nlines = torch.zeros(1, dtype=torch.int32, device=dev)
        self._segs = torch.empty(cap // 2048 + 2, dtype=torch.int32,
                                 device=dev)

    @staticmethod
    def _pad_pinned(pin, n):
        """Newline-pad pin[:n] (16B cursor window) -> padded length."""
        padded = _pad(n)
        pin[n:padded] = 10
        return padded

    def _index(self, dev_data, start, end):
        """Newline index of dev_data[start:end] -> (pos, nlines)."""
        self.eng.ops.newline_index(dev_data, start, end, self._segs,
                                   self._pos, self._nlines)
        return self._pos, self._nlines

    def _submit(self, dev_data, start, end, index=None):
        """Newline index (unless a pre-built one is given) + fused
        scan of dev_data[start:end] on the current stream."""
        pos, nlines = index or self._index(dev_data, start, end)
        if self.planner is None:
            self.state.scan(dev_data, pos, nlines, start)
        else:
            self._scan_planned(dev_data, pos, nlines, start, end)

    # ---- growable scans (engine/capacity.py) ----

    def _scan_planned(self, dev_data, pos, nlines, start, end):
        """Scan the chunk as planner-sized sub-ranges of its records,
        growing whatever the next one might fill.  Records [a, b) are
        launched as pos[a:b] with first_start at record a's first byte;
        ScanState.scan clamps the device line count (the chunk's, at
        least b - a) to that slice.  One small D2H copy — the line
        count and the newline position ahead of every floor-th record —
        tells the host all it plans with: a host sync per chunk, on
        this path only."""
        torch = self.t
        pl = self.planner
        g = pl.floor
        # a chunk of end - start bytes holds at most that many lines
        host = torch.cat(
            [nlines, pos[g - 1:end - start:g]]).cpu().numpy()
        nrec = min(int(host[0]), pos.numel())
        marks = host[1:].view(np.uint32)

        def start_of(i):
            if i == 0:
                return start
            if i == nrec:
                return end  # at or past the last record's newline
            return int(marks[i // g - 1]) + 1

        a = 0
        while a < nrec:
            b = pl.next_range(a, nrec, start_of, self._measure, self.grow)
            self.state.scan(dev_data, pos[a:b], nlines, start_of(a))
            a = b

    def _measure(self, names):
        """True occupancy of the named structures (one device read)."""
        occ = self.state.occupancy().cpu().tolist()
        true = dict(zip(self.planner.names, occ))
        return {n: true[n] for n in names}

    def grow(self, name, new_size):
        """Grow one structure ("agg<m>", "sdict", "sdata", "ndict") to
        new_size on the device, contents and ids preserved."""
        old = self.planner.size[name]
        if name.startswith("agg"):
            self.state.grow_agg(int(name[3:]), new_size)
        else:
            getattr(self.state, "grow_" + name)(new_size)
        self.planner.size[name] = new_size
        from ..log import get_logger
        get_logger().child("gpu-engine").warn(
            "table grown in place", structure=name, size=old,
            new_size=new_size)

    def _run(self, buf):
        torch = self.t
        n = len(buf)
        self._ensure_buffers(_pad(n))
        pin = self._pinned
        # the previous chunk's async H2D copy must complete before the
        # pinned buffer is overwritten
        if self._copy_ev is None:
            self._copy_ev = torch.cuda.Event()
        else:
            self._copy_ev.synchronize()
        pin[:n] = torch.frombuffer(bytearray(buf), dtype=torch.uint8)
        padded = self._pad_pinned(pin, n)
        self._dev_data[:padded].copy_(pin[:padded], non_blocking=True)
        self._copy_ev.record()
        self._submit(self._dev_data, 0, n)

    def overflowed(self):
        return int(self.counters[C_OVERFLOW].item()) > 0

    # ---- zero-copy file scanning ----

    def scan_files(self, files):
        """Scan the concatenated bytes of `files`, read directly into
        ping-pong pinned buffers (no intermediate Python bytes):
        chunks.frame_files fills and cuts one buffer while the GPU
        works on the other.  (DRAGNET_CHUNK_MB=1024 adds ~10% on
        >=50 GB scans at the cost of slower pinned-buffer startup.)"""
        cap = self.eng.chunk_bytes
        if self._pinned is None:  # buffers not sized yet
            try:
                total = sum(os.stat(p).st_size for p in files)
            except OSError:
                total = 0
            cap = choose_chunk_bytes(total, cap,
                                     "DRAGNET_CHUNK_MB" in os.environ)
        pins = self._ensure_file_staging(cap)
        evs = [None, None]  # H2D-complete, per pinned buffer

        def wait(i):
            if evs[i] is not None:
                evs[i].synchronize()
                evs[i] = None

        frames = frame_files(files, [memoryview(p.numpy()) for p in pins],
                             cap, wait, _env_int("DRAGNET_READERS", 24))
        try:
            for i, n in frames:
                evs[i] = self._run_pinned(pins[i], n)
        finally:
            frames.close()  # descriptors + reader pool

    def _ensure_file_staging(self, cap):
        """Ping-pong pinned and DEVICE buffers with the H2D on a
        dedicated copy stream: chunk k+1's copy overlaps chunk k's
        kernels, so the steady state is max(fill, copy, kernels)
        instead of their sum (serial: 12-15 GB/s end-to-end vs the
        67 GB/s the readers deliver; profiles/r02).  Returns the pins."""
        torch = self.t
        if self._files is None:
            if self._pinned is None:
                self._ensure_buffers(_pad(cap))
            self._files = SimpleNamespace(
                pins=[self._pinned, torch.empty(
                    self._pinned.numel(), dtype=torch.uint8,
                    pin_memory=True)],
                copy_stream=torch.cuda.Stream(device=self.eng.device),
                dev=[self._dev_data, torch.empty_like(self._dev_data)],
                done=[torch.cuda.Event(), torch.cuda.Event()],
                idx=0)
        return self._files.pins

    def _run_pinned(self, pin, n):
        """H2D + kernels for pin[:n] (already newline-terminated).
        Returns the H2D-complete event — the caller must wait on it
        before refilling this pinned buffer."""
        torch = self.t
        f = self._files
        padded = self._pad_pinned(pin, n)
        idx = f.idx
        f.idx ^= 1
        dev_data = f.dev[idx]
        main = torch.cuda.current_stream(self.eng.device)
        cs = f.copy_stream
        # last kernel reader of this device buffer must finish first
        cs.wait_event(f.done[idx])
        ev = torch.cuda.Event()
        with torch.cuda.stream(cs):
            dev_data[:padded].copy_(pin[:padded], non_blocking=True)
            ev.record(cs)
        main.wait_event(ev)
        self._submit(dev_data, 0, n)
        f.done[idx].record(main)
        return ev

    # ---- resident-pool path (bench / repeated scans) ----

    def stage_resident(self, buf, n_slices=None):
        """Stage a byte pool into the pinned buffer once; later
        scan_resident() calls re-run the H2D + kernels without the
        host-side copy.  The pool is split into newline-aligned
        slices so the H2D copy of slice k+1 overlaps the scan of
        slice k (copy stream + events)."""
        torch = self.t
        if n_slices is None:
            n_slices = _env_int("DRAGNET_SLICES", 6)
        n = len(buf)
        self._ensure_buffers(_pad(n))
        pin = self._pinned
        pin[:n] = torch.frombuffer(bytearray(buf), dtype=torch.uint8)
        padded = self._pad_pinned(pin, n)

        # newline-aligned slice boundaries
        bounds = sorted({0, n} | {buf.rfind(b"\n", 0, n * k // n_slices) + 1
                                  for k in range(1, n_slices)})
        slices = list(zip(bounds, bounds[1:]))
        # Ping-pong device pools for streaming passes: pass k+1's H2D
        # lands in the buffer pass k is NOT reading, so the copy
        # stream runs back-to-back at link rate instead of stalling
        # behind pass k's kernel tail + extraction + reset.
        self._pool = p = SimpleNamespace(
            n=n, padded=padded, slices=slices,
            copy_stream=torch.cuda.Stream(device=self.eng.device),
            evs=[torch.cuda.Event() for _ in slices],
            dev_pp=torch.empty_like(self._dev_data),
            pass_done=[torch.cuda.Event(), torch.cuda.Event()],
            idx=0, pos=[])

        # Pre-index line positions per slice: the pool bytes are
        # identical on every pass, so the line index is computed once
        # here (a re-scanning engine retains its line index the same
        # way the reference retains its on-disk indexes).
        self._dev_data[:padded].copy_(pin[:padded])
        for (s, e) in slices:
            pos, nlines = self._index(self._dev_data, s, e)
            p.pos.append(
                (pos[:int(nlines.item())].clone(), nlines.clone()))

    def scan_resident(self, h2d=True):
        """One full streaming pass over the staged pool: sliced async
        H2D on a copy stream overlapping newline-index + fused scan on
        the compute stream.  h2d=False skips the copies (device-
        resident re-scan: data already in HBM from a previous pass)."""
        torch = self.t
        p = self._pool
        padded = p.padded
        dev_data = self._dev_data
        pin = self._pinned
        main = torch.cuda.current_stream(self.eng.device)
        if h2d:
            # ping-pong: write the buffer the PREVIOUS pass did not
            # read; wait only for the pass-before-last (the last
            # reader of this buffer), which has long finished — so
            # the copies chain back-to-back across passes
            idx = p.idx
            p.idx ^= 1
            dev_data = self._dev_data if idx == 0 else p.dev_pp
            ev_done = p.pass_done[idx]
            p.copy_stream.wait_event(ev_done)
            with torch.cuda.stream(p.copy_stream):
                for k, (s, e) in enumerate(p.slices):
                    s16 = s & ~15
                    e16 = min((e + 15) & ~15, padded)
                    dev_data[s16:e16].copy_(pin[s16:e16],
                                            non_blocking=True)
                    p.evs[k].record(p.copy_stream)
        # kernels per slice on the compute stream.  Streaming passes
        # (h2d=True) model fresh data and re-index newlines each pass;
        # device-resident re-scans reuse the staged line index.
        for k, (s, e) in enumerate(p.slices):
            if h2d:
                main.wait_event(p.evs[k])
                self._submit(dev_data, s, e)
            else:
                self._submit(dev_data, s, e, p.pos[k])
        if h2d:
            ev_done.record(main)  # last reader of this pass's buffer

    # ---- wave-transposed staging (prototype; DRAGNET_XPOSE) ----

    def stage_xpose(self, buf=None):
        """Wave-transposed staging for scan_kernel_x (engine/xpose.py).

        Default: built ON DEVICE from the resident pool — no host
        staging pass.  DRAGNET_XPOSE_HOST=1 selects the r1 numpy
        builder (A/B + layout unit tests)."""
        gran = _env_int("DRAGNET_XGRAN", 64)
        if gran not in (32, 64, 128):
            # the scan kernel is templated on the granule size; an
            # unsupported value would mismatch the staged layout
            raise ValueError("DRAGNET_XGRAN must be 32, 64 or 128")
        if os.environ.get("DRAGNET_XPOSE_HOST") == "1":
            self._x = xpose.build_on_host(self.t, buf, gran,
                                          self.eng.device)
            return
        if self._pool is None:
            if buf is None:
                raise ValueError("no resident pool to transpose")
            self.stage_resident(buf)
        # full-pool line index (the staged slice indexes cover slices)
        pos, nlines = self._index(self._dev_data, 0, self._pool.n)
        self._x = xpose.build_on_device(self.t, self.eng.ops,
                                        self._dev_data, pos, nlines, gran)

    def scan_xpose(self):
        """One scan pass over the wave-transposed staging."""
        self.state.scan_xpose(*self._x)

    def make_graph(self, h2d=True, xpose=False):
        """Capture reset + the whole scan pass into a hipGraph so a
        step replays as one launch (the per-slice kernel+copy launch
        overhead otherwise costs ~0.5-1 ms per step).  Returns a
        replayable graph or None if capture fails."""
        torch = self.t

        def pass_():
            self.reset()
            if xpose:
                self.scan_xpose()
            else:
                self.scan_resident(h2d=h2d)

        try:
            # warm up the exact op sequence outside capture
            pass_()
            torch.cuda.synchronize(self.eng.device)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                pass_()
            torch.cuda.synchronize(self.eng.device)
            return g
        except Exception:
            return None

    def reset(self):
        """Zero tables/dictionaries/counters for a fresh scan job
        (one binding call; ~10 separate .zero_() dispatches otherwise
        show up at 5 ms/step)."""
        self.state.reset()
        if self.planner is not None:
            self.planner.occ = dict.fromkeys(self.planner.names, 0)

    # ---- results ----

    def finalize(self, queries):
        return self.decode_extracted(self.extract_async(queries),
                                     queries)

    def extract_async(self, queries):
        """Enqueue the table/dictionary extraction kernels and snapshot
        everything decode needs into fresh device tensors, WITHOUT any
        host sync.  The returned handle is safe across a subsequent
        reset()/scan of this context (the snapshots are ordered on the
        current stream before the reset's zeroing), which lets a caller
        software-pipeline host-side decode of step k with step k+1's
        copies/kernels (bench.py streaming mode)."""
        h = self.state.extract_all()
        h["ev"] = self.t.cuda.Event()
        h["ev"].record()
        return h

    def decode_extracted(self, h, queries):
        """Host-side half of finalize(): wait for the extraction
        snapshot (ONLY — via its event, on a dedicated D2H stream, so
        in-flight work from a subsequent step is not drained), copy it
        to the host and decode into Aggregators (engine/decode.py)."""
        torch = self.t
        if self._fin_stream is None:
            self._fin_stream = torch.cuda.Stream(device=self.eng.device)
        with torch.cuda.stream(self._fin_stream):
            self._fin_stream.wait_event(h["ev"])
            host = {"cnt": h["cnt"].cpu().numpy()}
            host.update(self._fetch_dicts(h))
            host["aggs"] = []
            for k_full, c_full, out_n in h["aggs"][:len(queries)]:
                n_out = min(int(out_n.item()), k_full.shape[0])
                host["aggs"].append((k_full[:n_out].cpu().numpy(),
                                     c_full[:n_out].cpu().numpy()))
        return decode.decode_snapshot(host, queries, self.cplan)

    @staticmethod
    def _fetch_dicts(h):
        """Host copies of the extraction's dictionaries (decode.py's
        `host` keys).  The caller has waited for h["ev"]."""
        n_str = int(h["n_str"].item())
        n_num = int(h["n_num"].item())
        host = {"n_str": n_str, "n_num": n_num}
        if n_str:
            host["str_off"] = h["str_off"][:n_str].cpu().numpy()
            host["str_len"] = h["str_len"][:n_str].cpu().numpy()
            used = int(h["used"].item())
            host["blob"] = h["blob"][:used].cpu().numpy()
        if n_num:
            host["numbers"] = h["numbers"][:n_num].cpu().numpy()
        return host

    @classmethod
    def _decode_dicts(cls, h):
        return decode.decode_dicts(cls._fetch_dicts(h))

"""
Host-side capacity planner for growable GPU scans: no torch, no GPU.

A growable scan (engine/gpu.py: byte sources, pipes, DRAGNET_GROW=1)
never lets a table overflow.  The engine cuts each chunk's records into
sub-ranges; before every launch the planner checks, for every
structure, that

    occupancy + worst-case demand of the sub-range <= load cap

and otherwise has the engine measure the true occupancy and, if that
still does not fit, grow the structure on the device (ScanState.grow_*)
before the launch.  The host figure is pessimistic: after each launch
it rises by the whole demand, with no device read; it is reset to the
truth only when it stands in the way.

Structures, by name: "agg0".."agg<nm-1>" (one aggregation table per
metric, in slots), "sdict" (string dictionary slots), "sdata" (string
payload bytes), "ndict" (number dictionary slots).  Each grows on its
own.

Worst-case demand of R records spanning B bytes:

  agg<m>  R             every record a new group
  sdict   R * S         S = non-bucketized breakdown columns over all
                        metrics (a companion slot changes which slot a
                        column reads, not how many strings it interns)
  sdata   S * (B + 8R)  an interned span lies inside its record, so a
                        column's spans sum to at most B; payloads are
                        stored in 8-byte granules (< 8 bytes of padding
                        each)
  ndict   R * N         N = all breakdown columns (a bucketized column
                        interns its ordinal when it is not small)

Load cap.  A slot table stays at or below 3/4 full after the sub-range;
the payload buffer at or below its size.  What bounds the load is the
probe limits in ops/hip/scan_tables.h: agg_insert gives up after
AGG_MAX_PROBES = 4096 probes and the dictionaries after a whole-table
walk.  With linear probing the longest run of full slots in a table of
n slots at load a is about ln(n) / (a - 1 - ln a): at a = 3/4 and the
largest table allowed (2^29 slots) that is ~530, an 8x margin under
4096; at 7/8 it is ~2400, too close.  1/2 would be gentler on probe
lengths, but a table reaches its cap only right before it grows (after
a 4x growth it is at most 3/16 full), and at 1/2 a 128-slot table could
not hold one 64-record sub-range next to even a handful of live groups.
"""

import os

MAX_KEY = 8

LOAD_NUM, LOAD_DEN = 3, 4

DEFAULT_MIN_RECORDS = 65536

# Hard limits (largest permitted size of each structure)
#  agg:   the device indexes keys as slot * MAX_KEY in uint32
#  sdict: a string id must fit SPECIAL_ARRJSON's 27 bits (any string
#         column may hold arrays; ids < 3/4 of the slots) and, being
#         smaller, make_code's 30
#  sdata: payload offsets are uint32
#  ndict: a number id must fit make_code's 30-bit payload
LIMITS = {
    "agg": ((1 << 32) // MAX_KEY,
            "uint32 slot index times MAX_KEY"),
    "sdict": (1 << 27, "27-bit string id of SPECIAL_ARRJSON"),
    "sdata": ((1 << 32) - 1, "32-bit payload offset"),
    "ndict": (1 << 30, "30-bit id payload of make_code"),
}


class CapacityError(RuntimeError):
    pass


def kind_of(name):
    return "agg" if name.startswith("agg") else name


def min_records_from_env():
    try:
        v = int(os.environ.get("DRAGNET_GROW_MIN_RECORDS",
                               DEFAULT_MIN_RECORDS))
    except ValueError:
        v = DEFAULT_MIN_RECORDS
    return max(1, v)


def plan_shape(metric_rows, bd_rows):
    """(n_metrics, S, N) of a compiled plan: metric_rows is
    CompiledPlan.metrics[0] ([prog, n_bd, bd_off, ...] per metric),
    bd_rows is CompiledPlan.breakdown_descs[0] ([kind, ref, bucket, _]
    per breakdown column; bucket 0 = none)."""
    s = n = 0
    for row in metric_rows:
        nbd, off = int(row[1]), int(row[2])
        for b in range(off, off + nbd):
            n += 1
            if int(bd_rows[b][2]) == 0:
                s += 1
    return len(metric_rows), s, n


def _pow2_at_least(n):
    p = 1
    while p < n:
        p <<= 1
    return p


class CapacityPlanner(object):
    """Occupancy book-keeping and sub-range planning for one scan.

    sizes: {"agg": slots (or a per-metric list), "sdict": slots,
            "sdata": bytes, "ndict": slots}
    floor: smallest sub-range worth a launch (records); sub-ranges are
           whole multiples of it except the one that ends the chunk.
    """

    def __init__(self, n_metrics, str_cols, num_cols, sizes, floor=None):
        self.nm = n_metrics
        self.S = str_cols
        self.N = num_cols
        self.floor = floor if floor is not None else min_records_from_env()
        agg = sizes["agg"]
        if isinstance(agg, int):
            agg = [agg] * n_metrics
        self.names = ["agg%d" % m for m in range(n_metrics)] + \
            ["sdict", "sdata", "ndict"]
        self.size = dict(zip(self.names, list(agg) + [
            sizes["sdict"], sizes["sdata"], sizes["ndict"]]))
        self.occ = dict.fromkeys(self.names, 0)      # pessimistic
        self.growths = dict.fromkeys(self.names, 0)
        self.measures = 0

    # ---- the invariant ----

    def cap(self, name, size=None):
        """Largest occupancy `name` may reach at `size`."""
        size = self.size[name] if size is None else size
        if name == "sdata":
            return size
        return size * LOAD_NUM // LOAD_DEN

    def demand(self, nrec, nbytes):
        d = {}
        for m in range(self.nm):
            d["agg%d" % m] = nrec
        d["sdict"] = nrec * self.S
        d["sdata"] = self.S * (nbytes + 8 * nrec)
        d["ndict"] = nrec * self.N
        return d

    def unfit(self, nrec, nbytes):
        """Names of the structures a sub-range does not fit under."""
        d = self.demand(nrec, nbytes)
        return [n for n in self.names
                if d[n] and self.occ[n] + d[n] > self.cap(n)]

    # ---- growth ----

    def grown_size(self, name, need):
        """New size of `name` so that `need` (occupancy + demand) fits
        under the cap: the smallest power of two that does, and at
        least 4x the present size.  Where 4x would pass the hard limit
        but a smaller power of two still fits, that one is taken; else
        CapacityError names the structure, its size and the limit."""
        size = self.size[name]
        limit, why = LIMITS[kind_of(name)]
        new = _pow2_at_least(4 * size)
        while self.cap(name, new) < need:
            new <<= 1
        if new > limit:
            new = 1 << (limit.bit_length() - 1)  # largest power of two
            if new <= size or self.cap(name, new) < need:
                raise CapacityError(
                    "cannot grow %s (size %d) to hold %d: the hard "
                    "limit is %d (%s)" % (name, size, need, limit, why))
        return new

    # ---- planning ----

    def next_range(self, a, nrec, start_of, measure, grow):
        """End b of the sub-range [a, b) to launch next in a chunk of
        nrec records; grows structures first where needed and books the
        sub-range's demand.

        start_of(i): byte offset at which record i starts, for i a
            multiple of the floor or i == nrec (the end of the chunk)
        measure(names) -> {name: true occupancy}   (one device read)
        grow(name, new_size): grow on the device; may raise
        """
        g = self.floor
        kmax = -(-(nrec - a) // g)
        base = start_of(a)

        def end(k):
            return min(a + k * g, nrec)

        def fits(k):
            b = end(k)
            return not self.unfit(b - a, start_of(b) - base)

        def largest():
            # demand is monotone in k
            if fits(kmax):
                return kmax
            if not fits(1):
                return 0
            lo, hi = 1, kmax
            while hi - lo > 1:
                mid = (lo + hi) // 2
                if fits(mid):
                    lo = mid
                else:
                    hi = mid
            return lo

        k = kmax if fits(kmax) else 0
        if not k:
            # the pessimistic figures stand in the way of launching the
            # rest of the chunk at once: replace them by the truth
            b = end(kmax)
            names = self.unfit(b - a, start_of(b) - base)
            self.occ.update(measure(names))
            self.measures += 1
            k = largest()
        if not k:
            b = end(1)
            d = self.demand(b - a, start_of(b) - base)
            for name in self.unfit(b - a, start_of(b) - base):
                new = self.grown_size(name, self.occ[name] + d[name])
                grow(name, new)
                self.size[name] = new
                self.growths[name] += 1
            k = largest()
            assert k >= 1
        b = end(k)
        d = self.demand(b - a, start_of(b) - base)
        for name in self.names:
            self.occ[name] += d[name]
        return b

    def grow_counts(self):
        """Growths per structure, in ScanResult.gpu_stats form."""
        return {"agg": [self.growths["agg%d" % m]
                        for m in range(self.nm)],
                "sdict": self.growths["sdict"],
                "sdata": self.growths["sdata"],
                "ndict": self.growths["ndict"]}

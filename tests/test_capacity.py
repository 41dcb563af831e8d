"""
The host-side capacity planner of growable GPU scans
(dragnet_amd/engine/capacity.py), alone: no torch, no GPU.  A simulated
device holds the true occupancies; the planner must keep
occupancy + worst-case demand under the load cap before every launch,
tile every chunk exactly, grow by powers of two and at least 4x, and
name the structure, its size and the limit when it cannot grow.
"""

import random

import pytest

from dragnet_amd.engine import capacity
from dragnet_amd.engine.capacity import CapacityError, CapacityPlanner


class SimDevice(object):
    """True occupancies; each launched record adds a random share of
    its worst-case demand."""

    def __init__(self, planner, rng, fill, ceiling=None):
        self.pl = planner
        self.rng = rng
        self.fill = fill  # 0..1: how much of the worst case comes true
        self.ceiling = ceiling  # distinct values the input holds at all
        self.true = dict.fromkeys(planner.names, 0)
        self.size = dict(planner.size)
        self.grown = []
        self.launches = []

    def measure(self, names):
        return {n: self.true[n] for n in names}

    def grow(self, name, new_size):
        self.grown.append((name, self.size[name], new_size))
        self.size[name] = new_size

    def launch(self, a, b, nbytes):
        pl = self.pl
        d = pl.demand(b - a, nbytes)
        for n in pl.names:
            # the invariant, against the TRUE occupancy and the size
            # the device really has
            assert self.true[n] + d[n] <= pl.cap(n, self.size[n]), n
            # the host figure is never below the truth
            assert pl.occ[n] - d[n] >= self.true[n], n
            self.true[n] += int(d[n] * self.fill * self.rng.random())
            if self.ceiling is not None:
                self.true[n] = min(self.true[n], self.ceiling)
        self.launches.append((a, b))


def run_chunk(pl, dev, rng, nrec):
    """Plan and 'launch' one chunk of nrec records of random lengths;
    returns the sub-ranges."""
    lens = [rng.randrange(1, 300) for _ in range(nrec)]
    starts = [0]
    for ln in lens:
        starts.append(starts[-1] + ln)
    g = pl.floor

    def start_of(i):
        assert i % g == 0 or i == nrec, "only sampled boundaries"
        return starts[i]

    ranges = []
    a = 0
    while a < nrec:
        b = pl.next_range(a, nrec, start_of, dev.measure, dev.grow)
        dev.launch(a, b, starts[b] - starts[a])
        ranges.append((a, b))
        a = b
    return ranges


@pytest.mark.parametrize("seed", range(12))
def test_invariant_and_tiling(seed):
    rng = random.Random(seed)
    nm = rng.randrange(1, 4)
    n_cols = rng.randrange(nm, 3 * nm + 1)
    s_cols = rng.randrange(0, n_cols + 1)
    floor = rng.choice([1, 7, 64, 100])
    pl = CapacityPlanner(
        nm, s_cols, n_cols,
        {"agg": rng.choice([128, 1024]), "sdict": rng.choice([128, 4096]),
         "sdata": rng.choice([1 << 12, 1 << 20]), "ndict": 128},
        floor=floor)
    dev = SimDevice(pl, rng, fill=rng.choice([0.0, 0.05, 0.5, 1.0]))
    for _ in range(rng.randrange(1, 6)):
        nrec = rng.randrange(1, 3000)
        ranges = run_chunk(pl, dev, rng, nrec)
        # exact tiling: no record skipped or repeated
        assert ranges[0][0] == 0 and ranges[-1][1] == nrec
        for (a0, b0), (a1, _b1) in zip(ranges, ranges[1:]):
            assert b0 == a1 and b0 > a0
        # the floor: only the sub-range that ends the chunk is short
        for a, b in ranges:
            assert b - a >= min(floor, nrec) or b == nrec
            assert a % floor == 0
    for name, old, new in dev.grown:
        assert new & (new - 1) == 0 and new >= 4 * old
    assert pl.size == dev.size
    assert sum(pl.growths.values()) == len(dev.grown)


def test_low_occupancy_never_grows():
    """Default sizes, true occupancy far below 1% of capacity: the
    pessimistic figure fills up and is re-measured, nothing grows."""
    rng = random.Random(5)
    pl = CapacityPlanner(1, 2, 2, {"agg": 1 << 20, "sdict": 1 << 20,
                                   "sdata": 256 << 20, "ndict": 1 << 20},
                         floor=65536)
    # a few hundred groups / strings, whatever the record count
    dev = SimDevice(pl, rng, fill=1.0, ceiling=500)
    for _ in range(4):
        run_chunk(pl, dev, rng, 700_000)
    assert dev.grown == []
    assert pl.grow_counts() == {"agg": [0], "sdict": 0, "sdata": 0,
                                "ndict": 0}
    assert pl.measures >= 1  # it did have to look


def test_small_scan_never_measures():
    pl = CapacityPlanner(1, 1, 1, {"agg": 1 << 20, "sdict": 1 << 20,
                                   "sdata": 256 << 20, "ndict": 1 << 20},
                         floor=65536)

    def no_device(*_a):
        raise AssertionError("no device read or growth expected")

    b = pl.next_range(0, 20_000, lambda i: i * 230, no_device, no_device)
    assert b == 20_000


def test_growth_sizes():
    pl = CapacityPlanner(1, 1, 1, {"agg": 128, "sdict": 128,
                                   "sdata": 1000, "ndict": 128}, floor=64)
    assert pl.grown_size("agg0", 10) == 512           # at least 4x
    assert pl.grown_size("agg0", 384) == 512          # 3/4 of 512
    assert pl.grown_size("agg0", 385) == 1024
    assert pl.grown_size("sdata", 1) == 4096          # pow2 >= 4 * 1000
    assert pl.grown_size("sdata", 5000) == 8192


@pytest.mark.parametrize("name,size,word", [
    ("agg0", 1 << 29, "MAX_KEY"),
    ("sdict", 1 << 27, "SPECIAL_ARRJSON"),
    ("sdata", 1 << 31, "32-bit payload offset"),
    ("ndict", 1 << 30, "make_code"),
])
def test_hard_limits(name, size, word):
    sizes = {"agg": 128, "sdict": 128, "sdata": 1 << 20, "ndict": 128}
    sizes[capacity.kind_of(name)] = size
    pl = CapacityPlanner(1, 1, 1, sizes, floor=64)
    pl.occ[name] = pl.cap(name)  # full, and at the largest legal size
    with pytest.raises(CapacityError) as ei:
        pl.grown_size(name, pl.occ[name] + 64)
    msg = str(ei.value)
    assert name in msg and str(size) in msg and word in msg
    assert str(capacity.LIMITS[capacity.kind_of(name)][0]) in msg
    assert isinstance(ei.value, RuntimeError)

    # through next_range too: nothing is launched, the error is loud
    def measure(names):
        return {n: pl.occ[n] for n in names}

    def grow(_n, _s):
        raise AssertionError("must not grow past a hard limit")

    with pytest.raises(CapacityError):
        pl.next_range(0, 64, lambda i: i * 100, measure, grow)


def test_last_step_below_limit_is_clamped():
    """4x would pass the limit, but a smaller power of two still fits."""
    pl = CapacityPlanner(1, 1, 1, {"agg": 128, "sdict": 128,
                                   "sdata": 1 << 30, "ndict": 128},
                         floor=64)
    assert pl.grown_size("sdata", (1 << 30) + 5) == 1 << 31


def test_floor_capped_at_chunk_records():
    pl = CapacityPlanner(1, 1, 1, {"agg": 1 << 20, "sdict": 1 << 20,
                                   "sdata": 256 << 20, "ndict": 1 << 20},
                         floor=65536)
    # a 10-record chunk is one 10-record sub-range, and only its two
    # ends are asked for
    asked = []

    def start_of(i):
        asked.append(i)
        return i * 100

    assert pl.next_range(0, 10, start_of, None, None) == 10
    assert set(asked) == {0, 10}
    assert pl.occ["agg0"] == 10


def test_floor_from_env(monkeypatch):
    monkeypatch.delenv("DRAGNET_GROW_MIN_RECORDS", raising=False)
    assert capacity.min_records_from_env() == 65536
    monkeypatch.setenv("DRAGNET_GROW_MIN_RECORDS", "64")
    assert capacity.min_records_from_env() == 64
    sizes = {"agg": 128, "sdict": 128, "sdata": 1 << 20, "ndict": 128}
    assert CapacityPlanner(1, 1, 1, sizes).floor == 64


def test_plan_shape():
    # two metrics: (plain, quantized) and (plain)
    metric_rows = [[1, 2, 0, 0, 0, 0, 0, 0], [2, 1, 2, 0, 0, 0, 0, 0]]
    bd_rows = [[0, 0, 0, 0], [0, 1, 1, 0], [0, 2, 0, 0]]
    assert capacity.plan_shape(metric_rows, bd_rows) == (2, 2, 3)
    # no breakdowns: the placeholder row is not counted
    assert capacity.plan_shape([[1, 0, 0, 0, 0, 0, 0, 0]],
                               [[0, 0, 0, 0]]) == (1, 0, 0)


def test_imports_no_torch():
    import subprocess
    import sys
    code = ("import sys; import dragnet_amd.engine.capacity; "
            "assert 'torch' not in sys.modules")
    subprocess.run([sys.executable, "-c", code], check=True)

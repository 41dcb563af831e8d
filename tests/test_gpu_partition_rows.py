"""
partition_rows (ops/hip/partition_rows.h): remap, hash and split int64
rows by hash % world on the GPU, stably, against the definition in numpy
(remap by fancy indexing, the FNV-style hash in uint64, a stable argsort
by bin).  Everything is integers and bit patterns: every comparison is
for equality.

All tests here require an MI355X (pytest -m gpu).
"""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

I64 = np.iinfo(np.int64)
EL_STR = 1


def ops():
    from dragnet_amd.ops import load_ops
    return load_ops(required=True)


def reference(rows, vals, world, remap=None):
    nk = rows.shape[1] - 1
    codes, tags = rows[:, :nk].copy(), rows[:, nk]
    h = np.zeros(rows.shape[0], dtype=np.uint64)
    for j in range(nk):
        is_str = ((tags >> (2 * j)) & 3) == EL_STR
        if remap is not None:
            codes[is_str, j] = remap[codes[is_str, j]]
        h = (h ^ codes[:, j].astype(np.uint64)) * np.uint64(0x100000001B3)
    h ^= tags.astype(np.uint64)
    part = (h % np.uint64(world)).astype(np.int64)
    wire = np.concatenate(
        [codes, tags[:, None], vals.view(np.int64)[:, None]], axis=1)
    return (wire[np.argsort(part, kind="stable")],
            np.bincount(part, minlength=world))


def device(rows, vals, world, remap=None, **kw):
    import torch
    if remap is not None:
        kw["remap"] = torch.from_numpy(remap).cuda()
    wire, counts = ops().partition_rows(
        torch.from_numpy(np.ascontiguousarray(rows)).cuda(),
        torch.from_numpy(vals).cuda(), rows.shape[1] - 1, world, **kw)
    assert wire.is_cuda and wire.dtype == torch.int64
    assert counts.is_cuda and counts.dtype == torch.int64
    return wire.cpu().numpy(), counts.cpu().numpy()


def check(rows, vals, world, remap=None, **kw):
    want_wire, want_counts = reference(rows, vals, world, remap)
    got_wire, got_counts = device(rows, vals, world, remap, **kw)
    assert got_wire.shape == (rows.shape[0], rows.shape[1] + 1)
    assert np.array_equal(got_counts, want_counts)
    assert np.array_equal(got_wire, want_wire)


def drawn(n, nk, seed):
    """Full-range codes, tags 0 or 2 (never a string), integer values."""
    rng = np.random.default_rng(seed)
    rows = rng.integers(I64.min, I64.max, size=(n, nk + 1), endpoint=True)
    rows[:, nk] = rng.integers(0, 2, size=n) * 2
    return rows, rng.integers(1, 1001, size=n).astype(np.float64)


@pytest.mark.parametrize("nk", [1, 2, 8])
@pytest.mark.parametrize("tiles,plus,max_blocks", [
    (0, 0, 0), (0, 1, 0), (0, 255, 0), (0, 256, 0), (0, 257, 0),
    (1, -1, 0), (1, 0, 0), (1, 1, 0), (3, 5, 0), (3, 5, 2)])
def test_shape_grid(nk, tiles, plus, max_blocks):
    """n = tiles * SORT_TILE + plus: nothing, round and tile edges, a
    block taking two tiles; wire rows of 3 (odd), 4 and 10 words, and
    the unaligned tail of a round (rows * words odd)."""
    rows, vals = drawn(tiles * ops().SORT_TILE + plus, nk,
                       seed=100 * nk + plus)
    check(rows, vals, 8, max_blocks=max_blocks)


@pytest.mark.parametrize("nk", [1, 2])
@pytest.mark.parametrize("world", [1, 2, 3, 8, 256])
def test_worlds(nk, world):
    """No ballot, one, a world that is no power of two, every bin."""
    rows, vals = drawn(ops().SORT_TILE + 300, nk, seed=world)
    check(rows, vals, world)


def test_skew():
    """Every row the same, so one bin takes two tiles and the values
    alone show the order; then codes 0..255 at world 256: the hash's low
    byte is code * 0xB3, one row per bin."""
    n = ops().SORT_TILE + 100
    rows = np.tile(np.array([[7, -3, 0]], dtype=np.int64), (n, 1))
    check(rows, np.arange(n, dtype=np.float64), 8)
    rows = np.zeros((256, 2), dtype=np.int64)
    rows[:, 0] = np.arange(256)
    assert np.array_equal(reference(rows, np.ones(256), 256)[1],
                          np.ones(256, dtype=np.int64))
    check(rows, np.ones(256), 256)


@pytest.mark.parametrize("world", [3, 256])
def test_key_width_and_value_bits(world):
    """Pairs that differ only in the tag pack, in bit 40 of a code, in a
    sign, INT64_MIN against INT64_MAX: a hash over 32 bits, or one that
    drops a column, sends a pair to one bin.  The values' bits (NaN,
    -0.0, infinities) pass through."""
    rows = np.array([
        [5, 6, 0], [5, 6, 2],
        [1 << 40, 9, 2], [0, 9, 2],
        [11, -3, 8], [11, 3, 8],
        [I64.min, 1, 10], [I64.max, 1, 10],
    ], dtype=np.int64)
    vals = np.array([np.nan, -0.0, np.inf, -np.inf, 0.0, 0.5, 2.0 ** 53,
                     -np.nan])
    check(rows, vals, world)


def remapped():
    """Column 0 is string-tagged in the even rows; in the odd ones it is
    an integer that would be out of range for the table.  Column 1 is an
    integer, column 2 always a string."""
    n = ops().SORT_TILE + 17
    rng = np.random.default_rng(31)
    rows = np.empty((n, 4), dtype=np.int64)
    even = np.arange(n) % 2 == 0
    rows[:, 0] = np.where(even, rng.integers(0, 50, size=n),
                          rng.choice([-5, 50, 1 << 40], size=n))
    rows[:, 1] = rng.integers(I64.min, I64.max, size=n)
    rows[:, 2] = rng.integers(0, 50, size=n)
    rows[:, 3] = even * EL_STR + (EL_STR << 4)
    remap = rng.integers(0, 1 << 45, size=50)
    return rows, rng.integers(1, 1001, size=n).astype(np.float64), remap


def test_remap():
    rows, vals, remap = remapped()
    check(rows, vals, 8, remap)
    check(rows, vals, 8)  # no table: string codes pass through


@pytest.mark.parametrize("code", [50, -1])
def test_code_outside_the_table_is_rejected(code):
    rows, vals, remap = remapped()
    rows[ops().SORT_TILE + 2, 0] = code  # an even row of the last tile
    with pytest.raises(RuntimeError, match="remap"):
        device(rows, vals, 8, remap)


@pytest.mark.parametrize("world", [0, 257])
def test_world_out_of_range_is_rejected(world):
    rows, vals = drawn(10, 2, seed=1)
    with pytest.raises(RuntimeError, match="256"):
        device(rows, vals, world)


@pytest.mark.parametrize("remap_on", ["device", "numpy"])
def test_seam_gpu_equals_host(remap_on, monkeypatch):
    import torch

    from dragnet_amd import merge
    rows, vals, remap = remapped()
    codes, tags = np.ascontiguousarray(rows[:, :3]), rows[:, 3].copy()
    monkeypatch.setenv("DRAGNET_PARTITION_GPU", "0")
    want_wire, want_counts = merge.partition_rows(codes, tags, vals, remap, 8)
    assert isinstance(want_wire, np.ndarray)
    monkeypatch.setenv("DRAGNET_PARTITION_GPU", "1")
    if remap_on == "device":
        remap = torch.from_numpy(remap).cuda()
    got_wire, got_counts = merge.partition_rows(codes, tags, vals, remap, 8)
    assert got_wire.is_cuda and got_counts.is_cuda
    assert np.array_equal(got_wire.cpu().numpy(), want_wire)
    assert np.array_equal(got_counts.cpu().numpy(), want_counts)

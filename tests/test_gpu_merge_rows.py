"""
merge_rows (ops/hip/merge_rows.h): group identical int64 rows and sum
their f64 values on the GPU, against np.unique(axis=0) + np.bincount in
float64 on the rows after a numpy remap.  Weights are integers, so every
comparison is for equality.

All tests here require an MI355X (pytest -m gpu).
"""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

I64 = np.iinfo(np.int64)
EL_STR = 1


def reference(rows, vals):
    uniq, inv = np.unique(rows, axis=0, return_inverse=True)
    return uniq, np.bincount(inv.reshape(-1), weights=vals,
                             minlength=uniq.shape[0])


def device(rows, vals, **kw):
    """merge_rows on cuda:0 -> (uniq sorted as np.unique does, sums,
    exact)."""
    import torch

    from dragnet_amd.ops import load_ops
    ops = load_ops(required=True)
    kw = {k: torch.as_tensor(v).cuda() if k == "remap" else v
          for k, v in kw.items()}
    uniq, sums, exact = ops.merge_rows(
        torch.from_numpy(rows).cuda(), torch.from_numpy(vals).cuda(),
        rows.shape[1] - 1, **kw)
    uniq, sums = uniq.cpu().numpy(), sums.cpu().numpy()
    order = np.lexsort(uniq.T[::-1])
    return uniq[order], sums[order], exact


def check(rows, vals, **kw):
    want_rows, want_sums = reference(rows, vals)
    got_rows, got_sums, exact = device(rows, vals, **kw)
    assert np.array_equal(got_rows, want_rows)
    assert np.array_equal(got_sums, want_sums)
    assert exact is True


def drawn(n, nk, pool, seed):
    """n rows drawn from `pool` distinct ones, integer weights."""
    rng = np.random.default_rng(seed)
    distinct = rng.integers(I64.min, I64.max, size=(pool, nk + 1),
                            endpoint=True)
    rows = distinct[rng.integers(0, pool, size=n)]
    return np.ascontiguousarray(rows), \
        rng.integers(1, 1001, size=n).astype(np.float64)


@pytest.mark.parametrize("nk", [1, 2, 8])
@pytest.mark.parametrize("n,max_blocks", [
    (1, 0), (255, 0), (256, 0), (257, 0), (3 * 256 + 5, 2)])
def test_shape_grid(nk, n, max_blocks):
    """Tile edges, odd and even row strides, the unaligned tail (n * w
    odd) and one block taking several tiles."""
    rows, vals = drawn(n, nk, n // 4 + 1, seed=100 * nk + n)
    check(rows, vals, max_blocks=max_blocks)


@pytest.mark.parametrize("pool,hash_mask", [
    (1, -1),       # 1000 identical rows: one slot, all combining
    (None, -1),    # 1000 distinct rows
    (300, 0),      # one home slot: the whole chain is probed and the
    (300, 3),      # full-key compare decides; then four home slots
])
def test_contention_and_probing(pool, hash_mask):
    if pool is None:
        rows, vals = drawn(1000, 2, 1000, seed=7)
        rows[:, 0] = np.arange(1000)  # distinct for certain
    else:
        rows, vals = drawn(1000, 2, pool, seed=8)
    check(rows, vals, hash_mask=hash_mask)


def test_key_width():
    """Pairs that differ in one place only stay two groups each: the
    tag pack alone, bit 40 of a code, the sign of a code, INT64_MIN
    against INT64_MAX (a 32-bit compare or a dropped column merges
    them)."""
    rows = np.array([
        [5, 6, 0], [5, 6, 1],
        [1 << 40, 9, 2], [0, 9, 2],
        [11, -3, 4], [11, 3, 4],
        [I64.min, 1, 6], [I64.max, 1, 6],
    ], dtype=np.int64)
    vals = np.arange(1, 9, dtype=np.float64)
    got_rows, _sums, _exact = device(rows, vals)
    assert got_rows.shape[0] == 8
    check(rows, vals)
    check(rows, vals, hash_mask=0)


def segmented():
    """Three segments, the middle one empty, each with its own
    permutation of a 5-entry dictionary.  Column 0 is string-tagged in
    the even rows and integer-tagged in the odd ones, with the same
    numeric codes; column 1 is always an integer."""
    rng = np.random.default_rng(21)
    sizes = [300, 0, 417]
    n = sum(sizes)
    rows = np.empty((n, 3), dtype=np.int64)
    rows[:, 0] = rng.integers(0, 5, size=n)
    rows[:, 1] = rng.integers(0, 3, size=n)
    rows[:, 2] = (np.arange(n) % 2 == 0) * EL_STR
    vals = rng.integers(1, 1001, size=n).astype(np.float64)
    remaps = [rng.permutation(5), np.zeros(0, np.int64),
              rng.permutation(5)]
    return rows, vals, sizes, remaps


def seg_kw(sizes, remaps):
    import torch
    return dict(
        seg_start=torch.tensor(np.concatenate([[0], np.cumsum(sizes)])),
        remap=np.concatenate(remaps).astype(np.int64),
        remap_off=torch.tensor(
            np.concatenate([[0], np.cumsum([len(m) for m in remaps])])))


def test_segments_and_remap():
    rows, vals, sizes, remaps = segmented()
    mapped = rows.copy()
    at = 0
    for size, remap in zip(sizes, remaps):
        seg = mapped[at:at + size]
        is_str = seg[:, 2] == EL_STR
        seg[is_str, 0] = remap[seg[is_str, 0]]
        at += size
    want_rows, want_sums = reference(mapped, vals)
    got_rows, got_sums, exact = device(rows, vals, **seg_kw(sizes, remaps))
    assert np.array_equal(got_rows, want_rows)
    assert np.array_equal(got_sums, want_sums)
    assert exact is True


def test_code_outside_its_segment_is_rejected():
    """The code equals the first segment's dictionary length: an
    unguarded kernel would read the next segment's table."""
    rows, vals, sizes, remaps = segmented()
    rows[0, 0] = len(remaps[0])
    with pytest.raises(RuntimeError, match="remap"):
        device(rows, vals, **seg_kw(sizes, remaps))


@pytest.mark.parametrize("vals", [[1.0, 0.5, 2.0], [2.0 ** 52, 2.0 ** 52]])
def test_inexact_is_reported(vals):
    """One weight of 0.5; two rows of 2^52 on one key."""
    vals = np.array(vals)
    rows = np.zeros((len(vals), 2), dtype=np.int64)
    _rows, _sums, exact = device(rows, vals)
    assert exact is False


def three_aggregators(query, odd_weight):
    from dragnet_amd.points import Aggregator
    tables = [
        {("GET", 200): 3, ("PUT", 200): 1, (7, 404): 2},
        {("PUT", 200): 10, ("GET", 200): 4, ("HEAD", 1): odd_weight},
        {(7, 404): 6, ("DELETE", "x"): 8, ("GET", 200): 1},
    ]
    aggs = []
    for table in tables:
        aggs.append(Aggregator(query))
        aggs[-1].table.update(table)
    return aggs


@pytest.mark.parametrize("odd_weight", [5, 0.25])
def test_reaggregate_gpu_equals_host(odd_weight, monkeypatch):
    """Same keys, values and insertion order as the host path; a
    fractional weight silently takes the host path."""
    from dragnet_amd.merge import _encode_table, reaggregate
    from dragnet_amd.query import query_load
    q = query_load(breakdown_specs="a,b")
    parts, strings = [], []
    for agg in three_aggregators(q, odd_weight):
        codes, tags, vals, strs = _encode_table(agg, 2)
        parts.append((codes, tags, vals))
        strings.append(strs)
    monkeypatch.setenv("DRAGNET_MERGE_GPU", "0")
    want = reaggregate(q, parts, strings)
    monkeypatch.setenv("DRAGNET_MERGE_GPU", "1")
    got = reaggregate(q, parts, strings)
    assert list(got.table.items()) == list(want.table.items())
    assert got.table[("GET", 200)] == 8

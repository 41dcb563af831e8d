"""
sort_rows (ops/hip/sort_rows.h): the stable lexicographic radix sort of
int64 rows on the GPU, against np.lexsort(rows.T[::-1]) (stable, column
0 first, signed), and merge_rows(sort=True) against np.unique(axis=0) +
np.bincount with no host sort.  Everything is integer: every comparison
is for equality.

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


def tile():
    return ops().SORT_TILE


def drawn(n, w, seed):
    rng = np.random.default_rng(seed)
    pool = rng.integers(I64.min, I64.max, size=(n // 4 + 1, w),
                        endpoint=True)
    return pool[rng.integers(0, pool.shape[0], size=n)]


def check_perm(rows):
    import torch
    rows = np.ascontiguousarray(rows)
    perm = ops().sort_rows(torch.from_numpy(rows).cuda())
    assert perm.dtype == torch.int32 and perm.is_cuda
    assert np.array_equal(perm.cpu().numpy(), np.lexsort(rows.T[::-1]))


@pytest.mark.parametrize("w", [1, 2, 9])
@pytest.mark.parametrize("tiles,plus", [
    (0, 1), (0, 63), (0, 64), (0, 65), (1, -1), (1, 0), (1, 1), (3, 5)])
def test_permutation(w, tiles, plus):
    """n = tiles * SORT_TILE + plus full-range rows drawn with
    replacement from n // 4 + 1: all 8 bytes of every column vary, and
    equal rows test stability.  The single-tile kernel, the first
    multi-tile size, wave edges."""
    check_perm(drawn(tiles * tile() + plus, w, seed=100 * w + plus))


@pytest.mark.parametrize("big", [False, True], ids=["40", "T+40"])
def test_digit_selection_and_sign(big):
    """Codes below 300 (two bytes vary), a constant column, a column
    that differs in byte 5 alone, a column of {-1, 0} (every byte varies)
    holding INT64_MIN and INT64_MAX, and a signed last column with one
    pair of rows that differ in its sign alone."""
    draw = np.random.default_rng(5).integers(0, 300, size=(40, 5))
    rows = draw.astype(np.int64)
    rows[:, 1] = 7
    rows[:, 2] = (draw[:, 2] % 3) << 40
    rows[:, 3] = -(draw[:, 3] % 2)
    rows[0, 3], rows[1, 3] = I64.min, I64.max
    rows[:, 4] -= 150
    rows[3] = rows[2]
    rows[2, 4], rows[3, 4] = 5, -5
    if big:
        n = tile() + 40
        rows = np.tile(rows, (n // 40 + 1, 1))[:n]
        rows[:, 4] += np.arange(n) // 40
    check_perm(rows)


def test_skew():
    """95% zeros in column 0: whole tiles fall into one bin.  Then all
    rows identical: no digit varies and the identity comes back."""
    import torch
    n = 3 * tile() + 5
    rows = np.full((n, 3), 9, dtype=np.int64)
    rows[:, 0] = np.random.default_rng(6).integers(0, 100, size=n) >= 95
    check_perm(rows)
    rows[:, 0] = 1
    perm = ops().sort_rows(torch.from_numpy(rows).cuda())
    assert np.array_equal(perm.cpu().numpy(), np.arange(n))


def check_merge(rows, vals, want_from=None, **kw):
    """merge_rows(sort=True) equals np.unique + np.bincount as it comes
    off the device."""
    import torch
    uniq, inv = np.unique(rows if want_from is None else want_from,
                          axis=0, return_inverse=True)
    want = np.bincount(inv.reshape(-1), weights=vals,
                       minlength=uniq.shape[0])
    got_rows, got_sums, exact = ops().merge_rows(
        torch.from_numpy(rows).cuda(), torch.from_numpy(vals).cuda(),
        rows.shape[1] - 1, sort=True, **kw)
    assert got_rows.is_cuda and got_sums.is_cuda
    assert np.array_equal(got_rows.cpu().numpy(), uniq)
    assert np.array_equal(got_sums.cpu().numpy(), want)
    assert exact is True


@pytest.mark.parametrize("nk", [1, 8])
@pytest.mark.parametrize("n", [1, 257, 3 * 256 + 5])
def test_merge_sorted(nk, n):
    rows = np.ascontiguousarray(drawn(n, nk + 1, seed=10 * nk + n))
    check_merge(rows, (np.arange(n) % 1000 + 1).astype(np.float64))


def test_merge_sorted_multi_tile():
    """2T + 3 distinct rows: the multi-tile passes behind merge_rows."""
    n = 2 * tile() + 3
    rows = np.random.default_rng(11).integers(
        I64.min, I64.max, size=(n, 3), endpoint=True)
    rows[:, 1] = np.arange(n)  # distinct for certain
    check_merge(rows, np.ones(n))


def test_merge_sorted_segments():
    """The segmented, remapped input of test_gpu_merge_rows.segmented():
    the order is by the global codes, after the remap."""
    import torch
    rng = np.random.default_rng(21)
    sizes = [300, 0, 417]
    n = sum(sizes)
    draw = rng.integers(0, 15, size=(n, 3))
    rows = np.stack([draw[:, 0] % 5, draw[:, 1] % 3,
                     (np.arange(n) % 2 == 0) * EL_STR], axis=1)
    remaps = [np.array([3, 0, 4, 1, 2]), np.zeros(0, np.int64),
              np.array([1, 4, 2, 0, 3])]
    mapped = rows.copy()
    is_str = rows[:, 2] == EL_STR
    for lo, hi, remap in ((0, 300, remaps[0]), (300, n, remaps[2])):
        seg, s = mapped[lo:hi], is_str[lo:hi]
        seg[s, 0] = remap[seg[s, 0]]
    check_merge(
        rows, (draw[:, 2] + 1).astype(np.float64), want_from=mapped,
        seg_start=torch.tensor(np.concatenate([[0], np.cumsum(sizes)])),
        remap=torch.from_numpy(np.concatenate(remaps)).cuda(),
        remap_off=torch.tensor([0, 5, 5, 10]))


@pytest.mark.parametrize("bad", ["cpu", "int32", "wide"])
def test_bad_input_is_rejected(bad):
    import torch
    o = ops()
    rows = {"cpu": torch.zeros(4, 2, dtype=torch.int64),
            "int32": torch.zeros(4, 2, dtype=torch.int32, device="cuda"),
            "wide": torch.zeros(4, o.MAX_KEY + 2, dtype=torch.int64,
                                device="cuda")}[bad]
    with pytest.raises(RuntimeError):
        o.sort_rows(rows)

"""
unify_strings (ops/hip/unify_strings.h): number the distinct byte strings
among spans of a blob in order of first occurrence, against a Python dict
loop.  Integers and bytes only, so every comparison is for equality.

All tests here require an MI355X (pytest -m gpu).
"""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LENGTHS = [0, 1, 7, 8, 9, 15, 16, 17, 40]


def ops():
    from dragnet_amd.ops import load_ops
    return load_ops(required=True)


def reference(strings):
    ids, remap, first = {}, [], []
    for i, s in enumerate(strings):
        if s not in ids:
            ids[s] = len(first)
            first.append(i)
        remap.append(ids[s])
    return np.array(remap, np.int64), np.array(first, np.int64)


def packed(strings):
    """(blob, start, length) with the strings back to back, ascending."""
    length = np.array([len(s) for s in strings], np.int64)
    start = np.cumsum(length) - length
    return np.frombuffer(b"".join(strings), np.uint8).copy(), start, length


def check(strings, blob, start, length, **kw):
    import torch
    remap, first = ops().unify_strings(
        torch.from_numpy(blob).cuda(),
        torch.from_numpy(np.ascontiguousarray(start)).cuda(),
        torch.from_numpy(np.ascontiguousarray(length)).cuda(), **kw)
    remap, first = remap.cpu().numpy(), first.cpu().numpy()
    want_remap, want_first = reference(strings)
    assert remap.dtype == np.int64 and first.dtype == np.int64
    assert (np.diff(first) > 0).all()
    assert np.array_equal(first, want_first)
    assert np.array_equal(remap, want_remap)


def drawn(n, seed):
    """n strings drawn with replacement from a pool of n // 4 + 1.  Pool
    entry k has length LENGTHS[k % 9]; each run of 18 entries is cut from
    one 40-byte master, so it holds prefixes of one another and, in its
    second half, the same strings with the last byte changed."""
    rng = np.random.default_rng(seed)
    pool = []
    for k in range(n // 4 + 1):
        if k % 18 == 0:
            master = rng.integers(0, 256, size=40, dtype=np.uint8)
        s = master[:LENGTHS[k % 9]].copy()
        if k % 18 >= 9 and s.size:
            s[-1] ^= 1
        pool.append(s.tobytes())
    return [pool[k] for k in rng.integers(0, len(pool), size=n)]


@pytest.mark.parametrize("tiles,plus", [
    (0, 1), (0, 63), (0, 64), (0, 65), (1, -1), (1, 0), (1, 1), (3, 5)])
def test_sizes_and_lengths(tiles, plus):
    """n = tiles * UNIFY_TILE + plus packed, ascending spans (the staged
    path): wave and tile edges, every length around the 8-byte step."""
    n = tiles * ops().UNIFY_TILE + plus
    strings = drawn(n, seed=n)
    check(strings, *packed(strings))


@pytest.mark.parametrize("max_blocks", [1, 0])
def test_lowest_index_wins_in_any_order(max_blocks):
    """The last two tiles repeat the first: one block takes the tiles in
    order, many blocks in any order, and both number them alike."""
    T = ops().UNIFY_TILE
    strings = drawn(3 * T + 5, seed=11)
    strings[2 * T:3 * T] = strings[:T][::-1]
    strings[3 * T:] = strings[:5]
    check(strings, *packed(strings), max_blocks=max_blocks)


@pytest.mark.parametrize("hash_mask", [0, 3])
def test_equal_hashes(hash_mask):
    """One hash value, then four: length and bytes alone decide, along
    chains from one and from four home slots."""
    strings = drawn(300, seed=12)
    check(strings, *packed(strings), hash_mask=hash_mask)


def descending():
    strings = drawn(3 * ops().UNIFY_TILE + 5, seed=13)
    blob, start, length = packed(strings)
    return strings[::-1], blob, start[::-1], length[::-1]


def overlapping():
    """Sub-spans of one 64-byte run of period 8: equal strings at
    different places and alignments."""
    run = np.tile(np.arange(1, 9, dtype=np.uint8), 8)
    start = np.arange(300, dtype=np.int64) % 57
    length = (np.arange(300, dtype=np.int64) * 7) % (64 - start)
    strings = [run[s:s + n].tobytes() for s, n in zip(start, length)]
    return strings, run, start, length


def long_string():
    """Two tiles, each with one string beyond the stage; a third copy
    differs in its last byte."""
    T = ops().UNIFY_TILE
    rng = np.random.default_rng(14)
    big = rng.integers(0, 256, size=ops().UNIFY_STAGE_BYTES + 9,
                       dtype=np.uint8)
    strings = drawn(T + 5, seed=14)
    strings[3] = strings[T + 1] = big.tobytes()
    big[-1] ^= 1
    strings[7] = big.tobytes()
    return (strings,) + packed(strings)


@pytest.mark.parametrize("case", [descending, overlapping, long_string])
def test_unstaged_path(case):
    check(*case())


def test_empty_input():
    import torch
    none = torch.zeros(0, dtype=torch.int64).cuda()
    remap, first = ops().unify_strings(
        torch.zeros(4, dtype=torch.uint8).cuda(), none, none)
    assert remap.shape == (0,) and first.shape == (0,)
    assert remap.is_cuda and first.is_cuda


@pytest.mark.parametrize("case", [
    "cpu", "int32", "unequal", "past_the_end", "negative"])
def test_bad_input(case):
    import torch
    blob = torch.arange(10, dtype=torch.uint8).cuda()
    start = torch.tensor([0, 4]).cuda()
    length = torch.tensor([4, 6]).cuda()
    if case == "cpu":
        start = start.cpu()
    elif case == "int32":
        start = start.to(torch.int32)
    elif case == "unequal":
        length = length[:1].contiguous()
    elif case == "past_the_end":
        length[1] = 7
    elif case == "negative":
        length[0] = -1
    with pytest.raises(RuntimeError):
        ops().unify_strings(blob, start, length)


def test_reaggregate_gpu_equals_host(monkeypatch):
    """Dictionaries as (blob, offs) on the GPU, the middle part empty:
    same keys, values and insertion order as the host paths."""
    import torch

    from dragnet_amd.merge import (_encode_table, _strings_blob,
                                   reaggregate)
    from dragnet_amd.points import Aggregator
    from dragnet_amd.query import query_load
    q = query_load(breakdown_specs="a,b")
    tables = [{("GET", 200): 3, ("PUT", 200): 1, ("", 404): 2},
              {},
              {("PUT", 200): 10, ("HEAD", 1): 5, ("GET", 200): 4}]
    parts, pairs = [], []
    for table in tables:
        agg = Aggregator(q)
        agg.table.update(table)
        codes, tags, vals, strs = _encode_table(agg, 2)
        parts.append((codes, tags, vals))
        blob, offs = _strings_blob(strs)
        pairs.append((
            torch.from_numpy(np.frombuffer(blob, np.uint8).copy()).cuda(),
            torch.from_numpy(offs).cuda()))
    monkeypatch.setenv("DRAGNET_UNIFY_GPU", "0")
    monkeypatch.setenv("DRAGNET_MERGE_GPU", "0")
    want = reaggregate(q, parts, pairs)
    monkeypatch.setenv("DRAGNET_UNIFY_GPU", "1")
    monkeypatch.setenv("DRAGNET_MERGE_GPU", "1")
    got = reaggregate(q, parts, pairs)
    assert list(got.table.items()) == list(want.table.items())
    assert got.table[("GET", 200)] == 7 and got.table[("", 404)] == 2

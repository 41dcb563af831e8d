"""
reaggregate (the step after the multi-rank gather) on the host path
equals _rebuild_table over the parts remapped and concatenated by hand.
"""

import numpy as np
import pytest

from dragnet_amd.merge import (_EL_STR, _encode_table, _rebuild_table,
                               reaggregate)
from dragnet_amd.points import Aggregator
from dragnet_amd.query import query_load

# per rank: key (cut to the query's nk columns) -> value; the ranks
# share some string keys, differ in others, and mix int and str elements
RANKS = [
    {("GET", 200, "a"): 3, ("PUT", 200, "b"): 1, (7, 404, "a"): 2},
    {("PUT", 200, "b"): 10, ("GET", 200, "a"): 4, ("HEAD", 1, "c"): 5},
    {(7, 404, "a"): 1.5, ("DELETE", "x", "GET"): 8, ("GET", 200, "a"): 1},
]


@pytest.mark.parametrize("nk", [0, 1, 3])
def test_reaggregate_host_equals_rebuild(nk, monkeypatch):
    monkeypatch.setenv("DRAGNET_MERGE_GPU", "0")
    q = query_load(breakdown_specs=",".join("abc"[:nk]) or None)
    parts, strings_per_part = [], []
    for table in RANKS:
        agg = Aggregator(q)
        for k, v in table.items():
            agg.table[k[:nk]] = agg.table.get(k[:nk], 0) + v
        codes, tags, vals, strings = _encode_table(agg, nk)
        parts.append((codes, tags, vals))
        strings_per_part.append(strings)

    # by hand: global dictionary in first-seen order, numpy remap
    gstrings = []
    for strings in strings_per_part:
        gstrings += [s for s in strings if s not in gstrings]
    hand = []
    for (codes, tags, _v), strings in zip(parts, strings_per_part):
        codes = codes.copy()
        for i in range(codes.shape[0]):
            for j in range(nk):
                if (tags[i] >> (2 * j)) & 3 == _EL_STR:
                    codes[i, j] = gstrings.index(strings[codes[i, j]])
        hand.append(codes)
    want = _rebuild_table(q, np.concatenate(hand),
                          np.concatenate([p[1] for p in parts]),
                          np.concatenate([p[2] for p in parts]), gstrings)

    got = reaggregate(q, parts, strings_per_part)
    assert list(got.table.items()) == list(want.table.items())
    assert len(got.table) == len({k[:nk] for t in RANKS for k in t})


# (mode, threshold) -> the decision at 0, 9 and 10 items when a GPU is
# visible; without one every decision is False.  "0" never, "1" always
# (there is something to do), otherwise from the threshold up, where
# unset or unparsable is infinity.
_NEVER, _ALWAYS, _FROM_10 = (False,) * 3, (False, True, True), \
    (False, False, True)
POLICY = {
    (None, None): _NEVER, (None, "abc"): _NEVER, (None, "10"): _FROM_10,
    ("0", None): _NEVER, ("0", "abc"): _NEVER, ("0", "10"): _NEVER,
    ("1", None): _ALWAYS, ("1", "abc"): _ALWAYS, ("1", "10"): _ALWAYS,
    ("auto", None): _NEVER, ("auto", "abc"): _NEVER,
    ("auto", "10"): _FROM_10,
}


@pytest.mark.parametrize("cuda", [False, True])
@pytest.mark.parametrize("knobs", ["merge", "unify"])
def test_path_policy_table(knobs, cuda, monkeypatch):
    """The one path policy decides for both knob pairs what the two
    separate functions decided; nk == 0, an empty table and a
    list-of-str dictionary stay on the host whatever the mode."""
    import torch

    from dragnet_amd.merge import _merge_on_gpu, _unify_on_gpu
    monkeypatch.setattr(torch.cuda, "is_available", lambda: cuda)
    wire = [(np.zeros(4, dtype=np.uint8), np.arange(3, dtype=np.int64))]
    if knobs == "merge":
        mode_var, thr_var = "DRAGNET_MERGE_GPU", "DRAGNET_MERGE_GPU_ROWS"

        def decide(count):
            return _merge_on_gpu(count, 2)
    else:
        mode_var, thr_var = "DRAGNET_UNIFY_GPU", "DRAGNET_UNIFY_GPU_STRINGS"

        def decide(count):
            return _unify_on_gpu(wire, count)
    for (mode, thr), want in POLICY.items():
        for var, v in ((mode_var, mode), (thr_var, thr)):
            if v is None:
                monkeypatch.delenv(var, raising=False)
            else:
                monkeypatch.setenv(var, v)
        got = tuple(decide(count) for count in (0, 9, 10))
        assert got == tuple(cuda and w for w in want), (mode, thr)
        # whatever the mode: a scalar table, strings already on the host
        assert _merge_on_gpu(10, 0) is False
        assert _merge_on_gpu(0, 2) is False
        assert _unify_on_gpu([["a", "b"]], 10) is False
        assert _unify_on_gpu(wire + [["a"]], 10) is False

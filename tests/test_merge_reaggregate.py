"""
reaggregate (the step after the multi-rank gather) on the host path
equals _rebuild_table over the parts remapped and concatenated by hand.
"""

import numpy as np
import pytest

from dragnet_amd.distributed import (_EL_STR, _encode_table,
                                     _rebuild_table, reaggregate)
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

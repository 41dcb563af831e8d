"""
merge.unify_dictionaries, host path: dictionaries in the wire form
(blob, offs) give what the decoded lists give, through the seam and
through reaggregate.
"""

import numpy as np
import pytest

from dragnet_amd.merge import (_encode_table, _strings_blob, reaggregate,
                               unify_dictionaries)
from dragnet_amd.points import Aggregator
from dragnet_amd.query import query_load

DICTS = [["GET", "naïve", "日本語", ""], [], ["日本語", "PUT", "GET", "naive"]]


def pair(strings, as_torch):
    blob, offs = _strings_blob(strings)
    blob = np.frombuffer(blob, dtype=np.uint8).copy()
    if as_torch:
        import torch
        return torch.from_numpy(blob), torch.from_numpy(offs)
    return blob, offs


@pytest.mark.parametrize("as_torch", [False, True])
def test_pairs_equal_lists(as_torch):
    want_strings, want_remaps = unify_dictionaries(DICTS)
    assert want_strings == ["GET", "naïve", "日本語", "", "PUT", "naive"]
    got_strings, got_remaps = unify_dictionaries(
        [pair(d, as_torch) for d in DICTS])
    assert got_strings == want_strings
    assert len(got_remaps) == len(DICTS)
    for got, want in zip(got_remaps, want_remaps):
        assert got.dtype == np.int64 and np.array_equal(got, want)


def test_reaggregate_pairs_equal_lists():
    q = query_load(breakdown_specs="a,b")
    tables = [{("naïve", 200): 3, ("日本語", 200): 1, (7, 404): 2},
              {},
              {("日本語", 200): 10, ("naïve", 200): 4, ("naive", 1): 5}]
    parts, lists = [], []
    for table in tables:
        agg = Aggregator(q)
        agg.table.update(table)
        codes, tags, vals, strs = _encode_table(agg, 2)
        parts.append((codes, tags, vals))
        lists.append(strs)
    want = reaggregate(q, parts, lists)
    got = reaggregate(q, parts, [pair(s, False) for s in lists])
    assert list(got.table.items()) == list(want.table.items())
    assert got.table[("日本語", 200)] == 11

"""
The host form of merge.encode_table and a WireTable through
distributed.merge_tables_tensor: the merge of a rank's wire table is the
merge of its Aggregator.  No GPU: wire tables are plain arrays.
"""

import numpy as np

from dragnet_amd import merge
from dragnet_amd.points import Aggregator
from dragnet_amd.query import query_load


def test_merge_tables_tensor_takes_a_wire_table(tmp_path, monkeypatch):
    import torch
    import torch.distributed as dist

    from dragnet_amd.distributed import merge_tables_tensor
    monkeypatch.setenv("DRAGNET_ENCODE_GPU", "0")
    q = query_load(breakdown_specs="m,lat[aggr=lquantize,step=10]")
    agg = Aggregator(q)
    agg.table = {("GET", 3): 5, ("null", -2): 1.5, ("café", 2**70): 2}
    agg.ninputs, agg.ndropped_nonnumeric = 9, 1
    w = merge.encode_table(agg, q)
    assert w.codes.shape == (3, 2) and w.strings[0].dtype == np.uint8
    # as the device form leaves it: torch tensors, a string named twice,
    # a key in two rows
    blob, offs = w.strings
    twice = merge.WireTable(
        torch.from_numpy(np.concatenate([w.codes, w.codes[:1]])),
        torch.from_numpy(np.concatenate([w.tagpack, w.tagpack[:1]])),
        torch.from_numpy(np.concatenate([w.vals, [7.0]])),
        (torch.from_numpy(np.concatenate([blob, blob[:3]])),
         torch.from_numpy(np.concatenate([offs, offs[-1:] + 3]))), 9, 1)
    dist.init_process_group(
        "gloo", init_method="file://%s" % (tmp_path / "pg"), rank=0,
        world_size=1)
    try:
        want = merge_tables_tensor(agg, q)
        got = merge_tables_tensor(w, q)
        both = merge_tables_tensor(twice, q)
    finally:
        dist.destroy_process_group()
    assert got.table == want.table == agg.table
    assert (got.ninputs, got.ndropped_nonnumeric) == (9, 1)
    assert both.table == {**agg.table, ("GET", 3): 12}

"""
merge.reaggregate_points on the host path: reaggregate with
render_points in place of _decode_rows gives the NDJSON that
output.point_json gives for reaggregate(...).points().
"""

import numpy as np
import pytest

from dragnet_amd import merge
from dragnet_amd.output import point_json
from dragnet_amd.query import query_load

S, I = merge._EL_STR, merge._EL_INT
CASES = {
    "strings": ("a,b", [S | S << 2, S | S << 2],
                [[[0, 1], [1, 0], [0, 1]], [[0, 0]]],
                [["x", 'y"é'], ["y\"é", "x"]]),
    "date and lquantize": (
        "p,ts[date,field=time],lat[aggr=lquantize,step=10]",
        [S | I << 2 | I << 4] * 2,
        [[[0, -86400000, -3], [0, 0, 7]], [[0, 0, 7], [1, 5, 2**40]]],
        [["GET"], ["GET", "PUT"]]),
    "scalar": ("", [0, 0], [np.zeros((2, 0)), np.zeros((3, 0))], [[], []]),
}


def parts_of(case):
    spec, tags, codes, dicts = CASES[case]
    parts = [(np.asarray(c, dtype=np.int64), np.full(len(c), t, np.int64),
              np.arange(1.0, len(c) + 1)) for c, t in zip(codes, tags)]
    return query_load(breakdown_specs=spec), parts, dicts


@pytest.mark.parametrize("case", sorted(CASES))
@pytest.mark.parametrize("mode", ["0", None])
def test_reaggregate_points_is_reaggregate_rendered(monkeypatch, case, mode):
    # mode None: auto with no threshold set never leaves the host, so no
    # extension is loaded and no GPU is asked for
    monkeypatch.delenv("DRAGNET_RENDER_GPU_ROWS", raising=False)
    if mode is None:
        monkeypatch.delenv("DRAGNET_RENDER_GPU", raising=False)
        monkeypatch.setattr(merge, "_render_device", None)
    else:
        monkeypatch.setenv("DRAGNET_RENDER_GPU", mode)
    q, parts, dicts = parts_of(case)
    want = "".join(point_json(p) + "\n" for p in
                   merge.reaggregate(q, parts, dicts).points()).encode()
    assert want and merge.reaggregate_points(q, parts, dicts) == want

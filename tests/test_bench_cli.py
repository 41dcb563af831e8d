"""
bench.py host-side plumbing (no GPU): the seeded pool is the same bytes
however many workers generate it, and --dump-outputs writes the
aggregate in the documented .npy layout.
"""

import json
import os
import sys

import numpy as np

REPO_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO_ROOT not in sys.path:
    sys.path.insert(0, REPO_ROOT)

import bench  # noqa: E402


def test_pool_is_seeded_and_worker_independent(monkeypatch):
    monkeypatch.setattr(bench, "SLAB_MB", 1)
    serial, nrec = bench.build_pool(3, seed=1000, workers=1)
    forked, nrec2 = bench.build_pool(3, seed=1000, workers=3)
    assert serial == forked and nrec == nrec2
    assert len(serial) >= 3 << 20
    assert serial.endswith(b"\n") and serial.count(b"\n") == nrec
    other, _ = bench.build_pool(3, seed=1001, workers=1)
    assert other != serial
    # slabs are distinct draws, not one slab repeated
    assert serial[:1 << 19] != serial[1 << 20:(1 << 20) + (1 << 19)]
    for line in serial[:4096].split(b"\n")[:8]:
        rec = json.loads(line)
        assert "method" in rec["req"] and "statusCode" in rec["res"]


def test_dump_outputs_layout(tmp_path):
    from dragnet_amd.points import Aggregator
    from dragnet_amd.query import query_load
    q = query_load(filter={"eq": ["req.method", "GET"]},
                   breakdown_specs="req.method,res.statusCode")
    agg = Aggregator(q)
    for code, n in ((404, 5), (200, 7)):
        agg.write({"fields": {"req": {"method": "GET"},
                              "res": {"statusCode": code}}, "value": n})
    out = str(tmp_path / "dump")
    bench.dump_outputs(out, agg)
    assert sorted(os.listdir(out)) == ["point_keys.npy",
                                       "point_values.npy"]
    keys = np.load(os.path.join(out, "point_keys.npy"))
    vals = np.load(os.path.join(out, "point_values.npy"))
    assert keys.dtype == np.float64 and vals.dtype == np.float64
    assert vals.tolist() == [7.0, 5.0]  # points() order: sorted keys
    texts = [bytes(row.astype(np.uint8)).rstrip(b"\0").decode()
             for row in keys]
    assert [json.loads(t) for t in texts] == \
        [p["fields"] for p in agg.points()]

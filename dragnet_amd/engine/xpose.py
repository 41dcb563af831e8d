"""
Wave-transposed staging for scan_kernel_x (prototype; DRAGNET_XPOSE):
records length-sorted (aggregation is order-independent), 64
consecutive sorted records form a wave, each record's bytes split into
granules interleaved so granule g of lane l sits at
wave_base + g*64*gran + l*gran — a wave's window refills touch 64
CONSECUTIVE granules (coalesced) instead of 64 scattered records.

Both builders return (xdata, wave_base, rec_len, n_slots), the
arguments of ScanState.scan_xpose.
"""

import numpy as np


def build_on_device(torch, ops, dev_data, pos, nlines, gran):
    """Build the layout ON DEVICE from a resident pool and its full
    line index (torch sort + cumsum + the xpose_build_kernel scatter):
    no host staging pass."""
    dev = dev_data.device
    glog = gran.bit_length() - 1
    nrec = int(nlines.item())  # one-time staging sync
    if nrec == 0:
        raise ValueError("no records")
    pos = pos[:nrec].to(torch.int64)
    starts = torch.empty_like(pos)
    starts[0] = 0
    starts[1:] = pos[:-1] + 1
    lens_sorted, order = torch.sort(pos - starts)
    starts_sorted = starts[order]
    nslots = (nrec + 63) & ~63
    nw = nslots // 64
    slot_len = torch.full((nslots,), -1, dtype=torch.int32,
                          device=dev)
    slot_len[:nrec] = lens_sorted.to(torch.int32)
    sstart = torch.zeros(nslots, dtype=torch.int32, device=dev)
    sstart[:nrec] = starts_sorted.to(torch.int32)
    # per-wave granule count from each wave's longest (last) lane
    last = torch.clamp(
        torch.arange(nw, device=dev, dtype=torch.int64) * 64 + 63,
        max=nrec - 1)
    gwl = torch.clamp((lens_sorted[last] + gran - 1) // gran, min=1)
    stride = 64 * gran
    wbase = torch.zeros(nw + 1, dtype=torch.int64, device=dev)
    torch.cumsum(gwl * stride, 0, out=wbase[1:])
    total = int(wbase[-1].item()) + stride  # +slack
    xb = torch.empty(total, dtype=torch.uint8, device=dev)
    ops.xpose_build(dev_data, sstart, slot_len, wbase, nslots, glog, xb)
    # the kernel reads wave_base[0, nw); the +1 entry is harmless
    return xb, wbase, slot_len, nslots


def build_on_host(torch, buf, gran, dev):
    """r1 host-side numpy builder (kept for A/B and layout tests)."""
    xb, wave_base, slot_len, nslots, _n = _build_xpose_layout(buf, gran)
    return (torch.from_numpy(xb).to(dev),
            torch.from_numpy(wave_base).to(dev),
            torch.from_numpy(slot_len.view(np.int32)).to(dev),
            nslots)


def _build_xpose_layout(buf, gran=64):
    """Numpy construction of the wave-transposed layout: returns (xbuf,
    wave_base, slot_len, n_slots, n_records).  Byte p of slot r lives at
    wave_base[r//64] + (p//gran)*(64*gran) + (r%64)*gran + p%gran."""
    stride = 64 * gran
    arr = np.frombuffer(buf, dtype=np.uint8)
    nl = np.flatnonzero(arr == 10).astype(np.int64)
    if nl.size == 0:
        raise ValueError("no records")
    starts = np.empty_like(nl)
    starts[0] = 0
    starts[1:] = nl[:-1] + 1
    lens = (nl - starts).astype(np.int64)
    n = int(lens.size)
    order = np.argsort(lens, kind="stable")
    nslots = (n + 63) & ~63
    nw = nslots // 64
    so = starts[order]
    lo = lens[order]
    # per-wave granule count: lengths are sorted, so a wave's max is
    # its last real lane; the granule-row stride is a constant 4096
    # (64 lanes x 64B), so variable wave sizes need no device change
    last = np.minimum(np.arange(nw) * 64 + 63, n - 1)
    gw = np.maximum(1, (lo[last] + gran - 1) // gran).astype(np.int64)
    wave_base = np.zeros(nw, dtype=np.int64)
    np.cumsum(gw[:-1] * stride, out=wave_base[1:])
    total = int(wave_base[-1] + gw[-1] * stride) + stride  # +slack
    xb = np.full(total, 10, dtype=np.uint8)
    # build waves in batches of equal granule count (few distinct
    # values after sorting) with one vectorized gather per batch
    for g in np.unique(gw):
        ws = np.flatnonzero(gw == g)
        K = int(g) * gran
        rsel = (ws[:, None] * 64 + np.arange(64)[None, :]).reshape(-1)
        rl = np.where(rsel < n, lo[np.minimum(rsel, n - 1)], 0)
        rs = np.where(rsel < n, so[np.minimum(rsel, n - 1)], 0)
        idx = rs[:, None] + np.arange(K)[None, :]
        np.minimum(idx, arr.size - 1, out=idx)
        m = arr[idx]
        m[np.arange(K)[None, :] >= rl[:, None]] = 10
        # (wave, lane, granule, 64) -> (wave, granule, lane, 64)
        blk = np.ascontiguousarray(
            m.reshape(len(ws), 64, int(g), gran).transpose(0, 2, 1, 3)
        ).reshape(len(ws), -1)
        for i, w in enumerate(ws):
            b = int(wave_base[w])
            xb[b:b + K * 64] = blk[i]
    slot_len = np.full(nslots, 0xFFFFFFFF, dtype=np.uint32)
    slot_len[:n] = lo.astype(np.uint32)
    return xb, wave_base, slot_len, nslots, n

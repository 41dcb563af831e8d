"""
Host-side chunk framing for file scans: no torch, no GPU.  The GPU
engine (engine/gpu._ScanContext.scan_files) passes memoryviews of its
pinned tensors and submits each yielded chunk; tests pass bytearrays.
"""

import concurrent.futures as cf
import os
import stat


def _pad(n):
    """Pad a chunk length so the cursor's 8-byte windows never read
    past the buffer (>= 8 bytes of newline slack, 16B aligned)."""
    return (n + 16 + 15) & ~15


def choose_chunk_bytes(total, engine_bytes, env_set):
    """Chunk size for a file scan of `total` bytes: 1 GiB amortizes
    per-chunk overhead on big corpora (+~10% at 24 readers); small
    scans, and any with DRAGNET_CHUNK_MB set, keep the engine's value."""
    if not env_set and total > (16 << 30):
        return 1 << 30
    return engine_bytes


def _pread_full(fd, mv, off):
    """preadv until mv is full (a single preadv may legally return
    short; a short section would leave a HOLE of stale bytes that
    corrupts record framing — observed at the multi-GB scale)."""
    done = 0
    while done < len(mv):
        got = os.preadv(fd, [mv[done:]], off + done)
        if got <= 0:
            break
        done += got
    return done


def _open(path):
    """[file, pos, size]; size is None for anything but a regular file
    (char device, pipe), which is read sequentially."""
    f = open(path, "rb", buffering=0)
    st = os.fstat(f.fileno())
    return [f, 0, st.st_size if stat.S_ISREG(st.st_mode) else None]


def _read(f, view, pool, readers, parallel_min):
    """Read f into view -> contiguous bytes read, 0 at end of file.
    Regular-file reads of parallel_min bytes or more go as `readers`
    parallel preadv sections (one core reads page cache at ~10 GB/s)."""
    fobj, fpos, fsize = f
    if fsize is None:
        return fobj.readinto(view) or 0
    fd = fobj.fileno()
    view = view[:max(0, fsize - fpos)]
    if len(view) < parallel_min:
        return _pread_full(fd, view, fpos)
    sec = (len(view) + readers - 1) // readers
    futs = [pool.submit(_pread_full, fd, view[s:s + sec], fpos + s)
            for s in range(0, len(view), sec)]
    total = 0
    for fut in futs:
        got = fut.result()
        total += got
        if got < sec:  # only the contiguous prefix counts
            break
    return total


def _last_newline(buf, n):
    probe = max(0, n - (1 << 16))
    cut = bytes(buf[probe:n]).rfind(b"\n")
    if cut >= 0:
        return probe + cut
    return bytes(buf[:probe]).rfind(b"\n")


def frame_files(files, views, cap, wait, readers=24,
                parallel_min=8 << 20):
    """Yield (buf_index, n): views[buf_index][:n] holds whole records
    and ends in '\\n'.

    `views` is two writable buffers of at least _pad(cap) bytes.  Files
    are concatenated byte-wise (one without a trailing newline runs
    into the next); one '\\n' is appended at end of input if missing.
    Each buffer is filled to `cap` and cut at its last newline; the
    tail is carried into the head of the other buffer.  `wait(i)` is
    called before anything is written into buffer i (refill or tail
    carry); the consumer may overwrite the bytes past n."""
    views = [memoryview(v) for v in views]  # slices must alias
    pool = cf.ThreadPoolExecutor(max_workers=readers)
    files = iter(files)
    f = None
    cur, head, eof = 0, 0, False
    try:
        while not eof:
            wait(cur)
            n = head
            while n < cap:
                if f is None:
                    path = next(files, None)
                    if path is None:
                        eof = True
                        break
                    f = _open(path)
                got = _read(f, views[cur][n:cap], pool, readers,
                            parallel_min)
                if got <= 0:
                    f[0].close()
                    f = None
                    continue
                f[1] += got
                n += got
            if n == 0:
                break
            cut = _last_newline(views[cur], n)
            if eof and cut < n - 1:
                views[cur][n:n + 1] = b"\n"
                n += 1
                cut = n - 1
            if cut < 0:
                # a buffer starts at a record start, so it is full
                # without a newline only when one record fills it
                raise RuntimeError(
                    "record exceeds the chunk buffer (%d bytes); "
                    "raise DRAGNET_CHUNK_MB" % cap)
            head = n - (cut + 1)
            # carried BEFORE the chunk is yielded: the consumer pads
            # views[cur][cut+1:] with newlines and would clobber the tail
            # (record-splitting corruption observed at multi-GB scale)
            if head:
                wait(1 - cur)
                views[1 - cur][:head] = views[cur][cut + 1:n]
            yield cur, cut + 1
            cur = 1 - cur
    finally:
        if f is not None:
            f[0].close()
        pool.shutdown(wait=False)

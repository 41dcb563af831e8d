"""Host chunk framing (engine/chunks.py): CPU-only, no torch.

The framer must hand the engine chunks of whole records whose bytes,
joined, are exactly the input files' bytes (plus one final newline if
missing) — through short reads, buffer reuse, the consumer's newline
padding, and non-regular inputs."""

import os
import random
import threading

import pytest

from dragnet_amd.engine.chunks import (_pad, choose_chunk_bytes,
                                       frame_files)

TOO_LONG = "record exceeds the chunk buffer"


def write_files(tmp_path, contents, tag="f"):
    paths = []
    for i, data in enumerate(contents):
        p = tmp_path / ("%s%d.log" % (tag, i))
        p.write_bytes(data)
        paths.append(str(p))
    return paths


def expected(contents):
    data = b"".join(contents)
    if data and not data.endswith(b"\n"):
        data += b"\n"
    return data


def run(paths, cap, parallel_min=8 << 20, clobber=False, readers=4):
    """Frame `paths`; returns the list of chunks.  clobber=True pads
    past each chunk with newlines like the engine's submit path."""
    views = [bytearray(_pad(cap) + 64) for _ in range(2)]
    chunks = []
    for i, n in frame_files(paths, views, cap, lambda i: None,
                            readers=readers, parallel_min=parallel_min):
        chunks.append(bytes(views[i][:n]))
        if clobber:
            views[i][n:_pad(n)] = b"\n" * (_pad(n) - n)
    return chunks


def check(chunks, contents, cap):
    assert b"".join(chunks) == expected(contents)
    for c in chunks:
        assert c.endswith(b"\n")
        assert len(c) <= cap + 1


def random_case(rng):
    """0-4 files of 0-30 records with 0-60 byte bodies; 70% of files
    end in a newline.  A file that does not runs into the next one, so
    a record joined across files may be longer than 60 bytes: the
    generator keeps those under 80, which lets cap 64 reach the error
    branch while caps 80 and 257 never may."""
    contents = []
    open_len = 0  # unterminated bytes at the end of the files so far
    for _ in range(rng.randint(0, 4)):
        recs = []
        for _ in range(rng.randint(0, 30)):
            room = 79 - open_len if not recs else 60
            recs.append(bytes(rng.choice(b"abcxyz{}\": 01") for _ in
                              range(rng.randint(0, min(60, room)))))
        data = b"\n".join(recs)
        if recs and rng.random() < 0.7:
            data += b"\n"
        if recs:
            open_len = 0 if data.endswith(b"\n") else \
                len(recs[-1]) + (open_len if len(recs) == 1 else 0)
        contents.append(data)
    return contents


def test_property_seeded(tmp_path):
    rng = random.Random(20240)
    raised = 0
    for case in range(300):
        contents = random_case(rng)
        paths = write_files(tmp_path, contents)
        longest = max(len(r) for r in
                      b"".join(contents).split(b"\n"))
        for cap in (64, 80, 257):
            for pmin in (8 << 20, 16):
                if longest >= cap:
                    assert cap == 64
                    with pytest.raises(RuntimeError, match=TOO_LONG):
                        run(paths, cap, pmin)
                    raised += 1
                else:
                    check(run(paths, cap, pmin, clobber=True),
                          contents, cap)
    # no cases at all in the error branch would mean it is untested;
    # all of them there would mean nothing else is
    assert 0 < raised < 300


@pytest.mark.parametrize("pmin", [8 << 20, 16])
def test_record_length_boundary(tmp_path, pmin):
    cap = 64
    fits = b"a" * (cap - 1)
    contents = [b"x\nyy\n" + fits + b"\nzz\n"]
    chunks = run(write_files(tmp_path, contents), cap, pmin)
    check(chunks, contents, cap)
    assert fits + b"\n" in chunks  # yielded alone

    paths = write_files(tmp_path, [b"x\n" + b"a" * cap + b"\nzz\n"], "g")
    with pytest.raises(RuntimeError) as ei:
        run(paths, cap, pmin)
    assert str(ei.value) == ("record exceeds the chunk buffer (%d bytes);"
                             " raise DRAGNET_CHUNK_MB" % cap)


def test_padding_does_not_clobber_carried_tail(tmp_path):
    """Regression: the consumer's newline padding after a chunk once
    overwrote the tail bytes, which must already be in the other
    buffer."""
    rng = random.Random(5)
    contents = [b"".join(b"%d:%s\n" % (i, b"r" * rng.randint(0, 50))
                         for i in range(400))]
    paths = write_files(tmp_path, contents)
    for cap in (64, 100, 257):
        check(run(paths, cap, clobber=True), contents, cap)


def test_wait_precedes_every_buffer_write(tmp_path):
    """A yielded buffer belongs to the consumer until wait(i): poison
    it on yield, restore it in wait(i); a write before wait(i) would be
    lost to the restore, a read would see the poison."""
    contents = [b"".join(b"rec-%04d-%s\n" % (i, b"p" * (i % 37))
                         for i in range(300)), b"tail without newline"]
    paths = write_files(tmp_path, contents)
    cap = 96
    views = [bytearray(_pad(cap) + 64) for _ in range(2)]
    saved = [None, None]
    calls = []

    def wait(i):
        calls.append(i)
        if saved[i] is not None:
            # the framer must not have touched the poisoned buffer
            assert views[i] == b"\xff" * len(views[i])
            views[i][:] = saved[i]
            saved[i] = None

    out = []
    for i, n in frame_files(paths, views, cap, wait, readers=4):
        out.append(bytes(views[i][:n]))
        assert saved[i] is None
        saved[i] = bytes(views[i])
        views[i][:] = b"\xff" * len(views[i])
    data = b"".join(out)
    assert b"\xff" not in data
    assert data == expected(contents)
    assert set(calls) == {0, 1} and len(calls) >= len(out)


@pytest.mark.parametrize("pmin", [8 << 20, 16])
def test_short_reads(tmp_path, monkeypatch, pmin):
    real = os.preadv

    def short_preadv(fd, bufs, off):
        (mv,) = bufs
        return real(fd, [mv[:7]], off)

    monkeypatch.setattr(os, "preadv", short_preadv)
    rng = random.Random(11)
    contents = [b"".join(b"%d|%s\n" % (i, b"s" * rng.randint(0, 40))
                         for i in range(120)) for _ in range(3)]
    check(run(write_files(tmp_path, contents), 128, pmin, clobber=True),
          contents, 128)


def test_fifo_input(tmp_path):
    fifo = str(tmp_path / "pipe")
    os.mkfifo(fifo)
    parts = [b"".join(b"fifo-%d\n" % i for i in range(30)),
             b"".join(b"second-%d\n" % i for i in range(20)) + b"end"]

    def writer():
        with open(fifo, "wb", buffering=0) as f:
            for p in parts:
                f.write(p)

    t = threading.Thread(target=writer, daemon=True)
    t.start()
    before = write_files(tmp_path, [b"regular first\nno newline "])
    chunks = run(before + [fifo], 100, clobber=True)
    t.join()
    check(chunks, [b"regular first\nno newline "] + parts, 100)


def test_empty_inputs(tmp_path):
    assert run([], 64) == []
    assert run(write_files(tmp_path, [b"", b"", b""]), 64) == []


def test_descriptors_closed(tmp_path):
    ok = write_files(tmp_path, [b"a\nbb\n" * 40, b"c\n" * 10])
    bad = write_files(tmp_path, [b"a\n" + b"x" * 64 + b"\n", b"c\n"], "g")
    before = sorted(os.listdir("/proc/self/fd"))
    run(ok, 64)
    assert sorted(os.listdir("/proc/self/fd")) == before
    with pytest.raises(RuntimeError, match=TOO_LONG):
        run(bad, 64)
    assert sorted(os.listdir("/proc/self/fd")) == before


def test_choose_chunk_bytes():
    eng = 256 << 20
    assert choose_chunk_bytes(16 << 30, eng, False) == eng
    assert choose_chunk_bytes((16 << 30) + 1, eng, False) == 1 << 30
    assert choose_chunk_bytes((16 << 30) + 1, eng, True) == eng
    assert choose_chunk_bytes(1 << 40, 64 << 20, True) == 64 << 20
    assert choose_chunk_bytes(0, eng, False) == eng

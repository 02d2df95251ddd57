"""CPU tests (-m "not gpu") of the typed sinks (include/xlating_sinks.h: xlating_sinks_attach_file_as, xlating_sinks_write_bytes): cs16
files and gzip files hold exactly the bytes written, at sizes that are no multiple of 8; the cf32 calls behave as before beside them on
one object; an unknown extension is refused; a slow peer of write_bytes is dropped like one of write."""
import errno
import gzip
import os
import socket

import numpy as np

import sdr_server_amd as xl


def _chunks(seed, sizes):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in sizes]


SIZES = [4, 12, 20, 4100, 0, 36, 65540, 4]  # bytes: int16 pairs, totals that are no multiple of 8 along the way


def test_cs16_files_hold_exactly_the_bytes_written(tmp_path):
    s = xl.Sinks(writer_threads=2, queue_bytes=1 << 20)
    assert s.attach_file_as(3, tmp_path, "cs16") == 0
    assert s.attach_file_as(4, tmp_path, "cs16", use_gzip=True) == 0
    want = {3: b"", 4: b""}
    for cid in (3, 4):
        for part in _chunks(cid, SIZES):
            assert s.write_bytes(cid, part) == 0
            want[cid] += part
    assert s.flush() == 0
    assert s.detach(3) == 0 and s.detach(4) == 0
    assert len(want[3]) % 8 == 4
    assert open(tmp_path / "3.cs16", "rb").read() == want[3]
    assert gzip.open(tmp_path / "4.cs16.gz", "rb").read() == want[4]
    assert sorted(os.listdir(tmp_path)) == ["3.cs16", "4.cs16.gz"]
    written, dropped = s.stats()
    assert written == len(want[3]) + len(want[4]) and dropped == 0
    s.close()


def test_cf32_calls_behave_as_before_beside_the_new_ones(tmp_path):
    """attach_file == attach_file_as(..., "cf32"), write == write_bytes(n * 8): the four calls on one object, the files named and filled
    as the old calls alone would"""
    s = xl.Sinks(writer_threads=1, queue_bytes=1 << 20)
    assert s.attach_file(0, tmp_path) == 0
    assert s.attach_file_as(1, tmp_path, "cf32") == 0
    assert s.attach_file(2, tmp_path, use_gzip=True) == 0
    assert s.attach_file_as(5, tmp_path, "cs16") == 0
    assert s.attach_file_as(0, tmp_path, "cs16") == -errno.EEXIST  # (one sink per client, whatever its type)
    rng = np.random.default_rng(9)
    x = (rng.standard_normal(777) + 1j * rng.standard_normal(777)).astype(np.complex64)
    for cid in (0, 1, 2):
        assert s.write(cid, x[:300]) == 0
        assert s.write_bytes(cid, x[300:]) == 0  # (the same bytes by the other call)
    assert s.write_bytes(5, x.view(np.uint8)[:4 * 501]) == 0
    assert s.write(0, np.zeros(0, np.complex64)) == 0 and s.write_bytes(0, b"") == 0
    assert s.write_bytes(77, b"abcd") == -errno.ENOENT
    assert s.flush() == 0
    for cid in (0, 1, 2, 5):
        assert s.detach(cid) == 0
    assert open(tmp_path / "0.cf32", "rb").read() == x.tobytes()
    assert open(tmp_path / "1.cf32", "rb").read() == x.tobytes()
    assert gzip.open(tmp_path / "2.cf32.gz", "rb").read() == x.tobytes()
    assert open(tmp_path / "5.cs16", "rb").read() == x.tobytes()[:4 * 501]
    s.close()


def test_unknown_extension_and_null_arguments_are_refused(tmp_path):
    s = xl.Sinks(writer_threads=1, queue_bytes=4096)
    for ext in ("cu8", "", "cf32.gz", "CS16", "../x"):
        assert s.attach_file_as(1, tmp_path, ext) == -errno.EINVAL
    L = xl.lib()
    assert L.xlating_sinks_attach_file_as(s.h, 1, str(tmp_path).encode(), None, 0) == -errno.EINVAL
    assert L.xlating_sinks_attach_file_as(None, 1, str(tmp_path).encode(), b"cs16", 0) == -errno.EINVAL
    assert L.xlating_sinks_write_bytes(s.h, 1, None, 4) == -errno.EINVAL
    assert L.xlating_sinks_write_bytes(None, 1, None, 0) == -errno.EINVAL
    assert os.listdir(tmp_path) == []
    assert s.attach_file_as(1, tmp_path / "missing", "cs16") == -errno.ENOENT  # (the failed open's errno, as attach_file)
    s.close()


def test_slow_peer_on_write_bytes_is_dropped_like_one_on_write():
    s = xl.Sinks(writer_threads=1, queue_bytes=4 * 25000)
    a, b = socket.socketpair()
    a.setsockopt(socket.SOL_SOCKET, socket.SO_SNDBUF, 4096)
    assert s.attach_fd(5, a.fileno()) == 0
    blk = _chunks(5, [25000])[0]
    codes = [s.write_bytes(5, blk) for _ in range(200)]  # nobody reads from b
    assert codes[0] == 0 and -errno.EPIPE in codes
    assert all(c == -errno.EPIPE for c in codes[codes.index(-errno.EPIPE):])
    assert s.failed() == [5] and s.failed() == []  # reported once
    assert s.stats()[1] == codes.count(-errno.EPIPE)
    assert s.detach(5) == 0
    a.close()
    b.close()
    s.close()

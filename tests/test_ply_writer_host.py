"""CPU: the argument checks of the device PLY formatter (linr_ply_format_ascii, csrc/ply_format.hip), which all come before the
first launch and so run without a GPU, and the thread and queue logic of ply.PlyWriter fed with byte strings through
`submit_bytes`, the seam that takes a payload already on the host."""
import ctypes
import os
import threading

import pytest

MAX_ROWS = (2 ** 31 - 1) // 36


@pytest.fixture(scope='module')
def lib():
    from linr_pcgc_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.lib()


def test_size_functions(lib):
    assert [lib.linr_ply_format_text_bytes(n) for n in (-1, 0, 1, 2, 1000, MAX_ROWS, MAX_ROWS + 1, 1 << 40)] == \
        [0, 0, 36, 72, 36000, 36 * MAX_ROWS, 0, 0]
    assert 36 * MAX_ROWS <= 2 ** 31 - 1 < 36 * (MAX_ROWS + 1)
    assert [lib.linr_ply_format_ws_bytes(n) for n in (-1, 0, MAX_ROWS + 1, 1 << 40)] == [0, 0, 0, 0]
    for n in (1, 255, 256, 100003, MAX_ROWS):
        assert lib.linr_ply_format_ws_bytes(n) >= 4 * (n + 1)          # the n + 1 row offsets, then the scan's scratch


def test_entry_checks_its_arguments_before_any_launch(lib):
    buf = (ctypes.c_char * 8192)()
    p = (ctypes.addressof(buf) + 255) & ~255          # host memory: no call below may get as far as a launch
    n = 40
    cap, ws = lib.linr_ply_format_text_bytes(n), lib.linr_ply_format_ws_bytes(n)
    call = lib.linr_ply_format_ascii
    assert call(None, n, p, cap, p, ws, p, None) == -1
    assert call(p, n, None, cap, p, ws, p, None) == -1
    assert call(p, n, p, cap, None, ws, p, None) == -1
    assert call(p, n, p, cap, p, ws, None, None) == -1
    assert call(p, -1, p, cap, p, ws, p, None) == -1
    assert call(p, MAX_ROWS + 1, p, 1 << 40, p, 1 << 40, p, None) == -1
    assert call(p, 1 << 40, p, 1 << 62, p, 1 << 62, p, None) == -1
    assert call(p, n, p, 36 * n - 1, p, ws, p, None) == -2
    assert call(p, n, p, cap, p, ws - 1, p, None) == -2
    assert call(p, MAX_ROWS, p, cap, p, ws, p, None) == -2          # the largest n is an argument like any other
    assert call(p + 2, n, p, cap, p, ws, p, None) == -3             # xyz: 4-byte aligned
    assert call(p, n, p, cap, p + 128, ws, p, None) == -3           # ws: 256-byte aligned
    assert call(p, n, p, cap, p, ws, p + 4, None) == -3             # text_len: an int64
    assert call(p, 0, p, 0, p, 0, p, None) == 0                     # an empty frame is fine, nothing is launched
    assert call(None, 0, None, 0, None, 0, None, None) == 0
    assert bytes(buf) == bytes(8192)


def test_device_paths_refuse_what_they_cannot_format():
    import numpy as np
    import torch
    from linr_pcgc_amd import ply
    with pytest.raises(TypeError):
        ply.format_ascii_device(np.zeros((2, 3), dtype=np.int32))
    with pytest.raises(TypeError):
        ply.format_ascii_device(torch.zeros((2, 3), dtype=torch.int32))          # a CPU tensor: write_ply_ascii's numpy path is for it
    with pytest.raises(ValueError):
        ply.PlyWriter(max_pending=0)


def payloads(count):
    return [bytes([65 + i]) * (1000 * i) + b'\n' for i in range(count)]


@pytest.mark.parametrize('max_pending', [1, 2, 3])
def test_writer_writes_every_file(tmp_path, max_pending):
    from linr_pcgc_amd import ply
    data = payloads(7)
    with ply.PlyWriter(max_pending=max_pending) as w:
        for i, d in enumerate(data):
            kind = (bytes, bytearray, memoryview)[i % 3]          # anything bytes-like
            w.submit_bytes(str(tmp_path / ('f%d.ply' % i)), b'header %d\n' % i, kind(d))
    assert w.submitted == w.written == 7
    for i, d in enumerate(data):
        assert open(str(tmp_path / ('f%d.ply' % i)), 'rb').read() == b'header %d\n' % i + d
    with pytest.raises(RuntimeError):
        w.submit_bytes(str(tmp_path / 'late.ply'), b'', b'')
    w.close()          # closing twice is harmless


@pytest.mark.parametrize('max_pending', [1, 2, 4])
def test_at_most_max_pending_payloads_in_flight(tmp_path, max_pending):
    """The first write is held until the submitting thread has filled every buffer; each write then looks at how many payloads
    are accepted and not yet done with.  A submit past max_pending cannot have been accepted: it waits for a buffer that only the
    end of a write frees."""
    from linr_pcgc_amd import ply
    gate, seen = threading.Event(), []

    class Held(ply.PlyWriter):
        def _write(self, path, header, payload):
            gate.wait()
            seen.append(self.submitted - self.written)
            super()._write(path, header, payload)

    data = payloads(3 * max_pending + 1)
    with Held(max_pending=max_pending) as w:
        for i, d in enumerate(data):
            if i == max_pending:
                gate.set()          # every buffer is taken: the next submit blocks until the first write is over
            w.submit_bytes(str(tmp_path / ('f%d.ply' % i)), b'', d)
        gate.set()
    assert len(seen) == len(data) and seen[0] == max_pending and max(seen) == max_pending and min(seen) >= 1
    for i, d in enumerate(data):
        assert open(str(tmp_path / ('f%d.ply' % i)), 'rb').read() == d


def test_close_reraises_the_first_failed_write(tmp_path):
    from linr_pcgc_amd import ply
    data = payloads(5)
    w = ply.PlyWriter(max_pending=2)
    for i, d in enumerate(data):
        folder = tmp_path / 'missing' if i == 2 else tmp_path
        w.submit_bytes(str(folder / ('f%d.ply' % i)), b'h\n', d)          # no submit hangs behind the failed write
    with pytest.raises(FileNotFoundError) as err:
        w.close()
    assert 'missing' in str(err.value)
    for i in (0, 1):
        assert open(str(tmp_path / ('f%d.ply' % i)), 'rb').read() == b'h\n' + data[i]
    assert not os.path.exists(str(tmp_path / 'f3.ply')) and not os.path.exists(str(tmp_path / 'f4.ply'))
    w.close()          # the exception is raised once


def test_an_exception_in_the_with_block_wins_over_a_failed_write(tmp_path):
    from linr_pcgc_amd import ply
    with pytest.raises(AssertionError, match='frame 1'):
        with ply.PlyWriter() as w:
            w.submit_bytes(str(tmp_path / 'ok.ply'), b'h\n', b'1 2 3\n')
            w.submit_bytes(str(tmp_path / 'missing' / 'f.ply'), b'h\n', b'')
            raise AssertionError('frame 1 does not decode to the input')
    assert open(str(tmp_path / 'ok.ply'), 'rb').read() == b'h\n1 2 3\n'          # the writer was closed first: the file is complete
    assert w.submitted == w.written == 2

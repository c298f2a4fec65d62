"""CPU: the argument checks of the device PLY readers (linr_ply_parse_ascii_device, linr_ply_gather_binary, csrc/ply_parse.hip), which
all come before the first launch and so run without a GPU, the workspace size, and the header helper the host and the device
reader share."""
import ctypes
import io
import os

import pytest

LEN_MAX = 2 ** 31 - 1


@pytest.fixture(scope='module')
def lib():
    from linr_pcgc_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.lib()


def test_workspace_size(lib):
    ws = lib.linr_ply_parse_ws_bytes
    assert [ws(n, 10) for n in (LEN_MAX + 1, 1 << 40)] == [0, 0] and ws(100, -1) == 0
    lens, rows = (0, 1, 15, 16, 17, 4096, 4097, 10 ** 6, 17 * 10 ** 6, LEN_MAX), (0, 1, 64, 65, 10 ** 5, 10 ** 6, 10 ** 9, 1 << 40)
    table = [[ws(n, r) for r in rows] for n in lens]
    for i, n in enumerate(lens):
        for j, r in enumerate(rows):
            assert table[i][j] > 0 and table[i][j] % 256 == 0
            assert table[i][j] >= 8 * ((n + 15) // 16) + 4 * min(r, n // 2 + 1)          # chunk summaries and line offsets
            assert i == 0 or table[i][j] >= table[i - 1][j]                                # monotone in len
            assert j == 0 or table[i][j] >= table[i][j - 1]                                # ... and in n_rows
    assert ws(10 ** 6, 1 << 40) == ws(10 ** 6, 10 ** 6)          # no text holds more lines than len / 2 + 1


def test_ascii_entry_checks_its_arguments_before_any_launch(lib):
    buf = (ctypes.c_char * 16384)()
    p = (ctypes.addressof(buf) + 255) & ~255          # host memory: no call below may get as far as a launch
    n, length = 10, 200
    ws = lib.linr_ply_parse_ws_bytes(length, n)
    call = lib.linr_ply_parse_ascii_device
    good = [p, length, n, 3, 0, 1, 2, p, p, ws, p, None]

    def with_(**kw):
        names = ['text', 'len', 'n_rows', 'n_cols', 'cx', 'cy', 'cz', 'xyz', 'ws', 'ws_bytes', 'status', 'stream']
        a = list(good)
        for k, v in kw.items():
            a[names.index(k)] = v
        return call(*a)
    for name in ('text', 'xyz', 'ws', 'status'):
        assert with_(**{name: None}) == -1, name
    assert with_(n_rows=-1) == -1
    for n_cols in (-1, 0, 2, 65):
        assert with_(n_cols=n_cols) == -1
    for col in ('cx', 'cy', 'cz'):
        assert with_(**{col: -1}) == -1 and with_(**{col: 3}) == -1
    assert with_(n_cols=64, cx=63, n_rows=0) == 0 and with_(n_cols=64, cx=64, n_rows=0) == -1
    assert with_(len=LEN_MAX + 1, ws_bytes=1 << 40) == -1 and with_(len=1 << 40, ws_bytes=1 << 62) == -1
    assert with_(ws_bytes=ws - 1) == -2 and with_(ws_bytes=0) == -2
    assert with_(n_rows=10 ** 6, len=10 ** 7) == -2          # sizes are arguments like any other
    assert with_(text=p + 8) == -3                           # text: 16-byte aligned
    assert with_(ws=p + 128) == -3                           # ws: 256-byte aligned
    assert with_(status=p + 4) == -3                         # status: int64
    assert with_(n_rows=0) == 0                              # an empty frame is fine, nothing is launched
    assert call(None, 0, 0, 3, 0, 1, 2, None, None, 0, None, None) == 0
    assert bytes(buf) == bytes(16384)


def test_binary_entry_checks_its_arguments_before_any_launch(lib):
    buf = (ctypes.c_char * 4096)()
    p = (ctypes.addressof(buf) + 255) & ~255
    i3 = ctypes.c_int32 * 3
    call = lib.linr_ply_gather_binary
    off, typ = i3(0, 4, 8), i3(6, 6, 6)
    assert call(None, 5, 15, off, typ, 0, p, p, None) == -1
    assert call(p, 5, 15, off, typ, 0, None, p, None) == -1
    assert call(p, 5, 15, off, typ, 0, p, None, None) == -1
    assert call(p, 5, 15, None, typ, 0, p, p, None) == -1 and call(p, 5, 15, off, None, 0, p, p, None) == -1
    assert call(p, -1, 15, off, typ, 0, p, p, None) == -1
    assert call(p, 5, 0, off, typ, 0, p, p, None) == -1 and call(p, 5, -15, off, typ, 0, p, p, None) == -1
    assert call(p, 5, 11, off, typ, 0, p, p, None) == -1                              # z does not lie inside the record
    assert call(p, 5, 15, i3(0, 4, 8), i3(6, 6, 7), 0, p, p, None) == -1              # a double at 8 needs 16 bytes
    assert call(p, 5, 15, i3(-1, 4, 8), typ, 0, p, p, None) == -1
    assert call(p, 5, 15, off, i3(6, 8, 6), 0, p, p, None) == -1 and call(p, 5, 15, off, i3(-1, 6, 6), 0, p, p, None) == -1
    assert call(p, 5, 15, off, typ, 0, p + 2, p, None) == -3                          # xyz: int32
    assert call(p, 5, 15, off, typ, 0, p, p + 4, None) == -3                          # status: int64
    assert call(p, 0, 15, off, typ, 0, p, p, None) == 0 and call(None, 0, 15, off, typ, 0, None, None, None) == 0
    assert bytes(buf) == bytes(4096)


HEADERS = [
    (b'ply\nformat binary_little_endian 1.0\ncomment linr_pcgc_amd\nelement vertex 257\nproperty float x\nproperty float y\n'
     b'property float z\nend_header\n', ('binary_little_endian', 257, [('x', 'f4'), ('y', 'f4'), ('z', 'f4')])),
    (b'ply\nformat ascii 1.0\ncomment linr_pcgc_amd\nelement vertex 3\nproperty float x\nproperty float y\nproperty float z\nend_header\n',
     ('ascii', 3, [('x', 'f4'), ('y', 'f4'), ('z', 'f4')])),
    (b'ply\nformat binary_big_endian 1.0\nelement vertex 5\nproperty double x\nproperty uchar red\nproperty double y\nproperty double z\n'
     b'property uchar green\nelement face 0\nproperty list uchar int vertex_indices\nend_header\n',
     ('binary_big_endian', 5, [('x', 'f8'), ('red', 'u1'), ('y', 'f8'), ('z', 'f8'), ('green', 'u1')])),
    (b'ply\nformat ascii 1.0\ncomment generated\nelement vertex 5000\nproperty uchar red\nproperty uchar green\nproperty float z\n'
     b'property float x\nproperty uchar blue\nproperty float y\nelement face 0\nproperty list uchar int vertex_indices\nend_header\n',
     ('ascii', 5000, [('red', 'u1'), ('green', 'u1'), ('z', 'f4'), ('x', 'f4'), ('blue', 'u1'), ('y', 'f4')])),
]


@pytest.mark.parametrize('case', range(len(HEADERS)))
def test_header_helper(case):
    """The header variants of test_cpu_host.py (write_ply_xyz's two, the big-endian file with colours and a face element, the
    loot-like one): the fields read_ply_xyz goes on with, and the stream left at the first byte of the body."""
    from linr_pcgc_amd import ply
    head, want = HEADERS[case]
    f = io.BytesIO(head + b'BODY')
    assert ply._read_header(f, 'name.ply') == want
    assert f.read() == b'BODY'


@pytest.mark.parametrize('head, message', [
    (b'plx\n', 'is not a PLY file'),
    (b'ply\nformat ascii 1.0\nelement vertex 3\nproperty float x\n', 'header is not terminated'),
    (b'ply\nformat ascii 1.0\nelement face 3\nend_header\n', 'an element precedes the vertex element'),
    (b'ply\nformat ascii 1.0\nelement vertex 3\nproperty list uchar int x\nend_header\n', 'list property in the vertex element'),
    (b'ply\nelement vertex 3\nproperty float x\nend_header\n', 'no format / vertex element'),
    (b'ply\nformat ascii 1.0\nelement vertex 3\nproperty float x\nproperty float y\nend_header\n', 'has no x / y / z'),
])
def test_header_helper_raises_what_the_reader_raises(tmp_path, head, message):
    from linr_pcgc_amd import ply
    with pytest.raises(ValueError, match=message):
        ply._read_header(io.BytesIO(head), 'name.ply')
    path = str(tmp_path / 'bad.ply')
    open(path, 'wb').write(head)
    with pytest.raises(ValueError, match=message):
        ply.read_ply_xyz(path)


def test_device_readers_refuse_what_is_not_on_a_gpu(tmp_path, monkeypatch):
    import numpy as np
    import torch
    from linr_pcgc_amd import _lib, ply
    path = str(tmp_path / 'a.ply')
    ply.write_ply_xyz(path, np.arange(12).reshape(4, 3), binary=False)

    def no_library():
        raise AssertionError('the library was touched')
    monkeypatch.setattr(_lib, 'lib', no_library)
    for device in ('cpu', torch.device('cpu'), 'meta'):
        with pytest.raises(TypeError):
            ply.read_points_device(path, device)
        with pytest.raises(TypeError):
            ply.read_many_device([path], device)
    with pytest.raises(TypeError):
        ply.parse_ascii_device(torch.zeros(16, dtype=torch.uint8), 1, 3, (0, 1, 2))          # a CPU tensor
    with pytest.raises(TypeError):
        ply.gather_binary_device(np.zeros(16, dtype=np.uint8), 1, 12, (0, 4, 8), ('f4', 'f4', 'f4'))

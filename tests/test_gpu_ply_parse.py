"""GPU: input PLY frames parsed on the device (linr_ply_parse_ascii_device, linr_ply_gather_binary, csrc/ply_parse.hip) and the paths
built on them (ply.parse_ascii_device, gather_binary_device, read_points_device, read_many_device, MytestDataset(device_parse=True),
decoder.py / run.py --ply-parse device).  The reference is the host reader: ply.read_ply_xyz, or linr_ply_parse_ascii called directly
where rows_parsed matters.  Everything is integers and bytes: every comparison is exact.  `flags == 0` is what shows that the device
path produced a result, not the host fallback behind it."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1
TOKEN, COLUMNS, SHORT, RANGE = 1, 2, 4, 8
BLOCK_BYTES = 256 * 16          # what one block of the line kernels reads


def draw(n, seed):
    """Log-uniform magnitudes up to 2^31 - 1 with random signs: line lengths mix inside every wave."""
    rng = np.random.default_rng(seed)
    mag = np.floor(np.exp(rng.uniform(0.0, np.log(2.0 ** 31), size=(n, 3)))).astype(np.int64) - 1
    sign = np.where(rng.random((n, 3)) < 0.5, -1, 1)
    return np.clip(mag * sign, INT_MIN, INT_MAX).astype(np.int64)


def host_parse(text, n_rows, n_cols=3, cols=(0, 1, 2)):
    """linr_ply_parse_ascii: (return code, rows_parsed, xyz int64)."""
    from linr_pcgc_amd import _lib
    out = np.zeros((n_rows, 3), dtype=np.int64)
    done = ctypes.c_int64(-1)
    rc = _lib.lib().linr_ply_parse_ascii(bytes(text), len(text), n_rows, n_cols, cols[0], cols[1], cols[2], out.ctypes.data, ctypes.byref(done))
    return rc, done.value, out


def dev_parse(text, n_rows, n_cols=3, cols=(0, 1, 2)):
    from linr_pcgc_amd import ply
    t = torch.from_numpy(np.frombuffer(bytes(text), dtype=np.uint8).copy()).cuda()
    xyz, flags, first = ply.parse_ascii_device(t, n_rows, n_cols, cols)
    assert xyz.dtype == torch.int32 and xyz.is_cuda and tuple(xyz.shape) == (n_rows, 3)
    return xyz.cpu().numpy().astype(np.int64), flags, first


def same_as_host(text, n_rows, n_cols=3, cols=(0, 1, 2)):
    rc, done, want = host_parse(text, n_rows, n_cols, cols)
    assert rc == 0 and done == n_rows          # the case itself is a valid body
    got, flags, first = dev_parse(text, n_rows, n_cols, cols)
    assert (flags, first) == (0, n_rows)
    assert np.array_equal(got, want)
    return got


LAYOUTS = {'xyz': (3, (0, 1, 2)), 'xyzrgb': (6, (0, 1, 2)), 'nzyx': (6, (5, 4, 3))}


@functools.lru_cache(maxsize=None)
def round_trip_text(n, layout):
    xyz = draw(n, 100 + n)
    rng = np.random.default_rng(n)
    if layout == 'xyz':
        table = xyz
    elif layout == 'xyzrgb':
        table = np.concatenate([xyz, rng.integers(0, 256, size=(n, 3))], axis=1)
    else:
        table = np.concatenate([rng.integers(-1000, 1000, size=(n, 3)), xyz[:, ::-1]], axis=1)
    text = ''.join(' '.join(map(str, row)) + '\n' for row in table.tolist()).encode()
    return xyz, text


@pytest.mark.parametrize('layout', sorted(LAYOUTS))
@pytest.mark.parametrize('n', [0, 1, 2, 63, 64, 65, 255, 256, 257, 4097, 100003])
def test_round_trip(pkg, n, layout):
    xyz, text = round_trip_text(n, layout)
    n_cols, cols = LAYOUTS[layout]
    if n >= 63:
        assert len({len(line) for line in text.splitlines()[:64]}) > 8          # the first wave alone mixes many lengths
    got = same_as_host(text, n, n_cols, cols)
    assert np.array_equal(got, xyz)


def rows_text(rows, sep=b' ', eol=b'\n'):
    return b''.join(sep.join(b'%d' % v for v in r) + eol for r in rows)


def line_cases():
    r = draw(300, 5).tolist()
    two = [[1, 2, 3], [-4, 5, 6]]
    yield 'leading_blanks', b' ' * 1000 + b'1 2 3\n' + b'\t' * 1000 + b'-4 5 6\n', 2
    yield 'blank_lines_between', b'1 2 3\n' + b'\n \t\r\n' * 150 + b'-4 5 6\n', 2                       # 300 whitespace-only lines
    yield 'blank_lines_over_blocks', b'1 2 3\n' + b'\n \t\r\n' * (BLOCK_BYTES // 2) + b'-4 5 6\n', 2      # ... and more bytes than two blocks read
    yield 'blank_run_over_blocks', b'1 2 3\n' + b' ' * (3 * BLOCK_BYTES + 5) + b'-4 5 6\n', 2             # one line start hidden behind 12 KB of blanks
    yield 'crlf', rows_text(r, eol=b'\r\n'), 300
    yield 'tabs_ff_vt', rows_text(r[:100], sep=b'\t') + rows_text(r[100:200], sep=b'\f') + rows_text(r[200:], sep=b' \v '), 300
    yield 'trailing_blanks', rows_text(r, eol=b' \t \n'), 300
    yield 'no_final_newline', rows_text(r)[:-1], 300
    yield 'blank_lines_at_both_ends', b'\n\n \n\t\n' * 40 + rows_text(r) + b'\n \r\n\n' * 40, 300
    yield 'faces_and_junk_behind', rows_text(r) + b'3 0 1 2\n3 1 2 3\nabc\n1e3 x\n', 300
    yield 'junk_behind_without_newline', rows_text(two) + b'abc', 2


@pytest.mark.parametrize('name, text, n', list(line_cases()), ids=[c[0] for c in line_cases()])
def test_line_finding(pkg, name, text, n):
    same_as_host(text, n)


@pytest.mark.parametrize('last_byte_is_a_digit', [False, True])
@pytest.mark.parametrize('length', [16 * k + d for k in (BLOCK_BYTES // 16, 2 * BLOCK_BYTES // 16) for d in (-1, 0, 1)])
def test_text_lengths_around_a_block_boundary(pkg, length, last_byte_is_a_digit):
    body = rows_text(draw(2000, 9).tolist())
    body = body[:body.rindex(b'\n', 0, length - 40) + 1]
    pad = b' ' * (length - len(body) - 5)
    text = body + (pad + b'7 8 9' if last_byte_is_a_digit else b'7 8 9' + pad)          # no final newline
    assert len(text) == length
    n = text.count(b'\n') + 1
    got = same_as_host(text, n)
    assert got[-1].tolist() == [7, 8, 9]


@pytest.mark.parametrize('length', [6, 11, 16, 17, 31, 47, 100, BLOCK_BYTES - 1, BLOCK_BYTES + 13])
@pytest.mark.parametrize('final_newline', [False, True])
def test_nothing_at_or_past_len_is_read(pkg, length, final_newline):
    """The buffer is 64 bytes longer than the text and goes on with more digits and more lines: a read past len would lengthen the
    last number, or find vertices that are not there."""
    from linr_pcgc_amd import ply
    tail = b'4 5 6\n' if final_newline else b'-4 5 6'
    head = rows_text(draw(400, 3).tolist())
    text = (head[:head.rindex(b'\n', 0, length - len(tail)) + 1] if length > 20 else b'')
    text = text + b' ' * (length - len(text) - len(tail)) + tail
    assert len(text) == length
    lines = text.count(b'\n') + (0 if final_newline else 1)
    buf = torch.from_numpy(np.frombuffer(text + (b'9\n9 9 9\n' * 8)[:64], dtype=np.uint8).copy()).cuda()
    assert buf.numel() == length + 64 and buf.data_ptr() % 16 == 0
    for n_rows, want_flags in ((lines, 0), (lines + 1, SHORT)):
        rc, done, want = host_parse(text, n_rows)
        exact, flags_exact, first_exact = dev_parse(text, n_rows)
        xyz, flags, first = ply.parse_ascii_device(buf[:length], n_rows, 3, (0, 1, 2))
        assert (flags, first) == (flags_exact, first_exact) == (want_flags, lines) and done == lines and (rc == 0) == (want_flags == 0)
        assert np.array_equal(xyz.cpu().numpy()[:lines], want[:lines]) and np.array_equal(exact[:lines], want[:lines])


def test_rounding(pkg):
    tokens = []
    for k in (0, 1, 2, 3, 10, 11, 1000, 1001, 2147483645, 2147483646):
        tokens += ['%d.5' % k, '-%d.5' % k, '+%d.5' % k, '%d.50' % k, '%d.5001' % k, '%d.4999' % k]          # at most 14 digits
    tokens += ['0.5', '-0.5', '1.4999999', '2.5000001', '5.', '.5', '+3', '-0', '-0.4', '0.00000000000005', '2147483647.49',
               '-2147483648.5', '-2147483648', '2147483647', '000000000000001', '99999.9999999999', '12345678.5000000', '1.50000000000000',
               '0.50000000000001', '-.5', '+.50001', '007']
    tokens += ['0'] * (-len(tokens) % 3)
    text = ''.join(' '.join(tokens[i:i + 3]) + '\n' for i in range(0, len(tokens), 3)).encode()
    got = same_as_host(text, len(tokens) // 3)
    flat = dict(zip(tokens, got.reshape(-1).tolist()))
    assert [flat[t] for t in ('0.5', '1.5', '2.5', '3.5', '-0.5', '-1.5', '-2.5', '-0', '-0.4', '5.', '.5', '+3')] == \
        [0, 2, 2, 4, 0, -2, -2, 0, 0, 5, 0, 3]
    assert flat['2147483647.49'] == INT_MAX and flat['-2147483648.5'] == INT_MIN and flat['0.00000000000005'] == 0
    for token, value in (('2147483647.5', 2147483648), ('-2147483649', -2147483649), ('2147483648', 2147483648), ('-2147483648.51', -2147483649)):
        text = ('1 2 3\n4 %s 6\n7 8 9\n' % token).encode()
        rc, done, want = host_parse(text, 3)
        assert rc == 0 and want[1, 1] == value          # fine on the host, which writes int64
        got, flags, first = dev_parse(text, 3)
        assert (flags, first) == (RANGE, 1)
        assert np.array_equal(got[[0, 2]], want[[0, 2]])


FAULTS = [('1e3 2 3', TOKEN), ('1 1234567890123456 3', TOKEN), ('1 2 nan', TOKEN), ('abc 2 3', TOKEN), ('1 - 3', TOKEN), ('1 2', COLUMNS),
          ('1 2 3 4', COLUMNS)]


@functools.lru_cache(maxsize=None)
def clean_5000():
    xyz = draw(5000, 77)
    return xyz, [b'%d %d %d' % tuple(r) for r in xyz.tolist()]


@pytest.mark.parametrize('at', [0, 2500, 4999])
@pytest.mark.parametrize('line, flag', FAULTS, ids=[f[0].replace(' ', '_') for f in FAULTS])
def test_flags_and_first_row(pkg, line, flag, at):
    xyz, lines = clean_5000()
    lines = list(lines)
    lines[at] = line.encode()
    text = b'\n'.join(lines) + b'\n'
    rc, done, want = host_parse(text, 5000)
    got, flags, first = dev_parse(text, 5000)
    assert (flags, first) == (flag, at)
    if rc != 0:
        assert first == done
    else:
        assert line in ('1e3 2 3', '1 1234567890123456 3')          # valid on the host: strtod takes them
    keep = np.arange(5000) != at
    assert np.array_equal(got[keep], xyz[keep])          # rows without a flag are written whatever else the text holds


def test_short_body_and_two_faults(pkg):
    xyz, lines = clean_5000()
    for present in (0, 1, 4990):
        text = b'\n'.join(lines[:present]) + (b'\n\n \n' if present else b' \n')
        rc, done, _ = host_parse(text, 5000)
        got, flags, first = dev_parse(text, 5000)
        assert rc == -1 and (flags, first) == (SHORT, present) and done == present
        assert np.array_equal(got[:present], xyz[:present])
    assert dev_parse(b'', 7)[1:] == (SHORT, 0)
    two = list(lines)
    two[3000], two[100] = b'1 x 3', b'1 2'
    got, flags, first = dev_parse(b'\n'.join(two), 5000)
    assert (flags, first) == (TOKEN | COLUMNS, 100)
    assert host_parse(b'\n'.join(two), 5000)[:2] == (-1, 100)
    keep = ~np.isin(np.arange(5000), (100, 3000))
    assert np.array_equal(got[keep], xyz[keep])


PLY_NAMES = {'i1': 'char', 'u1': 'uchar', 'i2': 'short', 'u2': 'ushort', 'i4': 'int', 'u4': 'uint', 'f4': 'float', 'f8': 'double'}
RECORDS = {
    'float_xyz_uchar_rgb': [('x', 'f4'), ('y', 'f4'), ('z', 'f4'), ('red', 'u1'), ('green', 'u1'), ('blue', 'u1')],          # 15 bytes
    'double_xyz': [('x', 'f8'), ('y', 'f8'), ('z', 'f8')],
    'short_ushort_int': [('a', 'u1'), ('y', 'u2'), ('x', 'i2'), ('b', 'u1'), ('z', 'i4')],
    'uint_float_char': [('z', 'i1'), ('x', 'u4'), ('c', 'u1'), ('y', 'f4')],
    'uchar_double_float': [('x', 'u1'), ('y', 'f8'), ('z', 'f4')],
}


def write_binary(path, fields, n, big, seed, spoil=None):
    rng = np.random.default_rng(seed)
    e = '>' if big else '<'
    rec = np.zeros(n, dtype=[(name, e + t) for name, t in fields])
    for name, t in fields:
        if t[0] == 'f':          # halves (ties), thirds, both signs
            v = rng.integers(-2 ** 20, 2 ** 20, size=n) / rng.choice([1.0, 2.0, 3.0], size=n)
        else:
            info = np.iinfo(np.dtype(t))
            v = rng.integers(max(info.min, INT_MIN), min(info.max, INT_MAX), size=n, endpoint=True)
        rec[name] = v
    if spoil is not None:
        rec[spoil[0]][spoil[1]] = spoil[2]
    with open(path, 'wb') as f:
        f.write(('ply\nformat binary_%s_endian 1.0\nelement vertex %d\n' % ('big' if big else 'little', n)).encode())
        f.write(''.join('property %s %s\n' % (PLY_NAMES[t], name) for name, t in fields).encode())
        f.write(b'element face 0\nproperty list uchar int vertex_indices\nend_header\n')
        f.write(rec.tobytes())
    return rec


@pytest.mark.parametrize('big', [False, True])
@pytest.mark.parametrize('kind', sorted(RECORDS))
@pytest.mark.parametrize('n', [1, 257, 5001])
def test_binary_files(pkg, tmp_path, n, kind, big):
    from linr_pcgc_amd import ply
    path = str(tmp_path / 'b.ply')
    rec = write_binary(path, RECORDS[kind], n, big, seed=n)
    want = ply.read_ply_xyz(path)
    got = ply.read_points_device(path)
    assert got.is_cuda and got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), want)
    # ... and straight through the wrapper, which reports that every row was taken
    dt = rec.dtype
    raw = torch.from_numpy(np.frombuffer(rec.tobytes(), dtype=np.uint8).copy()).cuda()
    xyz, flags, first = ply.gather_binary_device(raw, n, dt.itemsize, [dt.fields[k][1] for k in 'xyz'], [dt.fields[k][0].str[1:] for k in 'xyz'], big)
    assert (flags, first) == (0, n) and np.array_equal(xyz.cpu().numpy(), want)


def test_binary_range_flag(pkg):
    from linr_pcgc_amd import ply
    rec = np.zeros(1000, dtype=[('x', '<f4'), ('y', '<f8'), ('z', '<u4'), ('pad', 'u1')])
    rec['x'], rec['y'], rec['z'] = np.arange(1000) + 0.5, -np.arange(1000) - 0.5, np.arange(1000)
    want = np.rint(np.stack([rec['x'], rec['y'], rec['z']], axis=1)).astype(np.int64)
    for field, row, value in (('x', 999, np.nan), ('x', 0, np.inf), ('y', 500, 2147483647.5), ('y', 501, -2147483648.51), ('z', 7, 2 ** 31)):
        bad = rec.copy()
        bad[field][row] = value
        raw = torch.from_numpy(np.frombuffer(bad.tobytes(), dtype=np.uint8).copy()).cuda()
        xyz, flags, first = ply.gather_binary_device(raw, 1000, 17, (0, 4, 12), ('f4', 'f8', 'u4'), False)
        assert (flags, first) == (RANGE, row)
        keep = np.arange(1000) != row
        assert np.array_equal(xyz.cpu().numpy()[keep], want[keep])
    edge = rec.copy()
    edge['y'][:2] = 2147483647.49, -2147483648.5
    raw = torch.from_numpy(np.frombuffer(edge.tobytes(), dtype=np.uint8).copy()).cuda()
    xyz, flags, first = ply.gather_binary_device(raw, 1000, 17, (0, 4, 12), ('f4', 'f8', 'u4'), False)
    assert (flags, first) == (0, 1000) and xyz[:2, 1].tolist() == [INT_MAX, INT_MIN]


def write_ascii(path, header_props, body):
    with open(path, 'wb') as f:
        f.write(b'ply\nformat ascii 1.0\ncomment test\nelement vertex %d\n' % header_props[0])
        f.write(b''.join(b'property %s %s\n' % p for p in header_props[1]))
        f.write(b'element face 0\nproperty list uchar int vertex_indices\nend_header\n')
        f.write(body)


XYZ_PROPS = [(b'float', b'x'), (b'float', b'y'), (b'float', b'z')]


@pytest.mark.parametrize('n', [0, 1, 257, 5001])
def test_files_written_by_write_ply_xyz(pkg, tmp_path, n):
    from linr_pcgc_amd import ply
    xyz = np.abs(draw(n, n)) % 1000000          # what '%g' spells without an exponent
    for binary in (True, False):
        path = str(tmp_path / ('w%d.ply' % binary))
        ply.write_ply_xyz(path, xyz, binary=binary)
        want = ply.read_ply_xyz(path)
        got = ply.read_points_device(path)
        assert got.is_cuda and tuple(got.shape) == (n, 3) and np.array_equal(got.cpu().numpy(), want)
        if n:
            assert got.dtype == torch.int32 and np.array_equal(want, xyz)
    np.save(str(tmp_path / 'c.npy'), xyz)
    assert np.array_equal(ply.read_points_device(str(tmp_path / 'c.npy')).cpu().numpy(), xyz)


def test_files_that_fall_back_or_fail_like_the_host_reader(pkg, tmp_path):
    from linr_pcgc_amd import ply
    xyz, lines = clean_5000()
    path = str(tmp_path / 'f.ply')
    for at, line in ((4000, b'1e3 2.5 -3.5'), (17, b'1 3000000000 3'), (0, b'-2147483649 0 0')):          # the host's values, int64
        body = list(lines)
        body[at] = line
        write_ascii(path, (5000, XYZ_PROPS), b'\n'.join(body) + b'\n')
        want = ply.read_ply_xyz(path)
        got = ply.read_points_device(path)
        assert got.is_cuda and np.array_equal(got.cpu().numpy(), want) and not np.array_equal(want[at], xyz[at])
    write_binary(path, RECORDS['double_xyz'], 300, False, seed=1, spoil=('y', 299, 3e9))
    want = ply.read_ply_xyz(path)
    assert want[299, 1] == 3000000000 and np.array_equal(ply.read_points_device(path).cpu().numpy(), want)
    # malformed: the host reader's exception, word for word
    bad = {'short_line': (5000, b'\n'.join(lines[:100] + [b'1 2'] + lines[101:])), 'word': (5000, b'\n'.join(lines[:4999] + [b'1 x 3'])),
           'too_few': (5000, b'\n'.join(lines[:4321]) + b'\n'), 'empty': (3, b''), 'token_too_many': (5000, b'\n'.join([b'1 2 3 4'] + lines[1:]))}
    for name, (n, body) in bad.items():
        write_ascii(path, (n, XYZ_PROPS), body)
        with pytest.raises(ValueError) as host:
            ply.read_ply_xyz(path)
        with pytest.raises(ValueError) as dev:
            ply.read_points_device(path)
        assert str(dev.value) == str(host.value) and 'malformed vertex line' in str(dev.value), name
    write_binary(path, RECORDS['float_xyz_uchar_rgb'], 100, False, seed=2)
    open(path, 'r+b').truncate(os.path.getsize(path) - 7)          # the last record is cut
    with pytest.raises(ValueError) as host:
        ply.read_ply_xyz(path)
    with pytest.raises(ValueError) as dev:
        ply.read_points_device(path)
    assert str(dev.value) == str(host.value)
    open(path, 'wb').write(b'plx\n')
    with pytest.raises(ValueError, match='is not a PLY file'):
        ply.read_points_device(path)


def test_read_many_device(pkg, tmp_path):
    from linr_pcgc_amd import ply
    paths = []
    for i in range(9):
        path = str(tmp_path / ('f%d.ply' % i))
        n = (300, 4097, 1, 2000, 17, 5001, 64, 900, 3000)[i]          # the pinned buffers grow and shrink
        rows = [b'%d %d %d %d %d %d' % (tuple(r) + (i, 2, 3)) for r in draw(n, i).tolist()]
        if i == 4:
            rows[9] = b'1e2 0.5 -7.5 0 0 0'          # this one needs the host
        if i == 3:
            write_binary(path, RECORDS['float_xyz_uchar_rgb'], n, True, seed=i)
        else:
            write_ascii(path, (n, XYZ_PROPS + [(b'uchar', b'red'), (b'uchar', b'green'), (b'uchar', b'blue')]), b'\n'.join(rows) + b'\n')
        paths.append(path)
    np.save(str(tmp_path / 'g.npy'), draw(50, 50))
    paths.insert(6, str(tmp_path / 'g.npy'))
    want = ply.read_many(paths)
    for max_pending, workers in ((2, None), (1, 1), (4, 3)):
        got = ply.read_many_device(paths, max_pending=max_pending, workers=workers)
        assert len(got) == len(want)
        for g, w in zip(got, want):
            assert g.is_cuda and np.array_equal(g.cpu().numpy(), w)
    assert ply.read_many_device([]) == []
    write_ascii(paths[2], (2, XYZ_PROPS), b'1 2 3\n')
    with pytest.raises(ValueError, match='malformed vertex line 2'):
        ply.read_many_device(paths, max_pending=2)


@functools.lru_cache(maxsize=None)
def sequence_dir(tmp):
    """Two frames of sphere_shell(7, 30) as ASCII PLY with colour columns, written once for the caller tests."""
    from linr_pcgc_amd import synthetic
    ori = os.path.join(tmp, 'ori')
    os.makedirs(ori)
    files, clouds = [], []
    for t in range(2):
        pts = np.asarray(synthetic.sphere_shell(7, 30, centre=(62 + t, 64, 66)))
        rows = [b'%d %d %d %d %d %d' % (tuple(r) + (t, 128, 255)) for r in pts.tolist()]
        path = os.path.join(ori, 'frame_%04d.ply' % t)
        write_ascii(path, (len(rows), XYZ_PROPS + [(b'uchar', b'red'), (b'uchar', b'green'), (b'uchar', b'blue')]), b'\n'.join(rows) + b'\n')
        files.append(path)
        clouds.append(pts)
    return ori, tuple(files), clouds


@pytest.fixture(scope='module')
def sequence(tmp_path_factory):
    return sequence_dir(str(tmp_path_factory.mktemp('plyseq')))


def test_dataset_with_device_parse(pkg, sequence):
    from linr_pcgc_amd import custom_dataset as cd
    ori, files, clouds = sequence
    host, dev = cd.MytestDataset(ori, ori_type='ply'), cd.MytestDataset(ori, ori_type='ply', device_parse=True)
    assert len(host) == len(dev) == 2
    for i in range(2):
        a, b = host[i], dev[i]
        assert a.dtype == b.dtype == torch.int32 and a.device == b.device and torch.equal(a, b)


def tree(root):
    out = {}
    for folder, _, names in os.walk(root):
        for name in names:
            full = os.path.join(folder, name)
            out[os.path.relpath(full, root)] = open(full, 'rb').read()
    return out


def test_encoder_and_decoder_programs(pkg, tmp_path, sequence, capsys):
    """run.py --ply-parse device writes the files --ply-parse host writes, byte for byte; the decoder program rebuilds the frames from
    them and finds each equal to the original it parsed on the GPU."""
    from linr_pcgc_amd import decoder, run
    ori, files, clouds = sequence
    trees = {}
    for mode in ('host', 'device'):
        out = str(tmp_path / mode)
        args = run.parse(['--input-glob', os.path.join(ori, 'frame_*.ply'), '--frames', '2', '--gop', '2', '--first-epoch', '1',
                          '--others-epoch', '1', '--out', out, '--ply-parse', mode])
        summary, _ = run.run_sequence_job(args, 0, 1, None, files=list(files))
        assert summary['gops'] == 1
        trees[mode] = tree(os.path.join(out, 'result_enc'))
    assert trees['host'] and sorted(trees['host']) == sorted(trees['device'])
    for name, data in trees['host'].items():
        assert trees['device'][name] == data, name
    capsys.readouterr()
    decoder.main(['--enc-dir', os.path.join(str(tmp_path / 'device'), 'result_enc'), '--dec-dir', str(tmp_path / 'dec'), '--ori-dir', ori,
                  '--ply-parse', 'device'])
    assert 'decoded 2 frames of 1 GOPs' in capsys.readouterr().out
    assert sorted(os.listdir(str(tmp_path / 'dec'))) == ['frame0000.ply', 'frame0001.ply']

"""GPU: decoded frames formatted as ASCII PLY text on the device (linr_ply_format_ascii, csrc/ply_format.hip) and the paths built on
it (ply.format_ascii_device, custom_dataset.write_ply_ascii with a CUDA tensor, ply.PlyWriter, the decoder program).  The reference
is the writer the package had before: np.savetxt(fmt='%d') behind the same header.  Everything is bytes: every comparison is exact."""
import ctypes
import io
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1


def savetxt_bytes(xyz):
    out = io.BytesIO()
    np.savetxt(out, np.asarray(xyz).astype('int32').reshape(-1, 3), fmt='%d')
    return out.getvalue()


def draw(n, seed):
    """Log-uniform magnitudes (every digit count about equally often) with random signs: line lengths vary inside every wave."""
    rng = np.random.default_rng(seed)
    mag = np.floor(np.exp(rng.uniform(0.0, np.log(2.0 ** 31), size=(n, 3)))).astype(np.int64) - 1
    sign = np.where(rng.random((n, 3)) < 0.5, -1, 1)
    return np.clip(mag * sign, INT_MIN, INT_MAX).astype(np.int32)


def text_of(t):
    return t.cpu().numpy().tobytes()


@pytest.mark.parametrize('n', [0, 1, 2, 63, 64, 65, 255, 256, 257, 4097, 100003])
def test_bytes_equal_savetxt(pkg, n):
    from linr_pcgc_amd import ply
    x = draw(n, 100 + n)
    if n >= 63:
        assert len({len(line) for line in savetxt_bytes(x[:64]).splitlines()}) > 8          # the first wave alone mixes many lengths
    got = ply.format_ascii_device(torch.from_numpy(x).cuda())
    assert got.dtype == torch.uint8 and got.is_cuda and got.dim() == 1
    assert text_of(got) == savetxt_bytes(x)


def boundary_rows():
    vals = {0, INT_MAX, INT_MIN}
    for k in range(10):
        vals |= {10 ** k - 1, -(10 ** k - 1), 10 ** k, -(10 ** k)}
    rows = []
    for v in sorted(vals):
        for col in range(3):
            for others in ((0, 0), (INT_MIN, INT_MIN), (7, INT_MIN), (INT_MAX, -1)):
                row = list(others)
                row.insert(col, v)
                rows.append(row)
    return np.asarray(rows, dtype=np.int64)


def test_every_digit_count_boundary(pkg):
    from linr_pcgc_amd import ply
    rows = boundary_rows()
    assert 300 < len(rows) < 1000 and rows.min() == INT_MIN and rows.max() == INT_MAX
    want = savetxt_bytes(rows)
    got = ply.format_ascii_device(torch.from_numpy(rows.astype(np.int32)).cuda())
    assert text_of(got) == want
    assert got.numel() == sum(len('%d %d %d\n' % tuple(int(v) for v in r)) for r in rows)
    # other integer dtypes are converted like .astype('int32')
    assert text_of(ply.format_ascii_device(torch.from_numpy(rows).cuda())) == want


def _raw_call(L, xyz, text, ws, ws_bytes, length, cap):
    return L.linr_ply_format_ascii(xyz.data_ptr(), xyz.shape[0], text.data_ptr(), cap, ws.data_ptr(), ws_bytes, length.data_ptr(),
                                   ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))


@pytest.mark.parametrize('n', [1, 257, 5001])
def test_nothing_outside_the_text_is_written(pkg, n):
    from linr_pcgc_amd import _lib
    L = _lib.lib()
    x = draw(n, 7 + n)
    want = savetxt_bytes(x)
    xyz = torch.from_numpy(x).cuda()
    cap, ws_bytes = L.linr_ply_format_text_bytes(n), L.linr_ply_format_ws_bytes(n)
    assert cap == 36 * n and ws_bytes >= 4 * (n + 1)
    results = []
    for ws_fill in (0xA5, 0xA5, 0xFF):          # twice the same; then the workspace LINR_DEBUG_POISON hands out
        text = torch.full((cap + 4096,), 0xA5, dtype=torch.uint8, device='cuda')
        ws = torch.full((ws_bytes + 4096,), ws_fill, dtype=torch.uint8, device='cuda')
        ws[ws_bytes:] = 0xA5
        length = torch.full((3,), -7, dtype=torch.int64, device='cuda')
        assert _raw_call(L, xyz, text, ws, ws_bytes, length[1:], cap) == 0
        assert length.tolist() == [-7, len(want), -7]
        assert bool((text[len(want):] == 0xA5).all()) and bool((ws[ws_bytes:] == 0xA5).all())
        results.append(text_of(text[:len(want)]))
    assert results == [want, want, want]
    # n == 0: nothing launched, nothing touched
    text = torch.full((64,), 0xA5, dtype=torch.uint8, device='cuda')
    length = torch.full((1,), -7, dtype=torch.int64, device='cuda')
    assert L.linr_ply_format_ascii(None, 0, None, 0, None, 0, None, None) == 0
    assert L.linr_ply_format_ascii(xyz.data_ptr(), 0, text.data_ptr(), 64, text.data_ptr(), 64, length.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert length.item() == -7 and bool((text == 0xA5).all())


@pytest.mark.parametrize('n', [0, 1, 1000])
def test_write_ply_ascii_with_a_cuda_tensor(pkg, tmp_path, n):
    from linr_pcgc_amd import custom_dataset as cd, ply
    x = np.abs(draw(n, 31 + n)) % (1 << 20)
    a, b, c = (str(tmp_path / name) for name in ('device.ply', 'numpy.ply', 'o3d.ply'))
    cd.write_ply_ascii(a, torch.from_numpy(x).cuda())
    cd.write_ply_ascii(b, x)
    cd.write_ply_o3d(c, torch.from_numpy(x.astype(np.int64)).cuda())
    data = open(b, 'rb').read()
    assert open(a, 'rb').read() == data and open(c, 'rb').read() == data
    assert data.startswith(b'ply\nformat ascii 1.0\nelement vertex %d\n' % n)
    if n == 0:
        assert data.endswith(b'end_header\n')
    else:
        assert np.array_equal(ply.read_ply_xyz(a), x)


def test_writer_thread_with_device_frames(pkg, tmp_path):
    from linr_pcgc_amd import custom_dataset as cd, ply
    frames = [draw(n, n) for n in (300, 0, 4097, 17, 2000)]          # the pinned buffers grow and shrink
    with ply.PlyWriter(max_pending=2) as w:
        for i, x in enumerate(frames):
            w.submit(str(tmp_path / ('f%d.ply' % i)), torch.from_numpy(x).cuda())
    assert w.submitted == w.written == len(frames)
    for i, x in enumerate(frames):
        cd.write_ply_ascii(str(tmp_path / 'want.ply'), x)
        assert open(str(tmp_path / ('f%d.ply' % i)), 'rb').read() == open(str(tmp_path / 'want.ply'), 'rb').read()


@pytest.mark.parametrize('lockstep', [0, 2])
def test_decoder_program_writes_the_files_of_the_numpy_writer(pkg, tmp_path, lockstep):
    """A GOP of 3 frames, one epoch, encoded to files; decoder.main rebuilds the frames from them, compares each with the input and
    writes it through the device formatter and the writer thread.  Each file is what write_ply_ascii makes of the decoded frame as
    a numpy array (the decoded frame is the sorted, de-duplicated input: main checked it) and reads back to the input."""
    from linr_pcgc_amd import custom_dataset as cd, decoder, ply, run, synthetic
    ori = tmp_path / 'ori'
    ori.mkdir()
    files, clouds = [], []
    for t in range(3):
        path = str(ori / ('frame_%04d.ply' % t))
        clouds.append(np.asarray(synthetic.sphere_shell(7, 39 + t, centre=(60 + t, 64, 66))))
        ply.write_ply_xyz(path, clouds[-1], binary=False)
        files.append(path)
    out = str(tmp_path / 'seq')
    args = run.parse(['--input-glob', str(ori / 'frame_*.ply'), '--frames', '3', '--gop', '3', '--first-epoch', '1', '--others-epoch', '1',
                      '--out', out])
    summary, _ = run.run_sequence_job(args, 0, 1, None, files=files)
    assert summary['gops'] == 1
    dec_dir = str(tmp_path / 'dec')
    decoder.main(['--enc-dir', os.path.join(out, 'result_enc'), '--dec-dir', dec_dir, '--ori-dir', str(ori), '--lockstep', str(lockstep)])
    assert sorted(os.listdir(dec_dir)) == ['frame%04d.ply' % t for t in range(3)]
    for t in range(3):
        frame = torch.unique(torch.from_numpy(clouds[t].astype(np.int32)), dim=0).numpy()
        got = os.path.join(dec_dir, 'frame%04d.ply' % t)
        cd.write_ply_ascii(str(tmp_path / 'want.ply'), frame)
        assert open(got, 'rb').read() == open(str(tmp_path / 'want.ply'), 'rb').read()
        assert np.array_equal(ply.read_ply_xyz(got), frame)

"""A/B of the decoder's output path, one process, one GPU: decoded frames written as ASCII PLY by np.savetxt on the thread that drives
the GPU (write_ply_ascii with a numpy array: what the decoder did before) against the device formatter (write_ply_ascii with the
CUDA tensor, csrc/ply_format.hip) and against the decoder program with its writer thread (ply.PlyWriter).

  python tools/ply_write_ab.py [--frames 32] [--runs 5] [--program-runs 3] [--skip-program] [--dir DIR]

Per frame - loot10 frame 0 and owlii11 frame 0, sorted and de-duplicated like a decoded frame: old and new path alternate, --runs
timed repetitions each after one warm-up, a device synchronisation on both sides of every timed region, median and min-max.  The
new path is also taken apart: the format kernels (scan + emit, device events around the library call), the device-to-host copy of
the text into pinned and into pageable memory (device events / wall), and the file write.  Files are compared byte for byte.
The emit kernel alone is not visible to events from outside the call; scan + emit is an upper bound for it, which is what the
emit-against-copy rule of csrc/ply_format.hip is decided on.

The decoder program - a loot10 GOP of --frames frames, model trained one epoch, written with codec.write_gop: wall time of
decoder.main with the writer the decoder had before (a stand-in for PlyWriter that calls write_ply_ascii(path, dec.cpu().numpy())
in submit) at --lockstep 0, and with PlyWriter at --lockstep 0 and --lockstep 8; the variants alternate, --program-runs runs each
after one warm-up of the decode, all files compared byte for byte with the first variant's."""
import argparse
import contextlib
import ctypes
import filecmp
import io
import os
import statistics
import sys
import tempfile
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from linr_pcgc_amd import _lib, codec, custom_dataset as cd, decoder, overfit, ply, synthetic      # noqa: E402
from linr_pcgc_amd.model_core import FlatAdam                                                      # noqa: E402
from linr_pcgc_amd.module_utils import unique_sorted                                               # noqa: E402

ap = argparse.ArgumentParser('ply_write_ab')
ap.add_argument('--frames', type=int, default=32)
ap.add_argument('--runs', type=int, default=5)
ap.add_argument('--program-runs', type=int, default=3)
ap.add_argument('--skip-program', action='store_true')
ap.add_argument('--dir', default=None, help='where the files go (default: a temporary directory)')
args = ap.parse_args()
torch.set_num_threads(4)
root = args.dir or tempfile.mkdtemp(prefix='ply_write_ab_')
os.makedirs(root, exist_ok=True)
print('files under %s; %d host threads available' % (root, len(os.sched_getaffinity(0))))


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def events(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b), out


def line(name, t, unit='ms'):
    t = sorted(t)
    print('  %-44s median %10.3f  min %10.3f  max %10.3f  %s' % (name, statistics.median(t), t[0], t[-1], unit))
    return statistics.median(t)


def per_frame(config):
    dec = unique_sorted(synthetic.sequence_frame_device(config, 0, 'cuda').to(torch.int32))
    n = int(dec.shape[0])
    old_path, new_path = os.path.join(root, config + '_old.ply'), os.path.join(root, config + '_new.ply')
    old = lambda: cd.write_ply_ascii(old_path, dec.cpu().numpy())
    new = lambda: cd.write_ply_ascii(new_path, dec)
    old(), new()                                                           # warm-up
    t_old, t_new = [], []
    for _ in range(args.runs):
        t_old.append(wall(old)[0])
        t_new.append(wall(new)[0])
    same = filecmp.cmp(old_path, new_path, shallow=False)
    size = os.path.getsize(new_path)
    print('%s frame 0: %d points, file %d bytes (%.2f MB), files identical: %s' % (config, n, size, size / 1e6, same))
    m_old = line('old: write_ply_ascii(path, dec.cpu().numpy())', t_old)
    m_new = line('new: write_ply_ascii(path, dec)', t_new)
    print('  old / new = %.1fx' % (m_old / m_new))
    # the new path taken apart
    L = _lib.lib()
    cap, ws_bytes = L.linr_ply_format_text_bytes(n), L.linr_ply_format_ws_bytes(n)
    text, ws = torch.empty(cap, dtype=torch.uint8, device='cuda'), _lib.scratch(ws_bytes, 'cuda')
    length = torch.zeros(1, dtype=torch.int64, device='cuda')
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    fmt = lambda: _lib.check(L.linr_ply_format_ascii(dec.data_ptr(), n, text.data_ptr(), cap, ws.data_ptr(), ws_bytes, length.data_ptr(),
                                                     stream), 'linr_ply_format_ascii')
    fmt()
    nbytes = int(length.item())
    body = text[:nbytes]
    pinned = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
    pinned.copy_(body)
    header = (ply.ASCII_HEADER % n).encode('ascii')

    def write_file():
        with open(new_path, 'wb') as f:
            f.write(header)
            f.write(pinned.numpy())

    t_fmt, t_pin, t_page, t_file = [], [], [], []
    for _ in range(args.runs):
        t_fmt.append(events(fmt)[0])
        t_pin.append(events(lambda: pinned.copy_(body, non_blocking=True))[0])
        t_page.append(wall(lambda: body.cpu())[0])
        t_file.append(wall(write_file)[0])
    m_fmt = line('format kernels, scan + emit (device events)', t_fmt)
    m_pin = line('copy of %d bytes to pinned memory (events)' % nbytes, t_pin)
    line('copy to pageable memory, .cpu() (wall)', t_page)
    line('file write of header + text (wall)', t_file)
    print('  emit against the copy it feeds: scan + emit %.3f ms %s pinned copy %.3f ms -> %s' % (
        m_fmt, '<=' if m_fmt <= m_pin else '>', m_pin,
        'the emit kernel is not slower than the copy: plain per-lane byte stores stay' if m_fmt <= m_pin else
        'scan + emit is slower than the copy: the emit kernel has to be timed alone'))
    return same


ok = [per_frame(c) for c in ('loot10', 'owlii11')]


class SavetxtWriter:
    """What the decoder did before PlyWriter: np.savetxt on the calling thread, one frame after the other."""

    def __init__(self, max_pending=2):
        pass

    def submit(self, path, coords):
        cd.write_ply_ascii(path, coords.cpu().numpy())

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


def program(enc_dir, dec_dir, writer, lockstep):
    os.makedirs(dec_dir, exist_ok=True)
    decoder.PlyWriter = writer
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            return wall(lambda: decoder.main(['--enc-dir', enc_dir, '--dec-dir', dec_dir, '--lockstep', str(lockstep)]))[0]
    finally:
        decoder.PlyWriter = ply.PlyWriter


if not args.skip_program:
    n = args.frames
    gop = overfit.Gop(None, [synthetic.sequence_frame_device('loot10', t, 'cuda') for t in range(n)], None, 64, 'cuda')
    model = overfit.gen_model(gop.scale_num, 'cuda', seed=8807)
    print('decoder program: loot10 GOP of %d frames, %d points, trained 1 epoch: %.3f bpp' % (
        n, sum(gop.point_nums), min(overfit.overfit_gop(model, FlatAdam(model), gop, 1))))
    enc_dir = os.path.join(root, 'result_enc')
    codec.write_gop(codec.encode_gop(model, overfit.gen_model(gop.scale_num, 'cuda'), gop, 8), os.path.join(enc_dir, 'gop_0_%d' % (n - 1)))
    variants = [('before: np.savetxt in the decode loop, --lockstep 0', SavetxtWriter, 0, 'dec_old'),
                ('PlyWriter, --lockstep 0', ply.PlyWriter, 0, 'dec_new0'),
                ('PlyWriter, --lockstep 8', ply.PlyWriter, 8, 'dec_new8')]
    for name, writer, lockstep, sub in variants[1:]:                       # warm-up of the decode; the old writer has nothing to warm
        program(enc_dir, os.path.join(root, sub), writer, lockstep)
    times = {name: [] for name, _, _, _ in variants}
    for _ in range(args.program_runs):
        for name, writer, lockstep, sub in variants:
            times[name].append(program(enc_dir, os.path.join(root, sub), writer, lockstep))
    med = {}
    for name, _, _, _ in variants:
        med[name] = line(name, [t / 1e3 for t in times[name]], 's wall')
        print('  %-44s %10.1f ms per frame' % ('', med[name] * 1e3 / n))
    for name, _, _, sub in variants[1:]:
        cmp = filecmp.cmpfiles(os.path.join(root, 'dec_old'), os.path.join(root, sub), ['frame%04d.ply' % t for t in range(n)], shallow=False)
        ok.append(len(cmp[0]) == n)
        print('  %s: %d of %d files identical to the old writer\'s; %.1fx' % (name, len(cmp[0]), n, med[variants[0][0]] / med[name]))
print('all files identical: %s' % all(ok))
sys.exit(0 if all(ok) else 1)

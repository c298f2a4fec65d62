"""A/B of the input path, one process, one GPU: PLY frames read by the host parser (ply.read_ply_xyz / ply.read_many, what every
caller does by default) against the device readers (ply.read_points_device / ply.read_many_device, csrc/ply_parse.hip), and the
decoder program with --ori-dir under --ply-parse host and --ply-parse device.

  python tools/ply_parse_ab.py [--frames 32] [--runs 5] [--program-runs 3] [--skip-program] [--dir DIR]

The frames are synthetic.sequence_frame('loot10', t) written as ASCII PLY with `x y z r g b` (the layout of the 8iVFB files), by
worker processes before this process touches the GPU.  Both paths are warmed, then alternate in this process: --runs timed
repetitions each, a device synchronisation on both sides of every timed region, median and min-max.  The device path of one frame
is also taken apart: the file read into pinned memory (wall), the H2D copy (device events) and the kernels (device events around
the library call).  Both paths must return equal arrays for every frame.

The decoder program - the same frames as one GOP, model trained one epoch, written with codec.write_gop: wall time of decoder.main
with --ori-dir (every frame decoded and compared with its original), --ply-parse host against --ply-parse device, alternating,
--program-runs runs each after one warm-up."""
import argparse
import contextlib
import ctypes
import io
import multiprocessing
import os
import statistics
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ap = argparse.ArgumentParser('ply_parse_ab')
ap.add_argument('--frames', type=int, default=32)
ap.add_argument('--runs', type=int, default=5)
ap.add_argument('--program-runs', type=int, default=3)
ap.add_argument('--skip-program', action='store_true')
ap.add_argument('--dir', default=None, help='where the files go (default: a temporary directory)')
args = ap.parse_args()
root = args.dir or tempfile.mkdtemp(prefix='ply_parse_ab_')
ori = os.path.join(root, 'ori')
os.makedirs(ori, exist_ok=True)
cpus = len(os.sched_getaffinity(0))


def write_frame(t):
    from linr_pcgc_amd import synthetic
    pts = np.asarray(synthetic.sequence_frame('loot10', t))
    table = np.concatenate([pts, np.random.default_rng(t).integers(0, 256, size=(len(pts), 3))], axis=1)
    path = os.path.join(ori, 'frame_%04d.ply' % t)
    with open(path, 'wb') as f:
        f.write(('ply\nformat ascii 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\nproperty uchar red\n'
                 'property uchar green\nproperty uchar blue\nend_header\n' % len(pts)).encode('ascii'))
        np.savetxt(f, table, fmt='%d')
    return path


t0 = time.perf_counter()
with multiprocessing.get_context('fork').Pool(min(16, cpus, args.frames)) as workers:          # before the GPU is initialised
    files = workers.map(write_frame, range(args.frames))
print('%d frames under %s (%.1f MB each, written in %.1f s); %d host threads available' % (
    len(files), ori, os.path.getsize(files[0]) / 1e6, time.perf_counter() - t0, cpus))

import torch                                                                                       # noqa: E402
from linr_pcgc_amd import _lib, codec, decoder, overfit, ply                                       # noqa: E402
from linr_pcgc_amd.model_core import FlatAdam                                                      # noqa: E402

torch.set_num_threads(4)


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
    print('  %-52s median %10.3f  min %10.3f  max %10.3f  %s' % (name, statistics.median(t), t[0], t[-1], unit))
    return statistics.median(t), t[-1] - t[0]


# ---- one frame -----------------------------------------------------------------------------------------------------------------------
host0, dev0 = ply.read_ply_xyz(files[0]), ply.read_points_device(files[0])          # warm-up of both
same = [dev0.dtype == torch.int32 and np.array_equal(dev0.cpu().numpy(), host0)]
t_host, t_dev = [], []
for _ in range(args.runs):
    t_host.append(wall(lambda: ply.read_ply_xyz(files[0]))[0])
    t_dev.append(wall(lambda: ply.read_points_device(files[0]))[0])
print('frame 0: %d points, file %d bytes' % (host0.shape[0], os.path.getsize(files[0])))
m_host, _ = line('host: read_ply_xyz, one thread', t_host)
m_dev, _ = line('device: read_points_device', t_dev)
print('  host / device = %.1fx' % (m_host / m_dev))
# the device path taken apart
slot = [None]
fr = ply._load_body(files[0], slot)
names = [p[0] for p in fr.props]
cols = [names.index(k) for k in ('x', 'y', 'z')]
body = torch.empty(fr.nbytes, dtype=torch.uint8, device='cuda')
L = _lib.lib()
ws_bytes = L.linr_ply_parse_ws_bytes(fr.nbytes, fr.n_vertex)
ws, xyz = _lib.scratch(ws_bytes, 'cuda'), torch.empty((fr.n_vertex, 3), dtype=torch.int32, device='cuda')
status = torch.empty(2, dtype=torch.int64, device='cuda')
stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
parse = lambda: _lib.check(L.linr_ply_parse_ascii_device(body.data_ptr(), fr.nbytes, fr.n_vertex, len(names), cols[0], cols[1], cols[2],
                                                         xyz.data_ptr(), ws.data_ptr(), ws_bytes, status.data_ptr(), stream),
                           'linr_ply_parse_ascii_device')
body.copy_(fr.pinned)
parse()
t_file, t_copy, t_kern = [], [], []
for _ in range(args.runs):
    t_file.append(wall(lambda: ply._load_body(files[0], slot))[0])
    t_copy.append(events(lambda: body.copy_(fr.pinned, non_blocking=True))[0])
    t_kern.append(events(parse)[0])
same.append(status.tolist() == [0, fr.n_vertex] and np.array_equal(xyz.cpu().numpy(), host0))
line('header + file read into pinned memory (wall)', t_file)
line('H2D copy of %d bytes (device events)' % fr.nbytes, t_copy)
line('kernels: init, scan, lines, parse (device events)', t_kern)
print('  workspace %d bytes' % ws_bytes)

# ---- a GOP ---------------------------------------------------------------------------------------------------------------------------
host_all, dev_all = ply.read_many(files), ply.read_many_device(files)                # warm-up of both
same.append(all(d.dtype == torch.int32 and np.array_equal(d.cpu().numpy(), h) for d, h in zip(dev_all, host_all)))
del dev_all
t_host, t_dev = [], []
for _ in range(args.runs):
    t_host.append(wall(lambda: ply.read_many(files))[0])
    t_dev.append(wall(lambda: ply.read_many_device(files))[0])
print('the %d frames of a GOP' % len(files))
m_host, s_host = line('host: read_many (%d threads)' % min(cpus, 16, len(files)), t_host)
m_dev, s_dev = line('device: read_many_device (4 buffers, 4 threads)', t_dev)
gain = m_host - m_dev
print('  host - device = %.1f ms per GOP, spreads %.1f / %.1f ms -> %s' % (
    gain, s_host, s_dev, 'the device path wins by more than the spread' if gain > max(s_host, s_dev) else
    'NO win beyond the spread'))


# ---- the decoder program ------------------------------------------------------------------------------------------------------------
def program(enc_dir, dec_dir, mode):
    os.makedirs(dec_dir, exist_ok=True)
    with contextlib.redirect_stdout(io.StringIO()):
        return wall(lambda: decoder.main(['--enc-dir', enc_dir, '--dec-dir', dec_dir, '--ori-dir', ori, '--ply-parse', mode]))[0]


if not args.skip_program:
    n = len(files)
    gop = overfit.Gop(None, [torch.as_tensor(h, device='cuda') for h in host_all], None, 64, 'cuda')
    model = overfit.gen_model(gop.scale_num, 'cuda', seed=8807)
    print('decoder program with --ori-dir: GOP of %d frames, %d points, trained 1 epoch: %.3f bpp' % (
        n, sum(gop.point_nums), min(overfit.overfit_gop(model, FlatAdam(model), gop, 1))))
    enc_dir = os.path.join(root, 'result_enc')
    codec.write_gop(codec.encode_gop(model, overfit.gen_model(gop.scale_num, 'cuda'), gop, 8), os.path.join(enc_dir, 'gop_0_%d' % (n - 1)))
    del gop
    program(enc_dir, os.path.join(root, 'dec_device'), 'device')                    # warm-up of the decode
    times = {'host': [], 'device': []}
    for _ in range(args.program_runs):
        for mode in ('host', 'device'):
            times[mode].append(program(enc_dir, os.path.join(root, 'dec_' + mode), mode))          # main raises if a frame differs
    med = {}
    for mode in ('host', 'device'):
        med[mode], _ = line('decoder.main --ori-dir --ply-parse %s' % mode, [t / 1e3 for t in times[mode]], 's wall')
        print('  %-52s %10.1f ms per frame' % ('', med[mode] * 1e3 / n))
    print('  host / device = %.2fx' % (med['host'] / med['device']))
print('both paths return equal arrays: %s' % all(same))
sys.exit(0 if all(same) else 1)

"""Octree levels of deep and thin clouds (csrc/octree.hip: bitmap levels against sparse levels).

  python tools/octree_deep.py sweep                 one level (max_levels = 1) of the loot10 / owlii11 stand-ins and of a 9-bit shell,
                                                    thinned to a series of densities, forced to a bitmap level and to a sparse level
                                                    (LINR_OCTREE_DENSE_RATIO): microseconds per call of both against words / rows -
                                                    the crossover behind LV_DENSE_RATIO (profiles/octree_crossover.txt)
  python tools/octree_deep.py frames [--tree DIR]   ms per prepare_frame of a ~3 M-point 12-bit shell and of a 100 k-point 18-bit random
                                                    cloud (and of loot10 / owlii11 frames: the shallow path); --tree: import the package
                                                    from another checkout, e.g. the parent commit's, run alternately on the same box
  python tools/octree_deep.py frames --prof         a few frames of the two deep clouds only, for rocprofv3 --kernel-trace --stats
"""
import argparse
import os
import statistics
import sys
import time


def _thin_shell(torch, synthetic):
    return synthetic.sphere_shell_device(12, 1900, [2048] * 3, 0.033, 'cuda')


def _random18(torch):
    g = torch.Generator(device='cuda').manual_seed(18)
    return torch.randint(0, 1 << 18, (100000, 3), generator=g, device='cuda', dtype=torch.int32)


def frames(args):
    import torch
    from linr_pcgc_amd import synthetic
    from linr_pcgc_amd.module_utils import prepare_frame
    clouds = [('shell12', _thin_shell(torch, synthetic)), ('random18', _random18(torch))]
    if not args.prof:
        clouds += [('loot10', synthetic.sequence_frame_device('loot10', 0, 'cuda')), ('owlii11', synthetic.sequence_frame_device('owlii11', 0, 'cuda'))]
    for name, pts in clouds:
        reps = 5 if args.prof else args.reps
        for _ in range(3):
            fr = prepare_frame(pts, None, 64, device='cuda', with_offsets=False)
        torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fr = prepare_frame(pts, None, 64, device='cuda', with_offsets=False)
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        print('%-9s %8d points %2d scales  prepare_frame median %.3f ms  min %.3f  max %.3f  (%d reps, %s)' % (
            name, fr['point_num'], fr['scale_num'], statistics.median(ts), min(ts), max(ts), reps, args.tag), flush=True)


def _one_level(torch, L, child, bits, ratio, reps):
    """microseconds per linr_octree_levels call of level 0 alone under a forced plan (device events around `reps` calls)"""
    os.environ['LINR_OCTREE_DENSE_RATIO'] = ratio
    m = child.shape[0]
    cap = L.linr_octree_levels_rows(m, bits, 1)
    nbytes = L.linr_octree_levels_workspace_bytes(m, bits, 1)
    parents = torch.empty((cap, 3), dtype=torch.int32, device='cuda')
    occ = torch.empty((cap, 8), dtype=torch.float32, device='cuda')
    counts = torch.empty(1, dtype=torch.int64, device='cuda')
    ws = torch.empty(nbytes + 256, dtype=torch.uint8, device='cuda')
    base = (ws.data_ptr() + 255) & ~255
    stream = torch.cuda.current_stream().cuda_stream

    def call():
        rc = L.linr_octree_levels(child.data_ptr(), m, None, bits, 1, parents.data_ptr(), occ.data_ptr(), counts.data_ptr(), base, nbytes, stream)
        assert rc == 0, rc
    for _ in range(5):
        call()
    torch.cuda.synchronize()
    best = []
    for _ in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            call()
        e1.record()
        torch.cuda.synchronize()
        best.append(e0.elapsed_time(e1) * 1e3 / reps)
    del os.environ['LINR_OCTREE_DENSE_RATIO']
    return min(best), int(counts), parents[:int(counts)].clone(), nbytes


def sweep(args):
    import torch
    from linr_pcgc_amd import _lib, ops, synthetic
    L = _lib.lib()
    bases = [(9, synthetic.sphere_shell_device(9, 230, [256] * 3, 0.5, 'cuda')), (10, synthetic.sequence_frame_device('loot10', 0, 'cuda')),
             (11, synthetic.sequence_frame_device('owlii11', 0, 'cuda'))]
    print('one octree level (level 0, max_levels = 1) forced to a bitmap level and to a sparse level; us per call = the best of 3 windows of '
          '%d calls between device events; words = 2^(3 (bits - 1)) / 32' % args.reps)
    print('%4s %9s %9s %9s %10s %10s %8s' % ('bits', 'rows', 'parents', 'words/row', 'bitmap us', 'sparse us', 'b/s'))
    for bits, pts in bases:
        full = ops.coords_sort_unique(pts.contiguous(), 0, bits)
        g = torch.Generator(device='cuda').manual_seed(bits)
        keep = 1.0
        while full.shape[0] * keep >= 1500:
            if keep == 1.0:
                child = full
            else:
                sel = torch.rand(full.shape[0], generator=g, device='cuda') < keep
                child = full[sel].contiguous()                      # a subset of a sorted unique list is sorted and unique
            td, nd, pd, _ = _one_level(torch, L, child, bits, '1e30', args.reps)
            tsp, ns, ps, _ = _one_level(torch, L, child, bits, '0', args.reps)
            assert nd == ns and torch.equal(pd, ps)
            words = (1 << (3 * (bits - 1))) >> 5
            print('%4d %9d %9d %9.1f %10.1f %10.1f %8.2f' % (bits, child.shape[0], nd, words / child.shape[0], td, tsp, td / tsp), flush=True)
            keep /= 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('mode', choices=['sweep', 'frames'])
    ap.add_argument('--tree', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument('--tag', default='')
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--prof', action='store_true')
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    args.tag = args.tag or os.path.abspath(args.tree)
    (sweep if args.mode == 'sweep' else frames)(args)


if __name__ == '__main__':
    main()

"""ms per training step of the channel-blocked executor (hidden_channel_conv 16 / 32) on frame 0 of a config, beside width 8.

--train-precision takes one name or several separated by commas (f32,bf16-mul), --schedules the schedules of the wide step (py = the
Python schedule, the default; c = linr_net_train_step_wide, LINR_WIDE_C_STEP=1): the arms of a width - every precision on every
schedule - run in ONE session, alternating, --rounds timed rounds of --steps steps each after a warm-up.  A line gives an arm's median
round and its spread (min .. max) of the wall time per step with a device synchronisation around the round ("GPU ms"), the calling
thread's CPU time per step (time.thread_time, nothing synchronises inside the loop), and for the C schedule the arena bytes.  Behind
the arms of a width every C arm is set against the Python arm of its precision: "faster" / "slower" only where the two min .. max
ranges do not overlap, else "not separated".  Width 8 runs in f32 only ('bf16-mul' is an option of the wide models).

--small: the launch-bound frame of profiles/wide_decode.txt (a 6-bit sphere shell, 2,134 rows) instead of a config's frame 0.
--parent-lib PATH: a build of the PARENT commit's library (it lacks the wide step's exports): one more arm per precision, the Python
schedule on that library, run by a child process of this tool with LINR_HIP_LIB=PATH - a separate session, so it says what the
Adam launcher's and the layout header's refactoring cost the old path, not more."""
import argparse, json, os, statistics, subprocess, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ap = argparse.ArgumentParser()
ap.add_argument('cfg', nargs='?', default='loot10')
ap.add_argument('--train-precision', '--train_precision', dest='train_precision', default='f32')
ap.add_argument('--schedules', default='py,c')
ap.add_argument('--hidden', default='8,16,32')
ap.add_argument('--rounds', type=int, default=5)
ap.add_argument('--steps', type=int, default=10)
ap.add_argument('--small', action='store_true')
ap.add_argument('--parent-lib', dest='parent_lib', default=None)
ap.add_argument('--as-parent', dest='as_parent', action='store_true', help=argparse.SUPPRESS)
args = ap.parse_args()

from linr_pcgc_amd import _lib          # noqa: E402
NEW_EXPORTS = ('linr_net_wide_train_arena_bytes', 'linr_net_forward_train_wide', 'linr_net_backward_wide', 'linr_net_train_step_wide')
if args.as_parent:                      # the parent's library: bind what it has, run the Python schedule only
    for name in NEW_EXPORTS:
        _lib._PROTOS.pop(name, None)
    args.schedules = 'py'
import torch                            # noqa: E402
from linr_pcgc_amd import overfit, synthetic          # noqa: E402
from linr_pcgc_amd.model_core import FlatAdam, train_step          # noqa: E402

cfg = 'shell6' if args.small else args.cfg
cloud = synthetic.sphere_shell(6, 20) if args.small else synthetic.sequence_frame_device(args.cfg, 0, 'cuda')
gop = overfit.Gop(None, [cloud], None, 64, 'cuda')
frame, pn = gop.frames[0], gop.point_nums[0]


def verdict(a, b):
    """a against the baseline b, by their medians and min .. max ranges."""
    ma, mb = statistics.median(a), statistics.median(b)
    if max(a) < min(b):
        return '%.2fx, faster' % (mb / ma)
    if min(a) > max(b):
        return '%.2fx, slower' % (mb / ma)
    return '%.2fx, not separated (the min .. max ranges overlap)' % (mb / ma)


results = []
for hidden in [int(h) for h in args.hidden.split(',')]:
    arms = []
    for tp in (args.train_precision.split(',') if hidden != 8 else ['f32']):
        for sched in (args.schedules.split(',') if hidden != 8 else ['c']):
            m = overfit.gen_model(gop.scale_num, 'cuda', seed=8807, hidden=hidden)
            m.train_precision = tp
            if hidden != 8:
                m._wide.c_step = sched == 'c'
            arms.append({'tp': tp, 'sched': sched if hidden != 8 else '-', 'm': m, 'o': FlatAdam(m),
                         'bits': torch.zeros(1, dtype=torch.float64, device='cuda'), 'ms': [], 'cpu': [], 'first': None})
    for a in arms:
        for _ in range(3):
            train_step(a['m'], a['o'], frame, pn, out=a['bits'])
    for _ in range(args.rounds):
        for a in arms:
            torch.cuda.synchronize(); t0 = time.time(); c0 = time.thread_time()
            for i in range(args.steps):
                a['bits'].zero_(); train_step(a['m'], a['o'], frame, pn, out=a['bits'])
                if a['first'] is None: a['first'] = float(a['bits'])
            c1 = time.thread_time()
            torch.cuda.synchronize()
            a['ms'].append((time.time() - t0) * 1e3 / args.steps)
            a['cpu'].append((c1 - c0) * 1e3 / args.steps)
    for a in arms:
        arena = ''
        if hidden != 8 and a['sched'] == 'c':
            arena = ', arena %d bytes' % _lib.lib().linr_net_wide_train_arena_bytes(frame.rows, hidden, a['m'].block_layers)
        name = ('parent library, ' if args.as_parent else '') + 'schedule %s' % a['sched']
        print('%s (%d rows) hidden %2d %-8s %-12s: GPU %.3f ms/step (median of %d rounds, %.3f .. %.3f), thread CPU %.3f ms/step (%.3f .. %.3f), '
              '%d parameters, bits %.0f -> %.0f%s' % (
                  cfg, frame.rows, hidden, a['tp'], name, statistics.median(a['ms']), args.rounds, min(a['ms']), max(a['ms']),
                  statistics.median(a['cpu']), min(a['cpu']), max(a['cpu']), a['m'].flat_parameters().numel(), a['first'], float(a['bits']), arena))
        results.append({'hidden': hidden, 'tp': a['tp'], 'sched': a['sched'], 'ms': a['ms'], 'cpu': a['cpu']})
    for a in arms:
        base = [b for b in arms if b['tp'] == a['tp'] and b['sched'] == 'py']
        if a['sched'] == 'c' and base:
            print('    hidden %2d %-8s C against Python schedule: GPU %s; thread CPU %s' % (
                hidden, a['tp'], verdict(a['ms'], base[0]['ms']), verdict(a['cpu'], base[0]['cpu'])))
    sys.stdout.flush()

if args.as_parent:
    print('RESULTS ' + json.dumps(results))
elif args.parent_lib:
    cmd = [sys.executable, os.path.abspath(__file__), args.cfg, '--train-precision', args.train_precision, '--hidden',
           ','.join(h for h in args.hidden.split(',') if h != '8'), '--rounds', str(args.rounds), '--steps', str(args.steps), '--as-parent']
    if args.small:
        cmd.append('--small')
    env = dict(os.environ, LINR_HIP_LIB=os.path.abspath(args.parent_lib))
    done = subprocess.run(cmd, env=env, capture_output=True, text=True)
    if done.returncode != 0:
        print('parent library arm failed (exit %d): %s' % (done.returncode, done.stderr[-1500:]))
        sys.exit(1)
    for line in done.stdout.splitlines():
        if not line.startswith('RESULTS '):
            print(line)
            continue
        for p in json.loads(line[8:]):
            for r in results:
                if r['hidden'] == p['hidden'] and r['tp'] == p['tp'] and r['sched'] == 'py':
                    print('    hidden %2d %-8s Python schedule, this library against the parent\'s (separate sessions): GPU %s; thread CPU %s' % (
                        p['hidden'], p['tp'], verdict(r['ms'], p['ms']), verdict(r['cpu'], p['cpu'])))

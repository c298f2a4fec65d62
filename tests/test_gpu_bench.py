"""bench.py end to end on a small workload: a plain run prints the headline line only, and two runs with the same arguments
write the same outputs of their last timed step."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('bits', 'parameters', 'adam_exp_avg', 'adam_exp_avg_sq')


def test_plain_bench_line_and_outputs(tmp_path):
    cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '3', '--warmup', '1', '--ramp-s', '0',
           '--config', 'sphere8', '--gop', '2']
    lines, dumps = [], []
    for k in range(2):
        d = tmp_path / ('run%d' % k)
        r = subprocess.run(cmd + ['--dump-outputs', str(d)], cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        lines.append(json.loads(r.stdout.strip().splitlines()[-1]))
        dumps.append({n: np.load(d / (n + '.npy')) for n in NAMES})
    line = lines[0]
    for key in ('metric', 'value', 'unit', 'higher_is_better', 'dtype', 'ms_per_step', 'steps', 'warmup', 'bits_per_point'):
        assert key in line, key
    assert line['metric'] == 'encode_sec_per_frame' and line['unit'] == 's/frame' and line['higher_is_better'] is False
    assert line['dtype'] == 'f32' and line['steps'] == 3 and line['warmup'] == 1 and line['full'] is False
    assert line['ms_per_step'] > 0 and 0 < line['value'] and line['bits_per_point'] > 0
    for key in ('roofline', 'cpu_baseline', 'sequence', 'sequence_cold', 'bf16_codec', 'bf16_train', 'rough', 'hidden16'):
        assert line[key] is None, key                         # the legs beside the headline run with --full only
    out = dumps[0]
    assert out['bits'].dtype == np.float64 and out['bits'].shape == (1,) and float(out['bits'][0]) > 0
    n = out['parameters'].size
    assert n > 0 and all(out[k].dtype == np.float32 and out[k].shape == (n,) for k in NAMES[1:])
    assert all(np.isfinite(out[k]).all() for k in NAMES) and float(out['adam_exp_avg_sq'].max()) > 0
    for k in NAMES:
        assert np.array_equal(out[k], dumps[1][k]), k

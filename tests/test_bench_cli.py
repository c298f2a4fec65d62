"""bench.py's command line and its output dump (host side; the GPU run of the benchmark is tests/test_gpu_bench.py)."""
import sys

import numpy as np
import pytest
import torch


def _parse(monkeypatch, *argv):
    from bench.common import parse
    monkeypatch.setattr(sys, 'argv', ['bench.py'] + list(argv))
    return parse()


def test_plain_run_is_the_default(monkeypatch):
    a = _parse(monkeypatch, '--gpus', '1', '--steps', '7', '--warmup', '2')
    assert a.steps == 7 and a.warmup == 2 and a.gpus == 1
    assert a.full is False and a.dump_outputs is None
    a = _parse(monkeypatch, '--steps', '7', '--full', '--dump-outputs', 'out')
    assert a.full is True and a.dump_outputs == 'out'


@pytest.mark.parametrize('argv', [('--steps', '0'), ('--sequence', '--dump-outputs', 'out')])
def test_rejected_arguments(monkeypatch, argv):
    with pytest.raises(SystemExit):
        _parse(monkeypatch, *argv)


def test_dump_outputs_writes_float32_and_float64(tmp_path):
    from bench.common import dump_outputs
    arrays = {'bits': torch.tensor([12.5], dtype=torch.float64), 'parameters': torch.arange(5, dtype=torch.float32),
              'counts': np.arange(3, dtype=np.int64)}
    dump_outputs(str(tmp_path / 'd'), arrays)
    bits, par, cnt = (np.load(tmp_path / 'd' / (n + '.npy')) for n in ('bits', 'parameters', 'counts'))
    assert bits.dtype == np.float64 and bits.tolist() == [12.5]
    assert par.dtype == np.float32 and par.tolist() == [0, 1, 2, 3, 4]
    assert cnt.dtype == np.float32 and cnt.tolist() == [0, 1, 2]


def test_dump_outputs_keeps_to_64_mb(tmp_path):
    from bench.common import dump_outputs
    with pytest.raises(AssertionError):
        dump_outputs(str(tmp_path), {'big': np.zeros((64 << 20) // 4 + 1, dtype=np.float32)})
    assert not list(tmp_path.iterdir())

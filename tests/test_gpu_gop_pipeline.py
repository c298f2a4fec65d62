"""GPU: run.py --pipeline (GOP g is coded, written and checked on a background thread and stream while GOP g+1 overfits) leaves the
files, the losses and the checkpoint of the plain flow, reports the overlap, and fails the way the plain flow fails."""
import os
import threading

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SPHERE8 = ['--config', 'sphere8', '--frames', '6', '--gop', '2', '--first-epoch', '2', '--others-epoch', '2', '--decode']      # three GOPs
GOPS = ['gop_0_1', 'gop_2_3', 'gop_4_5']
# the plain flow's summary and per-GOP result, key for key, as they were before the flag existed
PLAIN_SUMMARY_KEYS = ['bits_per_point', 'frames', 'gops', 'ideal_speedup_bound', 'inputs_resident_before_t0', 'lossless', 'n_gpus', 'phase_a_s',
                      'phase_b_efficiency', 'phase_b_s', 'schedule', 'sec_per_frame', 'staging_s_this_rank', 'wall_s']
PLAIN_RESULT_KEYS = ['bpp', 'coded_epoch', 'coded_loss', 'decode_s', 'encode_s', 'epochs', 'frames', 'gop', 'lossless', 'loss', 'overfit_s', 'points',
                     'rank', 'seconds', 'stage_s']


def run_job(argv, out, pipeline=False):
    from linr_pcgc_amd import run
    args = run.parse(list(argv) + ['--out', str(out)] + (['--pipeline'] if pipeline else []))
    summary, results = run.run_sequence_job(args, 0, 1, None, files=run.resolve_files(args))
    return {'summary': summary, 'results': results, 'out': str(out)}


def tree(root):
    """{relative path: bytes} of every file under root."""
    files = {}
    for d, _, names in os.walk(root):
        for n in names:
            p = os.path.join(d, n)
            with open(p, 'rb') as f:
                files[os.path.relpath(p, root)] = f.read()
    return files


def same_streams(plain, piped):
    a, b = tree(os.path.join(plain['out'], 'result_enc')), tree(os.path.join(piped['out'], 'result_enc'))
    assert sorted(a) == sorted(b) and len(a) > 3 * 4
    for name in sorted(a):
        assert a[name] == b[name], name


def same_identities(plain, piped, gops):
    same_streams(plain, piped)
    rp, rq = plain['results'], piped['results']
    assert sorted(rp) == sorted(rq) == list(range(len(gops)))
    for g, name in enumerate(gops):
        assert rp[g]['gop'] == rq[g]['gop'] == name
        assert len(rp[g]['loss']) == 2 and rp[g]['loss'] == rq[g]['loss'], g
        assert rp[g]['coded_epoch'] == rq[g]['coded_epoch'] and rp[g]['coded_loss'] == rq[g]['coded_loss']
        assert rp[g]['bpp'] == rq[g]['bpp'] and rp[g]['points'] == rq[g]['points']
        assert rp[g]['lossless'] is True and rq[g]['lossless'] is True
    assert plain['summary']['bits_per_point'] == piped['summary']['bits_per_point']
    assert plain['summary']['lossless'] is True and piped['summary']['lossless'] is True
    cks = [torch.load(os.path.join(r['out'], 'output', gops[0], 'model.pth'), map_location='cpu', weights_only=False) for r in (plain, piped)]
    assert sorted(cks[0]['model']) == sorted(cks[1]['model']) and len(cks[0]['model']) > 0
    for k in cks[0]['model']:
        assert torch.equal(cks[0]['model'][k], cks[1]['model'][k]), k
    assert cks[0]['epoch'] == cks[1]['epoch'] and cks[0]['loss'] == cks[1]['loss']


@pytest.fixture(scope='module')
def sphere8_runs(pkg, tmp_path_factory):
    """The sphere8 sequence once plain and once with --pipeline (computed once, read by the tests below)."""
    root = tmp_path_factory.mktemp('pipeline')
    return run_job(SPHERE8, root / 'plain'), run_job(SPHERE8, root / 'piped', pipeline=True)


def test_pipelined_sequence_equals_the_plain_one(sphere8_runs):
    plain, piped = sphere8_runs
    same_identities(plain, piped, GOPS)


def test_summaries_and_results(sphere8_runs):
    plain, piped = sphere8_runs
    sp, sq = plain['summary'], piped['summary']
    assert sorted(sp) == PLAIN_SUMMARY_KEYS                                   # flag off: exactly the keys of before
    assert sorted(sq) == sorted(PLAIN_SUMMARY_KEYS + ['pipeline', 'gpu_train_fraction', 'finish_wait_s'])
    assert sq['pipeline'] is True and 0.0 < sq['gpu_train_fraction'] <= 1.0 and sq['finish_wait_s'] >= 0.0
    assert sq['phase_b_efficiency'] is not None and 0.0 < sq['phase_b_efficiency'] <= 1.0
    for g in range(3):
        assert sorted(plain['results'][g]) == sorted(PLAIN_RESULT_KEYS)
        assert sorted(piped['results'][g]) == sorted(PLAIN_RESULT_KEYS + ['finish_wait_s'])
        r = piped['results'][g]
        assert r['overfit_s'] > 0 and r['encode_s'] > 0 and r['decode_s'] > 0 and r['stage_s'] >= 0 and r['finish_wait_s'] >= 0
        assert abs(r['seconds'] - (r['stage_s'] + r['overfit_s'] + r['encode_s'] + r['decode_s'])) < 1e-2
    assert abs(sum(r['finish_wait_s'] for r in piped['results'].values()) - sq['finish_wait_s']) < 1e-3
    # the main thread's time: what it trained and what it waited lies inside the wall
    assert sum(r['overfit_s'] + r['finish_wait_s'] for r in piped['results'].values()) <= sq['wall_s'] + 1e-3
    ck = torch.load(os.path.join(piped['out'], 'output', GOPS[0], 'model.pth'), map_location='cpu', weights_only=False)
    assert 'encode_s' not in ck['result'] and ck['result']['loss'] == piped['results'][0]['loss']      # the training half only
    assert os.path.exists(os.path.join(piped['out'], 'output', 'rank0_done'))


def test_uneven_frames(pkg, tmp_path):
    """Three GOPs of two frames, every frame of another size: the GOP in the finish and the one in training differ in every shape."""
    from linr_pcgc_amd import synthetic
    ori = tmp_path / 'ori'
    ori.mkdir()
    for k in range(3):
        for t in range(2):
            np.save(str(ori / ('f%03d.npy' % (2 * k + t))), np.asarray(synthetic.sphere_shell(7, 30 + 5 * k + t)))
    argv = ['--ori_dir', str(ori), '--ori_dtype', 'npy', '--frames', '6', '--gop', '2', '--first-epoch', '2', '--others-epoch', '2', '--decode']
    plain = run_job(argv, tmp_path / 'plain')
    piped = run_job(argv, tmp_path / 'piped', pipeline=True)
    same_identities(plain, piped, GOPS)
    assert len({r['points'] for r in plain['results'].values()}) == 3


def test_bf16_device_codes_lockstep_decode(pkg, tmp_path):
    argv = SPHERE8 + ['--precision', 'bf16', '--device-codes', '--decode-lockstep', '2']
    plain = run_job(argv, tmp_path / 'plain')
    piped = run_job(argv, tmp_path / 'piped', pipeline=True)
    same_streams(plain, piped)
    assert [plain['results'][g]['loss'] for g in range(3)] == [piped['results'][g]['loss'] for g in range(3)]
    assert plain['summary']['lossless'] is True and piped['summary']['lossless'] is True


def test_a_failing_finish_fails_the_rank(pkg, tmp_path, monkeypatch):
    """A host-side error in the background half (here: writing GOP 1's files) raises out of run_sequence_job, leaves rank0_failed and
    no rank0_done, and no worker thread."""
    from linr_pcgc_amd import codec, run
    write_gop = codec.write_gop

    def failing_write(enc, result_dir):
        if os.path.basename(result_dir) == GOPS[1]:
            raise OSError('no space left for %s' % result_dir)
        return write_gop(enc, result_dir)

    monkeypatch.setattr(codec, 'write_gop', failing_write)
    out = tmp_path / 'out'
    args = run.parse(SPHERE8 + ['--out', str(out), '--pipeline'])
    before = set(threading.enumerate())
    with pytest.raises(OSError, match='no space left'):
        run.run_sequence_job(args, 0, 1, None)
    torch.cuda.synchronize()
    work = out / 'output'
    assert (work / 'rank0_failed').exists() and not (work / 'rank0_done').exists()
    assert set(threading.enumerate()) <= before
    assert (out / 'result_enc' / GOPS[0] / 'side_info.json').exists()        # GOP 0 was finished before
    assert not (out / 'result_enc' / GOPS[2]).exists()                        # nothing was started behind the failure

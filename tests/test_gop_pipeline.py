"""CPU: the GOP pipeline's hand-over logic (gop_parallel.FinishPipeline, run_sequence_pipelined) with fake train / finish callables:
finish(g) really runs beside train(g+1), one at a time and in order, its exception reaches the caller and the rank's markers."""
import os
import threading
import time

import pytest
import torch

from linr_pcgc_amd import gop_parallel as gp

WAIT_S = 10.0          # upper bound of every wait below: an implementation without overlap fails after it instead of hanging


def drive(pipe, n, train):
    """What a rank does: train(g), then hand GOP g over, for g = 0..n-1; then drain."""
    try:
        for g in range(n):
            pipe.hand_over(g, train(g))
        return pipe.drain()
    finally:
        pipe.close()


def test_finish_runs_while_the_next_gop_trains():
    n = 4
    trained = [threading.Event() for _ in range(n + 1)]
    trained[n].set()                                     # nothing is trained behind the last GOP

    def train(g):
        trained[g].set()
        return 'payload %d' % g

    def finish(g, payload):
        assert payload == 'payload %d' % g
        return trained[g + 1].wait(WAIT_S)               # True only if train(g+1) ran while this finish was in flight

    pipe = gp.FinishPipeline(finish)
    assert drive(pipe, n, train) == {g: True for g in range(n)}


def test_finishes_start_in_hand_over_order_one_at_a_time():
    n = 5
    lock = threading.Lock()
    state = {'in_flight': 0, 'max_in_flight': 0, 'started': [], 'threads': set(), 'handed': []}

    def train(g):
        state['handed'].append(g)
        return g * g

    def finish(g, payload):
        with lock:
            state['in_flight'] += 1
            state['max_in_flight'] = max(state['max_in_flight'], state['in_flight'])
            state['started'].append(g)
            state['threads'].add(threading.get_ident())
        time.sleep(0.002 * (n - g))                      # the earlier ones are the slower ones: a second worker would overtake
        with lock:
            state['in_flight'] -= 1
        return payload + 1

    pipe = gp.FinishPipeline(finish)
    out = drive(pipe, n, train)
    assert out == {g: g * g + 1 for g in range(n)}       # the drain returns every result, keyed by GOP
    assert state['started'] == state['handed'] == list(range(n))
    assert state['max_in_flight'] == 1 and len(state['threads']) == 1
    assert threading.get_ident() not in state['threads']


@pytest.mark.parametrize('bad', [1, 3])
def test_a_raising_finish_surfaces_at_the_next_hand_over_or_at_the_drain(bad):
    n = 4                                                # bad = 3: the last one, nothing is handed over behind it
    started, trained = [], []
    before = set(threading.enumerate())

    def train(g):
        trained.append(g)
        return g

    def finish(g, payload):
        started.append(g)
        if g == bad:
            raise KeyError('finish %d' % g)
        return g

    pipe = gp.FinishPipeline(finish)
    with pytest.raises(KeyError, match='finish %d' % bad):
        drive(pipe, n, train)
    assert started == list(range(bad + 1))               # no later finish is started
    assert trained == list(range(min(bad + 2, n)))       # it surfaced at the hand-over of bad + 1 (behind train(bad + 1)) or at the drain
    with pytest.raises(KeyError):
        pipe.drain()                                     # it stays raised
    assert set(pipe.results) == set(range(bad))
    assert set(threading.enumerate()) <= before          # close() ended the worker


def test_blocked_seconds_add_up():
    nap = 0.05

    def finish(g, payload):
        time.sleep(nap)
        return g

    pipe = gp.FinishPipeline(finish)
    t0 = time.time()
    out = drive(pipe, 3, lambda g: g)                    # training takes no time: the caller waits for all three finishes
    wall = time.time() - t0
    assert out == {0: 0, 1: 1, 2: 2}
    assert sorted(pipe.blocked) == [0, 1, 2] and all(v > 0.5 * nap for v in pipe.blocked.values())
    assert abs(sum(pipe.blocked.values()) - pipe.blocked_s) < 1e-9
    assert 3 * nap * 0.9 <= pipe.blocked_s <= wall


def _rank(rank, groups, work, out, release=None, fail_gop=None):
    """One rank of run_sequence_pipelined on fake halves; `out` receives what happened."""
    ck_path = os.path.join(work, gp.gop_name(groups[0]), 'model.pth')

    def train_first(group):
        return {'model': {'w': torch.full((2,), 3.0)}, 'result': {'trained': 0}}, ('half', 0)

    def train_other(group, ckpt):
        assert float(ckpt['model']['w'][0]) == 3.0 and ckpt['result'] == {'trained': 0}
        if release is not None and rank == 1:
            out['ckpt_there_when_rank1_trains'] = os.path.exists(ck_path)
            release.set()
        return {'trained': group[0]}, ('half', group[0])

    def finish(g, payload):
        assert payload == ('half', groups[g][0])
        if g == 0 and release is not None:
            out['finish0_released'] = release.wait(WAIT_S)
        if g == fail_gop:
            raise OSError('disk full in GOP %d' % g)
        return {'finished': g, 'rank': rank}

    try:
        out['results'], pipe = gp.run_sequence_pipelined(groups, work, train_first, train_other, finish, rank, 2, None, schedule='static')
        out['blocked'] = pipe.blocked
    except BaseException as e:
        out['error'] = e


def test_two_ranks_the_checkpoint_is_there_before_gop0_is_finished(tmp_path):
    """Rank 1 trains only once it has the GOP-0 checkpoint; rank 0's finish(0) is held until rank 1 has trained.  A flow that codes
    GOP 0 before it writes model.pth leaves rank 1 waiting for the file and finish(0) for rank 1: the wait times out."""
    groups = gp.split_gops(12, 4)                        # rank 0: GOPs 0 and 1, rank 1: GOP 2
    work = str(tmp_path / 'work')
    release = threading.Event()
    outs = [{}, {}]
    threads = [threading.Thread(target=_rank, args=(r, groups, work, outs[r], release)) for r in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(3 * WAIT_S)
    assert not any(t.is_alive() for t in threads)
    assert 'error' not in outs[0] and 'error' not in outs[1], (outs[0].get('error'), outs[1].get('error'))
    assert outs[0]['finish0_released'] is True and outs[1]['ckpt_there_when_rank1_trains'] is True
    assert outs[0]['results'] == {0: {'finished': 0, 'rank': 0}, 1: {'finished': 1, 'rank': 0}}      # no placeholder is left
    assert outs[1]['results'] == {2: {'finished': 2, 'rank': 1}}
    assert sorted(outs[0]['blocked']) == [0, 1]
    ck = torch.load(os.path.join(work, 'gop_0_3', 'model.pth'), weights_only=False)
    assert ck['result'] == {'trained': 0}                # the training half only: nothing of the finish is pickled
    gp.wait_all_done(work, 2, timeout_s=WAIT_S)


def test_two_ranks_a_failing_finish_marks_the_rank_failed(tmp_path):
    groups = gp.split_gops(12, 4)
    work = str(tmp_path / 'work')
    before = set(threading.enumerate())
    outs = [{}, {}]
    _rank(0, groups, work, outs[0], fail_gop=1)          # GOP 1 is rank 0's last: its finish raises in the drain
    assert isinstance(outs[0].get('error'), OSError) and 'GOP 1' in str(outs[0]['error'])
    assert os.path.exists(os.path.join(work, 'rank0_failed')) and not os.path.exists(os.path.join(work, 'rank0_done'))
    assert set(threading.enumerate()) <= before
    _rank(1, groups, work, outs[1])                      # GOP 0 was trained: its checkpoint is there, rank 1 does its share
    assert outs[1].get('results') == {2: {'finished': 2, 'rank': 1}} and os.path.exists(os.path.join(work, 'rank1_done'))
    t0 = time.time()
    with pytest.raises(RuntimeError, match='rank0_failed'):
        gp.wait_all_done(work, 2, timeout_s=WAIT_S)      # ... and raises in front of the reductions instead of waiting for rank 0
    assert time.time() - t0 < 0.5 * WAIT_S


def test_a_failing_first_finish_surfaces_behind_the_next_training(tmp_path):
    """finish(0) raises: rank 0 notices at the hand-over of its next GOP; the checkpoint was written (GOP 0 was trained)."""
    groups = gp.split_gops(12, 4)
    work = str(tmp_path / 'work')
    out = {}
    _rank(0, groups, work, out, fail_gop=0)
    assert isinstance(out.get('error'), OSError) and 'GOP 0' in str(out['error'])
    assert os.path.exists(os.path.join(work, 'gop_0_3', 'model.pth'))
    assert os.path.exists(os.path.join(work, 'rank0_failed')) and not os.path.exists(os.path.join(work, 'rank0_done'))


def test_pipeline_flag_is_opt_in(capsys):
    from linr_pcgc_amd import run
    assert run.parse([]).pipeline is False and run.parse(['--pipeline']).pipeline is True
    with pytest.raises(SystemExit):
        run.parse(['--help'])
    assert 'three GOPs are resident' in ' '.join(capsys.readouterr().out.split())

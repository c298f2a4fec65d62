"""The live kernel timing of the library (csrc/prof.hip; include/linr_hip.h: linr_prof_mask / _enable / _read) as bench/headline.py,
bench/roofline.py and bench/bf16_train.py use it: which launches of a training step are bracketed under which kernel class and with
how many row passes, what the class mask selects, and what the three modes of linr_prof_enable do to the records.
"""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

KINDS = 24          # LINR_PROF_KINDS

# (launches, passes) of classes 0 .. 23 (the list in include/linr_hip.h) for ONE training step on the golden shell (5 scales,
# block_layers 1, default schedule).  Pasted from what _collect() below printed with LINR_HIP_LIB pointed at a build of the commit
# BEFORE the profiler moved out of csrc/net.hip - not taken from the code under test.  Cross-check only: DESIGN.md counts 21 / 22
# launches per step, 20 / 19 of them are bracketed (the reduction's bracket also holds the embedding-gradient launch).
Z = (0, 0)
FP32_STEP = [(3, 17), (3, 9), (1, 8), (1, 8), (1, 8), (1, 8), (1, 8), (1, 7), (1, 8), (1, 7), Z, (2, 2), (4, 0), Z,
             Z, Z, Z,
             Z, Z, Z, Z, Z, Z, Z]
BF16_STEP = [Z, Z, Z, Z, Z, Z, Z, Z, Z, Z, Z, (1, 1), (1, 0), Z,
             Z, Z, Z,
             (3, 17), (1, 8), (1, 8), (7, 40), (1, 8), (1, 7), (3, 2)]

def _read(L, kind):
    tot, nl, npass = ctypes.c_double(), ctypes.c_int64(), ctypes.c_int64()
    assert L.linr_prof_read(kind, ctypes.byref(tot), ctypes.byref(nl), ctypes.byref(npass)) == 0
    return tot.value, nl.value, npass.value


def _stepper(pkg, shell, precision):
    from linr_pcgc_amd.model_core import FlatAdam, train_step
    from gpu_common import _model_and_oracle
    model, _ = _model_and_oracle(pkg, 5)
    model.train_precision = precision
    frame = model.make_frame(shell['scales'])
    opt = FlatAdam(model)

    def step():
        train_step(model, opt, frame, shell['point_num'])
        torch.cuda.synchronize()
    return step


def _collect(pkg, shell, precision, mask=0xFFFFFFFF):
    """One training step with every class of `mask` recorded -> [(total_ms, launches, passes)] of all 24 classes"""
    from linr_pcgc_amd import _lib
    L = _lib.lib()
    step = _stepper(pkg, shell, precision)
    torch.cuda.synchronize()
    try:
        L.linr_prof_mask(mask)
        assert L.linr_prof_enable(1) == 0
        step()
        L.linr_prof_enable(0)
        return [_read(L, k) for k in range(KINDS)]
    finally:
        L.linr_prof_mask(3)
        L.linr_prof_enable(0)


@pytest.mark.parametrize('precision', ['f32', 'bf16'])
def test_a_training_step_records_the_expected_launches_per_class(pkg, shell, precision):
    want = FP32_STEP if precision == 'f32' else BF16_STEP
    got = _collect(pkg, shell, precision)
    print(precision, [(nl, npass) for _, nl, npass in got])
    assert [(nl, npass) for _, nl, npass in got] == want
    for k, (ms, nl, _) in enumerate(got):
        assert (ms > 0) == (nl > 0), (k, ms, nl)


def test_mask_selects_the_classes_and_the_modes_keep_or_clear_the_records(pkg, shell):
    from linr_pcgc_amd import _lib
    L = _lib.lib()
    got = _collect(pkg, shell, 'f32', mask=3)
    assert [(nl, npass) for _, nl, npass in got[:2]] == FP32_STEP[:2] and all(nl > 0 for _, nl, _ in got[:2])
    assert all((nl, npass) == (0, 0) and ms == 0 for ms, nl, npass in got[2:])
    step = _stepper(pkg, shell, 'f32')
    try:
        L.linr_prof_mask(3)
        step()                                             # stopped (mode 0): nothing is added
        assert [_read(L, k)[1:] for k in range(KINDS)] == [g[1:] for g in got]
        assert L.linr_prof_enable(2) == 0                  # resume: the records stay, this step's come on top
        step()
        L.linr_prof_enable(0)
        assert [_read(L, k)[1:] for k in range(2)] == [(2 * nl, 2 * npass) for _, nl, npass in got[:2]]
        assert all(_read(L, k)[0] > got[k][0] for k in range(2))
        assert all(_read(L, k) == (0.0, 0, 0) for k in range(2, KINDS))
        assert L.linr_prof_enable(1) == 0                  # clear + start
        L.linr_prof_enable(0)
        assert all(_read(L, k) == (0.0, 0, 0) for k in range(KINDS))
    finally:
        L.linr_prof_mask(3)
        L.linr_prof_enable(0)


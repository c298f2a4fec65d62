"""CPU: the averaged weights' host side.  linr_params_average_host - the plain-loop twin of the averaging kernel and the definition of
its arithmetic, avg[k][i] = fmaf(w_k, params[i] - avg[k][i], avg[k][i]) with the difference rounded to fp32 on its own - against the
same expression in float64; the debias scale; run.py's flags; and codec.search_average on CPU models with a stub in the place of the
codec's forward.

The float64 comparison is a sanity bound, the twin's text is the definition: with d = fl32(p - a) exact in double, w * d is exact in
double too (24 x 24 bits), so the float64 value w * d + a is within 2^-53 relative of the exact one and the twin's single fp32 rounding
of the exact value is within ONE fp32 ulp of the float64 value rounded to fp32.

On `w = 1 copies params`: fmaf(1, fl32(p - a), a) is p exactly where the average is zero (the first update from the zeroed buffer; -0
comes out as +0), where a == p, and wherever p - a is exact (p within a factor of two of a, Sterbenz).  Elsewhere the difference is
rounded BEFORE a is added back, so the result is p only to half an ulp of the difference plus half an ulp of the result; the test
asserts exactly these three statements and that bound, not more than the defined arithmetic gives."""
import ctypes
import os

import numpy as np
import pytest
import torch

NS = (1, 3, 4, 5, 1023, 1024, 1025, 54712)
KS = (1, 4)
UPDATES = 5
SENTINEL = np.float32(77.0)
DECAYS = (0.5, 0.9, 0.97, 0.99)


@pytest.fixture(scope='module')
def lib():
    from linr_pcgc_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.lib()


def values(n, seed):
    """n floats with magnitudes over 2^-20 .. 2^4, both signs, and +-0, +-inf and NaN planted where n leaves room."""
    rng = np.random.default_rng(seed)
    p = (np.ldexp(1.0 + rng.random(n), rng.integers(-20, 5, n)) * rng.choice([-1.0, 1.0], n)).astype(np.float32)
    special = [0.0, -0.0, np.inf, -np.inf, np.nan]
    if n >= 1023:
        for j, v in enumerate(special):
            p[(seed + 1 + 11 * j) % n] = np.float32(v)
    elif n >= 3:
        p[seed % n] = np.float32(special[seed % 5])
    return p


def weights(K):
    from linr_pcgc_amd import overfit
    return overfit.avg_weights(DECAYS[:K])


def chain_host(lib, n, K, stride, seed, updates=UPDATES, w=None):
    """`updates` chained calls of the twin on a [K][stride] buffer whose rows start at zero and whose padding holds a sentinel.
    Returns (the parameter vectors, the buffer after every update)."""
    w = weights(K) if w is None else np.ascontiguousarray(w, dtype=np.float32)
    avg = np.full((K, stride), SENTINEL, dtype=np.float32)
    avg[:, :n] = 0.0
    ps, states = [], []
    for t in range(updates):
        p = values(n, seed + t)
        rc = lib.linr_params_average_host(p.ctypes.data, n, w.ctypes.data, K, stride, avg.ctypes.data)
        assert rc == 0
        ps.append(p)
        states.append(avg.copy())
    return ps, states


def _ulp_apart(got, want32):
    """|got - want32| <= one fp32 ulp, elementwise; NaN matches NaN, an infinity itself."""
    same = (got == want32) | (np.isnan(got) & np.isnan(want32))
    up, down = np.nextafter(want32, np.float32(np.inf)), np.nextafter(want32, np.float32(-np.inf))
    return same | (got == up) | (got == down)


@pytest.mark.parametrize('K', KS)
@pytest.mark.parametrize('n', NS)
def test_twin_agrees_with_float64_within_one_ulp(lib, n, K):
    for stride in ((n + 3) & ~3, ((n + 3) & ~3) + 8):
        w = weights(K)
        ps, states = chain_host(lib, n, K, stride, 31 * n + K)
        before = np.zeros((K, n), dtype=np.float32)
        with np.errstate(invalid='ignore', over='ignore'):
            for p, after in zip(ps, states):
                d = (p[None, :].astype(np.float64) - before.astype(np.float64)).astype(np.float32)          # one fp32 rounding
                want = w[:, None].astype(np.float64) * d.astype(np.float64) + before.astype(np.float64)
                got = after[:, :n]
                ok = _ulp_apart(got, want.astype(np.float32))
                assert ok.all(), (n, K, stride, np.argwhere(~ok)[:4])
                assert np.all(after[:, n:] == SENTINEL)                                # stride > n: the tail is not touched
                before = got.copy()
        if n >= 1023:                                                                  # NaN and inf propagate into every row
            assert np.isnan(states[-1][:, :n]).any(axis=1).all()


@pytest.mark.parametrize('n', NS)
def test_weight_one(lib, n):
    stride = (n + 3) & ~3
    ps, states = chain_host(lib, n, 1, stride, 7 * n, updates=3, w=[1.0])
    # into a zero average: the parameters themselves (-0 as +0), NaN and inf included
    first, p0 = states[0][0, :n], ps[0]
    assert np.array_equal(first[~np.isnan(p0)], p0[~np.isnan(p0)]) and np.isnan(first[np.isnan(p0)]).all()
    assert not np.signbit(first[p0 == 0]).any()
    # onto itself: unchanged where finite
    w1 = np.ones(1, np.float32)
    buf = np.zeros((1, stride), np.float32)
    buf[0, :n] = first
    assert lib.linr_params_average_host(p0.ctypes.data, n, w1.ctypes.data, 1, stride, buf.ctypes.data) == 0
    fin = np.isfinite(first)
    assert np.array_equal(buf[0, :n][fin].view(np.uint32), first[fin].view(np.uint32))
    # onto another finite average: exact where p - a is exact (Sterbenz), and within half an ulp of the difference plus half an ulp of
    # the result everywhere - the difference is rounded before the average is added back
    a, p, got = states[0][0, :n], ps[1], states[1][0, :n]
    both = np.isfinite(a) & np.isfinite(p)
    with np.errstate(invalid='ignore', divide='ignore'):
        sterbenz = both & (a != 0) & (p / a >= 0.5) & (p / a <= 2.0)
        assert np.array_equal(got[sterbenz], p[sterbenz])
        d = p.astype(np.float64) - a.astype(np.float64)
        bound = 0.5 * np.spacing(np.abs(d).astype(np.float32)).astype(np.float64) + 0.5 * np.spacing(np.abs(got)).astype(np.float64)
        assert np.all(np.abs(got.astype(np.float64) - p.astype(np.float64))[both] <= bound[both])
    # an infinite average does not come back: inf - inf
    assert np.isnan(got[np.isinf(a)]).all()


def test_every_refused_argument_returns_its_code_and_writes_nothing(lib):
    p = values(64, 1)
    w = np.array([0.5, 1.0], dtype=np.float32)
    avg = np.full((2, 64), SENTINEL, dtype=np.float32)
    bad_w = {name: np.array(v, dtype=np.float32) for name, v in
             (('zero', [0.0, 0.5]), ('big', [0.5, 1.0000001]), ('neg', [-0.1, 0.5]), ('nan', [0.5, np.nan]), ('inf', [np.inf, 0.5]))}
    good = dict(params=p.ctypes.data, n=64, w=w.ctypes.data, K=2, stride=64, avg=avg.ctypes.data)
    bad = [({'n': -1}, -1), ({'K': 0}, -1), ({'K': 5}, -1), ({'K': -1}, -1), ({'w': None}, -1)] + \
          [({'w': v.ctypes.data}, -1) for v in bad_w.values()] + \
          [({'stride': 63}, -1), ({'stride': 60}, -1), ({'stride': 66}, -1), ({'n': 62, 'stride': 62}, -1), ({'params': None}, -1), ({'avg': None}, -1)]

    def host(a):
        return lib.linr_params_average_host(a['params'], a['n'], a['w'], a['K'], a['stride'], a['avg'])
    for change, code in bad:
        assert host(dict(good, **change)) == code, change
        assert np.all(avg == SENTINEL), change                                          # refused: nothing written
    assert host(dict(good, n=0, stride=0, params=None, avg=None)) == 0                     # empty: nothing to do
    assert host(dict(good, n=0)) == 0 and np.all(avg == SENTINEL)
    avg[:] = 0.0
    assert host(good) == 0 and np.array_equal(avg[1, ~np.isnan(p)], p[~np.isnan(p)])

    # the device entry checks the same, and the alignment of what the kernel reads and writes 16 bytes at a time, before any launch
    buf = (ctypes.c_char * 4096)()
    a = (ctypes.addressof(buf) + 63) & ~63
    good = dict(params=a, n=64, w=w.ctypes.data, K=2, stride=64, avg=a + 1024)
    bad = bad + [({'params': a + 4}, -3), ({'avg': a + 1028}, -3), ({'avg': a + 1032}, -3)]

    def device(x):
        return lib.linr_params_average(x['params'], x['n'], x['w'], x['K'], x['stride'], x['avg'], None)
    for change, code in bad:
        assert device(dict(good, **change)) == code, change
    assert device(dict(good, n=0, stride=0, params=None, avg=None)) == 0                   # empty: nothing is launched

    # linr_overfit_gop_avg refuses what linr_overfit_gop refuses, in front of anything else
    assert lib.linr_overfit_gop_avg(None, None, None, None, None) == -1 == lib.linr_overfit_gop(None, None, None, None)


def test_weights_and_debias_scales():
    from linr_pcgc_amd import overfit
    w = overfit.avg_weights((0.5, 0.9, 0.99))
    assert w.dtype == np.float32 and w.tolist() == [np.float32(0.5), np.float32(1 - 0.9), np.float32(1 - 0.99)]
    assert overfit.avg_weights(None).size == 0 and overfit.avg_weights(()).size == 0
    assert overfit.avg_weights((0.0,)).tolist() == [1.0]
    for bad in ((1.0,), (-0.1,), (1.5,), (float('nan'),), (0.1, 0.2, 0.3, 0.4, 0.5)):
        with pytest.raises(ValueError):
            overfit.avg_weights(bad)
    for T in (1, 2, 8, 64, 320):
        s = overfit.avg_debias_scales(w, T)
        assert s.dtype == np.float32
        for wk, sk in zip(w, s):
            d = 1.0 - float(wk)                                   # the decay that is applied: of the fp32 weight, in double
            assert sk == np.float32(1.0 / (1.0 - d ** T))
    assert overfit.avg_debias_scales(overfit.avg_weights((0.0,)), 3).tolist() == [1.0]
    assert overfit.avg_debias_scales(w, 1).tolist() == [np.float32(1.0 / float(x)) for x in w]
    with pytest.raises(ValueError):
        overfit.avg_debias_scales(w, 0)


def test_debiased_average_of_a_constant_is_the_constant(lib):
    """T updates with the same vector c leave avg = (1 - d^T) c up to rounding: the debiased read-out gives c back within a few ulp."""
    from linr_pcgc_amd import overfit
    c = values(1024, 3)
    c = c[np.isfinite(c)]
    n, stride = c.size, (c.size + 3) & ~3
    w = overfit.avg_weights((0.5, 0.9, 0.99))
    for T in (1, 5, 40):
        avg = np.zeros((3, stride), dtype=np.float32)
        for _ in range(T):
            assert lib.linr_params_average_host(c.ctypes.data, n, w.ctypes.data, 3, stride, avg.ctypes.data) == 0
        hat = avg[:, :n] * overfit.avg_debias_scales(w, T)[:, None]
        # every update rounds twice (the difference, the fma): the error of the sum stays below 2 T ulp of |c|, the scale adds one
        err = np.abs(hat.astype(np.float64) - c.astype(np.float64)[None, :])
        assert np.all(err <= (2 * T + 2) * overfit.avg_debias_scales(w, T)[:, None].astype(np.float64) * np.spacing(np.abs(c)).astype(np.float64)[None, :])


def test_run_flags_are_parsed():
    from linr_pcgc_amd import run
    a = run.parse([])
    assert a.avg_decays is None and a.avg_frames == 4
    a = run.parse(['--avg-decays', '0.9,0.97,0.99', '--avg-frames', '0'])
    assert a.avg_decays == (0.9, 0.97, 0.99) and a.avg_frames == 0
    assert run.parse(['--avg_decays', '0', '--avg_frames', '2']).avg_decays == (0.0,)
    for bad in (['--avg-decays', '0.9,x'], ['--avg-decays', '1.0'], ['--avg-decays', '-0.5'], ['--avg-decays', '0.1,0.2,0.3,0.4,0.5'],
                ['--avg-decays', ''], ['--avg-decays', 'nan'], ['--avg-frames', '-1']):
        with pytest.raises(SystemExit):
            run.parse(bad)


# ---- the choice, on CPU models with a stub in the place of the codec's forward ------------------------------------------------------
def _cpu_models(seed=8807):
    from linr_pcgc_amd.model_core import LINR_PCGC_Model
    torch.manual_seed(seed)
    gen = lambda: LINR_PCGC_Model({'scale_num': 3, 'in_channel': 7, 'hidden_channel_conv': 8, 'block_layers': 1, 'outstage': 8, 'instage': 1})
    return gen(), gen()


def _stub(table):
    """frame_bits(candidate, i): looked up by the candidate's filled parameters - the bits of frame i as a float64[1] tensor."""
    calls = []

    def frame_bits(cand, i):
        key = float(cand.flat_parameters().detach().double().sum())
        calls.append((key, i))
        return torch.tensor([table(key, i)], dtype=torch.float64)
    frame_bits.calls = calls
    return frame_bits


def test_search_average_tie_goes_to_the_plain_candidate(lib):
    from linr_pcgc_amd import codec
    model, shell = _cpu_models()
    flat = model.flat_parameters().detach()
    same = torch.stack([flat.clone(), flat.clone()])
    got = codec.search_average(model, shell, [None] * 6, same, (0.5, 0.9), 8, 'f32', 4, frame_bits=_stub(lambda key, i: 1000.0 + i))
    assert got['decays'] == [0.5, 0.9] and got['frames'] == [0, 2, 3, 5] == codec.qrange_eval_frames(6, 4)
    assert got['objective_bits'][0] == got['objective_bits'][1] == got['objective_bits'][2] and got['chosen'] == 0
    assert got['search_s'] >= 0


def test_search_average_objective_and_nan(lib):
    from linr_pcgc_amd import codec
    from linr_pcgc_amd.model_codec import compress_params, laplace_bits_est
    model, shell = _cpu_models()
    flat = model.flat_parameters().detach()
    n = flat.numel()
    rng = torch.Generator().manual_seed(5)
    better = flat * 0.5                                                        # another vector: other codes, another model size
    poisoned = flat.clone()
    poisoned[n // 2] = float('nan')
    infinite = flat.clone()
    infinite[3] = float('inf')
    noisy = flat + 0.01 * torch.randn(n, generator=rng)
    cands = torch.stack([poisoned, better, infinite, noisy])
    # frame bits per candidate, keyed by what _fill wrote: the NaN and inf candidates would be cheapest by far if they were asked
    recon = {j: compress_params(v, 8)['recon_ret'] for j, v in ((0, flat), (2, better), (4, noisy))}
    key_of = {float(r.double().sum()): j for j, r in recon.items()}
    per_frame = {0: 5000.0, 2: 4000.0, 4: 9000.0}
    stub = _stub(lambda key, i: per_frame[key_of[key]] + 0.25 * i)
    got = codec.search_average(model, shell, [None] * 3, cands, (0.1, 0.2, 0.3, 0.4), 8, 'f32', 2, frame_bits=stub)
    todo = [0, 2]
    assert got['frames'] == todo
    assert got['objective_bits'][1] is None and got['objective_bits'][3] is None          # never evaluated ...
    assert sorted({key_of[k] for k, _ in stub.calls}) == [0, 2, 4] and len(stub.calls) == 3 * len(todo)
    want = {}
    for j, v in ((0, flat), (2, better), (4, noisy)):
        out = compress_params(v, 8)
        dev = int(np.abs(out['symbols'].astype(np.int64) - int(out['mu'])).sum())
        want[j] = laplace_bits_est(n, dev, 8) + 3 / 2 * sum(per_frame[j] + 0.25 * i for i in todo)
        assert got['objective_bits'][j] == want[j], j
    assert got['chosen'] == min(want, key=lambda j: (want[j], j)) == 2                    # ... and never win
    # what was filled is the codec's own de-quantised vector, bit for bit (the host twin of the range kernel under the own range)
    assert torch.equal(shell.flat_parameters().detach().view(torch.int32), recon[4].view(torch.int32))
    # only non-finite candidates beside the plain one: plain
    only = codec.search_average(model, shell, [None] * 3, torch.stack([poisoned, infinite]), (0.1, 0.2), 8, 'f32', 0, frame_bits=_stub(lambda k, i: 1.0))
    assert only['chosen'] == 0 and only['objective_bits'][1:] == [None, None] and only['frames'] == [0, 1, 2]
    with pytest.raises(ValueError):
        codec.search_average(model, shell, [None] * 3, cands[:2], (0.1, 0.2, 0.3), 8, 'f32', 2, frame_bits=stub)
    with pytest.raises(ValueError):
        codec.search_average(model, shell, [None] * 3, cands[:, :-1], (0.1, 0.2, 0.3, 0.4), 8, 'f32', 2, frame_bits=stub)


def test_declared_exported_and_bound(lib):
    from linr_pcgc_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, 'include', 'linr_hip.h')).read()
    for name in ('linr_params_average', 'linr_params_average_host', 'linr_overfit_gop_avg'):
        assert name in _lib.EXPORTS and hasattr(lib, name) and name + '(' in header
    assert '#define LINR_ABI_VERSION 27' in header and _lib.ABI_VERSION == 27 == lib.linr_abi_version()          # additive: the ABI stays
    assert ctypes.sizeof(_lib.LinrOverfitAvg) == 40 and _lib.LinrOverfitAvg.avg.offset == 24 and _lib.LinrOverfitAvg.stride.offset == 32


def test_twin_under_sanitizers(tmp_path):
    """tools/params_average_emul.cpp: the twin on exact-size heap buffers - the sizes, row counts and strides above over chained
    updates against a restatement in double, the padding, the refusals - under AddressSanitizer + UBSan.  Host code only, a program of
    its own."""
    import shutil
    import subprocess
    if shutil.which('g++') is None:
        pytest.skip('no g++')
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / 'params_average_emul')
    build = subprocess.run(['g++', '-O1', '-g', '-std=c++17', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined',
                            '-fno-omit-frame-pointer', '-o', exe, os.path.join(root, 'tools', 'params_average_emul.cpp'),
                            os.path.join(root, 'linr_pcgc_amd', 'csrc', 'params_avg_host.cpp')], capture_output=True, text=True, timeout=600)
    if build.returncode != 0 and 'asan' in (build.stderr or '').lower():
        pytest.skip('sanitizer runtime not installed')
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0 and 'all as expected' in run.stdout, (run.stdout[-500:], run.stderr[-3000:])

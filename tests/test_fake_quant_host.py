"""CPU: the weight quantiser behind the quantisation-aware overfit (linr_params_fake_quant_host, a plain loop over the element
functions of csrc/fake_quant.h that the device kernel is built from) against the model codec itself: model_codec.quant_uniform2's
codes and its de-quantised vector, which is what decompress_params rebuilds.  Every comparison is exact: codes as integers,
reconstructions as bit patterns.  Also the small pure pieces of the feature's Python surface."""
import os

import numpy as np
import pytest
import torch

DEPTHS = (4, 8, 12)
NS = (1, 2, 63, 64, 65, 1023, 1024, 1025, 70001)
SCALES = (1e-3, 0.05, 1.0, 30.0)


@pytest.fixture(scope='module')
def lib():
    from linr_pcgc_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.lib()


def fake_quant_host(lib, p, bitdepth, codes=True, minmax=True):
    p = np.ascontiguousarray(p, dtype=np.float32)
    q = np.full(p.size, 7.0, dtype=np.float32)
    c = np.full(p.size, 77, dtype=np.uint16) if codes else None
    mm = np.full(2, 7.0, dtype=np.float32) if minmax else None
    rc = lib.linr_params_fake_quant_host(p.ctypes.data, p.size, bitdepth, q.ctypes.data, None if c is None else c.ctypes.data,
                                         None if mm is None else mm.ctypes.data)
    assert rc == 0
    return q, c, mm


def codec_reference(p, bitdepth):
    """quant_uniform2 on the CPU in fp32: (codes, reconstruction)."""
    from linr_pcgc_amd import model_codec
    codes, recon = model_codec.quant_uniform2(torch.from_numpy(np.ascontiguousarray(p, dtype=np.float32)), bitdepth)
    return codes.numpy(), recon.numpy()


def assert_equals_codec(lib, p, bitdepth):
    q, c, mm = fake_quant_host(lib, p, bitdepth)
    codes, recon = codec_reference(p, bitdepth)
    assert np.array_equal(c.astype(np.float32), codes)
    assert np.array_equal(q.view(np.uint32), recon.view(np.uint32))
    assert mm[0] == p.min() and mm[1] == p.max()
    assert int(c.max()) <= 2 ** bitdepth - 1


def planted(n, scale, bitdepth, seed):
    """A random vector of n floats with, where they fit, values at exact half steps of the quantiser (round-half-to-even ties as far
    as fp32 lets them be ties), one ulp above the minimum and one ulp below the maximum."""
    rng = np.random.default_rng(seed)
    p = (rng.standard_normal(n) * scale).astype(np.float32)
    if n < 8:
        return p
    lo, hi = np.float32(-3.0 * scale), np.float32(4.0 * scale)
    p = np.clip(p, lo, hi)
    p[0], p[1] = lo, hi
    p[2], p[3] = np.nextafter(lo, hi), np.nextafter(hi, lo)
    s = 2 ** bitdepth - 1
    k = np.arange(min(s, 255, n - 4), dtype=np.float64)
    if bitdepth > 8:
        k = k * (s // 255)                          # 255 of the half steps, spread over the whole range
    half = (np.float64(lo) + (k + 0.5) / s * (np.float64(hi) - np.float64(lo))).astype(np.float32)
    p[4:4 + half.size] = half
    return p


def test_golden_model_weights(lib, golden_dir):
    flat = np.load(os.path.join(golden_dir, 'loot_model_kat.npz'))['flat'].astype(np.float32)
    assert flat.size == 54712
    for bitdepth in DEPTHS:
        assert_equals_codec(lib, flat, bitdepth)


@pytest.mark.parametrize('bitdepth', DEPTHS)
@pytest.mark.parametrize('n', NS)
def test_random_vectors_with_planted_ties(lib, n, bitdepth):
    for i, scale in enumerate(SCALES):
        p = planted(n, scale, bitdepth, 1000 * n + 10 * bitdepth + i)
        if n == 1:
            continue                                # one value: min == max, see test_constant_vector
        if p.min() == p.max():
            p[1] = p[0] + np.float32(scale)
        assert_equals_codec(lib, p, bitdepth)


def test_all_255_half_steps_at_8_bits(lib):
    """On a range where the half steps are exact in fp32 (min 0, max 255: step 1) every x.5 is a true tie: the codes must be the
    even neighbours, as torch.round gives them."""
    p = np.concatenate([[0.0, 255.0], np.arange(255) + 0.5]).astype(np.float32)
    q, c, _ = fake_quant_host(lib, p, 8)
    want = np.concatenate([[0, 255], 2 * ((np.arange(255) + 1) // 2)])
    assert np.array_equal(c, want)
    assert_equals_codec(lib, p, 8)
    for scale in SCALES:                            # ... and scaled ranges, whatever fp32 makes of the ties there
        assert_equals_codec(lib, (p * np.float32(scale / 255.0) - np.float32(0.37 * scale)).astype(np.float32), 8)


def test_constant_vector(lib):
    """max == min: codes 0 and the parameters themselves (quant_uniform2 yields NaN here; no trained model hits it)."""
    for n in (1, 5, 1025):
        p = np.full(n, 0.25, dtype=np.float32)
        q, c, mm = fake_quant_host(lib, p, 8)
        assert np.array_equal(q, p) and not c.any() and mm.tolist() == [0.25, 0.25]


def test_nan_and_code_range(lib):
    p = np.array([0.5, np.nan, -1.0, 2.0, 0.0], dtype=np.float32)
    q, c, mm = fake_quant_host(lib, p, 8)
    assert np.isnan(q[1]) and c[1] == 0
    assert mm.tolist() == [-1.0, 2.0]
    keep = np.array([0, 2, 3, 4])
    codes, recon = codec_reference(p[keep], 8)
    assert np.array_equal(c[keep].astype(np.float32), codes) and np.array_equal(q[keep].view(np.uint32), recon.view(np.uint32))
    p = np.array([-np.inf, 0.0, 1.0, np.inf], dtype=np.float32)
    for bitdepth in (2, 8, 16):
        _, c, _ = fake_quant_host(lib, p, bitdepth)
        assert int(c.max()) <= 2 ** bitdepth - 1


def test_optional_outputs_and_arguments(lib):
    p = np.linspace(-1, 1, 50).astype(np.float32)
    q0, _, _ = fake_quant_host(lib, p, 8)
    q1, c1, mm1 = fake_quant_host(lib, p, 8, codes=False, minmax=False)
    assert c1 is None and mm1 is None and np.array_equal(q0, q1)
    a = p.ctypes.data
    assert lib.linr_params_fake_quant_host(a, 50, 1, a, None, None) == -1
    assert lib.linr_params_fake_quant_host(a, 50, 17, a, None, None) == -1
    assert lib.linr_params_fake_quant_host(a, -1, 8, a, None, None) == -1
    assert lib.linr_params_fake_quant_host(None, 50, 8, a, None, None) == -1
    assert lib.linr_params_fake_quant_host(a, 50, 8, None, None, None) == -1
    assert lib.linr_params_fake_quant_host(None, 0, 8, None, None, None) == 0


def test_device_entry_checks_its_arguments_before_any_launch(lib):
    import ctypes
    buf = (ctypes.c_char * 4096)()
    a = (ctypes.addressof(buf) + 63) & ~63
    assert lib.linr_params_fake_quant(a, 64, 1, a + 1024, None, None, None) == -1
    assert lib.linr_params_fake_quant(a, 64, 17, a + 1024, None, None, None) == -1
    assert lib.linr_params_fake_quant(a, -1, 8, a + 1024, None, None, None) == -1
    assert lib.linr_params_fake_quant(None, 64, 8, a + 1024, None, None, None) == -1
    assert lib.linr_params_fake_quant(a, 64, 8, None, None, None, None) == -1
    assert lib.linr_params_fake_quant(a + 4, 64, 8, a + 1024, None, None, None) == -3
    assert lib.linr_params_fake_quant(a, 64, 8, a + 1028, None, None, None) == -3
    assert lib.linr_params_fake_quant(a, 64, 8, a + 1024, a + 2050, None, None) == -3
    assert lib.linr_params_fake_quant(None, 0, 8, None, None, None, None) == 0          # empty: nothing is launched


def test_first_quantisation_aware_epoch():
    from linr_pcgc_amd.overfit import qat_first_epoch
    assert qat_first_epoch(10, 0) == 10
    assert qat_first_epoch(10, 1) == 9 and qat_first_epoch(10, 2) == 8
    assert qat_first_epoch(10, 10) == 0 and qat_first_epoch(10, 25) == 0
    assert qat_first_epoch(0, 3) == 0
    with pytest.raises(ValueError):
        qat_first_epoch(10, -1)


def test_run_flag_is_parsed_and_rejected_for_the_wide_models():
    from linr_pcgc_amd import run
    assert run.parse([]).qat_epochs == 0
    assert run.parse(['--qat-epochs', '2']).qat_epochs == 2 and run.parse(['--qat_epochs', '3']).qat_epochs == 3
    assert run.parse(['--hidden-channel-conv', '16']).qat_epochs == 0
    for width in ('16', '32'):
        with pytest.raises(SystemExit):
            run.parse(['--qat-epochs', '1', '--hidden-channel-conv', width])
    with pytest.raises(SystemExit):
        run.parse(['--qat-epochs', '-1'])

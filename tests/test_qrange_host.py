"""CPU: the quantiser under GIVEN candidate ranges (linr_params_fake_quant_ranges_host, the plain-loop twin of the kernel behind the
encoder's range search) against a restatement in torch - clamp into (lo, hi), then model_codec.quant_uniform2's expression with lo and
hi in the place of the minimum and maximum - and the model codec's side of the feature: compress_params(qrange=), candidate_ranges,
laplace_bits_est.  Every comparison is exact: codes and counts as integers, reconstructions as bit patterns."""
import ctypes
import os

import numpy as np
import pytest
import torch

DEPTHS = (2, 8, 16)
NS = (1, 3, 4, 7, 4099, 54712)
KS = (1, 2, 16)
POISON_Q, POISON_C, POISON_S = 7.0, 77, -7


@pytest.fixture(scope='module')
def lib():
    from linr_pcgc_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.lib()


def ranges_host(lib, p, bitdepth, ranges, stride=None, codes=True, stats=True, expect=0):
    """The host twin on poisoned [K][stride] outputs: (rc checked) qparams, codes, stats as full arrays, padding included."""
    p = np.ascontiguousarray(p, dtype=np.float32)
    r = np.ascontiguousarray(np.asarray(ranges, dtype=np.float32).reshape(-1, 2))
    K, n = r.shape[0], p.size
    stride = (n + 3) & ~3 if stride is None else stride
    q = np.full((K, stride), POISON_Q, dtype=np.float32)
    c = np.full((K, stride), POISON_C, dtype=np.uint16) if codes else None
    st = np.full((K, 4), POISON_S, dtype=np.int64) if stats else None
    rc = lib.linr_params_fake_quant_ranges_host(p.ctypes.data, n, bitdepth, r.ctypes.data, K, stride, q.ctypes.data,
                                                None if c is None else c.ctypes.data, None if st is None else st.ctypes.data)
    assert rc == expect
    return q, c, st


def restated(p, bitdepth, lo, hi):
    """(codes, reconstruction, stats) of one candidate in torch fp32: clamp, then quant_uniform2's expression at the given lo / hi.
    hi == lo (quant_uniform2 yields NaN there): code 0 and the clamped parameter, as the C-ABI defines it."""
    t = torch.from_numpy(np.ascontiguousarray(p, dtype=np.float32))
    lo_t, hi_t = torch.tensor(lo, dtype=torch.float32), torch.tensor(hi, dtype=torch.float32)
    pc = torch.where(t < lo_t, lo_t, torch.where(t > hi_t, hi_t, t))
    sym_max = float(2 ** bitdepth - 1)
    rng = hi_t - lo_t
    if float(rng) == 0.0:
        level, recon = torch.zeros_like(pc), pc
    else:
        level = torch.round((pc - lo_t) / rng * sym_max)
        recon = level / sym_max * rng + lo_t
    codes = torch.nan_to_num(level, nan=0.0).clamp(0, sym_max).numpy().astype(np.int64)
    sum_q = int(codes.sum())
    mu = int(np.rint(np.float32(sum_q) / np.float32(codes.size)))
    stats = [int((t < lo_t).sum()), int((t > hi_t).sum()), sum_q, int(np.abs(codes - mu).sum())]
    return codes, recon.numpy(), stats


def outliers(n, seed, nan=False):
    """Weights of a trained model's size (normal, 0.05) with a few planted far outside at both ends."""
    rng = np.random.default_rng(seed)
    p = (rng.standard_normal(n) * 0.05).astype(np.float32)
    if n >= 4:
        p[n // 3], p[n // 2] = np.float32(7.5), np.float32(-3.25)
    if n >= 4099:
        p[5], p[n - 2] = np.float32(0.9), np.float32(-1.1)
    if nan and n >= 3:
        p[1] = np.nan
    return p


def some_ranges(p, K):
    """K candidate ranges for p: its own (min, max) first, then order statistics further in (repeated when p is short), for K == 16 the
    last one with lo == hi."""
    v = np.sort(p[~np.isnan(p)])
    out = [(float(v[min(t, (v.size - 1) // 2)]), float(v[max(v.size - 1 - t, v.size // 2)])) for t in [0, 1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 144, 233, 377, 610, 987][:K]]
    if K == 16:
        out[-1] = (float(v[v.size // 2]), float(v[v.size // 2]))
    return out


def assert_equals_restatement(lib, p, bitdepth, ranges, stride=None):
    q, c, st = ranges_host(lib, p, bitdepth, ranges, stride)
    n = p.size
    for k, (lo, hi) in enumerate(ranges):
        codes, recon, stats = restated(p, bitdepth, np.float32(lo), np.float32(hi))
        assert np.array_equal(c[k, :n].astype(np.int64), codes), (k, lo, hi)
        assert np.array_equal(q[k, :n].view(np.uint32), recon.view(np.uint32)), (k, lo, hi)
        assert st[k].tolist() == stats, (k, lo, hi)
        assert int(c[k, :n].max()) <= 2 ** bitdepth - 1
    assert np.all(q[:, n:] == POISON_Q) and np.all(c[:, n:] == POISON_C)           # the padding of a row is not written
    return q, c, st


@pytest.mark.parametrize('bitdepth', DEPTHS)
@pytest.mark.parametrize('n', NS)
@pytest.mark.parametrize('K', KS)
def test_host_twin_equals_the_torch_restatement(lib, n, K, bitdepth):
    p = outliers(n, 100 * n + K)
    assert_equals_restatement(lib, p, bitdepth, some_ranges(p, K))
    if n >= 3:
        pn = outliers(n, 100 * n + K + 1, nan=True)
        q, c, _ = assert_equals_restatement(lib, pn, bitdepth, some_ranges(pn, K), stride=((n + 3) & ~3) + 8)
        assert np.isnan(q[:, 1]).all() and not c[:, 1].any()                    # a NaN parameter stays NaN, code 0


@pytest.mark.parametrize('bitdepth', DEPTHS)
def test_all_equal_vector_and_empty_range(lib, bitdepth):
    p = np.full(1025, 0.25, dtype=np.float32)
    q, c, st = assert_equals_restatement(lib, p, bitdepth, [(0.25, 0.25), (0.0, 1.0), (0.5, 0.5)])
    assert np.array_equal(q[0, :1025], p) and not c[0, :1025].any() and st[0].tolist() == [0, 0, 0, 0]
    assert np.all(q[2, :1025] == 0.5) and not c[2, :1025].any() and st[2].tolist() == [1025, 0, 0, 0]     # all below lo: clamped, code 0


@pytest.mark.parametrize('bitdepth', DEPTHS)
@pytest.mark.parametrize('n', NS)
def test_true_range_candidate_is_the_plain_quantiser(lib, golden_dir, n, bitdepth):
    from test_fake_quant_host import fake_quant_host
    p = outliers(n, 7 * n + bitdepth, nan=n >= 7)
    if n == 54712:
        p = np.load(os.path.join(golden_dir, 'loot_model_kat.npz'))['flat'].astype(np.float32)
    q0, c0, mm = fake_quant_host(lib, p, bitdepth)
    q, c, st = ranges_host(lib, p, bitdepth, [(mm[0], mm[1]), (mm[0], mm[1])])
    for k in range(2):
        assert np.array_equal(q[k, :n].view(np.uint32), q0.view(np.uint32)) and np.array_equal(c[k, :n], c0)
    assert st[0, 0] == 0 and st[0, 1] == 0 and st[0, 2] == int(c0.astype(np.int64).sum())


def test_optional_outputs(lib):
    p = outliers(4099, 3)
    r = some_ranges(p, 2)
    q0, c0, st0 = ranges_host(lib, p, 8, r)
    q1, c1, st1 = ranges_host(lib, p, 8, r, codes=False, stats=False)
    assert c1 is None and st1 is None and np.array_equal(q0.view(np.uint32), q1.view(np.uint32))
    q2, c2, _ = ranges_host(lib, p, 8, r, stats=False)
    assert np.array_equal(c2, c0)


def _refused(call, good, bad_cases, buffers):
    before = [b.copy() for b in buffers]
    for change, code in bad_cases:
        args = dict(good)
        args.update(change)
        assert call(args) == code, change
        for b, b0 in zip(buffers, before):
            assert np.array_equal(b, b0), change                                # refused: nothing written


def test_every_refused_argument_returns_its_code_and_writes_nothing(lib):
    p = outliers(64, 1)
    r = np.array([[-0.1, 0.1], [-0.2, 0.3]], dtype=np.float32)
    q = np.full((2, 64), POISON_Q, dtype=np.float32)
    c = np.full((2, 64), POISON_C, dtype=np.uint16)
    st = np.full((2, 4), POISON_S, dtype=np.int64)
    rev = np.array([[-0.1, 0.1], [0.3, -0.2]], dtype=np.float32)
    nan_lo = np.array([[np.nan, 0.1], [-0.2, 0.3]], dtype=np.float32)
    nan_hi = np.array([[-0.1, 0.1], [-0.2, np.nan]], dtype=np.float32)
    good = dict(params=p.ctypes.data, n=64, bitdepth=8, ranges=r.ctypes.data, K=2, stride=64, q=q.ctypes.data, c=c.ctypes.data, st=st.ctypes.data)
    bad = [({'bitdepth': 1}, -1), ({'bitdepth': 17}, -1), ({'n': -1}, -1), ({'K': 0}, -1), ({'K': 17}, -1), ({'K': -3}, -1),
           ({'ranges': None}, -1), ({'ranges': rev.ctypes.data}, -1), ({'ranges': nan_lo.ctypes.data}, -1), ({'ranges': nan_hi.ctypes.data}, -1),
           ({'stride': 63}, -1), ({'stride': 60}, -1), ({'stride': 66}, -1), ({'n': 62, 'stride': 63}, -1),
           ({'params': None}, -1), ({'q': None}, -1)]

    def host(a):
        return lib.linr_params_fake_quant_ranges_host(a['params'], a['n'], a['bitdepth'], a['ranges'], a['K'], a['stride'], a['q'], a['c'], a['st'])
    _refused(host, good, bad, [q, c, st])
    assert host(dict(good, n=0, stride=0, params=None, q=None, c=None, st=None)) == 0          # empty: nothing to do
    assert host(dict(good, n=0)) == 0 and np.all(q == POISON_Q) and np.all(st == POISON_S)
    assert host(good) == 0 and not np.any(q == POISON_Q)

    # the device entry checks the same, and the alignment of what the kernel reads and writes 16 / 8 bytes at a time, before any launch
    buf = (ctypes.c_char * 8192)()
    a = (ctypes.addressof(buf) + 63) & ~63
    good = dict(params=a, n=64, bitdepth=8, ranges=r.ctypes.data, K=2, stride=64, q=a + 1024, c=a + 4096, st=a + 6144)
    bad = bad + [({'params': a + 4}, -3), ({'q': a + 1028}, -3), ({'c': a + 4098}, -3), ({'st': a + 6148}, -3)]

    def device(x):
        return lib.linr_params_fake_quant_ranges(x['params'], x['n'], x['bitdepth'], x['ranges'], x['K'], x['stride'], x['q'], x['c'], x['st'], None)
    for change, code in bad:
        assert device(dict(good, **change)) == code, change
    assert device(dict(good, n=0, stride=0, params=None, q=None, c=None, st=None)) == 0       # empty: nothing is launched


@pytest.mark.parametrize('bitdepth', (4, 8, 12))
def test_compress_params_with_a_range_round_trips_and_equals_the_host_twin(lib, golden_dir, bitdepth):
    from linr_pcgc_amd import model_codec
    flat = np.load(os.path.join(golden_dir, 'loot_model_kat.npz'))['flat'].astype(np.float32)
    flat[100], flat[40000] = np.float32(3.0), np.float32(-2.0)
    trims, ranges = model_codec.candidate_ranges(torch.from_numpy(flat))
    for lo, hi in (ranges[0], ranges[1], ranges[-1]):
        out = model_codec.compress_params(torch.from_numpy(flat), bitdepth, qrange=(lo, hi))
        assert out['min_param'] == lo and out['max_param'] == hi
        back, sym = model_codec.decompress_params(out, flat.size, with_symbols=True)
        assert np.array_equal(back.numpy().view(np.uint32), out['recon_ret'].numpy().view(np.uint32))
        q, c, st = ranges_host(lib, flat, bitdepth, [(lo, hi)])
        assert np.array_equal(q[0, :flat.size].view(np.uint32), out['recon_ret'].numpy().view(np.uint32))
        assert np.array_equal(c[0, :flat.size], np.asarray(sym).astype(np.uint16)) and np.array_equal(c[0, :flat.size], out['symbols'].astype(np.uint16))
        # the stats are what the codec's Laplace model is made of
        assert int(np.rint(np.float32(st[0, 2]) / np.float32(flat.size))) == int(out['mu'])
        assert float(np.rint(np.float32(st[0, 3]) / np.float32(flat.size))) == out['b']
    codes, recon = model_codec.quant_uniform2(torch.from_numpy(flat), 8, qrange=ranges[1])
    assert int(codes.min()) == 0 and int(codes.max()) == 255 and float(recon.min()) == ranges[1][0] and float(recon.max()) == ranges[1][1]
    with pytest.raises(ValueError):
        model_codec.quant_uniform2(torch.from_numpy(flat), 8, qrange=(1.0, -1.0))


def test_no_range_gives_todays_dictionary(golden_dir):
    from linr_pcgc_amd import model_codec
    flat = torch.from_numpy(np.load(os.path.join(golden_dir, 'loot_model_kat.npz'))['flat'].astype(np.float32))

    def today(params, bitdepth):
        """compress_params' quantiser front as it stood before the option (the rest of the dictionary follows from these)."""
        mn, mx = params.min(), params.max()
        sym_max = float(np.ceil(2 ** bitdepth) - 1)
        new_p = torch.round((params - mn) / (mx - mn) * sym_max)
        return new_p, new_p / sym_max * (mx - mn) + mn, float(mn), float(mx)

    for bitdepth in (8, 12):
        a, b = model_codec.compress_params(flat, bitdepth), model_codec.compress_params(flat, bitdepth, None)
        true = model_codec.compress_params(flat, bitdepth, qrange=(float(flat.min()), float(flat.max())))
        codes, recon, mn, mx = today(flat, bitdepth)
        assert list(a) == ['bpp_real', 'bit_real', 'side_info_bit', 'bitdepth', 'enc_mode', 'laplace_real_bpp', 'zlib_bpp', 'min_param',
                           'max_param', 'mu', 'b', 'final_bytes', 'recon_ret', 'symbols']
        assert a['min_param'] == mn and a['max_param'] == mx
        assert np.array_equal(a['recon_ret'].numpy().view(np.uint32), recon.numpy().view(np.uint32))
        assert np.array_equal(a['symbols'].astype(np.float32), codes.numpy())
        for other in (b, true):                                  # ... and the vector's own range, given explicitly, is the same model
            assert list(other) == list(a)
            for key in a:
                if key in ('recon_ret', 'symbols'):
                    assert np.array_equal(np.asarray(a[key]), np.asarray(other[key]))
                else:
                    assert a[key] == other[key], key
    q0, r0 = model_codec.quant_uniform2(flat, 8)
    q1, r1 = model_codec.Model_Estimate.quant_uniform2(flat, 8, None)
    assert torch.equal(q0, q1) and torch.equal(r0, r1)


def test_candidate_ranges_are_exact_order_statistics():
    from linr_pcgc_amd import model_codec
    rng = np.random.default_rng(5)
    flat = (rng.standard_normal(54712) * 0.05).astype(np.float32)
    v = np.sort(flat)
    trims, ranges = model_codec.candidate_ranges(torch.from_numpy(flat))
    assert tuple(trims) == model_codec.DEFAULT_QRANGE_TRIMS == (0, 1, 2, 4, 8, 16, 32, 64)
    assert ranges == [(float(v[t]), float(v[-1 - t])) for t in trims]
    assert ranges[0] == (float(flat.min()), float(flat.max()))
    # t = 0 stays first whatever is asked for, in whatever order
    trims, ranges = model_codec.candidate_ranges(torch.from_numpy(flat), (8, 3))
    assert trims == [0, 3, 8] and ranges == [(float(v[t]), float(v[-1 - t])) for t in (0, 3, 8)]
    assert model_codec.candidate_ranges(torch.from_numpy(flat), (0,)) == ([0], [(float(v[0]), float(v[-1]))])
    # duplicates collapse: equal parameters at both ends make neighbouring trims the same range
    dup = flat.copy()
    dup[:3], dup[3:6] = v[-1] + np.float32(1.0), v[0] - np.float32(1.0)
    trims, ranges = model_codec.candidate_ranges(torch.from_numpy(dup), (0, 1, 2, 3, 4))
    s = np.sort(dup)
    assert trims == [0, 3, 4] and ranges == [(float(s[t]), float(s[-1 - t])) for t in (0, 3, 4)]
    # a trim that would leave nothing is dropped; negative trims and more than 16 candidates are refused
    assert model_codec.candidate_ranges(torch.tensor([1.0, 2.0, 3.0]), (0, 1, 2, 64)) == ([0, 1], [(1.0, 3.0), (2.0, 2.0)])
    with pytest.raises(ValueError):
        model_codec.candidate_ranges(torch.from_numpy(flat), (0, -1))
    with pytest.raises(ValueError):
        model_codec.candidate_ranges(torch.from_numpy(flat), range(17))


def test_laplace_estimate_from_the_stats_is_the_codecs_estimate(lib, golden_dir):
    """laplace_bits_est from (n, sum |q - mu|) against compress_params' own float32 sum over the codes."""
    from linr_pcgc_amd import model_codec
    flat = np.load(os.path.join(golden_dir, 'loot_model_kat.npz'))['flat'].astype(np.float32)
    codes, _ = model_codec.quant_uniform2(torch.from_numpy(flat), 8)
    mu = torch.round(codes.mean())
    b = torch.round((codes - mu).abs().mean())
    want = float(-torch.sum(torch.log2(torch.exp(-torch.abs(codes - mu) / b) / (2 * b)))) + 2 * 8 + 2 + 2 * 32
    _, _, st = ranges_host(lib, flat, 8, [(float(flat.min()), float(flat.max()))])
    got = model_codec.laplace_bits_est(flat.size, int(st[0, 3]), 8)
    assert abs(got - want) <= 1e-4 * want                        # (the codec sums 54,712 float32 terms)
    assert model_codec.laplace_bits_est(1000, 0, 8) == 8 * 1000 + 66          # b == 0: no Laplace figure, the raw bound
    assert model_codec.laplace_bits_est(1000, 1000 * 120, 8) == 8 * 1000 + 66   # ... and where the figure passes it


def test_evaluated_frames_are_evenly_spaced():
    from linr_pcgc_amd import codec
    assert codec.qrange_eval_frames(32, 4) == [4, 12, 20, 28]
    assert codec.qrange_eval_frames(32, 0) == list(range(32)) == codec.qrange_eval_frames(32, 32) == codec.qrange_eval_frames(32, 99)
    assert codec.qrange_eval_frames(2, 4) == [0, 1] and codec.qrange_eval_frames(5, 1) == [2] and codec.qrange_eval_frames(3, 2) == [0, 2]


def test_run_flags_are_parsed():
    from linr_pcgc_amd import run
    a = run.parse([])
    assert a.qrange_search is False and a.qrange_trims is None and a.qrange_frames == 4
    a = run.parse(['--qrange-search', '--qrange-trims', '0,1,4', '--qrange-frames', '0'])
    assert a.qrange_search is True and a.qrange_trims == (0, 1, 4) and a.qrange_frames == 0
    assert run.parse(['--qrange_search', '--qrange_trims', '2']).qrange_trims == (2,)
    for bad in (['--qrange-trims', '1,x'], ['--qrange-trims', '-1'], ['--qrange-frames', '-2']):
        with pytest.raises(SystemExit):
            run.parse(bad)

"""CPU: the range coder fed with 16-bit code values and symbol bit planes (linr_ac_encode_binary_codes, _decode_binary_codes,
_encode_binary_codes_batch) against the same coder fed with fp32 probabilities and byte symbols (linr_ac_encode_binary, itself
checked against the oracle in tests/test_cpu_host.py).  The two forms share one loop body, so with code values computed by the
documented formula the streams must be the same bytes: every comparison here is exact."""
import ctypes
import os

import numpy as np
import pytest

NS = (0, 1, 31, 32, 33, 255, 256, 257, 5000)
REGIMES = ('uniform', 'peaked', 'exact')


@pytest.fixture(scope='module')
def lib():
    from linr_pcgc_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.lib()


def code_values(p):
    """binary_c1 of csrc/ac.cpp in numpy float32: two fp32 roundings, round half to even, + 1, 16-bit wrap."""
    p = np.asarray(p, dtype=np.float32)
    return (((np.rint((np.float32(1) - p) * np.float32(65534)).astype(np.int64) + 1) & 0xFFFF)).astype(np.uint16)


def pack_symbols(s):
    """Bit i & 31 of word i >> 5 = symbol i; the unused high bits of the last word are zero."""
    bits = np.zeros(((len(s) + 31) // 32) * 32, dtype=np.uint8)
    bits[:len(s)] = np.asarray(s) != 0
    return np.packbits(bits, bitorder='little').view('<u4').astype(np.uint32)


def draw(regime, n, seed):
    rng = np.random.default_rng(seed)
    if regime == 'uniform':
        p = rng.random(n).astype(np.float32)
        s = (rng.random(n) < p).astype(np.uint8)
    elif regime == 'peaked':
        # all but certain symbols, coded as predicted: thousands of symbols between two renormalisations
        s = (rng.random(n) < 0.5).astype(np.uint8)
        p = np.where(s == 1, np.float32(1 - 1e-4), np.float32(1e-4)).astype(np.float32)
        flip = rng.random(n) < 0.01                         # and now and then the symbol the model all but excluded: 13 bits at once
        s = np.where(flip, 1 - s, s).astype(np.uint8)
    else:
        p = rng.choice(np.array([0.0, 1.0, 0.5], dtype=np.float32), n)
        s = np.where(p == 0.5, rng.random(n) < 0.5, p == 1.0).astype(np.uint8)          # 0.0 / 1.0: only the possible symbol
        if n > 3:
            s[:3], p[:3] = [1, 0, 1], [0.0, 1.0, 0.5]       # ... except these: a symbol of code width 1 / 65535
    return p, s


def enc_probs(lib, p, s, cap=None):
    out = np.empty(2 * len(p) + 64 if cap is None else cap, dtype=np.uint8)
    r = lib.linr_ac_encode_binary(p.ctypes.data, s.ctypes.data, len(p), out.ctypes.data, out.size)
    return r, out[:max(r, 0)].tobytes()


def enc_codes(lib, c1, w, n, cap=None):
    out = np.empty(2 * n + 64 if cap is None else cap, dtype=np.uint8)
    r = lib.linr_ac_encode_binary_codes(c1.ctypes.data, w.ctypes.data, n, out.ctypes.data, out.size)
    return r, out[:max(r, 0)].tobytes()


def test_numpy_helpers():
    assert code_values([0.0, 1.0, 0.5, 0.25]).tolist() == [65535, 1, 32768, 49151]
    assert pack_symbols([1, 0, 1]).tolist() == [5] and pack_symbols([0] * 32 + [1]).tolist() == [0, 1] and pack_symbols([]).size == 0


@pytest.mark.parametrize('regime', REGIMES)
@pytest.mark.parametrize('n', NS)
def test_codes_encoder_gives_the_bytes_of_the_probability_encoder_and_decodes(lib, n, regime):
    p, s = draw(regime, n, 1000 * REGIMES.index(regime) + n)
    c1, w = code_values(p), pack_symbols(s)
    r0, ref = enc_probs(lib, p, s)
    r1, got = enc_codes(lib, c1, w, n)
    assert r0 >= 1 and r1 == r0 and got == ref
    back = np.full(n, 7, dtype=np.uint8)
    stream = np.frombuffer(got, dtype=np.uint8)
    assert lib.linr_ac_decode_binary_codes(c1.ctypes.data, n, stream.ctypes.data, stream.size, back.ctypes.data) == 0
    assert np.array_equal(back, s)
    back2 = np.full(n, 7, dtype=np.uint8)
    assert lib.linr_ac_decode_binary(p.ctypes.data, n, stream.ctypes.data, stream.size, back2.ctypes.data) == 0
    assert np.array_equal(back2, s)


def straddling_sequence(pairs):
    """Code values and symbols that keep the coder's interval astride the middle, found by following its state (the interval update
    and renormalisation of csrc/ac.cpp in plain integers): symbol 1 with the largest code value that leaves the middle inside lifts
    the lower end to just below it, symbol 0 at a quarter then cuts the upper end to within the middle half: two more pending bits per
    pair, none resolved.  Returns (c1, symbols, pending bits collected)."""
    low, high, pend, c1s, syms = 0, 0xFFFFFFFF, 0, [], []
    for _ in range(pairs):
        for sym in (1, 0):
            span = high - low + 1
            c1 = max(1, (((1 << 31) - low) << 16) // span - 1) if sym else 16384
            t = (span * c1) >> 16
            if sym:
                low += t
            else:
                high = low + t - 1
            c1s.append(c1)
            syms.append(sym)
            while True:
                if high < 1 << 31 or low >= 1 << 31:
                    raise AssertionError('the interval left the middle')
                if low >= 1 << 30 and high < 3 << 30:
                    pend += 1
                    low, high = (low << 1) & 0x7FFFFFFF, ((high << 1) | 0x80000001) & 0xFFFFFFFF
                else:
                    break
    return np.array(c1s, dtype=np.uint16), np.array(syms, dtype=np.uint8), pend


def test_pending_runs_longer_than_a_word(lib):
    """Pending bits are written as a run of equal bits once a symbol decides them, 32 to a put_run word.  The peaked regime above
    does not collect many (its intervals are narrow but land anywhere; a straddle of m steps needs the middle within 2^-m of them),
    so this sequence is built to: 40 pairs of symbols that keep the interval astride the middle, then ordinary symbols that resolve
    the run.  Both forms of the coder must write the same bytes, with the run in them."""
    c1, s, pend = straddling_sequence(40)
    assert pend > 64
    p = (np.float32(1) - (c1.astype(np.float64) - 1) / 65534).astype(np.float32)
    assert np.array_equal(code_values(p), c1)
    rng = np.random.default_rng(12)
    tail_p = rng.random(60).astype(np.float32)
    p, s = np.concatenate([p, tail_p]), np.concatenate([s, (rng.random(60) < tail_p).astype(np.uint8)])
    c1, w = code_values(p), pack_symbols(s)
    r0, ref = enc_probs(lib, p, s)
    r1, got = enc_codes(lib, c1, w, len(p))
    assert r1 == r0 and got == ref
    assert b'\x00' * (pend // 8 - 1) in ref or b'\xff' * (pend // 8 - 1) in ref          # the whole bytes of a run of `pend` equal bits
    back = np.empty(len(p), dtype=np.uint8)
    stream = np.frombuffer(got, dtype=np.uint8)
    assert lib.linr_ac_decode_binary_codes(c1.ctypes.data, len(p), stream.ctypes.data, stream.size, back.ctypes.data) == 0
    assert np.array_equal(back, s)


def test_symbol_bits_beyond_n_are_not_read_as_symbols(lib):
    p, s = draw('uniform', 33, 5)
    c1, w = code_values(p), pack_symbols(s)
    dirty = w.copy()
    dirty[-1] |= np.uint32(0xFFFFFFFE)                      # bits 33..63
    assert enc_codes(lib, c1, dirty, 33)[1] == enc_probs(lib, p, s)[1]


@pytest.mark.parametrize('threads', [1, 4])
def test_codes_batch_equals_single(lib, threads):
    from linr_pcgc_amd.model_core import encode_streams, encode_streams_codes
    ps, ss = zip(*[draw(REGIMES[i % 3], n, 77 + i) for i, n in enumerate(NS)])
    assert len(ps) == 9
    c1s, ws = [code_values(p) for p in ps], [pack_symbols(s) for s in ss]
    single = [enc_codes(lib, c, w, len(c))[1] for c, w in zip(c1s, ws)]
    got = encode_streams_codes(c1s, ws, [len(c) for c in c1s], n_threads=threads)
    assert got == single
    assert got == encode_streams(list(ps), list(ss), n_threads=threads)


def test_codes_batch_reports_a_failed_stream(lib):
    ps, ss = zip(*[draw('uniform', n, n) for n in (100, 200)])
    c1s, ws = [code_values(p) for p in ps], [pack_symbols(s) for s in ss]
    outs = [np.empty(400, dtype=np.uint8), np.empty(3, dtype=np.uint8)]
    arr = lambda xs: (ctypes.c_void_p * 2)(*[x.ctypes.data for x in xs])
    n, cap, got = (ctypes.c_int64 * 2)(100, 200), (ctypes.c_int64 * 2)(400, 3), (ctypes.c_int64 * 2)()
    assert lib.linr_ac_encode_binary_codes_batch(arr(c1s), arr(ws), n, 2, arr(outs), cap, got, 2) == -2
    assert got[0] == len(enc_codes(lib, c1s[0], ws[0], 100)[1]) and got[1] == -2
    assert lib.linr_ac_encode_binary_codes_batch(None, arr(ws), n, 2, arr(outs), cap, got, 2) == -1
    assert lib.linr_ac_encode_binary_codes_batch(arr(c1s), arr(ws), n, -1, arr(outs), cap, got, 2) == -1
    assert lib.linr_ac_encode_binary_codes_batch(None, None, None, 0, None, None, None, 2) == 0


def test_small_cap_is_enospc_and_bad_arguments_are_einval(lib):
    p, s = draw('uniform', 257, 3)
    c1, w = code_values(p), pack_symbols(s)
    r, ref = enc_codes(lib, c1, w, 257)
    assert r > 8
    assert enc_codes(lib, c1, w, 257, cap=r)[0] == r
    for cap in (r - 1, 1, 0):
        assert enc_codes(lib, c1, w, 257, cap=cap)[0] == -2 == enc_probs(lib, p, s, cap=cap)[0]
    out = np.empty(64, dtype=np.uint8)
    o, c, y = out.ctypes.data, c1.ctypes.data, w.ctypes.data
    assert lib.linr_ac_encode_binary_codes(None, y, 4, o, 64) == -1
    assert lib.linr_ac_encode_binary_codes(c, None, 4, o, 64) == -1
    assert lib.linr_ac_encode_binary_codes(c, y, -1, o, 64) == -1
    assert lib.linr_ac_encode_binary_codes(c, y, 4, o, -1) == -1
    assert lib.linr_ac_encode_binary_codes(c, y, 4, None, 64) == -1
    assert lib.linr_ac_encode_binary_codes(None, None, 0, o, 64) == 1 == lib.linr_ac_encode_binary(None, None, 0, o, 64)
    assert lib.linr_ac_decode_binary_codes(None, 4, o, 8, o) == -1
    assert lib.linr_ac_decode_binary_codes(c, 4, o, 8, None) == -1
    assert lib.linr_ac_decode_binary_codes(c, -1, o, 8, o) == -1
    assert lib.linr_ac_decode_binary_codes(c, 4, None, 8, o) == -1
    assert lib.linr_ac_decode_binary_codes(c, 4, o, -1, o) == -1
    assert lib.linr_ac_decode_binary_codes(None, 0, None, 0, None) == 0


def test_device_entry_checks_its_arguments_before_any_launch(lib):
    """linr_ac_codes (csrc/ac_codes.hip) refuses bad arguments before it touches the device, so this runs without a GPU."""
    buf = (ctypes.c_char * 4096)()
    p = (ctypes.addressof(buf) + 63) & ~63
    assert [lib.linr_ac_codes_sym_words(n) for n in (-1, 0, 1, 32, 33, 64, 65)] == [0, 0, 1, 1, 2, 2, 3]
    assert lib.linr_ac_codes(None, 40, p, 8, 40, p, 40, p, 2, None) == -1
    assert lib.linr_ac_codes(p, 40, None, 8, 40, p, 40, p, 2, None) == -1
    assert lib.linr_ac_codes(p, 40, p, 8, 40, None, 40, p, 2, None) == -1
    assert lib.linr_ac_codes(p, 40, p, 8, 40, p, 40, None, 2, None) == -1
    assert lib.linr_ac_codes(p, 40, p, 8, -1, p, 40, p, 2, None) == -1          # n < 0
    assert lib.linr_ac_codes(p, 39, p, 8, 40, p, 40, p, 2, None) == -1          # probs_ld < n
    assert lib.linr_ac_codes(p, 40, p, 8, 40, p, 39, p, 2, None) == -1          # c1_ld < n
    assert lib.linr_ac_codes(p, 40, p, 8, 40, p, 40, p, 1, None) == -1          # sym_ld < words
    assert lib.linr_ac_codes(p, 40, p, 7, 40, p, 40, p, 2, None) == -1          # occ_ld < 8
    bound = (1 << 27) - 1                                                       # the shared 32-bit row bound (csrc/common.h)
    assert lib.linr_ac_codes(p, bound, p, 8, bound, p, bound, p, bound, None) == -1
    assert lib.linr_ac_codes(p, 0, p, 8, 0, p, 0, p, 0, None) == 0              # empty input is fine, nothing is launched
    assert lib.linr_ac_codes(None, 0, p, 8, 0, p, 0, p, 0, None) == -1


def test_run_flag_is_parsed_and_off_by_default():
    from linr_pcgc_amd import run
    assert run.parse([]).device_codes is False and run.parse(['--device-codes']).device_codes is True

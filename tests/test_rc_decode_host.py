"""CPU: the device range decoder's body (csrc/rc_dec_body.h), which rc_decode_k runs a wave per entry, run for one stream on the host
(linr_ac_decode_binary_twin: 64-symbol chunks, 64-word windows, as the wave walks them) against the library's host decoder
(linr_ac_decode_binary), which shares no text with it: on streams the host encoder wrote and on bytes that are no streams at all.  The
table checks of linr_rc_decode_probs that need no GPU, the drivers' flags, and the body with the kernel's aligned-window access under
AddressSanitizer + UBSan (tools/rc_decode_emul.cpp, a stand-alone program).  Symbols and return codes, all exact."""
import ctypes
import os

import numpy as np
import pytest

from test_device_coder_host import REGIMES, draw, greedy_prefix, pack_symbols      # noqa: E402,F401

# each side of the 32-symbol word and the 64-symbol chunk; 4097 and 20000: several 256-byte windows
NS = (0, 1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 4097, 20000)
GARBAGE_LENGTHS = (0, 1, 3, 4, 5, 255, 256, 257, 1000)
GARBAGE_SYMBOLS = 3000


@pytest.fixture(scope='module')
def lib():
    from linr_pcgc_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.lib()


def c1_of(p):
    """binary_c1 of csrc/ac.cpp in numpy: two float32 roundings, round half to even, + 1, & 0xFFFF."""
    p = np.asarray(p, dtype=np.float32)
    return ((np.rint((np.float32(1) - p) * np.float32(65534)).astype(np.int64) + 1) & 0xFFFF).astype(np.uint16)


def p_for_c1(c1):
    """A finite float32 p in [0, 1] for every code value c1 in 1..65535, checked: c1_of(p) == c1."""
    c1 = np.asarray(c1, dtype=np.int64)
    p = (1.0 - (c1 - 1) / 65534.0).astype(np.float32)
    for _ in range(4):                                   # a neighbouring float where the two roundings land beside the target
        got = c1_of(p).astype(np.int64)
        if (got == c1).all():
            break
        p = np.where(got > c1, np.nextafter(p, np.float32(2)), np.where(got < c1, np.nextafter(p, np.float32(-1)), p)).astype(np.float32)
    assert (c1_of(p) == c1).all() and (p >= 0).all() and (p <= 1).all()
    return np.ascontiguousarray(p)


def encode(lib, p, s):
    n = len(p)
    p = np.ascontiguousarray(p, dtype=np.float32)
    s = np.ascontiguousarray(s, dtype=np.uint8)
    out = np.zeros(2 * n + 64, dtype=np.uint8)
    r = lib.linr_ac_encode_binary(p.ctypes.data if n else None, s.ctypes.data if n else None, n, out.ctypes.data, out.size)
    assert r >= 1
    return out[:r].tobytes()


def decode(fn, p, data):
    """n = len(p) symbols from an exact-size copy of `data` through entry fn; the bytes behind the symbols stay as they were."""
    n = len(p)
    p = np.ascontiguousarray(p, dtype=np.float32)
    buf = np.frombuffer(bytes(data), dtype=np.uint8).copy()
    sym = np.full(n + 16, 0xA5, dtype=np.uint8)
    assert fn(p.ctypes.data if n else None, n, buf.ctypes.data if buf.size else None, buf.size, sym.ctypes.data) == 0
    assert (sym[n:] == 0xA5).all()
    return sym[:n]


def both(lib, p, data, what):
    want = decode(lib.linr_ac_decode_binary, p, data)
    got = decode(lib.linr_ac_decode_binary_twin, p, data)
    assert np.array_equal(got, want), (what, int(np.argmax(got != want)))
    return want


@pytest.mark.parametrize('regime', REGIMES)
def test_twin_decodes_the_host_encoders_streams(lib, regime):
    tails = set()
    for n in NS:
        c1, s = draw(regime, n, 3000 * REGIMES.index(regime) + n % 991)
        p = p_for_c1(c1)
        data = encode(lib, p, s)
        tails.add(len(data) % 4)
        assert np.array_equal(both(lib, p, data, (regime, n)), s)
        if regime == 'loud' and n >= 4097:
            assert len(data) > 3 * 256                    # several 256-byte windows
    if regime == 'uniform':
        assert len(tails) >= 3                            # (all four over the regimes: test_all_tails_occur)


def test_all_tails_occur(lib):
    tails = set()
    for regime in REGIMES:
        for n in NS:
            c1, s = draw(regime, n, 3000 * REGIMES.index(regime) + n % 991)
            tails.add(len(encode(lib, p_for_c1(c1), s)) % 4)
    assert tails == {0, 1, 2, 3}


def test_the_ends_of_the_probability_range_and_the_half_way_values(lib):
    """p exactly 0 and 1, and p whose (1 - p) * 65534 lies half-way between two integers (c1 by round-half-to-even)."""
    rng = np.random.default_rng(5)
    k = rng.integers(0, 65534, 3000)
    half = (np.float32(1) - ((k + 0.5) / 65534.0).astype(np.float32)).astype(np.float32)
    p = np.concatenate([np.zeros(50, np.float32), np.ones(50, np.float32), half, rng.random(900).astype(np.float32)])
    rng.shuffle(p)
    assert ((p >= 0) & (p <= 1)).all()
    s = (rng.random(p.size) < p).astype(np.uint8)
    assert np.array_equal(both(lib, p, encode(lib, p, s), 'edges'), s)


@pytest.mark.parametrize('steps', [16, 40])
def test_long_straddle_runs(lib, steps):
    c1s, syms, pending = greedy_prefix(steps)
    assert pending >= 96, 'the generator: a straddle run longer than the bit window'
    rng = np.random.default_rng(steps)
    for sym in (0, 1):                                    # a near-certain symbol at either end resolves the run with bit 0 / bit 1
        c1 = c1s + [65535 if sym else 1] + rng.integers(1, 65536, 70).tolist()
        s = np.asarray(syms + [sym] + rng.integers(0, 2, 70).tolist(), dtype=np.uint8)
        p = p_for_c1(c1)
        assert np.array_equal(both(lib, p, encode(lib, p, s), ('resolved by', sym)), s)
    p = p_for_c1(c1s)
    s = np.asarray(syms, dtype=np.uint8)
    assert np.array_equal(both(lib, p, encode(lib, p, s), 'end of stream'), s)


def garbage_cases():
    """[(p, bytes)]: random strings that are no streams, n = 3000; valid streams cut at every length up to 16 bytes."""
    rng = np.random.default_rng(99)
    out = []
    for m in GARBAGE_LENGTHS:
        out.append((rng.random(GARBAGE_SYMBOLS).astype(np.float32), rng.integers(0, 256, m).astype(np.uint8).tobytes()))
    return out


def test_any_bytes_decode_alike(lib):
    for p, data in garbage_cases():
        both(lib, p, data, ('garbage', len(data)))
    for regime in REGIMES:
        c1, s = draw(regime, 300, 41)
        p = p_for_c1(c1)
        data = encode(lib, p, s)
        for cut in range(0, min(16, len(data)) + 1):
            both(lib, p, data[:cut], (regime, 'cut at', cut))


def test_twin_checks_its_arguments(lib):
    assert lib.linr_ac_decode_binary_twin(None, -1, None, 0, None) == -1
    assert lib.linr_ac_decode_binary_twin(None, 1, None, 0, None) == -1
    assert lib.linr_ac_decode_binary_twin(None, 0, None, 1, None) == -1
    assert lib.linr_ac_decode_binary_twin(None, 0, None, 0, None) == 0


def test_device_entry_checks_its_table_before_any_launch(lib):
    """The checks of linr_rc_decode_probs that need no GPU: they come before the first launch, so a bad table is refused without one."""
    from linr_pcgc_amd import _lib
    assert lib.linr_rc_decode_ws_bytes(-1) == 0 and lib.linr_rc_decode_ws_bytes(8) >= 8 * 40
    P = 0x1000                                            # never dereferenced: every call below fails its checks

    def call(rows, n_probs=100, bytes_len=64, n_rows=100, n=None, ws_bytes=1 << 16, occ_ld=8):
        tab = (_lib.LinrRcDecEntry * max(1, len(rows)))(*[_lib.LinrRcDecEntry(*r) for r in rows])
        return lib.linr_rc_decode_probs(P, n_probs, P, bytes_len, ctypes.addressof(tab), len(rows) if n is None else n, P, occ_ld, n_rows,
                                        None, P, ws_bytes, None)
    good = [(0, 10, 0, 7, 0), (10, 10, 7, 9, 10)]         # {p_off, n, in_off, in_len, out_row}
    assert call(good, n=-1) == -1
    for field in range(5):                                # a negative field
        row = list(good[1])
        row[field] = -1
        assert call([good[0], tuple(row)]) == -1, field
    assert call(good, n_probs=19) == -1                   # p_off + n > n_probs
    assert call(good, bytes_len=15) == -1                 # in_off + in_len > bytes_len
    assert call(good, n_rows=19) == -1                    # out_row + n > n_rows
    assert call([(0, 10, 0, 7, 0), (10, 10, 7, 9, 9)]) == -1              # overlapping row ranges
    assert call([(10, 10, 7, 9, 5), (0, 10, 0, 7, 0)]) == -1              # ... in any order
    assert call([(0, 1 << 62, 0, 7, 1 << 62)], n_probs=1 << 62, n_rows=1 << 62) == -1          # out_row + n overflows nothing
    assert call(good, occ_ld=0) == -1
    assert call(good, ws_bytes=lib.linr_rc_decode_ws_bytes(2) - 1) == -1
    assert lib.linr_rc_decode_probs(None, 0, None, 0, None, 0, None, 8, 0, None, None, 0, None) == 0


def test_flags_are_parsed_and_off_by_default():
    from linr_pcgc_amd import decoder, run
    base = ['--input-glob', 'x*.npy', '--out', 'o']
    assert run.parse(base).device_decoder is False
    assert run.parse(base + ['--decode', '--device-decoder']).device_decoder is True
    assert run.parse(base + ['--decode', '--pipeline', '--decode-lockstep', '4', '--device_decoder']).device_decoder is True
    with pytest.raises(SystemExit):
        run.parse(base + ['--decode', '--device-decoder', '--hidden-channel-conv', '16'])
    dec = ['--enc-dir', 'e', '--dec-dir', 'd']
    assert decoder.parser().parse_args(dec).device_decoder is False
    a = decoder.parser().parse_args(dec + ['--device-decoder', '--lockstep', '3'])
    assert a.device_decoder is True and a.lockstep == 3


def test_body_with_the_kernels_window_access_under_sanitizers(tmp_path):
    """tools/rc_decode_emul.cpp: the body with an In that reads aligned 64-word windows as the wave does, entries back to back at byte
    offsets 0..7 among non-zero neighbours in exact-size heap buffers, each against the host decoder on its bytes alone - under
    AddressSanitizer + UBSan.  Host code only, a program of its own."""
    import shutil
    import subprocess
    if shutil.which('g++') is None:
        pytest.skip('no g++')
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / 'rc_decode_emul')
    build = subprocess.run(['g++', '-O1', '-g', '-std=c++17', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined',
                            '-fno-omit-frame-pointer', '-o', exe, os.path.join(root, 'tools', 'rc_decode_emul.cpp'),
                            os.path.join(root, 'linr_pcgc_amd', 'csrc', 'ac.cpp'), '-lpthread'], capture_output=True, text=True, timeout=600)
    if build.returncode != 0 and 'asan' in (build.stderr or '').lower():
        pytest.skip('sanitizer runtime not installed')
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([exe, '40'], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0 and 'all as expected' in run.stdout, (run.stdout[-500:], run.stderr[-3000:])
    assert 'ERROR' not in run.stderr and 'runtime error' not in run.stderr

"""CPU: the range encoder's one body (csrc/rc_body.h), which the device coder runs a wave per stream, run for one stream on the host
(linr_ac_encode_binary_codes: a 64-word array stands in for the lanes' staging registers) against the library's bit-at-a-time coder
(linr_ac_encode_cdf16 on the rows [0, c1, 0], lp = 3, unshared), which shares no code with it; tests/test_cpu_host.py pins the body
to the oracle's coder.  Bytes and lengths, all exact."""
import os

import numpy as np
import pytest

# each side of the 32-symbol word, the 64-symbol chunk and 256 (the host decoder's AC_CHUNK); one long stream
NS = (0, 1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1000, 70001)
REGIMES = ('uniform', 'quiet', 'loud', 'half')


@pytest.fixture(scope='module')
def lib():
    from linr_pcgc_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.lib()


def pack_symbols(s):
    """Bit i & 31 of word i >> 5 = symbol i; the unused high bits of the last word are zero."""
    bits = np.zeros(((len(s) + 31) // 32) * 32, dtype=np.uint8)
    bits[:len(s)] = np.asarray(s) != 0
    return np.packbits(bits, bitorder='little').view('<u4').astype(np.uint32)


def draw(regime, n, seed):
    """(c1 uint16 [n], symbols uint8 [n]) of one stream."""
    rng = np.random.default_rng(seed)
    if regime == 'uniform':
        return rng.integers(1, 65536, n).astype(np.uint16), rng.integers(0, 2, n).astype(np.uint8)
    if regime == 'quiet':            # symbol 1 owns all but c1 / 65536 of the interval: long stretches with no output
        return rng.integers(1, 4, n).astype(np.uint16), (rng.random(n) >= 0.001).astype(np.uint8)
    if regime == 'loud':             # symbol 0 almost always: ~16 bits per symbol, the output crosses the 64-word staging block often
        return rng.integers(1, 4, n).astype(np.uint16), (rng.random(n) < 0.001).astype(np.uint8)
    return np.full(n, 32768, dtype=np.uint16), (np.arange(n) & 1).astype(np.uint8)


GUARD = 32


def encode(fn, c1, s, cap=None):
    """One stream through entry fn: (return value, the bytes it reports) - and the guard bytes behind cap are as they were."""
    n = len(c1)
    c1 = np.ascontiguousarray(c1, dtype=np.uint16)
    w = pack_symbols(s)
    cap = 2 * n + 64 if cap is None else cap
    out = np.full(cap + GUARD, 0xA5, dtype=np.uint8)
    r = fn(c1.ctypes.data if n else None, w.ctypes.data if n else None, n, out.ctypes.data, cap)
    assert (out[cap:] == 0xA5).all(), 'bytes behind cap were written'
    return r, out[:max(r, 0)].tobytes()


def encode_cdf16(lib, c1, s, cap=None):
    """The same stream through linr_ac_encode_cdf16, one row [0, c1, 0] per symbol: the return convention of encode()."""
    n = len(c1)
    rows = np.zeros((n, 3), dtype=np.uint16)
    rows[:, 1] = c1
    sym = (np.asarray(s) != 0).astype(np.int16)
    cap = 2 * n + 64 if cap is None else cap
    out = np.full(cap + GUARD, 0xA5, dtype=np.uint8)
    r = lib.linr_ac_encode_cdf16(rows.ctypes.data if n else None, 3, 0, sym.ctypes.data if n else None, n, out.ctypes.data, cap)
    assert (out[cap:] == 0xA5).all(), 'bytes behind cap were written'
    return r, out[:max(r, 0)].tobytes()


def same(lib, c1, s, what):
    want = encode_cdf16(lib, c1, s)
    got = encode(lib.linr_ac_encode_binary_codes, c1, s)
    assert want[0] >= 1
    assert got[0] == want[0], (what, got[0], want[0])
    assert got[1] == want[1], what
    return want


@pytest.mark.parametrize('regime', REGIMES)
def test_body_gives_the_host_coders_bytes(lib, regime):
    for n in NS:
        c1, s = draw(regime, n, 1000 * REGIMES.index(regime) + n % 997)
        r, data = same(lib, c1, s, (regime, n))
        if n == 0:
            assert data == b'\x40'                        # the host's one byte
        if regime == 'loud' and n >= 1000:
            assert r > 4 * 256                            # several staging blocks
        if regime == 'quiet' and n == 1000:
            assert r < 64


# ---- long runs of pending bits ---------------------------------------------------------------------------------------------

def model_step(low, high, pending, c1, sym):
    """The coder's interval, one bit at a time: (low, high, pending, emitted a bit)."""
    span = high - low + 1
    t = (span * c1) >> 16
    if sym:
        low = low + t
    else:
        high = low + t - 1
    emitted = False
    while True:
        if high < 0x80000000 or low >= 0x80000000:
            emitted, pending = True, 0
            low = (low << 1) & 0xFFFFFFFF
            high = ((high << 1) & 0xFFFFFFFF) | 1
        elif low >= 0x40000000 and high < 0xC0000000:
            pending += 1
            low = (low << 1) & 0x7FFFFFFF
            high = ((high << 1) & 0xFFFFFFFF) | 0x80000001
        else:
            return low, high, pending, emitted


def greedy_prefix(steps):
    """Symbols that emit no bit and leave `pending` as large as possible: the interval is kept around the middle."""
    low, high, pending = 0, 0xFFFFFFFF, 0
    c1s, syms = [], []
    for _ in range(steps):
        span = high - low + 1
        c = ((0x80000000 - low) << 16) // span
        best = None
        for cc in (c - 1, c, c + 1, c + 2):
            for sym in (0, 1):
                if not 1 <= cc <= 65535:
                    continue
                lo, hi, pe, emitted = model_step(low, high, pending, cc, sym)
                if not emitted and (best is None or pe > best[2]):
                    best = (lo, hi, pe, cc, sym)
        if best is None:
            break
        low, high, pending = best[:3]
        c1s.append(best[3])
        syms.append(best[4])
    return c1s, syms, pending


@pytest.mark.parametrize('steps', [16, 40])
def test_long_pending_runs(lib, steps):
    c1s, syms, pending = greedy_prefix(steps)
    assert pending >= 96, 'the generator: a run that crosses the 32- and 64-bit pieces of the run writer'
    rng = np.random.default_rng(steps)
    # the end of the stream: the finish path flushes the outstanding run
    r, data = same(lib, c1s, syms, 'end of stream')
    assert r >= pending // 8
    for sym in (0, 1):                                    # a near-certain symbol at either end resolves the run with bit 0 / bit 1
        c1 = c1s + [65535 if sym else 1] + rng.integers(1, 65536, 70).tolist()
        s = syms + [sym] + rng.integers(0, 2, 70).tolist()
        same(lib, c1, s, ('resolved by', sym))
    with_run, without = (encode(lib.linr_ac_encode_binary_codes, c1s + [c], syms + [b])[1] for c, b in ((1, 0), (65535, 1)))
    assert with_run[:8] != without[:8]                    # the two endings do differ in the run's polarity


# ---- no space ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('regime', REGIMES)
def test_small_cap_is_enospc_and_guard_bytes_stay(lib, regime):
    for n in (0, 1, 33, 257, 1000):
        c1, s = draw(regime, n, 77 + n)
        want, data = same(lib, c1, s, (regime, n))
        r, got = encode(lib.linr_ac_encode_binary_codes, c1, s, cap=want)            # exactly enough
        assert (r, got) == (want, data)
        for cap in (want - 1, 0):
            assert encode(lib.linr_ac_encode_binary_codes, c1, s, cap=cap)[0] == -2, (regime, n, cap)
            assert encode_cdf16(lib, c1, s, cap=cap)[0] == -2


def test_device_entry_checks_its_table_before_any_launch(lib):
    """The checks of linr_rc_encode_codes that need no GPU: they come before the first launch, so a bad table is refused without a GPU."""
    import ctypes
    from linr_pcgc_amd import _lib
    assert lib.linr_rc_encode_ws_bytes(-1, 0) == 0 and lib.linr_rc_encode_ws_bytes(8, 1000) > 0
    P = 0x1000                                            # never dereferenced: every call below fails its checks

    def call(rows, out_bytes=4096, payload_bytes=4096, n=None, ws_bytes=1 << 20):
        tab = (_lib.LinrRcStream * len(rows))(*[_lib.LinrRcStream(*r) for r in rows])
        return lib.linr_rc_encode_codes(P, P, ctypes.addressof(tab), len(rows) if n is None else n, P, out_bytes, P, P, payload_bytes, P, P,
                                        ws_bytes, None)
    good = [(0, 0, 10, 0, 84), (10, 1, 10, 84, 84)]
    assert call(good, n=-1) == -1
    assert call([(0, 0, -1, 0, 84)]) == -1                # negative n
    assert call([(0, 0, 10, 0, -1)]) == -1                # negative cap
    assert call([(0, 0, 10, 2, 84)]) == -1                # unaligned out offset
    assert call([(0, 0, 10, 0, 84), (10, 1, 10, 80, 84)]) == -1          # overlapping regions
    assert call(good, out_bytes=167) == -1                # a region past out_bytes
    assert call(good, payload_bytes=167) == -1            # a payload smaller than the caps together
    assert call([(0, 0, (1 << 27) - 1, 0, 84)]) == -1     # n over the row bound
    assert call(good, ws_bytes=lib.linr_rc_encode_ws_bytes(2, 168) - 1) == -1
    assert lib.linr_rc_encode_codes(None, None, None, 0, None, 0, None, None, 0, None, None, 0, None) == 0


def test_run_flags_are_parsed_and_off_by_default():
    from linr_pcgc_amd import run
    base = ['--input-glob', 'x*.npy', '--out', 'o']
    a = run.parse(base)
    assert a.device_coder is False and a.coder_group == 8
    a = run.parse(base + ['--device-coder', '--coder-group', '3'])
    assert a.device_coder is True and a.coder_group == 3

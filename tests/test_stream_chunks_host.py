"""CPU: chunked stage streams (linr_pcgc_amd/stream_chunks.py; opt-in, side_info.json's stream_chunk = S).  The format's helpers, the
checked parsers (Python and linr_stream_split_chunks, the latter also under AddressSanitizer + UBSan through tools/stream_chunks_emul.cpp),
and both host coder entries with chunk=S: chunk j of a chunked stream is the unchunked coder on that slice, byte for byte.  All exact."""
import ctypes
import os

import numpy as np
import pytest

from test_device_coder_host import pack_symbols      # noqa: E402

SIZES = (64, 128, 4096)


def lengths(S):
    return (1, S - 1, S, S + 1, 2 * S, 2 * S + 1, 5 * S + 17)


@pytest.fixture(scope='module')
def lib():
    from linr_pcgc_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.lib()


def draw(n, seed):
    """Probabilities of symbol 1 (float32 [n]) with both saturated ends among them, and symbols drawn from them."""
    rng = np.random.default_rng(seed)
    p = rng.random(n).astype(np.float32)
    ends = rng.random(n)
    p[ends < 0.15] = 0.0
    p[ends > 0.85] = 1.0
    return p, (rng.random(n) < p).astype(np.uint8)


def code_values(p):
    """The coder's code value of a probability, as csrc/ac.cpp computes it in fp32."""
    return ((np.rint((np.float32(1) - p) * np.float32(65534)).astype(np.int64) + 1) & 0xFFFF).astype(np.uint16)


@pytest.fixture(scope='module')
def coded(lib):
    """For every S and n: the inputs, the unchunked coder's stream of every slice [j S, (j + 1) S) and of the whole (computed once)."""
    from linr_pcgc_amd.model_core import encode_streams
    out = {}
    for S in SIZES:
        for n in lengths(S):
            p, s = draw(n, 7 * S + n)
            slices = [(a, min(a + S, n)) for a in range(0, n, S)]
            want = encode_streams([p[a:b] for a, b in slices], [s[a:b] for a, b in slices])
            out[S, n] = (p, s, want, encode_streams([p], [s])[0])
    return out


def test_leb128_round_trips():
    from linr_pcgc_amd import stream_chunks as sc
    for v in (0, 127, 128, 16383, 16384, 2 ** 32 - 1):
        b = sc.leb128(v)
        assert sc.read_leb128(b + b'\xff', 0) == (v, len(b))
        assert len(b) == max(1, (v.bit_length() + 6) // 7) <= 5
    assert sc.leb128(127) == b'\x7f' and sc.leb128(128) == b'\x80\x01' and sc.leb128(16384) == b'\x80\x80\x01'
    for bad in (-1, 1 << 35):
        with pytest.raises(ValueError):
            sc.leb128(bad)


def test_chunk_size_rules(lib):
    from linr_pcgc_amd import stream_chunks as sc
    for good in (0, None, 64, 128, 65536, 1 << 24):
        assert sc.check_chunk(good) == (good or 0)
    for bad in (-64, 1, 63, 65, 96, (1 << 24) + 64):
        with pytest.raises(ValueError):
            sc.check_chunk(bad)
        assert lib.linr_stream_chunk_count(10, bad) == -1
    assert [sc.chunk_count(n, 64) for n in (0, 1, 64, 65, 128, 129)] == [1, 1, 1, 2, 2, 3]
    assert [lib.linr_stream_chunk_count(n, 64) for n in (0, 1, 64, 65, 128, 129)] == [1, 1, 1, 2, 2, 3]
    assert sc.chunk_count(10 ** 6, 0) == 1 and lib.linr_stream_chunk_count(10 ** 6, 0) == 1 and lib.linr_stream_chunk_count(-1, 64) == -1
    assert sc.chunk_entries([130, 5, 0], 64) == [(0, 0, 64), (0, 64, 64), (0, 128, 2), (1, 0, 5), (2, 0, 0)]
    assert sc.chunk_entries([130, 5], 0) == [(0, 0, 130), (1, 0, 5)]


def c_split(lib, stream, n, S, k_arrays=None):
    """linr_stream_split_chunks on a copy of `stream`: (return value, [(offset, length)] or None); a refusal left the arrays alone."""
    from linr_pcgc_amd.stream_chunks import chunk_count
    k = chunk_count(n, S) if k_arrays is None else k_arrays
    buf = np.frombuffer(bytes(stream), dtype=np.uint8).copy()
    ptrs = (ctypes.c_void_p * max(k, 1))(*([0x5A5A] * max(k, 1)))
    lens = (ctypes.c_int64 * max(k, 1))(*([-77] * max(k, 1)))
    r = lib.linr_stream_split_chunks(buf.ctypes.data if buf.size else None, int(buf.size), n, S, ptrs, lens, k)
    if r < 0:
        assert all(p == 0x5A5A for p in ptrs) and all(v == -77 for v in lens), 'a refused stream wrote to the chunk arrays'
        return r, None
    return r, [((ptrs[j] or buf.ctypes.data) - buf.ctypes.data, lens[j]) for j in range(r)]


def test_join_and_split_agree_in_python_and_c(lib):
    from linr_pcgc_amd import stream_chunks as sc
    rng = np.random.default_rng(3)
    for k, S in ((1, 64), (2, 64), (5, 128), (40, 64)):
        chunks = [bytes(rng.integers(0, 256, int(m), dtype=np.uint8)) for m in rng.integers(1, 400, k)]
        n = (k - 1) * S + 1
        stream = sc.join_chunks(chunks)
        assert sc.split_chunks(stream, n, S) == chunks
        if k == 1:
            assert stream == chunks[0]
        r, got = c_split(lib, stream, n, S)
        assert r == k and [stream[o:o + m] for o, m in got] == chunks


def test_malformed_headers_are_refused_and_write_nothing(lib):
    from linr_pcgc_amd import stream_chunks as sc
    S, k = 64, 4
    n = (k - 1) * S + 9
    chunks = [b'a' * 200, b'b' * 3, b'c' * 130, b'd' * 7]
    stream = sc.join_chunks(chunks)
    header = len(stream) - sum(len(c) for c in chunks)
    assert header == 2 + 1 + 2
    bad = {'truncated at %d' % cut: stream[:cut] for cut in range(header)}          # every cut inside the header, the empty stream too
    bad['a varint of six bytes'] = b'\x80\x80\x80\x80\x80\x00' + stream
    bad['an unterminated fifth byte'] = b'\xff' * 5
    bad['lengths one past the bytes'] = stream[:header + 200 + 3 + 130 - 1]
    bad['a length of 2^34'] = sc.leb128(1 << 34) + stream
    for what, data in bad.items():
        with pytest.raises(ValueError):
            sc.split_chunks(data, n, S)
        assert c_split(lib, data, n, S) == (-1, None), what
    assert c_split(lib, stream, n, S, k_arrays=k - 1) == (-2, None)                 # a chunk array one short
    # the lengths may take every byte present: the last chunk is then empty (no coder writes one, the parser does not judge that)
    assert sc.split_chunks(stream[:header + 333], n, S)[-1] == b'' and c_split(lib, stream[:header + 333], n, S)[0] == k
    with pytest.raises(ValueError):
        sc.split_chunks(stream, n, 96)


def test_parser_under_sanitizers(tmp_path):
    """tools/stream_chunks_emul.cpp: linr_stream_split_chunks on streams in exact-size heap buffers - good ones, every truncation of
    their headers, oversized varints, lengths past the end - under AddressSanitizer + UBSan.  Host code only."""
    import shutil
    import subprocess
    if shutil.which('g++') is None:
        pytest.skip('no g++')
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / 'stream_chunks_emul')
    build = subprocess.run(['g++', '-O1', '-g', '-std=c++17', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined',
                            '-fno-omit-frame-pointer', '-o', exe, os.path.join(root, 'tools', 'stream_chunks_emul.cpp'),
                            os.path.join(root, 'linr_pcgc_amd', 'csrc', 'ac.cpp'), '-lpthread'], capture_output=True, text=True, timeout=600)
    if build.returncode != 0 and 'asan' in (build.stderr or '').lower():
        pytest.skip('sanitizer runtime not installed')
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([exe, '200'], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0 and 'all as expected' in run.stdout, (run.stdout[-500:], run.stderr[-3000:])


@pytest.mark.parametrize('S', SIZES)
def test_chunks_from_probabilities_are_the_unchunked_coder_on_the_slices(coded, S):
    from linr_pcgc_amd import stream_chunks as sc
    from linr_pcgc_amd.model_core import encode_streams
    ns = lengths(S)
    got = encode_streams([coded[S, n][0] for n in ns], [coded[S, n][1] for n in ns], 3, S)          # all lengths in one call
    for n, stream in zip(ns, got):
        _, _, want, plain = coded[S, n]
        assert sc.split_chunks(stream, n, S) == want, n
        assert stream == sc.join_chunks(want)
        if n <= S:
            assert stream == plain
        else:
            assert len(want) == -(-n // S) and stream != plain
    assert encode_streams([coded[S, n][0] for n in ns], [coded[S, n][1] for n in ns]) == [coded[S, n][3] for n in ns]


@pytest.mark.parametrize('S', SIZES)
def test_chunks_from_code_values_are_the_same_streams(coded, S):
    from linr_pcgc_amd import stream_chunks as sc
    from linr_pcgc_amd.model_core import encode_streams_codes
    ns = lengths(S)
    c1s = [code_values(coded[S, n][0]) for n in ns]
    ws = [pack_symbols(coded[S, n][1]) for n in ns]
    got = encode_streams_codes(c1s, ws, ns, 3, S)
    for n, stream in zip(ns, got):
        assert stream == sc.join_chunks(coded[S, n][2]), n
    assert encode_streams_codes(c1s, ws, ns) == [coded[S, n][3] for n in ns]          # chunk 0: today's streams
    with pytest.raises(ValueError):
        encode_streams_codes(c1s, ws, ns, 3, 100)


@pytest.mark.parametrize('threads', [1, 4])
@pytest.mark.parametrize('S', SIZES)
def test_decoding_returns_the_symbols(coded, S, threads):
    from linr_pcgc_amd import _lib
    from linr_pcgc_amd.model_core import decode_streams
    from linr_pcgc_amd.stream_chunks import join_chunks
    ns = lengths(S)
    ps = [coded[S, n][0] for n in ns]
    got = decode_streams(ps, [join_chunks(coded[S, n][2]) for n in ns], threads, S)
    for n, sym in zip(ns, got):
        assert np.array_equal(sym, coded[S, n][1]), n
    plain = decode_streams(ps, [coded[S, n][3] for n in ns], threads)
    assert all(np.array_equal(sym, coded[S, n][1]) for n, sym in zip(ns, plain))
    n = ns[-1]
    with pytest.raises(_lib.LinrError):
        decode_streams([coded[S, n][0]], [join_chunks(coded[S, n][2])[:3]], threads, S)


def test_device_entry_checks_before_any_launch(lib):
    """The checks of linr_rc_encode_codes_chunked that need no GPU: they come before the first launch."""
    from linr_pcgc_amd import _lib
    from linr_pcgc_amd.model_core import DeviceCoderSet
    assert lib.linr_rc_encode_chunked_ws_bytes(-1, 0) == 0 and lib.linr_rc_encode_chunked_ws_bytes(4, 3) == 0
    assert lib.linr_rc_encode_chunked_ws_bytes(4, 9) > 0
    P = 0x1000                                            # never dereferenced: every call below fails its checks

    def call(rows, S, out_bytes=1 << 16, payload_bytes=1 << 16, ws_bytes=1 << 20):
        tab = (_lib.LinrRcStream * len(rows))(*[_lib.LinrRcStream(*r) for r in rows])
        return lib.linr_rc_encode_codes_chunked(P, P, ctypes.addressof(tab), len(rows), S, P, out_bytes, P, P, payload_bytes, P, P, ws_bytes, None)
    tab, total = DeviceCoderSet.table([(0, 0, 200), (200, 7, 64), (264, 9, 65)], 64)
    assert tab[:, 4].tolist() == [2 * 200 + 64 * 4, 2 * 64 + 64, 2 * 65 + 64 * 2] and total == int(tab[-1, 3] + tab[-1, 4] + 2)
    assert DeviceCoderSet.chunks(tab[:, :3], 64) == 7 and DeviceCoderSet.chunks(tab[:, :3]) == 3
    rows = [tuple(int(v) for v in r) for r in tab]
    for bad_s in (1, 96, -64, (1 << 24) + 64):
        assert call(rows, bad_s) == -1
    short = list(rows)
    short[0] = rows[0][:4] + (rows[0][4] - 1,)             # a region one byte short of its chunks' regions
    assert call(short, 64) == -1
    assert call(rows, 64, payload_bytes=int(tab[:, 4].sum()) + 5 * 4 - 1) == -1          # the payload: the caps and a full header each
    assert call(rows, 64, out_bytes=total - 3) == -1
    assert call(rows, 64, ws_bytes=lib.linr_rc_encode_chunked_ws_bytes(3, 7) - 1) == -1
    overlap = list(rows)
    overlap[1] = rows[1][:3] + (rows[0][3] + 4, rows[1][4])
    assert call(overlap, 64) == -1
    assert lib.linr_rc_encode_codes_chunked(None, None, None, 0, 64, None, 0, None, None, 0, None, None, 0, None) == 0


def test_run_flag_is_parsed_and_off_by_default():
    from linr_pcgc_amd import run
    base = ['--input-glob', 'x*.npy', '--out', 'o']
    assert run.parse(base).stream_chunk == 0
    assert run.parse(base + ['--stream-chunk', '128']).stream_chunk == 128
    for bad in (['--stream-chunk', '100'], ['--stream-chunk', '32'], ['--stream-chunk', '128', '--hidden-channel-conv', '16']):
        with pytest.raises(SystemExit):
            run.parse(base + bad)

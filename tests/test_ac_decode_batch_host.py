"""CPU: linr_ac_decode_binary_batch, the decode twin of linr_ac_encode_binary_batch (the range decoders of a lock-step decode
group on a pool of host threads), against one linr_ac_decode_binary call per stream: byte for byte, for every pool size.
linr_ac_decode_binary reads a truncated stream as if zeros followed (like torchac) and returns 0, so there is no per-stream
error code to propagate from a short stream; the batch entry's own argument checks are covered instead."""
import ctypes
import os

import numpy as np
import pytest

N_STREAMS = 24


@pytest.fixture(scope='module')
def lib():
    from linr_pcgc_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.lib()


@pytest.fixture(scope='module')
def streams(lib):
    """24 random binary streams (lengths 0, 1 and 1 000 .. 50 000; probabilities down to 1e-7 from 0 and 1), coded as a batch."""
    rng = np.random.default_rng(4)
    ns = [0, 1] + [int(v) for v in rng.integers(1000, 50001, N_STREAMS - 2)]
    ps, ss = [], []
    for i, n in enumerate(ns):
        p = rng.random(n).astype(np.float32)
        if i % 3 == 1:          # all but certain
            p = np.where(rng.random(n) < 0.5, np.float32(1e-7), np.float32(1) - np.float32(1e-7)).astype(np.float32)
        if i % 3 == 2:          # a mix, with exact 0 and 1 now and then
            edge = rng.random(n)
            p = np.where(edge < 0.05, np.float32(0), np.where(edge > 0.95, np.float32(1), p)).astype(np.float32)
        s = (rng.random(n) < p).astype(np.uint8)          # p == 0 / 1: only the possible symbol
        ps.append(np.ascontiguousarray(p))
        ss.append(np.ascontiguousarray(s))
    outs = [np.empty(2 * n + 64, dtype=np.uint8) for n in ns]
    arr = lambda xs: (ctypes.c_void_p * N_STREAMS)(*[x.ctypes.data for x in xs])
    lens = (ctypes.c_int64 * N_STREAMS)()
    rc = lib.linr_ac_encode_binary_batch(arr(ps), arr(ss), (ctypes.c_int64 * N_STREAMS)(*ns), N_STREAMS, arr(outs),
                                         (ctypes.c_int64 * N_STREAMS)(*[o.size for o in outs]), lens, 8)
    assert rc == 0
    coded = [np.ascontiguousarray(outs[i][:lens[i]]) for i in range(N_STREAMS)]
    single = []
    for i, n in enumerate(ns):          # the reference: one call per stream
        back = np.full(n + 1, 9, dtype=np.uint8)
        assert lib.linr_ac_decode_binary(ps[i].ctypes.data, n, coded[i].ctypes.data if coded[i].size else None, coded[i].size,
                                         back.ctypes.data) == 0
        assert back[n] == 9 and np.array_equal(back[:n], ss[i])
        single.append(back[:n].copy())
    return ns, ps, coded, single


def batch_decode(lib, ns, ps, coded, n_threads):
    outs = [np.full(n + 1, 9, dtype=np.uint8) for n in ns]
    k = len(ns)
    rc = lib.linr_ac_decode_binary_batch((ctypes.c_void_p * k)(*[p.ctypes.data for p in ps]), (ctypes.c_int64 * k)(*ns),
                                         (ctypes.c_void_p * k)(*[c.ctypes.data if c.size else None for c in coded]),
                                         (ctypes.c_int64 * k)(*[c.size for c in coded]), k,
                                         (ctypes.c_void_p * k)(*[o.ctypes.data for o in outs]), n_threads)
    return rc, outs


@pytest.mark.parametrize('n_threads', [1, 4, 16])
def test_batch_decode_equals_per_stream_decode(lib, streams, n_threads):
    ns, ps, coded, single = streams
    rc, outs = batch_decode(lib, ns, ps, coded, n_threads)
    assert rc == 0
    for i, n in enumerate(ns):
        assert outs[i][n] == 9, i                          # nothing behind a stream's symbols
        assert outs[i][:n].tobytes() == single[i].tobytes(), i


def test_truncated_stream_is_tolerated_as_by_the_single_stream_entry(lib, streams):
    """What linr_ac_decode_binary does with half a stream today: it returns 0 (the missing bytes read as zeros).  The batch
    returns the same, decodes that stream to the same symbols as the single call, and leaves the other streams alone."""
    ns, ps, coded, single = streams
    k = max(range(N_STREAMS), key=lambda i: ns[i])
    half = np.ascontiguousarray(coded[k][:coded[k].size // 2])
    alone = np.empty(ns[k], dtype=np.uint8)
    assert lib.linr_ac_decode_binary(ps[k].ctypes.data, ns[k], half.ctypes.data, half.size, alone.ctypes.data) == 0
    cut = list(coded)
    cut[k] = half
    rc, outs = batch_decode(lib, ns, ps, cut, 4)
    assert rc == 0
    for i, n in enumerate(ns):
        want = alone if i == k else single[i]
        assert outs[i][:n].tobytes() == want.tobytes(), i


def test_batch_decode_argument_checks(lib):
    """A bad stream's code comes back from the batch (the first non-zero one), the others are still decoded."""
    p = np.full(8, 0.5, dtype=np.float32)
    s = np.array([1, 0, 1, 1, 0, 0, 1, 0], dtype=np.uint8)
    out = np.empty(64, dtype=np.uint8)
    n = lib.linr_ac_encode_binary(p.ctypes.data, s.ctypes.data, 8, out.ctypes.data, out.size)
    assert n > 0
    backs = [np.zeros(8, dtype=np.uint8) for _ in range(3)]
    P = (ctypes.c_void_p * 3)(p.ctypes.data, None, p.ctypes.data)          # stream 1: NULL probabilities -> LINR_EINVAL
    N = (ctypes.c_int64 * 3)(8, 8, 8)
    I = (ctypes.c_void_p * 3)(*[out.ctypes.data] * 3)
    IL = (ctypes.c_int64 * 3)(n, n, n)
    O = (ctypes.c_void_p * 3)(*[b.ctypes.data for b in backs])
    for threads in (1, 3):
        for b in backs:
            b[:] = 0
        assert lib.linr_ac_decode_binary_batch(P, N, I, IL, 3, O, threads) == -1
        assert np.array_equal(backs[0], s) and np.array_equal(backs[2], s)
    assert lib.linr_ac_decode_binary_batch(None, N, I, IL, 3, O, 2) == -1
    assert lib.linr_ac_decode_binary_batch(P, N, I, IL, -1, O, 2) == -1
    assert lib.linr_ac_decode_binary_batch(None, None, None, None, 0, None, 2) == 0


def test_lockstep_groups_follow_the_frame_list_and_split_on_the_scale_count():
    """codec.lockstep_groups: up to B consecutive entries of the frame list per group, in its order; frames with another number of
    scale streams start a new group."""
    from linr_pcgc_amd import codec
    five = {i: 5 for i in range(8)}
    assert codec.lockstep_groups(list(range(5)), five, 2) == [[0, 1], [2, 3], [4]]
    assert codec.lockstep_groups([3, 1], five, 2) == [[3, 1]]
    assert codec.lockstep_groups(list(range(5)), five, 1) == [[0], [1], [2], [3], [4]]
    assert codec.lockstep_groups([0, 1, 2, 3], {0: 5, 1: 2, 2: 2, 3: 5}, 4) == [[0], [1, 2], [3]]

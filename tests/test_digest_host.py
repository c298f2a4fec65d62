"""CPU: the geometry digest of self-checking streams (opt-in; stream_digests.py, include/linr_hip.h "geometry digests").  The numpy
restatement (tests/digest_ref.py) against the definition's known answers, the host twin linr_coords_digest_host - the text the GPU
kernels run (csrc/digest_body.h) - against the restatement, the file format's pack / unpack, and the twin under AddressSanitizer +
UBSan as a program of its own (tools/digest_emul.cpp).  All exact."""
import os

import numpy as np
import pytest

import digest_ref

NS = (0, 1, 63, 64, 65, 1000, 100003)
I32 = np.iinfo(np.int32)


@pytest.fixture(scope='module')
def lib():
    from linr_pcgc_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.lib()


def host_digest(lib, rows, origin=None):
    rows = np.ascontiguousarray(rows, dtype=np.int32).reshape(-1, 3)
    org = None if origin is None else np.ascontiguousarray(origin, dtype=np.int32)
    return int(lib.linr_coords_digest_host(rows.ctypes.data if rows.size else None, rows.shape[0], None if org is None else org.ctypes.data))


def random_rows(rng, n):
    """n rows over the whole int32 range, both ends and duplicates of earlier rows included."""
    rows = rng.integers(I32.min, int(I32.max) + 1, size=(n, 3), dtype=np.int64).astype(np.int32)
    if n >= 4:
        rows[0] = (I32.min, I32.max, -1)
        rows[1] = (I32.max, I32.min, 0)
        dup = rng.integers(0, n, size=max(1, n // 10))
        rows[dup] = rows[rng.integers(0, n, size=dup.size)]
        rows[n - 1] = rows[n - 2]
    return rows


def test_reference_known_answers():
    for rows, origin, want in digest_ref.KNOWN:
        assert digest_ref.digest(rows, origin) == want
        assert digest_ref.digest(rows, origin) >> 32 == want >> 32
    # the same values from plain Python integers (stream_digests.mix), row by row
    from linr_pcgc_amd import stream_digests as sd
    for rows, origin, want in digest_ref.KNOWN:
        s = 0
        for row in rows:
            x, y, z = [(c + o) & 0xFFFFFFFF for c, o in zip(row, origin)]
            s = (s + sd.mix(sd.mix(x | (y << 32)) + z + sd.G)) & (2 ** 64 - 1)
        assert sd.mix(s ^ sd.mix(len(rows) + sd.G)) == want
    assert sd.empty_digest() == digest_ref.KNOWN[0][2]


def test_host_twin_known_answers(lib):
    for rows, origin, want in digest_ref.KNOWN:
        assert host_digest(lib, rows, origin) == want
        if not any(origin):
            assert host_digest(lib, rows) == want


@pytest.mark.parametrize('n', NS)
def test_host_twin_equals_reference(lib, n):
    rng = np.random.default_rng(8807 + n)
    rows = random_rows(rng, n)
    want = digest_ref.digest(rows)
    assert host_digest(lib, rows) == want
    for origin in ((0, 0, 0), (10, -20, 30), (I32.max, I32.min, -1)):
        with_origin = digest_ref.digest(rows, origin)
        assert host_digest(lib, rows, origin) == with_origin
        if n and any(origin):
            assert with_origin != want
    perm = rng.permutation(n)
    assert host_digest(lib, rows[perm]) == want
    assert digest_ref.digest(rows[perm]) == want


def test_single_bit_changes_change_the_stored_value(lib):
    """2000 single-bit changes of a 5000-row set: with the reference alone all 2000 values of D >> 32 are distinct from each other and
    from the base's; the host twin gives each of them."""
    rng = np.random.default_rng(5000)
    rows = rng.integers(I32.min, int(I32.max) + 1, size=(5000, 3), dtype=np.int64).astype(np.int32)
    base_terms = digest_ref.row_terms(rows)
    base = digest_ref.digest(rows)
    flat = rng.choice(rows.size * 32, size=2000, replace=False)
    seen = {base >> 32}
    for k, f in enumerate(flat.tolist()):
        cell, bit = divmod(f, 32)
        r, a = divmod(cell, 3)
        changed = rows[r].copy()
        changed.view(np.uint32)[a] ^= np.uint32(1 << bit)
        # D of the changed set from the base's terms: one term replaced (the sum is what makes this cheap)
        with np.errstate(over='ignore'):
            s = np.add.reduce(base_terms, dtype=np.uint64) - base_terms[r] + digest_ref.row_terms(changed)[0]
            d = int(digest_ref.mix(np.uint64(s) ^ digest_ref.mix(np.uint64(5000) + digest_ref.G)))
        assert d >> 32 not in seen, (k, r, a, bit)
        seen.add(d >> 32)
        if k % 100 == 0:                                  # the twin, and the shortcut above against the whole restatement
            other = rows.copy()
            other[r] = changed
            assert digest_ref.digest(other) == d
            assert host_digest(lib, other) == d
    assert len(seen) == 2001


def test_pack_unpack():
    from linr_pcgc_amd import stream_digests as sd
    frames = [[0x8e58975f6d0dc556, 0x2fb051dd12d1e535, 0], [0xffffffff00000000], []]
    data = sd.pack(frames)
    assert data == bytes.fromhex('5f97588e' 'dd51b02f' '00000000' 'ffffffff')
    assert sd.unpack(data, [3, 1, 0]) == [[0x8e58975f, 0x2fb051dd, 0], [0xffffffff], []]
    assert sd.unpack(b'', []) == [] and sd.pack([]) == b''
    for bad in (data[:-1], data + b'\0', b''):
        with pytest.raises(ValueError, match='digests.bin has %d bytes' % len(bad)):
            sd.unpack(bad, [3, 1, 0])
    with pytest.raises(ValueError):
        sd.unpack(data, [3, 2])
    assert sd.bits(None) == 0 and sd.bits(data) == 8 * 16 + 8
    assert sd.VERSION == 1
    assert sd.check_version({}) == 0 and sd.check_version({'digests': 1}) == 1
    from linr_pcgc_amd._lib import LinrError
    with pytest.raises(LinrError, match='written by a newer build'):
        sd.check_version({'digests': 2})


def test_digest_error_names_frame_and_scale():
    from linr_pcgc_amd._lib import LinrDigestError, LinrError
    e = LinrDigestError(3, 2, 0x11, 0x22)
    assert isinstance(e, LinrError) and (e.frame, e.scale, e.want, e.got) == (3, 2, 0x11, 0x22)
    assert 'frame 3' in str(e) and 'scale 2' in str(e) and 'another build' in str(e) and 'damaged' in str(e)


def test_twin_under_sanitizers(tmp_path):
    """tools/digest_emul.cpp: linr_coords_digest_host on coordinate lists in exact-size heap buffers - the known answers, random lists
    with both ends of int32 in rows and origins - under AddressSanitizer + UBSan.  Host code only, a program of its own."""
    import shutil
    import subprocess
    if shutil.which('g++') is None:
        pytest.skip('no g++')
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / 'digest_emul')
    build = subprocess.run(['g++', '-O1', '-g', '-std=c++17', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined',
                            '-fno-omit-frame-pointer', '-o', exe, os.path.join(root, 'tools', 'digest_emul.cpp'),
                            os.path.join(root, 'linr_pcgc_amd', 'csrc', 'digest_host.cpp')], capture_output=True, text=True, timeout=600)
    if build.returncode != 0 and 'asan' in (build.stderr or '').lower():
        pytest.skip('sanitizer runtime not installed')
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([exe, '200'], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0 and 'all as expected' in run.stdout, (run.stdout[-500:], run.stderr[-3000:])

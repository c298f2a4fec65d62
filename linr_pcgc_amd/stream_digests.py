"""Per-scale geometry digests (opt-in; side_info.json's ``digests`` = 1, bins/digests.bin): what makes a stream self-checking.

The decoder reproduces the encoder's probabilities bit for bit or decodes garbage, and the range decoders are defined on any bytes:
another code object, a flipped bit, two swapped files all decode "successfully" into a wrong cloud.  With digests the encoder records,
for every frame i of the GOP in order and every scale s = 0 .. n_scales_i - 1, one little-endian uint32 = D(i, s) >> 32, where D is the
64-bit digest (include/linr_hip.h, "geometry digests"; csrc/digest_body.h) of the child coordinates scale s of frame i decodes to:
for s >= 1 the level's coordinates in the frame's shifted system, for s = 0 the frame's voxels with the frame's origin
(coord_data_min) added - the decoder's output, so the origin carried in low_enc_bytes.bin is covered too.  No header: the file is
4 * sum(n_scales_i) bytes, anything else is an error.  A decoder checks each level as soon as it has decoded it and raises
_lib.LinrDigestError at the first that differs, before garbage is expanded eightfold per scale.

Counted in model_bpp / bpp_all as 8 * len(digests.bin) + 8 bits (the file and the one-byte side_info field).  Decoders of builds
that do not know the field ignore it and the file.
"""
import numpy as np

VERSION = 1                     # side_info.json's 'digests'
SIDE_BITS = 8                   # what that field is counted as in model_bpp / bpp_all, beside the file's own bytes
ENTRY_BYTES = 4

G = 0x9E3779B97F4A7C15
_M64 = (1 << 64) - 1


def mix(v):
    """m of the definition, on a Python integer."""
    v &= _M64
    v ^= v >> 30
    v = (v * 0xBF58476D1CE4E5B9) & _M64
    v ^= v >> 27
    v = (v * 0x94D049BB133111EB) & _M64
    v ^= v >> 31
    return v


def empty_digest():
    """D of no rows."""
    return mix(mix(G))


def bits(digests_bin):
    """What a GOP's digests cost in model_bpp / bpp_all."""
    return 0 if digests_bin is None else 8 * len(digests_bin) + SIDE_BITS


def pack(frames_digests):
    """digests.bin of per-frame lists of 64-bit digests D (scale 0 first): the top 32 bits of each, little endian."""
    flat = [int(d) >> 32 for fd in frames_digests for d in fd]
    return np.asarray(flat, dtype='<u4').tobytes()


def unpack(data, n_scales):
    """Per frame the stored values (D >> 32, scale 0 first) of a GOP whose frames have n_scales[i] scale streams; ValueError when the
    length is not 4 * sum(n_scales)."""
    want = ENTRY_BYTES * sum(int(n) for n in n_scales)
    if len(data) != want:
        raise ValueError('digests.bin has %d bytes; the GOP\'s stream files (%d frames, %d scales in all) need %d'
                         % (len(data), len(n_scales), want // ENTRY_BYTES, want))
    vals = np.frombuffer(data, dtype='<u4').tolist()
    out, at = [], 0
    for n in n_scales:
        out.append(vals[at:at + int(n)])
        at += int(n)
    return out


def check_version(side_info):
    """The format version of a GOP's digests (0: it has none); a version this build does not know raises LinrError."""
    v = int(side_info.get('digests', 0) or 0)
    if v > VERSION:
        from ._lib import LinrError
        raise LinrError('the GOP\'s digests have format version %d, written by a newer build; this build reads version %d (decode '
                        'with verify=False to ignore them)' % (v, VERSION))
    return v

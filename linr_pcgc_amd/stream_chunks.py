"""Chunked stage streams (opt-in; side_info.json's ``stream_chunk`` = S): a stage stream cut into chunks of S symbols that are coded
and decoded independently, so the range coding of ONE stream runs on several threads (or waves).

S is a multiple of 64 in 64..2^24.  A stage stream of n symbols has k = max(1, ceil(n / S)) chunks; chunk j is exactly the bytes the
coder emits for symbols [j S, min((j + 1) S, n)) as a stream of their own.  k == 1: the stream is that chunk, today's stream byte for
byte.  k > 1: the byte lengths of chunks 0 .. k - 2, each as unsigned LEB128 of at most 5 bytes, then the chunks; the last chunk takes
the bytes that remain (a decoder knows n and S, so there is no count field).  The C twin of split_chunks is linr_stream_split_chunks
(csrc/ac.cpp), which the decoder entries use.
"""

CHUNK_MIN, CHUNK_MAX = 64, 1 << 24
SIDE_BITS = 32                  # what the stream_chunk field of side_info.json is counted as in model_bpp / bpp_all


def check_chunk(chunk):
    """`chunk` as an int: 0 (off) or a valid S; anything else is a ValueError."""
    s = int(chunk or 0)
    if s != 0 and (s % 64 != 0 or not CHUNK_MIN <= s <= CHUNK_MAX):
        raise ValueError('stream_chunk must be 0 or a multiple of 64 in 64..2^24, got %r' % (chunk,))
    return s


def chunk_count(n, chunk):
    return 1 if chunk == 0 or n <= chunk else -(-n // chunk)


def chunk_entries(ns, chunk):
    """[(stream, first symbol, symbols)] of every chunk of streams with ns[i] symbols, stream by stream."""
    out = []
    for i, n in enumerate(ns):
        k = chunk_count(n, chunk)
        out += [(i, 0, n)] if k == 1 else [(i, j * chunk, min(chunk, n - j * chunk)) for j in range(k)]
    return out


def leb128(v):
    v = int(v)
    if not 0 <= v < 1 << 35:
        raise ValueError('a chunk length must fit 5 LEB128 bytes, got %d' % v)
    out = bytearray()
    while v >= 0x80:
        out.append((v & 0x7F) | 0x80)
        v >>= 7
    out.append(v)
    return bytes(out)


def read_leb128(data, pos):
    """(value, position behind it) of the varint at data[pos:]; ValueError for a truncated one or one of more than 5 bytes."""
    v = 0
    for b in range(5):
        if pos >= len(data):
            raise ValueError('truncated chunk length')
        byte = data[pos]
        pos += 1
        v |= (byte & 0x7F) << (7 * b)
        if not byte & 0x80:
            return v, pos
    raise ValueError('a chunk length of more than 5 bytes')


def join_chunks(chunks):
    """The stream of the coded chunks of one stage stream."""
    if len(chunks) == 1:
        return bytes(chunks[0])
    return b''.join([leb128(len(c)) for c in chunks[:-1]] + list(chunks))


def split_chunks(stream, n, chunk):
    """The coded chunks of a stage stream of n symbols; ValueError for a header that does not hold."""
    k = chunk_count(n, check_chunk(chunk))
    if k == 1:
        return [bytes(stream)]
    lens, pos = [], 0
    for _ in range(k - 1):
        v, pos = read_leb128(stream, pos)
        lens.append(v)
    if sum(lens) > len(stream) - pos:
        raise ValueError('the chunk lengths exceed the bytes of the stream')
    out = []
    for m in lens:
        out.append(bytes(stream[pos:pos + m]))
        pos += m
    out.append(bytes(stream[pos:]))
    return out

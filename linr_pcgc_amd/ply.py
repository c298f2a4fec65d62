"""Point-cloud file input of the data set (datautils/custom_dataset.py:9-14,263-269: `read_ply_o3d` / `np.load`):
x, y, z of a PLY (ascii, binary_little_endian or binary_big_endian; any extra vertex properties are skipped) or of an
.npy array, as an int64 [P, 3] array.  open3d is not needed.

And the output side of the decoder (datautils/custom_dataset.py:37-58): `format_ascii_device` turns decoded coordinates into the
text of an ASCII PLY on the GPU (csrc/ply_format.hip), `PlyWriter` writes such files on a background thread.

The input side has a device path too (csrc/ply_parse.hip): `read_points_device` / `read_many_device` parse the body of an ASCII or
binary PLY on the GPU and return CUDA tensors; whatever the device does not take goes through the host reader above."""
import queue
import threading

import numpy as np

ASCII_HEADER = 'ply\nformat ascii 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\nend_header\n'

_PLY_TYPES = {'char': 'i1', 'int8': 'i1', 'uchar': 'u1', 'uint8': 'u1', 'short': 'i2', 'int16': 'i2', 'ushort': 'u2',
              'uint16': 'u2', 'int': 'i4', 'int32': 'i4', 'uint': 'u4', 'uint32': 'u4', 'float': 'f4', 'float32': 'f4',
              'double': 'f8', 'float64': 'f8'}


def _read_header(f, path):
    """The header of the PLY opened (binary) as `f`, up to and including its end_header line: (format, vertex count, [(name, numpy
    type) of every vertex property]).  Raises ValueError for anything that is no PLY with an x / y / z vertex element."""
    if f.readline().strip() != b'ply':
        raise ValueError('%s is not a PLY file' % path)
    fmt, n_vertex, props, in_vertex = None, None, [], False
    while True:
        line = f.readline()
        if not line:
            raise ValueError('%s: PLY header is not terminated' % path)
        tok = line.decode('ascii', 'replace').split()
        if not tok or tok[0] == 'comment':
            continue
        if tok[0] == 'format':
            fmt = tok[1]
        elif tok[0] == 'element':
            in_vertex = tok[1] == 'vertex'
            if in_vertex:
                n_vertex = int(tok[2])
            elif n_vertex is None:
                raise ValueError('%s: an element precedes the vertex element' % path)
        elif tok[0] == 'property' and in_vertex:
            if tok[1] == 'list':
                raise ValueError('%s: list property in the vertex element' % path)
            props.append((tok[2], _PLY_TYPES[tok[1]]))
        elif tok[0] == 'end_header':
            break
    if fmt is None or n_vertex is None:
        raise ValueError('%s: no format / vertex element in the header' % path)
    names = [p[0] for p in props]
    if not all(k in names for k in ('x', 'y', 'z')):
        raise ValueError('%s: vertex element has no x / y / z' % path)
    return fmt, n_vertex, props


def _record_dtype(fmt, props):
    endian = '<' if fmt == 'binary_little_endian' else '>'
    return np.dtype([(n, endian + t) for n, t in props])


def _body_host(path, fmt, n_vertex, props, body):
    """The host reader behind the header: `body` holds the bytes behind end_header (ASCII: all of them; binary: up to n_vertex
    records) as bytes or as a uint8 numpy array."""
    if fmt == 'ascii':
        # the sequences of the data sets are ASCII: one pass of the library's host-side parser over the text (0.7 s -> tens of
        # milliseconds for a loot frame; the C call does not hold the GIL, so read_many scales over frames)
        import ctypes
        from . import _lib
        names = [p[0] for p in props]
        out = np.empty((n_vertex, 3), dtype=np.int64)
        done = ctypes.c_int64(0)
        cols = [names.index(k) for k in ('x', 'y', 'z')]
        text = body.ctypes.data if isinstance(body, np.ndarray) else body
        rc = _lib.lib().linr_ply_parse_ascii(text, len(body), n_vertex, len(names), cols[0], cols[1], cols[2],
                                             out.ctypes.data, ctypes.byref(done))
        if rc != 0:
            raise ValueError('%s: malformed vertex line %d (of %d announced)' % (path, done.value + 1, n_vertex))
        return out
    rec = np.frombuffer(body, dtype=_record_dtype(fmt, props), count=n_vertex)
    xyz = np.stack([rec['x'], rec['y'], rec['z']], axis=1)
    if xyz.shape[0] != n_vertex:
        raise ValueError('%s: %d vertices announced, %d read' % (path, n_vertex, xyz.shape[0]))
    return np.rint(xyz).astype(np.int64)


def read_ply_xyz(path):
    with open(path, 'rb') as f:
        fmt, n_vertex, props = _read_header(f, path)
        body = f.read() if fmt == 'ascii' else f.read(n_vertex * _record_dtype(fmt, props).itemsize)
    return _body_host(path, fmt, n_vertex, props, body)


def read_many(paths, workers=None):
    """The frames of a GOP, read and parsed on a thread pool (file reads and the C parser both release the GIL)."""
    import os
    from concurrent.futures import ThreadPoolExecutor
    paths = list(paths)
    if workers is None:
        try:
            workers = len(os.sched_getaffinity(0))
        except AttributeError:
            workers = os.cpu_count() or 1
    workers = max(1, min(int(workers), 16, len(paths)))
    if workers == 1:
        return [read_points(p) for p in paths]
    with ThreadPoolExecutor(max_workers=workers) as pool:
        return list(pool.map(read_points, paths))


def read_points(path):
    """`ori_type` 'ply' or 'npy' of the reference's data set, chosen by the file extension."""
    if str(path).lower().endswith('.npy'):
        return np.asarray(np.load(path))[:, :3].astype(np.int64)
    return read_ply_xyz(path)


# ---- the same frames parsed on the GPU (csrc/ply_parse.hip) ----------------------------------------------------------------------
_TYPE_CODES = {'i1': 0, 'u1': 1, 'i2': 2, 'u2': 3, 'i4': 4, 'u4': 5, 'f4': 6, 'f8': 7}


def _cuda_device(device):
    import torch
    dev = torch.device(device)
    if dev.type != 'cuda':
        raise TypeError('the device readers take a CUDA device, not %r (read_points / read_many are the host readers)' % (device,))
    return dev if dev.index is not None else torch.device('cuda', torch.cuda.current_device())


def _check_bytes(t, what):
    import torch
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.uint8 and t.dim() == 1):
        raise TypeError('%s takes a one-dimensional uint8 CUDA tensor' % what)
    return t if t.is_contiguous() and t.data_ptr() % 16 == 0 else t.clone()


def _launch_ascii(text, n_rows, n_cols, cols, status):
    """linr_ply_parse_ascii_device on the current stream: the int32 [n_rows, 3] result; `status` (2 int64 on the device) is read by
    the caller.  With n_rows == 0 nothing is launched and `status` stays as it is."""
    import ctypes
    import torch
    from . import _lib
    L = _lib.lib()
    xyz = torch.empty((n_rows, 3), dtype=torch.int32, device=text.device)
    ws_bytes = L.linr_ply_parse_ws_bytes(text.numel(), n_rows)
    if ws_bytes == 0:
        raise ValueError('a text of %d bytes is more than one call parses' % text.numel())
    with torch.cuda.device(text.device):
        ws = _lib.scratch(ws_bytes, text.device)
        _lib.check(L.linr_ply_parse_ascii_device(text.data_ptr(), text.numel(), n_rows, n_cols, cols[0], cols[1], cols[2],
                                                 xyz.data_ptr(), ws.data_ptr(), ws_bytes, status.data_ptr(),
                                                 ctypes.c_void_p(_lib.current_stream_handle())), 'linr_ply_parse_ascii_device')
    return xyz


def _launch_binary(rec, n_rows, stride, offsets, types, big_endian, status):
    import ctypes
    import torch
    from . import _lib
    xyz = torch.empty((n_rows, 3), dtype=torch.int32, device=rec.device)
    if rec.numel() < n_rows * stride:
        raise ValueError('%d records of %d bytes do not fit %d bytes' % (n_rows, stride, rec.numel()))
    i3 = ctypes.c_int32 * 3
    with torch.cuda.device(rec.device):
        _lib.check(_lib.lib().linr_ply_gather_binary(rec.data_ptr(), n_rows, stride, i3(*offsets), i3(*types), int(bool(big_endian)),
                                                     xyz.data_ptr(), status.data_ptr(),
                                                     ctypes.c_void_p(_lib.current_stream_handle())), 'linr_ply_gather_binary')
    return xyz


def parse_ascii_device(text, n_rows, n_cols, cols):
    """The body of an ASCII PLY (a uint8 CUDA tensor holding the bytes behind end_header) -> (xyz int32 CUDA [n_rows, 3], flags,
    first_row) of linr_ply_parse_ascii_device (include/linr_hip.h): columns `cols` = (x, y, z) of n_rows lines of n_cols numbers.
    flags == 0: every row was parsed on the device; otherwise an OR of _lib.LINR_PLY_* and the caller takes the bytes to the host
    parser.  One library call on the current stream and one host read (the status)."""
    text = _check_bytes(text, 'parse_ascii_device')
    import torch
    status = torch.tensor([0, 0], dtype=torch.int64).to(text.device) if int(n_rows) == 0 else \
        torch.empty(2, dtype=torch.int64, device=text.device)          # an empty frame launches nothing
    xyz = _launch_ascii(text, int(n_rows), int(n_cols), [int(c) for c in cols], status)
    flags, first_row = status.tolist()
    return xyz, flags, first_row


def gather_binary_device(rec, n_rows, stride, offsets, types, big_endian=False):
    """The records of a binary PLY (uint8 CUDA tensor, `stride` bytes each) -> (xyz int32 CUDA [n_rows, 3], flags, first_row) of
    linr_ply_gather_binary: the three fields at byte `offsets` with numpy type strings `types` ('i1' .. 'f8'), rounded like np.rint.
    flags is 0 or _lib.LINR_PLY_RANGE (a value that is not finite or outside int32)."""
    rec = _check_bytes(rec, 'gather_binary_device')
    import torch
    status = torch.tensor([0, 0], dtype=torch.int64).to(rec.device) if int(n_rows) == 0 else \
        torch.empty(2, dtype=torch.int64, device=rec.device)
    xyz = _launch_binary(rec, int(n_rows), int(stride), [int(o) for o in offsets], [_TYPE_CODES[t] for t in types], big_endian, status)
    flags, first_row = status.tolist()
    return xyz, flags, first_row


class _Frame:
    """One PLY on its way to the device: the header's fields and the body in a pinned host buffer."""
    __slots__ = ('path', 'fmt', 'n_vertex', 'props', 'nbytes', 'pinned')


def _load_body(path, slot):
    """Header parsed as by read_ply_xyz, body read straight into the slot's pinned buffer (slot = [tensor or None]; it grows)."""
    import os
    import torch
    fr = _Frame()
    fr.path = path
    with open(path, 'rb') as f:
        fr.fmt, fr.n_vertex, fr.props = _read_header(f, path)
        left = max(os.fstat(f.fileno()).st_size - f.tell(), 0)
        want = left if fr.fmt == 'ascii' else min(left, fr.n_vertex * _record_dtype(fr.fmt, fr.props).itemsize)
        if slot[0] is None or slot[0].numel() < want:
            slot[0] = torch.empty(max(want + want // 8, 1), dtype=torch.uint8, pin_memory=True)
        view = slot[0][:want].numpy()
        got = 0
        while got < want:
            k = f.readinto(view[got:])
            if not k:
                break
            got += k
    fr.nbytes, fr.pinned = got, slot[0][:got]
    return fr


def _issue(fr, device, status):
    """One H2D copy and the parse / gather of a loaded frame on the current stream -> int32 [n, 3], or None when only the host reader
    can say what the file holds (too few records, a text beyond 2^31 - 1 bytes)."""
    import torch
    names = [p[0] for p in fr.props]
    if fr.fmt == 'ascii':
        if fr.nbytes > 2 ** 31 - 1 or not 3 <= len(names) <= 64:
            return None
    else:
        dt = _record_dtype(fr.fmt, fr.props)
        if fr.nbytes < fr.n_vertex * dt.itemsize:
            return None
    if fr.n_vertex <= 0:
        return None if fr.n_vertex < 0 else torch.empty((0, 3), dtype=torch.int32, device=device)
    body = torch.empty(fr.nbytes, dtype=torch.uint8, device=device)
    body.copy_(fr.pinned, non_blocking=True)
    if fr.fmt == 'ascii':
        return _launch_ascii(body, fr.n_vertex, len(names), [names.index(k) for k in ('x', 'y', 'z')], status)
    return _launch_binary(body, fr.n_vertex, dt.itemsize, [dt.fields[k][1] for k in ('x', 'y', 'z')],
                          [_TYPE_CODES[dt.fields[k][0].str[1:]] for k in ('x', 'y', 'z')], fr.fmt != 'binary_little_endian', status)


_local = threading.local()


def read_points_device(path, device='cuda'):
    """read_points with the body parsed on the GPU: the frame as a CUDA [n, 3] tensor, int32.  The header is read as by read_ply_xyz,
    the body goes through a pinned buffer and one H2D copy into linr_ply_parse_ascii_device / linr_ply_gather_binary.  Whatever the
    device does not take (exponents, values beyond int32, malformed or short bodies) goes through the host reader on the same bytes:
    its values (int64 then) or its ValueError.  .npy files are loaded on the host as by read_points."""
    import torch
    dev = _cuda_device(device)
    if str(path).lower().endswith('.npy'):
        return torch.as_tensor(read_points(path), device=dev)
    with torch.cuda.device(dev):
        slot = _local.__dict__.setdefault('slot', [None])
        fr = _load_body(path, slot)
        status = torch.empty(2, dtype=torch.int64, device=dev)
        xyz = _issue(fr, dev, status)
        if xyz is not None and (fr.n_vertex == 0 or status.tolist()[0] == 0):
            return xyz
        return torch.as_tensor(_body_host(path, fr.fmt, fr.n_vertex, fr.props, fr.pinned.numpy()), device=dev)


def read_many_device(paths, device='cuda', workers=None, max_pending=4):
    """read_many for the GPU - PlyWriter mirrored: the files are read on a small thread pool into `max_pending` reused pinned buffers,
    copies and parses are issued in order on the caller's current stream, the statuses of all frames are read after ONE
    synchronisation and only the frames the device flagged are read again by the host reader.  Returns CUDA [n, 3] tensors in the
    order of `paths` (int32; int64 where the host reader stepped in)."""
    import collections
    import torch
    from concurrent.futures import ThreadPoolExecutor
    dev = _cuda_device(device)
    paths = list(paths)
    if max_pending < 1:
        raise ValueError('max_pending must be at least 1')
    if not paths:
        return []
    workers = max(1, min(int(workers if workers is not None else max_pending), 16, int(max_pending), len(paths)))
    out = [None] * len(paths)
    with torch.cuda.device(dev):
        index = dev.index
        stream = torch.cuda.current_stream()
        status = torch.zeros((len(paths), 2), dtype=torch.int64, device=dev)
        free = [{'buf': [None], 'copied': None} for _ in range(int(max_pending))]
        pending = collections.deque()

        def load(path, slot):
            if str(path).lower().endswith('.npy'):
                return None
            torch.cuda.set_device(index)          # a new thread starts on device 0
            if slot['copied'] is not None:
                slot['copied'].synchronize()      # the buffer's previous frame has left it
            return _load_body(path, slot['buf'])

        def drain():
            i, slot, fut = pending.popleft()
            try:
                fr = fut.result()
                if fr is None:
                    out[i] = torch.as_tensor(read_points(paths[i]), device=dev)
                else:
                    out[i] = _issue(fr, dev, status[i])
                    slot['copied'] = torch.cuda.Event()
                    slot['copied'].record(stream)
            finally:
                free.append(slot)

        with ThreadPoolExecutor(max_workers=workers) as pool:
            try:
                for i, path in enumerate(paths):
                    if not free:
                        drain()
                    slot = free.pop()
                    pending.append((i, slot, pool.submit(load, path, slot)))
                while pending:
                    drain()
            finally:
                for _, _, fut in pending:
                    fut.cancel()
        flags = status[:, 0].cpu().tolist()          # the one synchronisation
        for i, path in enumerate(paths):
            if out[i] is None or flags[i] != 0:
                out[i] = torch.as_tensor(read_points(path), device=dev)
    return out


def write_ply_xyz(path, xyz, binary=True):
    """Minimal writer (tests, exporting decoded frames): float x y z like open3d's write_point_cloud."""
    xyz = np.asarray(xyz, dtype=np.float32).reshape(-1, 3)
    header = 'ply\nformat %s 1.0\ncomment linr_pcgc_amd\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\nend_header\n' \
        % ('binary_little_endian' if binary else 'ascii', xyz.shape[0])
    with open(path, 'wb') as f:
        f.write(header.encode('ascii'))
        if binary:
            f.write(xyz.astype('<f4').tobytes())
        else:
            np.savetxt(f, xyz, fmt='%g')


def format_ascii_device(coords):
    """The body of write_ply_ascii's file for an integer CUDA [n, 3] tensor, as a uint8 CUDA tensor holding exactly the text:
    the bytes np.savetxt(fmt='%d') writes for the coordinates as int32.  One library call on the current stream and one host
    read (the length of the text)."""
    import ctypes
    import torch
    from . import _lib
    if not (isinstance(coords, torch.Tensor) and coords.is_cuda):
        raise TypeError('format_ascii_device takes a CUDA tensor')
    if coords.is_floating_point() or coords.is_complex() or coords.dtype == torch.bool:
        raise TypeError('format_ascii_device takes integer coordinates, not %s' % coords.dtype)
    xyz = coords.reshape(-1, 3).to(torch.int32).contiguous()
    n = int(xyz.shape[0])
    if n == 0:
        return torch.empty(0, dtype=torch.uint8, device=xyz.device)
    L = _lib.lib()
    cap, ws_bytes = L.linr_ply_format_text_bytes(n), L.linr_ply_format_ws_bytes(n)
    if cap == 0:
        raise ValueError('%d vertices are more than one call formats' % n)
    with torch.cuda.device(xyz.device):
        text = torch.empty(cap, dtype=torch.uint8, device=xyz.device)
        ws = _lib.scratch(ws_bytes, xyz.device)
        length = torch.empty(1, dtype=torch.int64, device=xyz.device)
        _lib.check(L.linr_ply_format_ascii(xyz.data_ptr(), n, text.data_ptr(), cap, ws.data_ptr(), ws_bytes, length.data_ptr(),
                                           ctypes.c_void_p(_lib.current_stream_handle())), 'linr_ply_format_ascii')
        return text[:int(length.item())]


class PlyWriter:
    """ASCII PLY files written off the thread that drives the GPU.  `submit` formats a frame on the current stream
    (format_ascii_device), copies the text into one of `max_pending` pinned host buffers and hands it to ONE background thread
    that writes the file; it blocks while all buffers are in use.  `close` (or leaving the `with` block) joins the thread and
    re-raises the first exception a write raised; files submitted after a failed write are not written."""

    def __init__(self, max_pending=2):
        if max_pending < 1:
            raise ValueError('max_pending must be at least 1')
        self.max_pending = int(max_pending)
        self.submitted = self.written = 0          # payloads accepted / payloads the thread is done with
        self._free = queue.Queue()
        for slot in range(self.max_pending):
            self._free.put(slot)
        self._pinned = [None] * self.max_pending
        self._jobs = queue.Queue()
        self._error = None
        self._thread = threading.Thread(target=self._run, name='PlyWriter', daemon=True)
        self._thread.start()

    def submit(self, path, coords):
        """Frame `coords` (an integer CUDA [n, 3] tensor) -> file `path`.  Returns once the text is on its way to a host buffer."""
        import torch
        text = format_ascii_device(coords)
        header = (ASCII_HEADER % (coords.numel() // 3)).encode('ascii')
        slot = self._take_slot()
        try:
            buf = self._pinned[slot]
            if buf is None or buf.numel() < text.numel():
                buf = self._pinned[slot] = torch.empty(max(text.numel(), 1), dtype=torch.uint8, pin_memory=True)
            view = buf[:text.numel()]
            view.copy_(text, non_blocking=True)
            ready = torch.cuda.Event()
            ready.record()          # the thread waits for the copy, not this one; `text` is reused in stream order
        except BaseException:
            self._free.put(slot)
            raise
        self._jobs.put((path, header, view.numpy(), slot, ready))

    def submit_bytes(self, path, header, payload):
        """The same queue for a payload that is already on the host (anything bytes-like): file = header + payload."""
        self._jobs.put((path, header, payload, self._take_slot(), None))

    def _take_slot(self):
        if self._thread is None:
            raise RuntimeError('PlyWriter is closed')
        slot = self._free.get()          # blocks while max_pending payloads are in flight
        self.submitted += 1
        return slot

    def _write(self, path, header, payload):
        with open(path, 'wb') as f:
            f.write(header)
            f.write(payload)

    def _run(self):
        while True:
            job = self._jobs.get()
            if job is None:
                return
            path, header, payload, slot, ready = job
            try:
                if self._error is None:
                    if ready is not None:
                        ready.synchronize()
                    self._write(path, header, payload)
            except BaseException as e:          # kept for close(); the queue keeps draining so that submit never hangs
                self._error = e
            finally:
                del job, payload
                self.written += 1
                self._free.put(slot)

    def close(self):
        if self._thread is not None:
            self._jobs.put(None)
            self._thread.join()
            self._thread = None
        if self._error is not None:
            e, self._error = self._error, None
            raise e

    def __enter__(self):
        return self

    def __exit__(self, exc_type, exc, tb):
        if exc_type is None:
            self.close()
        else:          # the caller's exception wins over a failed write
            try:
                self.close()
            except BaseException:
                pass
        return False

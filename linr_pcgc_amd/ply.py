"""Point-cloud file input of the data set (datautils/custom_dataset.py:9-14,263-269: `read_ply_o3d` / `np.load`):
x, y, z of a PLY (ascii, binary_little_endian or binary_big_endian; any extra vertex properties are skipped) or of an
.npy array, as an int64 [P, 3] array.  open3d is not needed.

And the output side of the decoder (datautils/custom_dataset.py:37-58): `format_ascii_device` turns decoded coordinates into the
text of an ASCII PLY on the GPU (csrc/ply_format.hip), `PlyWriter` writes such files on a background thread."""
import queue
import threading

import numpy as np

ASCII_HEADER = 'ply\nformat ascii 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\nend_header\n'

_PLY_TYPES = {'char': 'i1', 'int8': 'i1', 'uchar': 'u1', 'uint8': 'u1', 'short': 'i2', 'int16': 'i2', 'ushort': 'u2',
              'uint16': 'u2', 'int': 'i4', 'int32': 'i4', 'uint': 'u4', 'uint32': 'u4', 'float': 'f4', 'float32': 'f4',
              'double': 'f8', 'float64': 'f8'}


def read_ply_xyz(path):
    with open(path, 'rb') as f:
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
        if fmt == 'ascii':
            # the sequences of the data sets are ASCII: one pass of the library's host-side parser over the text (0.7 s -> tens of
            # milliseconds for a loot frame; the C call does not hold the GIL, so read_many scales over frames)
            import ctypes
            from . import _lib
            text = f.read()
            out = np.empty((n_vertex, 3), dtype=np.int64)
            done = ctypes.c_int64(0)
            cols = [names.index(k) for k in ('x', 'y', 'z')]
            rc = _lib.lib().linr_ply_parse_ascii(text, len(text), n_vertex, len(names), cols[0], cols[1], cols[2],
                                                 out.ctypes.data, ctypes.byref(done))
            if rc != 0:
                raise ValueError('%s: malformed vertex line %d (of %d announced)' % (path, done.value + 1, n_vertex))
            return out
        else:
            endian = '<' if fmt == 'binary_little_endian' else '>'
            dt = np.dtype([(n, endian + t) for n, t in props])
            rec = np.frombuffer(f.read(n_vertex * dt.itemsize), dtype=dt, count=n_vertex)
            xyz = np.stack([rec['x'], rec['y'], rec['z']], axis=1)
    if xyz.shape[0] != n_vertex:
        raise ValueError('%s: %d vertices announced, %d read' % (path, n_vertex, xyz.shape[0]))
    return np.rint(xyz).astype(np.int64)


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

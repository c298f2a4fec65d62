"""LINR_PCGC_Model: drop-in mirror of models/model_core.py on the MI355X engine.

Same constructor dict, same state_dict (189 tensors, reference order), same call surface
(``forward -> bits``, ``codec``, ``encode``, ``decode``).  All network arithmetic is in HIP kernels
(csrc/*.hip) behind include/linr_hip.h; this class owns the parameters (as views into ONE flat buffer, the layout
the kernels index), caches one kernel map + arena per coordinate set, and feeds the C++ range coder.

Two ways in:
  * reference-style: ``bits = model(putin_args)`` per scale, ``loss.backward()``, any torch optimiser
    (main.py:457-475,305-321) - autograd is bridged by ``_NetBits``;
  * fast path used by ``overfit.py`` / ``bench.py``: ``Frame`` with all scales batched + ``train_step`` (forward,
    backward and the fused Adam update without touching autograd).
"""
import ctypes
import time

import numpy as np
import torch
from torch import nn

from . import _lib, engine, ops
from .function_utils import pack_bitstream, unpack_bitstream
from .module_utils import BinaryArithmeticCoding, PointwiseMLP
from .stream_chunks import check_chunk, chunk_count, chunk_entries, join_chunks
from .upsample import CNP


class _NetBits(torch.autograd.Function):
    """bits(frame; params) with the hand-written backward of csrc/net.hip.  Parameter gradients are accumulated straight
    into the model's flat gradient buffer (the 189 ``.grad`` tensors are views of it)."""

    @staticmethod
    def forward(ctx, model, frame, *params):
        bits = torch.zeros(1, dtype=torch.float64, device=frame.device)
        engine.net_forward(frame, model._flat, 0, 8, None, bits)
        ctx.model, ctx.frame = model, frame
        return bits[0].to(torch.float32)

    @staticmethod
    def backward(ctx, gout):
        model, frame = ctx.model, ctx.frame
        tmp = torch.zeros_like(model._flat)
        engine.net_backward(frame, model._flat, tmp, 1.0)
        model._ensure_grad_views()
        model._flat_grad.addcmul_(tmp, gout.to(torch.float32).reshape(1).expand_as(tmp))
        return (None, None) + (None,) * len(model._plist)


class _WideBits(torch.autograd.Function):
    """The same for hidden_channel_conv = 16 / 32 (wide_net.py: forward with the activations kept, hand-written backward)."""

    @staticmethod
    def forward(ctx, model, frame, *params):
        bits = torch.zeros(1, dtype=torch.float64, device=frame.device)
        with torch.no_grad():
            ctx.tape = model._wide.forward(frame, 0, 8, None, bits, keep=True)
        ctx.model, ctx.frame = model, frame
        return bits[0].to(torch.float32)

    @staticmethod
    def backward(ctx, gout):
        model, frame = ctx.model, ctx.frame
        model._ensure_grad_views()
        keep = model._flat_grad.clone()                      # the wide backward WRITES the gradients: accumulate around it
        with torch.no_grad():
            model._flat_grad.zero_()
            if ctx.tape is not None:
                model._wide.backward(frame, ctx.tape, 1.0)
            model._flat_grad.mul_(gout.to(torch.float32).reshape(1)).add_(keep)
        return (None, None) + (None,) * len(model._plist)


class LINR_PCGC_Model(nn.Module):
    """models/model_core.py:19-37.  inargs: scale_num, in_channel (=7), hidden_channel_conv (=8), block_layers (1..4),
    outstage (=8), instage (=1).  outstage / instage / in_channel are hard-coded by the reference's drivers
    (main.py:97,218); block_layers is its live --block_layers flag (main.py:521: the Inception layers of block_in's
    ResNetBlock, with the extra skip of models/resnet.py:160-161 when > 1).  hidden_channel_conv (main.py:520): 8 runs on the
    tuned kernels (every one is specialised for 8-wide feature rows), 16 and 32 on the channel-blocked executor of wide_net.py."""

    def __init__(self, inargs):
        super().__init__()
        self.scale_num = int(inargs['scale_num'])
        if not 1 <= self.scale_num <= 16:
            raise ValueError('scale_num must be in 1..16 (the executor batches at most 16 scales per frame; the reference runs 6 to 8), '
                             'got %d' % self.scale_num)
        in_channel = int(inargs['in_channel'])
        hidden = int(inargs['hidden_channel_conv'])
        block_layers = int(inargs['block_layers'])
        if in_channel != 7 or inargs['outstage'] != 8 or inargs['instage'] != 1:
            raise ValueError('the gfx950 engine is specialised for in_channel=7, outstage=8, instage=1 (what main.py:97,218 '
                             'hard-code); got %r' % (inargs,))
        if hidden not in (8, 16, 32):
            raise ValueError('hidden_channel_conv=%d is not supported: 8 (the reference default, main.py:520) runs on the tuned '
                             'gfx950 kernels, 16 and 32 on the channel-blocked executor (wide_net.py); a checkpoint of another '
                             'width cannot be loaded' % hidden)
        self.hidden = hidden
        if not 1 <= block_layers <= 4:
            raise ValueError('block_layers must be in 1..4 (main.py:521 default 1), got %d' % block_layers)
        self.block_layers = block_layers
        self.scale_emb = nn.Embedding(self.scale_num, 8)
        self.scale_mlp = nn.ModuleList([PointwiseMLP([8 + in_channel, 16, 8]) for _ in range(self.scale_num)])
        self.upsampler = CNP(in_channels=8, channels=hidden, block_layers=block_layers, outstage=8, instage=1)
        self.sigmoid = nn.Sigmoid()
        self._flat = None
        self._flat_grad = None
        self._plist = []
        self._frame_cache = {}
        # inference numerics of frame_probs / codec / encode / decode: 'f32' (default) or 'bf16' = BASELINE config[4]'s bf16
        # features + uint8 weight codes (needs set_quantised, which the model codec calls)
        self.inference_precision = 'f32'
        # arithmetic of train_step: 'f32' (default, the headline) or 'bf16' = bf16 feature / gradient rows with fp32 master
        # parameters and accumulation (linr_net_train_step_bf16; hidden_channel_conv 8, block_layers 1)
        self.train_precision = 'f32'
        self._qcodes = None
        self._qrange = None
        self._wide = None
        if hidden != 8:
            from .wide_net import WideNet
            self._wide = WideNet(self, hidden)
        self._flatten()

    # ---- flat parameter buffer ------------------------------------------------------------------------------------
    def _lib_param_count(self):
        """The library's count of this model's parameters: the layout its whole-network entries index the flat buffer by."""
        L = _lib.lib()
        if self.hidden == 8:
            return L.linr_param_count(self.scale_num, self.block_layers)
        return L.linr_param_count_wide(self.scale_num, self.block_layers, self.hidden)

    def _flatten(self):
        """Re-home all parameters as views of one contiguous buffer in parameters() order (the kernels' layout)."""
        plist = list(self.parameters())
        total = sum(p.numel() for p in plist)
        if plist and plist[0].is_cuda and total != self._lib_param_count():
            raise _lib.LinrError('parameter layout mismatch with liblinr_hip.so')
        flat = torch.empty(total, dtype=torch.float32, device=plist[0].device)
        off = 0
        with torch.no_grad():
            for p in plist:
                n = p.numel()
                flat[off:off + n].copy_(p.detach().reshape(-1))
                p.data = flat[off:off + n].view(p.shape)
                p.grad = None
                off += n
        self._flat, self._plist, self._flat_grad = flat, plist, None
        self._frame_cache = {}
        if getattr(self, '_wide', None) is not None:
            self._wide._built = False                 # the parameter tensors were re-homed

    def _apply(self, fn, *args, **kwargs):
        # .cuda() / .to(device) / .cpu(): ONE conversion of the flat buffer and 189 new views instead of nn.Module's per-tensor
        # conversion followed by a second flattening (8.5 -> 3 ms per model; the drivers build three models per GOP).  Anything that
        # changes the dtype, and modules with buffers, take the general road.
        flat = None
        if self._flat is not None and not any(True for _ in self.buffers()):
            with torch.no_grad():
                flat = fn(self._flat)
            if flat.dtype != torch.float32 or flat.numel() != self._flat.numel() or not flat.is_contiguous():
                flat = None
        if flat is None:
            out = super()._apply(fn, *args, **kwargs)
            self._flatten()
            return out
        if flat.is_cuda and flat.numel() != self._lib_param_count():
            raise _lib.LinrError('parameter layout mismatch with liblinr_hip.so')
        off = 0
        with torch.no_grad():
            for q in self._plist:
                n = q.numel()
                q.data = flat[off:off + n].view(q.shape)
                q.grad = None
                off += n
        self._flat, self._flat_grad, self._frame_cache = flat, None, {}
        if self._qcodes is not None:
            self._qcodes = self._qcodes.to(flat.device)
        if getattr(self, '_wide', None) is not None:
            self._wide._built = False                 # the parameter tensors were re-homed
        return self

    def _ensure_grad_views(self):
        if self._flat_grad is None or self._flat_grad.device != self._flat.device:
            self._flat_grad = torch.zeros_like(self._flat)
        off = 0
        for p in self._plist:
            n = p.numel()
            if p.grad is None or p.grad.data_ptr() != self._flat_grad.data_ptr() + 4 * off:
                if p.grad is None:
                    self._flat_grad[off:off + n].zero_()        # zero_grad(set_to_none=True) semantics
                else:
                    self._flat_grad[off:off + n].copy_(p.grad.reshape(-1))
                p.grad = self._flat_grad[off:off + n].view(p.shape)
            off += n

    def set_quantised(self, codes, min_param, max_param):
        """The model as its uint8 codes of quant_uniform2 (model_compression/model_size_est.py:72-91): what model.bin holds.
        Called by Model_Estimate.compress_model / decompress_model next to the de-quantised fp32 fill."""
        if codes.numel() != self._flat.numel():
            raise ValueError('expected %d codes, got %d' % (self._flat.numel(), codes.numel()))
        self._qcodes = codes.to(device=self._flat.device, dtype=torch.uint8).contiguous()
        self._qrange = (float(min_param), float(max_param))

    def _precision(self, precision):
        precision = self.inference_precision if precision is None else precision
        if precision not in ('f32', 'bf16'):
            raise ValueError("precision must be 'f32' or 'bf16'")
        if precision == 'bf16' and self._qcodes is None:
            raise _lib.LinrError('the bf16 path runs from the 8-bit weight codes: quantise the model first, at bitdepth 8 '
                                 '(Model_Estimate.compress_model(model, 8, derive_new_model=True) / decompress_model)')
        return precision

    def flat_parameters(self):
        """The contiguous float32 buffer holding every parameter in parameters() order (what the model codec codes)."""
        return self._flat

    def qat_parameters(self):
        """The buffer the quantisation-aware train step writes the fake-quantised weights into (allocated on first use; it follows
        the flat buffer when the model moves)."""
        q = getattr(self, '_qat_flat', None)
        if q is None or q.device != self._flat.device or q.numel() != self._flat.numel():
            q = self._qat_flat = torch.empty_like(self._flat)
        return q

    # ---- frames ----------------------------------------------------------------------------------------------------
    def make_frame(self, scales, validate=True, with_arena=True):
        """Batched multi-scale frame for the fast path.  scales: list of per-scale input dicts (see engine.Frame)."""
        return engine.Frame(scales, self.scale_num, self._flat.device, validate, with_arena and self._wide is None, self.block_layers)

    def _scale_frame(self, d, need_occ=True):
        """Kernel map + arena for one scale's inputs.  Encoder-side inputs are cached by tensor identity; the cache
        entry pins the tensors so a recycled allocation can never alias a stale kernel map.  Decoder-side frames
        (fresh coordinates every call) are not cached."""
        coord = d['coord']
        s = {'coord': coord, 'offset_tensor': d.get('offset_tensor'), 'scale_idx': d['scale_idx']}
        if not need_occ:
            return self.make_frame([s])
        occ_lst, off = d.get('occ_lst'), d.get('offset_tensor')
        if occ_lst is None:                                  # the GOP drivers' lean dicts carry the matrix only (module_utils.prepare_frame)
            occ_lst = list(d['occ'].split(1, dim=1))
        occ0 = occ_lst[0]
        # identity AND shape of every input: slices of the cached tensors share their data pointers
        key = (coord.data_ptr(), tuple(coord.shape), int(d['scale_idx']), None if off is None else (off.data_ptr(), tuple(off.shape)),
               occ0.data_ptr(), len(occ_lst), tuple(tuple(o.shape) for o in occ_lst))
        hit = self._frame_cache.get(key)
        if hit is None:
            if len(self._frame_cache) >= 1024:
                self._frame_cache.pop(next(iter(self._frame_cache)))
            s['occ_lst'] = occ_lst
            hit = (self.make_frame([s]), coord, off, list(occ_lst))
            self._frame_cache[key] = hit
        return hit[0]

    # ---- reference call surface --------------------------------------------------------------------------------------
    def forward(self, inargs):
        """models/model_core.py:72-81: bits of one scale (0-dim float32, differentiable w.r.t. the parameters)."""
        if int(inargs['coord'].shape[0]) == 0:          # a scale without voxels costs nothing (and has nothing to differentiate)
            return self._flat.sum() * 0.0
        frame = self._scale_frame(inargs)
        if torch.is_grad_enabled() and any(p.requires_grad for p in self._plist):
            return (_WideBits if self._wide is not None else _NetBits).apply(self, frame, *self._plist)
        bits = torch.zeros(1, dtype=torch.float64, device=frame.device)
        self._stage_forward(frame, 0, 8, None, bits, 'f32')
        return bits[0].to(torch.float32)

    def _stage_forward(self, frame, k0, k1, probs, bits, precision):
        if self._wide is not None:
            with torch.no_grad():
                if self._wide.c_forward and (k0, k1) == (0, 8):
                    # the full-range inference forward as one C call (csrc/wide_fwd.hip); stage ranges - decode_frame's loop - stay on
                    # the Python schedule, the same launches
                    self._wide.forward_c(frame, probs, bits, precision == 'bf16')
                elif precision == 'bf16':          # csrc/wide_bf16.hip: the uint8 codes as the model, bf16 activations
                    self._wide.forward_bf16(frame, k0, k1, probs, bits)
                else:
                    self._wide.forward(frame, k0, k1, probs, bits)
        elif precision == 'bf16':
            engine.net_forward_bf16(frame, self._qcodes, self._qrange[0], self._qrange[1], k0, k1, probs, bits)
        else:
            engine.net_forward(frame, self._flat, k0, k1, probs, bits)

    @torch.no_grad()
    def frame_probs(self, frame, precision=None):
        """One inference forward over a (possibly multi-scale) frame: probs float32 [8, rows], bits float64[1]."""
        probs = torch.empty((8, frame.rows), dtype=torch.float32, device=frame.device)
        bits = torch.zeros(1, dtype=torch.float64, device=frame.device)
        self._stage_forward(frame, 0, 8, probs, bits, self._precision(precision))
        return probs, bits

    @torch.no_grad()
    def frame_codes(self, frame, precision=None, out=None):
        """frame_probs, then the range coder's inputs on the GPU (linr_ac_codes, csrc/ac_codes.hip) on the current stream:
        c1 uint16 [8, rows], the code value of every probability; sym uint32 [8, words], the occupancy as bit planes; bits float64[1].
        The coder cuts a frame into per-scale streams and the scales' row offsets are no multiples of 32, so every scale gets words of
        its own: scale i's symbols are bits 0 .. n_i - 1 of the words from codes_word_off(frame.row_off)[i] on (one launch per scale).
        out=(c1, sym): contiguous tensors of those shapes and types to write into (a frame's part of a group-wide buffer)."""
        probs, bits = self.frame_probs(frame, precision)
        woff = codes_word_off(frame.row_off)
        rows, words = frame.rows, int(woff[-1])
        if out is None:
            c1 = torch.empty((8, rows), dtype=torch.uint16, device=frame.device)
            sym = torch.empty((8, words), dtype=torch.uint32, device=frame.device)
        else:
            c1, sym = out
            if (c1.dtype, tuple(c1.shape), sym.dtype, tuple(sym.shape)) != (torch.uint16, (8, rows), torch.uint32, (8, words)) or \
                    not (c1.is_contiguous() and sym.is_contiguous()):
                raise ValueError('frame_codes: out must be contiguous uint16 [8, %d] and uint32 [8, %d]' % (rows, words))
        L, st = _lib.lib(), _lib.current_stream_handle()
        for i in range(frame.n_scales):
            a, n = int(frame.row_off[i]), int(frame.row_off[i + 1] - frame.row_off[i])
            if n:
                _lib.check(L.linr_ac_codes(probs.data_ptr() + 4 * a, rows, frame.occ.data_ptr() + 32 * a, 8, n, c1.data_ptr() + 2 * a, rows,
                                           sym.data_ptr() + 4 * int(woff[i]), words, st), 'linr_ac_codes')
        return c1, sym, bits

    @torch.no_grad()
    def codec(self, inargs):
        """models/model_core.py:169-227: one forward, the 8 stages as ONE arithmetic-coded stream, timed enc/dec."""
        st1 = time.time()
        frame = self._scale_frame(inargs)
        probs, bits_t = self.frame_probs(frame)
        p_host = probs.reshape(-1).cpu()
        sym = frame.occ.t().contiguous().reshape(-1).to(torch.int16).cpu()
        bac = BinaryArithmeticCoding()
        st2 = time.time()
        enc_bytes = bac.encode(p_host, sym)
        st3 = time.time()
        recon = bac.decode(p_host, enc_bytes)
        st4 = time.time()
        assert bool((recon == sym).all())
        return {'bits': len(enc_bytes) * 8, 'enc_bytes': enc_bytes, 'enc_time': st3 - st1,
                'dec_time': (st2 - st1) + (st4 - st3), 'bits_t': bits_t[0].to(torch.float32)}

    @torch.no_grad()
    def encode(self, in_args, DBG=False):
        """models/model_core.py:235-266 + CNP.encode (models/upsample.py:219-246): 8 per-stage streams, packed."""
        frame = self._scale_frame(in_args)
        probs, _ = self.frame_probs(frame)
        p_host = probs.cpu().numpy()
        occ_host = frame.occ.t().contiguous().cpu().numpy().astype(np.uint8)
        chunk = check_chunk(in_args.get('stream_chunk', 0))          # opt-in chunked stage streams (stream_chunks); width 8 only
        if chunk and self._wide is not None:
            raise ValueError('stream_chunk needs hidden_channel_conv 8: the widths 16 and 32 decode stage-wise in Python, without chunks')
        streams = encode_streams([p_host[k] for k in range(8)], [occ_host[k] for k in range(8)], chunk=chunk)
        if DBG and not chunk:
            bac = BinaryArithmeticCoding()
            for k in range(8):
                assert (bac.decode(p_host[k], streams[k]).numpy() == occ_host[k]).all()
        enc_bytes = pack_bitstream(streams)
        return {'enc_bytes': enc_bytes, 'bits': len(enc_bytes) * 8, 'x_low': None}

    @torch.no_grad()
    def decode(self, inagrs):
        """models/model_core.py:268-286 + CNP.decode (models/upsample.py:249-295): stage-serial, the SAME launches as
        the encoder's forward, so probabilities are bitwise identical.  Returns 8 x [N,1] float32 occupancy."""
        streams = unpack_bitstream(inagrs['enc_bytes'])
        s = {'coord': inagrs['coord'], 'offset_tensor': inagrs.get('offset_tensor'), 'scale_idx': inagrs['scale_idx']}
        # decoder-side frames are never cached (fresh coordinates every call); the bf16 path brings its own small arena
        frame = self.make_frame([s], with_arena=self._precision(None) == 'f32')
        return self.decode_frame(frame, [streams])

    def _decode_scale_args(self, size_fn, size_args, coord, streams, chunk, n_threads, device_entries=None):
        """What decode_scale and decode_scale_batch hand their C entry alike, in the entries' order: (params, codes, lo, hi, stream
        pointers, stream lengths, aligned workspace, its bytes, pinned probabilities, pinned symbols, child buffer, its rows), the
        options (LinrDecodeOpts), the workspace bytes (size_fn(*size_args, block_layers, bf16, stream bytes, entries, and for the
        widths 16 / 32 - the _wide entries - hidden); 0: the entry refuses the size, nothing else is returned) and the objects that own
        that memory, child buffer first: keep them until the call has returned.
        device_entries = the table entries of the scale: the device decoders, whose workspace also holds the streams' bytes and that
        many entries, and which take no pinned buffers (None in their place); None: the host decoders."""
        n = int(coord.shape[0])
        ptrs, lens, bufs = engine.stream_arrays(streams)
        bf16 = self._precision(None) == 'bf16'
        device = device_entries is not None
        extra = (sum(len(b) for b in streams), int(device_entries)) if device else (-1, 0)
        need = size_fn(*size_args, self.block_layers, 1 if bf16 else 0, *extra, *self._width_arg())
        if need == 0:
            return None, None, 0, None
        ws = _lib.scratch(need + 256, coord.device)
        child = torch.empty((8 * n, 3), dtype=torch.int32, device=coord.device)
        pinned = (None, None) if device else tuple(b.data_ptr() for b in self._host_buffers(n))
        codes, lo, hi, params = (self._qcodes.data_ptr(), float(self._qrange[0]), float(self._qrange[1]), None) if bf16 else \
            (None, 0.0, 0.0, self._flat.data_ptr())
        opts = _lib.LinrDecodeOpts(int(chunk), int(n_threads), 1 if device else 0)
        return (params, codes, lo, hi, ptrs, lens, (ws.data_ptr() + 255) & ~255, need, *pinned,
                child.data_ptr(), 8 * n), opts, need, (child, ws, bufs)

    def _width_arg(self):
        """What the _wide twin of a decoder entry takes behind the plain entry's arguments: (hidden,) for the widths 16 / 32."""
        return () if self._wide is None else (self.hidden,)

    @torch.no_grad()
    def decode_scale(self, coord, scale_idx, enc_bytes, child_bits, chunk=0, n_threads=1, device_decoder=False):
        """One scale of decoder.decode_one_frame (decoder.py:153-176) as ONE C call that does not hold the GIL
        (linr_decode_scale; hidden_channel_conv 16 / 32: linr_decode_scale_wide, the same scale on the wide C forward): kernel map
        of `coord` (int32 [n,3] on the GPU, sorted x-major), the 8 decode stages against the packed stream `enc_bytes`,
        octree_level.upper_layer.  Returns the next finer level's coordinates (int32 [m,3]).
        chunk = S > 0: the stage streams are chunked (stream_chunks) and a stage's chunks are decoded on `n_threads` host threads
        (linr_decode_opts.chunk_symbols, n_threads).
        device_decoder=True (opt-in): the range decoders run on the GPU, a wave per stream or chunk, from the probabilities where the
        stage forward left them (linr_decode_opts.device): no host round trip per stage, one synchronisation per scale; n_threads is
        ignored.  The streams and the result are the same."""
        L = _lib.lib()
        n = int(coord.shape[0])
        if n == 0:
            return coord.new_zeros((0, 3))
        coord = coord.contiguous()
        entries = 8 * chunk_count(n, int(chunk)) if device_decoder else None
        size_fn, entry = (L.linr_decode_scale_ws_bytes, L.linr_decode_scale) if self._wide is None else \
            (L.linr_decode_scale_wide_ws_bytes, L.linr_decode_scale_wide)
        shared, opts, need, keep = self._decode_scale_args(size_fn, (n,), coord, unpack_bitstream(enc_bytes), chunk, n_threads, entries)
        if need == 0:
            raise ValueError('linr_decode_scale has no workspace for %d rows at block_layers %d' % (n, self.block_layers))
        m = ctypes.c_int64(0)
        _lib.check(entry(coord.data_ptr(), n, int(scale_idx), self.scale_num, self.block_layers, int(child_bits), *shared,
                         ctypes.byref(m), ctypes.byref(opts), *self._width_arg(), torch.cuda.current_stream().cuda_stream),
                   'linr_decode_scale')
        return keep[0][:m.value]

    @torch.no_grad()
    def decode_scale_batch(self, coords_list, scale_idx, enc_bytes_list, n_threads=8, chunk=0, device_decoder=False):
        """decode_scale for several frames in lock step as ONE C call (linr_decode_scale_batch): the frames' levels `coords_list`
        (int32 [n_i,3] on the GPU, each sorted x-major) are one row space whose kernel map never links two frames, every decode stage
        is one launch set and one copy each way for all of them, their range decoders run on `n_threads` host threads, and the
        children come from prefix sums instead of a sort.  Returns the list of the next finer levels' coordinates (int32 [m_i,3]).
        chunk = S > 0: the stage streams are chunked (stream_chunks; linr_decode_opts.chunk_symbols).
        device_decoder=True (opt-in): as in decode_scale - every stream or chunk of the group's frames a wave of one launch per stage
        (linr_decode_opts.device); n_threads is ignored."""
        L = _lib.lib()
        nf = len(coords_list)
        if nf < 1 or nf > 64 or len(enc_bytes_list) != nf:
            raise ValueError('decode_scale_batch takes 1 to 64 frames and one packed stream per frame')
        seg = np.zeros(nf + 1, dtype=np.int64)
        seg[1:] = np.cumsum([int(c.shape[0]) for c in coords_list])
        n = int(seg[-1])
        if n == 0:
            return [c.new_zeros((0, 3)) for c in coords_list]
        coord = torch.cat(coords_list, dim=0).contiguous() if nf > 1 else coords_list[0].contiguous()
        streams = [b for e in enc_bytes_list for b in unpack_bitstream(e)]
        if len(streams) != 8 * nf:
            raise ValueError('every frame needs the 8 stage streams of the scale')
        entries = 8 * sum(chunk_count(int(c.shape[0]), int(chunk)) for c in coords_list if c.shape[0]) if device_decoder else None
        size_fn, entry = (L.linr_decode_scale_batch_ws_bytes, L.linr_decode_scale_batch) if self._wide is None else \
            (L.linr_decode_scale_batch_wide_ws_bytes, L.linr_decode_scale_batch_wide)
        shared, opts, need, keep = self._decode_scale_args(size_fn, (n, nf), coord, streams, chunk, n_threads, entries)
        if need == 0:
            raise ValueError('%d rows in one decode group: the bound is 2^26 - 64' % n)
        off = (ctypes.c_int64 * (nf + 1))()
        _lib.check(entry(coord.data_ptr(), seg.ctypes.data, nf, int(scale_idx), self.scale_num, self.block_layers,
                         *shared, off, ctypes.byref(opts), *self._width_arg(), torch.cuda.current_stream().cuda_stream),
                   'linr_decode_scale_batch')
        self._lockstep_ws_peak = max(getattr(self, '_lockstep_ws_peak', 0), int(need))
        return [keep[0][off[i]:off[i + 1]] for i in range(nf)]

    def _host_buffers(self, rows):
        """Pinned staging buffers of the staged decoder (probabilities down, decoded symbols up), grown on demand."""
        import threading
        tls = self.__dict__.setdefault('_dec_tls', threading.local())          # one pair per decoding thread
        buf = getattr(tls, 'buf', None)
        if buf is None or buf[0].numel() < rows:
            cap = max(rows, 1 << 16)
            buf = (torch.empty(cap, dtype=torch.float32, pin_memory=True), torch.empty(cap, dtype=torch.uint8, pin_memory=True))
            tls.buf = buf
        return buf

    @torch.no_grad()
    def decode_frame(self, frame, streams_per_scale, precision=None):
        """Staged decode of every scale of `frame` at once: stage k of all scales is one launch set.  Host side per
        stage: one D2H of the probabilities into pinned memory, linr_ac_decode_binary per scale straight on those
        buffers, one H2D of the decoded byte column (no torch CPU ops: they fan out over every host core)."""
        frame.occ.zero_()
        frame.invalidate_occ()
        rows = frame.rows
        probs = torch.empty((8, rows), dtype=torch.float32, device=frame.device)
        s_dev = torch.empty(max(rows, 1), dtype=torch.uint8, device=frame.device)
        p_host, s_host = self._host_buffers(rows)
        precision = self._precision(precision)
        if self._wide is not None:          # stage loop in Python: stage forward, D2H, range decoder, H2D
            L = _lib.lib()
            for k in range(8):
                self._stage_forward(frame, k, k + 1, probs, None, precision)
                p_host[:rows].copy_(probs[k])
                for i in range(frame.n_scales):
                    r0, r1 = int(frame.row_off[i]), int(frame.row_off[i + 1])
                    if r1 == r0:
                        continue
                    buf = np.frombuffer(streams_per_scale[i][k], dtype=np.uint8)
                    _lib.check(L.linr_ac_decode_binary(ctypes.c_void_p(p_host.data_ptr() + 4 * r0), r1 - r0,
                                                       ctypes.c_void_p(buf.ctypes.data if buf.size else None), int(buf.size),
                                                       ctypes.c_void_p(s_host.data_ptr() + r0)), 'linr_ac_decode_binary')
                frame.occ[:, k].copy_(s_host[:rows].to(frame.device, torch.float32))
            return [frame.occ[:, k:k + 1].clone() for k in range(8)]
        # the whole stage loop is one C call (csrc/decode.hip: linr_net_decode_stages): no Python between the stages, no GIL held
        if precision == 'bf16':
            engine.net_decode_stages(frame, None, streams_per_scale, probs, p_host, s_host, s_dev, self._qcodes, self._qrange)
        else:
            engine.net_decode_stages(frame, self._flat, streams_per_scale, probs, p_host, s_host, s_dev)
        return [frame.occ[:, k:k + 1].clone() for k in range(8)]


def _code_entries(ns, chunk, in_a, in_b, entry, n_threads, what):
    """The streams of ns[i] symbols through a batch entry of the host coder (`entry`), every chunk (stream_chunks; chunk 0: every
    stream) as an entry of its own.  in_a / in_b = (the streams' input arrays, bytes per 64 symbols): a chunk starts at a multiple
    of 64 symbols, so its inputs start that many bytes into them.  The chunks are handed over longest first - the full chunks of the
    finest scales, then the tails and the coarse scales - and the coder threads take them in that order, so all chunks of a frame
    balance across them.  The tables are built with numpy: this runs under the GIL, beside the thread that launches the forwards.
    Returns the streams, chunks joined."""
    ns = np.asarray(ns, dtype=np.int64).reshape(-1)
    k = np.maximum(1, -(-ns // chunk)) if chunk else np.ones(len(ns), dtype=np.int64)
    first = np.zeros(len(ns) + 1, dtype=np.int64)
    first[1:] = np.cumsum(k)
    n = int(first[-1])
    stream = np.repeat(np.arange(len(ns)), k)
    start = (np.arange(n) - first[stream]) * chunk
    m = np.minimum(ns[stream] - start, chunk) if chunk else ns.copy()
    order = np.argsort(-m, kind='stable') if chunk else np.arange(n)          # stable: equal lengths keep the order of the streams
    cap = 2 * m + 64
    off = np.cumsum(cap) - cap
    out = np.empty(int(cap.sum()), dtype=np.uint8)
    blocks = start[order] // 64
    ptr = [np.asarray([x.ctypes.data for x in arrays], dtype=np.int64)[stream[order]] + per64 * blocks for arrays, per64 in (in_a, in_b)]
    arr_o = out.ctypes.data + off[order]
    arr_n, arr_c = np.ascontiguousarray(m[order]), np.ascontiguousarray(cap[order])
    arr_l = np.empty(n, dtype=np.int64)
    _lib.check(entry(ptr[0].ctypes.data, ptr[1].ctypes.data, arr_n.ctypes.data, n, arr_o.ctypes.data, arr_c.ctypes.data, arr_l.ctypes.data,
                     n_threads), what)
    lens = np.empty(n, dtype=np.int64)
    lens[order] = arr_l
    view, off, lens, first = memoryview(out), off.tolist(), lens.tolist(), first.tolist()
    return [join_chunks([view[off[e]:off[e] + lens[e]] for e in range(first[i], first[i + 1])]) for i in range(len(ns))]


def encode_streams(probs, symbols, n_threads=8, chunk=0):
    """Codes independent binary streams on a host thread pool (linr_ac_encode_binary_batch).  chunk = S > 0 (stream_chunks): a stream
    of more than S symbols is coded as chunks of S symbols, each an entry of the batch, and comes back as header + chunks."""
    chunk = check_chunk(chunk)
    probs = [np.ascontiguousarray(p, dtype=np.float32).reshape(-1) for p in probs]
    symbols = [np.ascontiguousarray(s, dtype=np.uint8).reshape(-1) for s in symbols]
    return _code_entries([p.size for p in probs], chunk, (probs, 256), (symbols, 64), _lib.lib().linr_ac_encode_binary_batch, n_threads,
                         'linr_ac_encode_binary_batch')


def decode_streams(probs, streams, n_threads=8, chunk=0):
    """The twin of encode_streams: stream i decoded against probs[i] (float32 [n_i]) into uint8 [n_i], on a host thread pool
    (linr_ac_decode_binary_batch).  chunk = S > 0: the streams are cut by the checked parser (linr_stream_split_chunks: a header that
    does not hold raises LinrError, nothing is decoded) and every chunk is an entry of the batch, as in the decoder's scale entries."""
    chunk = check_chunk(chunk)
    L = _lib.lib()
    probs = [np.ascontiguousarray(p, dtype=np.float32).reshape(-1) for p in probs]
    bufs = [np.frombuffer(b, dtype=np.uint8) for b in streams]
    syms = [np.empty(p.size, dtype=np.uint8) for p in probs]
    ks = [chunk_count(p.size, chunk) for p in probs]
    n = sum(ks)
    arr_in, arr_len = (ctypes.c_void_p * n)(), (ctypes.c_int64 * n)()
    at = 0
    for p, b, k in zip(probs, bufs, ks):
        got = L.linr_stream_split_chunks(b.ctypes.data if b.size else None, int(b.size), p.size, chunk,
                                         ctypes.byref(arr_in, at * ctypes.sizeof(ctypes.c_void_p)),
                                         ctypes.byref(arr_len, at * ctypes.sizeof(ctypes.c_int64)), k)
        if got != k:
            _lib.check(int(got), 'linr_stream_split_chunks')
        at += k
    entries = chunk_entries([p.size for p in probs], chunk)
    arr_p = (ctypes.c_void_p * n)(*[probs[i].ctypes.data + 4 * a for i, a, _ in entries])
    arr_s = (ctypes.c_void_p * n)(*[syms[i].ctypes.data + a for i, a, _ in entries])
    arr_n = (ctypes.c_int64 * n)(*[e[2] for e in entries])
    _lib.check(L.linr_ac_decode_binary_batch(arr_p, arr_n, arr_in, arr_len, n, arr_s, n_threads), 'linr_ac_decode_binary_batch')
    return syms


def codes_word_off(row_off):
    """Word offsets of the scales' symbol bit planes in what frame_codes returns: scale i owns ceil(n_i / 32) words."""
    n = np.diff(np.asarray(row_off, dtype=np.int64))
    off = np.zeros(len(n) + 1, dtype=np.int64)
    off[1:] = np.cumsum((n + 31) // 32)
    return off


def encode_streams_codes(c1s, syms, ns, n_threads=8, chunk=0):
    """encode_streams from code values and symbol bit planes (linr_ac_encode_binary_codes_batch): stream i has ns[i] symbols,
    c1s[i] uint16 [>= ns[i]], syms[i] uint32 [>= ceil(ns[i] / 32)], bit j & 31 of word j >> 5 = symbol j.  chunk = S > 0: chunk j of a
    stream reads its code values from j S and its symbol words from j S / 32 on (S is a multiple of 64)."""
    chunk = check_chunk(chunk)
    ns = [int(v) for v in ns]
    c1s = [np.ascontiguousarray(c, dtype=np.uint16).reshape(-1) for c in c1s]
    syms = [np.ascontiguousarray(w, dtype=np.uint32).reshape(-1) for w in syms]
    if any(c.size < m or w.size < (m + 31) // 32 for c, w, m in zip(c1s, syms, ns)):
        raise ValueError('a stream has fewer code values or symbol words than symbols')

    return _code_entries(ns, chunk, (c1s, 128), (syms, 8), _lib.lib().linr_ac_encode_binary_codes_batch, n_threads,
                         'linr_ac_encode_binary_codes_batch')


class DeviceCoderSet:
    """One buffer set of the device range coder (linr_rc_encode_codes, csrc/ac_device.hip): stream regions, lengths, the dense payload
    and its offsets on the device, pinned copies of the last two, and a stream of its own for the two small reads a call needs, so
    that reading one set never queues behind the coding of another.  launch() on the current stream, collect() anywhere later.
    chunk = S > 0 (stream_chunks): linr_rc_encode_codes_chunked, a wave per chunk; total_cap and n_chunks are then those of
    table(descriptors, S) and chunks(descriptors, S)."""

    def __init__(self, n_streams, total_cap, device, chunk=0, n_chunks=0):
        L = _lib.lib()
        self.chunk = check_chunk(chunk)
        self.n_max, self.cap_max = int(n_streams), max(8, int(total_cap))
        self.chunks_max = max(int(n_chunks), self.n_max) if self.chunk else 0
        # the final bytes of a chunked stream: at most its region and a header of 5 bytes per further chunk
        self.payload_max = self.cap_max + 5 * max(0, self.chunks_max - self.n_max)
        self.out = torch.empty(self.cap_max, dtype=torch.uint8, device=device)
        self.payload = torch.empty(self.payload_max, dtype=torch.uint8, device=device)
        self.len = torch.empty(self.n_max, dtype=torch.int64, device=device)
        self.offsets = torch.empty(self.n_max + 1, dtype=torch.int64, device=device)
        self.ws = _lib.scratch(L.linr_rc_encode_chunked_ws_bytes(self.n_max, self.chunks_max) if self.chunk else
                               L.linr_rc_encode_ws_bytes(self.n_max, self.cap_max), device)
        self.offsets_pin = torch.empty(self.n_max + 1, dtype=torch.int64, pin_memory=True)
        self.payload_pin = torch.empty(self.payload_max, dtype=torch.uint8, pin_memory=True)
        self.read_stream = torch.cuda.Stream(device=device)
        self.coded, self.read = torch.cuda.Event(), torch.cuda.Event()
        self.n = 0

    @staticmethod
    def chunks(descriptors, chunk=0):
        """The chunks of all streams of rows {c1 offset, symbol word offset, n} together."""
        return sum(chunk_count(int(n), chunk) for n in np.asarray(descriptors, dtype=np.int64).reshape(-1, 3)[:, 2])

    @staticmethod
    def table(descriptors, chunk=0):
        """int64 [n, 5] rows {c1 offset, symbol word offset, n, out offset, cap} from rows {c1 offset, symbol word offset, n}: cap is the
        host path's 2 n + 64 - with chunk = S > 0 that of every chunk, 2 n + 64 k together -, the regions follow each other on 4-byte
        boundaries.  Returns (table, bytes of all regions)."""
        d = np.asarray(descriptors, dtype=np.int64).reshape(-1, 3)
        tab = np.empty((len(d), 5), dtype=np.int64)
        tab[:, :3] = d
        k = np.maximum(1, -(-d[:, 2] // chunk)) if chunk else 1
        tab[:, 4] = 2 * d[:, 2] + 64 * k
        ends = np.cumsum((tab[:, 4] + 3) & ~3)
        tab[:, 3] = ends - ((tab[:, 4] + 3) & ~3)
        return tab, int(ends[-1]) if len(d) else 0

    def launch(self, c1, sym, descriptors):
        """Codes the streams {c1 element offset, symbol word offset, n} of c1 (uint16) / sym (uint32) on the current stream."""
        tab, total = self.table(descriptors, self.chunk)
        n = len(tab)
        if n == 0 or n > self.n_max or total > self.cap_max:
            raise ValueError('DeviceCoderSet: %d streams / %d bytes in a set made for %d / %d' % (n, total, self.n_max, self.cap_max))
        if self.chunk and self.chunks(descriptors, self.chunk) > self.chunks_max:
            raise ValueError('DeviceCoderSet: more chunks than the set was made for (%d)' % self.chunks_max)
        if c1.dtype != torch.uint16 or sym.dtype != torch.uint32 or not (c1.is_contiguous() and sym.is_contiguous()):
            raise ValueError('DeviceCoderSet: c1 must be contiguous uint16, sym contiguous uint32')
        if (tab[:, :3] < 0).any() or (tab[:, 0] + tab[:, 2] > c1.numel()).any() or (tab[:, 1] + (tab[:, 2] + 31) // 32 > sym.numel()).any():
            raise ValueError('DeviceCoderSet: a stream reads outside c1 or sym')
        L = _lib.lib()
        if self.chunk:
            _lib.check(L.linr_rc_encode_codes_chunked(c1.data_ptr(), sym.data_ptr(), tab.ctypes.data, n, self.chunk, self.out.data_ptr(),
                                                      self.out.numel(), self.len.data_ptr(), self.payload.data_ptr(), self.payload.numel(),
                                                      self.offsets.data_ptr(), self.ws.data_ptr(), self.ws.numel(),
                                                      _lib.current_stream_handle()), 'linr_rc_encode_codes_chunked')
        else:
            _lib.check(L.linr_rc_encode_codes(c1.data_ptr(), sym.data_ptr(), tab.ctypes.data, n, self.out.data_ptr(), self.out.numel(),
                                              self.len.data_ptr(), self.payload.data_ptr(), self.payload.numel(), self.offsets.data_ptr(),
                                              self.ws.data_ptr(), self.ws.numel(), _lib.current_stream_handle()), 'linr_rc_encode_codes')
        self.coded.record(torch.cuda.current_stream())
        with torch.cuda.stream(self.read_stream):
            self.read_stream.wait_event(self.coded)
            self.offsets_pin[:n + 1].copy_(self.offsets[:n + 1], non_blocking=True)
            self.read.record(self.read_stream)
        self.n = n

    def collect(self):
        """The streams of the last launch as a list of bytes: waits for it, reads payload[:total]."""
        n = self.n
        self.read.synchronize()
        offs = self.offsets_pin[:n + 1].numpy().copy()
        total = int(offs[-1])
        if (np.diff(offs) < 1).any() or total > self.payload_max:          # every stream has at least one byte; LINR_ENOSPC counts 0
            raise _lib.LinrError('linr_rc_encode_codes: a stream did not fit its region')
        with torch.cuda.stream(self.read_stream):
            self.payload_pin[:total].copy_(self.payload[:total], non_blocking=True)
        self.read_stream.synchronize()
        data = self.payload_pin[:total].numpy().tobytes()
        return [data[int(offs[i]):int(offs[i + 1])] for i in range(n)]


def encode_streams_device(c1, sym, descriptors, chunk=0):
    """encode_streams_codes on the GPU (linr_rc_encode_codes; with chunk = S > 0 linr_rc_encode_codes_chunked): c1 uint16 and sym
    uint32 device tensors, descriptors rows of {c1 element offset, symbol word offset, n}; stream i's symbols are bits 0 .. n - 1 from
    its word offset on.  Returns the streams as a list of bytes, byte for byte what the host coder gives."""
    d = np.asarray(descriptors, dtype=np.int64).reshape(-1, 3)
    if len(d) == 0:
        return []
    coder = DeviceCoderSet(len(d), DeviceCoderSet.table(d, chunk)[1], c1.device, chunk, DeviceCoderSet.chunks(d, chunk))
    coder.launch(c1.reshape(-1), sym.reshape(-1), d)
    return coder.collect()


def rc_decode_probs(probs, data, entries, occ, column, sym=None):
    """The range decoder on the GPU, a wave per entry (linr_rc_decode_probs): probs a float32 device tensor of probabilities, data a
    uint8 device tensor of stream bytes (padded to a multiple of 4), entries rows of {probability offset, n, byte offset, byte length,
    first row}; entry i's decoded symbols go to occ[first row .. first row + n, column] (occ: float32 [rows, ld] on the device) as 0.0 /
    1.0 and, with sym (uint8 [rows]), there as bytes.  Nothing else is written; the call does not synchronise."""
    L = _lib.lib()
    tab = np.ascontiguousarray(np.asarray(entries, dtype=np.int64).reshape(-1, 5))
    if occ.dim() != 2 or occ.dtype != torch.float32 or not occ.is_contiguous() or not 0 <= int(column) < occ.shape[1]:
        raise ValueError('occ is a contiguous float32 [rows, ld] tensor and column one of its columns')
    if data.dtype != torch.uint8 or probs.dtype != torch.float32 or (sym is not None and (sym.dtype != torch.uint8 or sym.numel() < occ.shape[0])):
        raise ValueError('probs float32, data uint8, sym uint8 [rows]')
    if data.numel() % 4:
        raise ValueError('the byte buffer is read in 32-bit words: pad it to a multiple of 4 bytes')
    need = int(L.linr_rc_decode_ws_bytes(len(tab)))
    ws = _lib.scratch(need + 8, occ.device)
    _lib.check(L.linr_rc_decode_probs(probs.data_ptr(), probs.numel(), data.data_ptr(), data.numel(), tab.ctypes.data, len(tab),
                                      occ.data_ptr() + 4 * int(column), int(occ.shape[1]), int(occ.shape[0]),
                                      None if sym is None else sym.data_ptr(), ws.data_ptr(), need, _lib.current_stream_handle()),
               'linr_rc_decode_probs')          # (ws may go: the caching allocator hands it out again in stream order only)


class FlatAdam:
    """torch.optim.Adam(lr, betas, eps, L2 weight_decay) + StepLR(step_size, gamma) of main.py:231-252,319-321 over the
    model's flat parameter buffer: one fused launch per step (linr_adam_step).  state_dict()/load_state_dict() use
    torch.optim.Adam's format so reference checkpoints (``optimizer_state_dict``) round-trip."""

    def __init__(self, model, lr=0.01, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-4, step_size=32, gamma=0.992):
        self.model = model
        self.lr, self.initial_lr = float(lr), float(lr)
        self.betas, self.eps, self.weight_decay = tuple(betas), float(eps), float(weight_decay)
        self.step_size, self.gamma = int(step_size), float(gamma)
        flat = model.flat_parameters()
        self.exp_avg = torch.zeros_like(flat)
        self.exp_avg_sq = torch.zeros_like(flat)
        self.grad = torch.zeros_like(flat)
        self.t = 0                      # optimiser steps taken
        self.sched_steps = 0            # scheduler.step() calls (StepLR epoch counter)
        # torch.optim.Adam keeps one step counter per parameter and skips a parameter whose .grad is None.  The reference pins
        # torch 1.13.1 (enviroment.yaml:30), whose optimizer.zero_grad() (main.py:320) leaves ZERO tensors behind, not None: the
        # context MLP of a scale is therefore skipped only until a frame containing that scale has given it its first gradient
        # (custom_dataset.py:325 drops the coarsest scales of small frames); from then on it is updated on every step, with a
        # zero gradient on frames that lack the scale (weight decay and moment decay still act, its counter advances).
        # t_scale[s] = Adam updates applied to scale s so far (0: never had a gradient).
        self.t_scale = np.zeros(model.scale_num, dtype=np.int64)
        self._segments = None

    def zero_grad(self):
        self.grad.zero_()

    def reset(self):
        """Back to the state of a freshly constructed optimiser, in place (no allocation, no host round trip)."""
        self.exp_avg.zero_()
        self.exp_avg_sq.zero_()
        self.grad.zero_()
        self.lr = self.initial_lr
        self.t = 0
        self.sched_steps = 0
        self.t_scale[:] = 0

    def advance(self, frame=None):
        """Step counters of the next update: (t, t_scale) after an optimiser step on `frame` (None: a dense gradient, every scale
        present).  Scales of the frame start their counter; started scales advance on every step (see __init__)."""
        t_scale = self.t_scale.copy()
        if frame is None:
            t_scale += 1
        else:
            present = np.zeros(len(t_scale), dtype=bool)
            for i in range(frame.n_scales):
                if frame.row_off[i + 1] > frame.row_off[i]:
                    present[frame.scale_idx[i]] = True
            t_scale[present | (t_scale > 0)] += 1
        return self.t + 1, t_scale

    def _param_segments(self):
        """[(begin, end, scale or -1)] over the flat buffer: maximal runs of parameters with the same owner."""
        if self._segments is None:
            segs, off = [], 0
            for own, p in zip(self._scale_of_param(), self.model._plist):
                n = p.numel()
                if segs and segs[-1][2] == own:
                    segs[-1][1] = off + n
                else:
                    segs.append([off, off + n, own])
                off += n
            self._segments = [tuple(x) for x in segs]
        return self._segments

    def step(self, frame=None):
        """torch.optim.Adam.step() on the dense gradient buffer self.grad: the same update, segment by segment, that the fused
        train_step applies in one launch (a scale's context MLP is skipped until its first gradient; `frame` says which scales
        the gradient came from, None = all)."""
        t, t_scale = self.advance(frame)
        flat = self.model.flat_parameters()
        runs = []                                   # adjacent segments with the same step count are one launch (usually: all of them)
        for b, e, own in self._param_segments():
            ts = t if own < 0 else int(t_scale[own])
            if ts < 1:
                continue
            if runs and runs[-1][1] == b and runs[-1][2] == ts:
                runs[-1][1] = e
            else:
                runs.append([b, e, ts])
        for b, e, ts in runs:
            ops.adam_step(flat[b:e], self.grad[b:e], self.exp_avg[b:e], self.exp_avg_sq[b:e], ts, self.lr,
                          self.betas[0], self.betas[1], self.eps, self.weight_decay)
        self.t, self.t_scale = t, t_scale

    def scheduler_step(self):
        """StepLR.step(): multiply lr by gamma every `step_size` calls (chainable form, so a clamp persists)."""
        self.sched_steps += 1
        if self.sched_steps % self.step_size == 0:
            self.lr *= self.gamma

    def clamp_lr(self, min_lr):
        """main.py:433-437."""
        if self.lr < min_lr:
            self.lr = min_lr

    def _scale_of_param(self):
        """parameter index -> scale of its scale_mlp, or -1 (names: scale_mlp.<s>.<layer>.<weight|bias>)."""
        out = []
        for name, _ in self.model.named_parameters():
            out.append(int(name.split('.')[1]) if name.startswith('scale_mlp.') else -1)
        return out

    def state_dict(self):
        state, off = {}, 0
        owner = self._scale_of_param()
        for i, p in enumerate(self.model._plist):
            n = p.numel()
            t = self.t if owner[i] < 0 else int(self.t_scale[owner[i]])
            if t > 0:                     # torch creates a parameter's state at its first update
                state[i] = {'step': torch.tensor(float(t)), 'exp_avg': self.exp_avg[off:off + n].view(p.shape).clone(),
                            'exp_avg_sq': self.exp_avg_sq[off:off + n].view(p.shape).clone()}
            off += n
        group = {'lr': self.lr, 'betas': self.betas, 'eps': self.eps, 'weight_decay': self.weight_decay,
                 'amsgrad': False, 'maximize': False, 'foreach': None, 'capturable': False,
                 'initial_lr': self.initial_lr, 'params': list(range(len(self.model._plist)))}
        return {'state': state, 'param_groups': [group]}

    def load_state_dict(self, sd):
        g = sd['param_groups'][0]
        self.lr = float(g['lr'])
        self.initial_lr = float(g.get('initial_lr', self.initial_lr))
        self.betas, self.eps, self.weight_decay = tuple(g['betas']), float(g['eps']), float(g['weight_decay'])
        off = 0
        steps = set()
        owner = self._scale_of_param()
        self.t_scale[:] = 0
        self.exp_avg.zero_()
        self.exp_avg_sq.zero_()
        for i, p in enumerate(self.model._plist):
            n = p.numel()
            st = sd['state'].get(i)
            if st is not None:
                self.exp_avg[off:off + n].copy_(st['exp_avg'].reshape(-1))
                self.exp_avg_sq[off:off + n].copy_(st['exp_avg_sq'].reshape(-1))
                t = int(float(st['step']))
                if owner[i] < 0:
                    steps.add(t)
                else:
                    if self.t_scale[owner[i]] not in (0, t):
                        raise ValueError('step counts differ inside scale_mlp.%d' % owner[i])
                    self.t_scale[owner[i]] = t
            off += n
        if len(steps) > 1:
            raise ValueError('step counts of the shared parameters differ; the fused Adam keeps one counter for them')
        self.t = steps.pop() if steps else 0


TRAIN_PRECISIONS = ('f32', 'bf16', 'bf16-deep', 'bf16-mul')


def train_step(model, opt, frame, point_num, out=None, qat_bitdepth=0):
    """One iteration of main.py:305-321 on a batched frame: bits -> loss = bits/point_num -> backward -> Adam ->
    StepLR, as ONE C-ABI call (linr_net_train_step).  Returns the device-resident bits accumulator (float64[1]);
    nothing synchronises with the host.  `out`: a zeroed float64[1] device tensor to add the bits into (e.g. one slot of a
    per-GOP vector that is cleared once per epoch) - saves the per-step allocation + fill.
    qat_bitdepth > 0: the quantisation-aware step (linr_step_args.qparams) - bits and gradient are those of the
    weights the model codec would code with at that depth (quant_uniform2 and back), Adam updates the fp32 master."""
    # what cannot run is refused before anything is allocated or called
    if model.train_precision not in TRAIN_PRECISIONS:
        raise ValueError('train_precision must be one of ' + ', '.join(repr(p) for p in TRAIN_PRECISIONS))
    if model._wide is not None and model.train_precision in ('bf16', 'bf16-deep'):
        raise _lib.LinrError('the bf16 training executor exists for hidden_channel_conv=8 only')
    if model._wide is None and model.train_precision == 'bf16-mul':          # the wide step with bf16 products (wide_net._Pass.mul)
        raise _lib.LinrError("train_precision 'bf16-mul' exists for hidden_channel_conv 16 / 32 only: width 8 has the bf16 training executor")
    bits = torch.zeros(1, dtype=torch.float64, device=frame.device) if out is None else out
    extra = {}                           # keyword arguments of the step beyond the common ones
    if qat_bitdepth:
        if model._wide is not None and not model._wide.c_step:
            raise _lib.LinrError('quantisation-aware training exists for hidden_channel_conv=8 only, and for 16 / 32 with the one-call '
                                 'step (WideNet.c_step, LINR_WIDE_C_STEP=1)')
        extra = {'qparams': model.qat_parameters(), 'bitdepth': int(qat_bitdepth)}
    if model._wide is not None and model._wide.c_step:          # hidden_channel_conv 16 / 32, opt-in: one C call (csrc/wide_train.hip)
        t, t_scale = opt.advance(frame)
        w = model._wide
        engine.net_train_step_wide(frame, model.flat_parameters(), w.C, w.step_arena(frame), opt.exp_avg, opt.exp_avg_sq, 1.0 / float(point_num), t,
                                   opt.lr, opt.betas[0], opt.betas[1], opt.eps, opt.weight_decay, bits, mul=w._train_mul(),
                                   scale_steps=t_scale, **extra)
        opt.t, opt.t_scale = t, t_scale              # committed only after the call returned without an error
        opt.scheduler_step()
        return bits
    if model._wide is not None:          # the default: the channel-blocked executor's Python schedule + the segment-wise Adam
        with torch.no_grad(), model._wide.lock:          # (the pooled buffers of the forward must survive until the backward has run)
            tape = model._wide.forward(frame, 0, 8, None, bits, keep=True, pool=True)
            model._ensure_grad_views()
            model._flat_grad.zero_()
            if tape is not None:
                model._wide.backward(frame, tape, 1.0 / float(point_num), pool=True)
            opt.grad.copy_(model._flat_grad)
            opt.step(frame)
        opt.scheduler_step()
        return bits
    t, t_scale = opt.advance(frame)
    if model.train_precision == 'bf16' and model.block_layers != 1:
        raise _lib.LinrError('the bf16 training executor supports block_layers=1 only')
    if model.train_precision != 'f32':                   # one executor; 'bf16-deep' lets it take block_layers 2..4
        extra['deep'] = model.train_precision == 'bf16-deep'
    step = engine.net_train_step if model.train_precision == 'f32' else engine.net_train_step_bf16
    step(frame, model.flat_parameters(), opt.exp_avg, opt.exp_avg_sq, 1.0 / float(point_num), t, opt.lr, opt.betas[0], opt.betas[1],
         opt.eps, opt.weight_decay, bits, scale_steps=t_scale, **extra)
    opt.t, opt.t_scale = t, t_scale              # committed only after the call returned without an error
    opt.scheduler_step()
    return bits

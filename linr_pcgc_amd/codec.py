"""Per-GOP encode / decode: mirror of encoder.py:57-203, decoder.py:51-176 and test_utils.py:199-232,299-312.

Stream layout is the reference's: per frame and scale ``pack_bitstream`` of the 8 per-stage
torchac-format streams (csrc/ac.cpp); ``low_enc_bytes`` = pack of per-frame uint8 coarsest coordinates + int32 minima;
``model.bin`` + side info from model_codec.  An encoded GOP is a dict of byte strings; ``write_gop`` / ``read_gop``
map it to the reference's directory layout (bins/frameFFFF_scaleS.bin, bins/model.bin, bins/low_enc_bytes.bin,
side_info.json).
"""
import glob
import json
import os

import numpy as np
import torch

from .function_utils import pack_bitstream, unpack_bitstream
from .model_codec import Model_Estimate, candidate_ranges, compress_params, laplace_bits_est
from .model_core import DeviceCoderSet, codes_word_off, encode_streams, encode_streams_codes
from .module_utils import octree_level_obj, qscTensor, unique_sorted  # noqa: F401
from . import stream_digests
from .stream_chunks import SIDE_BITS as STREAM_CHUNK_SIDE_BITS, check_chunk

# The probabilities the range coder sees must be reproduced BIT FOR BIT by the decoder, so the fp32 evaluation order of the
# network is part of the stream format.  ARITH_VERSION names it: 1 = taps in ascending index order (rounds 1 and 2 up to the
# "joined schedule" builds), 2 = slab-major tap order (csrc/common.h: LINR_TAP).  A stream carries the version it was coded
# with in side_info.json; decoding one of another version raises instead of silently producing wrong geometry.
ARITH_VERSION = 2


def enc_all_frame_low_xyz(gop):
    """test_utils.py:199-232: uint8 coarsest-scale coordinates per frame + int32 coordinate minima."""
    chunks = []
    for low in gop.low_xyz:
        mx = int(low.max())
        if int(np.ceil(np.log2(mx + 1))) > 8:
            raise AssertionError('downsampled xyzQ should be less than 8 bit')
        chunks.append(low.cpu().numpy().astype(np.uint8).tobytes())
    chunks.append(np.asarray(gop.coord_mins, dtype=np.int32).reshape(-1).tobytes())
    return pack_bitstream(chunks)


def dec_all_frame_low_xyz(low_byte):
    """test_utils.py:299-312."""
    chunks = unpack_bitstream(low_byte)
    mins = np.frombuffer(chunks.pop(), dtype=np.int32).reshape(-1, 3)
    return [np.frombuffer(c, dtype=np.uint8).reshape(-1, 3) for c in chunks], mins


EXTRA_SIDE_BITS = 40          # arith_version, precision and the model's shape (scale_num, block_layers, hidden_channel_conv: the reference's
                              # decoder hard-codes it, decoder.py:189) in side_info.json, one byte each, beyond the reference's side information


def model_shape(model):
    """What a decoder needs to build the model a stream was coded with (the reference's decoder hard-codes it, decoder.py:189)."""
    return {'scale_num': int(model.scale_num), 'block_layers': int(model.block_layers), 'hidden_channel_conv': int(model.hidden)}


def _code_frames_device(coded_model, gop, coder_group, chunk=0):
    """The frames' streams from the device range coder (linr_rc_encode_codes), coder_group frames per call.  The forwards stay on the
    caller's stream and write their code values and symbol planes (model.frame_codes) into group-wide buffers; the group is coded on a
    second stream behind an event, so group g is coded under the forwards of group g + 1.  Two buffer sets alternate: the forwards
    of group g + 2 wait (on the device) for the coding of group g, and the host has read group g's payload before that set is
    launched again.  chunk = S > 0: the chunked entry, a wave per chunk (DeviceCoderSet(chunk=)); the table stays per stream.
    Returns (per frame the per-scale pack_bitstream containers, per frame the bits estimate on the device)."""
    frames = gop.frames
    dev = frames[0].device
    groups = [frames[i:i + coder_group] for i in range(0, len(frames), coder_group)]
    plans = []                       # per group: per frame (c1 base, rows, word base, words), the stream table, sizes
    for group in groups:
        cb = wb = 0
        parts, desc = [], []
        for f in group:
            woff = codes_word_off(f.row_off)
            rows, words = f.rows, int(woff[-1])
            parts.append((cb, rows, wb, words))
            for i in range(f.n_scales):
                a, n = int(f.row_off[i]), int(f.row_off[i + 1] - f.row_off[i])
                desc += [(cb + k * rows + a, wb + k * words + int(woff[i]), n) for k in range(8)]
            cb, wb = cb + 8 * rows, wb + 8 * words
        plans.append((parts, np.asarray(desc, dtype=np.int64).reshape(-1, 3), cb, wb))
    n_sets = min(2, len(groups))
    max_c1, max_w = max(1, max(p[2] for p in plans)), max(1, max(p[3] for p in plans))
    max_n, max_cap = max(len(p[1]) for p in plans), max(DeviceCoderSet.table(p[1], chunk)[1] for p in plans)
    max_chunks = max(DeviceCoderSet.chunks(p[1], chunk) for p in plans)
    sets = [(torch.empty(max_c1, dtype=torch.uint16, device=dev), torch.empty(max_w, dtype=torch.uint32, device=dev),
             DeviceCoderSet(max_n, max_cap, dev, chunk, max_chunks)) for _ in range(n_sets)]
    main = torch.cuda.current_stream()
    coder_stream = torch.cuda.Stream(device=dev)
    streams, bits_dev = [None] * len(groups), []
    for g, (group, (parts, desc, _, _)) in enumerate(zip(groups, plans)):
        c1, sym, coder = sets[g % n_sets]
        if g >= n_sets:
            main.wait_event(coder.coded)                     # group g - 2 has read c1 / sym
        for f, (cb, rows, wb, words) in zip(group, parts):
            _, _, bits = coded_model.frame_codes(f, out=(c1[cb:cb + 8 * rows].view(8, rows), sym[wb:wb + 8 * words].view(8, words)))
            bits_dev.append(bits)
        ready = torch.cuda.Event()
        ready.record(main)
        if g >= n_sets:
            streams[g - n_sets] = coder.collect() if len(plans[g - n_sets][1]) else []   # ... and its payload is on the host before the set is coded into again
        if len(desc):
            with torch.cuda.stream(coder_stream):
                coder_stream.wait_event(ready)
                coder.launch(c1, sym, desc)
    for g in range(max(0, len(groups) - n_sets), len(groups)):
        streams[g] = sets[g % n_sets][2].collect() if len(plans[g][1]) else []
    frames_bytes = []
    for group, got in zip(groups, streams):
        at = 0
        for f in group:
            frames_bytes.append([pack_bitstream(got[at + 8 * i:at + 8 * i + 8]) for i in range(f.n_scales)])
            at += 8 * f.n_scales
    return frames_bytes, bits_dev


def _levels_back_to_back(levels):
    """Whether the coordinate lists are consecutive slices of one buffer (the levels of a frame staged by ops.octree_levels are)."""
    for a, b in zip(levels, levels[1:]):
        # (by storage offsets: an empty slice has no data pointer to compare)
        if not (a.is_contiguous() and b.is_contiguous() and b.storage_offset() == a.storage_offset() + a.numel() and
                a.untyped_storage().data_ptr() == b.untyped_storage().data_ptr()):
            return False
    return levels[0].is_contiguous()


def _as_segments(levels):
    """(coords, seg_off) of coordinate lists as the segments of ONE list: a view where they lie back to back in one buffer (the
    levels ops.octree_levels stages, the children of a lock-step call), a copy otherwise."""
    seg = np.zeros(len(levels) + 1, dtype=np.int64)
    seg[1:] = np.cumsum([int(c.shape[0]) for c in levels])
    if len(levels) == 1:
        return levels[0].contiguous(), seg
    if _levels_back_to_back(levels):
        return levels[0].new_empty(0).set_(levels[0].untyped_storage(), levels[0].storage_offset(), (int(seg[-1]), 3)), seg
    return torch.cat(levels, dim=0), seg


def verify_levels(levels, wants, frame_ids, scale, origins=None):
    """The decoder's check of one scale (decode_gop verify=True): the digests of the decoded children `levels` (one list per frame;
    origins: per frame the origin to add, scale 0) against the stream's values `wants` (D >> 32) - one ops.coords_digest call and one
    small read.  The first frame that differs raises _lib.LinrDigestError."""
    from . import ops
    from ._lib import LinrDigestError
    coords, seg = _as_segments(levels)
    got = ops.coords_digest(coords, seg, origins).cpu().numpy().view(np.uint64) >> np.uint64(32)
    for f, w, g in zip(frame_ids, wants, got.tolist()):
        if int(w) != int(g):
            raise LinrDigestError(f, scale, w, g)


def gop_digests_launch(gop):
    """The digests of every octree level of every frame of a staged GOP - an overfit.Gop, or any sequence of prepare_frame's frame
    dicts (encoder.encode_one_gop's reading data) - (stream_digests.py: D(i, s) of
    gop.infos[i]['all_input_info'][s]['ground_truth'], scale 0 with gop.coord_mins[i] as origin), launched on the caller's stream:
    per frame one call for scale 0 and one segmented call for the levels s >= 1 where they lie back to back in one buffer (a call per
    level otherwise).  No synchronisation, no draw from torch's generator.  Returns (device int64 [sum n_scales] - frame by frame,
    scale 0 first -, the frames' scale counts); gop_digests_bin reads it."""
    from . import ops
    infos = gop.infos if hasattr(gop, 'infos') else list(gop)
    coord_mins = gop.coord_mins if hasattr(gop, 'coord_mins') else [fr['coord_data_min'] for fr in infos]
    levels = [[sc['ground_truth'] for sc in info['all_input_info']] for info in infos]
    n_scales = [len(lv) for lv in levels]
    out = torch.empty(sum(n_scales), dtype=torch.int64, device=levels[0][0].device)
    at = 0
    for lv, cmin in zip(levels, coord_mins):
        ops.coords_digest(lv[0].contiguous(), origins=[cmin], out=out[at:at + 1])
        rest = lv[1:]
        if 1 < len(rest) <= LOCKSTEP_MAX_FRAMES and _levels_back_to_back(rest):
            ops.coords_digest(*_as_segments(rest), out=out[at + 1:at + len(lv)])
        else:
            for s, c in enumerate(rest, 1):
                ops.coords_digest(c.contiguous(), out=out[at + s:at + s + 1])
        at += len(lv)
    return out, n_scales


def gop_digests_bin(launched):
    """digests.bin of what gop_digests_launch returned: the GOP's one host read."""
    dev, n_scales = launched
    vals = dev.cpu().numpy().view(np.uint64).tolist()
    it = iter(vals)
    return stream_digests.pack([[next(it) for _ in range(n)] for n in n_scales])


def _gop_result(gop, comp, side_info, frames_bytes, bits_dev, found=None, digests=None, averaged=None):
    bits_est = float(torch.stack(bits_dev).sum())
    low = enc_all_frame_low_xyz(gop)
    points = sum(gop.point_nums)
    occ_bits = 8 * sum(len(b) for fb in frames_bytes for b in fb)
    # ... and the stream_chunk field, when the GOP has one, as 32 bits
    side_bits = EXTRA_SIDE_BITS + (STREAM_CHUNK_SIDE_BITS if side_info.get('stream_chunk') else 0)
    extra = {} if found is None else {'qrange': {'trims': found['trims'], 'objective_bits': found['objective_bits'],
                                                 'chosen': found['trims'][found['chosen']], 'search_s': found['search_s']}}
    if averaged is not None:
        extra['average'] = averaged
    if digests is not None:
        # ... and the digests, when the GOP has them: their file and the one-byte field (stream_digests.bits)
        digests_bin = gop_digests_bin(digests)
        if [len(fb) for fb in frames_bytes] != digests[1]:
            raise AssertionError('a frame has another number of scale streams than of staged levels')
        side_bits += stream_digests.bits(digests_bin)
        extra.update({'digests_bin': digests_bin, 'digest_bits': stream_digests.bits(digests_bin)})
    return {**extra, 'frames': frames_bytes, 'model_bin': comp['final_bytes'], 'side_info': side_info, 'low_enc_bytes': low,
            'point_num': points, 'bits_est': bits_est,
            # the five one-byte side-info fields this codec adds (arith_version, precision, scale_num, block_layers,
            # hidden_channel_conv: EXTRA_SIDE_BITS = 40) are counted with the model
            'bpp': {'point_bpp': occ_bits / points, 'model_bpp': (comp['bit_real'] + side_bits) / points,
                    'xyzlow_bpp': len(low) * 8 / points,
                    'bpp_all': (occ_bits + comp['bit_real'] + side_bits + len(low) * 8) / points}}       # test_utils.py:146-157


def _coder_threads(n_threads):
    """The host threads of the range coders: as asked, by default the cores this process may use, at most 16."""
    if n_threads is not None:
        return n_threads
    return max(1, min(16, len(os.sched_getaffinity(0)) if hasattr(os, 'sched_getaffinity') else 8))


def qrange_eval_frames(n_frames, want):
    """The frames the range search evaluates: `want` of a GOP's n_frames, evenly spaced (the middles of `want` equal stretches); 0 or a
    value >= n_frames: all of them."""
    want = int(want)
    if want <= 0 or want >= n_frames:
        return list(range(n_frames))
    return [(2 * i + 1) * n_frames // (2 * want) for i in range(want)]


def _quantise_own_range(vec, lo, hi, bitdepth, with_codes):
    """One vector under the given range through linr_params_fake_quant_ranges (a device vector) or its host twin (a CPU vector: the
    search on stub frames, no GPU needed) -> (de-quantised [n], codes as a host array or None, sum |q - mu|)."""
    from . import _lib, engine
    n = vec.numel()
    if vec.is_cuda:
        q, codes, stats = engine.params_fake_quant_ranges(vec, [(lo, hi)], bitdepth, codes=with_codes)
        return q[0, :n], codes.cpu().numpy()[0, :n] if with_codes else None, stats
    p = np.ascontiguousarray(vec.detach().numpy(), dtype=np.float32)
    stride = (n + 3) & ~3
    r = np.asarray([lo, hi], dtype=np.float32)
    q, c, st = np.empty((1, stride), np.float32), np.empty((1, stride), np.uint16), np.empty((1, 4), np.int64)
    _lib.check(_lib.lib().linr_params_fake_quant_ranges_host(p.ctypes.data, n, int(bitdepth), r.ctypes.data, 1, stride, q.ctypes.data,
                                                             c.ctypes.data, st.ctypes.data), 'linr_params_fake_quant_ranges_host')
    return torch.from_numpy(q[0, :n].copy()), c[0, :n] if with_codes else None, torch.from_numpy(st)


def search_average(model, model_ori, gop, candidates, decays, bitdepth=8, precision='f32', eval_frames=4, frame_bits=None):
    """The encoder's rate-checked choice between the model's own parameters and averages of the overfit's iterates (encode_gop avg=).
    Adam's steps stay about one quantiser step wide to the end of an overfit, so the last iterate is a noisy one; an average of the
    iterates (overfit_gop avg_decays=) may code cheaper - or not, so it is measured, like the quantiser range (search_qrange).
    Candidate 0 is model.flat_parameters() (today's call), candidates 1..K the rows of `candidates` ([K][n], on the model's device)
    with the decays `decays`.  Each is quantised under its OWN (min, max) - one small host read of the K + 1 pairs, then
    linr_params_fake_quant_ranges per vector, whose integer stats give model_codec.laplace_bits_est -, filled into `model_ori` through
    Model_Estimate._fill and asked for its bits on the evaluated frames (qrange_eval_frames) by the codec's own forward.  Objective:
        model_bits_est_j + (frames / evaluated frames) * sum of the evaluated frames' bits
    The smallest wins, a tie goes to the smaller index, so on the frames it evaluates the choice is never worse than the plain model.
    A candidate with a non-finite element is never evaluated and never wins (its objective is None).  On the caller's stream, no draw
    from torch's generator.  gop / frame_bits: as in search_qrange.  Returns {'decays' (K), 'objective_bits' (K + 1, plain first),
    'chosen' (an index into the candidates: 0 = plain, j = decays[j - 1]), 'frames', 'search_s'}; `model_ori` is left filled with the
    last evaluated candidate."""
    import time
    t0 = time.time()
    flat = model.flat_parameters().detach()
    n = flat.numel()
    decays = [float(d) for d in decays]
    cands = torch.as_tensor(candidates).detach()
    if cands.dim() != 2 or cands.shape[0] != len(decays) or cands.shape[1] != n or cands.dtype != torch.float32 or cands.device != flat.device:
        raise ValueError('search_average: %d decays need float32 candidates [%d][%d] on %s, got %s %s on %s'
                         % (len(decays), len(decays), n, flat.device, cands.dtype, tuple(cands.shape), cands.device))
    vecs = [flat] + [cands[k].contiguous() for k in range(len(decays))]
    pairs = torch.stack([torch.stack([v.min(), v.max()]) for v in vecs]).cpu().tolist()          # NaN and inf show here
    with_codes = bitdepth == 8
    frames = gop.frames if frame_bits is None else gop
    if frame_bits is None:
        frame_bits = lambda cand, i: cand.frame_probs(frames[i])[1]
    todo = qrange_eval_frames(len(frames), eval_frames)
    bits, stats, evaluated = [], [], []
    for j, (v, (lo, hi)) in enumerate(zip(vecs, pairs)):
        if not (np.isfinite(lo) and np.isfinite(hi)):
            continue
        q, codes_h, st = _quantise_own_range(v, lo, hi, bitdepth, with_codes)
        cand = Model_Estimate._fill(model_ori, q, codes_h, lo, hi, bitdepth)
        cand.inference_precision = precision
        bits.append(torch.stack([frame_bits(cand, i) for i in todo]).sum())
        stats.append(st)
        evaluated.append(j)
    objective = [None] * len(vecs)
    if evaluated:
        bits = torch.stack(bits).cpu().tolist()
        stats = torch.cat(stats).cpu().tolist()
        up = len(frames) / len(todo)
        for j, st, b in zip(evaluated, stats, bits):
            objective[j] = laplace_bits_est(n, st[3], bitdepth) + up * b
    finite = [j for j in evaluated if np.isfinite(objective[j])]
    chosen = min(finite, key=lambda j: (objective[j], j)) if finite else 0
    return {'decays': decays, 'objective_bits': objective, 'chosen': chosen, 'frames': todo, 'search_s': time.time() - t0}


def search_qrange(model, model_ori, gop, bitdepth=8, precision='f32', trims=None, eval_frames=4, frame_bits=None, flat=None):
    """The encoder's rate-checked quantiser range (encode_gop qrange_search=True).  The model codec quantises with ONE step for the
    whole parameter vector, (max - min) / (2^bitdepth - 1), so a single outlier weight widens it for every other weight.  A decoder
    reads the range from side_info.json (min_param / max_param) and never checks that it is the vector's own, so the encoder may
    write a narrower one and let the few weights outside it saturate.  Whether that pays is not predictable - the outlier may
    matter to the network - so it is measured: every candidate (model_codec.candidate_ranges: `trims` weights cut at either end;
    trim 0, today's range, is always the first) is quantised by one call of linr_params_fake_quant_ranges for all of them, filled
    into `model_ori` through Model_Estimate._fill, and asked for its bits on the evaluated frames (qrange_eval_frames) by the
    codec's own forward (frame_probs: any precision, any width).  Objective of candidate j:
        model_bits_est_j + (frames / evaluated frames) * sum of the evaluated frames' bits
    (model_codec.laplace_bits_est from the kernel's integer stats).  The smallest wins, a tie goes to the smaller trim, so on the
    frames it evaluates the choice is never worse than trim 0.  On the caller's stream, no draw from torch's generator.
    gop: an overfit.Gop, or - with frame_bits(candidate model, i) -> device float64[1], the bits of frame i - any sequence of frames
    (encoder.encode_one_gop's per-scale inputs).  Returns
    {'trims', 'ranges', 'objective_bits', 'chosen' (an index into trims), 'frames', 'search_s'}; `model_ori` is left filled with
    the last candidate.  flat (None: model.flat_parameters()): the vector to search the range of instead - the average that
    search_average chose."""
    import time
    from . import engine
    t0 = time.time()
    flat = (model.flat_parameters() if flat is None else flat).detach()
    kept, ranges = candidate_ranges(flat.to('cpu', torch.float32), trims)
    with_codes = bitdepth == 8                               # what _fill hands to the executors that run from codes
    q, codes, stats = engine.params_fake_quant_ranges(flat, ranges, bitdepth, codes=with_codes)
    n = flat.numel()                                         # (the rows are padded to the kernel's stride)
    codes_h = codes.cpu().numpy()[:, :n] if with_codes else None
    frames = gop.frames if frame_bits is None else gop
    if frame_bits is None:
        frame_bits = lambda cand, i: cand.frame_probs(frames[i])[1]
    todo = qrange_eval_frames(len(frames), eval_frames)
    bits = []
    for j, (lo, hi) in enumerate(ranges):
        cand = Model_Estimate._fill(model_ori, q[j, :n], None if codes_h is None else codes_h[j], lo, hi, bitdepth)
        cand.inference_precision = precision
        bits.append(torch.stack([frame_bits(cand, i) for i in todo]).sum())
    bits = torch.stack(bits).cpu().tolist()
    stats = stats.cpu().tolist()
    up = len(frames) / len(todo)
    objective = [laplace_bits_est(n, st[3], bitdepth) + up * b for st, b in zip(stats, bits)]
    chosen = min(range(len(objective)), key=lambda j: (objective[j], j))
    return {'trims': kept, 'ranges': ranges, 'objective_bits': objective, 'chosen': chosen, 'frames': todo, 'search_s': time.time() - t0}


def encode_gop(model, model_ori, gop, bitdepth=8, n_threads=None, precision='f32', device_codes=False, device_coder=False,
               coder_group=8, qrange_search=False, qrange_trims=None, qrange_frames=4, stream_chunk=0, digests=False, avg=None, avg_frames=4):
    """encoder.encode_one_gop: quantise the model, then per frame ONE forward over all scales and 8 x scales
    independent arithmetic-coded streams (thread pool).  precision='bf16': the forward runs on the bf16 / uint8-weight
    executor (BASELINE config[4]); the choice is recorded in side_info so that the decoder reproduces it.
    device_codes=True: the coder's inputs are prepared on the GPU (model.frame_codes): 16-bit code values and one symbol bit cross to
    the host per symbol instead of an fp32 probability and a byte, and the coder threads read the code values instead of computing
    them.  The streams are byte for byte those of the default path, so nothing about it is recorded.
    device_coder=True (implies device codes): the range coder itself runs on the GPU, coder_group (1..64) frames per call
    (_code_frames_device); only stream bytes and lengths cross to the host and no coder thread is started.  Again the same bytes,
    again nothing recorded.
    qrange_search=True (opt-in): the quantiser's range is chosen by search_qrange among the candidates of qrange_trims (default
    model_codec.DEFAULT_QRANGE_TRIMS) on qrange_frames evaluated frames (0: all); the winner goes through the model codec
    (compress_model(qrange=)) and everything behind it is unchanged: min_param / max_param carry the range, every decoder decodes the
    stream.  The result then has 'qrange' = {'trims', 'objective_bits', 'chosen' (the chosen trim), 'search_s'}, and - when there was
    more than the plain range to choose from - side_info the informational 'qrange_trim' and 'qrange_candidates'.
    stream_chunk=S > 0 (opt-in; a multiple of 64 in 64..2^24; stream_chunks.py has the format): every stage stream of more than S
    symbols is cut into chunks of S symbols that are coded - and later decoded - independently, on the coder threads or a wave each,
    at a few bytes per chunk.  The decoder needs S: side_info gets 'stream_chunk', counted as 32 bits in model_bpp / bpp_all, and a
    build that does not know the field cannot decode such a GOP.  The three coder paths write the same bytes at the same S; a GOP
    whose streams all have at most S symbols differs from the plain one in that field only.  hidden_channel_conv 8 only.
    digests=True (opt-in; stream_digests.py has the format): the GOP becomes self-checking.  The digest of every octree level of every
    frame is computed on the GPU where the staged levels are (gop_digests_launch: two library calls per frame on the caller's stream,
    ONE host read per GOP, no draw from torch's generator) and returned as 'digests_bin' (write_gop: bins/digests.bin); side_info gets
    'digests' = 1, and 8 * len(digests_bin) + 8 bits are counted in model_bpp / bpp_all and reported as 'digest_bits'.  Every stream
    and every other file is what digests=False writes; decode_gop checks each level as it decodes it.
    avg = overfit_gop's info['averages'] (opt-in; {'decays', 'steps', 'params' [K][n]}): search_average chooses by measured rate, on
    avg_frames evaluated frames (0: all), between the model's own parameters and the K averages of the overfit's iterates.  A chosen
    average goes through compress_params / _fill into `model_ori` - the training model, its optimiser and hence the checkpoint and the
    next GOP's warm start are only read - and with qrange_search the range search then runs on it.  When the model's own parameters
    win, every file but side_info.json's informational fields is byte for byte the plain run's.  side_info gains 'avg_decay' (the
    chosen decay, null: the model's own) and 'avg_candidates' (not counted, ignored by the decoders), the result
    'average' = {'decays', 'objective_bits', 'chosen', 'frames', 'search_s'}."""
    if device_coder and not 1 <= int(coder_group) <= 64:
        raise ValueError('coder_group must be in 1..64, got %r' % (coder_group,))
    stream_chunk = check_chunk(stream_chunk)
    if stream_chunk and getattr(model, '_wide', None) is not None:
        raise ValueError('stream_chunk needs hidden_channel_conv 8: the widths 16 and 32 decode stage-wise in Python, without chunks')
    n_threads = _coder_threads(n_threads)
    averaged, avg_vec = None, None
    if avg is not None and len(avg['decays']):
        averaged = search_average(model, model_ori, gop, avg['params'], avg['decays'], bitdepth, precision, avg_frames)
        if averaged['chosen']:                           # (0: the model's own parameters - everything below is today's call)
            avg_vec = avg['params'][averaged['chosen'] - 1].detach().contiguous()
    found = search_qrange(model, model_ori, gop, bitdepth, precision, qrange_trims, qrange_frames, flat=avg_vec) if qrange_search else None
    # trim 0 is the vector's own (min, max): today's call, to the letter
    qrange = found['ranges'][found['chosen']] if found is not None and found['chosen'] else None
    if avg_vec is None:
        comp = Model_Estimate().compress_model(model, bitdepth, True, model_ori, **({} if qrange is None else {'qrange': qrange}))
    else:
        # the chosen average through the same model codec into the shell; the training model is only read
        comp = compress_params(avg_vec, bitdepth, qrange)
        comp['new_model'] = Model_Estimate._fill(model_ori, comp['recon_ret'], comp['symbols'], comp['min_param'], comp['max_param'], bitdepth)
    coded_model = comp['new_model']                      # the de-quantised model is what codes the geometry
    coded_model.inference_precision = precision
    side_info = {'mu': comp['mu'], 'b': comp['b'], 'min_param': comp['min_param'], 'max_param': comp['max_param'],
                 'enc_mode': comp['enc_mode'], 'bitdepth': bitdepth}
    if precision != 'f32':
        side_info['precision'] = precision
    side_info['arith_version'] = ARITH_VERSION
    side_info.update(model_shape(model))
    if stream_chunk:
        side_info['stream_chunk'] = stream_chunk
    launched = None
    if digests:
        side_info['digests'] = stream_digests.VERSION
        launched = gop_digests_launch(gop)               # read in _gop_result, behind the coding
    # informational (the decoder does not need it): which training executor produced the coded model
    side_info['train_precision'] = getattr(model, 'train_precision', 'f32')
    # ... and, when the driver says so, how many of its last epochs were quantisation-aware (overfit_gop qat_epochs=): not counted
    # in EXTRA_SIDE_BITS, ignored by the decoders
    if getattr(model, 'qat_epochs', 0):
        side_info['qat_epochs'] = int(model.qat_epochs)
    # ... and which quantiser range the search chose among how many: not counted, ignored by the decoders (min_param / max_param are
    # the range).  A search with nothing but the plain range to choose from records nothing: its files are the plain files.
    if found is not None and len(found['trims']) > 1:
        side_info['qrange_trim'] = int(found['trims'][found['chosen']])
        side_info['qrange_candidates'] = len(found['trims'])
    # ... and which average of the iterates was coded (null: the model's own parameters) among how many candidates: not counted,
    # ignored by the decoders (model.bin holds the vector)
    if averaged is not None:
        side_info['avg_decay'] = averaged['decays'][averaged['chosen'] - 1] if averaged['chosen'] else None
        side_info['avg_candidates'] = len(averaged['decays']) + 1
    if device_coder:
        frames_bytes, bits_dev = _code_frames_device(coded_model, gop, int(coder_group), stream_chunk)
        return _gop_result(gop, comp, side_info, frames_bytes, bits_dev, found, launched, averaged)
    # Pipeline: the GPU forward + D2H of frame i+1 runs while host workers range-code earlier frames (the coder's C call
    # releases the GIL).  A frame has 8 x scales independent streams, but the 8 streams of its finest scale carry 73 % of the
    # symbols, so one frame keeps only ~8 threads busy: TWO frames are coded concurrently, each on half of the threads
    # (measured: 2.1 ms per frame with one worker x 16 threads, the forward + copies take 1.3 ms).
    from concurrent.futures import ThreadPoolExecutor
    workers = 2 if n_threads >= 4 else 1
    per_job = max(1, n_threads // workers)

    def code(p_host, occ_host, row_off, n_scales):
        # device_codes: p_host holds code values, occ_host bit planes in which every scale has words of its own (model.frame_codes)
        ps, ss, ns = [], [], []
        col_off = codes_word_off(row_off) if device_codes else row_off
        for i in range(n_scales):
            a, b = int(row_off[i]), int(row_off[i + 1])
            sa, sb = int(col_off[i]), int(col_off[i + 1])
            for k in range(8):
                ps.append(p_host[k, a:b])
                ss.append(occ_host[k, sa:sb])
                ns.append(b - a)
        streams = encode_streams_codes(ps, ss, ns, per_job, stream_chunk) if device_codes else encode_streams(ps, ss, per_job, stream_chunk)
        return [pack_bitstream(streams[8 * i:8 * i + 8]) for i in range(n_scales)]

    # Device side: forward of frame i+1 on the caller's stream while a copy stream moves the probabilities (fp32) and the
    # occupancy symbols (cast to 1 byte on the GPU) of frame i into a ring of pinned buffers; the host thread only waits for
    # a copy that is already one frame old before it hands the buffers to a coder worker.
    RING = 4
    max_rows = max(f.rows for f in gop.frames)
    dev = gop.frames[0].device
    if device_codes:
        max_cols = max(int(codes_word_off(f.row_off)[-1]) for f in gop.frames)
        p_pin = [torch.empty(8 * max_rows, dtype=torch.uint16, pin_memory=True) for _ in range(RING)]
        o_pin = [torch.empty(8 * max_cols, dtype=torch.uint32, pin_memory=True) for _ in range(RING)]
    else:
        p_pin = [torch.empty(8 * max_rows, dtype=torch.float32, pin_memory=True) for _ in range(RING)]
        o_pin = [torch.empty(8 * max_rows, dtype=torch.uint8, pin_memory=True) for _ in range(RING)]
    copy_stream = torch.cuda.Stream(device=dev)
    jobs, bits_dev, pending = [], [], []

    def hand_over(entry, coder):
        slot, rows, f, keep, ev_c = entry
        ev_c.synchronize()
        cols = keep[1].shape[1]
        p_host = p_pin[slot][:8 * rows].view(8, rows).numpy()
        occ_host = o_pin[slot][:8 * cols].view(8, cols).numpy()
        jobs.append(coder.submit(code, p_host, occ_host, f.row_off, f.n_scales))

    with ThreadPoolExecutor(max_workers=workers) as coder:
        for i, f in enumerate(gop.frames):
            slot = i % RING
            if i >= RING:
                jobs[i - RING].result()                     # the worker that read this slot's buffers has finished
            if device_codes:
                probs, occ_t, bits = coded_model.frame_codes(f)          # code values and symbol bit planes: no transpose, no cast
            else:
                probs, bits = coded_model.frame_probs(f)
                occ_t = f.occ.t().to(torch.uint8).contiguous()
            bits_dev.append(bits)
            ev_f = torch.cuda.Event()
            ev_f.record()
            with torch.cuda.stream(copy_stream):
                copy_stream.wait_event(ev_f)
                p_pin[slot][:8 * f.rows].view(8, f.rows).copy_(probs, non_blocking=True)
                o_pin[slot][:8 * occ_t.shape[1]].view(8, occ_t.shape[1]).copy_(occ_t, non_blocking=True)
                ev_c = torch.cuda.Event()
                ev_c.record(copy_stream)
            pending.append((slot, f.rows, f, (probs, occ_t), ev_c))         # keeps the device tensors alive until copied
            if len(pending) > 1:
                hand_over(pending.pop(0), coder)
        while pending:
            hand_over(pending.pop(0), coder)
        frames_bytes = [j.result() for j in jobs]
    return _gop_result(gop, comp, side_info, frames_bytes, bits_dev, found, launched, averaged)


def decode_one_frame(model, frame_enc_bytes, xyz_low, chunk=0, n_threads=1, device_decoder=False, digests=None, origin=None, frame=0):
    """decoder.decode_one_frame (decoder.py:153-176): coarse to fine, 8 AC-decoded stages per scale.  A scale is ONE call into the
    library (model.decode_scale -> linr_decode_scale: kernel map, the 7-neighbour occupancy read off it instead of
    qscTensor.set_offset_tensor's searches, the 8 stage forwards with their host round trips, upper_layer), so the Python side of a
    frame is seven buffer allocations.  chunk = S > 0: the stage streams are chunked (side_info's stream_chunk) and a stage's chunks are
    decoded on n_threads host threads.  device_decoder=True: the range decoders run on the GPU (model.decode_scale(device_decoder=True)
    -> linr_decode_opts.device), no host round trip per stage; n_threads is ignored.
    digests = the frame's stored values (stream_digests.unpack: one per scale; None: no check): every scale's children are checked
    (verify_levels) before the next scale is started, scale 0 with `origin` (the frame's coord_data_min) added; a level that differs
    raises _lib.LinrDigestError naming `frame` and the scale."""
    lowx = unique_sorted(xyz_low)          # (hidden_channel_conv 16 / 32: the same loop, model.decode_scale -> linr_decode_scale_wide)
    bits = max(1, int(xyz_low.max()).bit_length()) if xyz_low.numel() else 1       # coordinates of the coarsest level
    for s_idx in range(len(frame_enc_bytes) - 1, -1, -1):
        bits = min(bits + 1, 21)
        lowx = model.decode_scale(lowx, s_idx, frame_enc_bytes[s_idx], bits, chunk, n_threads, device_decoder)
        if digests is not None:
            verify_levels([lowx], [digests[s_idx]], [frame], s_idx, [origin] if s_idx == 0 and origin is not None else None)
    return {'dec_coord': lowx}


def decode_one_frame_stagewise(model, frame_enc_bytes, xyz_low):
    """The same through the reference-shaped surface (model.decode per scale + octree_level.upper_layer in torch): kept as the
    cross-check of decode_one_frame."""
    lowx = unique_sorted(xyz_low)
    for s_idx in range(len(frame_enc_bytes) - 1, -1, -1):
        occ_lst = model.decode({'enc_bytes': frame_enc_bytes[s_idx], 'coord': lowx, 'offset_tensor': None,
                                'scale_idx': s_idx})
        lowx = octree_level_obj.upper_layer(lowx, torch.cat(occ_lst, dim=-1))
    return {'dec_coord': lowx}


LOCKSTEP_MAX_FRAMES = 64                  # LINR_DECODE_MAX_FRAMES of include/linr_hip.h
LOCKSTEP_MAX_ROWS = (1 << 26) - 64        # rows of one lock-step call: the compressed kernel map's 32-bit bound (linr_cmap_fits32)


def _lockstep_scale(model, lows, s_idx, encs, n_threads, chunk=0, device_decoder=False, check=None):
    """One scale of a lock-step group; a group whose levels together pass the row bound of one call is halved.  check = (the frames'
    stored digests of this scale, their frame ids, their origins or None): the call's children - back to back, the frames as
    segments - are verified (verify_levels) behind it."""
    if len(lows) > 1 and sum(int(c.shape[0]) for c in lows) > LOCKSTEP_MAX_ROWS:
        h = len(lows) // 2
        halves = [None, None] if check is None else [tuple(None if c is None else c[:h] for c in check),
                                                     tuple(None if c is None else c[h:] for c in check)]
        return (_lockstep_scale(model, lows[:h], s_idx, encs[:h], n_threads, chunk, device_decoder, halves[0]) +
                _lockstep_scale(model, lows[h:], s_idx, encs[h:], n_threads, chunk, device_decoder, halves[1]))
    out = model.decode_scale_batch(lows, s_idx, encs, n_threads, chunk, device_decoder)
    if check is not None:
        verify_levels(out, check[0], check[1], s_idx, check[2])
    return out


def decode_frames_lockstep(model, frames_enc_bytes, xyz_lows, n_threads=8, chunk=0, device_decoder=False, digests=None, origins=None,
                           frame_ids=None):
    """decode_one_frame for a group of frames with the same number of scales, in lock step: coarse to fine, every scale of the whole
    group is ONE call into the library (model.decode_scale_batch -> linr_decode_scale_batch; with device_decoder
    linr_decode_opts.device, the group's range decoders on the GPU).  Returns the frames' coordinates.
    digests = per frame its stored values (stream_digests.unpack; None: no check): every scale of the group is verified before the next
    is started, scale 0 with the frames' `origins` added; frame_ids (default 0, 1, ...) name the frames in a LinrDigestError."""
    if device_decoder and getattr(model, '_wide', None) is not None:
        raise ValueError('the device decoder needs hidden_channel_conv 8')
    lows = [unique_sorted(x) for x in xyz_lows]
    ids = list(range(len(lows))) if frame_ids is None else list(frame_ids)
    for s_idx in range(len(frames_enc_bytes[0]) - 1, -1, -1):
        check = None if digests is None else ([d[s_idx] for d in digests], ids, list(origins) if s_idx == 0 and origins is not None else None)
        lows = _lockstep_scale(model, lows, s_idx, [f[s_idx] for f in frames_enc_bytes], n_threads, chunk, device_decoder, check)
    return lows


def lockstep_groups(todo, n_scales, lockstep):
    """`todo` cut into groups of up to `lockstep` consecutive entries whose frames have the same number of scale streams."""
    groups = []
    for i in todo:
        if groups and len(groups[-1]) < lockstep and n_scales[groups[-1][0]] == n_scales[i]:
            groups[-1].append(i)
        else:
            groups.append([i])
    return groups


def decode_gop(model_ori, enc, device='cuda', frames=None, workers=1, timing=None, lockstep=0, n_threads=None, device_decoder=False,
               verify=True):
    """decoder.decode_one_gop: rebuild the model from model.bin, then every frame from its streams alone.
    lockstep=B > 0 (opt-in; 0 = the per-frame path below, untouched): the requested frames are decoded in groups of up to B
    consecutive entries, the scales of a group from coarsest to finest in lock step (decode_frames_lockstep), the group's range
    decoders on `n_threads` host threads (default: the cores this process may use, at most 16).  `workers` then means groups in
    flight, each on its own stream.  Models of hidden_channel_conv 16 / 32 take workers and lockstep as width 8 does: their scales are
    C calls, too (linr_decode_scale_wide / _batch_wide), which keep nothing on the model.  The streams are the same either way.
    `timing` (a dict) receives 'setup_s': the once-per-GOP part (model.bin -> parameters, the coarsest coordinates), and with
    lockstep 'lockstep_ws_bytes': the largest device workspace of a lock-step call.
    side_info's 'stream_chunk' = S (absent or 0: nothing changes): the stage streams are chunked (stream_chunks.py) and a stage's
    chunks are range-decoded in parallel - with lockstep on the group's threads as ever, and per frame on n_threads threads, too
    (default: the cores this process may use, at most 16, divided by `workers`).  A stream whose chunk header does not hold raises
    LinrError.
    device_decoder=True (opt-in; hidden_channel_conv 8 only, ValueError otherwise): the range decoders of every scale run on the GPU,
    a wave per stream or chunk, from the probabilities where the stage forward left them (linr_decode_opts.device of
    linr_decode_scale / linr_decode_scale_batch): no host coder threads (n_threads is ignored) and one synchronisation per scale instead of one
    per stage.  It reads the same streams and side_info.json and decodes the same geometry; it composes with workers, lockstep and
    stream_chunk.
    verify=True (the default; it does nothing for a GOP without digests, i.e. without side_info's 'digests'; with the field but without
    enc['digests_bin'] - a deleted file - it is LinrError):
    every decoded scale of every requested frame is digested on the GPU and compared with the stream's value before the next scale is
    started (verify_levels: one library call and one small read per scale; in lock step the group's frames as segments), on every
    path above.  The first level that differs raises _lib.LinrDigestError (frame, scale, want, got) - before garbage is expanded
    further.  A digests.bin whose length does not fit the GOP's stream files, or a format version of a newer build, is LinrError
    before any launch.  verify=False: nothing of this runs.
    Frames are independent once the model is known; with workers > 1 they are decoded by a host thread pool, each
    thread on its own HIP stream (a frame's own chain - 56 stage forwards with a serial range decode in between - cannot
    be parallelised, but the range decoding of one frame overlaps the stage forwards and copies of the others; the
    C calls release the GIL)."""
    import time
    t_setup = time.time()
    side = dict(enc['side_info'])
    coded_with = int(side.pop('arith_version', 1))
    if coded_with != ARITH_VERSION:
        from ._lib import LinrError
        raise LinrError('this stream was coded with network arithmetic version %d; this build decodes version %d (the fp32 '
                        'accumulation order of the convolutions is part of the stream format: decode with the build that '
                        'encoded it)' % (coded_with, ARITH_VERSION))
    stored = None
    if verify and side.get('digests'):
        from ._lib import LinrError
        stream_digests.check_version(side)
        if enc.get('digests_bin') is None:
            raise LinrError('side_info.json says that the GOP carries digests, but there is no bins/digests.bin (decode with verify=False '
                            'to do without)')
        try:
            stored = stream_digests.unpack(enc['digests_bin'], [len(f) for f in enc['frames']])
        except ValueError as e:
            raise LinrError(str(e)) from None
    side.pop('digests', None)
    want = {k: side[k] for k in ('scale_num', 'block_layers', 'hidden_channel_conv') if k in side}
    have = model_shape(model_ori)
    if any(int(v) != have[k] for k, v in want.items()):
        raise ValueError('the stream was coded with a model of shape %s; the model handed to the decoder has %s' % (want, have))
    side['final_bytes'] = enc['model_bin']
    model, _ = Model_Estimate().decompress_model(model_ori, side)
    model.inference_precision = side.get('precision', 'f32')
    chunk = check_chunk(side.get('stream_chunk', 0))
    if chunk and getattr(model, '_wide', None) is not None:
        raise ValueError('chunked stage streams decode with hidden_channel_conv 8 only')
    device_decoder = bool(device_decoder)
    if device_decoder and getattr(model, '_wide', None) is not None:
        raise ValueError('the device decoder needs hidden_channel_conv 8: the widths 16 and 32 decode stage-wise in Python')
    lows, mins = dec_all_frame_low_xyz(enc['low_enc_bytes'])
    todo = list(range(len(enc['frames'])) if frames is None else frames)
    if timing is not None:
        if device != 'cpu':
            torch.cuda.synchronize()
        timing['setup_s'] = time.time() - t_setup

    per_frame = max(1, _coder_threads(n_threads) // max(1, int(workers))) if chunk else 1

    def one(i):
        xyz_low = torch.tensor(lows[i].astype(np.int32), device=device)
        dec = decode_one_frame(model, list(enc['frames'][i]), xyz_low, chunk, per_frame, device_decoder,
                               None if stored is None else stored[i], mins[i].tolist(), i)['dec_coord']
        return dec + torch.tensor(mins[i], device=device, dtype=torch.int32)

    if lockstep and lockstep > 0 and todo:
        out = _decode_gop_lockstep(model, enc, lows, mins, todo, device, workers, min(int(lockstep), LOCKSTEP_MAX_FRAMES), n_threads, chunk,
                                   device_decoder, stored)
        if timing is not None:
            timing['lockstep_ws_bytes'] = int(getattr(model, '_lockstep_ws_peak', 0))          # the largest workspace of a call
        return out
    return _map_on_streams(one, todo, workers)


def _map_on_streams(fn, items, workers):
    """[fn(x) for x in items] on a pool of `workers` host threads, every call on a fresh HIP stream of the caller's device that
    waits on the caller's stream first and is synchronised before the call's result is handed back; serial on the caller's stream
    with one worker or one item."""
    if workers <= 1 or len(items) <= 1:
        return [fn(x) for x in items]
    from concurrent.futures import ThreadPoolExecutor
    main_stream = torch.cuda.current_stream()
    dev_index = torch.cuda.current_device()

    def job(x):
        torch.cuda.set_device(dev_index)
        st = torch.cuda.Stream()
        st.wait_stream(main_stream)                 # the decompressed parameters were written on the caller's stream
        with torch.cuda.stream(st):
            out = fn(x)
        st.synchronize()
        return out

    with ThreadPoolExecutor(max_workers=workers) as pool:
        return list(pool.map(job, items))


def _decode_gop_lockstep(model, enc, lows, mins, todo, device, workers, lockstep, n_threads, chunk=0, device_decoder=False, stored=None):
    n_threads = _coder_threads(n_threads)
    groups = lockstep_groups(todo, {i: len(enc['frames'][i]) for i in set(todo)}, lockstep)
    workers = max(1, min(int(workers), len(groups)))
    per_group = max(1, n_threads // workers)

    def one(group):
        xyz_lows = [torch.tensor(lows[i].astype(np.int32), device=device) for i in group]
        dec = decode_frames_lockstep(model, [list(enc['frames'][i]) for i in group], xyz_lows, per_group, chunk, device_decoder,
                                     None if stored is None else [stored[i] for i in group], [mins[i].tolist() for i in group], group)
        return [d + torch.tensor(mins[i], device=device, dtype=torch.int32) for i, d in zip(group, dec)]

    return [x for out in _map_on_streams(one, groups, workers) for x in out]


def write_gop(enc, result_dir):
    bins = os.path.join(result_dir, 'bins')
    os.makedirs(bins, exist_ok=True)
    for fi, scales in enumerate(enc['frames']):
        for si, b in enumerate(scales):
            with open(os.path.join(bins, 'frame%s_scale%d.bin' % (str(fi).zfill(4), si)), 'wb') as f:
                f.write(b)
    with open(os.path.join(bins, 'model.bin'), 'wb') as f:
        f.write(enc['model_bin'])
    with open(os.path.join(bins, 'low_enc_bytes.bin'), 'wb') as f:
        f.write(enc['low_enc_bytes'])
    if enc.get('digests_bin') is not None:
        with open(os.path.join(bins, 'digests.bin'), 'wb') as f:
            f.write(enc['digests_bin'])
    with open(os.path.join(result_dir, 'side_info.json'), 'w') as f:
        json.dump(enc['side_info'], f, indent=4)


def read_gop(result_dir):
    bins = os.path.join(result_dir, 'bins')
    frames, fi = [], 0
    while True:
        files = glob.glob(os.path.join(bins, 'frame%s_scale*.bin' % str(fi).zfill(4)))
        if not files:
            break
        scales = []
        for si in range(len(files)):
            with open(os.path.join(bins, 'frame%s_scale%d.bin' % (str(fi).zfill(4), si)), 'rb') as f:
                scales.append(f.read())
        frames.append(scales)
        fi += 1
    with open(os.path.join(bins, 'model.bin'), 'rb') as f:
        model_bin = f.read()
    with open(os.path.join(bins, 'low_enc_bytes.bin'), 'rb') as f:
        low = f.read()
    with open(os.path.join(result_dir, 'side_info.json')) as f:
        side = json.load(f)
    digests_bin = None
    if os.path.exists(os.path.join(bins, 'digests.bin')):
        with open(os.path.join(bins, 'digests.bin'), 'rb') as f:
            digests_bin = f.read()
    return {'frames': frames, 'model_bin': model_bin, 'low_enc_bytes': low, 'side_info': side, 'digests_bin': digests_bin}

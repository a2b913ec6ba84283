"""Thin Python wrappers over the C ABI (include/axtrack_hip.h): torch tensors own the device
memory and the stream, the HIP library does the work. Each wrapper names the reference call
it stands in for."""
import ctypes
import os

import numpy as np
import torch

from . import _lib

TILE, S, CELLS = 512, 12, 144
FEATURES = 160 * 16 * 16                # what the first linear layer reads per tile (model.py:50-53)
# Detector.features_frames(block=): floats per item after conv block 7 / 6 / 4
BLOCK_FEATURES = {7: FEATURES, 6: 80 * 16 * 16, 4: 80 * 32 * 32}
# Detector.trunk_features_frames(block=): floats per item after conv block 2 and its pool
TRUNK_FEATURES = {2: 80 * 64 * 64}
CONF_FLOOR = float(np.float32(0.55))   # all_conf_thrs.min() as f32 (AxonDetections.py:76,122)
MAX_PX_ASSOC_DIST = 500                # AxonDetections.py:77
AXON_BOX_SIZE = 70                     # AxonDetections.py:78


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _require_gpu():
    if not torch.cuda.is_available():
        raise _lib.AxtError('axtrack_amd needs a ROCm GPU (MI355X, gfx950); there is no CPU path')


# ConvBlock_i modules of the deployed ARCHITECTURE that hold a convolution (blocks 3, 6, 9 are the max-pools;
# deployed_model/params.txt:34, model.py:85-103)
CONV_BLOCKS = (0, 1, 2, 4, 5, 7, 8, 10)
# per conv block 0..7 of the package's numbering: the side of the square map its convolution writes, and whether one of the
# max-pools follows it (training.ConvTrunkTrainer takes keys, sizes and pools from here)
CONV_MAP_SIDE = (256, 128, 128, 64, 64, 32, 32, 16)
CONV_POOLED = (False, False, True, False, True, False, True, False)
# (input, output) channels per conv block 0..7, and (in, out) of the linear layers fcs.1 / 3 / 5: what the device loads
# (Detector.load_conv_block, load_linear) check their tensors against
CONV_CHANNELS = ((5, 20), (20, 40), (40, 80), (80, 80), (80, 80), (80, 80), (80, 80), (80, 160))
LINEAR_SHAPES = ((FEATURES, 1024), (1024, 1024), (1024, CELLS * 3))


def conv_block_key(i):
    """State-dict prefix of conv block i of the package's numbering (0..7)."""
    return f'ConvNet.ConvBlock_{CONV_BLOCKS[i]}'


def state_dict_tensor_order():
    """Key order axt_detector_create expects (include/axtrack_hip.h)."""
    keys = []
    for name in (f'ConvBlock_{i}' for i in CONV_BLOCKS):
        for k in ('conv.weight', 'conv.bias', 'batchnorm.weight', 'batchnorm.bias',
                  'batchnorm.running_mean', 'batchnorm.running_var'):
            keys.append(f'ConvNet.{name}.{k}')
    for idx in (1, 3, 5):
        keys += [f'fcs.{idx}.weight', f'fcs.{idx}.bias']
    return keys


def _frames_args(frames, tile_yx, t0=0, n_frames=None, device=None):
    """What every entry point that reads a timelapse hands the library: frames checked (a contiguous f32 [T_all, H, W] on
    the GPU; on `device` where one is given) -> (T_all, H, W, n_frames, tile_yx), n_frames defaulting to every detection
    frame from t0 on and tile_yx as contiguous i32 [n_tiles, 2]."""
    if not (isinstance(frames, torch.Tensor) and frames.is_cuda and frames.dim() == 3 and frames.is_contiguous()
            and frames.dtype == torch.float32 and device in (None, frames.device)):
        raise ValueError('frames must be a contiguous f32 tensor [T_all, H, W] on the GPU')
    T_all, H, W = frames.shape
    if n_frames is None:
        n_frames = T_all - 4 - t0
    return T_all, H, W, n_frames, np.ascontiguousarray(tile_yx, np.int32).reshape(-1, 2)


class Detector:
    """Device-resident YOLO_AXTrack (model.py:20-125) in eval mode; `detect_axons` keeps the
    reference's name and tensor contract (model.py:119-125)."""

    ARITH = {'f32': 2, 'f32_winograd': 2, 'f32_direct': 0, 'bf16x3': 1}

    def __init__(self, state_dict, max_batch=256, device='cuda:0', arith='f32'):
        _require_gpu()
        self.device = torch.device(device)
        self.max_batch = int(max_batch)
        lib = _lib.load()
        keep = []
        for k in state_dict_tensor_order():
            if k not in state_dict:
                raise KeyError(f'state_dict lacks {k}')
            v = state_dict[k]
            v = v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)
            keep.append(np.ascontiguousarray(v, np.float32))
        arr = (ctypes.c_void_p * len(keep))(*[a.ctypes.data for a in keep])
        handle = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            _lib.check(lib.axt_detector_create(arr, len(keep), self.max_batch, ctypes.byref(handle)),
                       'axt_detector_create')
        self._h = handle
        self._lib = lib
        self.state_dict_source = state_dict     # training.fine_tune_head starts the linear head from these tensors
        self.arith = 'f32'              # axt_detector_create leaves the handle in its default mode (f32 Winograd)
        self.fused_front = os.environ.get('AXT_FUSE_S2', '1') != '0'     # what axt_detector_create read
        self.set_arith(arith)

    def set_arith(self, arith):
        """Arithmetic of the stride-1 conv blocks (parameters['CNN_ARITH']): 'f32' (default; the
        same as 'f32_winograd': Winograd F(2x2,3x3) on the f32 matrix pipe, every operation f32), 'f32_direct' (direct
        convolution on the f32 matrix pipe: a k-ordered chain of f32 FMAs) or 'bf16x3' (opt-in: operands split into three
        bf16 terms, six partial products on the bf16 matrix pipe, f32 accumulation). See axt_detector_set_arith."""
        if arith not in self.ARITH:
            raise ValueError(f"CNN_ARITH must be one of {sorted(self.ARITH)}, got {arith!r}")
        if self.ARITH[arith] != self.ARITH[self.arith]:
            with torch.cuda.device(self.device):
                _lib.check(self._lib.axt_detector_set_arith(self._h, self.ARITH[arith]), 'axt_detector_set_arith')
        self.arith = arith

    def set_fused_front(self, fused):
        """The two stride-2 conv blocks as one kernel that keeps block 0's output in LDS (default) or as the two separate
        kernels (axt_detector_set_fused_front): the grids agree to f32 rounding, not bit for bit."""
        _lib.check(self._lib.axt_detector_set_fused_front(self._h, 1 if fused else 0), 'axt_detector_set_fused_front')
        self.fused_front = bool(fused)

    def __del__(self):
        h, self._h = getattr(self, '_h', None), None
        if h:
            self._lib.axt_detector_destroy(h)

    def _check_device_tensors(self, what, tensors, shapes):
        """Everything a device load asks of its tensors, before any launch: contiguous f32 CUDA tensors of these shapes on
        the detector's device."""
        for (name, t), shape in zip(tensors, shapes):
            if not isinstance(t, torch.Tensor):
                raise TypeError(f'{what}: {name} must be a torch tensor on {self.device}, got {type(t).__name__}')
            if t.device != self.device:
                raise ValueError(f'{what}: {name} is on {t.device}, the detector on {self.device}')
            if t.dtype != torch.float32:
                raise ValueError(f'{what}: {name} must be float32, got {t.dtype}')
            if tuple(t.shape) != tuple(shape):
                raise ValueError(f'{what}: {name} must have shape {tuple(shape)}, got {tuple(t.shape)}')
            if not t.is_contiguous():
                raise ValueError(f'{what}: {name} must be contiguous')

    def load_conv_block(self, i, weight, bias, bn_weight, bn_bias, running_mean, running_var):
        """Replace conv block i (0..7 of the package's numbering) by these tensors of the state-dict layout -- conv.weight
        [Co, Ci, 3, 3] and conv.bias, batchnorm.weight, batchnorm.bias, running_mean, running_var [Co], contiguous f32 on
        the detector's device -- without leaving the device (axt_detector_load_conv_block): BatchNorm is folded and every
        packed image the block has is rewritten by kernels, on the current stream. The detector then computes, byte for
        byte, what one created from the same tensors computes, in every arithmetic. state_dict_source becomes None."""
        if isinstance(i, bool) or not isinstance(i, (int, np.integer)) or not 0 <= i < len(CONV_BLOCKS):
            raise IndexError(f'conv block must be in 0..{len(CONV_BLOCKS) - 1}, got {i!r}')
        ci, co = CONV_CHANNELS[i]
        names = ('weight', 'bias', 'bn_weight', 'bn_bias', 'running_mean', 'running_var')
        tensors = (weight, bias, bn_weight, bn_bias, running_mean, running_var)
        self._check_device_tensors(f'load_conv_block({i})', zip(names, tensors), [(co, ci, 3, 3)] + [(co,)] * 5)
        with torch.cuda.device(self.device):
            _lib.check(self._lib.axt_detector_load_conv_block(self._h, int(i), *[t.data_ptr() for t in tensors], _stream()),
                       'axt_detector_load_conv_block')
        self.state_dict_source = None

    def load_linear(self, layer, weight, bias):
        """Replace linear layer 0..2 (fcs.1, fcs.3, fcs.5) by weight [out, in] and bias [out], contiguous f32 on the
        detector's device, without leaving the device (axt_detector_load_linear): a tiled transpose into the GEMM's
        layout on the current stream. state_dict_source becomes None."""
        if isinstance(layer, bool) or not isinstance(layer, (int, np.integer)) or not 0 <= layer < 3:
            raise IndexError(f'linear layer must be in 0..2, got {layer!r}')
        fin, fout = LINEAR_SHAPES[layer]
        self._check_device_tensors(f'load_linear({layer})', zip(('weight', 'bias'), (weight, bias)), [(fout, fin), (fout,)])
        with torch.cuda.device(self.device):
            _lib.check(self._lib.axt_detector_load_linear(self._h, int(layer), weight.data_ptr(), bias.data_ptr(), _stream()),
                       'axt_detector_load_linear')
        self.state_dict_source = None

    def load_state_dict(self, sd):
        """load_conv_block for the eight conv blocks and load_linear for the three linear layers from a state dict whose
        tensors are already on the detector's device (contiguous f32): no host copy. Every tensor is checked before the
        first launch."""
        keys = state_dict_tensor_order()
        for k in keys:
            if k not in sd:
                raise KeyError(f'state_dict lacks {k}')
        conv = [[sd[k] for k in keys[6 * i:6 * i + 6]] for i in range(len(CONV_BLOCKS))]
        fcs = [[sd[k] for k in keys[48 + 2 * l:50 + 2 * l]] for l in range(3)]
        names = ('weight', 'bias', 'bn_weight', 'bn_bias', 'running_mean', 'running_var')
        for i, t in enumerate(conv):
            ci, co = CONV_CHANNELS[i]
            self._check_device_tensors(f'load_state_dict: conv block {i}', zip(names, t), [(co, ci, 3, 3)] + [(co,)] * 5)
        for l, t in enumerate(fcs):
            fin, fout = LINEAR_SHAPES[l]
            self._check_device_tensors(f'load_state_dict: linear {l}', zip(names, t), [(fout, fin), (fout,)])
        for i, t in enumerate(conv):
            self.load_conv_block(i, *t)
        for l, t in enumerate(fcs):
            self.load_linear(l, *t)

    @property
    def device_bytes(self):
        return int(self._lib.axt_detector_device_bytes(self._h))

    KERNEL_NAMES = ['conv0 5>20 s2', 'conv1 20>40 s2', 'conv2 40>80 +pool', 'conv4 80>80', 'conv5 80>80 +pool',
                    'conv7 80>80', 'conv8 80>80 +pool', 'conv10 80>160', 'fc1 gemm', 'fc1 reduce', 'fc2 gemm',
                    'fc2 reduce', 'fc3 gemm', 'fc3 reduce']

    def set_profiling(self, on, only=None):
        """Bracket the forward pass's kernel launches with HIP events: all of them, or only kernel index `only`."""
        mode = 0 if not on else (1 if only is None else 2 + int(only))
        _lib.check(self._lib.axt_detector_set_profiling(self._h, mode), 'axt_detector_set_profiling')

    def read_profile(self):
        """Per-kernel HIP-event times since the last read: list of dicts (name, ms, launches, tiles, flops_per_tile)."""
        n = len(self.KERNEL_NAMES)
        ms = np.zeros(n, np.float64)
        launches = np.zeros(n, np.int64)
        items = np.zeros(n, np.int64)
        _lib.check(self._lib.axt_detector_read_profile(self._h, ms.ctypes.data, launches.ctypes.data,
                                                       items.ctypes.data, n), 'axt_detector_read_profile')
        rows = [dict(name=self.KERNEL_NAMES[i], ms=float(ms[i]), launches=int(launches[i]), tiles=int(items[i]),
                     flops_per_tile=float(self._lib.axt_cnn_kernel_flops_per_tile(i))) for i in range(n)]
        if rows[0]['launches'] and not rows[1]['launches']:
            # the fused front kernel is bracketed as kernel 0 and does the work of kernels 0 and 1 (row 1 stays, empty)
            rows[0]['name'] = 'conv0+1 5>20>40 s2 fused'
            rows[0]['flops_per_tile'] += rows[1]['flops_per_tile']
        return rows

    def eval(self):
        return self

    def train(self, mode=True):
        return self

    def to(self, device):
        if torch.device(device) != self.device:
            raise _lib.AxtError('the detector is bound to the device it was created on')
        return self

    def detect_axons(self, X):
        """X f32 [B,5,512,512] on the GPU -> [B,12,12,3] (model.py:119-125)."""
        if X.dim() != 4 or tuple(X.shape[1:]) != (5, TILE, TILE):
            raise ValueError(f'expected [B,5,{TILE},{TILE}], got {tuple(X.shape)}')
        X = X.to(self.device, torch.float32).contiguous()
        out = torch.empty((X.shape[0], S, S, 3), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self._lib.axt_cnn_forward(self._h, X.data_ptr(), X.shape[0], out.data_ptr(), _stream()),
                       'axt_cnn_forward')
        return out

    def detect_frames(self, frames, tile_yx, t0=0, n_frames=None):
        """frames f32 [T_all,H,W] on the GPU -> YOLO grids [n_frames, n_tiles, 12,12,3] for detection
        frames t0..t0+n_frames-1 (get_frametiles_stack + detect_axons, AxonDetections.py:115-118)."""
        T_all, H, W, n_frames, tile_yx = _frames_args(frames, tile_yx, t0, n_frames, self.device)
        out = torch.empty((n_frames, len(tile_yx), S, S, 3), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self._lib.axt_cnn_forward_frames(self._h, frames.data_ptr(), T_all, H, W, t0, n_frames,
                                                        tile_yx.ctypes.data, len(tile_yx), out.data_ptr(), _stream()),
                       'axt_cnn_forward_frames')
        return out


    def features_frames(self, frames, tile_yx, t0=0, n_frames=None, out=None, block=7):
        """The frozen trunk of detect_frames: frames f32 [T_all,H,W] on the GPU -> [n_frames * n_tiles, 40960], the input of
        the first linear layer per (frame, tile) item in the flatten order of model.py:50-53 (axt_cnn_features_frames).
        What training.HeadTrainer trains on. out: a contiguous f32 table of at least that many rows to write into (its
        first n_frames * n_tiles rows are returned) instead of a new one. block=6: the trunk one conv block earlier,
        [n_frames * n_tiles, 20480] = [item, 80, 16, 16], what training.ConvBlockTrainer reads
        (axt_cnn_block_features_frames); block=4: three conv blocks earlier, [n_frames * n_tiles, 81920] = [item, 80, 32, 32],
        what a training.ConvTrunkTrainer from conv block 5 on (ConvStageTrainer) reads; block=7 is the default table."""
        if block not in BLOCK_FEATURES:
            raise ValueError(f'block must be one of {sorted(BLOCK_FEATURES)}, got {block}')
        return self._block_table(frames, tile_yx, t0, n_frames, out, block, BLOCK_FEATURES[block])

    def trunk_features_frames(self, frames, tile_yx, block=2, t0=0, n_frames=None, out=None):
        """features_frames for the taps in front of the last stage: block=2 -> [n_frames * n_tiles, 327680] =
        [item, 80, 64, 64], conv block 2's output after its pool, the bytes of the detector's own buffer
        (axt_cnn_block_features_frames); conv blocks 3..7 do not run. What training.ConvTrunkTrainer(first_block=3) reads.
        The widths are TRUNK_FEATURES; frames, tile_yx, t0, n_frames and out as features_frames takes them."""
        if block not in TRUNK_FEATURES:
            raise ValueError(f'block must be one of {sorted(TRUNK_FEATURES)}, got {block}')
        return self._block_table(frames, tile_yx, t0, n_frames, out, block, TRUNK_FEATURES[block])

    def _block_table(self, frames, tile_yx, t0, n_frames, out, block, width):
        T_all, H, W, n_frames, tile_yx = _frames_args(frames, tile_yx, t0, n_frames, self.device)
        n_items = n_frames * len(tile_yx)
        if out is None:
            out = torch.empty((n_items, width), dtype=torch.float32, device=self.device)
        else:
            if not (out.is_contiguous() and out.dtype == torch.float32 and out.device == self.device and out.dim() == 2
                    and out.shape[1] == width and out.shape[0] >= n_items):
                raise ValueError(f'out must be a contiguous f32 table [>= {n_items}, {width}] on {self.device}')
            out = out[:n_items]
        with torch.cuda.device(self.device):
            if block == 7:
                _lib.check(self._lib.axt_cnn_features_frames(self._h, frames.data_ptr(), T_all, H, W, t0, n_frames,
                                                             tile_yx.ctypes.data, len(tile_yx), out.data_ptr(), _stream()),
                           'axt_cnn_features_frames')
            else:
                _lib.check(self._lib.axt_cnn_block_features_frames(self._h, frames.data_ptr(), T_all, H, W, t0, n_frames,
                                                                   tile_yx.ctypes.data, len(tile_yx), int(block),
                                                                   out.data_ptr(), _stream()),
                           'axt_cnn_block_features_frames')
        return out

    def front_frames(self, frames, tile_yx, t0, n_frames, item0):
        """Conv blocks 0-5 of detection frames t0 .. t0+n_frames-1 into the detector's batch buffer from item `item0`
        (axt_cnn_front_frames): input that arrives in chunks. back() finishes the pass for all items at once."""
        T_all, H, W, n_frames, tile_yx = _frames_args(frames, tile_yx, t0, n_frames, self.device)
        with torch.cuda.device(self.device):
            _lib.check(self._lib.axt_cnn_front_frames(self._h, frames.data_ptr(), T_all, H, W, t0, n_frames, tile_yx.ctypes.data,
                                                      len(tile_yx), int(item0), _stream()), 'axt_cnn_front_frames')

    def back(self, n_frames, n_tiles):
        """The rest of the forward pass for items 0 .. n_frames*n_tiles-1 of the batch buffer -> [n_frames, n_tiles, 12,12,3]."""
        out = torch.empty((n_frames, n_tiles, S, S, 3), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self._lib.axt_cnn_back(self._h, n_frames * n_tiles, out.data_ptr(), _stream()), 'axt_cnn_back')
        return out


def tile_stacks(frames, tile_yx, index, out=None):
    """The raw 5-frame stacks of a batch of (frame, tile) items, the input of conv block 0 (axt_tile_stacks): frames f32
    [T_all, H, W] on the GPU, index: item numbers frame * n_tiles + tile in the order of Detector.features_frames (an i32
    tensor on the GPU, or host integers, which are checked) -> f32 [B, 5, 512, 512]: channel c of item (f, k) is frame f + c,
    from the tile's origin, +0.0 beyond H or W. out: a contiguous f32 tensor of at least B stacks to write into."""
    _require_gpu()
    T_all, H, W, n_frames, tile_yx = _frames_args(frames, tile_yx)
    if n_frames < 1:
        raise ValueError(f'{T_all} frames hold no stack of 5')
    if isinstance(index, torch.Tensor):
        index = index.to(frames.device, torch.int32).contiguous().reshape(-1)
    else:
        index = np.ascontiguousarray(index, np.int64).reshape(-1)
        if ((index < 0) | (index >= n_frames * len(tile_yx))).any():
            raise IndexError(f'item outside the {n_frames * len(tile_yx)} of {n_frames} frames x {len(tile_yx)} tiles')
        index = torch.from_numpy(index.astype(np.int32)).to(frames.device)
    B = len(index)
    if out is None:
        out = torch.empty((B, 5, TILE, TILE), dtype=torch.float32, device=frames.device)
    elif not (out.is_contiguous() and out.dtype == torch.float32 and out.device == frames.device
              and out.numel() >= B * 5 * TILE * TILE):
        raise ValueError(f'out must be a contiguous f32 tensor of at least [{B}, 5, {TILE}, {TILE}] on {frames.device}')
    else:
        out = out.reshape(-1)[:B * 5 * TILE * TILE].view(B, 5, TILE, TILE)
    with torch.cuda.device(frames.device):
        _lib.check(_lib.load().axt_tile_stacks(frames.data_ptr(), T_all, H, W, 0, n_frames, tile_yx.ctypes.data, len(tile_yx),
                                               index.data_ptr(), B, out.data_ptr(), _stream()), 'axt_tile_stacks')
    return out


def preprocess_u16(raw, mask=None, offset=0.0, clip_lower=0.0, log_correct=True, scale=1.0, out=None):
    """Fused dense preprocessing (Timelapse.py:205-326) of a raw uint16 timelapse that already sits on the GPU.
    raw: torch.uint16 (or int16-viewed) [T,H,W]; mask: uint8/bool [H,W] on the same device or None; out: optional
    contiguous f32 [T,H,W] to write into (a slice of the timelapse's frame buffer when the input arrives in chunks)."""
    T, H, W = raw.shape
    assert raw.is_contiguous() and raw.element_size() == 2
    if out is None:
        out = torch.empty((T, H, W), dtype=torch.float32, device=raw.device)
    assert out.is_contiguous() and out.dtype == torch.float32 and tuple(out.shape) == (T, H, W) and out.device == raw.device
    if mask is not None:
        mask = mask.to(device=raw.device, dtype=torch.uint8).contiguous()
    lib = _lib.load()
    with torch.cuda.device(raw.device):
        _lib.check(lib.axt_preprocess_u16(raw.data_ptr(), _lib.dptr(mask), T, H, W, ctypes.c_float(offset),
                                          ctypes.c_float(clip_lower), int(bool(log_correct)), ctypes.c_float(scale),
                                          out.data_ptr(), _stream()), 'axt_preprocess_u16')
    return out


# axt_frame_stats (include/axtrack_hip.h): one 32-byte record per frame
FRAME_STATS_DTYPE = np.dtype([('n', np.int64), ('sum', np.float64), ('sumsq', np.float64), ('max', np.float32),
                              ('reserved', np.float32)])


def preprocess_stats_u16(raw, mask=None, offset=0.0, clip_lower=0.0, log_correct=True):
    """Per-frame (n, sum, sumsq, max) of the values preprocess_u16 would write with scale=1, without writing them: what
    Timelapse._standardize measures before it scales (Timelapse.py:286-302). raw, mask as in preprocess_u16.
    -> numpy record array [T] of FRAME_STATS_DTYPE on the host (the call waits for the result)."""
    T, H, W = raw.shape
    assert raw.is_contiguous() and raw.element_size() == 2
    if mask is not None:
        mask = mask.to(device=raw.device, dtype=torch.uint8).contiguous()
    lib = _lib.load()
    args = (T, H, W, ctypes.c_float(offset), ctypes.c_float(clip_lower), int(bool(log_correct)))
    need = ctypes.c_size_t(0)
    _lib.check(lib.axt_preprocess_stats_u16(None, None, *args, None, None, ctypes.byref(need), None),
               'axt_preprocess_stats_u16 (scratch size)')
    scratch = torch.empty(need.value, dtype=torch.uint8, device=raw.device)
    stats = torch.empty(T * FRAME_STATS_DTYPE.itemsize, dtype=torch.uint8, device=raw.device)
    with torch.cuda.device(raw.device):
        _lib.check(lib.axt_preprocess_stats_u16(raw.data_ptr(), _lib.dptr(mask), *args, stats.data_ptr(),
                                                scratch.data_ptr(), ctypes.byref(need), _stream()),
                   'axt_preprocess_stats_u16')
    return stats.cpu().numpy().view(FRAME_STATS_DTYPE)


def preprocess_u16_framewise(raw, scale, mask=None, offset=0.0, clip_lower=0.0, log_correct=True, out=None):
    """preprocess_u16 with one scale per frame (STANDARDIZE_FRAMEWISE, Timelapse.py:309-312). scale: T positive finite
    numbers (host array or tensor); a scale that is not would put inf / NaN into a frame and is refused here."""
    T, H, W = raw.shape
    assert raw.is_contiguous() and raw.element_size() == 2
    sc = np.ascontiguousarray(scale.detach().cpu().numpy() if isinstance(scale, torch.Tensor) else scale, np.float32)
    if sc.shape != (T,):
        raise ValueError(f'{T} frames need {T} scales, got an array of shape {sc.shape}')
    if not (np.isfinite(sc) & (sc > 0)).all():
        raise ValueError(f'frame scales must be finite and > 0; frames {np.flatnonzero(~(np.isfinite(sc) & (sc > 0))).tolist()} are not')
    if out is None:
        out = torch.empty((T, H, W), dtype=torch.float32, device=raw.device)
    assert out.is_contiguous() and out.dtype == torch.float32 and tuple(out.shape) == (T, H, W) and out.device == raw.device
    if mask is not None:
        mask = mask.to(device=raw.device, dtype=torch.uint8).contiguous()
    d_scale = torch.from_numpy(sc).to(raw.device)
    lib = _lib.load()
    with torch.cuda.device(raw.device):
        _lib.check(lib.axt_preprocess_u16_framewise(raw.data_ptr(), _lib.dptr(mask), T, H, W, ctypes.c_float(offset),
                                                    ctypes.c_float(clip_lower), int(bool(log_correct)), d_scale.data_ptr(),
                                                    out.data_ptr(), _stream()), 'axt_preprocess_u16_framewise')
    return out


def tile_occupancy_bytes(frames):
    """Per-tile occupancy of this block of frames as a device u8 tensor [tile_rows * tile_cols] (1 = some pixel of
    the tile is non-zero at some time point)."""
    T_all, H, W = frames.shape
    nty, ntx = -(-H // TILE), -(-W // TILE)
    occ = torch.empty(nty * ntx, dtype=torch.uint8, device=frames.device)
    lib = _lib.load()
    with torch.cuda.device(frames.device):
        _lib.check(lib.axt_tile_occupancy(frames.data_ptr(), T_all, H, W, occ.data_ptr(), _stream()),
                   'axt_tile_occupancy')
    return occ


def tile_list(occ, H, W):
    """Occupancy bytes -> row-major list of kept (tile_row, tile_col)."""
    nty, ntx = -(-H // TILE), -(-W // TILE)
    occ = occ.cpu().numpy().reshape(nty, ntx)
    return [tuple(int(v) for v in ix) for ix in np.argwhere(occ)]


def tile_occupancy(frames):
    """Kept tiles, row-major list of (tile_row, tile_col) (Timelapse.py:551-558)."""
    return tile_list(tile_occupancy_bytes(frames), frames.shape[1], frames.shape[2])


def decode_stitch_nms(yolo, tile_yx, conf_thr=CONF_FLOOR, min_dist=23, cap=None):
    """_yolo_Y2pandas_det + stitch_tiles + _non_max_supression per frame
    (AxonDetections.py:122-128). yolo [n_frames, n_tiles, 12,12,3] on the GPU.
    Returns device tensors conf f32 [F,cap], x i32, y i32, count i32 [F]."""
    n_frames, n_tiles = yolo.shape[0], yolo.shape[1]
    tile_yx = np.ascontiguousarray(tile_yx, np.int32).reshape(-1, 2)
    assert len(tile_yx) == n_tiles and yolo.is_contiguous()
    cap = cap or n_tiles * CELLS
    dev = yolo.device
    # one zeroed block for the four outputs (one fill launch instead of four; slots beyond a frame's count stay zero)
    slots = n_frames * cap
    sec = (slots + 63) // 64 * 64                        # every output starts 256-byte aligned, like a tensor of its own
    block = torch.zeros((3 * sec + n_frames,), dtype=torch.int32, device=dev)
    conf = block[:slots].view(torch.float32).view(n_frames, cap)
    x = block[sec:sec + slots].view(n_frames, cap)
    y = block[2 * sec:2 * sec + slots].view(n_frames, cap)
    count = block[3 * sec:]
    lib = _lib.load()
    with torch.cuda.device(dev):
        _lib.check(lib.axt_decode_stitch_nms(yolo.data_ptr(), n_frames, n_tiles, tile_yx.ctypes.data,
                                             ctypes.c_float(conf_thr), int(min_dist), cap, conf.data_ptr(),
                                             x.data_ptr(), y.data_ptr(), count.data_ptr(), _stream()),
                   'axt_decode_stitch_nms')
    return conf, x, y, count


def obs_costs(conf, count, method='scale_to_max', max_conf_cost=4.6):
    """conf capping + observation_model (AxonDetections.py:655-659, mincostflow_models.py:6-27)."""
    n_frames, cap = conf.shape
    cost = torch.zeros((n_frames, cap), dtype=torch.float64, device=conf.device)
    m = {'scale_to_max': 0, 'ceil': 1}[method]
    lib = _lib.load()
    with torch.cuda.device(conf.device):
        _lib.check(lib.axt_obs_costs(conf.data_ptr(), count.data_ptr(), n_frames, cap, m, float(max_conf_cost),
                                     cost.data_ptr(), _stream()), 'axt_obs_costs')
    return cost


class Grid:
    """Masked grid handle (axt_grid): byte mask, bit rows and connected-component labels on the GPU."""

    def __init__(self, mask, conn8=False, device='cuda:0'):
        _require_gpu()
        m = np.ascontiguousarray(np.asarray(mask) == 1, np.uint8)
        self.H, self.W, self.conn8 = int(m.shape[0]), int(m.shape[1]), bool(conn8)
        self._lib = _lib.load()
        h = ctypes.c_void_p()
        with torch.cuda.device(torch.device(device)):
            _lib.check(self._lib.axt_grid_create(m.ctypes.data, self.H, self.W, int(self.conn8), ctypes.byref(h)),
                       'axt_grid_create')
        self._h = h

    def __del__(self):
        h, self._h = getattr(self, '_h', None), None
        if h:
            self._lib.axt_grid_destroy(h)


def _as_grid(mask, conn8, device):
    """A mask argument (None = all ones, a Grid, or an array / tensor [H, W]) -> None or a Grid on `device`."""
    if mask is None or isinstance(mask, Grid):
        return mask
    return Grid(mask.cpu().numpy() if isinstance(mask, torch.Tensor) else mask, conn8, device)


def path_cost(xa, ya, xb, yb, H, W, mask=None, max_dist=MAX_PX_ASSOC_DIST, conn8=False):
    """A* path-length matrix of one frame pair (AxonDetections.py:526-629,717-752)."""
    na, nb = xa.numel(), xb.numel()
    D = torch.empty((na, nb), dtype=torch.int32, device=xa.device)
    lib = _lib.load()
    mask = _as_grid(mask, conn8, xa.device)
    with torch.cuda.device(xa.device):
        _lib.check(lib.axt_path_cost(xa.data_ptr(), ya.data_ptr(), na, xb.data_ptr(), yb.data_ptr(), nb,
                                     mask._h if mask is not None else None, H, W, int(max_dist), int(bool(conn8)),
                                     D.data_ptr(), _stream()), 'axt_path_cost')
    return D


def path_cells(xa, ya, xb, yb, H, W, mask, max_dist=MAX_PX_ASSOC_DIST, conn8=False):
    """The A* paths of one frame pair on a masked grid (utils.py:379-387): (D i32 [na,nb], cells i32 [na,nb,max_dist]),
    cells[i,j,:D[i,j]] = y*W + x along one minimum-cost path, source first, for the pairs with D < max_dist."""
    na, nb = xa.numel(), xb.numel()
    D = torch.empty((na, nb), dtype=torch.int32, device=xa.device)
    cells = torch.full((na, nb, int(max_dist)), -1, dtype=torch.int32, device=xa.device)
    mask = _as_grid(mask, conn8, xa.device)
    with torch.cuda.device(xa.device):
        _lib.check(_lib.load().axt_path_cells(xa.data_ptr(), ya.data_ptr(), na, xb.data_ptr(), yb.data_ptr(), nb, mask._h,
                                              H, W, int(max_dist), int(bool(conn8)), D.data_ptr(), cells.data_ptr(),
                                              _stream()), 'axt_path_cells')
    return D, cells


def box_histograms(frames, x, y, count, t_offset=2, box=AXON_BOX_SIZE):
    """feature_model (mincostflow_models.py:30-65) for every detection: (hist f32 [F,cap,180], bin sums f64 [F,cap]).
    frames f32 [T_all,H,W] on the GPU; detection frame f is shown frame f + t_offset (its centre frame)."""
    n_frames, cap = x.shape
    T_all, H, W = frames.shape
    hist = torch.zeros((n_frames, cap, 180), dtype=torch.float32, device=x.device)
    hsum = torch.zeros((n_frames, cap), dtype=torch.float64, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().axt_box_histograms(frames.data_ptr(), T_all, H, W, int(t_offset), x.data_ptr(), y.data_ptr(),
                                                  count.data_ptr(), n_frames, cap, int(box), hist.data_ptr(),
                                                  hsum.data_ptr(), _stream()), 'axt_box_histograms')
    return hist, hsum


def build_arcs(x, y, count, H, W, dmax, cost_units=None, mask=None, max_dist=MAX_PX_ASSOC_DIST, conn8=False, vis=None,
               length_table=None, src_count=None):
    """Admissible transition arcs of the whole timelapse, CSR by tail detection (global numbering).
    cost_units: optional int64 [max_gap, max_dist+1] = round(transition cost * 1e6) per (gap, D).
    vis: None, or dict(hist, hsum, weight, miss_rate, thr) -- the appearance term (MCF_VIS_SIM_WEIGHT > 0): costs
    are then computed per pair on the GPU and cost_units is ignored.
    length_table: None, or i16 device tensor [F, cap, max_gap, cap] of precomputed path lengths (<= 0: none), e.g.
    from a path cache written by the reference; mask is then ignored.
    src_count: None, or i32 [F]: build rows only for the first src_count[t] detections of frame t (a frame-sharded
    rank: its own frames' counts, zeros elsewhere); numbering and costs stay those of the whole timelapse.
    Returns device tensors (row_ptr i64 [n_frames*cap+1], col i32, length i16, gap u8, cost i64|None)."""
    n_frames, cap = x.shape
    max_gap = len(dmax)
    dev = x.device
    h_dmax = np.ascontiguousarray(dmax, np.int32)
    row_ptr = torch.empty((n_frames * cap + 1,), dtype=torch.int64, device=dev)
    n_work = n_frames * cap * max_gap + n_frames + 1 + max_gap + 4
    if length_table is not None:
        assert tuple(length_table.shape) == (n_frames, cap, max_gap, cap) and length_table.dtype == torch.int16
        mask = None
    mask = _as_grid(mask, conn8, dev)
    if mask is not None:
        n_work += (n_frames * cap * max_gap * cap + 1) // 2
    work = torch.empty((n_work,), dtype=torch.int32, device=dev)
    n_arcs = ctypes.c_int64(0)
    lib = _lib.load()
    hist, hsum, weight, miss_rate, thr = (None, None, 0.0, 0.0, 0.0) if vis is None else (
        vis['hist'], vis['hsum'], vis['weight'], vis['miss_rate'], vis['thr'])

    def call(col, length, gap, cu, cost, what):
        rc = lib.axt_build_arcs(x.data_ptr(), y.data_ptr(), count.data_ptr(), _lib.dptr(src_count), n_frames, cap,
                                mask._h if mask is not None else None, H, W, int(max_dist), int(bool(conn8)), max_gap,
                                h_dmax.ctypes.data, _lib.dptr(hist), _lib.dptr(hsum), float(weight), float(miss_rate),
                                float(thr), row_ptr.data_ptr(), work.data_ptr(), _lib.dptr(col), _lib.dptr(length), _lib.dptr(gap),
                                _lib.dptr(cu), _lib.dptr(cost), ctypes.byref(n_arcs), _lib.dptr(length_table), _stream())
        _lib.check(rc, f'axt_build_arcs({what})')

    with torch.cuda.device(dev):
        call(None, None, None, None, None, 'count')
        n = max(int(n_arcs.value), 1)
        col = torch.empty((n,), dtype=torch.int32, device=dev)
        length = torch.empty((n,), dtype=torch.int16, device=dev)
        gap = torch.empty((n,), dtype=torch.uint8, device=dev)
        cost = cu = None
        if vis is not None:
            cost = torch.empty((n,), dtype=torch.int64, device=dev)
        elif cost_units is not None:
            cu = cost_units if isinstance(cost_units, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(cost_units, np.int64)).to(dev)
            assert cu.shape == (max_gap, max_dist + 1)
            cost = torch.empty((n,), dtype=torch.int64, device=dev)
        call(col, length, gap, cu, cost, 'fill')
    n = int(n_arcs.value)
    return row_ptr, col[:n], length[:n], gap[:n], (cost[:n] if cost is not None else None)


HUNGARIAN_NO_LINK = 0x3fffffffffffffff          # entry of a cost table where a link is not admitted


def hungarian_assoc(x, y, count, H, W, dmax, cost_units, thr_units, max_dist=MAX_PX_ASSOC_DIST, conn8=False,
                    frame_range=None, group=None, mask=None, ctab=None):
    """Frame-to-frame Hungarian association (BASELINE config 3) of a whole timelapse on the GPU.
    frame_range=(a, b): this rank solves only the pairs of source frames a..b-1; the link arrays are then
    combined over `group` with one MAX all-reduce and every rank numbers the chains (frame-sharded runs).
    mask: None (all-ones) or a Grid: path lengths then come from the masked-grid searches of the arc builder.
    ctab: optional i64 device tensor [F, cap, len(dmax), cap] of link costs (HUNGARIAN_NO_LINK where not admitted), used
    instead of the costs derived from the path lengths (d_ctab of axt_hungarian_pairs; the appearance term).
    Returns (track i32 [F,cap] device tensor, n_tracks device tensor [1])."""
    n_frames, cap = x.shape
    max_gap = len(dmax)
    dev = x.device
    h_dmax = np.ascontiguousarray(dmax, np.int32)
    cu = cost_units if isinstance(cost_units, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(cost_units, np.int64)).to(dev)
    slots = n_frames * cap
    pred = torch.empty((2 * slots,), dtype=torch.int32, device=dev)
    work = torch.empty((2 * slots + n_frames + 1,), dtype=torch.int32, device=dev)
    track = torch.empty((n_frames, cap), dtype=torch.int32, device=dev)
    n_tracks = torch.empty((1,), dtype=torch.int32, device=dev)       # (axt_chain_tracks always writes it)
    a, b = (0, n_frames) if frame_range is None else frame_range
    lib = _lib.load()
    with torch.cuda.device(dev):
        if ctab is not None and (ctab.dtype != torch.int64 or tuple(ctab.shape) != (n_frames, cap, max_gap, cap)
                                 or not ctab.is_contiguous()):
            raise ValueError(f'ctab must be a contiguous int64 tensor [{n_frames}, {cap}, {max_gap}, {cap}]')
        _lib.check(lib.axt_hungarian_pairs(x.data_ptr(), y.data_ptr(), count.data_ptr(), n_frames, cap,
                                           mask._h if mask is not None else None, H, W, int(max_dist), int(bool(conn8)),
                                           max_gap, h_dmax.ctypes.data, cu.data_ptr(), int(thr_units), int(a), int(b),
                                           pred.data_ptr(), work.data_ptr(), _stream(), _lib.dptr(ctab)), 'axt_hungarian_pairs')
        if frame_range is not None:
            import torch.distributed as dist
            from . import sharded
            sharded._collective('hungarian_links_allreduce', lambda: dist.all_reduce(pred, op=dist.ReduceOp.MAX, group=group))
        _lib.check(lib.axt_chain_tracks(count.data_ptr(), n_frames, cap, pred.data_ptr(), work.data_ptr(),
                                        track.data_ptr(), n_tracks.data_ptr(), _stream()), 'axt_chain_tracks')
    return track, n_tracks


def ided_table(track, conf, x, y, count, n_ids, label_quirk=True, id_row=None, n_rows=None):
    """IDed_dets_all's values (AxonDetections.py:825-842) as a pinned host f64 array [n_rows, 3*F]: filled on the
    GPU (axt_ided_table), copied across once. id_row: optional i32 device tensor id -> row for ids with gaps.
    Returns (array, wait): the copy is asynchronous, wait() returns when the array holds the table."""
    n_frames, cap = x.shape
    dev = x.device
    n_rows = int(n_ids if n_rows is None else n_rows)
    table = torch.empty((n_rows, 3 * n_frames), dtype=torch.float64, device=dev)
    work = torch.empty((n_frames,), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().axt_ided_table(track.data_ptr(), conf.data_ptr(), x.data_ptr(), y.data_ptr(),
                                              count.data_ptr(), n_frames, cap, int(n_ids),
                                              id_row.data_ptr() if id_row is not None else None, n_rows,
                                              int(bool(label_quirk)), work.data_ptr(), table.data_ptr(), _stream()),
                   'axt_ided_table')
    host = torch.empty(table.shape, dtype=torch.float64, pin_memory=True)
    host.copy_(table, non_blocking=True)             # the caller wraps the array while the copy is in flight ...
    return host.numpy(), torch.cuda.current_stream(dev).synchronize       # ... and calls this before handing it on


def track_links(track, count, max_gap):
    """The links of the tracks (what the reference's unbuilt _reconstruct_axons starts from, AxonDetections.py:924-934):
    track i32 [F, cap] (-1 = none) -> i32 device tensor [n_links, 3] of (tail slot f*cap+i, head slot, gap), the head
    being the first detection of the same id within max_gap frames, in ascending tail order (axt_track_links)."""
    n_frames, cap = track.shape
    dev = track.device
    links = torch.empty((max(n_frames * cap, 1), 3), dtype=torch.int32, device=dev)
    work = torch.empty((2 * n_frames * cap + 2 * n_frames + 1,), dtype=torch.int32, device=dev)
    n = ctypes.c_int64(0)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().axt_track_links(track.data_ptr(), count.data_ptr(), n_frames, cap, int(max_gap), links.data_ptr(),
                                               work.data_ptr(), ctypes.byref(n), _stream()), 'axt_track_links')
    return links[:int(n.value)]


def link_paths(links, x, y, H, W, grids, head_group=None, max_dist=MAX_PX_ASSOC_DIST, conn8=False, max_gap=2):
    """One minimum-cost path per link (axt_link_paths + axt_link_cells): the cells path_cells (masked grid) or the
    closed-form staircase of astar_dets_paths (all-ones mask) gives for that pair. grids: list of Grid / None (all ones),
    one per distinct mask; head_group: None (one grid) or i32 [F] device tensor, the grid of the links that end in frame f.
    Returns device tensors (len i32 [n] (max_dist = no path), cell_ptr i64 [n+1], cells i32 y*W+x, source first,
    interp i32 [n, max_gap-1]: the cell of the interpolated anchor of frame tail+k, -1 where there is none)."""
    n = int(links.shape[0])
    dev = x.device
    lib = _lib.load()
    length = torch.zeros((max(n, 1),), dtype=torch.int32, device=dev)
    stage = torch.empty((max(n, 1), int(max_dist)), dtype=torch.int32, device=dev)
    cell_ptr = torch.empty((n + 1,), dtype=torch.int64, device=dev)
    interp = torch.empty((max(n, 1), max(int(max_gap) - 1, 1)), dtype=torch.int32, device=dev)
    total = ctypes.c_int64(0)
    cap = int(x.shape[1])
    with torch.cuda.device(dev):
        for g, grid in enumerate(grids):
            _lib.check(lib.axt_link_paths(grid._h if grid is not None else None, x.data_ptr(), y.data_ptr(), cap,
                                          links.data_ptr(), n, _lib.dptr(head_group), g, int(H), int(W), int(max_dist),
                                          int(bool(conn8)), length.data_ptr(), stage.data_ptr(), _stream()), 'axt_link_paths')
        _lib.check(lib.axt_link_cells(links.data_ptr(), n, length.data_ptr(), stage.data_ptr(), int(max_dist), int(max_gap),
                                      cell_ptr.data_ptr(), None, None, ctypes.byref(total), _stream()), 'axt_link_cells(count)')
        cells = torch.empty((max(int(total.value), 1),), dtype=torch.int32, device=dev)
        _lib.check(lib.axt_link_cells(links.data_ptr(), n, length.data_ptr(), stage.data_ptr(), int(max_dist), int(max_gap),
                                      cell_ptr.data_ptr(), cells.data_ptr(), interp.data_ptr(), ctypes.byref(total),
                                      _stream()), 'axt_link_cells(fill)')
    return length[:n], cell_ptr, cells[:int(total.value)], interp[:n, :int(max_gap) - 1]


def target_field(target_cells, H, W, mask=None, conn8=False, return_rounds=False):
    """The target screen's field (axt_target_field; the StructureScreen video_plotting.py:170-177 reads): for every cell
    of the [H, W] grid the key (off-mask cells entered, moves) of its minimum-cost path to the nearest of target_cells
    (i32 device tensor of y*W + x) on weights {1 on mask, 65536 off}. mask: None (all ones), a Grid, or an array.
    Returns device tensors (off i32 [H,W], moves i32 [H,W]), with return_rounds also the rounds the search took."""
    _require_gpu()
    dev = target_cells.device
    cells = target_cells.to(torch.int32).contiguous()
    mask = _as_grid(mask, conn8, dev)
    off = torch.empty((int(H), int(W)), dtype=torch.int32, device=dev)
    moves = torch.empty((int(H), int(W)), dtype=torch.int32, device=dev)
    rounds = ctypes.c_int(0)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().axt_target_field(mask._h if mask is not None else None, int(H), int(W), int(bool(conn8)),
                                                cells.data_ptr(), int(cells.numel()), off.data_ptr(), moves.data_ptr(),
                                                ctypes.byref(rounds), _stream()), 'axt_target_field')
    return (off, moves, int(rounds.value)) if return_rounds else (off, moves)


def target_sample(off, moves, x, y, count, field_index=None):
    """The field at every detection slot (axt_target_sample): off / moves i32 [H,W] or [n_fields,H,W]; field_index i32 [F]
    device tensor, the field of every frame (needed for several fields). Returns (off, moves) i32 [F,cap], -1 for empty
    slots and for detections outside the grid."""
    n_frames, cap = x.shape
    H, W = int(off.shape[-2]), int(off.shape[-1])
    n_fields = int(off.shape[0]) if off.dim() == 3 else 1
    d_off = torch.empty((n_frames, cap), dtype=torch.int32, device=x.device)
    d_moves = torch.empty((n_frames, cap), dtype=torch.int32, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().axt_target_sample(off.data_ptr(), moves.data_ptr(), n_fields, _lib.dptr(field_index), H, W,
                                                 x.data_ptr(), y.data_ptr(), count.data_ptr(), n_frames, cap,
                                                 d_off.data_ptr(), d_moves.data_ptr(), _stream()), 'axt_target_sample')
    return d_off, d_moves


def target_paths(fields, grids, x, y, det_moves, H, W, field_index=None, conn8=False):
    """The target paths of all detection slots as CSR (axt_target_paths): fields = list of (off, moves) i32 [H,W] device
    tensors and grids = list of Grid / None, one per distinct mask; field_index i32 [F] device tensor (None: one field).
    Returns device tensors (cell_ptr i64 [F*cap+1], cells i32 y*W + x, detection first, target cell last)."""
    n_frames, cap = x.shape
    dev = x.device
    lib = _lib.load()
    cell_ptr = torch.empty((n_frames * cap + 1,), dtype=torch.int64, device=dev)
    total = ctypes.c_int64(0)

    def call(grid, off, moves, group, cells):
        _lib.check(lib.axt_target_paths(grid._h if grid is not None else None, _lib.dptr(off), _lib.dptr(moves), int(H), int(W),
                                        int(bool(conn8)), x.data_ptr(), y.data_ptr(), n_frames, cap, det_moves.data_ptr(),
                                        _lib.dptr(field_index), group, cell_ptr.data_ptr(), _lib.dptr(cells),
                                        ctypes.byref(total), _stream()), 'axt_target_paths')
    with torch.cuda.device(dev):
        call(None, None, None, 0, None)
        cells = torch.empty((max(int(total.value), 1),), dtype=torch.int32, device=dev)
        for g, (grid, (off, moves)) in enumerate(zip(grids, fields)):
            call(grid, off, moves, g, cells)
    return cell_ptr, cells[:int(total.value)]


def segment_tile_size():
    """Tile edge of the flood's reachability search (axt_segment_tile_size)."""
    return int(_lib.load().axt_segment_tile_size())


def segment_edges(img, sigma=1.0):
    """filters.prewitt + filters.gaussian of 00_segment_bg.ipynb's segment_microchannels in one launch
    (axt_segment_edges). img: uint16 (or int16-viewed) [H,W] device tensor. Returns device tensors (P f32 [H,W] edge
    magnitude, G f32 [H,W] smoothed, minmax f32 [2] = min(G), max(G))."""
    _require_gpu()
    H, W = img.shape
    assert img.is_contiguous() and img.element_size() == 2
    P = torch.empty((H, W), dtype=torch.float32, device=img.device)
    G = torch.empty((H, W), dtype=torch.float32, device=img.device)
    minmax = torch.empty((2,), dtype=torch.float32, device=img.device)
    with torch.cuda.device(img.device):
        _lib.check(_lib.load().axt_segment_edges(img.data_ptr(), int(H), int(W), float(sigma), P.data_ptr(), G.data_ptr(),
                                                 minmax.data_ptr(), _stream()), 'axt_segment_edges')
    return P, G, minmax


def segment_histogram(G, mn, mx):
    """np.histogram(G, 256, range=(mn, mx)) of the notebook's threshold_otsu(prewitt_gaussian) (axt_segment_histogram).
    G: f32 device tensor. Returns the counts as an i64 [256] device tensor."""
    _require_gpu()
    assert G.is_contiguous() and G.dtype == torch.float32
    hist = torch.empty((256,), dtype=torch.int64, device=G.device)
    with torch.cuda.device(G.device):
        _lib.check(_lib.load().axt_segment_histogram(G.data_ptr(), int(G.numel()), float(mn), float(mx), hist.data_ptr(),
                                                     _stream()), 'axt_segment_histogram')
    return hist


def segment_close(P, thr, k=4):
    """morphology.binary_closing(prewitt > thr, morphology.square(k)) of segment_microchannels (axt_segment_close).
    P: f32 [H,W] device tensor. Returns a u8 [H,W] device tensor of 0 / 1."""
    _require_gpu()
    H, W = P.shape
    assert P.is_contiguous() and P.dtype == torch.float32
    out = torch.empty((H, W), dtype=torch.uint8, device=P.device)
    with torch.cuda.device(P.device):
        _lib.check(_lib.load().axt_segment_close(P.data_ptr(), int(H), int(W), float(thr), int(k), out.data_ptr(), _stream()),
                   'axt_segment_close')
    return out


def segment_flood(img, seed_y, seed_x, conn8=True, return_rounds=False):
    """flood(filled_mask, floodpoint) of the notebook's flood_initial_mask (axt_segment_flood). img: u8 / bool [H,W]
    device tensor. Returns a u8 [H,W] device tensor, 1 on the cells connected to the seed through cells of the seed's
    value; with return_rounds also the rounds the search took."""
    _require_gpu()
    H, W = img.shape
    img = img.to(torch.uint8).contiguous()
    out = torch.empty((H, W), dtype=torch.uint8, device=img.device)
    rounds = ctypes.c_int(0)
    with torch.cuda.device(img.device):
        _lib.check(_lib.load().axt_segment_flood(img.data_ptr(), int(H), int(W), int(seed_y), int(seed_x), int(bool(conn8)),
                                                 out.data_ptr(), ctypes.byref(rounds), _stream()), 'axt_segment_flood')
    return (out, int(rounds.value)) if return_rounds else out


def detection_confusion(conf, x, y, count, gx, gy, gcount, thrs, min_dist=23, k_mask=-1):
    """compute_TP_FP_FN (AxonDetections.py:409-466) for all frames and thresholds at once: i32 [F,3,n_thr] on the
    device (TP, FP, FN); with k_mask >= 0 also (fp_mask u8 [F,cap], fn_mask u8 [F,gcap]) for that threshold."""
    n_frames, cap = x.shape
    gcap = gx.shape[1]
    dev = x.device
    th = torch.from_numpy(np.array(thrs, np.float64)).to(dev)            # (a copy: the cached thresholds are read-only)
    out = torch.zeros((n_frames, 3, len(th)), dtype=torch.int32, device=dev)
    fp = fn = None
    if k_mask >= 0:
        fp = torch.zeros((n_frames, cap), dtype=torch.uint8, device=dev)
        fn = torch.zeros((n_frames, gcap), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().axt_detection_confusion(conf.data_ptr(), x.data_ptr(), y.data_ptr(), count.data_ptr(), n_frames,
                                                       cap, gx.data_ptr(), gy.data_ptr(), gcount.data_ptr(), gcap,
                                                       th.data_ptr(), len(th), int(min_dist), int(k_mask), out.data_ptr(),
                                                       _lib.dptr(fp), _lib.dptr(fn), _stream()), 'axt_detection_confusion')
    return (out, fp, fn) if k_mask >= 0 else out


MOT_MAX_SIDE, MOT_MAX_DIST = 1024, 255       # axt_mot_scores: labels / detections per frame, max_dist


def mot_scores_scratch_bytes(n_assoc, n_frames, cap, gcap, no, nh, max_dist=23):
    """Bytes of scratch axt_mot_scores needs for n_assoc associations (the size query; no GPU work)."""
    need = ctypes.c_size_t(0)
    _lib.check(_lib.load().axt_mot_scores(None, int(n_assoc), None, None, None, int(n_frames), int(cap), None, None, None,
                                          None, int(gcap), int(no), int(nh), int(max_dist), None, None, None, None, None,
                                          None, ctypes.byref(need), None), 'axt_mot_scores (scratch size)')
    return int(need.value)


def mot_scores(tracks, x, y, count, gid, gx, gy, gcount, no, nh, max_dist=23, events=False):
    """The counts behind mot_metrics.summarize(mot_metrics.accumulate(...)) for K associations of the same detections
    (axt_mot_scores). tracks i32 [K,F,cap] (-1 = no identity, identities < nh); labels gid (dense, < no),
    gx, gy i32 [F,gcap], gcount i32 [F]. -> (counts i64 [K,10], tallies i32 [K,no,2]) on the device; with events also
    (kind u8 [K,F,gcap], partner slot i32 [K,F,gcap], fp u8 [K,F,cap])."""
    K, n_frames, cap = tracks.shape
    gcap = gx.shape[1]
    dev = x.device
    assert tracks.dtype == torch.int32 and tracks.is_contiguous() and tuple(x.shape) == (n_frames, cap)
    need = ctypes.c_size_t(mot_scores_scratch_bytes(K, n_frames, cap, gcap, no, nh, max_dist))
    scratch = torch.empty(max(need.value, 8), dtype=torch.uint8, device=dev)
    counts = torch.empty((K, 10), dtype=torch.int64, device=dev)
    tallies = torch.empty((K, int(no), 2), dtype=torch.int32, device=dev)
    kind = part = fp = None
    if events:
        kind = torch.empty((K, n_frames, gcap), dtype=torch.uint8, device=dev)
        part = torch.empty((K, n_frames, gcap), dtype=torch.int32, device=dev)
        fp = torch.empty((K, n_frames, cap), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().axt_mot_scores(tracks.data_ptr(), K, x.data_ptr(), y.data_ptr(), count.data_ptr(), n_frames,
                                              cap, gid.data_ptr(), gx.data_ptr(), gy.data_ptr(), gcount.data_ptr(), gcap,
                                              int(no), int(nh), int(max_dist), counts.data_ptr(), tallies.data_ptr(),
                                              _lib.dptr(kind), _lib.dptr(part), _lib.dptr(fp), scratch.data_ptr(),
                                              ctypes.byref(need), _stream()), 'axt_mot_scores')
    return (counts, tallies, kind, part, fp) if events else (counts, tallies)


_HOST_STAGING = {}


def render_tile_size():
    """Edge of the output tiles the render lists are binned by (axt_render_tile_size)."""
    return int(_lib.load().axt_render_tile_size())


def render_frames(frames, mask, mask_stride, ts, H, W, ymin, xmin, Ho, Wo, grid, bg, trail_ptr, trail, trail_col, prim_ptr,
                  prims, tables):
    """video_plotting.draw_frame / draw_detections of the output frames ts (axt_render_frames): u8 [len(ts), Ho, Wo, 3] on
    the frames' device. frames: detection frame t at frames[t]; mask: u8 (None = all ones), frame t at mask + t * mask_stride
    elements; the binned lists as axtrack_amd.render builds them."""
    _require_gpu()
    out = torch.empty((int(ts.numel()), Ho, Wo, 3), dtype=torch.uint8, device=frames.device)
    _lib.check(_lib.load().axt_render_frames(
        frames.data_ptr(), _lib.dptr(mask), int(mask_stride), ts.data_ptr(), int(ts.numel()), int(H), int(W), int(ymin),
        int(xmin), int(Ho), int(Wo), int(grid), int(bool(bg)), trail_ptr.data_ptr(), trail.data_ptr(), trail_col.data_ptr(),
        prim_ptr.data_ptr(), prims.data_ptr(), tables.data_ptr(), out.data_ptr(), _stream()), 'axt_render_frames')
    return out


def to_host(*tensors):
    """Device tensors -> numpy arrays through pinned staging buffers (kept per dtype and grown as needed): the arc list of a
    300 k-detection timelapse is 120 MB, which a pageable copy moves at a few GB/s and a pinned one at PCIe speed. The copies
    are enqueued together and waited for once. The arrays are views of the staging buffers: valid until the next call."""
    out = []
    for k, t in enumerate(tensors):
        n = int(t.numel())
        key = (k, t.dtype)
        buf = _HOST_STAGING.get(key)
        if buf is None or buf.numel() < n:
            buf = _HOST_STAGING[key] = torch.empty((max(n, 1) * 5 // 4 + 16,), dtype=t.dtype, pin_memory=True)
        buf[:n].copy_(t.reshape(-1), non_blocking=True)
        out.append(buf[:n].numpy().reshape(tuple(t.shape)))
    # a non_blocking D2H copy runs on the current stream of the SOURCE tensor's device, which need not be the current
    # device (Detector(device='cuda:1') without set_device): wait on every device that holds one of the tensors
    for dev in {t.device for t in tensors if t.is_cuda}:
        torch.cuda.current_stream(dev).synchronize()
    return out


def arc_cost_int(cost, kind, a, b):
    return int(_lib.load().axt_arc_cost_int(float(cost), int(kind), int(a), int(b)))


def mcf_solve(obs_int, entry_int, exit_int, row_ptr, col, cost_int, min_flow, max_flow, duals=False):
    """MinCostFlowTracker.compute_trajectories (AxonDetections.py:690) on host arrays.
    Returns (next i32 [n], track i32 [n], n_tracks, total_cost) or None when infeasible; with duals=True a fifth element
    (pot_u i64 [n], pot_v i64 [n], pot_t): the node potentials that certify the optimum (axt_mcf_solve_duals)."""
    n = len(obs_int)
    arrs = [np.ascontiguousarray(a, np.int64) for a in (obs_int, entry_int, exit_int, row_ptr)]
    arrs += [np.ascontiguousarray(col, np.int32), np.ascontiguousarray(cost_int, np.int64)]
    return _flow_solve('axt_mcf_solve', (n, *(a.ctypes.data for a in arrs), int(min_flow), int(max_flow)), n, duals)


def _flow_solve(what, head, n, duals):
    """Call the flow-solve entry point `what` over n detections (head: its arguments before the outputs), with duals its
    `_duals` symbol, and return what mcf_solve returns."""
    what += '_duals' if duals else ''
    nxt, track, n_tracks, total = np.empty(n, np.int32), np.empty(n, np.int32), ctypes.c_int(0), ctypes.c_int64(0)
    out = [nxt.ctypes.data, track.ctypes.data, ctypes.byref(n_tracks), ctypes.byref(total)]
    if duals:
        pu, pv, pt = np.zeros(n, np.int64), np.zeros(n, np.int64), ctypes.c_int64(0)
        out += [pu.ctypes.data, pv.ctypes.data, ctypes.byref(pt)]
    if _lib.check(getattr(_lib.load(), what)(*head, *out), what) == 1:
        return None
    res = (nxt, track, int(n_tracks.value), int(total.value))
    return res + ((pu, pv, int(pt.value)),) if duals else res


class McfShard:
    """One rank's part of the frame-sharded flow solve (axt_mcf_shard_*): begin() solves this rank's run of time blocks
    and returns its state (uint8 array) for the all-gather; finish(states) joins the runs and returns what mcf_solve
    returns. The network arrays are kept alive by this object."""

    def __init__(self, obs_int, entry_int, exit_int, row_ptr, col, cost_int, rank, world):
        self._lib = _lib.load()
        self.n = len(obs_int)
        self._keep = [np.ascontiguousarray(a, np.int64) for a in (obs_int, entry_int, exit_int, row_ptr)]
        self._keep += [np.ascontiguousarray(col, np.int32), np.ascontiguousarray(cost_int, np.int64)]
        h, nbytes = ctypes.c_void_p(), ctypes.c_int64(0)
        k = self._keep
        _lib.check(self._lib.axt_mcf_shard_begin(self.n, k[0].ctypes.data, k[1].ctypes.data, k[2].ctypes.data, k[3].ctypes.data,
                                                 k[4].ctypes.data, k[5].ctypes.data, int(rank), int(world), ctypes.byref(h),
                                                 ctypes.byref(nbytes)), 'axt_mcf_shard_begin')
        self._h, self.rank, self.world = h, int(rank), int(world)
        self.state = np.zeros(int(nbytes.value), np.uint8)
        _lib.check(self._lib.axt_mcf_shard_export(self._h, self.state.ctypes.data), 'axt_mcf_shard_export')

    def finish(self, states, min_flow, max_flow, duals=False):
        """states: list over ranks of uint8 arrays (this rank's own entry is not read). duals: as mcf_solve."""
        states = [np.ascontiguousarray(s, np.uint8) for s in states]
        ptrs = (ctypes.c_void_p * self.world)(*[s.ctypes.data if len(s) else None for s in states])
        sizes = np.array([len(s) for s in states], np.int64)
        return _flow_solve('axt_mcf_shard_finish', (self._h, ptrs, sizes.ctypes.data, int(min_flow), int(max_flow)), self.n, duals)

    def __del__(self):
        h, self._h = getattr(self, '_h', None), None
        if h:
            self._lib.axt_mcf_shard_free(h)


# ------------------------------------------------------------------ TIFF strips (csrc/tiff.hip, include/axtrack_hip_tiff.h)
TIFF_STATUS_TEXT = {1: 'the input ends before the rows are complete', 2: 'an invalid LZW code or Deflate stream',
                    3: 'the data decodes to more than the rows of the strip', 4: 'the segment descriptor is out of range',
                    5: 'checksum: the Adler-32 of the Deflate stream is not that of the inflated bytes'}
TIFF_INFLATE = (8, 32946)                            # Compression values of Deflate strips: csrc/tiff_inflate.hip


def tiff_decode_launch(d_src, segs, W, compression, predictor, big_endian, out, status):
    """axt_tiff_decode_u16 -- for Deflate strips (compression 8, 32946) axt_tiff_inflate_u16 -- on the current stream,
    nothing waited for. d_src: uint8 device tensor; segs: TIFF_SEGMENT_DTYPE
    records (host; uploaded here from pinned memory) or a device uint8 tensor that already holds them; out: contiguous
    2-byte device tensor, the records' dst_offset counted in its elements; status: int32 device tensor [n_segs]. Returns
    the device copy of the records, which the caller keeps until the stream has passed the launch."""
    from .tiff import TIFF_SEGMENT_DTYPE
    assert d_src.dtype == torch.uint8 and d_src.is_contiguous() and out.is_contiguous() and out.element_size() == 2
    if isinstance(segs, torch.Tensor):
        d_segs, n = segs, segs.numel() // TIFF_SEGMENT_DTYPE.itemsize
    else:
        segs = np.ascontiguousarray(segs, TIFF_SEGMENT_DTYPE)
        n = len(segs)
        pinned = torch.empty(max(segs.nbytes, 1), dtype=torch.uint8, pin_memory=True)
        pinned.numpy()[:segs.nbytes] = segs.view(np.uint8)
        d_segs = pinned.to(out.device, non_blocking=True)
        d_segs._axt_pinned = pinned                                       # (alive as long as the device copy)
    assert status.dtype == torch.int32 and status.is_contiguous() and status.numel() >= n and status.device == out.device
    assert d_src.device == out.device
    lib = _lib.load()
    with torch.cuda.device(out.device):
        if int(compression) in TIFF_INFLATE:
            _lib.check(lib.axt_tiff_inflate_u16(d_src.data_ptr(), d_src.numel(), d_segs.data_ptr(), n, int(W), int(predictor),
                                                int(bool(big_endian)), out.data_ptr(), out.numel(), status.data_ptr(), _stream()),
                       'axt_tiff_inflate_u16')
        else:
            _lib.check(lib.axt_tiff_decode_u16(d_src.data_ptr(), d_src.numel(), d_segs.data_ptr(), n, int(W), int(compression),
                                               int(predictor), int(bool(big_endian)), out.data_ptr(), out.numel(),
                                               status.data_ptr(), _stream()), 'axt_tiff_decode_u16')
    return d_segs


def tiff_raise_on_status(status, frame=None, row0=None, what='the TIFF data'):
    """Read the statuses (one copy to the host, which waits for the stream) and raise TiffError for the first failing
    segment, naming its frame and row where the caller knows them."""
    from .tiff import TiffError
    st = status.cpu().numpy()
    bad = np.flatnonzero(st)
    if len(bad):
        k = int(bad[0])
        where = f'segment {k}' if frame is None else f'the strip of frame {int(frame[k])}, row {int(row0[k])} (segment {k})'
        raise TiffError(f'{what}: {where} does not decode: {TIFF_STATUS_TEXT.get(int(st[k]), "status " + str(int(st[k])))} '
                        f'(status {int(st[k])}; {len(bad)} of {len(st)} segments fail)')


def tiff_decode_u16(d_src, segs, W, compression, predictor, big_endian, out, frame=None, row0=None):
    """Decode strips that are already on the device into `out` and check them: tiff_decode_launch, then the statuses read
    once. Raises tiff.TiffError naming the first failing segment's frame and row. Returns out."""
    n = len(segs)
    status = torch.empty(max(n, 1), dtype=torch.int32, device=out.device)
    keep = tiff_decode_launch(d_src, segs, W, compression, predictor, big_endian, out, status)
    tiff_raise_on_status(status[:n], frame, row0)
    del keep
    return out


# ------------------------------------------------------------------ TIFF strips, deflated (csrc/tiff_deflate.hip, csrc/axt_tiff_deflate.h)
TIFF_DEFLATE_STATUS_TEXT = {3: 'the stream does not fit its slot', 4: 'the segment descriptor is out of range'}


def tiff_deflate_bound(raw_bytes):
    """The longest stream axt_tiff_deflate_u16 writes for raw_bytes bytes: all stored (axt_tiff_deflate_bound)."""
    return int(_lib.load().axt_tiff_deflate_bound(int(raw_bytes)))


def _device_records(segs, device):
    from .tiff import TIFF_SEGMENT_DTYPE
    segs = np.ascontiguousarray(segs, TIFF_SEGMENT_DTYPE)
    pinned = torch.empty(max(segs.nbytes, 1), dtype=torch.uint8, pin_memory=True)
    pinned.numpy()[:segs.nbytes] = segs.view(np.uint8)
    d_segs = pinned.to(device, non_blocking=True)
    d_segs._axt_pinned = pinned                                           # (alive as long as the device copy)
    return d_segs


def tiff_deflate_launch(samples, segs, W, predictor, slots, nbytes, status):
    """axt_tiff_deflate_u16 on the current stream, nothing waited for. samples: contiguous 2-byte device tensor; segs:
    TIFF_SEGMENT_DTYPE records (host; uploaded here from pinned memory) or a device uint8 tensor that holds them, with the
    roles of csrc/axt_tiff_deflate.h: dst_offset / rows name the strip's samples, src_offset / src_bytes its slot in
    `slots` (uint8 device tensor); nbytes: int64 [n_segs], status: int32 [n_segs], on the device. Returns the device copy of
    the records, which the caller keeps until the stream has passed the launch."""
    from .tiff import TIFF_SEGMENT_DTYPE
    assert samples.is_contiguous() and samples.element_size() == 2 and slots.dtype == torch.uint8 and slots.is_contiguous()
    if isinstance(segs, torch.Tensor):
        d_segs, n = segs, segs.numel() // TIFF_SEGMENT_DTYPE.itemsize
    else:
        n = len(segs)
        d_segs = _device_records(segs, samples.device)
    assert nbytes.dtype == torch.int64 and status.dtype == torch.int32 and nbytes.numel() >= n and status.numel() >= n
    assert nbytes.is_contiguous() and status.is_contiguous() and slots.device == samples.device == nbytes.device == status.device
    with torch.cuda.device(samples.device):
        _lib.check(_lib.load().axt_tiff_deflate_u16(samples.data_ptr(), samples.numel(), d_segs.data_ptr(), n, int(W), int(predictor),
                                                    slots.data_ptr(), slots.numel(), nbytes.data_ptr(), status.data_ptr(), _stream()),
                   'axt_tiff_deflate_u16')
    return d_segs


def tiff_compact_launch(slots, d_segs, nbytes, n, packed, offsets):
    """axt_tiff_compact_streams on the current stream: the n streams back to back in `packed` (uint8 device tensor),
    offsets: int64 [n + 1] on the device, the exclusive scan of the lengths and their sum."""
    assert packed.dtype == torch.uint8 and packed.is_contiguous() and offsets.dtype == torch.int64 and offsets.numel() >= n + 1
    with torch.cuda.device(slots.device):
        _lib.check(_lib.load().axt_tiff_compact_streams(slots.data_ptr(), d_segs.data_ptr(), nbytes.data_ptr(), int(n), packed.data_ptr(),
                                                        packed.numel(), offsets.data_ptr(), _stream()), 'axt_tiff_compact_streams')


def tiff_deflate_strips(samples, segs, W, predictor, frame=None, row0=None):
    """Deflate strips of a device tensor and bring the streams to the host: the launch into slots of the all-stored bound,
    the compaction, then two copies -- the table of offsets and statuses, and the packed bytes through a pinned buffer, so
    that only compressed bytes cross. segs: records with dst_offset / rows set; the slots are laid out here. Returns
    (uint8 numpy view of the pinned buffer, int64 offsets [n + 1]). Raises tiff.TiffError naming the first failing strip."""
    from .tiff import TIFF_SEGMENT_DTYPE, TiffError
    segs = np.array(segs, TIFF_SEGMENT_DTYPE)
    n, dev = len(segs), samples.device
    caps = np.array([tiff_deflate_bound(2 * int(r) * int(W)) for r in np.unique(segs['rows'])], np.int64)
    segs['src_bytes'] = caps[np.searchsorted(np.unique(segs['rows']), segs['rows'])]
    segs['src_offset'] = np.concatenate([[0], np.cumsum(segs['src_bytes'])[:-1]]) if n else 0
    total_cap = int(segs['src_bytes'].sum())
    slots = torch.empty(max(total_cap, 1), dtype=torch.uint8, device=dev)
    packed = torch.empty(max(total_cap, 1), dtype=torch.uint8, device=dev)
    table = torch.zeros(2 * n + 2, dtype=torch.int64, device=dev)        # lengths [n], offsets [n + 1], pad
    status = torch.zeros(max(n, 1), dtype=torch.int32, device=dev)
    d_segs = tiff_deflate_launch(samples, segs, W, predictor, slots, table[:n], status)
    tiff_compact_launch(slots, d_segs, table[:n], n, packed, table[n:2 * n + 1])
    st = status[:n].cpu().numpy()                                         # (waits for the stream)
    bad = np.flatnonzero(st)
    if len(bad):
        k = int(bad[0])
        where = f'segment {k}' if frame is None else f'the strip of frame {int(frame[k])}, row {int(row0[k])} (segment {k})'
        raise TiffError(f'{where} does not deflate: {TIFF_DEFLATE_STATUS_TEXT.get(int(st[k]), "status " + str(int(st[k])))} '
                        f'(status {int(st[k])}; {len(bad)} of {n} segments fail)')
    offsets = table[n:2 * n + 1].cpu().numpy()
    total = int(offsets[-1])
    host = torch.empty(max(total, 1), dtype=torch.uint8, pin_memory=True)
    host[:total].copy_(packed[:total])
    del d_segs
    return host.numpy()[:total], offsets


# ------------------------------------------------------------------ JPEG scan segments (csrc/jpeg.hip, include/axtrack_hip_jpeg.h)
def jpeg_scan_bound(H, W):
    """Worst-case bytes of one frame's scan segment (axt_jpeg_scan_bound)."""
    return int(_lib.check(_lib.load().axt_jpeg_scan_bound(int(H), int(W)), 'axt_jpeg_scan_bound'))


def jpeg_scratch_bytes(n_frames, H, W):
    return int(_lib.check(_lib.load().axt_jpeg_scratch_bytes(int(n_frames), int(H), int(W)), 'axt_jpeg_scratch_bytes'))


def jpeg_encode_launch(rgb, quality, scan, scan_bytes, status, scratch):
    """axt_jpeg_encode_rgb8 on the current stream, nothing waited for. rgb: uint8 device tensor [N, H, W, 3] whose frames
    are contiguous (the frame stride may exceed 3 H W); scan: uint8 [N, capacity]; scan_bytes: int64 [N]; status: int32
    [N]; scratch: uint8, at least jpeg_scratch_bytes(N, H, W)."""
    _require_gpu()
    N, H, W, C = rgb.shape
    assert rgb.dtype == torch.uint8 and C == 3 and (N == 0 or rgb[0].is_contiguous()) and (N <= 1 or rgb.stride(0) >= 3 * H * W)
    assert scan.dtype == torch.uint8 and scan.is_contiguous() and scan.shape[0] == N
    assert scan_bytes.dtype == torch.int64 and scan_bytes.numel() >= N and status.dtype == torch.int32 and status.numel() >= N
    assert scratch.dtype == torch.uint8 and scratch.is_contiguous()
    assert all(t.device == rgb.device for t in (scan, scan_bytes, status, scratch))
    stride = rgb.stride(0) if N > 1 else 3 * H * W
    with torch.cuda.device(rgb.device):
        _lib.check(_lib.load().axt_jpeg_encode_rgb8(rgb.data_ptr(), N, H, W, int(stride), int(quality), scan.data_ptr(),
                                                    int(scan.shape[1]), scan_bytes.data_ptr(), status.data_ptr(),
                                                    scratch.data_ptr(), scratch.numel(), _stream()), 'axt_jpeg_encode_rgb8')

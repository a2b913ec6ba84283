"""Fine-tuning of the detector's linear head on labelled frames.

The convolutional trunk stays frozen: its output per (frame, tile) item -- what the first linear layer reads -- is computed
by the inference kernels (Detector.features_frames; once, or once per epoch when the frames are augmented), and an epoch is nothing but head steps on that table: forward
(model.py:105-117), YOLO_AXTrack_loss (loss.py:18-68), backward and torch.optim.Adam with L2 weight decay
(core_functionality.py:81), all in csrc/train.hip. The epoch loop restates one_epoch / run_epoch
(core_functionality.py:109-165); its every-tenth-epoch metrics run when a labelled test timelapse is given
(fine_tune_head(test_timelapse=...)). With use_transforms it also restates the reference's augmentation (augment.py): a new
translate / flip / rotate of frames and labels every epoch, the prepare_data resampling loop, and the feature table
recomputed from the warped frames, which costs about one trunk pass per epoch.

The last one to three conv blocks can be trained jointly with the head (csrc/train_conv.hip): ConvBlockTrainer is one
block, ConvTrunkTrainer chains any run of the last conv blocks with their pools, either with BatchNorm's running
statistics or with train-mode BatchNorm; ConvStageTrainer is its three-block case, the last stage (conv blocks 5 and 6,
the 2 x 2 max-pool, conv block 7). The cached table is then the trunk's output that many blocks earlier.
fine_tune_head's docstring says what each option (train_conv_blocks, train_last_conv, bn_batch_stats) does to a step.

fine_tune_detector goes on to every depth: ConvBlockTrainer(stride=2) is a block of the stride-2 front, and the input is
the block-2 table (depths 4, 5) or the raw stacks gathered per batch (depths 6..8). Both functions share one step loop
(_fine_tune), which builds one ConvTrunkTrainer at every depth of 1 or more.

Every trainer can put its weights of the moment into a live Detector without leaving the device (export_to;
csrc/repack.hip), which is what test_loss=True does after every epoch to take the loss on a test set."""
import ctypes
import functools
import os

import numpy as np
import torch

from . import _lib
from .hotpath import S, CELLS, _require_gpu, _stream

COMPONENTS = ('total_no_object_loss', 'total_object_loss', 'total_xy_anchors_loss', 'total_summed_loss',
              'total_pos_labels_rate')
FC_KEYS = ('fcs.1.weight', 'fcs.1.bias', 'fcs.3.weight', 'fcs.3.bias', 'fcs.5.weight', 'fcs.5.bias')
# deployed_model/params.txt: what a key missing from `parameters` takes
TRAIN_DEFAULTS = dict(LR=0.0005, WEIGHT_DECAY=0.0005, LR_DECAYRATE=15, L_OBJECT=49.5, L_COORD_ANCHOR=49.5, L_NOBJECT=1,
                      BATCH_SIZE=32, SHUFFLE=True, DROP_LAST=False)
ADAM_BETAS, ADAM_EPS = (0.9, 0.999), 1e-8          # torch.optim.Adam's defaults, which the reference leaves alone


def label_arrays(labels):
    """labels in the format AxonDetections.set_groundtruth takes -- per detection frame (x, y) or (x, y, ids) -> i32
    [F, cap] x, y (unused slots -1) and i32 [F] counts. Negative coordinates mean "no label" (the reference's fillna(-1))."""
    cap = max([len(l[0]) for l in labels] + [1])
    lx = np.full((len(labels), cap), -1, np.int32)
    ly = np.full((len(labels), cap), -1, np.int32)
    cnt = np.zeros(len(labels), np.int32)
    for t, l in enumerate(labels):
        x, y = np.asarray(l[0], np.int64), np.asarray(l[1], np.int64)
        if len(x) != len(y):
            raise ValueError(f'frame {t}: {len(x)} x anchors and {len(y)} y anchors')
        lx[t, :len(x)] = x
        ly[t, :len(y)] = y
        cnt[t] = len(x)
    return lx, ly, cnt


def yolo_targets(labels, tile_yx, device='cuda:0'):
    """Timelapse.construct_tiles (target half, :513-548) + tiled_target2yolo_format (:451-490) for the kept tiles:
    -> f32 [F, n_tiles, 12, 12, 4] on the GPU, dim 2 the x cell, dim 3 the y cell, last (1, x_in_cell, y_in_cell, label
    index). `labels` may also be the (lx, ly, count) arrays of label_arrays()."""
    _require_gpu()
    if isinstance(labels, tuple) and len(labels) == 3 and getattr(labels[2], 'ndim', 0) == 1 and np.ndim(labels[0]) == 2:
        lx, ly, cnt = (np.ascontiguousarray(a, np.int32) for a in labels)
    else:
        lx, ly, cnt = label_arrays(labels)
    dev = torch.device(device)
    tile_yx = np.ascontiguousarray(tile_yx, np.int32).reshape(-1, 2)
    F, cap = lx.shape
    out = torch.empty((F, len(tile_yx), S, S, 4), dtype=torch.float32, device=dev)
    d_lx, d_ly, d_cnt = (torch.from_numpy(a).to(dev) for a in (lx, ly, cnt))
    with torch.cuda.device(dev):
        _lib.check(_lib.load().axt_yolo_targets(d_lx.data_ptr(), d_ly.data_ptr(), d_cnt.data_ptr(), F, cap,
                                                tile_yx.ctypes.data, len(tile_yx), out.data_ptr(), _stream()),
                   'axt_yolo_targets')
    return out


def learning_rate(lr, decayrate, epoch):
    """LR * e^(-sqrt(E) / LR_DECAYRATE) (the LambdaLR of core_functionality.py:83-87), LR if the rate is falsy."""
    return float(lr * np.e ** ((-1 / decayrate) * np.sqrt(epoch))) if decayrate else float(lr)


def epoch_batches(n_items, batch_size, shuffle, drop_last, rng):
    """The index batches of one epoch as the reference's DataLoader forms them (core_functionality.py:99-107): a
    permutation drawn from `rng` when shuffling, batches of batch_size, the last smaller one kept unless drop_last."""
    order = rng.permutation(n_items) if shuffle else np.arange(n_items)
    batches = [order[i:i + batch_size] for i in range(0, n_items, batch_size)]
    if drop_last and batches and len(batches[-1]) < batch_size:
        batches.pop()
    return [np.ascontiguousarray(b, np.int32) for b in batches]


def _np32(v):
    v = v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)
    return np.ascontiguousarray(v, np.float32)


def _train_parameters(parameters):
    """TRAIN_DEFAULTS with the keys of `parameters` that it knows replaced."""
    P = dict(TRAIN_DEFAULTS)
    P.update({k: v for k, v in (parameters or {}).items() if k in TRAIN_DEFAULTS})
    return P


@functools.lru_cache(maxsize=None)
def _first_rows(B, device):
    """Rows 0..B-1 as an i32 tensor on `device`: the index with which a trainer reads the whole output of the one in front
    of it. One tensor per batch size (at most max_batch of them) for every trainer and the step loop."""
    return torch.arange(B, dtype=torch.int32, device=device)


def _check_export(trainer, detector):
    """What every export_to asks before any launch: a live Detector on the trainer's device."""
    from .hotpath import Detector
    if not isinstance(detector, Detector) or not getattr(detector, '_h', None):
        raise TypeError(f'export_to takes a live hotpath.Detector, got {type(detector).__name__}')
    if detector.device != trainer.device:
        raise ValueError(f'the trainer is on {trainer.device}, the detector on {detector.device}')


class _HandleTrainer:
    """What HeadTrainer and ConvBlockTrainer share: the training parameters, the library handle's life, and the checks of
    a batch's index and of a table. _CREATE, _DESTROY, _DEVICE_BYTES: the library's functions for the handle."""
    _CREATE = _DESTROY = _DEVICE_BYTES = None

    def __init__(self, state_dict, keys, parameters, max_batch, device):
        _require_gpu()
        self.device = torch.device(device)
        self.max_batch = int(max_batch)
        self.P = _train_parameters(parameters)
        self._sd = state_dict
        for k in keys:
            if k not in state_dict:
                raise KeyError(f'state_dict lacks {k}')

    def _create(self, *args):
        """The handle from _CREATE(*args, max_batch, &handle); the caller has checked everything it can on the host."""
        self._lib = _lib.load()
        handle = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            _lib.check(getattr(self._lib, self._CREATE)(*args, self.max_batch, ctypes.byref(handle)), self._CREATE)
        self._h = handle

    def __del__(self):
        h, self._h = getattr(self, '_h', None), None
        if h:
            getattr(self._lib, self._DESTROY)(h)

    @property
    def device_bytes(self):
        return int(getattr(self._lib, self._DEVICE_BYTES)(self._h))

    def _index(self, index, n):
        """Batch rows as a device i32 tensor, checked against the table's n rows (on the host where the index is there)."""
        if index is None:
            index = np.arange(n)
        on_device = isinstance(index, torch.Tensor)
        index = index.to(self.device, torch.int32).contiguous() if on_device else np.ascontiguousarray(index, np.int32)
        if bool(((index < 0) | (index >= n)).any()):
            raise IndexError(f'batch index outside the table of {n} rows')
        if not on_device:
            index = torch.from_numpy(index).to(self.device)
        if not 1 <= len(index) <= self.max_batch:
            raise ValueError(f'a batch of {len(index)} rows; this trainer takes 1..{self.max_batch}')
        return index

    def _check_table(self, t, width, what):
        if not (t.is_contiguous() and t.dtype == torch.float32 and t.device == self.device and t.dim() >= 2
                and t[0].numel() == width):
            raise ValueError(f'{what} must be a contiguous f32 tensor [n, {width}] on {self.device}')


class HeadTrainer(_HandleTrainer):
    """Device-resident fcs.1/3/5 with their Adam moments (axt_head_trainer). forward / loss / step work on batches picked
    by index from a feature table [n_items, K0] and a target table [n_items, 12, 12, 4] that stay on the GPU."""
    _CREATE, _DESTROY, _DEVICE_BYTES = (f'axt_head_trainer_{f}' for f in ('create', 'destroy', 'device_bytes'))

    def __init__(self, state_dict, parameters=None, max_batch=64, device='cuda:0'):
        super().__init__(state_dict, FC_KEYS, parameters, max_batch, device)
        w = [_np32(state_dict[k]) for k in FC_KEYS]
        self.dims = (w[0].shape[1], w[0].shape[0], w[2].shape[0], w[4].shape[0])
        if w[2].shape[1] != self.dims[1] or w[4].shape[1] != self.dims[2] or any(
                w[2 * i + 1].shape != (self.dims[i + 1],) for i in range(3)):
            raise ValueError(f'inconsistent head shapes: {[a.shape for a in w]}')
        self._create(*self.dims, *[a.ctypes.data for a in w])

    def forward(self, features, index=None):
        """features f32 [n_items, K0] on the GPU, index: which rows form the batch (default: all) -> [B, 12, 12, 3]."""
        self._check_table(features, self.dims[0], 'features')
        index = self._index(index, features.shape[0])
        out = torch.empty((len(index), S, S, 3), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self._lib.axt_head_trainer_forward(self._h, features.data_ptr(), index.data_ptr(), len(index),
                                                          out.data_ptr(), _stream()), 'axt_head_trainer_forward')
        return out

    def loss(self, yolo, targets, index=None, read=True):
        """YOLO_AXTrack_loss of the batch grids `yolo` [B,12,12,3] against rows `index` of the target table
        [n_items,12,12,4] -> (components: dict of the reference's five names, or None with read=False; dY [B,12,12,3])."""
        targets = targets.reshape(-1, S, S, 4)
        self._check_table(targets, CELLS * 4, 'targets')
        self._check_table(yolo, CELLS * 3, 'yolo')
        index = self._index(index, targets.shape[0])
        if len(index) != yolo.shape[0]:
            raise ValueError(f'{yolo.shape[0]} grids for {len(index)} targets')
        dy = torch.empty_like(yolo)
        comp = np.zeros(5, np.float64)
        P = self.P
        with torch.cuda.device(self.device):
            _lib.check(self._lib.axt_head_trainer_loss(self._h, yolo.data_ptr(), targets.data_ptr(), index.data_ptr(),
                                                       len(index), float(P['L_OBJECT']), float(P['L_NOBJECT']),
                                                       float(P['L_COORD_ANCHOR']), comp.ctypes.data if read else None,
                                                       dy.data_ptr(), _stream()), 'axt_head_trainer_loss')
        return (dict(zip(COMPONENTS, (float(c) for c in comp))) if read else None), dy

    def step(self, features, index, dy, lr=None, eps=ADAM_EPS):
        """Backward pass of the batch the last forward() ran, and one Adam step (lr: default P['LR']; eps: Adam's, which the
        reference leaves at torch's default)."""
        self._check_table(features, self.dims[0], 'features')
        self._check_table(dy, CELLS * 3, 'dy')
        index = self._index(index, features.shape[0])
        if len(index) != dy.shape[0]:
            raise ValueError(f'{dy.shape[0]} gradients for a batch of {len(index)}')
        P = self.P
        with torch.cuda.device(self.device):
            _lib.check(self._lib.axt_head_trainer_step(self._h, features.data_ptr(), index.data_ptr(), len(index),
                                                       dy.data_ptr(), float(P['LR'] if lr is None else lr), ADAM_BETAS[0],
                                                       ADAM_BETAS[1], float(eps), float(P['WEIGHT_DECAY']), _stream()),
                       'axt_head_trainer_step')

    def input_grad(self, dy):
        """The gradient of the loss with respect to the feature rows the last forward() read: dy [B,12,12,3] -> [B, K0]
        (axt_head_trainer_input_grad). From the weights as they stand, so call it before step(); it changes nothing that
        step() reads."""
        self._check_table(dy, CELLS * 3, 'dy')
        out = torch.empty((dy.shape[0], self.dims[0]), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self._lib.axt_head_trainer_input_grad(self._h, dy.data_ptr(), dy.shape[0], out.data_ptr(), _stream()),
                       'axt_head_trainer_input_grad')
        return out

    def weights(self):
        """The six fcs.* tensors as numpy arrays, in FC_KEYS order."""
        K0, H1, H2, NO = self.dims
        out = [np.empty(s, np.float32) for s in ((H1, K0), (H1,), (H2, H1), (H2,), (NO, H2), (NO,))]
        with torch.cuda.device(self.device):
            _lib.check(self._lib.axt_head_trainer_read_weights(self._h, *[a.ctypes.data for a in out]),
                       'axt_head_trainer_read_weights')
        return out

    def moments(self, layer):
        """Adam state of linear layer 0..2: (m of the weights, v of the weights, m of the bias, v of the bias, step count)."""
        k, n = self.dims[layer], self.dims[layer + 1]
        out = [np.empty((n, k), np.float32), np.empty((n, k), np.float32), np.empty(n, np.float32), np.empty(n, np.float32)]
        step = ctypes.c_int64()
        with torch.cuda.device(self.device):
            _lib.check(self._lib.axt_head_trainer_read_moments(self._h, layer, *[a.ctypes.data for a in out],
                                                               ctypes.byref(step)), 'axt_head_trainer_read_moments')
        return (*out, int(step.value))

    def export_to(self, detector):
        """The three linear layers as they stand into a live Detector on the same device, without a host copy
        (axt_head_trainer_export: Detector.load_linear from the trainer's own device tensors, on the current stream). The
        detector then computes what Detector(self.state_dict()) computes in these layers, byte for byte."""
        _check_export(self, detector)
        with torch.cuda.device(self.device):
            _lib.check(self._lib.axt_head_trainer_export(self._h, detector._h, _stream()), 'axt_head_trainer_export')
        detector.state_dict_source = None

    def state_dict(self):
        """The state dict this trainer was built from with the six fcs.* tensors replaced by the trained ones (numpy f32)."""
        sd = dict(self._sd)
        sd.update(zip(FC_KEYS, self.weights()))
        return sd


CONV_SUFFIXES = ('conv.weight', 'conv.bias', 'batchnorm.weight', 'batchnorm.bias')         # what ConvBlockTrainer trains
CONV_STATS = ('batchnorm.running_mean', 'batchnorm.running_var')                           # read; moved with batch_stats only
CONV_COUNTER = 'batchnorm.num_batches_tracked'
LAST_CONV_BLOCK = 'ConvNet.ConvBlock_10'            # conv block 7 of the package's numbering: 80 -> 160 on 16 x 16 maps


class ConvBlockTrainer(_HandleTrainer):
    """One block Conv2d 3x3 + BatchNorm2d + LeakyReLU(0.1) of the state dict (model.py:5-18) on the device with the Adam
    moments of its four trainable tensors (axt_conv_trainer). forward / step work on batches picked by index from a table
    [n_items, Ci*H*W] of the block's inputs (Detector.features_frames(block=6) for the last block); forward's output
    [B, Co*H*W] is what HeadTrainer.forward reads. BatchNorm runs with its running statistics and never updates them,
    or with batch_stats=True as nn.BatchNorm2d in train mode (momentum: its momentum): forward normalises the batch with
    its own mean and biased variance and moves running_mean, running_var (by the unbiased variance) and the batch count;
    step and input_grad take the gradients through the statistics, and conv.bias, whose gradient is then 0 by definition,
    moves by its weight decay alone. A batch of fewer than 2 values per channel is a ValueError then.
    stride, in_size: a convolution of stride 1 or 2 on input maps of in_size = (Hin, Win) (default: map_size), up to
    512 x 512 (axt_conv_trainer_create_strided); the tables are then [n, Ci*Hin*Win] in and [B, Co*H*W] out with
    H = (Hin - 1) // stride + 1. With stride=1 and no in_size the trainer makes the calls it always made, on maps up to
    64 x 64."""
    _CREATE, _DESTROY, _DEVICE_BYTES = (f'axt_conv_trainer_{f}' for f in ('create', 'destroy', 'device_bytes'))

    def __init__(self, state_dict, block_key=LAST_CONV_BLOCK, parameters=None, map_size=(16, 16), max_batch=64,
                 device='cuda:0', batch_stats=False, momentum=0.1, stride=1, in_size=None):
        if isinstance(stride, bool) or stride not in (1, 2):
            raise ValueError(f'stride must be 1 or 2, got {stride!r}')
        self.block_key = block_key
        self.keys = tuple(f'{block_key}.{k}' for k in CONV_SUFFIXES + CONV_STATS)
        super().__init__(state_dict, self.keys, parameters, max_batch, device)
        w = [_np32(state_dict[k]) for k in self.keys]
        if w[0].ndim != 4 or w[0].shape[2:] != (3, 3) or any(a.shape != (w[0].shape[0],) for a in w[1:]):
            raise ValueError(f'not a 3x3 conv block: {[a.shape for a in w]}')
        self.Co, self.Ci = int(w[0].shape[0]), int(w[0].shape[1])
        self.stride = int(stride)
        if self.stride == 1 and in_size is None:
            self.H, self.W = self.Hin, self.Win = tuple(int(v) for v in map_size)
            self._create(self.Ci, self.Co, self.H, self.W, *[a.ctypes.data for a in w])
        else:
            self.Hin, self.Win = (int(v) for v in (map_size if in_size is None else in_size))
            self.H, self.W = (self.Hin - 1) // self.stride + 1, (self.Win - 1) // self.stride + 1
            self._CREATE = 'axt_conv_trainer_create_strided'
            self._create(self.Ci, self.Co, self.Hin, self.Win, self.stride, *[a.ctypes.data for a in w])
        self.in_width, self.out_width = self.Ci * self.Hin * self.Win, self.Co * self.H * self.W
        self.batch_stats = bool(batch_stats)
        self.momentum = float(momentum) if self.batch_stats else momentum       # read with batch statistics only
        if self.batch_stats:                            # a trainer that never asks makes the calls it always made
            if not 0 < self.momentum <= 1:
                raise ValueError(f'momentum must be in (0, 1], got {momentum!r}')
            with torch.cuda.device(self.device):
                _lib.check(self._lib.axt_conv_trainer_set_batch_stats(self._h, 1, self.momentum),
                           'axt_conv_trainer_set_batch_stats')

    def forward(self, inputs, index=None):
        """inputs f32 [n_items, Ci*Hin*Win] on the GPU, index: which rows form the batch (default: all) -> [B, Co*H*W]."""
        self._check_table(inputs, self.in_width, 'inputs')
        index = self._index(index, inputs.shape[0])
        out = torch.empty((len(index), self.out_width), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            rc = self._lib.axt_conv_trainer_forward(self._h, inputs.data_ptr(), index.data_ptr(), len(index), out.data_ptr(),
                                                    _stream())
        if self.batch_stats and rc == -22:              # the one thing left to refuse here: fewer than 2 values per channel
            raise ValueError(self._lib.axt_last_error().decode())
        _lib.check(rc, 'axt_conv_trainer_forward')
        return out

    def step(self, inputs, index, dfeat, lr=None, eps=ADAM_EPS):
        """Backward pass of the batch the last forward() ran from dfeat [B, Co*H*W], the gradient with respect to its
        output (HeadTrainer.input_grad), and one Adam step of the four tensors."""
        self._check_table(inputs, self.in_width, 'inputs')
        self._check_table(dfeat, self.out_width, 'dfeat')
        index = self._index(index, inputs.shape[0])
        if len(index) != dfeat.shape[0]:
            raise ValueError(f'{dfeat.shape[0]} gradients for a batch of {len(index)}')
        P = self.P
        with torch.cuda.device(self.device):
            _lib.check(self._lib.axt_conv_trainer_step(self._h, inputs.data_ptr(), index.data_ptr(), len(index),
                                                       dfeat.data_ptr(), float(P['LR'] if lr is None else lr), ADAM_BETAS[0],
                                                       ADAM_BETAS[1], float(eps), float(P['WEIGHT_DECAY']), _stream()),
                       'axt_conv_trainer_step')

    def input_grad(self, dfeat):
        """The gradient of the loss with respect to the input rows the last forward() read: dfeat [B, Co*H*W] ->
        [B, Ci*H*W] (axt_conv_trainer_input_grad). From gamma and the weights as they stand, so call it before step(); it
        changes nothing that step() reads."""
        self._check_table(dfeat, self.out_width, 'dfeat')
        out = torch.empty((dfeat.shape[0], self.in_width), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self._lib.axt_conv_trainer_input_grad(self._h, dfeat.data_ptr(), dfeat.shape[0], out.data_ptr(),
                                                             _stream()), 'axt_conv_trainer_input_grad')
        return out

    def _shapes(self):
        return [(self.Co, self.Ci, 3, 3), (self.Co,), (self.Co,), (self.Co,)]

    def weights(self):
        """conv.weight, conv.bias, batchnorm.weight, batchnorm.bias as numpy arrays."""
        out = [np.empty(s, np.float32) for s in self._shapes()]
        with torch.cuda.device(self.device):
            _lib.check(self._lib.axt_conv_trainer_read_weights(self._h, *[a.ctypes.data for a in out]),
                       'axt_conv_trainer_read_weights')
        return out

    def moments(self, tensor):
        """Adam state of tensor 0..3 (the order of weights()): (m, v, step count)."""
        shape = self._shapes()[tensor]
        m, v = np.empty(shape, np.float32), np.empty(shape, np.float32)
        step = ctypes.c_int64()
        with torch.cuda.device(self.device):
            _lib.check(self._lib.axt_conv_trainer_read_moments(self._h, int(tensor), m.ctypes.data, v.ctypes.data,
                                                               ctypes.byref(step)), 'axt_conv_trainer_read_moments')
        return m, v, int(step.value)

    def stats(self):
        """BatchNorm's statistics as the handle holds them: dict(running_mean, running_var [Co] f32,
        num_batches_tracked: the forwards that ran with batch statistics, batch_mean, batch_var: the mean and biased
        variance of the last such forward, None before there was one)."""
        rm, rv, bm, bv = (np.empty(self.Co, np.float32) for _ in range(4))
        n = ctypes.c_int64()
        with torch.cuda.device(self.device):
            _lib.check(self._lib.axt_conv_trainer_read_stats(self._h, rm.ctypes.data, rv.ctypes.data, ctypes.byref(n), None,
                                                             None), 'axt_conv_trainer_read_stats')
            if n.value:
                _lib.check(self._lib.axt_conv_trainer_read_stats(self._h, None, None, None, bm.ctypes.data, bv.ctypes.data),
                           'axt_conv_trainer_read_stats')
        return dict(running_mean=rm, running_var=rv, num_batches_tracked=int(n.value), batch_mean=bm if n.value else None,
                    batch_var=bv if n.value else None)

    def export_to(self, detector, block=None):
        """The block as it stands into conv block `block` (0..7 of the package's numbering; default: the one block_key
        names) of a live Detector on the same device, without a host copy (axt_conv_trainer_export:
        Detector.load_conv_block from the trainer's own device tensors, on the current stream): the four trained tensors
        and the running statistics, the moved ones with batch_stats. The detector then computes what
        Detector(self.state_dict()) computes in this block, byte for byte, in every arithmetic. A trainer whose channels or
        stride are not that block's is refused."""
        from .hotpath import CONV_BLOCKS, conv_block_key
        _check_export(self, detector)
        if block is None:
            known = [conv_block_key(i) for i in range(len(CONV_BLOCKS))]
            if self.block_key not in known:
                raise ValueError(f'{self.block_key} is no conv block of the detector: say which block (0..7) to export to')
            block = known.index(self.block_key)
        if isinstance(block, bool) or not isinstance(block, (int, np.integer)) or not 0 <= block < len(CONV_BLOCKS):
            raise IndexError(f'conv block must be in 0..{len(CONV_BLOCKS) - 1}, got {block!r}')
        with torch.cuda.device(self.device):
            rc = self._lib.axt_conv_trainer_export(self._h, detector._h, int(block), _stream())
        if rc == -22:
            raise ValueError(self._lib.axt_last_error().decode())
        _lib.check(rc, 'axt_conv_trainer_export')
        detector.state_dict_source = None

    def state_dict(self, base=None):
        """The state dict this trainer was built from (or `base`) with the block's four trained tensors replaced (numpy
        f32); the running statistics and num_batches_tracked pass through. With batch_stats, running_mean and running_var
        are replaced too and num_batches_tracked grows by the number of forwards, each in the dtype and container (torch
        tensor or numpy array) it came in; a missing num_batches_tracked is created as int64."""
        sd = dict(self._sd if base is None else base)
        sd.update(zip(self.keys[:4], self.weights()))
        if self.batch_stats:
            st = self.stats()

            def like(old, new):
                if isinstance(old, torch.Tensor):
                    return torch.from_numpy(np.asarray(new)).to(dtype=old.dtype, device=old.device)
                return np.asarray(new).astype(np.asarray(old).dtype)

            for k, name in zip(self.keys[4:6], ('running_mean', 'running_var')):
                sd[k] = like(sd[k], st[name])
            k = f'{self.block_key}.{CONV_COUNTER}'
            old = sd.get(k)
            if old is None:
                sd[k] = np.array(st['num_batches_tracked'], np.int64)
            else:
                before = int(old.cpu()) if isinstance(old, torch.Tensor) else int(np.asarray(old))
                sd[k] = like(old, np.asarray(before + st['num_batches_tracked']))
        return sd


def _check_maps(x, H, W, what):
    if not (isinstance(x, torch.Tensor) and x.is_cuda and x.is_contiguous() and x.dtype == torch.float32
            and x.numel() % (H * W) == 0):
        raise ValueError(f'{what} must be a contiguous f32 tensor of whole {H} x {W} maps on the GPU')
    return x.numel() // (H * W)


def maxpool2_forward(x, H, W):
    """nn.MaxPool2d(2, 2) on every H x W map of x (f32 on the GPU, any leading shape, H*W innermost) -> a flat tensor of
    the [H//2, W//2] maps in the same order (axt_maxpool2_forward)."""
    n = _check_maps(x, H, W, 'x')
    out = torch.empty(n * (H // 2) * (W // 2), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().axt_maxpool2_forward(x.data_ptr(), n, int(H), int(W), out.data_ptr(), _stream()),
                   'axt_maxpool2_forward')
    return out


def maxpool2_backward(x, dout, H, W):
    """The gradient of maxpool2_forward(x, H, W) with respect to x from dout, the gradient with respect to its output: each
    window's gradient goes to its first maximum (torch's choice on the CPU), every other element is +0.0
    (axt_maxpool2_backward) -> a tensor shaped like x."""
    n = _check_maps(x, H, W, 'x')
    if _check_maps(dout, max(H // 2, 1), max(W // 2, 1), 'dout') != n or dout.device != x.device:
        raise ValueError(f'dout does not hold the {n} pooled maps of x')
    din = torch.empty_like(x)
    with torch.cuda.device(x.device):
        _lib.check(_lib.load().axt_maxpool2_backward(x.data_ptr(), dout.data_ptr(), n, int(H), int(W), din.data_ptr(),
                                                     _stream()), 'axt_maxpool2_backward')
    return din


class ConvTrunkTrainer:
    """Conv blocks first_block..7 of the state dict as ConvBlockTrainers chained on the device, a 2 x 2 max-pool behind
    every block whose `pooled` flag is set; the last n_trained of them are trained, the blocks in front run forward only and
    never step. forward / backward_and_step work on batches picked by index from a table [n_items, in_width] of
    first_block's inputs: Detector.trunk_features_frames(block=2) for first_block=3, hotpath.tile_stacks' stacks (as
    [B, 5*512*512]) for first_block=0. forward's output is what HeadTrainer.forward reads.
    block_keys, strides, pooled: per block first_block..7 its state-dict prefix, its convolution's stride and whether a pool
    follows it; in_size: the (H, W) of first_block's input maps. Defaults: the deployed architecture's, from hotpath's table
    of conv blocks, with stride 2 for conv blocks 0 and 1. batch_stats, momentum: train-mode BatchNorm
    (ConvBlockTrainer's) in the trained blocks; a forward-only block keeps its running statistics."""

    def __init__(self, state_dict, first_block, n_trained, parameters=None, max_batch=64, device='cuda:0', batch_stats=False,
                 momentum=0.1, block_keys=None, strides=None, pooled=None, in_size=None):
        from .hotpath import CONV_BLOCKS, CONV_MAP_SIDE, CONV_POOLED, conv_block_key
        n_all = len(CONV_BLOCKS)
        if isinstance(first_block, bool) or first_block not in range(n_all):
            raise ValueError(f'first_block must be in 0..{n_all - 1}, got {first_block!r}')
        self.numbers = list(range(first_block, n_all))
        n = len(self.numbers)
        if isinstance(n_trained, bool) or n_trained not in range(n + 1):
            raise ValueError(f'n_trained must be in 0..{n} for first_block={first_block}, got {n_trained!r}')
        if block_keys is None:
            block_keys = [conv_block_key(i) for i in self.numbers]
        if strides is None:
            strides = [2 if i < 2 else 1 for i in self.numbers]
        if pooled is None:
            pooled = [CONV_POOLED[i] for i in self.numbers]
        if in_size is None:
            in_size = (CONV_MAP_SIDE[first_block] * (2 if first_block < 2 else 1),) * 2
        if not len(block_keys) == len(strides) == len(pooled) == n:
            raise ValueError(f'block_keys, strides and pooled describe conv blocks {first_block}..{n_all - 1}: {n} entries each')
        self.first_block, self.n_trained = int(first_block), int(n_trained)
        self.trained = [k >= n - self.n_trained for k in range(n)]
        self.pooled = [bool(p) for p in pooled]
        self.batch_stats = bool(batch_stats)
        self.blocks = []
        h, w = (int(v) for v in in_size)
        for key, s, pool, tr in zip(block_keys, strides, self.pooled, self.trained):
            ho, wo = (h - 1) // s + 1, (w - 1) // s + 1
            if pool and (ho < 2 or wo < 2):
                raise ValueError(f'{key}: maps of {ho} x {wo} leave its max-pool nothing')
            old = s == 1 and h <= 64 and w <= 64                    # the maps ConvBlockTrainer always took: its own calls
            self.blocks.append(ConvBlockTrainer(state_dict, key, parameters, map_size=(h, w), max_batch=max_batch,
                                                device=device, batch_stats=self.batch_stats and tr, momentum=momentum,
                                                stride=s, in_size=None if old else (h, w)))
            h, w = (ho // 2, wo // 2) if pool else (ho, wo)
        for a, b in zip(self.blocks, self.blocks[1:]):
            if a.Co != b.Ci:
                raise ValueError(f'{a.block_key} writes {a.Co} channels, {b.block_key} reads {b.Ci}')
        self.device, self.max_batch = self.blocks[0].device, int(max_batch)
        self.in_width = self.blocks[0].in_width
        self.out_width = self.blocks[-1].Co * h * w
        self._sd = state_dict
        self._kept = None

    @property
    def device_bytes(self):
        return sum(b.device_bytes for b in self.blocks)

    def forward(self, table, batch=None):
        """table f32 [n_items, in_width] on the GPU, batch: which rows (default: all) -> [B, out_width], the head's input
        rows. Every block's input and output are kept for backward_and_step."""
        x, rows, kept = table, batch, []
        for blk, pool in zip(self.blocks, self.pooled):
            f = blk.forward(x, rows)
            out = maxpool2_forward(f, blk.H, blk.W).reshape(f.shape[0], -1) if pool else f
            kept.append((x, rows, f))
            x, rows = out, _first_rows(f.shape[0], self.device)
        self._kept = kept
        return x

    def backward_and_step(self, table, batch, dfeat, lr=None, eps=ADAM_EPS):
        """From dfeat [B, out_width], the gradient with respect to forward's output of the same batch: back to front
        through the trained blocks, per block the gradient of the pool behind it, its input gradient where a trained block
        lies in front of it, then its Adam step -- so every gradient is taken from weights that have not moved yet. A
        forward-only block is never reached. table, batch: what forward read. Returns the gradients handed on, named per
        link by the conv block i whose output they belong to: 'p{i}' with respect to its pooled output, 'f{i}' with respect to
        its output in front of the pool (or the output itself where no pool follows)."""
        if self._kept is None or self._kept[-1][2].shape[0] != dfeat.shape[0]:
            raise ValueError('backward_and_step needs forward() on this batch first')
        grads, g = {}, dfeat
        first_trained = len(self.blocks) - self.n_trained
        for k in range(len(self.blocks) - 1, first_trained - 1, -1):
            blk, (x, rows, f) = self.blocks[k], self._kept[k]          # (the first block's x, rows are table, batch)
            if self.pooled[k]:
                g = grads[f'f{self.numbers[k]}'] = maxpool2_backward(f, g, blk.H, blk.W).reshape(f.shape)
            dx = blk.input_grad(g) if k > first_trained else None
            blk.step(x, rows, g, lr=lr, eps=eps)
            if dx is not None:
                grads[f"{'p' if self.pooled[k - 1] else 'f'}{self.numbers[k - 1]}"] = g = dx
        return grads

    def export_to(self, detector):
        """ConvBlockTrainer.export_to for the trained blocks, each into the conv block its key names; a forward-only block did
        not change and is left alone."""
        for blk, trained in zip(self.blocks, self.trained):
            if trained:
                blk.export_to(detector)

    def state_dict(self, base=None):
        """The state dict this trunk was built from (or `base`) with the trained blocks' four tensors each replaced (numpy
        f32), and with batch_stats their running statistics and batch counts (ConvBlockTrainer.state_dict); everything
        else, a forward-only block's tensors included, passes through."""
        sd = dict(self._sd if base is None else base)
        for blk, trained in zip(self.blocks, self.trained):
            if trained:
                sd = blk.state_dict(sd)
        return sd


STAGE_BLOCKS = (5, 6, 7)                            # the last conv stage: conv blocks 5 and 6, the max-pool, conv block 7


class ConvStageTrainer(ConvTrunkTrainer):
    """The last conv stage of the state dict -- conv block 5, conv block 6, the 2 x 2 max-pool, conv block 7 -- as the
    three-block case of ConvTrunkTrainer: stride 1 throughout, one pool behind the second block, the last `depth` (1..3)
    blocks trained. The table [n_items, Ci*H*W] is Detector.features_frames(block=4); forward, backward_and_step (whose
    gradients are 'p6', 'f6', 'f5'), export_to, state_dict and device_bytes are the trunk's, contract included.
    block_keys, map_size: the three blocks' state-dict prefixes and the (H, W) of the maps the first two run on (the third
    runs on the pooled (H // 2, W // 2)); default: the deployed architecture's, from hotpath's table of conv blocks."""

    def __init__(self, state_dict, depth=3, parameters=None, max_batch=64, device='cuda:0', block_keys=None, map_size=None,
                 batch_stats=False, momentum=0.1):
        from .hotpath import CONV_MAP_SIDE
        if depth not in (1, 2, 3):
            raise ValueError(f'depth must be 1, 2 or 3, got {depth!r}')
        if block_keys is None:
            map_size = (CONV_MAP_SIDE[STAGE_BLOCKS[0]],) * 2
        elif len(block_keys) != 3 or map_size is None:
            raise ValueError('a stage is three blocks (block_keys) on maps of map_size = (H, W)')
        self.depth = int(depth)
        self.H, self.W = (int(v) for v in map_size)
        if self.H < 2 or self.W < 2:
            raise ValueError(f'maps of {self.H} x {self.W} leave the max-pool nothing')
        super().__init__(state_dict, STAGE_BLOCKS[0], self.depth, parameters, max_batch, device, batch_stats, momentum,
                         block_keys=block_keys, strides=(1, 1, 1), pooled=(False, True, False), in_size=map_size)


def save_checkpoint(state_dict, filename):
    """The reference's checkpoint layout (utils.py:258-264) without optimiser state; setup_inference(weights=filename)
    and the reference's load_checkpoint read it."""
    sd = {k: (v.detach().cpu() if isinstance(v, torch.Tensor) else torch.from_numpy(np.array(v))) for k, v in state_dict.items()}
    torch.save({'state_dict': sd, 'optimizer': None, 'lr_schedular': None}, filename)


def _augmented_epoch(frames, labels, transform, draw, min_pos_rate, max_redraws, warped):
    """One epoch's draw: warp the frames by `transform`, or by draw() again and again while prepare_data's
    rate stays below min_pos_rate (one_epoch's loop, core_functionality.py:141, which has no limit: here max_redraws)
    -> (transform, warped frames, kept tiles, (lx, ly, count))."""
    from . import augment
    from .hotpath import tile_list
    H, W = int(frames.shape[1]), int(frames.shape[2])
    best = -1.0
    for _ in range(1 + (max_redraws if transform is None else 0)):
        tf = augment.as_transform(transform) if transform is not None else draw()
        warped, occ = augment.augment_frames(frames, tf, return_occupancy=True, out=warped)
        lab = augment.transform_labels(labels, tf, H, W)
        occ = occ.cpu()
        if transform is not None:                       # an explicit transform is used as it is
            break
        rate = augment.pos_label_rate(occ, *lab)
        best = max(best, rate)
        if rate >= min_pos_rate:
            break
    else:
        raise RuntimeError(f'{max_redraws} redraws of the augmentation gave no labels-per-tile rate of {min_pos_rate} or '
                           f'more (best: {best:.3f}): too few labels for USE_TRANSFORMS, or lower min_pos_rate')
    tiles = tile_list(occ.amax(0), H, W)                # kept: not empty at some time point (Timelapse.py:551-558)
    if not tiles:
        raise ValueError(f'{tf} leaves every frame empty')
    return tf, warped, tiles, lab


def _epoch_metrics(sd, timelapse, labels, parameters, subset, detector=None):
    """one_epoch's every-tenth-epoch evaluation (core_functionality.py:150-161) of the detector with state dict `sd` (or of
    `detector`, a live one that holds these weights already: the test-loss detector of _fine_tune) on the
    detection frames `subset` of a labelled timelapse: detect, sum compute_TP_FP_FN('all', t) over the frames (one launch:
    detection_confusion), precision / recall / F1 at the 13 thresholds as compute_prc_rcl_F1's Series."""
    from . import params as _params
    from .detections import AxonDetections
    from .hotpath import Detector
    P = _params.load_parameters()
    P.update(parameters or {})
    if detector is None:
        detector = Detector(sd, max_batch=32, device=timelapse.device)
    dets = AxonDetections(detector, timelapse, P, None, timepoint_subset=subset)
    if labels is not None:
        dets.set_groundtruth([labels[t] for t in subset])
    dets.detect_dataset()
    return dets.compute_prc_rcl_F1(dets.detection_confusion().sum(axis=0), return_dataframe=True)


def fine_tune_head(timelapse, labels=None, model=None, parameters=None, epochs=1, dest_dir=None, seed=None,
                   use_transforms=None, transforms=None, min_pos_rate=0.65, max_redraws=50, test_timelapse=None,
                   metrics_every=10, train_conv_blocks=None, bn_batch_stats=False, bn_momentum=0.1, test_loss=False,
                   train_last_conv=False):
    """Train fcs.1/3/5 of `model` (a Detector, or a state dict) on the labelled timelapse for `epochs` epochs of
    one_epoch / run_epoch (core_functionality.py:109-165) -> (state_dict, history). labels: per detection frame (x, y) or
    (x, y, ids), as AxonDetections.set_groundtruth takes them. history: DataFrame, one column per epoch, rows the
    reference's five loss components, each the mean over the epoch's batches. dest_dir: E{epoch:04}.pth checkpoints for
    the epochs in parameters['MODEL_CHECKPOINTS'] (default: the last one).

    use_transforms: a list of augmentation keys (parameters['USE_TRANSFORMS']: 'vflip', 'hflip', 'rot', 'translateY',
    'translateX'). Every epoch then draws one transform (augment.draw_transform, from a generator of its own seeded by
    `seed`), warps the frames and the labels with it, redraws while the labels-per-tile rate (augment.pos_label_rate) is
    below min_pos_rate -- RuntimeError after max_redraws -- and recomputes the trunk features and the targets of the
    tiles the warped frames keep. transforms: instead, one explicit transform per epoch (augment.Transform or a dict of
    its fields), used as given. The transforms used are history.attrs['transforms'], which `transforms=` replays. With
    neither (None or an empty list) nothing is augmented and the features are computed once.

    labels=None takes the labels of a labelled timelapse (prepare_training_data). test_timelapse: a labelled timelapse to
    validate on. Then every epoch with epoch % metrics_every == 0 ends with one_epoch's evaluation
    (core_functionality.py:150-161): a Detector built from the trainer's weights of that moment (one host round trip)
    detects every 10th frame of the train set, from a start in 0..9 drawn from a generator of its own seeded by `seed`
    (taken modulo the number of frames where the set has fewer than ten), and all frames of the test set; the confusion
    counts are summed over the frames and turned into precision / recall / F1 at the 13 thresholds. The result is
    history.attrs['metrics']: a DataFrame, rows (metric, threshold), columns (epoch, 'train' | 'test'). The evaluation
    reads the weights only: history and the returned state dict are what they are without it.

    train_last_conv: also train the last convolutional block (ConvNet.ConvBlock_10: conv.weight, conv.bias,
    batchnorm.weight, batchnorm.bias; BatchNorm keeps its running statistics, as at inference) with the same learning
    rate, Adam eps and weight decay. The cached table is then the trunk's output one block earlier
    (Detector.features_frames(block=6)), and a step is conv forward, head forward, loss, the head's input gradient, conv
    step, head step. The returned state dict and the checkpoints carry both sets of tensors.

    train_conv_blocks: how many of the last conv blocks to train with the head, 0..3 (None: 1 with train_last_conv, else
    0; train_last_conv=True with another number than 1 is a ValueError). 0 is the head alone, 1 is train_last_conv. 3
    trains the whole last stage (ConvTrunkTrainer from conv block 5 on, the chain that ConvStageTrainer is: conv blocks 5
    and 6 on 32 x 32 maps, the max-pool, conv block 7) on the cached table Detector.features_frames(block=4); a step is
    the three forwards with the pool, head forward, loss, the head's input gradient, then back to front each block's
    input gradient, the pool's gradient and the block's step, and the head's step. 2 reads the same table (conv block 5's output is not offered as one) and runs conv block 5 forward
    only: its tensors come back as they went in. Every trained block takes the head's learning rate, Adam eps and weight
    decay and keeps its running statistics. Conv blocks 0-4 stay frozen.

    bn_batch_stats: train-mode BatchNorm in the trained conv blocks, as the reference's model.train() has it
    (bn_momentum: nn.BatchNorm2d's momentum, 0.1). Each trained block normalises a batch with the batch's own mean and
    biased variance, its gradients go through those statistics (conv.bias then has gradient 0 by definition and moves by
    weight decay alone), and every forward moves running_mean, running_var and num_batches_tracked; the returned state
    dict and the checkpoints carry them, and the every-tenth-epoch evaluation reads them. A forward-only block
    (train_conv_blocks=2's conv block 5) and the frozen trunk keep their running statistics. With the head alone
    (train_conv_blocks=0) it is a ValueError: nothing would use it. Default False: running statistics, never updated.

    test_loss: also the loss on the test set after every epoch, as the reference's optimize() runs one_epoch on its test
    data with model.eval() (experiment.py). Needs a labelled test_timelapse (ValueError otherwise). One evaluation Detector
    is created before the first epoch; after every training epoch the trainers export their weights of that moment into it
    on the device (export_to: no host copy, no repacking on the host), it runs its ordinary inference forward -- eval mode
    by construction: the running statistics, the ones bn_batch_stats has moved included -- over all frames and kept tiles
    of the test set, and HeadTrainer.loss is taken on batches of BATCH_SIZE in order, unshuffled, DROP_LAST honoured,
    against yolo_targets of the test labels (made once). The result is history.attrs['test_loss']: a DataFrame with
    history's five rows and one column per epoch, each the mean over the test batches. The test set is never augmented
    (the reference passes USE_TRANSFORMS to its test set too). It reads weights only: history, the
    returned state dict and the checkpoints are what they are without it. The every-tenth-epoch evaluation then uses the
    same detector for the test set instead of building one. A test batch may not be larger than the trainer's own
    (min(BATCH_SIZE, training items)): ValueError."""
    if train_conv_blocks is None:
        depth = 1 if train_last_conv else 0
    else:
        if isinstance(train_conv_blocks, bool) or train_conv_blocks not in (0, 1, 2, 3):
            raise ValueError(f'train_conv_blocks must be 0, 1, 2 or 3, got {train_conv_blocks!r}')
        depth = int(train_conv_blocks)
        if train_last_conv and depth != 1:
            raise ValueError(f'train_last_conv=True means train_conv_blocks=1, not {depth}')
    return _fine_tune('fine_tune_head', timelapse, labels, model, parameters, epochs, dest_dir, seed, use_transforms,
                      transforms, min_pos_rate, max_redraws, test_timelapse, metrics_every, depth, bn_batch_stats, bn_momentum,
                      test_loss)


# fine_tune_detector's depth (how many of the last conv blocks train) -> (the conv block whose output the cached table
# holds, None: no table, the raw stacks are gathered per batch; the first conv block the trunk trainer runs, read at every
# depth of 1 or more, None: no trunk)
DEPTH_INPUT = {0: (7, None), 1: (6, 7), 2: (4, 5), 3: (4, 5), 4: (2, 3), 5: (2, 3), 6: (None, 0), 7: (None, 0), 8: (None, 0)}


def fine_tune_detector(timelapse, labels=None, model=None, parameters=None, epochs=1, dest_dir=None, seed=None,
                       use_transforms=None, transforms=None, min_pos_rate=0.65, max_redraws=50, test_timelapse=None,
                       metrics_every=10, train_conv_blocks=0, bn_batch_stats=False, bn_momentum=0.1, test_loss=False):
    """fine_tune_head for every depth: train the head and the last train_conv_blocks (0..8, default 0) conv blocks of
    `model` -> (state_dict, history). Every other argument, the history, the checkpoints, the augmentation and the
    evaluation are fine_tune_head's. Depths 0..3 run exactly what fine_tune_head runs; every depth of 1 or more is one
    ConvTrunkTrainer from the first block DEPTH_INPUT names. Beyond 3:

      4  the cached table is conv block 2's output after its pool (Detector.trunk_features_frames(block=2), 1.3 MB per
         item); conv block 3 runs forward only and comes back as it went in, conv blocks 4..7 train
      5  the same table; conv blocks 3..7 train
      6  no table: every batch gathers its raw 5-frame stacks from the frames (hotpath.tile_stacks); conv blocks 0 and 1,
         the stride-2 front, run forward only, conv blocks 2..7 train
      7  raw stacks; conv block 0 runs forward only, conv blocks 1..7 train
      8  raw stacks; all eight conv blocks train, so a detector can be trained from a random start

    A step is the chain's forwards with the three pools, head forward, loss, the head's input gradient, then back to front
    per trained block the gradient of the pool behind it, its input gradient, its step, and last the head's step: every
    gradient is taken from weights that have not moved. bn_batch_stats works in the trained blocks at every depth; a
    forward-only block keeps its running statistics. At depths 6..8 an augmented epoch recomputes no table: the stacks are
    gathered from the warped frames. test_loss: fine_tune_head's, at every depth."""
    if isinstance(train_conv_blocks, bool) or train_conv_blocks not in DEPTH_INPUT:
        raise ValueError(f'train_conv_blocks must be in 0..{max(DEPTH_INPUT)}, got {train_conv_blocks!r}')
    return _fine_tune('fine_tune_detector', timelapse, labels, model, parameters, epochs, dest_dir, seed, use_transforms,
                      transforms, min_pos_rate, max_redraws, test_timelapse, metrics_every, int(train_conv_blocks),
                      bn_batch_stats, bn_momentum, test_loss)


class _TableInput:
    """The step loop's input at the depths that read a cached table of the frozen trunk's output after conv block `block`:
    fill() computes it from the epoch's frames, pick() hands a batch's rows to whoever reads them."""

    def __init__(self, detector, block, n_rows=None):
        from .hotpath import BLOCK_FEATURES, TRUNK_FEATURES
        self.detector, self.block = detector, block
        self._tap = detector.features_frames if block in BLOCK_FEATURES else detector.trunk_features_frames
        width = BLOCK_FEATURES[block] if block in BLOCK_FEATURES else TRUNK_FEATURES[block]
        # augmented epochs keep different tiles: one table for all tiles (n_rows), of which an epoch uses the first rows
        self.out = None if n_rows is None else torch.empty((n_rows, width), dtype=torch.float32, device=detector.device)

    def fill(self, frames, tile_yx):
        self.table = self._tap(frames, tile_yx, out=self.out, block=self.block)
        return self.table.shape[0]

    def pick(self, batch):
        return self.table, batch


class _StackInput:
    """The step loop's input at the depths that train the front: nothing is cached (a stack is 5.2 MB per item), pick()
    gathers the batch's raw stacks from the epoch's frames into one buffer, of which the trunk reads rows 0..B-1."""

    def __init__(self, max_batch, device):
        from .hotpath import TILE
        self.buf = torch.empty((max_batch, 5 * TILE * TILE), dtype=torch.float32, device=device)

    def fill(self, frames, tile_yx):
        self.frames, self.tile_yx = frames, np.ascontiguousarray(tile_yx, np.int32).reshape(-1, 2)
        return (frames.shape[0] - 4) * len(self.tile_yx)

    def pick(self, batch):
        from .hotpath import tile_stacks
        stacks = tile_stacks(self.frames, self.tile_yx, batch, out=self.buf)
        return stacks.view(len(batch), -1), _first_rows(len(batch), self.buf.device)


def _fine_tune(name, timelapse, labels, model, parameters, epochs, dest_dir, seed, use_transforms, transforms, min_pos_rate,
               max_redraws, test_timelapse, metrics_every, depth, bn_batch_stats, bn_momentum, test_loss=False):
    """fine_tune_head and fine_tune_detector behind their own checks of the depth: the rest of the checks, the set-up and
    the one step loop. The trunk (none, or one chain of conv blocks) and the input it reads (a cached table, or stacks
    gathered per batch) are chosen by the depth (DEPTH_INPUT); the loop is the same for all."""
    import pandas as pd
    from .hotpath import Detector
    if bn_batch_stats and depth == 0:
        raise ValueError('bn_batch_stats=True needs trained conv blocks (train_conv_blocks >= 1): the head has no BatchNorm')
    if bn_batch_stats and not 0 < float(bn_momentum) <= 1:
        raise ValueError(f'bn_momentum must be in (0, 1], got {bn_momentum!r}')
    block, first_block = DEPTH_INPUT[depth]             # which conv block's output the cached table holds; the trunk's first
    for tl in (timelapse, test_timelapse):
        if getattr(tl, 'frame_sharded', False):
            raise NotImplementedError('fine-tuning on a frame-sharded timelapse is not implemented: train in a single '
                                      'process on the whole timelapse')
    if model is None:
        raise ValueError(f'{name} needs the model to start from: a Detector or a state dict')
    explicit_labels = labels is not None
    if labels is None:
        labels = getattr(timelapse, 'labels', None)
        if labels is None:
            raise ValueError('no labels: pass them, or a labelled timelapse (prepare_training_data)')
    with_metrics = test_timelapse is not None and bool(metrics_every)
    if with_metrics and not getattr(test_timelapse, 'labelled', False):
        raise ValueError('test_timelapse carries no labels (prepare_training_data makes labelled timelapses)')
    if test_loss and (test_timelapse is None or not getattr(test_timelapse, 'labelled', False)):
        raise ValueError('test_loss=True needs a labelled test_timelapse (prepare_training_data makes labelled timelapses)')
    if len(labels) != len(timelapse):
        raise ValueError(f'{len(labels)} label frames for {len(timelapse)} detection frames')
    augmented = bool(use_transforms) or transforms is not None
    if transforms is not None and use_transforms:
        raise ValueError('pass use_transforms (drawn every epoch) or transforms (one per epoch), not both')
    if transforms is not None and len(transforms) != epochs:
        raise ValueError(f'{len(transforms)} transforms for {epochs} epochs')
    P = _train_parameters(parameters)
    if isinstance(model, Detector):
        detector, sd = model, getattr(model, 'state_dict_source', None)
        if sd is None:
            raise ValueError('this Detector does not remember its state dict; pass the state dict instead')
    else:
        sd = model.get('state_dict', model)
        detector = Detector(sd, max_batch=32, device=timelapse.device)
    timelapse.make_resident()
    bs = int(P['BATCH_SIZE'])
    if augmented:
        from . import augment
        unknown = [k for k in (use_transforms or []) if k not in augment.TRANSFORM_KEYS]
        if unknown:
            raise ValueError(f'unknown augmentation keys {unknown}; known: {augment.TRANSFORM_KEYS}')
        n_rows = len(timelapse) * timelapse.ytiles * timelapse.xtiles
        source = _TableInput(detector, block, n_rows) if block is not None else _StackInput(bs, timelapse.device)
        warped = torch.empty_like(timelapse.frames)
        label_xy = augment.label_floats(labels)
        label_xy = (*label_xy, np.full(len(labels), label_xy[0].shape[1], np.int32))
        # the draws have a generator of their own, so that replaying them through `transforms` leaves the batch order alone
        t_rng = np.random.default_rng(np.random.SeedSequence(seed).spawn(1)[0])
        draw = lambda: augment.draw_transform(use_transforms, t_rng)
        used = []
        trainer = HeadTrainer(sd, P, max_batch=bs, device=timelapse.device)
    else:
        tile_yx = timelapse.tile_yx
        n_items = len(timelapse) * len(np.reshape(tile_yx, (-1, 2)))
        source = _TableInput(detector, block) if block is not None else _StackInput(min(bs, n_items), timelapse.device)
        n_items = source.fill(timelapse.frames, tile_yx)
        targets = yolo_targets(labels, tile_yx, device=timelapse.device).reshape(-1, S, S, 4)
        trainer = HeadTrainer(sd, P, max_batch=min(bs, n_items), device=timelapse.device)
    # the conv blocks in front of the head: one chain from first_block on, its last `depth` blocks trained, or none
    trunk = ConvTrunkTrainer(sd, first_block, depth, P, max_batch=trainer.max_batch, device=timelapse.device,
                             batch_stats=bn_batch_stats, momentum=bn_momentum) if depth else None

    def current():
        """The state dict of this moment: the head's tensors, and the conv blocks' where they are trained."""
        return trunk.state_dict(trainer.state_dict()) if trunk else trainer.state_dict()

    eval_detector = None
    if test_loss:
        # one detector for every epoch's look at the test set: the trainers export into it on the device
        test_timelapse.make_resident()
        test_tiles = test_timelapse.tile_yx
        test_targets = yolo_targets(test_timelapse.labels, test_tiles, device=timelapse.device).reshape(-1, S, S, 4)
        test_batches = epoch_batches(test_targets.shape[0], bs, False, P['DROP_LAST'], None)
        if not test_batches:
            raise ValueError(f'DROP_LAST leaves no batch of {bs} among the {test_targets.shape[0]} test items')
        if len(test_batches[0]) > trainer.max_batch:
            raise ValueError(f'a test batch of {len(test_batches[0])} items is larger than the training batches '
                             f'({trainer.max_batch}): the train set holds less than one batch')
        eval_detector = Detector(sd, max_batch=32, device=timelapse.device)
        test_history = {}

    def test_epoch():
        """The loss components of the weights of this moment on the test set: export, inference forward, loss per batch."""
        trainer.export_to(eval_detector)
        if trunk:
            trunk.export_to(eval_detector)
        eval_detector.set_arith('f32')                  # (the evaluation below may have switched it: CNN_ARITH)
        yolo = eval_detector.detect_frames(test_timelapse.frames, test_tiles).reshape(-1, S, S, 3)
        rows = []
        for batch in test_batches:                      # in order: a batch is a run of rows
            comp, _ = trainer.loss(yolo[int(batch[0]):int(batch[-1]) + 1], test_targets, batch)
            rows.append([comp[k] for k in COMPONENTS])
        return np.mean(np.array(rows, np.float64).reshape(-1, 5), axis=0)

    rng = np.random.default_rng(seed)
    checkpoints = (parameters or {}).get('MODEL_CHECKPOINTS') or [epochs - 1]
    history, metrics = {}, {}
    m_rng = np.random.default_rng(np.random.SeedSequence(seed).spawn(2)[1])      # the evaluation's own draws
    for epoch in range(epochs):
        if augmented:
            tf, warped, tile_yx, lab = _augmented_epoch(timelapse.frames, label_xy, None if transforms is None else
                                                        transforms[epoch], draw, min_pos_rate, max_redraws, warped)
            used.append(tf)
            n_items = source.fill(warped, tile_yx)
            targets = yolo_targets(lab, tile_yx, device=timelapse.device).reshape(-1, S, S, 4)
        lr = learning_rate(P['LR'], P['LR_DECAYRATE'], epoch)
        rows = []
        for batch in epoch_batches(n_items, bs, P['SHUFFLE'], P['DROP_LAST'], rng):
            # what the head reads: the trunk's output for this batch, of which it takes rows 0..B-1, or the cached table
            features, rows_in = source.pick(batch)
            if trunk:
                feats, head_rows = trunk.forward(features, rows_in), _first_rows(len(batch), trainer.device)
            else:
                feats, head_rows = features, rows_in
            yolo = trainer.forward(feats, head_rows)
            comp, dy = trainer.loss(yolo, targets, batch)
            # the order: the head's input gradient is taken from the head's weights before they move, so before any step;
            # then the trunk steps (back to front, each block's input gradient before its own step), then the head
            if trunk:
                dfeat = trainer.input_grad(dy)
                trunk.backward_and_step(features, rows_in, dfeat, lr=lr)
            trainer.step(feats, head_rows, dy, lr=lr)
            rows.append([comp[k] for k in COMPONENTS])
        history[epoch] = np.mean(np.array(rows, np.float64).reshape(-1, 5), axis=0)
        if dest_dir is not None and epoch in checkpoints:
            os.makedirs(dest_dir, exist_ok=True)
            save_checkpoint(current(), f'{dest_dir}/E{epoch:04}.pth')
        if test_loss:
            test_history[epoch] = test_epoch()
        if with_metrics and epoch % int(metrics_every) == 0:
            now = current()
            tstart = int(m_rng.integers(0, 10)) % len(timelapse)
            metrics[(epoch, 'train')] = _epoch_metrics(now, timelapse, labels if explicit_labels else None, parameters,
                                                       list(range(tstart, len(timelapse), 10)))
            metrics[(epoch, 'test')] = _epoch_metrics(now, test_timelapse, None, parameters,
                                                      list(range(len(test_timelapse))), detector=eval_detector)
    history = pd.DataFrame(history, index=list(COMPONENTS))
    if with_metrics:
        history.attrs['metrics'] = pd.DataFrame(metrics)
    if augmented:
        history.attrs['transforms'] = used
    if test_loss:
        history.attrs['test_loss'] = pd.DataFrame(test_history, index=list(COMPONENTS))
    return current(), history

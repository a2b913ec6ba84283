"""Layer-by-layer reference for the detector CNN (CPU only): every layer restated in torch f64 from the f32 tensors of the
state dict (`ref_*`), the same layer in plain f32 through the oracle's C loops (`yard_*`: the error a correct f32
implementation makes on this very input), a judge that compares a layer's output with both, and a driver that walks the
buffers a forward pass left on the GPU (axt_debug_cnn_activation), feeding every layer the GPU's own input to it, so that
errors do not accumulate from layer to layer and every layer meets the same tight bound.

The semantics restated here are model.py's (CNNBlock: conv 3x3 pad 1 + bias, eval BatchNorm eps 1e-5, LeakyReLU 0.1;
MaxPool2d(2,2) after blocks 2, 4, 6; flatten in (c, h, w) order; Linear + Sigmoid twice, Linear)."""
import ctypes
import os

import numpy as np
import torch
import torch.nn.functional as F

from axtrack_amd import synth
from oracle import oracle as orc

SPECS = synth.conv_layer_specs()            # [(cin, cout, stride, pool_after)] x 8
NAMES = synth.conv_block_names()
FC = ((1, True), (3, True), (5, False))     # (index in model.fcs, sigmoid after)
LAYER_NAMES = [f'conv block {i}' for i in range(8)] + ['fc1', 'fc2', 'grid']
BN_EPS = 1e-5
SLOPE = 0.1

torch.set_num_threads(min(len(os.sched_getaffinity(0)), 16))

# ---- the bound (nothing here is taken from the kernels under test)
# got is accepted when  max|got-ref| <= C_max * (max|yard-ref| + 1e-6)  and  rms(got-ref) <= C_rms * (rms(yard-ref) + 1e-7):
# the constants and floors tests/test_winograd_numerics.py uses for this very comparison (an f32 Winograd convolution
# against a direct f32 one, both measured against f64). The floors are NOT scaled by max|ref|: activations here reach 20-30
# with an rms near 1, so a floor of 1e-7 * max|ref| is five times the rms error of a plain f32 layer, and the two-term bf16
# split (rms 6.1 ... 8.4 times that of f32 with the plain floor, test_cnn_layers_cpu.py) would sink to 1.5 ... 2.6 and pass.
# The yardstick's output is itself rounded to f32, so its own error never falls far below an ulp of the largest outputs and
# the plain floors only matter for near-constant maps. No constant may exceed the caps: every fault seeded in
# test_cnn_layers_cpu.py lies above them.
CAP_MAX, CAP_RMS = 8.0, 4.0
FLOOR_MAX, FLOOR_RMS = 1e-6, 1e-7
BOUND_DEFAULT = (2.0, 1.5)
# Worst ratios measured on MI355X over every case of test_cnn_layers_gpu.py (per item; max / rms; full table in DESIGN.md 6.4a):
#   stride-2 kernels, blocks 0 and 1 (separate)      0.95 / 0.44, 1.93 / 0.96
#   fused stride-2 pair (blocks 0+1 from the frames)  1.96 / 0.97
#   f32 Winograd, blocks 2-7                          0.92 / 0.52
#   bf16x3, blocks 2-6                                1.78 / 0.86
#   direct f32 MFMA, blocks 2-7                       2.43 / 1.02   <- the only family beyond the default on max
#   fc1, fc2 (split-K GEMM + reduction), grid         0.92 / 0.50, 0.65 / 0.60, 0.51 / 0.67
# Exceptions per (arithmetic, layer): twice the worst measured ratio, rounded up to a whole number. The direct kernel's rms
# equals the yardstick's (1.0); its largest single error over 1.3 million outputs x 130 items lands up to 2.43x the
# largest of the CPU loops, which add the 9 * cin products in another order.
BOUND_OVERRIDES = {('f32_direct', layer): (5.0, BOUND_DEFAULT[1]) for layer in range(2, 8)}


def bound_for(arith, layer, fused_pair=False):
    """(C_max, C_rms) for a layer under an arithmetic; `fused_pair`: block 1 judged against blocks 0+1 from the frames."""
    b = BOUND_OVERRIDES.get((arith, 'fused01' if fused_pair else layer), BOUND_DEFAULT)
    assert b[0] <= CAP_MAX and b[1] <= CAP_RMS, f'bound {b} for {(arith, layer)} exceeds the caps {(CAP_MAX, CAP_RMS)}'
    return b


# ------------------------------------------------------------------------------------------------ f64 reference
def _t64(a):
    return torch.from_numpy(np.ascontiguousarray(a)).double()


def ref_block(sd, i, x):
    """Conv block i in f64: x [B,cin,H,W] (any float type) -> f64 [B,cout,H',W'], BatchNorm unfolded."""
    cin, cout, stride, pool = SPECS[i]
    pre = f'ConvNet.{NAMES[i]}.'
    y = F.conv2d(_t64(x), _t64(sd[pre + 'conv.weight']), _t64(sd[pre + 'conv.bias']), stride=stride, padding=1)
    mean, var = _t64(sd[pre + 'batchnorm.running_mean']), _t64(sd[pre + 'batchnorm.running_var'])
    gamma, beta = _t64(sd[pre + 'batchnorm.weight']), _t64(sd[pre + 'batchnorm.bias'])
    y = (y - mean[None, :, None, None]) / torch.sqrt(var + BN_EPS)[None, :, None, None] * gamma[None, :, None, None] \
        + beta[None, :, None, None]
    y = torch.where(y >= 0, y, SLOPE * y)
    if pool:
        y = F.max_pool2d(y, 2, 2)
    return y.numpy()


def ref_linear(sd, idx, x, sigmoid):
    """Linear layer model.fcs[idx] in f64: x [B,K] -> f64 [B,N]."""
    y = _t64(x) @ _t64(sd[f'fcs.{idx}.weight']).T + _t64(sd[f'fcs.{idx}.bias'])
    if sigmoid:
        y = 1.0 / (1.0 + torch.exp(-y))
    return y.numpy()


def ref_forward(sd, X):
    """The whole net in f64: X [B,5,512,512] -> f64 [B,12,12,3]."""
    x = X
    for i in range(8):
        x = ref_block(sd, i, x)
    x = x.reshape(x.shape[0], -1)
    for idx, sig in FC:
        x = ref_linear(sd, idx, x, sig)
    return x.reshape(-1, 12, 12, 3)


def ref_tail(sd, i, x):
    """The rest of the net in f64 from the output x of conv block i -> f64 [B,12,12,3]."""
    for k in range(i + 1, 8):
        x = ref_block(sd, k, x)
    x = x.reshape(x.shape[0], -1)
    for idx, sig in FC:
        x = ref_linear(sd, idx, x, sig)
    return x.reshape(-1, 12, 12, 3)


# ------------------------------------------------------------------------------------------------ f32 yardstick
def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def yard_block(sd, i, x, slope=SLOPE):
    """Conv block i in plain f32 on the CPU (orc_conv3x3_bn_lrelu + orc_maxpool2, as oracle.cnn_forward calls them)."""
    L = orc.lib()
    cin, cout, stride, pool = SPECS[i]
    pre = f'ConvNet.{NAMES[i]}.'
    x = np.ascontiguousarray(x, np.float32)
    B, C, H, W = x.shape
    assert C == cin
    Ho, Wo = (H + 2 - 3) // stride + 1, (W + 2 - 3) // stride + 1
    out = np.empty((B, cout, Ho, Wo), np.float32)
    arrs = [np.ascontiguousarray(sd[pre + k], np.float32) for k in
            ('conv.weight', 'conv.bias', 'batchnorm.weight', 'batchnorm.bias', 'batchnorm.running_mean',
             'batchnorm.running_var')]
    L.orc_conv3x3_bn_lrelu(_p(x), B, cin, H, W, *[_p(a) for a in arrs], cout, stride, ctypes.c_float(slope), _p(out))
    if pool:
        pooled = np.empty((B, cout, Ho // 2, Wo // 2), np.float32)
        L.orc_maxpool2(_p(out), B * cout, Ho, Wo, _p(pooled))
        out = pooled
    return out


def yard_linear(sd, idx, x, sigmoid):
    """Linear layer in plain f32 on the CPU (orc_linear)."""
    L = orc.lib()
    x = np.ascontiguousarray(x, np.float32)
    w = np.ascontiguousarray(sd[f'fcs.{idx}.weight'], np.float32)
    b = np.ascontiguousarray(sd[f'fcs.{idx}.bias'], np.float32)
    out = np.empty((x.shape[0], w.shape[0]), np.float32)
    L.orc_linear(_p(x), x.shape[0], w.shape[1], _p(w), _p(b), w.shape[0], 1 if sigmoid else 0, _p(out))
    return out


# ------------------------------------------------------------------------------------------------ weights with BN edges
def edge_state_dict(seed=7):
    """synth_state_dict(seed) edited the way trained checkpoints look and the synthetic ones never do: per conv block every
    third batchnorm.weight is negative, running_var spans 1e-3 ... 10 (log-spaced over the channels, in an order that does
    not follow the sign pattern) and the conv bias is 10x larger. A channel's conv weights and its bias/mean offset are
    scaled by sqrt(new var / old var), as a trained net's running_var follows the variance of the channel it normalises:
    the fold factor gamma/sqrt(var+eps) spans 0.24 ... 39 in magnitude while the activations stay O(10)."""
    sd = {k: np.array(v, copy=True) for k, v in synth.synth_state_dict(seed).items()}
    for bi, name in enumerate(NAMES):
        pre = f'ConvNet.{name}.'
        co = sd[pre + 'conv.weight'].shape[0]
        c = np.arange(co)
        gamma = sd[pre + 'batchnorm.weight'].astype(np.float64)
        gamma[c % 3 == 1] *= -1.0
        order = (c * 7 + bi) % co if co % 7 else (c * 3 + bi) % co          # a permutation: 7 (or 3) is coprime with cout
        var_new = 10.0 ** (-3.0 + 4.0 * order / (co - 1))
        k = np.sqrt(var_new / sd[pre + 'batchnorm.running_var'].astype(np.float64))
        sd[pre + 'batchnorm.weight'] = gamma.astype(np.float32)
        sd[pre + 'batchnorm.running_var'] = var_new.astype(np.float32)
        sd[pre + 'conv.weight'] = (sd[pre + 'conv.weight'].astype(np.float64) * k[:, None, None, None]).astype(np.float32)
        sd[pre + 'conv.bias'] = (10.0 * sd[pre + 'conv.bias'].astype(np.float64) * k).astype(np.float32)
        sd[pre + 'batchnorm.running_mean'] = (sd[pre + 'batchnorm.running_mean'].astype(np.float64) * k).astype(np.float32)
    return sd


# ------------------------------------------------------------------------------------------------ the judge
class LayerMismatch(AssertionError):
    pass


def judge(got, ref, yard, c_max=BOUND_DEFAULT[0], c_rms=BOUND_DEFAULT[1], layer='', items=None, tile=16, check=True):
    """Ratios (max, rms) of got's error against the yardstick's, both measured against the f64 reference:
        max|got-ref| / (max|yard-ref| + 1e-6),  rms(got-ref) / (rms(yard-ref) + 1e-7).
    Raises LayerMismatch when a ratio exceeds its constant, naming the worst element: layer, item (items[b] if given),
    channel, position, and whether it lies on the border of the map or of a `tile`-pixel tile of the kernel's grid."""
    got, ref, yard = np.asarray(got, np.float64), np.asarray(ref, np.float64), np.asarray(yard, np.float64)
    assert got.shape == ref.shape == yard.shape, (got.shape, ref.shape, yard.shape)
    if not np.isfinite(got).all():
        bad = np.unravel_index(int(np.argmin(np.isfinite(got))), got.shape)
        raise LayerMismatch(f'{layer}: non-finite value at {bad}')
    s = max(1.0, float(np.abs(ref).max()))
    eg, ey = np.abs(got - ref), np.abs(yard - ref)
    r_max = float(eg.max() / (ey.max() + FLOOR_MAX))
    r_rms = float(np.sqrt(np.mean(eg ** 2)) / (np.sqrt(np.mean(ey ** 2)) + FLOOR_RMS))
    if check and (r_max > c_max or r_rms > c_rms):
        idx = np.unravel_index(int(np.argmax(eg)), eg.shape)
        item = items[idx[0]] if items is not None else idx[0]
        if len(idx) == 4:
            _, ch, y, x = idx
            H, W = got.shape[2:]
            where = []
            if y in (0, H - 1) or x in (0, W - 1):
                where.append('map border')
            if y % tile in (0, tile - 1) or x % tile in (0, tile - 1):
                where.append(f'{tile}-pixel tile border')
            pos = f'channel {ch}, position (y {y}, x {x}) of {H}x{W}: {" and ".join(where) or "interior"}'
        else:
            pos = f'element {idx[1:]}'
        raise LayerMismatch(f'{layer}: error is {r_max:.2f}x (max; allowed {c_max}) and {r_rms:.2f}x (rms; allowed {c_rms}) that of a '
                            f'plain f32 layer on the same input. Worst element: item {item}, {pos}: got {got[idx]:.9g}, '
                            f'f64 reference {ref[idx]:.9g}, f32 yardstick {yard[idx]:.9g} (yardstick max error {ey.max():.3g}, '
                            f'max |ref| {s:.3g})')
    return r_max, r_rms


# ------------------------------------------------------------------------------------------------ item -> slot
def slots_after_forward(n_items, max_batch, chunk_a, chunk_b):
    """Which item each buffer's slots hold after forward_items (cnn.hip) ran n_items: a replay of its three loops, later
    writes replacing earlier ones. Returns [10] dicts slot -> item. Slots the pass did not write are absent."""
    held = [dict() for _ in range(10)]
    for base in range(0, n_items, max_batch):
        nb = min(n_items - base, max_batch)
        for cb in range(0, nb, chunk_b):
            nbb = min(nb - cb, chunk_b)
            for c in range(0, nbb, chunk_a):
                nc = min(nbb - c, chunk_a)
                for j in range(nc):
                    held[0][j] = held[1][j] = base + cb + c + j
                    held[2][c + j] = base + cb + c + j
            for j in range(nbb):
                held[3][j] = base + cb + j
                held[4][cb + j] = base + cb + j
        for k in range(5, 10):
            for j in range(nb):
                held[k][j] = base + j
    return held


def slots_after_chunked(calls, chunk_a, chunk_b):
    """The same for axt_cnn_front_frames calls [(item0, n_items), ...] followed by one axt_cnn_back over all of them."""
    held = [dict() for _ in range(10)]
    total = 0
    for item0, n in calls:
        for cb in range(0, n, chunk_b):
            nbb = min(n - cb, chunk_b)
            for c in range(0, nbb, chunk_a):
                nc = min(nbb - c, chunk_a)
                for j in range(nc):
                    held[0][j] = held[1][j] = item0 + cb + c + j
                    held[2][c + j] = item0 + cb + c + j
            for j in range(nbb):
                held[3][j] = item0 + cb + j
                held[4][item0 + cb + j] = item0 + cb + j
        total = max(total, item0 + n)
    for k in range(5, 10):
        for j in range(total):
            held[k][j] = j
    return held


# ------------------------------------------------------------------------------------------------ the driver
# tile of the kernel's work decomposition in OUTPUT pixels (what "tile border" means in a message): the stride-2 kernels
# work on 16x32 output tiles, the stride-1 kernels on 16x16 (32x16 for bf16x3) tiles before the pool
_TILE = [16, 16, 8, 16, 8, 16, 8, 16]


def walk_layers(read, sd, X, grid, held, arith, fused, label='', group=8, log=print):
    """Judge every layer of every item a pass left observable.

    read(which, slot0, n) -> f32 array (axt_debug_cnn_activation); X f32 [n_items,5,512,512]: the input of every item as
    the reference builds it (oracle.frame_tile_stack); grid f32 [n_items,12,12,3]: what the pass returned; held: the slot
    maps (slots_after_*); fused: the pass ran the fused front kernel (block 0 unobservable: block 1 is judged against blocks
    0+1 in f64 from the frames, yardstick = the two f32 layers chained).
    Layer k of item i is judged when buffer k holds it and the buffer of its input does; items whose input was overwritten
    by a later chunk are judged from the first layer whose input survives. Returns {layer: (worst max ratio, worst rms
    ratio, items judged)}; raises LayerMismatch after the walk, listing every layer that failed."""
    n_items = X.shape[0]
    where = [{item: slot for slot, item in h.items()} for h in held]          # item -> slot, per buffer
    if fused:
        where[0] = {}
    ratios = {}
    failures = []

    def fetch(which, items):
        out = np.empty((len(items),) + read(which, 0, 0).shape[1:], np.float32)
        slots = [where[which][i] for i in items]
        k = 0
        while k < len(items):                       # runs of consecutive slots in one copy
            e = k + 1
            while e < len(items) and slots[e] == slots[e - 1] + 1:
                e += 1
            out[k:e] = read(which, slots[k], e - k)
            k = e
        return out

    def record(layer, got, ref, yard, items, fused_pair=False):
        c_max, c_rms = bound_for(arith, layer, fused_pair)
        for b, item in enumerate(items):            # per item: one bad item is not diluted by the good ones
            name = f'{label} {LAYER_NAMES[layer]}' + (' (judged with block 0 from the frames)' if fused_pair else '')
            try:
                r = judge(got[b:b + 1], ref[b:b + 1], yard[b:b + 1], c_max, c_rms, name, [item],
                          _TILE[layer] if layer < 8 else 16)
            except LayerMismatch as e:
                failures.append(str(e))
                r = judge(got[b:b + 1], ref[b:b + 1], yard[b:b + 1], check=False)
            key = 'fused01' if fused_pair else layer
            old = ratios.get(key, (0.0, 0.0, 0))
            ratios[key] = (max(old[0], r[0]), max(old[1], r[1]), old[2] + 1)

    for g0 in range(0, n_items, group):
        items = list(range(g0, min(g0 + group, n_items)))
        prev, prev_items = None, []                 # the GPU's output of the previous layer for prev_items
        for k in range(8):
            have = [i for i in items if i in where[k]]
            if not have:
                prev, prev_items = None, []
                continue
            got = fetch(k, have)
            if k == 0:
                x = X[have]
                record(0, got, ref_block(sd, 0, x), yard_block(sd, 0, x), have)
            elif k == 1 and not prev_items:
                x = X[have]
                record(1, got, ref_block(sd, 1, ref_block(sd, 0, x)), yard_block(sd, 1, yard_block(sd, 0, x)), have,
                       fused_pair=True)
            else:
                both = [i for i in have if i in prev_items]
                if both:
                    x = prev[[prev_items.index(i) for i in both]]
                    sel = [have.index(i) for i in both]
                    record(k, got[sel], ref_block(sd, k, x), yard_block(sd, k, x), both)
            prev, prev_items = got, have
        # the linear layers: buffers 7, 8, 9 and the grid hold the same items
        have = [i for i in items if i in where[8] and i in prev_items]
        if have:
            x = prev[[prev_items.index(i) for i in have]].reshape(len(have), -1)
            for layer, (idx, sig) in zip((8, 9), FC[:2]):
                got = fetch(layer, have)
                record(layer, got, ref_linear(sd, idx, x, sig), yard_linear(sd, idx, x, sig), have)
                x = got
            got = np.asarray(grid[have], np.float32).reshape(len(have), -1)
            record(10, got, ref_linear(sd, 5, x, False), yard_linear(sd, 5, x, False), have)
    for key in sorted(ratios, key=str):
        r = ratios[key]
        name = 'conv blocks 0+1 (fused)' if key == 'fused01' else LAYER_NAMES[key]
        log(f'LAYER-RATIO | {label} | {arith} | {"fused" if fused else "separate"} | {name} | max {r[0]:.3f} | rms {r[1]:.3f} | items {r[2]}')
    if failures:
        raise LayerMismatch(f'{len(failures)} layer/item comparisons failed:\n' + '\n'.join(failures[:12]))
    return ratios

"""Reference for the head trainer (CPU only; nothing here is taken from the kernels in csrc/train.hip).

`ref_*`: YOLO targets, the head's forward pass, YOLO_AXTrack_loss with its gradient, the backward pass and the Adam update
restated in numpy / torch f64 from f32 inputs. `yard_*`: the same step in plain torch f32 on the CPU -- the error a correct
f32 implementation makes on this very input. The judge is that of tests/cnn_reference.py: `got` passes when
    max|got-ref| <= C_max * (max|yard-ref| + 1e-6)   and   rms(got-ref) <= C_rms * (rms(yard-ref) + 1e-7).
Updated weights are judged by their UPDATE w_new - w_old: the weights themselves would hide any error behind their
own magnitude.

The semantics restated: Timelapse.py:451-548 (targets), model.py:105-117 (Linear, Sigmoid, Linear, Sigmoid, Linear),
loss.py:18-68, torch.optim.Adam(lr, weight_decay) as core_functionality.py:81 builds it (betas 0.9 / 0.999, eps 1e-8, L2
decay added to the gradient before the moments), one_epoch / run_epoch (core_functionality.py:109-165)."""
import os

import numpy as np
import torch

torch.set_num_threads(min(len(os.sched_getaffinity(0)), 16))

TS, S = 512, 12
COMPONENTS = ('total_no_object_loss', 'total_object_loss', 'total_xy_anchors_loss', 'total_summed_loss',
              'total_pos_labels_rate')
TENSORS = ('w1', 'b1', 'w2', 'b2', 'w3', 'b3')
BETAS, EPS = (0.9, 0.999), 1e-8

# ---- the bound: constants, floors and caps of tests/cnn_reference.py
CAP_MAX, CAP_RMS = 8.0, 4.0
FLOOR_MAX, FLOOR_RMS = 1e-6, 1e-7
BOUND_DEFAULT = (2.0, 1.5)
# quantity -> (C_max, C_rms) where the MI355X needs more than the default: twice the worst measured ratio, rounded up to a
# whole number (the measured table is in DESIGN.md 6.8e). Over every case of test_train_gpu.py the worst ratios were
# 1.56 (max: v of fcs.5.bias) and 1.15 (rms: m of fcs.5.bias) for the steps -- within the default -- and for the history of
# the end-to-end run 1.21 / 1.58 on total_no_object_loss: three numbers per row, each the mean of two batch losses near 20
# ... 47 that differ from the f64 ones by 1e-5, of which the f32 yardstick happens to hit two closer.
BOUND_OVERRIDES = {'history total_no_object_loss': (BOUND_DEFAULT[0], 4.0)}


def bound_for(name):
    b = BOUND_OVERRIDES.get(name, BOUND_DEFAULT)
    assert b[0] <= CAP_MAX and b[1] <= CAP_RMS, f'bound {b} for {name} exceeds the caps {(CAP_MAX, CAP_RMS)}'
    return b


class TrainMismatch(AssertionError):
    pass


def judge(got, ref, yard, name='', check=True, log=None, bound=None):
    """(max ratio, rms ratio) of got's error against the yardstick's, both against the f64 reference; raises
    TrainMismatch when a ratio exceeds the quantity's constant (`bound`: these two instead), naming the worst element."""
    got, ref, yard = (np.asarray(a, np.float64) for a in (got, ref, yard))
    assert got.shape == ref.shape == yard.shape, (name, got.shape, ref.shape, yard.shape)
    if not np.isfinite(got).all():
        raise TrainMismatch(f'{name}: non-finite values')
    eg, ey = np.abs(got - ref), np.abs(yard - ref)
    r_max = float(eg.max() / (ey.max() + FLOOR_MAX)) if eg.size else 0.0
    r_rms = float(np.sqrt(np.mean(eg ** 2)) / (np.sqrt(np.mean(ey ** 2)) + FLOOR_RMS)) if eg.size else 0.0
    if log:
        log(f'TRAIN-RATIO | {name} | max {r_max:.3f} | rms {r_rms:.3f} | yard max err {ey.max():.3g} | max |ref| {np.abs(ref).max():.3g}')
    c_max, c_rms = bound or bound_for(name.split(' @')[0])
    if check and (r_max > c_max or r_rms > c_rms):
        idx = np.unravel_index(int(np.argmax(eg)), eg.shape)
        raise TrainMismatch(f'{name}: error is {r_max:.2f}x (max; allowed {c_max}) and {r_rms:.2f}x (rms; allowed {c_rms}) that of '
                            f'plain f32 on the same input. Worst element {idx}: got {got[idx]:.9g}, f64 reference '
                            f'{ref[idx]:.9g}, f32 yardstick {yard[idx]:.9g} (yardstick max error {ey.max():.3g})')
    return r_max, r_rms


# ------------------------------------------------------------------------------------------------ targets
def ref_targets(lx, ly, cnt, tile_yx):
    """lx, ly i32 [F, cap] whole-frame anchors, cnt [F], kept tiles [(ty, tx)] -> f32 [F, n_tiles, 12, 12, 4]: dim 2 the x
    cell, dim 3 the y cell, last (1, x_in_cell, y_in_cell, label index). f32 arithmetic as the reference's; labels are
    written in list order, so that of two labels in a cell the later one wins all four channels (the reference's CPU
    index_put)."""
    F = len(cnt)
    out = np.zeros((F, len(tile_yx), S, S, 4), np.float32)
    for f in range(F):
        for k, (ty, tx) in enumerate(tile_yx):
            for l in range(int(cnt[f])):
                x, y = int(lx[f, l]), int(ly[f, l])
                if not (ty * TS <= y < (ty + 1) * TS and tx * TS <= x < (tx + 1) * TS):
                    continue
                vx = np.float32(S) * (np.float32(x - tx * TS) / np.float32(TS))
                vy = np.float32(S) * (np.float32(y - ty * TS) / np.float32(TS))
                bx, by = int(vx), int(vy)
                out[f, k, bx, by] = (1.0, vx - np.float32(bx), vy - np.float32(by), np.float32(l))
    return out


# ------------------------------------------------------------------------------------------------ one training step
def _t(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype)


def new_state(weights, dtype):
    """weights: the six f32 arrays in TENSORS order ([out, in] matrices) -> the trainer's state in `dtype`."""
    return dict(w=[_t(a, dtype).clone() for a in weights],          # (adam() works in place: never on the caller's arrays)
                 m=[torch.zeros(a.shape, dtype=dtype) for a in weights],
                v=[torch.zeros(a.shape, dtype=dtype) for a in weights], t=0, dtype=dtype)


def forward(state, X):
    w = state['w']
    a1 = torch.sigmoid(X @ w[0].T + w[1])
    a2 = torch.sigmoid(a1 @ w[2].T + w[3])
    return a1, a2, a2 @ w[4].T + w[5]


def loss(y, target, lam, fault=None):
    """loss.py:18-68 and its gradient. y [B,432], target [B,12,12,4], lam = (L_OBJECT, L_NOBJECT, L_COORD_ANCHOR) ->
    (the five components, dY [B,432])."""
    l_obj, l_noobj, l_coord = lam
    if fault == 'swap_lambda':
        l_obj, l_noobj = l_noobj, l_obj
    bs = y.shape[0]
    div = 1.0 if fault == 'no_bs' else float(bs)
    p = y.reshape(bs, S, S, 3)
    obj, txy = target[..., 0:1], target[..., 1:3]
    e_no = p[..., 0:1] * (1 - obj)
    e_obj = p[..., 0:1] * obj - obj
    e_xy = p[..., 1:3] * obj - txy
    no, ob, xy = l_noobj * (e_no ** 2).sum() / div, l_obj * (e_obj ** 2).sum() / div, l_coord * (e_xy ** 2).sum() / div
    comps = torch.stack([no, ob, xy, no + ob + xy, obj.sum() / (bs * S * S)])
    dy = torch.zeros_like(p)
    dy[..., 0:1] = (2 * l_obj * obj * e_obj + 2 * l_noobj * (1 - obj) * e_no) / div
    dy[..., 1:3] = 2 * l_coord * obj * e_xy / div
    return comps, dy.reshape(bs, -1)


def adam(p, g, m, v, t, lr, wd, fault=None, eps=EPS):
    """torch.optim.Adam's update of one tensor (L2 decay joins the gradient before the moments). p, m, v change in place."""
    b1, b2 = BETAS
    decay = lr * wd * p if fault == 'wd_after' else None
    if fault != 'wd_after':
        g = g.add(p, alpha=wd)
    m.mul_(b1).add_(g, alpha=1 - b1)
    v.mul_(b2).addcmul_(g, g, value=1 - b2)
    bc1, bc2 = (1.0, 1.0) if fault == 'no_bias_corr' else (1 - b1 ** t, 1 - b2 ** t)
    p.addcdiv_(m, v.sqrt().div_(np.sqrt(bc2)).add_(eps), value=-lr / bc1)
    if decay is not None:
        p.sub_(decay)


def step(state, X, target, lam, lr, wd, fault=None, eps=EPS):
    """Forward, loss, backward and the Adam update of all six tensors, in place in `state`. X [B,K0], target [B,12,12,4]
    in the state's dtype. Returns dict(y, comps, dy, dz2, dz1)."""
    w = state['w']
    a1, a2, y = forward(state, X)
    comps, dy = loss(y, target, lam, fault)
    state['t'] += 1
    t = state['t']

    def update(i, g):
        adam(w[i], g, state['m'][i], state['v'][i], t, lr, wd, fault, eps)

    if fault == 'post_update_dz':           # every dZ from weights that have already moved
        update(4, dy.T @ a2), update(5, dy.sum(0))
        dz2 = (dy @ w[4]) * a2 * (1 - a2)
        update(2, dz2.T @ a1), update(3, dz2.sum(0))
        dz1 = (dz2 @ w[2]) * a1 * (1 - a1)
        update(0, dz1.T @ X), update(1, dz1.sum(0))
    else:
        dz2 = (dy @ w[4]) * a2 * (1 - a2)
        dz1 = (dz2 @ w[2]) * a1 * (1 - a1)
        for i, g in ((4, dy.T @ a2), (5, dy.sum(0)), (2, dz2.T @ a1), (3, dz2.sum(0)), (0, dz1.T @ X), (1, dz1.sum(0))):
            update(i, g)
    return dict(y=y, comps=comps, dy=dy, dz2=dz2, dz1=dz1, a1=a1, a2=a2)


def gradients(state, X, target, lam):
    """The six closed-form gradients (TENSORS order) of the summed loss, without weight decay."""
    w = state['w']
    a1, a2, y = forward(state, X)
    _, dy = loss(y, target, lam)
    dz2 = (dy @ w[4]) * a2 * (1 - a2)
    dz1 = (dz2 @ w[2]) * a1 * (1 - a1)
    return [dz1.T @ X, dz1.sum(0), dz2.T @ a1, dz2.sum(0), dy.T @ a2, dy.sum(0)]


def run_steps(weights, feats, targets, batches, lam, lrs, wd, dtype, fault=None, snapshots=True, eps=EPS):
    """`len(batches)` steps from `weights` (six f32 arrays) on rows `batches[i]` of the f32 tables feats [n,K0] and targets
    [n,12,12,4] -> (state, list of step() results as numpy, list of per-step snapshots {name: array} of w, m, v)."""
    state = new_state(weights, dtype)
    Xall, Tall = _t(feats, dtype), _t(np.asarray(targets).reshape(-1, S, S, 4), dtype)
    outs, snaps = [], []
    for idx, lr in zip(batches, lrs):
        idx = torch.from_numpy(np.asarray(idx, np.int64))
        r = step(state, Xall[idx], Tall[idx], lam, lr, wd, fault, eps)
        outs.append({k: v.numpy().copy() for k, v in r.items()})
        if snapshots:
            snaps.append(dict(w=[a.numpy().copy() for a in state['w']], m=[a.numpy().copy() for a in state['m']],
                              v=[a.numpy().copy() for a in state['v']]))
    return state, outs, snaps


def ref_steps(*a, **k):
    return run_steps(*a, dtype=torch.float64, **k)


def yard_steps(*a, **k):
    return run_steps(*a, dtype=torch.float32, **k)


# ------------------------------------------------------------------------------------------------ epochs
def learning_rate(lr, decayrate, epoch):
    return lr * np.exp(-np.sqrt(epoch) / decayrate) if decayrate else lr


def epoch_schedule(n_items, epochs, batch_size, shuffle, drop_last, seed, lr, decayrate):
    """[(epoch, index batch, learning rate)] of a whole run: one default_rng(seed) permutation per epoch, batches of
    batch_size, the last smaller one kept unless drop_last (core_functionality.py:99-107, 83-87)."""
    rng = np.random.default_rng(seed)
    sched = []
    for e in range(epochs):
        order = rng.permutation(n_items) if shuffle else np.arange(n_items)
        for i in range(0, n_items, batch_size):
            b = order[i:i + batch_size]
            if drop_last and len(b) < batch_size:
                continue
            sched.append((e, b, learning_rate(lr, decayrate, e)))
    return sched


def history(sched, outs, epochs):
    """Mean of the five components over an epoch's batches -> f64 [5, epochs]."""
    h = np.zeros((5, epochs))
    for e in range(epochs):
        rows = [o['comps'] for (ee, _, _), o in zip(sched, outs) if ee == e]
        h[:, e] = np.mean(np.array(rows, np.float64), axis=0)
    return h


# ------------------------------------------------------------------------------------------------ synthetic heads
def synth_head(K0, H1, H2, seed, scale=1.0):
    """Six f32 arrays of a head K0 -> H1 -> H2 -> 432: U(-1,1) * scale / sqrt(fan_in) weights (torch's Linear init)."""
    rng = np.random.default_rng(seed)
    out = []
    for k, n in ((K0, H1), (H1, H2), (H2, S * S * 3)):
        out.append((rng.uniform(-1, 1, (n, k)) * scale / np.sqrt(k)).astype(np.float32))
        out.append((rng.uniform(-1, 1, n) * scale / np.sqrt(k)).astype(np.float32))
    return out


def synth_table(n, K0, seed, labels_per_item=3):
    """A feature table f32 [n, K0] (activation-like: half zeros, the rest |N(0,1)|) and a target table f32 [n,12,12,4] with
    `labels_per_item` occupied cells per item."""
    rng = np.random.default_rng(seed)
    feats = (np.abs(rng.normal(0, 1, (n, K0))) * (rng.random((n, K0)) < 0.5)).astype(np.float32)
    tgt = np.zeros((n, S, S, 4), np.float32)
    for i in range(n):
        for l in range(labels_per_item):
            cx, cy = rng.integers(0, S, 2)
            tgt[i, cx, cy] = (1.0, np.float32(rng.integers(0, 512)) / np.float32(512), np.float32(rng.integers(0, 512)) / np.float32(512), l)
    return feats, tgt


# ------------------------------------------------------------------------------------------------ the end-to-end case
# fine_tune_head on a 512 x 512 x (8 + 4) synthetic timelapse, one planted label per frame, shuffled batches of 5 (so the
# last batch of an epoch has 3 items and its own bs in the loss). Epoch count and learning rate are chosen so that the
# f64 REFERENCE more than halves total_summed_loss from the first epoch to the last (test_train_cpu.py checks that on
# trunk features from the CPU oracle; the GPU is not what decides it).
E2E = dict(T_all=12, H=512, W=512, frames_seed=11, weights_seed=42, epochs=3, seed=5,
           parameters=dict(BATCH_SIZE=5, LR=0.0001, SHUFFLE=True, DROP_LAST=False))


def e2e_labels():
    """Per detection frame ([x], [y]): one label that walks through the tile, one cell per frame."""
    return [([60 + 47 * t], [450 - 53 * t]) for t in range(E2E['T_all'] - 4)]


def e2e_reference(weights, feats, targets, dtype=torch.float64):
    """Replay of fine_tune_head's schedule on the f32 tables -> (history [5, epochs], final six tensors, schedule)."""
    from axtrack_amd.training import TRAIN_DEFAULTS
    P = dict(TRAIN_DEFAULTS, **E2E['parameters'])
    sched = epoch_schedule(len(feats), E2E['epochs'], P['BATCH_SIZE'], P['SHUFFLE'], P['DROP_LAST'], E2E['seed'], P['LR'],
                           P['LR_DECAYRATE'])
    lam = (P['L_OBJECT'], P['L_NOBJECT'], P['L_COORD_ANCHOR'])
    state, outs, _ = run_steps(weights, feats, targets, [b for _, b, _ in sched], lam, [lr for _, _, lr in sched],
                               P['WEIGHT_DECAY'], dtype, snapshots=False)
    return history(sched, outs, E2E['epochs']), [a.numpy() for a in state['w']], sched


def cpu_features(sd, frames):
    """Trunk features of every detection frame of a one-tile timelapse through the CPU oracle's f32 loops -> [n, 40960]."""
    import cnn_reference as cr
    from oracle import oracle as orc
    x = np.concatenate([orc.frame_tile_stack(frames, t, [(0, 0)]) for t in range(frames.shape[0] - 4)])
    for i in range(8):
        x = cr.yard_block(sd, i, x)
    return x.reshape(x.shape[0], -1)

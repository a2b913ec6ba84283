"""Reference for the conv-block trainer and the joint step with the head (CPU only; nothing here is taken from the kernels
in csrc/train_conv.hip or csrc/train.hip).

The block is the reference's CNNBlock (model.py:5-18): Conv2d 3x3 pad 1, BatchNorm2d in eval mode (running statistics,
eps 1e-5; the stated deviation from train-mode batch statistics), LeakyReLU(0.1). Its forward pass, the
closed-form gradients and the joint step are restated in torch for any dtype: f64 from f32 inputs is the reference
(`ref_*`), the same in plain f32 on the CPU the yardstick (`yard_*`). Head forward, loss and Adam are
tests/train_reference.py's. The judge is train_reference.judge.

A joint step (fine_tune_head(train_last_conv=True)): conv forward on rows of the block-input table, head forward on its
output, loss, the head's input gradient dF = dZ1 W1 from the head's weights BEFORE they move, the conv block's gradients
and Adam update, the head's gradients and Adam update; one learning rate, eps and weight decay for all ten tensors."""
import numpy as np
import torch
import torch.nn.functional as F

import train_reference as tr

BN_EPS, SLOPE = 1e-5, 0.1
CONV_TENSORS = ('conv.weight', 'conv.bias', 'batchnorm.weight', 'batchnorm.bias')
FAULTS = ('slope_side', 'no_fold', 'swap_k', 'wrap', 'no_bn_wd', 'post_update_df')


def _t(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype)


# ------------------------------------------------------------------------------------------------ the block
def block_forward(w, stats, x, fault=None):
    """w = [conv.weight, conv.bias, gamma, beta], stats = (running_mean, running_var), x [B,Ci,H,W] ->
    dict(z, zhat, y, F [B,Co,H,W], inv_sigma)."""
    ch = (None, slice(None), None, None)
    if fault == 'wrap':
        z = F.conv2d(F.pad(x, (1, 1, 1, 1), mode='circular'), w[0], w[1])
    else:
        z = F.conv2d(x, w[0], w[1], padding=1)
    inv = 1.0 / torch.sqrt(stats[1] + BN_EPS)
    zhat = (z - stats[0][ch]) * inv[ch]
    y = w[2][ch] * zhat + w[3][ch]
    return dict(z=z, zhat=zhat, y=y, F=torch.where(y > 0, y, SLOPE * y), inv_sigma=inv)


def block_gradients(w, x, fwd, dF, fault=None):
    """Closed-form gradients of the four tensors (CONV_TENSORS order, no weight decay) from dF [B,Co,H,W]."""
    ch = (None, slice(None), None, None)
    y, zhat = fwd['y'], fwd['zhat']
    pos = (y >= 0) if fault == 'slope_side' else (y > 0)            # y == 0 takes the slope, as torch's leaky_relu does
    dy = dF * torch.where(pos, torch.ones_like(y), torch.full_like(y, SLOPE))
    dgamma, dbeta = (dy * zhat).sum((0, 2, 3)), dy.sum((0, 2, 3))
    dz = dy if fault == 'no_fold' else dy * (w[2] * fwd['inv_sigma'])[ch]
    dbias = dz.sum((0, 2, 3))
    H, W = x.shape[2:]
    xp = F.pad(x, (1, 1, 1, 1), mode='circular') if fault == 'wrap' else F.pad(x, (1, 1, 1, 1))
    dW = torch.zeros_like(w[0])
    for ky in range(3):
        for kx in range(3):
            g = torch.einsum('bohw,bihw->oi', dz, xp[:, :, ky:ky + H, kx:kx + W])
            if fault == 'swap_k':
                dW[:, :, kx, ky] = g
            else:
                dW[:, :, ky, kx] = g
    return [dW, dbias, dgamma, dbeta]


# ------------------------------------------------------------------------------------------------ the joint step
def new_state(conv, head, dtype, start=None):
    """conv: six f32 arrays (conv.weight, conv.bias, gamma, beta, running_mean, running_var); head: the six of
    train_reference.TENSORS. start = (snapshot, t): instead of fresh tensors and zero moments, the ten tensors with their
    m and v as a snapshot() holds them (f32 arrays), after t steps."""
    cw = [_t(a, dtype).clone() for a in conv[:4]]
    state = dict(cw=cw, cm=[torch.zeros_like(a) for a in cw], cv=[torch.zeros_like(a) for a in cw],
                 stats=(_t(conv[4], dtype), _t(conv[5], dtype)), head=tr.new_state(head, dtype), t=0, dtype=dtype)
    if start is not None:
        snap, t = start
        for k in ('cw', 'cm', 'cv'):
            state[k] = [_t(a, dtype).clone() for a in snap[k]]
        for k in ('w', 'm', 'v'):
            state['head'][k] = [_t(a, dtype).clone() for a in snap[k]]
        state['t'] = state['head']['t'] = int(t)
    return state


def joint_step(state, x, target, lam, lr, wd, fault=None, eps=tr.EPS):
    """x [B,Ci,H,W], target [B,12,12,4] in the state's dtype; every tensor of `state` moves in place.
    Returns dict(F [B, Co*H*W], y, comps, dy, dfeat)."""
    head = state['head']
    hw = head['w']
    B = x.shape[0]
    fwd = block_forward(state['cw'], state['stats'], x, fault)
    feats = fwd['F'].reshape(B, -1)
    a1, a2, y = tr.forward(head, feats)
    comps, dy = tr.loss(y, target, lam)
    state['t'] += 1
    head['t'] += 1
    t = state['t']
    dz2 = (dy @ hw[4]) * a2 * (1 - a2)
    dz1 = (dz2 @ hw[2]) * a1 * (1 - a1)
    head_grads = ((4, dy.T @ a2), (5, dy.sum(0)), (2, dz2.T @ a1), (3, dz2.sum(0)), (0, dz1.T @ feats), (1, dz1.sum(0)))

    def update_head():
        for i, g in head_grads:
            tr.adam(hw[i], g, head['m'][i], head['v'][i], t, lr, wd, None, eps)

    if fault == 'post_update_df':           # the input gradient from a first layer that has already moved
        update_head()
    dfeat = dz1 @ hw[0]
    grads = block_gradients(state['cw'], x, fwd, dfeat.reshape(fwd['F'].shape), fault)
    for i, g in enumerate(grads):
        tr.adam(state['cw'][i], g, state['cm'][i], state['cv'][i], t, lr, 0.0 if fault == 'no_bn_wd' and i >= 2 else wd,
                None, eps)
    if fault != 'post_update_df':
        update_head()
    return dict(F=feats, y=y, comps=comps, dy=dy, dfeat=dfeat)


def snapshot(state):
    c = lambda L: [a.numpy().copy() for a in L]
    return dict(cw=c(state['cw']), cm=c(state['cm']), cv=c(state['cv']), w=c(state['head']['w']), m=c(state['head']['m']),
                v=c(state['head']['v']))


def run_steps(conv, head, shape, table, targets, batches, lam, lrs, wd, dtype, fault=None, eps=tr.EPS, start=None):
    """`len(batches)` joint steps on rows batches[i] of the f32 tables table [n, Ci*H*W] and targets [n,12,12,4];
    shape = (Ci, H, W) -> (state, list of joint_step results as numpy, list of per-step snapshots). start: new_state's."""
    state = new_state(conv, head, dtype, start)
    X = _t(table, dtype).reshape(len(table), *shape)
    T = _t(np.asarray(targets).reshape(-1, tr.S, tr.S, 4), dtype)
    outs, snaps = [], []
    for idx, lr in zip(batches, lrs):
        idx = torch.from_numpy(np.asarray(idx, np.int64))
        r = joint_step(state, X[idx], T[idx], lam, lr, wd, fault, eps)
        outs.append({k: v.numpy().copy() for k, v in r.items()})
        snaps.append(snapshot(state))
    return state, outs, snaps


def ref_steps(*a, **k):
    return run_steps(*a, dtype=torch.float64, **k)


def yard_steps(*a, **k):
    return run_steps(*a, dtype=torch.float32, **k)


JUDGED = [('cw', 'cm', 'cv', CONV_TENSORS), ('w', 'm', 'v', tr.TENSORS)]
# quantity -> (C_max, C_rms) where the MI355X needs more than train_reference.BOUND_DEFAULT: twice the worst measured
# ratio, rounded up to a whole number and limited by the caps, which every seeded fault of test_train_conv_cpu.py exceeds
# (the measured table is in DESIGN.md 6.8e). Every step is judged on its own (judge_restarted). Every quantity of the new
# kernels stayed within the default (F 0.82 / 0.54, dfeat 0.78 / 0.78, conv.weight's update, m, v 0.83 / 0.72) except the per-channel tensors named
# here: 8 numbers (3 in the one-row case), each one sum over the batch of gradients that carry the roundings of the whole
# chain before them, against a yardstick whose own error on them is a third of an ulp. `v b3` is the head's: at B = 1
# it is 0.001 dY^2, twice the relative error of one grid value.
BOUND_OVERRIDES = {'v conv.bias': (2.0, 4.0),                       # measured 1.45 / 1.76
                   'm batchnorm.weight': (2.0, 4.0),                # 0.74 / 1.94 (the one-row case, step 3)
                   'm batchnorm.bias': (2.0, 4.0),                  # 0.72 / 2.01
                   'v batchnorm.bias': (2.0, 4.0),                  # 0.78 / 2.11
                   'v b3': (7.0, 4.0),                              # 3.34 / 2.66
                   'history total_object_loss': (4.0, 4.0),         # 1.96 / 2.23: three numbers, as train_reference's exception
                   'history total_xy_anchors_loss': (4.0, 4.0)}     # 1.65 / 1.71


def bound_for(name):
    b = BOUND_OVERRIDES.get(name) or tr.bound_for(name)
    assert b[0] <= tr.CAP_MAX and b[1] <= tr.CAP_RMS, f'bound {b} for {name} exceeds the caps {(tr.CAP_MAX, tr.CAP_RMS)}'
    return b


def judge_run(outs, snaps, ref, yard, conv0, head0, steps, label='', bound=None, log=None, collect=None, number=None):
    """What the tests assert of a run of joint steps: F, dfeat, and update, m, v of the four conv tensors and the six head
    tensors at the listed steps, each under train_reference.judge. The references are whole runs from the same start, so at
    a later step they have parted from `got` by what the steps before did to the weights: see judge_restarted. collect: a
    list that receives the failures' texts instead of the first one being raised. number: the step's number in the labels."""
    (_, r_outs, r_snaps), (_, y_outs, y_snaps) = ref, yard
    start = dict(cw=conv0[:4], w=head0)

    def one(got, r, y, name):
        try:
            tr.judge(got, r, y, f'{name} @{label} step {number or s + 1}', log=log, bound=bound or bound_for(name))
        except tr.TrainMismatch as e:
            if collect is None:
                raise
            collect.append(str(e))

    for s in steps:
        for q in ('F', 'dfeat'):
            one(outs[s][q], r_outs[s][q], y_outs[s][q], q)
        for kw, km, kv, names in JUDGED:
            for i, name in enumerate(names):
                w0 = np.asarray(start[kw][i], np.float64)
                one(snaps[s][kw][i] - w0, r_snaps[s][kw][i] - w0, y_snaps[s][kw][i] - w0, f'update {name}')
                one(snaps[s][km][i], r_snaps[s][km][i], y_snaps[s][km][i], f'm {name}')
                one(snaps[s][kv][i], r_snaps[s][kv][i], y_snaps[s][kv][i], f'v {name}')


def judge_restarted(outs, snaps, args, steps, label='', eps=tr.EPS, bound=None, log=None, collect=None):
    """judge_run without the chaining: step s of the run under test (outs, snaps: per step, from the start of `args`) is
    judged against ONE step of the f64 reference and of the f32 yardstick, both restarted from the ten tensors, moments
    and step count that the run under test itself held after step s - 1 (its snapshot; the given start for s = 0). Every
    judged quantity is then the arithmetic of one step on identical inputs, as tests/cnn_reference.py feeds every layer
    the GPU's own input; updates are taken from the restart's weights. args: run_steps' positional arguments up to wd."""
    conv, head, shape, table, targets, batches, lam, lrs, wd = args
    for s in steps:
        start = None if s == 0 else (snaps[s - 1], s)
        one = (conv, head, shape, table, targets, [batches[s]], lam, [lrs[s]], wd)
        ref, yard = ref_steps(*one, eps=eps, start=start), yard_steps(*one, eps=eps, start=start)
        conv0, head0 = (conv, head) if s == 0 else (snaps[s - 1]['cw'], snaps[s - 1]['w'])
        judge_run([outs[s]], [snaps[s]], ref, yard, conv0, head0, (0,), label, bound, log, collect, number=s + 1)


# ------------------------------------------------------------------------------------------------ synthetic cases
def synth_block(Ci, Co, seed, scale=1.0):
    """Six f32 arrays of a block: U(-1,1) * scale / sqrt(9 Ci) weights and bias (torch's Conv2d init), gamma of both signs
    in 0.5 ... 1.5, beta and mean N(0, 0.2), var in 0.5 ... 1.5."""
    rng = np.random.default_rng(seed)
    k = scale / np.sqrt(9 * Ci)
    gamma = rng.uniform(0.5, 1.5, Co) * np.where(np.arange(Co) % 3 == 1, -1.0, 1.0)
    return [a.astype(np.float32) for a in (rng.uniform(-1, 1, (Co, Ci, 3, 3)) * k, rng.uniform(-1, 1, Co) * k, gamma,
                                           rng.normal(0, 0.2, Co), rng.normal(0, 0.2, Co), rng.uniform(0.5, 1.5, Co))]


def synth_inputs(n, Ci, H, W, seed, labels_per_item=3):
    """A block-input table f32 [n, Ci*H*W] (activation-like: a third zeros, the rest N(0,1) leaky-rectified) and a target
    table f32 [n,12,12,4]."""
    rng = np.random.default_rng(seed)
    x = rng.normal(0, 1, (n, Ci * H * W))
    x = np.where(x > 0, x, SLOPE * x) * (rng.random(x.shape) < 0.67)
    _, tgt = tr.synth_table(n, 1, seed + 1, labels_per_item)
    return x.astype(np.float32), tgt


def border_ring(table, Ci, H, W):
    """The table with everything but the outermost ring of each map set to zero: only padding-adjacent data is left."""
    x = table.reshape(len(table), Ci, H, W).copy()
    x[:, :, 1:H - 1, 1:W - 1] = 0
    return x.reshape(len(table), -1)


def y_zero_block(conv):
    """The block with output channel 0 pinned to y == 0 everywhere: zero weights, bias == running_mean (so z - mean is
    exactly 0) and beta 0. LeakyReLU's derivative at 0 is its slope: the channel's dgamma, dbeta and dbias are a tenth of
    what an implementation that gives y == 0 slope 1 computes."""
    conv = [a.copy() for a in conv]
    conv[0][0] = 0
    conv[1][0] = conv[4][0]
    conv[3][0] = 0
    return conv

"""Reference for train-mode BatchNorm (batch statistics) in the trained conv blocks (CPU only; nothing here is taken from the
kernels in csrc/train_conv.hip), on top of tests/train_conv_reference.py, tests/train_stage_reference.py and
tests/train_reference.py, whose head, loss, Adam, pool, judge and restarted-judging scheme it uses as they are.

Restated in torch for any dtype (f64 from f32 inputs is the reference, plain f32 on the CPU the yardstick), per channel over
the n = B*H*W values of z = conv(x) + bias:
    mu = sum z / n,  var = sum (z - mu)^2 / n (two passes, biased),  zhat = (z - mu) / sqrt(var + 1e-5),
    y = gamma zhat + beta,  F = leaky(y),
    running_mean <- (1 - m) running_mean + m mu,  running_var <- (1 - m) running_var + m var n / (n - 1),  count += 1
(all three in the forward pass, once per forward), and from dF
    dy = dF (y > 0 ? 1 : 0.1),  dbeta = sum dy,  dgamma = sum dy zhat,  dz = gamma inv (dy - dbeta / n - zhat dgamma / n),
dW and dx from this dz, and dbias = 0 BY DEFINITION: sum dz vanishes identically, autograd's value is rounding noise
(test_train_bn_cpu.py measures it), and Adam would turn that noise into steps of order lr.

LeakyReLU's side is discrete: a y that f32 puts on the other side of 0 than f64 turns a rounding into a factor of 10. Every
case's seed is therefore one for which the f64 reference has no element with 0 < |y| < SIDE_MARGIN (|gamma zhat| + |beta|)
at any judged step (`near_zero` counts them; test_train_bn_cpu.py asserts 0 for every case, and the GPU judge asserts it of
the restarted reference). No element is ever excluded. y == 0 exactly (the constant channel) takes the slope on both sides."""
import numpy as np
import torch
import torch.nn.functional as F

import train_conv_reference as cr
import train_reference as tr
import train_stage_reference as sr

BN_EPS, SLOPE, MOMENTUM = cr.BN_EPS, cr.SLOPE, 0.1
SIDE_MARGIN = 16 * 2.0 ** -23
FAULTS = ('rv_biased', 'fwd_unbiased', 'momentum_swapped', 'dz_eval', 'dgamma_no_n', 'one_pass', 'stats_in_step')
CH = (None, slice(None), None, None)
_t = cr._t


# ------------------------------------------------------------------------------------------------ one block
def bn_forward(w, stats, x, momentum=MOMENTUM, fault=None):
    """w = [conv.weight, conv.bias, gamma, beta], stats = (running_mean, running_var), x [B,Ci,H,W] -> dict(z, zhat, y, F,
    inv_sigma, mu, var, n, stats: the moved running statistics, near_zero: elements that break the side condition)."""
    z = F.conv2d(x, w[0], w[1], padding=1)
    n = z.numel() // z.shape[1]
    if n < 2:
        raise ValueError(f'batch statistics need more than {n} value per channel')
    if fault == 'one_pass':
        mu = z.sum((0, 2, 3)) / n
        var = (z * z).sum((0, 2, 3)) / n - mu * mu
    else:
        mu = z.sum((0, 2, 3)) / n
        var = ((z - mu[CH]) ** 2).sum((0, 2, 3)) / n
    unbiased = var * (n / (n - 1))
    inv = 1.0 / torch.sqrt((unbiased if fault == 'fwd_unbiased' else var) + BN_EPS)
    zhat = (z - mu[CH]) * inv[CH]
    y = w[2][CH] * zhat + w[3][CH]
    a, b = (momentum, 1 - momentum) if fault == 'momentum_swapped' else (1 - momentum, momentum)
    moved = (a * stats[0] + b * mu, a * stats[1] + b * (var if fault == 'rv_biased' else unbiased))
    near = (y.abs() < SIDE_MARGIN * ((w[2][CH] * zhat).abs() + w[3][CH].abs())) & (y != 0)
    return dict(z=z, zhat=zhat, y=y, F=torch.where(y > 0, y, SLOPE * y), inv_sigma=inv, mu=mu, var=var, n=n, stats=moved,
                near_zero=int(near.sum()))


def bn_gradients(w, x, fwd, dF, fault=None):
    """-> ([dW, dbias = 0, dgamma, dbeta] (train_conv_reference.CONV_TENSORS order, no weight decay), dz)."""
    y, zhat, n = fwd['y'], fwd['zhat'], fwd['n']
    dy = dF * torch.where(y > 0, torch.ones_like(y), torch.full_like(y, SLOPE))
    dgamma, dbeta = (dy * zhat).sum((0, 2, 3)), dy.sum((0, 2, 3))
    fold = (w[2] * fwd['inv_sigma'])[CH]
    if fault == 'dz_eval':
        dz = dy * fold
    else:
        dz = fold * (dy - (dbeta / n)[CH] - zhat * (dgamma if fault == 'dgamma_no_n' else dgamma / n)[CH])
    H, W = x.shape[2:]
    xp = F.pad(x, (1, 1, 1, 1))
    dW = torch.zeros_like(w[0])
    for ky in range(3):
        for kx in range(3):
            dW[:, :, ky, kx] = torch.einsum('bohw,bihw->oi', dz, xp[:, :, ky:ky + H, kx:kx + W])
    return [dW, torch.zeros_like(w[1]), dgamma, dbeta], dz


def bn_input_grad(w, dz):
    """dx[b,ci,h,w] = sum dz[b,co,h-ky+1,w-kx+1] weight[co,ci,ky,kx]: train_stage_reference.block_input_grad's product, fed
    the finished dz (unit gamma and inv_sigma, no slope)."""
    one = torch.ones(dz.shape[1], dtype=dz.dtype)
    return sr.block_input_grad([w[0], None, one, None], dict(y=dz, inv_sigma=one), dz, fault='no_slope')


def forward_commit(blk, x, momentum=MOMENTUM, fault=None):
    """bn_forward on a block of a state (dict(cw, stats, nbt, ...)); the running statistics and the count move here, as
    nn.BatchNorm2d moves them (stats_in_step: only when backward_commit runs)."""
    fwd = bn_forward(blk['cw'], blk['stats'], x, momentum, fault)
    if fault == 'stats_in_step':
        blk['pending'] = fwd['stats']
    else:
        blk['stats'], blk['nbt'] = fwd['stats'], blk['nbt'] + 1
    return fwd


def backward_commit(blk, x, fwd, dF, t, lr, wd, eps, fault=None, need_dx=True):
    """Gradients from the parameters as they stand, the input gradient, then Adam on the four tensors -> dx or None."""
    grads, dz = bn_gradients(blk['cw'], x, fwd, dF, fault)
    dx = bn_input_grad(blk['cw'], dz) if need_dx else None
    for i, g in enumerate(grads):
        tr.adam(blk['cw'][i], g, blk['cm'][i], blk['cv'][i], t, lr, wd, None, eps)
    if 'pending' in blk:
        blk['stats'], blk['nbt'] = blk.pop('pending'), blk['nbt'] + 1
    return dx


def _head_backward(head, feats, target, lam):
    hw = head['w']
    a1, a2, y = tr.forward(head, feats)
    comps, dy = tr.loss(y, target, lam)
    dz2 = (dy @ hw[4]) * a2 * (1 - a2)
    dz1 = (dz2 @ hw[2]) * a1 * (1 - a1)
    grads = ((4, dy.T @ a2), (5, dy.sum(0)), (2, dz2.T @ a1), (3, dz2.sum(0)), (0, dz1.T @ feats), (1, dz1.sum(0)))
    return dict(y=y, comps=comps, dy=dy, dfeat=dz1 @ hw[0]), grads


def _head_update(head, grads, t, lr, wd, eps):
    for i, g in grads:
        tr.adam(head['w'][i], g, head['m'][i], head['v'][i], t, lr, wd, None, eps)


# ------------------------------------------------------------------------------------------------ one block with the head
def new_state(conv, head, dtype, start=None):
    """train_conv_reference.new_state plus the batch count; start = (snapshot, t) also restores the running statistics and
    the count the snapshot holds."""
    state = cr.new_state(conv, head, dtype, start)
    state['nbt'] = 0
    if start is not None:
        state['stats'] = tuple(_t(a, dtype).clone() for a in start[0]['stats'])
        state['nbt'] = int(start[0]['nbt'])
    return state


def joint_step(state, x, target, lam, lr, wd, momentum=MOMENTUM, fault=None, eps=tr.EPS):
    """train_conv_reference.joint_step in batch mode. Returns dict(F, y, comps, dy, dfeat, dx, mu, var, near_zero)."""
    B = x.shape[0]
    fwd = forward_commit(state, x, momentum, fault)
    feats = fwd['F'].reshape(B, -1)
    out, head_grads = _head_backward(state['head'], feats, target, lam)
    state['t'] += 1
    state['head']['t'] += 1
    dx = backward_commit(state, x, fwd, out['dfeat'].reshape(fwd['F'].shape), state['t'], lr, wd, eps, fault)
    _head_update(state['head'], head_grads, state['t'], lr, wd, eps)
    out.update(F=feats, dx=dx.reshape(B, -1), mu=fwd['mu'], var=fwd['var'], near_zero=torch.tensor(fwd['near_zero']))
    return out


def snapshot(state):
    snap = cr.snapshot(state)
    snap.update(stats=[a.numpy().copy() for a in state['stats']], nbt=int(state['nbt']))
    return snap


def run_steps(conv, head, shape, table, targets, batches, lam, lrs, wd, dtype, momentum=MOMENTUM, fault=None, eps=tr.EPS,
              start=None):
    """train_conv_reference.run_steps in batch mode -> (state, per-step results as numpy, per-step snapshots)."""
    state = new_state(conv, head, dtype, start)
    X = _t(table, dtype).reshape(len(table), *shape)
    T = _t(np.asarray(targets).reshape(-1, tr.S, tr.S, 4), dtype)
    outs, snaps = [], []
    for idx, lr in zip(batches, lrs):
        idx = torch.from_numpy(np.asarray(idx, np.int64))
        r = joint_step(state, X[idx], T[idx], lam, lr, wd, momentum, fault, eps)
        outs.append({k: v.numpy().copy() for k, v in r.items()})
        snaps.append(snapshot(state))
    return state, outs, snaps


def ref_steps(*a, **k):
    return run_steps(*a, dtype=torch.float64, **k)


def yard_steps(*a, **k):
    return run_steps(*a, dtype=torch.float32, **k)


# ------------------------------------------------------------------------------------------------ the stage
def new_stage_state(convs, head, dtype, start=None):
    state = sr.new_state(convs, head, dtype, start)
    for name in sr.BLOCKS:
        state[name]['nbt'] = 0
        if start is not None:
            state[name]['stats'] = tuple(_t(a, dtype).clone() for a in start[0][name]['stats'])
            state[name]['nbt'] = int(start[0][name]['nbt'])
    return state


def stage_step(state, x, target, lam, lr, wd, depth=3, momentum=MOMENTUM, eps=tr.EPS, winners=None):
    """train_stage_reference.stage_step with batch statistics in the trained blocks; a forward-only block (b5 at depth 2)
    keeps train_conv_reference.block_forward and its running statistics. Returns stage_step's keys plus per trained block
    `mu <name>`, `var <name>`, and near_zero."""
    B = x.shape[0]
    trained = {n: i >= 3 - depth for i, n in enumerate(sr.BLOCKS)}

    def fw(name, inp):
        blk = state[name]
        return forward_commit(blk, inp, momentum) if trained[name] else cr.block_forward(blk['cw'], blk['stats'], inp)

    f5 = fw('b5', x)
    f6 = fw('b6', f5['F'])
    win = sr.pool_winners(f6['F']) if winners is None else winners
    pooled = sr.pool_forward(f6['F'], win)
    f7 = fw('b7', pooled)
    feats = f7['F'].reshape(B, -1)
    out, head_grads = _head_backward(state['head'], feats, target, lam)
    state['t'] += 1
    state['head']['t'] += 1
    t = state['t']
    out.update(F5=f5['F'].reshape(B, -1), F6=f6['F'].reshape(B, -1), pooled=pooled.reshape(B, -1), F=feats)
    dpooled = backward_commit(state['b7'], pooled, f7, out['dfeat'].reshape(f7['F'].shape), t, lr, wd, eps, need_dx=depth >= 2)
    if depth >= 2:
        dF6 = sr.pool_backward(f6['F'], dpooled, win)
        out.update(dpooled=dpooled.reshape(B, -1), dF6=dF6.reshape(B, -1))
        dx6 = backward_commit(state['b6'], f5['F'], f6, dF6, t, lr, wd, eps, need_dx=depth >= 3)
        if depth >= 3:
            out['dx6'] = dx6.reshape(B, -1)
            backward_commit(state['b5'], x, f5, dx6, t, lr, wd, eps, need_dx=False)
    _head_update(state['head'], head_grads, t, lr, wd, eps)
    near = 0
    for name, fwd in zip(sr.BLOCKS, (f5, f6, f7)):
        if trained[name]:
            out[f'mu {name}'], out[f'var {name}'] = fwd['mu'], fwd['var']
            near += fwd['near_zero']
    out['near_zero'] = torch.tensor(near)
    return out


def stage_snapshot(state):
    snap = sr.snapshot(state)
    for name in sr.BLOCKS:
        snap[name].update(stats=[a.numpy().copy() for a in state[name]['stats']], nbt=int(state[name]['nbt']))
    return snap


def run_stage_steps(convs, head, shape, table, targets, batches, lam, lrs, wd, dtype, depth=3, momentum=MOMENTUM, eps=tr.EPS,
                    start=None, winners=None):
    state = new_stage_state(convs, head, dtype, start)
    X = _t(table, dtype).reshape(len(table), *shape)
    T = _t(np.asarray(targets).reshape(-1, tr.S, tr.S, 4), dtype)
    outs, snaps = [], []
    for s, (idx, lr) in enumerate(zip(batches, lrs)):
        idx = torch.from_numpy(np.asarray(idx, np.int64))
        r = stage_step(state, X[idx], T[idx], lam, lr, wd, depth, momentum, eps, None if winners is None else winners[s])
        outs.append({k: v.numpy().copy() for k, v in r.items()})
        snaps.append(stage_snapshot(state))
    return state, outs, snaps


# ------------------------------------------------------------------------------------------------ the judge
# quantity -> (C_max, C_rms) where the MI355X needs more than train_reference.BOUND_DEFAULT (2.0 / 1.5), by the project's rule:
# twice the worst measured ratio, rounded up to a whole number, never above the caps 8 / 4, which every seeded fault of
# test_train_bn_cpu.py exceeds. Measured over every case of test_train_bn_gpu.py, each step judged on its own against the f64
# reference (the table is in DESIGN.md 6.8e). The head's six tensors run through the kernels they ran through before and keep
# the overrides train_conv_reference / train_stage_reference measured for them where none is named here.
# Every quantity stayed within the default at every case of 8 or more channels (F 0.81 / 0.79, batch mean 0.50 / 0.62, batch
# var 0.62 / 0.86, running_var 0.58 / 0.70, update conv.weight 0.93 / 0.67, update conv.bias 0.78 / 0.97). Beyond it, all on
# rms, all but the last in the two cases of 3 channels and one item (one row, n = 6; n = 2), where a per-channel tensor is 3
# numbers and dfeat and dx are 6 to 18, each carrying the roundings of the whole chain before it:
BOUND_OVERRIDES = {'dfeat': (4.0, 4.0),                             # measured 1.99 / 1.65 (one row, step 3)
                   'dx': (4.0, 4.0),                                # 1.73 / 1.77 (one row, step 3)
                   'm batchnorm.weight': (2.0, 4.0),                # 0.94 / 1.56 (one row)
                   'v batchnorm.weight': (2.0, 4.0),                # 0.84 / 1.84 (one row)
                   'm batchnorm.bias': (2.0, 4.0),                  # 0.97 / 2.14 (one row): twice that is beyond the cap
                   'v w2': (3.0, 4.0),                              # 1.48 / 1.64 (n = 2)
                   'v b2': (4.0, 4.0),                              # 1.89 / 1.63 (n = 2)
                   # the offset case: z near 100, so a sum of 75 of them rounds at 5e-4 and mu at 7e-6, in any order of summation
                   'running_mean': (3.0, 4.0),                      # 1.18 / 2.20: twice that is beyond the cap
                   # the deployed stage at B = 2: 160 updates of 0.002 at lr 0.01, gradients near Adam's eps, where the update
                   # is steepest in the gradient
                   'update b7 batchnorm.weight': (4.0, 4.0)}                # 1.81 / 1.59


def bound_for(name):
    if name not in BOUND_OVERRIDES and name.split(' ')[-1] in tr.TENSORS:
        return sr.bound_for(name)
    b = BOUND_OVERRIDES.get(name) or tr.BOUND_DEFAULT
    assert b[0] <= tr.CAP_MAX and b[1] <= tr.CAP_RMS, f'bound {b} for {name} exceeds the caps {(tr.CAP_MAX, tr.CAP_RMS)}'
    return b


def _one(got, r, y, name, label, s, log, collect, bound=None):
    try:
        tr.judge(got, r, y, f'{name} @{label} step {s + 1}', log=log, bound=bound or bound_for(name))
    except tr.TrainMismatch as e:
        if collect is None:
            raise
        collect.append(str(e))


def _judge_block_state(got, r, y, before, prefix, label, s, log, collect, bound):
    """update, m, v of a block's four tensors, its running statistics by their update, and the count (exact)."""
    for i, name in enumerate(cr.CONV_TENSORS):
        w0 = np.asarray(before['cw'][i], np.float64)
        _one(got['cw'][i] - w0, r['cw'][i] - w0, y['cw'][i] - w0, f'update {prefix}{name}', label, s, log, collect, bound)
        _one(got['cm'][i], r['cm'][i], y['cm'][i], f'm {prefix}{name}', label, s, log, collect, bound)
        _one(got['cv'][i], r['cv'][i], y['cv'][i], f'v {prefix}{name}', label, s, log, collect, bound)
    for i, name in enumerate(('running_mean', 'running_var')):
        s0 = np.asarray(before['stats'][i], np.float64)
        _one(got['stats'][i] - s0, r['stats'][i] - s0, y['stats'][i] - s0, f'{prefix}{name}', label, s, log, collect, bound)
    if not got['nbt'] == r['nbt'] == y['nbt'] == before['nbt'] + 1:
        msg = f'{prefix}num_batches_tracked @{label} step {s + 1}: got {got["nbt"]}, reference {r["nbt"]}'
        if collect is None:
            raise tr.TrainMismatch(msg)
        collect.append(msg)


def _judge_head(got, r, y, head0, label, s, log, collect, bound):
    for i, name in enumerate(tr.TENSORS):
        w0 = np.asarray(head0[i], np.float64)
        _one(got['w'][i] - w0, r['w'][i] - w0, y['w'][i] - w0, f'update {name}', label, s, log, collect, bound)
        _one(got['m'][i], r['m'][i], y['m'][i], f'm {name}', label, s, log, collect, bound)
        _one(got['v'][i], r['v'][i], y['v'][i], f'v {name}', label, s, log, collect, bound)


def _side_condition(r, label, s, collect):
    if int(r['near_zero']):
        msg = f'side condition @{label} step {s + 1}: {int(r["near_zero"])} elements of the f64 reference lie within the margin of 0'
        if collect is None:
            raise tr.TrainMismatch(msg)
        collect.append(msg)


def judge_restarted(outs, snaps, args, steps, label='', momentum=MOMENTUM, eps=tr.EPS, bound=None, log=None, collect=None):
    """train_conv_reference.judge_restarted's scheme in batch mode: step s of the run under test against ONE step of the f64
    reference and of the f32 yardstick, both restarted from the tensors, moments, step count, running statistics and batch
    count that the run under test held after step s - 1. outs: per step dict(F, dfeat, dx, mu, var); snaps: snapshot()s."""
    conv, head, shape, table, targets, batches, lam, lrs, wd = args
    for s in steps:
        start = None if s == 0 else (snaps[s - 1], s)
        one = (conv, head, shape, table, targets, [batches[s]], lam, [lrs[s]], wd)
        (_, (r,), (rs,)), (_, (y,), (ys,)) = (run_steps(*one, dtype=d, momentum=momentum, eps=eps, start=start)
                                              for d in (torch.float64, torch.float32))
        _side_condition(r, label, s, collect)
        for q, name in (('F', 'F'), ('dfeat', 'dfeat'), ('dx', 'dx'), ('mu', 'batch mean'), ('var', 'batch var')):
            _one(outs[s][q], r[q], y[q], name, label, s, log, collect, bound)
        before = dict(cw=conv[:4], stats=conv[4:6], nbt=0, w=head) if s == 0 else snaps[s - 1]
        _judge_block_state(snaps[s], rs, ys, before, '', label, s, log, collect, bound)
        _judge_head(snaps[s], rs, ys, before['w'], label, s, log, collect, bound)


STAGE_QUANTITIES = sr.QUANTITIES


def judge_stage_restarted(outs, snaps, args, steps, depth=3, label='', momentum=MOMENTUM, eps=tr.EPS, bound=None, log=None,
                          collect=None):
    """train_stage_reference.judge_restarted's scheme in batch mode, the pool's winners taken from the F6 of the run under
    test. outs: per step stage_step's keys (`mu <name>`, `var <name>` per trained block); snaps: stage_snapshot()s."""
    convs, head, shape, table, targets, batches, lam, lrs, wd = args
    Ci, H, W = shape
    trained = sr.BLOCKS[3 - depth:]
    C6 = np.asarray(convs[1][0]).shape[0]
    for s in steps:
        start = None if s == 0 else (snaps[s - 1], s)
        B = len(batches[s])
        win = [sr.pool_winners(torch.from_numpy(outs[s]['F6']).reshape(B, C6, H, W))]
        a = (convs, head, shape, table, targets, [batches[s]], lam, [lrs[s]], wd)
        (_, (r,), (rs,)), (_, (y,), (ys,)) = (run_stage_steps(*a, dtype=d, depth=depth, momentum=momentum, eps=eps, start=start,
                                                              winners=win) for d in (torch.float64, torch.float32))
        _side_condition(r, label, s, collect)
        for q in STAGE_QUANTITIES:
            if q in outs[s]:
                _one(outs[s][q], r[q], y[q], q, label, s, log, collect, bound)
        for n in trained:
            for q, name in ((f'mu {n}', f'{n} batch mean'), (f'var {n}', f'{n} batch var')):
                _one(outs[s][q], r[q], y[q], name, label, s, log, collect, bound)
            before = dict(cw=convs[sr.BLOCKS.index(n)][:4], stats=convs[sr.BLOCKS.index(n)][4:6], nbt=0) if s == 0 else snaps[s - 1][n]
            _judge_block_state(snaps[s][n], rs[n], ys[n], before, f'{n} ', label, s, log, collect, bound)
        _judge_head(snaps[s], rs, ys, head if s == 0 else snaps[s - 1]['w'], label, s, log, collect, bound)


# ------------------------------------------------------------------------------------------------ the cases of both test files
LAM = (49.5, 1.0, 49.5)
LR, WD = 1e-2, 0.05                 # as tests/test_train_conv_gpu.py: an update is far above the judge's absolute floors
EPS = 1e-3                          # Adam's eps in the judged steps, for the reason test_train_gpu.py gives

# name -> (Ci, Co, H, W), (H1, H2), B, steps, judged steps, seed, kind. n = B*H*W per channel. The seeds are the first from
# each case's base for which the f64 reference meets the side condition at every step (module docstring).
BLOCK_CASES = {}
for _dims, _head, _base in (((3, 8, 5, 5), (72, 40), 3008), ((5, 41, 10, 10), (130, 68), 5041)):
    for _B in (1, 3, 33, 64):                                       # n = 25 (fewer than threads) ... 6400
        BLOCK_CASES[f'{"x".join(map(str, _dims))} B={_B}'] = (_dims, _head, _B, 3, (0, 2), _base + _B, None)
BLOCK_CASES.update({
    'n=255': ((2, 8, 5, 17), (32, 24), 3, 1, (0,), 255, None),      # one short of the thread stride
    'n=256': ((2, 8, 16, 16), (32, 24), 1, 1, (0,), 256, None),     # the stride exactly
    'n=258': ((2, 8, 3, 43), (32, 24), 2, 1, (0,), 258, None),      # two past it
    'one row': ((2, 3, 1, 6), (7, 5), 1, 3, (0, 2), 6, None),       # n = 6
    'n=2': ((2, 3, 1, 2), (7, 5), 1, 3, (0, 2), 2, None),           # the smallest n: the unbiased factor is 2
    'constant': ((3, 8, 4, 4), (32, 24), 2, 1, (0,), 32, 'constant'),   # n = 32; channel 0: zero weights, bias 0.5, beta 0
    'offset': ((3, 8, 5, 5), (72, 40), 3, 3, (0, 2), 100, 'offset'),    # bias 100 on unit-scale weights: |mu| >> sigma
})
SEED_OVERRIDES = {}                 # case -> the seed that replaced a base seed which broke the side condition


def block_case(name, n_items=None):
    """-> (conv, head, shape, table, targets, batches, lrs, judged steps)."""
    (Ci, Co, H, W), heads, B, steps, judged, seed, kind = BLOCK_CASES[name]
    seed = SEED_OVERRIDES.get(name, seed)
    conv = cr.synth_block(Ci, Co, seed, scale=3.0 if kind == 'offset' else 2.0)
    if kind == 'constant':
        conv[0][0], conv[1][0], conv[3][0] = 0, 0.5, 0
    if kind == 'offset':
        conv[1][:] = 100
    head = tr.synth_head(Co * H * W, *heads, seed=seed + 1, scale=3.0)
    n_items = n_items or max(B + 2, 12)
    table, tgt = cr.synth_inputs(n_items, Ci, H, W, seed + 2)
    rng = np.random.default_rng(seed + 3)
    batches = [rng.integers(0, n_items, B)[::-1].copy() for _ in range(steps)]      # with repetition, out of order
    return conv, head, (Ci, H, W), table, tgt, batches, [LR * 0.9 ** s for s in range(steps)], judged


STAGE_SEEDS = {3: 100, 33: 100}     # batch size -> seed of the 'unequal' stage (train_stage_reference.CASES)


def stage_case(B, steps=3, n_items=40, seed=None):
    """The 'unequal' stage (3, 5, 4, 8, 6, 6) -> (convs, head, shape, table, targets, batches, lrs)."""
    dims, heads = sr.CASES['unequal']
    seed = STAGE_SEEDS[B] if seed is None else seed
    convs, head, shape, table, tgt = sr.synth_stage(dims, heads, seed=seed, n=n_items)
    rng = np.random.default_rng(seed + B)
    batches = [rng.integers(0, n_items, B)[::-1].copy() for _ in range(steps)]
    return convs, head, shape, table, tgt, batches, [LR * 0.9 ** s for s in range(steps)]

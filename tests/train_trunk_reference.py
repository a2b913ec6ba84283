"""Reference for the training of every conv block, the stride-2 front included (CPU only; nothing here is taken from the
kernels in csrc/train_conv.hip), on top of tests/train_conv_reference.py (the block, synthetic cases), tests/
train_stage_reference.py (the pool and its winners), tests/train_bn_reference.py (batch statistics: the formulas are
restated here for a strided z and compared with it bit for bit at stride 1 by test_train_trunk_cpu.py) and
tests/train_reference.py (Adam, the judge).

A block is Conv2d 3x3, padding 1, stride s in (1, 2), BatchNorm2d, LeakyReLU(0.1): Hout = (Hin - 1) // s + 1, and
    z[b,co,h,w] = bias[co] + sum_{ci,ky,kx} weight[co,ci,ky,kx] x[b,ci,h*s+ky-1,w*s+kx-1]   (0 outside the input map),
    dW[co,ci,ky,kx] = sum_{b,h,w} dz[b,co,h,w] x[b,ci,h*s+ky-1,w*s+kx-1],
    dx[b,ci,hi,wi] = sum over those (co,ky,kx) of weight[co,ci,ky,kx] dz[b,co,(hi-ky+1)/s,(wi-kx+1)/s] for which both
                     numerators are multiples of s and the position lies in the output map.
Restated in torch for any dtype: f64 from f32 inputs is the reference, plain f32 on the CPU the yardstick. The chain is any
list of blocks with a (stride, pooled, trained) each, an nn.MaxPool2d(2, 2) behind every pooled block, driven by a fixed
gradient dfeat with respect to its output: ConvTrunkTrainer's contract -- back to front, a block's input gradient before its
own step and only where a trained block lies in front, every gradient from weights that have not moved, a forward-only
block never stepping.

LeakyReLU's side and the pools' winners are discrete. The judge takes the winners from the run under test (as
train_stage_reference does), and every case's seed is one for which the f64 reference has no element with 0 < |y| <
SIDE_MARGIN (|gamma zhat| + |beta|) (train_bn_reference's side condition; `near_zero` counts, test_train_trunk_cpu.py asserts
0 for every case of the GPU file). No element is ever excluded."""
import re

import numpy as np
import torch
import torch.nn.functional as F

import train_bn_reference as bn
import train_conv_reference as cr
import train_reference as tr
import train_stage_reference as sr

SLOPE, BN_EPS, MOMENTUM, SIDE_MARGIN = cr.SLOPE, cr.BN_EPS, bn.MOMENTUM, bn.SIDE_MARGIN
CH = bn.CH
_t = cr._t
# seeded faults. Of one block: the window starting at 0 instead of -1; the output size rounded up (Hin // s + 1) in the flat
# index; the data gradient's parity test dropped, or taken on hi - ky instead of hi - ky + 1; H and W exchanged in the
# strided index. Of the chain: the second pool's gradient not routed (handed to the whole window); a forward-only block
# that steps.
BLOCK_FAULTS = ('window0', 'size_up', 'no_parity', 'parity_shift', 'hw_swapped')
CHAIN_FAULTS = ('pool2_skipped', 'frozen_steps')
FAULTS = BLOCK_FAULTS + CHAIN_FAULTS


def out_size(n, s):
    return (n - 1) // s + 1


# ------------------------------------------------------------------------------------------------ one strided block
def conv_z(w, x, s, fault=None):
    """z [B,Co,Hout,Wout] of x [B,Ci,Hin,Win]."""
    B, Ci, Hin, Win = x.shape
    Ho, Wo = out_size(Hin, s), out_size(Win, s)
    if fault == 'window0':
        return F.conv2d(F.pad(x, (0, 2, 0, 2)), w[0], w[1], stride=s)[:, :, :Ho, :Wo]
    if fault == 'hw_swapped':                             # the flat input read as [Win][Hin] maps, the flat output as such
        return F.conv2d(x.reshape(B, Ci, Win, Hin), w[0], w[1], stride=s, padding=1).reshape(B, -1, Ho, Wo)
    if fault == 'size_up':                                # Hin // s + 1 rows and columns in the flat index of the output
        Hu, Wu = Hin // s + 1, Win // s + 1
        z = F.conv2d(F.pad(x, (1, 1 + s * (Wu - Wo), 1, 1 + s * (Hu - Ho))), w[0], w[1], stride=s)
        return z.reshape(B, z.shape[1], -1)[:, :, :Ho * Wo].reshape(B, -1, Ho, Wo)
    return F.conv2d(x, w[0], w[1], stride=s, padding=1)


def block_forward(w, stats, x, s=1, batch_stats=False, momentum=MOMENTUM, fault=None):
    """w = [conv.weight, conv.bias, gamma, beta], stats = (running_mean, running_var) -> dict(z, zhat, y, F, inv_sigma,
    near_zero; with batch_stats also n and stats: the moved running statistics). The normalisation is
    train_conv_reference.block_forward's, or train_bn_reference.bn_forward's with batch_stats."""
    z = conv_z(w, x, s, fault)
    out = {}
    if batch_stats:
        n = z.numel() // z.shape[1]
        if n < 2:
            raise ValueError(f'batch statistics need more than {n} value per channel')
        mu = z.sum((0, 2, 3)) / n
        var = ((z - mu[CH]) ** 2).sum((0, 2, 3)) / n
        inv = 1.0 / torch.sqrt(var + BN_EPS)
        zhat = (z - mu[CH]) * inv[CH]
        out = dict(n=n, mu=mu, var=var,
                   stats=((1 - momentum) * stats[0] + momentum * mu, (1 - momentum) * stats[1] + momentum * (var * (n / (n - 1)))))
    else:
        inv = 1.0 / torch.sqrt(stats[1] + BN_EPS)
        zhat = (z - stats[0][CH]) * inv[CH]
    y = w[2][CH] * zhat + w[3][CH]
    near = (y.abs() < SIDE_MARGIN * ((w[2][CH] * zhat).abs() + w[3][CH].abs())) & (y != 0)
    out.update(z=z, zhat=zhat, y=y, F=torch.where(y > 0, y, SLOPE * y), inv_sigma=inv, near_zero=int(near.sum()))
    return out


def block_dz(w, fwd, dF, batch_stats=False):
    """-> (dz, dgamma, dbeta, dbias): dbias = sum dz, or 0 by definition with batch statistics."""
    y, zhat = fwd['y'], fwd['zhat']
    dy = dF * torch.where(y > 0, torch.ones_like(y), torch.full_like(y, SLOPE))
    dgamma, dbeta = (dy * zhat).sum((0, 2, 3)), dy.sum((0, 2, 3))
    fold = (w[2] * fwd['inv_sigma'])[CH]
    if batch_stats:
        n = fwd['n']
        return fold * (dy - (dbeta / n)[CH] - zhat * (dgamma / n)[CH]), dgamma, dbeta, torch.zeros_like(w[1])
    dz = dy * fold
    return dz, dgamma, dbeta, dz.sum((0, 2, 3))


def weight_grad(x, dz, s, fault=None):
    """dW [Co,Ci,3,3] in closed form."""
    Ho, Wo = dz.shape[2:]
    off = 1 if fault == 'window0' else 0
    xp = F.pad(x, (1, 1 + off, 1, 1 + off))
    dW = torch.zeros((dz.shape[1], x.shape[1], 3, 3), dtype=dz.dtype)
    for ky in range(3):
        for kx in range(3):
            win = xp[:, :, ky + off:ky + off + s * (Ho - 1) + 1:s, kx + off:kx + off + s * (Wo - 1) + 1:s]
            dW[:, :, ky, kx] = torch.einsum('bohw,bihw->oi', dz, win)
    return dW


def input_grad(weight, dz, in_size, s, fault=None):
    """dx [B,Ci,Hin,Win] in gather form: per tap, the input positions whose (hi - ky + 1, wi - kx + 1) are multiples of s and
    lie in the output map take weight[:, :, ky, kx]^T dz there."""
    Hin, Win = in_size
    B, Co, Ho, Wo = dz.shape
    dx = torch.zeros((B, weight.shape[1], Hin, Win), dtype=dz.dtype)

    def reach(n_in, n_out, k):
        i = np.arange(n_in)
        num = i - k + 1
        if fault == 'no_parity' or s == 1:
            ok = num >= 0
        elif fault == 'parity_shift':
            ok = (num >= 0) & ((i - k) % s == 0)
        else:
            ok = (num >= 0) & (num % s == 0)
        o = num // s
        ok &= (o >= 0) & (o < n_out)
        return torch.from_numpy(i[ok]), torch.from_numpy(o[ok])

    for ky in range(3):
        hi, ho = reach(Hin, Ho, ky)
        for kx in range(3):
            wi, wo = reach(Win, Wo, kx)
            if len(hi) and len(wi):
                part = torch.einsum('bohw,oi->bihw', dz[:, :, ho][:, :, :, wo], weight[:, :, ky, kx])
                dx[:, :, hi[:, None], wi[None, :]] += part
    return dx


def block_gradients(w, x, fwd, dF, s=1, batch_stats=False, fault=None):
    """-> ([dW, dbias, dgamma, dbeta] (train_conv_reference.CONV_TENSORS order, no weight decay), dz)."""
    dz, dgamma, dbeta, dbias = block_dz(w, fwd, dF, batch_stats)
    return [weight_grad(x, dz, s, fault), dbias, dgamma, dbeta], dz


# ------------------------------------------------------------------------------------------------ the chain
def new_state(convs, dtype, start=None):
    """convs: per block six f32 arrays (train_conv_reference.synth_block's order) -> list of dict(cw, cm, cv, stats, nbt, t).
    start: a snapshot() to take tensors, moments, statistics, batch and step counts from."""
    state = []
    for k, conv in enumerate(convs):
        cw = [_t(a, dtype).clone() for a in conv[:4]]
        blk = dict(cw=cw, cm=[torch.zeros_like(a) for a in cw], cv=[torch.zeros_like(a) for a in cw],
                   stats=(_t(conv[4], dtype), _t(conv[5], dtype)), nbt=0, t=0)
        if start is not None:
            for key in ('cw', 'cm', 'cv'):
                blk[key] = [_t(a, dtype).clone() for a in start[k][key]]
            blk['stats'] = tuple(_t(a, dtype) for a in start[k]['stats'])
            blk['nbt'], blk['t'] = start[k]['nbt'], start[k]['t']
        state.append(blk)
    return state


def snapshot(state):
    c = lambda L: [a.numpy().copy() for a in L]
    return [dict(cw=c(b['cw']), cm=c(b['cm']), cv=c(b['cv']), stats=c(b['stats']), nbt=b['nbt'], t=b['t']) for b in state]


def chain_forward(state, spec, x, batch_stats=False, momentum=MOMENTUM, winners=None, commit=True):
    """spec: per block (stride, pooled, trained). -> per block dict(x: its input, fwd, win, out: what the next block reads).
    A trained block normalises with batch statistics when asked and then moves its running statistics and its count."""
    kept = []
    for k, (blk, (s, pooled, trained)) in enumerate(zip(state, spec)):
        bs = batch_stats and trained
        fwd = block_forward(blk['cw'], blk['stats'], x, s, bs, momentum)
        if bs and commit:
            blk['stats'], blk['nbt'] = fwd['stats'], blk['nbt'] + 1
        win = None
        out = fwd['F']
        if pooled:
            win = sr.pool_winners(fwd['F']) if winners is None or winners[k] is None else winners[k]
            out = sr.pool_forward(fwd['F'], win)
        kept.append(dict(x=x, fwd=fwd, win=win, out=out))
        x = out
    return kept


def chain_step(state, spec, x, dfeat, lr, wd, eps=tr.EPS, batch_stats=False, momentum=MOMENTUM, winners=None, fault=None):
    """One step of the chain from dfeat, the gradient with respect to its output; every tensor of `state` moves in place.
    -> dict of [B, .] tensors: 'F{k}' every block's output, 'P{k}' its pooled output, and the gradients handed on, 'dF{k}'
    with respect to block k's output in front of its pool and 'dP{k}' with respect to the pooled one (k counts the chain's
    blocks from 0), plus 'near_zero'."""
    B = x.shape[0]
    kept = chain_forward(state, spec, x, batch_stats, momentum, winners)
    out = dict(near_zero=sum(k['fwd']['near_zero'] for k in kept))
    for k, kp in enumerate(kept):
        out[f'F{k}'] = kp['fwd']['F'].reshape(B, -1)
        if spec[k][1]:
            out[f'P{k}'] = kp['out'].reshape(B, -1)
    trained = [tr_ for _, _, tr_ in spec]
    first = trained.index(True) if True in trained else len(spec)
    assert all(trained[first:]), 'the trained blocks are the last ones'
    stop = first - 1 if fault == 'frozen_steps' and first > 0 else first
    pools = [k for k, (_, p, _) in enumerate(spec) if p]
    g = dfeat.reshape(kept[-1]['out'].shape)
    for k in range(len(spec) - 1, stop - 1, -1):
        blk, (s, pooled, _), kp = state[k], spec[k], kept[k]
        bs = batch_stats and trained[k]
        if pooled:
            if fault == 'pool2_skipped' and len(pools) > 1 and k == pools[1]:
                f = kp['fwd']['F']
                up = torch.zeros_like(f)
                up[:, :, :2 * g.shape[2], :2 * g.shape[3]] = g.repeat_interleave(2, 2).repeat_interleave(2, 3)
                g = up
            else:
                g = sr.pool_backward(kp['fwd']['F'], g, kp['win'])
            out[f'dF{k}'] = g.reshape(B, -1)
        grads, dz = block_gradients(blk['cw'], kp['x'], kp['fwd'], g, s, bs)
        dx = input_grad(blk['cw'][0], dz, kp['x'].shape[2:], s) if k > stop else None
        blk['t'] += 1
        for i, gr in enumerate(grads):
            tr.adam(blk['cw'][i], gr, blk['cm'][i], blk['cv'][i], blk['t'], lr, wd, None, eps)
        if dx is not None:
            out[f"d{'P' if spec[k - 1][1] else 'F'}{k - 1}"] = dx.reshape(B, -1)
            g = dx
    return out


def run_steps(convs, spec, shape, table, batches, dfeats, lrs, wd, dtype, eps=tr.EPS, batch_stats=False, momentum=MOMENTUM,
              start=None, winners=None, fault=None):
    """len(batches) steps on rows batches[i] of the f32 table [n, Ci*Hin*Win] with the gradients dfeats[i] [B, out width];
    shape = (Ci, Hin, Win) -> (list of chain_step results as numpy, list of per-step snapshots). winners: per step, per
    block the pool winners to use or None."""
    state = new_state(convs, dtype, start)
    X = _t(table, dtype).reshape(len(table), *shape)
    outs, snaps = [], []
    for i, (idx, dfe, lr) in enumerate(zip(batches, dfeats, lrs)):
        idx = torch.from_numpy(np.asarray(idx, np.int64))
        r = chain_step(state, spec, X[idx], _t(dfe, dtype), lr, wd, eps, batch_stats, momentum,
                       None if winners is None else winners[i], fault)
        outs.append({k: (v.numpy().copy() if isinstance(v, torch.Tensor) else v) for k, v in r.items()})
        snaps.append(snapshot(state))
    return outs, snaps


def chain_sizes(spec, shape, convs):
    """Per block (Ci, Co, Hin, Win, Hout, Wout) and the chain's output (C, H, W)."""
    _, h, w = shape
    sizes = []
    for conv, (s, pooled, _) in zip(convs, spec):
        Co, Ci = np.asarray(conv[0]).shape[:2]
        ho, wo = out_size(h, s), out_size(w, s)
        sizes.append((Ci, Co, h, w, ho, wo))
        h, w = (ho // 2, wo // 2) if pooled else (ho, wo)
    return sizes, (sizes[-1][1], h, w)


# ------------------------------------------------------------------------------------------------ the judge
# quantity -> (C_max, C_rms) where the MI355X needs more than train_reference.BOUND_DEFAULT, by the project's rule: twice the
# worst measured ratio, rounded up to a whole number, never above the caps 8 / 4, which every seeded fault of
# test_train_trunk_cpu.py exceeds. The measured ratio stands beside each entry and in DESIGN.md 6.8e.
# Measured over every case of test_train_trunk_gpu.py, each step judged on its own. With running statistics every quantity
# of the strided kernels and of the chains at depths 4 to 8 stayed within the default (the worst: F 0.39 / 0.42, dx 0.54 /
# 0.63, the chain's outputs 0.91 / 1.16, its gradients 0.16 / 0.33, its updates and moments 0.52 / 0.70) except the two named
# first: four numbers and twenty numbers.
# The names ending in ' bs' are the chain with batch statistics (depth 8, B = 2), whose last block normalises over n = 4
# values per channel on its 2 x 1 maps: at step 3 the f32 yardstick itself is 16 ulp off there (1.2e-5 on gradients of 6),
# every gradient behind that block inherits its dz, and so do the first moments that are sums of them. Steps 1 and 2 and
# every other quantity of that run stayed within the default.
BOUND_OVERRIDES = {'update batchnorm.weight': (2.0, 4.0),           # measured 0.81 / 1.73 (stride 1 on 5 x 66, 4 numbers)
                   'P3': (2.0, 4.0),                                # 0.74 / 1.53 (first_block 3: block 6's pooled 2 x 1 maps)
                   'dP6 bs': (5.0, 4.0),                            # 2.08 / 2.48: twice the rms is beyond the cap, as below
                   'dF6 bs': (5.0, 4.0),                            # 2.08 / 2.44
                   'dF5 bs': (5.0, 4.0),                            # 2.23 / 2.36
                   'dP4 bs': (5.0, 4.0),                            # 2.48 / 2.59
                   'dF4 bs': (5.0, 4.0),                            # 2.48 / 2.54
                   'dF3 bs': (4.0, 4.0),                            # 2.00 / 2.53
                   'dP2 bs': (7.0, 4.0),                            # 3.12 / 2.50
                   'dF2 bs': (7.0, 4.0),                            # 3.12 / 2.45
                   'dF1 bs': (7.0, 4.0),                            # 3.07 / 2.61
                   'dF0 bs': (6.0, 4.0),                            # 2.75 / 2.52
                   'm b0 batchnorm.weight bs': (4.0, 4.0),          # 1.95 / 3.00
                   'm b0 batchnorm.bias bs': (3.0, 4.0),            # 1.42 / 2.02
                   'm b1 conv.weight bs': (4.0, 4.0),               # 1.68 / 1.57
                   'm b1 batchnorm.weight bs': (3.0, 4.0),          # 1.27 / 2.21
                   'm b1 batchnorm.bias bs': (2.0, 4.0),            # 0.99 / 1.77
                   'm b2 batchnorm.weight bs': (3.0, 4.0),          # 1.14 / 2.36
                   'm b2 batchnorm.bias bs': (2.0, 4.0),            # 0.94 / 1.74
                   'm b3 conv.weight bs': (3.0, 4.0),               # 1.27 / 1.60
                   'm b3 batchnorm.bias bs': (2.0, 4.0),            # 0.76 / 1.57
                   'm b4 batchnorm.bias bs': (2.0, 4.0),            # 0.58 / 1.98
                   'm b6 batchnorm.weight bs': (2.0, 4.0),          # 0.88 / 1.92
                   'm b6 batchnorm.bias bs': (2.0, 4.0),            # 0.56 / 1.57
                   'm b7 conv.weight bs': (3.0, 4.0)}               # 1.35 / 1.58


def bound_for(name):
    """The quantity's own override, else train_conv_reference's for the same tensor of any block (the same kernels on the
    same tensors, judged the same way: 'm b5 batchnorm.bias' -> 'm batchnorm.bias'), else train_reference's."""
    base = name[:-3] if name.endswith(' bs') else name          # the chain with batch statistics: its own entry, or the plain one
    b = (BOUND_OVERRIDES.get(name) or BOUND_OVERRIDES.get(base) or cr.BOUND_OVERRIDES.get(re.sub(r' b\d ', ' ', base))
         or tr.bound_for(base))
    assert b[0] <= tr.CAP_MAX and b[1] <= tr.CAP_RMS, f'bound {b} for {name} exceeds the caps {(tr.CAP_MAX, tr.CAP_RMS)}'
    return b


def _one(got, r, y, name, label, log, collect, bound):
    try:
        tr.judge(got, r, y, f'{name} @{label}', log=log, bound=bound or bound_for(name))
    except tr.TrainMismatch as e:
        if collect is None:
            raise
        collect.append(str(e))


def judge_restarted(outs, snaps, args, steps, label='', eps=tr.EPS, batch_stats=False, momentum=MOMENTUM, bound=None, log=None,
                    collect=None, names=None):
    """train_conv_reference.judge_restarted's scheme for the chain: step s of the run under test (outs: per step dicts with
    chain_step's keys, snaps: per step snapshot()s) against ONE step of the f64 reference and of the f32 yardstick, both
    restarted from what the run under test held after step s - 1, with the pool winners of its own outputs. Judged: every
    key of chain_step that `outs` holds; update, m, v of every trained block's tensors, and with batch_stats their running
    statistics; the counts exactly. A forward-only block must hold the bytes it held. The side condition is asserted of the
    restarted f64 reference. args = (convs, spec, shape, table, batches, dfeats, lrs, wd); names: per block its label."""
    convs, spec, shape, table, batches, dfeats, lrs, wd = args
    sizes, _ = chain_sizes(spec, shape, convs)
    names = names or [f'b{k}' for k in range(len(spec))]
    sfx = ' bs' if batch_stats else ''
    for s in steps:
        B = len(batches[s])
        win = [sr.pool_winners(torch.from_numpy(outs[s][f'F{k}']).reshape(B, sz[1], sz[4], sz[5])) if sp[1] else None
               for k, (sp, sz) in enumerate(zip(spec, sizes))]
        a = (convs, spec, shape, table, [batches[s]], [dfeats[s]], [lrs[s]], wd)
        kw = dict(eps=eps, batch_stats=batch_stats, momentum=momentum, start=None if s == 0 else snaps[s - 1], winners=[win])
        ((r,), (rs,)), ((y,), (ys,)) = run_steps(*a, dtype=torch.float64, **kw), run_steps(*a, dtype=torch.float32, **kw)
        lab = f'{label} step {s + 1}'
        if r['near_zero'] and collect is not None:
            collect.append(f'{lab}: {r["near_zero"]} elements of the f64 reference break the side condition: choose another seed')
        assert collect is not None or not r['near_zero'], lab
        want = set(r) - {'near_zero'}
        if want != set(outs[s]):                              # nothing the reference forms may be left out, nothing added
            msg = f'{lab}: quantities {sorted(want ^ set(outs[s]))} are missing or not the chain\'s'
            if collect is None:
                raise tr.TrainMismatch(msg)
            collect.append(msg)
        for q in sorted(want & set(outs[s])):
            _one(outs[s][q], r[q], y[q], q + sfx, lab, log, collect, bound)
        before = new_snapshot(convs) if s == 0 else snaps[s - 1]
        for k, (sp, name) in enumerate(zip(spec, names)):
            g, rr, yy, b0 = snaps[s][k], rs[k], ys[k], before[k]
            if not sp[2]:
                same = all(np.asarray(u).tobytes() == np.asarray(v).tobytes()
                           for key in ('cw', 'cm', 'cv', 'stats') for u, v in zip(g[key], b0[key]))
                if not (same and g['t'] == b0['t'] and g['nbt'] == b0['nbt']):
                    msg = f'{lab}: the forward-only block {name} has moved'
                    if collect is None:
                        raise tr.TrainMismatch(msg)
                    collect.append(msg)
                continue
            assert (g['t'], g['nbt']) == (rr['t'], rr['nbt']), (lab, name, g['t'], g['nbt'], rr['t'], rr['nbt'])
            for i, tname in enumerate(cr.CONV_TENSORS):
                w0 = np.asarray(b0['cw'][i], np.float64)
                _one(g['cw'][i] - w0, rr['cw'][i] - w0, yy['cw'][i] - w0, f'update {name} {tname}{sfx}', lab, log, collect, bound)
                _one(g['cm'][i], rr['cm'][i], yy['cm'][i], f'm {name} {tname}{sfx}', lab, log, collect, bound)
                _one(g['cv'][i], rr['cv'][i], yy['cv'][i], f'v {name} {tname}{sfx}', lab, log, collect, bound)
            if batch_stats:
                for i, sname in enumerate(('running_mean', 'running_var')):
                    _one(g['stats'][i], rr['stats'][i], yy['stats'][i], f'{sname} {name}{sfx}', lab, log, collect, bound)


def new_snapshot(convs):
    return snapshot(new_state(convs, torch.float32))


def judge_block(got, conv, x, dF, s, label, batch_stats=False, lr=1e-2, wd=0.05, eps=1e-3, momentum=MOMENTUM, bound=None,
                log=None, collect=None, fault=None):
    """One block on its own: got = dict(F, dx [B, .], cw, cm, cv: four arrays each after one step from zero moments, and with
    batch_stats stats: the moved running statistics) against the same step in f64 and in f32. x [B,Ci,Hin,Win], dF
    [B,Co,Hout,Wout] f32 arrays. fault: seed it into the f64 side's stand-in for `got` (test_train_trunk_cpu.py)."""
    res = []
    for dtype in (torch.float64, torch.float32):
        w = [_t(a, dtype).clone() for a in conv]
        xt, dFt = _t(x, dtype), _t(dF, dtype)
        fwd = block_forward(w[:4], (w[4], w[5]), xt, s, batch_stats, momentum, fault)
        grads, dz = block_gradients(w[:4], xt, fwd, dFt, s, batch_stats, fault)
        dx = input_grad(w[0], dz, xt.shape[2:], s, fault)
        m, v = [torch.zeros_like(a) for a in w[:4]], [torch.zeros_like(a) for a in w[:4]]
        for i, g in enumerate(grads):
            tr.adam(w[i], g, m[i], v[i], 1, lr, wd, None, eps)
        c = lambda L: [a.numpy().copy() for a in L]
        res.append(dict(F=fwd['F'].reshape(len(x), -1).numpy(), dx=dx.reshape(len(x), -1).numpy(), cw=c(w[:4]), cm=c(m), cv=c(v),
                        stats=c(fwd['stats']) if batch_stats else None, near_zero=fwd['near_zero']))
    if got is None:
        return res
    r, y = res
    assert not r['near_zero'], f'{label}: {r["near_zero"]} elements of the f64 reference break the side condition'
    for q in ('F', 'dx'):
        _one(got[q], r[q], y[q], q, label, log, collect, bound)
    for i, tname in enumerate(cr.CONV_TENSORS):
        w0 = np.asarray(conv[i], np.float64)
        _one(got['cw'][i] - w0, r['cw'][i] - w0, y['cw'][i] - w0, f'update {tname}', label, log, collect, bound)
        _one(got['cm'][i], r['cm'][i], y['cm'][i], f'm {tname}', label, log, collect, bound)
        _one(got['cv'][i], r['cv'][i], y['cv'][i], f'v {tname}', label, log, collect, bound)
    if batch_stats:
        for i, sname in enumerate(('running_mean', 'running_var')):
            _one(got['stats'][i], r['stats'][i], y['stats'][i], sname, label, log, collect, bound)


# ------------------------------------------------------------------------------------------------ synthetic cases
# (Ci, Co, Hin, Win, B) at stride 2: odd and even input sides, a single window (1 x 1), Co and Ci one past the 64-wide tile,
# r = B*Hout*Wout one past 64 (65 x 8 x 5 x 13: the data gradient's r = 65), K9 = 9 Ci no multiple of 16
BLOCK_CASES = [(5, 20, 7, 10, 2), (5, 20, 8, 9, 3), (20, 40, 6, 6, 1), (3, 65, 9, 16, 1), (65, 8, 5, 13, 1), (2, 3, 1, 1, 2),
               (2, 3, 2, 3, 2)]
BN_CASES = [(5, 20, 7, 10, 2), (5, 20, 8, 9, 3)]            # the two that also run with batch statistics
WIDE_CASE = (3, 4, 5, 66, 2)                                # stride 1 on a map beyond the old create's 64
BLOCK_SEEDS = {}                                            # (case, batch_stats) -> the seed that replaced a base seed which
                                                            # broke the side condition


def block_case(case, s=2, batch_stats=False):
    """-> (conv, x [B,Ci,Hin,Win], dF [B,Co,Hout,Wout]) f32 arrays."""
    Ci, Co, Hin, Win, B = case
    seed = BLOCK_SEEDS.get((case, batch_stats), 1000 + 7 * Ci + Co + 31 * Hin + Win)
    conv = cr.synth_block(Ci, Co, seed, scale=2.0)
    x, _ = cr.synth_inputs(B, Ci, Hin, Win, seed + 1)
    dF = np.random.default_rng(seed + 2).normal(0, 1, (B, Co, out_size(Hin, s), out_size(Win, s))).astype(np.float32)
    return conv, x.reshape(B, Ci, Hin, Win), dF


# The synthetic trunk: eight blocks with the deployed strides and pools and narrow channels. On an 80 x 48 input the maps
# are 40 x 24, 20 x 12, 20 x 12 -> 10 x 6, 10 x 6, 10 x 6 -> 5 x 3, 5 x 3, 5 x 3 -> 2 x 1, 2 x 1: the last pool floors both
# sides and leaves 2 x 1 maps.
TRUNK_STRIDES = (2, 2, 1, 1, 1, 1, 1, 1)
TRUNK_POOLED = (False, False, True, False, True, False, True, False)
TRUNK_CHANNELS = (5, 3, 4, 6, 5, 6, 4, 5, 7)
TRUNK_IN = (80, 48)
TRUNK_SEEDS = {}                                            # (first_block, n_trained, batch_stats) -> replacement seed


def trunk_case(first_block, n_trained, batch_stats=False, n=6, B=2, steps=3):
    """The synthetic trunk from first_block on, of which the last n_trained blocks train -> (convs, spec, shape, table,
    batches, dfeats, lrs, wd) -- judge_restarted's args -- for `steps` steps of batches of B rows out of n."""
    seed = TRUNK_SEEDS.get((first_block, n_trained, batch_stats), 500)
    blocks = list(range(first_block, 8))
    convs = [cr.synth_block(TRUNK_CHANNELS[k], TRUNK_CHANNELS[k + 1], seed + k, scale=2.0) for k in blocks]
    spec = [(TRUNK_STRIDES[k], TRUNK_POOLED[k], i >= len(blocks) - n_trained) for i, k in enumerate(blocks)]
    h, w = TRUNK_IN
    for k in range(first_block):
        h, w = out_size(h, TRUNK_STRIDES[k]), out_size(w, TRUNK_STRIDES[k])
        if TRUNK_POOLED[k]:
            h, w = h // 2, w // 2
    shape = (TRUNK_CHANNELS[first_block], h, w)
    table, _ = cr.synth_inputs(n, *shape, seed + 20)
    _, (C, ho, wo) = chain_sizes(spec, shape, convs)
    rng = np.random.default_rng(seed + 30)
    batches = [rng.integers(0, n, B)[::-1].copy() for _ in range(steps)]
    dfeats = [rng.normal(0, 1, (B, C * ho * wo)).astype(np.float32) for _ in range(steps)]
    return convs, spec, shape, table, batches, dfeats, [1e-2 * 0.9 ** i for i in range(steps)], 0.05

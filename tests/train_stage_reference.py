"""Reference for the training of the whole last conv stage with the head (CPU only; nothing here is taken from the kernels
in csrc/train_conv.hip or csrc/train.hip), on top of tests/train_conv_reference.py and tests/train_reference.py.

The stage is three blocks of train_conv_reference.block_forward with nn.MaxPool2d(2, 2) between the second and the third:
    x [B,Ci,H,W] -> block A -> F5 -> block B -> F6 -> pool -> P -> block C -> F7 -> head.
Restated in torch for any dtype (f64 from f32 inputs is the reference, plain f32 on the CPU the yardstick): the chained
forward, a block's closed-form gradient with respect to its input, the pool with its gradient, and the chained step of
fine_tune_head(train_conv_blocks=depth): every gradient from weights that have not moved, one learning rate, eps and weight
decay for all trained tensors. depth = 3 trains A, B and C; depth = 2 runs A forward only.

The pool gives a window's gradient to the first maximum in the order (0,0), (0,1), (1,0), (1,1) under a strict >, as torch's
CPU max_pool2d does (test_train_stage_cpu.py compares). The judge takes the winners from the F6 of the run under test
(`winners`): the pool itself is exact and is compared bit for bit on its own, and two window elements that differ by a
rounding of F6 must not route a gradient differently in f32 and in f64 (the role the stashed z plays for LeakyReLU's sign)."""
import numpy as np
import torch
import torch.nn.functional as F

import train_conv_reference as cr
import train_reference as tr

SLOPE = cr.SLOPE
FAULTS = ('no_flip', 'transposed', 'no_slope', 'post_update_dx', 'pool_last', 'pool_all_ties', 'pool_odd_row')
BLOCKS = ('b5', 'b6', 'b7')


def _t(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dtype)


# ------------------------------------------------------------------------------------------------ the pool
def _windows(x):
    """x [B,C,H,W] -> [B,C,H//2,W//2,4] in the order (0,0), (0,1), (1,0), (1,1)."""
    B, C, H, W = x.shape
    Ho, Wo = H // 2, W // 2
    v = x[:, :, :2 * Ho, :2 * Wo].reshape(B, C, Ho, 2, Wo, 2)
    return v.permute(0, 1, 2, 4, 3, 5).reshape(B, C, Ho, Wo, 4)


def pool_winners(x, fault=None):
    """Index 0..3 of each window's winner [B,C,H//2,W//2]: the first maximum under a strict > (pool_last: the last)."""
    v = _windows(x)
    win = torch.zeros(v.shape[:-1], dtype=torch.int64)
    m = v[..., 0]
    for k in range(1, 4):
        better = (v[..., k] >= m) if fault == 'pool_last' else (v[..., k] > m)
        win = torch.where(better, torch.full_like(win, k), win)
        m = torch.where(better, v[..., k], m)
    return win


def pool_forward(x, winners=None):
    """nn.MaxPool2d(2, 2): x [B,C,H,W] -> [B,C,H//2,W//2], the value at each window's winner."""
    win = pool_winners(x) if winners is None else winners
    return torch.gather(_windows(x), 4, win[..., None])[..., 0]


def pool_backward(x, dout, winners=None, fault=None):
    """The gradient with respect to x: dout at each window's winner, zero elsewhere and in a trailing odd row or column."""
    B, C, H, W = x.shape
    Ho, Wo = H // 2, W // 2
    v = _windows(x)
    if fault == 'pool_all_ties':
        hot = v == v.max(-1, keepdim=True).values
    else:
        win = pool_winners(x, fault) if winners is None else winners
        hot = torch.arange(4)[None, None, None, None, :] == win[..., None]
    g = torch.where(hot, dout[..., None].expand_as(v), torch.zeros_like(v))
    din = torch.zeros_like(x)
    din[:, :, :2 * Ho, :2 * Wo] = g.reshape(B, C, Ho, Wo, 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(B, C, 2 * Ho, 2 * Wo)
    if fault == 'pool_odd_row' and H % 2:
        din[:, :, H - 1] = din[:, :, H - 2]
    return din


# ------------------------------------------------------------------------------------------------ a block's input gradient
def block_input_grad(w, fwd, dF, fault=None):
    """dx[b,ci,h,w] = sum_{co,ky,kx} dz[b,co,h-ky+1,w-kx+1] weight[co,ci,ky,kx] with dz = dF * (y > 0 ? 1 : 0.1) * gamma *
    inv_sigma; positions outside the map contribute nothing. w, fwd: block_forward's arguments and result."""
    ch = (None, slice(None), None, None)
    y = fwd['y']
    dy = dF if fault == 'no_slope' else dF * torch.where(y > 0, torch.ones_like(y), torch.full_like(y, SLOPE))
    dz = dy * (w[2] * fwd['inv_sigma'])[ch]
    H, W = dz.shape[2:]
    dzp = F.pad(dz, (1, 1, 1, 1))
    dx = torch.zeros((dz.shape[0], w[0].shape[1], H, W), dtype=dz.dtype)
    for ky in range(3):
        for kx in range(3):
            oy, ox = (ky, kx) if fault == 'no_flip' else (2 - ky, 2 - kx)
            k = w[0][:, :, ky, kx]
            if fault == 'transposed' and k.shape[0] == k.shape[1]:      # weight[ci, co]: only a square block can take it
                k = k.T
            dx += torch.einsum('bohw,oi->bihw', dzp[:, :, oy:oy + H, ox:ox + W], k)
    return dx


# ------------------------------------------------------------------------------------------------ the chained step
def new_state(convs, head, dtype, start=None):
    """convs: three lists of six f32 arrays (train_conv_reference.synth_block's order); head: the six of
    train_reference.TENSORS. start = (snapshot, t): the tensors, m and v as a snapshot() holds them, after t steps."""
    state = dict(head=tr.new_state(head, dtype), t=0, dtype=dtype)
    for name, conv in zip(BLOCKS, convs):
        cw = [_t(a, dtype).clone() for a in conv[:4]]
        state[name] = dict(cw=cw, cm=[torch.zeros_like(a) for a in cw], cv=[torch.zeros_like(a) for a in cw],
                           stats=(_t(conv[4], dtype), _t(conv[5], dtype)))
    if start is not None:
        snap, t = start
        for name in BLOCKS:
            for k in ('cw', 'cm', 'cv'):
                state[name][k] = [_t(a, dtype).clone() for a in snap[name][k]]
        for k in ('w', 'm', 'v'):
            state['head'][k] = [_t(a, dtype).clone() for a in snap[k]]
        state['t'] = state['head']['t'] = int(t)
    return state


def stage_forward(state, x, winners=None):
    """-> (the three block_forward results, pool winners, pooled [B,C6,H//2,W//2])."""
    f5 = cr.block_forward(state['b5']['cw'], state['b5']['stats'], x)
    f6 = cr.block_forward(state['b6']['cw'], state['b6']['stats'], f5['F'])
    win = pool_winners(f6['F']) if winners is None else winners
    pooled = pool_forward(f6['F'], win)
    f7 = cr.block_forward(state['b7']['cw'], state['b7']['stats'], pooled)
    return (f5, f6, f7), win, pooled


def stage_step(state, x, target, lam, lr, wd, depth=3, fault=None, eps=tr.EPS, winners=None):
    """One joint step; every tensor of `state` moves in place. x [B,Ci,H,W], target [B,12,12,4] in the state's dtype.
    Returns dict(F5, F6, pooled, F [B, C7*h*w], y, comps, dy, dfeat, and dpooled, dF6, dx6 where the depth forms them)."""
    head = state['head']
    hw = head['w']
    B = x.shape[0]
    (f5, f6, f7), win, pooled = stage_forward(state, x, winners)
    feats = f7['F'].reshape(B, -1)
    a1, a2, y = tr.forward(head, feats)
    comps, dy = tr.loss(y, target, lam)
    state['t'] += 1
    head['t'] += 1
    t = state['t']
    dz2 = (dy @ hw[4]) * a2 * (1 - a2)
    dz1 = (dz2 @ hw[2]) * a1 * (1 - a1)
    dfeat = dz1 @ hw[0]
    out = dict(F5=f5['F'].reshape(B, -1), F6=f6['F'].reshape(B, -1), pooled=pooled.reshape(B, -1), F=feats, y=y, comps=comps,
               dy=dy, dfeat=dfeat)

    def update(name, inp, fwd, dF):
        blk = state[name]
        for i, g in enumerate(cr.block_gradients(blk['cw'], inp, fwd, dF)):
            tr.adam(blk['cw'][i], g, blk['cm'][i], blk['cv'][i], t, lr, wd, None, eps)

    dF7 = dfeat.reshape(f7['F'].shape)
    if fault == 'post_update_dx':                       # the input gradient from a block that has already moved
        update('b7', pooled, f7, dF7)
    if depth >= 2:
        dpooled = block_input_grad(state['b7']['cw'], f7, dF7, fault)
    if fault != 'post_update_dx':
        update('b7', pooled, f7, dF7)
    if depth >= 2:
        dF6 = pool_backward(f6['F'], dpooled, None if fault in ('pool_last', 'pool_all_ties') else win, fault)
        out.update(dpooled=dpooled.reshape(B, -1), dF6=dF6.reshape(B, -1))
        if depth >= 3:
            if fault == 'post_update_dx':
                update('b6', f5['F'], f6, dF6)
            dx6 = block_input_grad(state['b6']['cw'], f6, dF6, fault)
            out['dx6'] = dx6.reshape(B, -1)
        if fault != 'post_update_dx' or depth < 3:
            update('b6', f5['F'], f6, dF6)
        if depth >= 3:
            update('b5', x, f5, dx6)
    for i, g in ((4, dy.T @ a2), (5, dy.sum(0)), (2, dz2.T @ a1), (3, dz2.sum(0)), (0, dz1.T @ feats), (1, dz1.sum(0))):
        tr.adam(hw[i], g, head['m'][i], head['v'][i], t, lr, wd, None, eps)
    return out


def snapshot(state):
    c = lambda L: [a.numpy().copy() for a in L]
    snap = dict(w=c(state['head']['w']), m=c(state['head']['m']), v=c(state['head']['v']))
    for name in BLOCKS:
        snap[name] = {k: c(state[name][k]) for k in ('cw', 'cm', 'cv')}
    return snap


def run_steps(convs, head, shape, table, targets, batches, lam, lrs, wd, dtype, depth=3, fault=None, eps=tr.EPS, start=None,
              winners=None):
    """`len(batches)` joint steps on rows batches[i] of the f32 tables table [n, Ci*H*W] and targets [n,12,12,4]; shape =
    (Ci, H, W) -> (state, list of stage_step results as numpy, list of per-step snapshots). winners: per step, the pool
    winners to use (pool_winners of the F6 of the run under test) or None."""
    state = new_state(convs, head, dtype, start)
    X = _t(table, dtype).reshape(len(table), *shape)
    T = _t(np.asarray(targets).reshape(-1, tr.S, tr.S, 4), dtype)
    outs, snaps = [], []
    for s, (idx, lr) in enumerate(zip(batches, lrs)):
        idx = torch.from_numpy(np.asarray(idx, np.int64))
        r = stage_step(state, X[idx], T[idx], lam, lr, wd, depth, fault, eps, None if winners is None else winners[s])
        outs.append({k: v.numpy().copy() for k, v in r.items()})
        snaps.append(snapshot(state))
    return state, outs, snaps


def ref_steps(*a, **k):
    return run_steps(*a, dtype=torch.float64, **k)


def yard_steps(*a, **k):
    return run_steps(*a, dtype=torch.float32, **k)


# ------------------------------------------------------------------------------------------------ the judge
# quantity -> (C_max, C_rms) where the MI355X needs more than train_reference.BOUND_DEFAULT, by the project's rule: twice the
# worst measured ratio, rounded up to a whole number, never above the caps 8 / 4, which every seeded fault of
# test_train_stage_cpu.py exceeds (the measured table is in DESIGN.md 6.8e). The last block's tensors and the head's keep
# train_conv_reference's overrides where they have one: the same kernels on the same tensors, judged the same way.
# Measured over every case of test_train_stage_gpu.py, each step judged on its own: the outputs of the new kernels stayed
# within the default where they are judged on their own inputs (`dpooled alone` 0.77 / 1.02, `dx6 alone` 0.58 / 0.88; the
# pool is exact) and so did F5, F6, pooled, F, dF6, dfeat and every update. Beyond it on rms: the two chained data gradients
# at B = 1 (36 and 108 numbers, whose dF already carries the roundings of the head and of the block behind), and per-channel
# moments of 3 to 8 numbers, each one sum over the batch of such gradients against a yardstick that is a third of an ulp
# off. `v w3` exceeds on max by one element at B = 1, as `v b3` does in train_conv_reference.
BOUND_OVERRIDES = {'dpooled': (2.0, 4.0),                           # measured 1.22 / 1.58 (B = 1)
                   'dx6': (2.0, 4.0),                               # 1.29 / 1.67 (B = 1)
                   'm b5 conv.bias': (2.0, 4.0),                    # 0.79 / 2.27: twice that is beyond the cap
                   'm b5 batchnorm.weight': (2.0, 4.0),             # 0.51 / 1.77
                   'm b5 batchnorm.bias': (2.0, 4.0),               # 0.58 / 1.98
                   'v b5 conv.bias': (2.0, 4.0),                    # 0.50 / 2.07: twice that is beyond the cap
                   'm b6 conv.bias': (2.0, 4.0),                    # 0.79 / 1.56
                   'm b6 batchnorm.bias': (2.0, 4.0),               # 0.72 / 1.98
                   'v b6 conv.bias': (2.0, 4.0),                    # 0.53 / 1.78
                   'v b6 batchnorm.bias': (2.0, 4.0),               # 0.44 / 1.73
                   'v b7 batchnorm.weight': (2.0, 4.0),             # 1.48 / 2.08: twice that is beyond the cap
                   'v w3': (5.0, 1.5)}                              # 2.06 / 0.87 (B = 1)
QUANTITIES = ('F5', 'F6', 'pooled', 'F', 'dfeat', 'dpooled', 'dF6', 'dx6')


def bound_for(name):
    b = BOUND_OVERRIDES.get(name) or cr.BOUND_OVERRIDES.get(name.replace(' b7 ', ' ')) or tr.bound_for(name)
    assert b[0] <= tr.CAP_MAX and b[1] <= tr.CAP_RMS, f'bound {b} for {name} exceeds the caps {(tr.CAP_MAX, tr.CAP_RMS)}'
    return b


def judge_restarted(outs, snaps, args, steps, depth=3, label='', eps=tr.EPS, bound=None, log=None, collect=None,
                    own_winners=True):
    """train_conv_reference.judge_restarted's scheme for the stage: step s of the run under test (outs: per step dicts with
    stage_step's keys, snaps: per step snapshot()s) against ONE step of the f64 reference and of the f32 yardstick, both
    restarted from the tensors, moments and step count the run under test held after step s - 1. Judged: every quantity of
    QUANTITIES that `outs` holds, and update, m, v of the trained blocks' tensors and of the head's. Then each input
    gradient on its own: block_input_grad from the dF of the run under test, the block's input of the run under test and
    the parameters before the step. args: run_steps' positional arguments up to wd. own_winners: take the pool winners
    from outs[s]['F6'] (module docstring)."""
    convs, head, shape, table, targets, batches, lam, lrs, wd = args
    Ci, H, W = shape
    trained = BLOCKS[3 - depth:]

    def one(got, r, y, name, s):
        try:
            tr.judge(got, r, y, f'{name} @{label} step {s + 1}', log=log, bound=bound or bound_for(name))
        except tr.TrainMismatch as e:
            if collect is None:
                raise
            collect.append(str(e))

    for s in steps:
        start = None if s == 0 else (snaps[s - 1], s)
        B = len(batches[s])
        C6 = np.asarray(convs[1][0]).shape[0]
        win = [pool_winners(torch.from_numpy(outs[s]['F6']).reshape(B, C6, H, W))] if own_winners else None
        a = (convs, head, shape, table, targets, [batches[s]], lam, [lrs[s]], wd)
        (_, (r,), (rs,)), (_, (y,), (ys,)) = (ref_steps(*a, depth=depth, eps=eps, start=start, winners=win),
                                              yard_steps(*a, depth=depth, eps=eps, start=start, winners=win))
        for q in QUANTITIES:
            if q in outs[s]:
                one(outs[s][q], r[q], y[q], q, s)
        before = dict(w=head, **{n: dict(cw=c[:4]) for n, c in zip(BLOCKS, convs)}) if s == 0 else snaps[s - 1]
        groups = [(n, snaps[s][n], rs[n], ys[n], before[n]['cw'], 'cw', 'cm', 'cv', cr.CONV_TENSORS) for n in trained]
        groups.append(('', snaps[s], rs, ys, before['w'], 'w', 'm', 'v', tr.TENSORS))
        for n, g, rr, yy, w0s, kw, km, kv, names in groups:
            for i, name in enumerate(names):
                name = f'{n} {name}'.strip()
                w0 = np.asarray(w0s[i], np.float64)
                one(g[kw][i] - w0, rr[kw][i] - w0, yy[kw][i] - w0, f'update {name}', s)
                one(g[km][i], rr[km][i], yy[km][i], f'm {name}', s)
                one(g[kv][i], rr[kv][i], yy[kv][i], f'v {name}', s)
        # each input gradient from the dF, the block input and the parameters of the run under test
        for q, blk, inp, dF, side in (('dpooled', 'b7', 'pooled', 'dfeat', (H // 2, W // 2)), ('dx6', 'b6', 'F5', 'dF6', (H, W))):
            if q not in outs[s]:
                continue
            res = []
            for dtype in (torch.float64, torch.float32):
                st = new_state(convs, head, dtype, start)[blk]
                Co, Cin = st['cw'][0].shape[:2]
                fwd = cr.block_forward(st['cw'], st['stats'], _t(outs[s][inp], dtype).reshape(B, Cin, *side))
                res.append(block_input_grad(st['cw'], fwd, _t(outs[s][dF], dtype).reshape(B, Co, *side)).reshape(B, -1).numpy())
            one(outs[s][q], res[0], res[1], f'{q} alone', s)


# ------------------------------------------------------------------------------------------------ synthetic cases
# (Ci, C5, C6, C7, H, W), (H1, H2): the stage cases of both test files
CASES = {'unequal': ((3, 5, 4, 8, 6, 6), (72, 40)),         # no two channel counts equal; the third block on 3 x 3 maps
         'square_odd': ((2, 6, 6, 8, 5, 7), (130, 68)),     # the middle block square; odd maps: the pool floors to 2 x 3
         'one_row': ((2, 3, 3, 8, 2, 6), (32, 24))}         # the pooled map is one row


def synth_stage(dims, heads, seed, n=40):
    """dims = (Ci, C5, C6, C7, H, W), heads = (H1, H2) -> (convs, head, shape, table, targets), in the style of
    train_conv_reference's cases."""
    Ci, C5, C6, C7, H, W = dims
    convs = [cr.synth_block(a, b, seed + i, scale=2.0) for i, (a, b) in enumerate(((Ci, C5), (C5, C6), (C6, C7)))]
    head = tr.synth_head(C7 * (H // 2) * (W // 2), *heads, seed=seed + 5, scale=3.0)
    table, tgt = cr.synth_inputs(n, Ci, H, W, seed + 7)
    return convs, head, (Ci, H, W), table, tgt


def tied_table(table):
    """Rows that are all zero (the first half) and rows of one constant each: every pooling window that no tap reaches the
    zero padding from ties exactly (on 6 x 6 maps: the middle one of block 6's nine)."""
    out = np.zeros_like(table)
    half = len(table) // 2
    out[half:] = np.linspace(0.3, 1.7, len(table) - half, dtype=np.float32)[:, None]
    return out


def pool_input(n, H, W, seed):
    """[n, H, W] f32 with ties at each of the four window positions, -0.0 against +0.0 and whole constant maps."""
    rng = np.random.default_rng(seed)
    x = rng.normal(0, 1, (n, H, W)).astype(np.float32)
    x[0] = 0.0                                            # a whole map ties
    x[0, ::2, 1::2] = -0.0                                # ... with -0.0 behind +0.0
    if n > 1:
        x[1] = -0.0
        x[1, 1::2, 1::2] = 0.0                            # +0.0 last in its window: still a tie, the first wins
    for k, (dy, dx) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):   # the maximum twice: at position k and at another one
        sel = (np.arange(H // 2)[:, None] + np.arange(W // 2)[None, :]) % 4 == k
        x[-1, dy:2 * (H // 2):2, dx:2 * (W // 2):2][sel] = 5.0
        x[-1, 1 - dy:2 * (H // 2):2, dx:2 * (W // 2):2][sel] = 5.0
    return x


POOL_SHAPES = [(3, 2, 2), (5, 5, 7), (2, 3, 6), (4, 64, 64)]

"""tests/train_bn_reference.py against torch itself (CPU only): the batch-statistics forward, the closed-form gradients with
dbias = 0, the running update and the chained Adam steps against autograd through F.batch_norm(training=True),
nn.BatchNorm2d's buffers and torch.optim.Adam; against the golden file recorded from the reference's CNNBlock in train()
mode; the seeded faults, each of which the caps 8 / 4 catch on a named case; and the side condition on every case's seed."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import train_bn_reference as br
import train_conv_reference as cr
import train_reference as tr
import train_stage_reference as sr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'train_bn_parts.npz')
TOL = 1e-12
D = torch.float64


def _close(a, b, name, scale=None):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    scale = np.abs(b).max() if scale is None else scale
    err = np.abs(a - b).max()
    assert err <= TOL * scale, f'{name}: {err:.3g} against {TOL * scale:.3g}'


def _autograd(conv, x, dF, stats=None, momentum=br.MOMENTUM):
    """F.conv2d, F.batch_norm(training=True), leaky_relu in f64 -> (F, [dW, dbias, dgamma, dbeta], dx, running buffers)."""
    w = [torch.from_numpy(a).to(D).requires_grad_(True) for a in conv[:4]]
    rm, rv = (torch.from_numpy(a).to(D).clone() for a in (conv[4:6] if stats is None else stats))
    xt = x.clone().requires_grad_(True)
    z = F.conv2d(xt, w[0], w[1], padding=1)
    out = F.leaky_relu(F.batch_norm(z, rm, rv, w[2], w[3], True, momentum, br.BN_EPS), br.SLOPE)
    out.backward(dF)
    return out.detach(), [a.grad for a in w], xt.grad, (rm, rv)


@pytest.mark.parametrize('name', list(br.BLOCK_CASES))
def test_closed_form_is_autograd_through_batch_norm(name):
    """F, dW, dgamma, dbeta, dx to 1e-12 of the tensor's largest value; autograd's dbias is below 1e-12 of sum |dz|: it is
    rounding noise around the exact 0 the restatement defines."""
    conv, head, shape, table, tgt, batches, lrs, _ = br.block_case(name)
    Co = conv[0].shape[0]
    x = br._t(table[batches[0]], D).reshape(-1, *shape)
    dF = torch.from_numpy(np.random.default_rng(1).normal(0, 1, (len(x), Co, *shape[1:])))
    w = [br._t(a, D) for a in conv]
    fwd = br.bn_forward(w[:4], (w[4], w[5]), x)
    grads, dz = br.bn_gradients(w[:4], x, fwd, dF)
    dx = br.bn_input_grad(w[:4], dz)
    a_F, a_grads, a_dx, (rm, rv) = _autograd(conv, x, dF)
    # dW, dx are sums of dz, which is what is left of dy after two projections: the scale of their rounding is dy's
    fold = float((w[2].abs() * fwd['inv_sigma']).max())
    s_dz = fold * float(dF.abs().max())
    _close(fwd['F'], a_F, 'F')
    _close(grads[2], a_grads[2], 'dgamma', float((dF.abs() * fwd['zhat'].abs()).sum((0, 2, 3)).max()))
    _close(grads[3], a_grads[3], 'dbeta', float(dF.abs().sum((0, 2, 3)).max()))
    _close(grads[0], a_grads[0], 'dW', s_dz * float(x.abs().sum((0, 2, 3)).max()) * 2)
    _close(dx, a_dx, 'dx', s_dz * float(w[0].abs().sum((0, 2, 3)).max()) * 2)
    _close(fwd['stats'][0], rm, 'running_mean')
    _close(fwd['stats'][1], rv, 'running_var')
    assert not grads[1].any()
    assert a_grads[1].abs().max() <= TOL * s_dz * fwd['n'], 'autograd\'s dbias is more than rounding noise'


def test_buffers_follow_nn_batchnorm_over_three_forwards():
    """The unbiased factor, the momentum's direction and the counter against nn.BatchNorm2d in train mode."""
    conv, head, shape, table, tgt, batches, lrs, _ = br.block_case('3x8x5x5 B=3')
    bn = torch.nn.BatchNorm2d(8, momentum=0.3).double().train()
    bn.load_state_dict({'weight': br._t(conv[2], D), 'bias': br._t(conv[3], D), 'running_mean': br._t(conv[4], D),
                        'running_var': br._t(conv[5], D), 'num_batches_tracked': torch.tensor(4)})
    blk = dict(cw=[br._t(a, D) for a in conv[:4]], stats=(br._t(conv[4], D), br._t(conv[5], D)), nbt=4)
    for idx in batches:
        x = br._t(table[idx], D).reshape(-1, *shape)
        fwd = br.forward_commit(blk, x, momentum=0.3)
        y = bn(F.conv2d(x, blk['cw'][0], blk['cw'][1], padding=1))
        _close(fwd['y'], y.detach(), 'y')
        _close(blk['stats'][0], bn.running_mean, 'running_mean')
        _close(blk['stats'][1], bn.running_var, 'running_var')
        assert blk['nbt'] == int(bn.num_batches_tracked)
    assert blk['nbt'] == 7
    with pytest.raises(ValueError):
        br.bn_forward(blk['cw'], blk['stats'], x[:1, :, :1, :1])
    with pytest.raises(ValueError):                                     # torch refuses one value per channel too
        bn(torch.zeros(1, 8, 1, 1, dtype=D))


def test_three_chained_steps_follow_torch_adam():
    """Three joint steps in f64 against autograd and torch.optim.Adam(weight_decay) on all ten tensors, conv.bias's gradient
    set to the 0 it is by definition (autograd's noise would move it by lr)."""
    conv, head, shape, table, tgt, batches, lrs, _ = br.block_case('5x41x10x10 B=3')
    _, outs, snaps = br.ref_steps(conv, head, shape, table, tgt, batches, br.LAM, [br.LR] * 3, br.WD)
    cw = [br._t(a, D).requires_grad_(True) for a in conv[:4]]
    hw = [br._t(a, D).requires_grad_(True) for a in head]
    rm, rv = br._t(conv[4], D).clone(), br._t(conv[5], D).clone()
    opt = torch.optim.Adam(cw + hw, lr=br.LR, weight_decay=br.WD)
    for s, idx in enumerate(batches):
        x = br._t(table[idx], D).reshape(-1, *shape)
        z = F.conv2d(x, cw[0], cw[1], padding=1)
        feats = F.leaky_relu(F.batch_norm(z, rm, rv, cw[2], cw[3], True, br.MOMENTUM, br.BN_EPS), br.SLOPE).reshape(len(idx), -1)
        y = torch.sigmoid(torch.sigmoid(feats @ hw[0].T + hw[1]) @ hw[2].T + hw[3]) @ hw[4].T + hw[5]
        comps, _ = tr.loss(y, br._t(tgt[idx], D), br.LAM)
        opt.zero_grad()
        comps[3].backward()
        cw[1].grad.zero_()
        opt.step()
        for got, want, name in zip(snaps[s]['cw'] + snaps[s]['w'], cw + hw, cr.CONV_TENSORS + tr.TENSORS):
            assert np.abs(got - want.detach().numpy()).max() <= 1e-9 * br.LR, (s, name)
        _close(snaps[s]['stats'][0], rm, 'running_mean')
        _close(snaps[s]['stats'][1], rv, 'running_var')
        assert snaps[s]['nbt'] == s + 1


def test_golden_cnnblock_in_train_mode():
    g = np.load(GOLDEN)
    w = [torch.from_numpy(g[k]) for k in ('conv_weight', 'conv_bias', 'batchnorm_weight', 'batchnorm_bias')]
    blk = dict(cw=w, stats=(torch.from_numpy(g['batchnorm_running_mean']), torch.from_numpy(g['batchnorm_running_var'])), nbt=7)
    assert float(g['momentum']) == br.MOMENTUM and float(g['eps']) == br.BN_EPS
    x, dF = torch.from_numpy(g['x']), torch.from_numpy(g['dF'])
    fwd = br.forward_commit(blk, x)
    grads, dz = br.bn_gradients(w, x, fwd, dF)
    s_dz = float((w[2].abs() * fwd['inv_sigma']).max() * dF.abs().max())
    _close(fwd['F'], g['F'], 'F')
    _close(grads[0], g['grad_conv_weight'], 'dW', s_dz * float(x.abs().sum((0, 2, 3)).max()) * 2)
    _close(grads[2], g['grad_batchnorm_weight'], 'dgamma', float((dF.abs() * fwd['zhat'].abs()).sum((0, 2, 3)).max()))
    _close(grads[3], g['grad_batchnorm_bias'], 'dbeta', float(dF.abs().sum((0, 2, 3)).max()))
    _close(br.bn_input_grad(w, dz), g['grad_x'], 'dx', s_dz * float(w[0].abs().sum((0, 2, 3)).max()) * 2)
    assert not grads[1].any() and np.abs(g['grad_conv_bias']).max() <= TOL * s_dz * fwd['n']
    _close(blk['stats'][0], g['running_mean_1'], 'running_mean after one forward')
    _close(blk['stats'][1], g['running_var_1'], 'running_var after one forward')
    assert blk['nbt'] == int(g['num_batches_tracked_1']) == 8
    br.forward_commit(blk, torch.from_numpy(g['x2']))
    _close(blk['stats'][0], g['running_mean_2'], 'running_mean after two forwards')
    _close(blk['stats'][1], g['running_var_2'], 'running_var after two forwards')
    assert blk['nbt'] == int(g['num_batches_tracked_2']) == 9


# ------------------------------------------------------------------------------------------------ seeded faults
def _worst(name, fault, quantities):
    """The f32 restatement with `fault` judged as the GPU is: -> the failures the caps 8 / 4 collect."""
    conv, head, shape, table, tgt, batches, lrs, judged = br.block_case(name)
    _, outs, snaps = br.yard_steps(conv, head, shape, table, tgt, batches, br.LAM, lrs, br.WD, fault=fault, eps=br.EPS)
    failures = []
    br.judge_restarted(outs, snaps, (conv, head, shape, table, tgt, batches, br.LAM, lrs, br.WD), (0,), name, eps=br.EPS,
                       bound=(tr.CAP_MAX, tr.CAP_RMS), collect=failures)
    return [f for f in failures if any(f.startswith(q + ' @') for q in quantities)]


@pytest.mark.parametrize('fault, name, quantities', [
    ('rv_biased', '3x8x5x5 B=3', ('running_var',)),
    ('fwd_unbiased', '3x8x5x5 B=3', ('F',)),
    ('momentum_swapped', '3x8x5x5 B=3', ('running_mean', 'running_var')),
    ('dz_eval', '5x41x10x10 B=33', ('dx', 'update conv.weight')),
    ('dgamma_no_n', '5x41x10x10 B=33', ('dx', 'update conv.weight')),
    ('one_pass', 'offset', ('batch var', 'F')),
])
def test_seeded_faults_exceed_the_caps(fault, name, quantities):
    assert fault in br.FAULTS
    assert not _worst(name, None, quantities), 'the unfaulted yardstick fails its own judgement'
    caught = _worst(name, fault, quantities)
    print('\n'.join(caught))
    assert len(caught) == len(quantities), (fault, caught)


def test_statistics_move_in_forward_not_in_step():
    """A forward without a step: the statistics and the count have moved. The fault that moves them in the step differs
    exactly: nothing has moved."""
    conv, head, shape, table, tgt, batches, lrs, _ = br.block_case('3x8x5x5 B=3')
    x = br._t(table[batches[0]], D).reshape(-1, *shape)
    new = lambda: dict(cw=[br._t(a, D) for a in conv[:4]], stats=(br._t(conv[4], D), br._t(conv[5], D)), nbt=0)
    good, bad = new(), new()
    br.forward_commit(good, x)
    br.forward_commit(bad, x, fault='stats_in_step')
    assert good['nbt'] == 1 and (good['stats'][0] != br._t(conv[4], D)).all() and (good['stats'][1] != br._t(conv[5], D)).all()
    assert bad['nbt'] == 0 and torch.equal(bad['stats'][0], br._t(conv[4], D)) and torch.equal(bad['stats'][1], br._t(conv[5], D))


# ------------------------------------------------------------------------------------------------ the side condition
@pytest.mark.parametrize('name', list(br.BLOCK_CASES))
def test_no_y_of_a_block_case_lies_within_the_margin_of_zero(name):
    conv, head, shape, table, tgt, batches, lrs, _ = br.block_case(name)
    _, outs, _ = br.ref_steps(conv, head, shape, table, tgt, batches, br.LAM, lrs, br.WD, eps=br.EPS)
    assert [int(o['near_zero']) for o in outs] == [0] * len(batches)
    if name == 'constant':                                              # the deliberate exception: y == 0 exactly
        x = br._t(table[batches[0]], D).reshape(-1, *shape)
        fwd = br.bn_forward([br._t(a, D) for a in conv[:4]], (br._t(conv[4], D), br._t(conv[5], D)), x)
        assert not fwd['y'][:, 0].any() and fwd['y'][:, 1:].all() and float(fwd['mu'][0]) == 0.5 and float(fwd['var'][0]) == 0


@pytest.mark.parametrize('B, depth', [(3, 3), (33, 3), (3, 2)])
def test_no_y_of_a_stage_case_lies_within_the_margin_of_zero(B, depth):
    convs, head, shape, table, tgt, batches, lrs = br.stage_case(B)
    state, outs, snaps = br.run_stage_steps(convs, head, shape, table, tgt, batches, br.LAM, lrs, br.WD, D, depth=depth,
                                            eps=br.EPS)
    assert [int(o['near_zero']) for o in outs] == [0] * len(batches)
    assert [snaps[-1][n]['nbt'] for n in sr.BLOCKS] == [3 if i >= 3 - depth else 0 for i in range(3)]
    if depth == 2:                                                      # the forward-only block keeps what it had
        assert all(np.array_equal(a, b) for a, b in zip(snaps[-1]['b5']['cw'] + snaps[-1]['b5']['stats'], convs[0]))

"""The conv-block trainer's reference (tests/train_conv_reference.py) against torch autograd, torch.optim.Adam and arrays
recorded from the reference implementation's CNNBlock (tests/golden/train_conv_parts.npz); the judge against seeded
faults; the argument checks of the new entry points that need no GPU. No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import train_conv_reference as cr
import train_reference as tr
from axtrack_amd import _lib

LAM = (49.5, 1.0, 49.5)
AXT_EINVAL = -22
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _case(Ci=3, Co=8, H=5, W=5, n=9, seed=3, head=(72, 40)):
    conv = cr.synth_block(Ci, Co, seed, scale=2.0)
    head_w = tr.synth_head(Co * H * W, *head, seed=seed + 1, scale=3.0)
    table, tgt = cr.synth_inputs(n, Ci, H, W, seed + 2)
    return conv, head_w, (Ci, H, W), table, tgt


def _torch_joint_loss(params, stats, x, target):
    """The joint forward pass and the summed loss through torch's own conv2d / batch_norm / leaky_relu -> (loss, feats)."""
    z = F.conv2d(x, params[0], params[1], padding=1)
    y = F.batch_norm(z, stats[0], stats[1], params[2], params[3], training=False, eps=cr.BN_EPS)
    feats = F.leaky_relu(y, cr.SLOPE).reshape(x.shape[0], -1)
    feats.retain_grad()
    a1 = torch.sigmoid(feats @ params[4].T + params[5])
    a2 = torch.sigmoid(a1 @ params[6].T + params[7])
    yo = (a2 @ params[8].T + params[9]).reshape(-1, 12, 12, 3)
    obj = target[..., 0:1]
    total = (LAM[1] * ((yo[..., 0:1] * (1 - obj)) ** 2).sum() + LAM[0] * ((yo[..., 0:1] * obj - obj) ** 2).sum()
             + LAM[2] * ((yo[..., 1:3] * obj - target[..., 1:3]) ** 2).sum()) / x.shape[0]
    return total, feats


def test_ref_gradients_equal_autograd_in_f64():
    conv, head_w, shape, table, tgt = _case()
    state = cr.new_state(conv, head_w, torch.float64)
    x = torch.from_numpy(table[:6]).double().reshape(6, *shape)
    T = torch.from_numpy(tgt[:6]).double()
    params = [p.clone().requires_grad_(True) for p in state['cw'] + state['head']['w']]
    total, feats = _torch_joint_loss(params, state['stats'], x, T)
    total.backward()
    fwd = cr.block_forward(state['cw'], state['stats'], x)
    assert np.abs(fwd['F'].reshape(6, -1).numpy() - feats.detach().numpy()).max() <= 1e-12
    a1, a2, y = tr.forward(state['head'], fwd['F'].reshape(6, -1))
    _, dy = tr.loss(y, T, LAM)
    hw = state['head']['w']
    dz1 = (((dy @ hw[4]) * a2 * (1 - a2)) @ hw[2]) * a1 * (1 - a1)
    dfeat = dz1 @ hw[0]
    assert np.abs(dfeat.numpy() - feats.grad.numpy()).max() <= 1e-12 * max(1.0, np.abs(feats.grad.numpy()).max())
    for name, g, p in zip(cr.CONV_TENSORS, cr.block_gradients(state['cw'], x, fwd, dfeat.reshape(fwd['F'].shape)), params):
        assert np.abs(p.grad.numpy()).max() > 1e-3, name
        assert np.abs(g.numpy() - p.grad.numpy()).max() <= 1e-12 * max(1.0, np.abs(p.grad.numpy()).max()), name


def test_five_ref_joint_steps_equal_torch_optim_adam():
    conv, head_w, shape, table, tgt = _case()
    lr, wd = 1e-2, 0.05
    batches = [[0, 1, 2, 3, 4, 5], [5, 3, 3, 8], [7], [2, 0, 6, 1, 4], [8, 7, 6]]
    state, _, snaps = cr.ref_steps(conv, head_w, shape, table, tgt, batches, LAM, [lr] * 5, wd)
    X = torch.from_numpy(table).double().reshape(len(table), *shape)
    T = torch.from_numpy(tgt).double()
    params = [torch.from_numpy(a).double().requires_grad_(True) for a in conv[:4] + head_w]
    opt = torch.optim.Adam(params, lr=lr, weight_decay=wd)
    for idx in batches:
        total, _ = _torch_joint_loss(params, state['stats'], X[idx], T[idx])
        opt.zero_grad()
        total.backward()
        opt.step()
    mine = snaps[-1]['cw'] + snaps[-1]['w']
    for name, a, theirs, start in zip(cr.CONV_TENSORS + tr.TENSORS, mine, params, conv[:4] + head_w):
        assert np.abs(theirs.detach().numpy() - start).max() > 1e-3, name
        assert np.abs(a - theirs.detach().numpy()).max() <= 1e-12 * max(1.0, np.abs(a).max()), name


def test_ref_block_reproduces_the_reference_block(golden):
    """Forward and the autograd gradients of the reference's own CNNBlock in eval mode, (Ci,Co,H,W,B) = (3,8,5,5,3)."""
    g = golden('train_conv_parts')
    w = [torch.from_numpy(g[k]) for k in ('conv_weight', 'conv_bias', 'batchnorm_weight', 'batchnorm_bias')]
    stats = (torch.from_numpy(g['batchnorm_running_mean']), torch.from_numpy(g['batchnorm_running_var']))
    x, dF = torch.from_numpy(g['x']), torch.from_numpy(g['dF'])
    assert tuple(x.shape) == (3, 3, 5, 5) and tuple(dF.shape) == (3, 8, 5, 5) and (g['batchnorm_weight'] < 0).any()
    fwd = cr.block_forward(w, stats, x)
    assert np.abs(fwd['F'].numpy() - g['F']).max() <= 1e-12 * np.abs(g['F']).max()
    assert (g['F'] < 0).any() and (g['F'] > 0).any()
    grads = cr.block_gradients(w, x, fwd, dF)
    for got, key in zip(grads, ('grad_conv_weight', 'grad_conv_bias', 'grad_batchnorm_weight', 'grad_batchnorm_bias')):
        assert np.abs(got.numpy() - g[key]).max() <= 1e-12 * max(1.0, np.abs(g[key]).max()), key


# ------------------------------------------------------------------------------------------------ seeded faults
CAPS = (tr.CAP_MAX, tr.CAP_RMS)
BATCHES = [[0, 1, 2, 3, 4, 5], [8, 7, 7, 2], [4], [1, 0, 3], [6, 5, 2, 2, 8]]


@pytest.fixture(scope='module')
def fault_cases():
    """name -> (args of run_steps, f64 reference, f32 yardstick). plain: random input on 5 x 5 maps. border_ring: the input
    is non-zero on the outermost ring only. y_zero: output channel 0 sits at y == 0 exactly."""
    conv, head_w, shape, table, tgt = _case(seed=9)
    inputs = dict(plain=(conv, table), border_ring=(conv, cr.border_ring(table, *shape)), y_zero=(cr.y_zero_block(conv), table))
    out = {}
    for name, (c, t) in inputs.items():
        args = (c, head_w, shape, t, tgt, BATCHES, LAM, [1e-2] * 5, 0.05)
        out[name] = (args, cr.ref_steps(*args), cr.yard_steps(*args))
    return out


@pytest.mark.parametrize('case', ['plain', 'border_ring', 'y_zero'])
def test_judge_accepts_a_correct_f32_joint_step_in_another_order(fault_cases, case):
    """An f32 implementation that sums in another order (the batch reversed) stays within the caps on every named case."""
    args, ref, yard = fault_cases[case]
    conv, head_w, shape, table, tgt, batches, lam, lrs, wd = args
    _, outs, snaps = cr.yard_steps(conv, head_w, shape, table, tgt, [b[::-1] for b in batches], lam, lrs, wd)
    for o in outs:
        for q in ('F', 'dfeat'):
            o[q] = o[q][::-1]
    cr.judge_run(outs, snaps, ref, yard, conv, head_w, (0, 4), case, bound=CAPS)


@pytest.mark.parametrize('fault,case', [('slope_side', 'y_zero'), ('no_fold', 'plain'), ('swap_k', 'plain'), ('wrap', 'border_ring'),
                                        ('no_bn_wd', 'plain'), ('post_update_df', 'plain')])
def test_judge_rejects_seeded_faults_on_their_named_case(fault_cases, fault, case):
    assert fault in cr.FAULTS
    args, ref, yard = fault_cases[case]
    _, outs, snaps = cr.yard_steps(*args, fault=fault)
    with pytest.raises(tr.TrainMismatch):                       # even at the caps
        cr.judge_run(outs, snaps, ref, yard, args[0], args[1], (0, 4), case, bound=CAPS)


def test_restarted_judgement_accepts_another_order_and_rejects_a_fault(fault_cases):
    """judge_restarted, what the GPU tests use: step 5 of a run against one reference step from that run's own state after
    step 4. A correct f32 run that sums in another order passes at the default bounds of every quantity (no chaining is
    left to part the runs); the same run with `dz` without gamma / sigma in its fifth step alone fails even at the caps."""
    args, _, _ = fault_cases['plain']
    conv, head_w, shape, table, tgt, batches, lam, lrs, wd = args
    rev = [b[::-1] for b in batches]
    _, outs, snaps = cr.yard_steps(conv, head_w, shape, table, tgt, rev, lam, lrs, wd)
    for o in outs:
        for q in ('F', 'dfeat'):
            o[q] = o[q][::-1]
    cr.judge_restarted(outs, snaps, args, (0, 4), 'another order')
    _, bad_o, bad_s = cr.yard_steps(conv, head_w, shape, table, tgt, batches[4:], lam, lrs[4:], wd, fault='no_fold',
                                    start=(snaps[3], 4))
    with pytest.raises(tr.TrainMismatch):
        cr.judge_restarted(outs[:4] + bad_o, snaps[:4] + bad_s, args, (4,), 'fault in step 5', bound=CAPS)


def test_y_zero_case_holds_exact_zeros():
    conv, head_w, shape, table, tgt = _case(seed=9)
    state = cr.new_state(cr.y_zero_block(conv), head_w, torch.float32)
    fwd = cr.block_forward(state['cw'], state['stats'], torch.from_numpy(table).reshape(len(table), *shape))
    assert (fwd['y'][:, 0] == 0).all() and (fwd['y'][:, 1:] != 0).all()


# ------------------------------------------------------------------------------------------------ the library, without a GPU
def test_header_symbols_are_exported_and_bound():
    header = open(os.path.join(ROOT, 'include', 'axtrack_hip.h')).read()
    names = set(re.findall(r'\b(axt_conv_trainer_\w+|axt_head_trainer_input_grad|axt_cnn_block_features_frames)\s*\(', header))
    assert names == {'axt_conv_trainer_create', 'axt_conv_trainer_destroy', 'axt_conv_trainer_device_bytes',
                     'axt_conv_trainer_read_weights', 'axt_conv_trainer_read_moments', 'axt_conv_trainer_forward',
                     'axt_conv_trainer_step', 'axt_head_trainer_input_grad', 'axt_cnn_block_features_frames'}
    lib = _lib.load()
    assert lib.axt_abi_version() == 1
    for n in names:
        assert n in _lib.SIGNATURES and hasattr(lib, n), n


def test_new_entry_points_refuse_bad_arguments_before_any_device_call():
    lib = _lib.load()
    Ci, Co, H, W = 2, 3, 1, 6
    arrs = [np.zeros(s, np.float32) for s in ((Co, Ci, 3, 3), (Co,), (Co,), (Co,), (Co,), (Co,))]
    ptrs = [a.ctypes.data for a in arrs]
    handle = ctypes.c_void_p()

    def create(Ci=Ci, Co=Co, H=H, W=W, ptrs=ptrs, max_batch=4, out=ctypes.byref(handle)):
        return lib.axt_conv_trainer_create(Ci, Co, H, W, *ptrs, max_batch, out)

    bad = [dict(Ci=0), dict(Ci=513), dict(Co=0), dict(Co=513), dict(H=0), dict(H=65), dict(W=0), dict(W=65), dict(max_batch=0),
           dict(max_batch=65), dict(out=None)] + [dict(ptrs=ptrs[:i] + [None] + ptrs[i + 1:]) for i in range(6)]
    for kw in bad:
        assert create(**kw) == AXT_EINVAL, kw
        assert not handle.value
        assert (b'null argument' if 'ptrs' in kw or 'out' in kw else b'axt_conv_trainer_create') in lib.axt_last_error()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    assert lib.axt_conv_trainer_forward(None, p, None, 1, p, None) == AXT_EINVAL
    assert lib.axt_conv_trainer_step(None, p, None, 1, p, 1e-3, 0.9, 0.999, 1e-8, 0.0, None) == AXT_EINVAL
    assert lib.axt_conv_trainer_read_weights(None, p, p, p, p) == AXT_EINVAL
    assert lib.axt_conv_trainer_read_moments(None, 0, p, p, None) == AXT_EINVAL
    assert lib.axt_conv_trainer_device_bytes(None) == 0
    lib.axt_conv_trainer_destroy(None)
    assert lib.axt_head_trainer_input_grad(None, p, 1, p, None) == AXT_EINVAL
    tiles = np.zeros(2, np.int32)
    for block in (-1, 0, 5, 8):
        assert lib.axt_cnn_block_features_frames(None, p, 5, 512, 512, 0, 1, tiles.ctypes.data, 1, block, p, None) == AXT_EINVAL
        assert b'block' in lib.axt_last_error()
    for block in (6, 7):                                                    # a null detector is refused as well
        assert lib.axt_cnn_block_features_frames(None, p, 5, 512, 512, 0, 1, tiles.ctypes.data, 1, block, p, None) == AXT_EINVAL


def test_fine_tune_head_keeps_its_signature_and_gains_the_option():
    import inspect
    from axtrack_amd import training
    sig = inspect.signature(training.fine_tune_head)
    assert sig.parameters['train_last_conv'].default is False
    assert list(sig.parameters)[-1] == 'train_last_conv'
    assert inspect.signature(training.ConvBlockTrainer).parameters['block_key'].default == 'ConvNet.ConvBlock_10'

"""The stage trainer's reference (tests/train_stage_reference.py) against torch autograd through torch's own conv2d, eval
batch_norm, leaky_relu and max_pool2d, against torch.optim.Adam, and its pool against torch's CPU max_pool2d bit for bit;
the judge against seeded faults; what the new entry points and fine_tune_head(train_conv_blocks=) refuse without a GPU.
No GPU."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import train_conv_reference as cr
import train_reference as tr
import train_stage_reference as sr
from axtrack_amd import _lib

LAM = (49.5, 1.0, 49.5)
AXT_EINVAL = -22
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAPS = (tr.CAP_MAX, tr.CAP_RMS)
BATCHES = [[0, 1, 2, 3, 4, 5], [8, 7, 7, 2], [4]]


@pytest.fixture(scope='module')
def cases():
    out = {name: sr.synth_stage(dims, heads, seed=11 + i, n=9) for i, (name, (dims, heads)) in enumerate(sr.CASES.items())}
    convs, head, shape, table, tgt = out['unequal']
    out['tied'] = (convs, head, shape, sr.tied_table(table), tgt)
    return out


def _torch_stage(params, stats, x, target):
    """The chained forward and the summed loss through torch's own operators -> (loss, [F5, F6, pooled, F7])."""
    h, keep = x, []
    for i in range(3):
        p = params[4 * i:4 * i + 4]
        z = F.conv2d(h, p[0], p[1], padding=1)
        y = F.batch_norm(z, stats[i][0], stats[i][1], p[2], p[3], training=False, eps=cr.BN_EPS)
        h = F.leaky_relu(y, cr.SLOPE)
        keep.append(h)
        if i == 1:
            h = F.max_pool2d(h, 2, 2)
            keep.append(h)
    for k in keep:
        k.retain_grad()
    feats = h.reshape(x.shape[0], -1)
    hp = params[12:]
    a1 = torch.sigmoid(feats @ hp[0].T + hp[1])
    a2 = torch.sigmoid(a1 @ hp[2].T + hp[3])
    yo = (a2 @ hp[4].T + hp[5]).reshape(-1, 12, 12, 3)
    obj = target[..., 0:1]
    total = (LAM[1] * ((yo[..., 0:1] * (1 - obj)) ** 2).sum() + LAM[0] * ((yo[..., 0:1] * obj - obj) ** 2).sum()
             + LAM[2] * ((yo[..., 1:3] * obj - target[..., 1:3]) ** 2).sum()) / x.shape[0]
    return total, keep


def _close(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape, what
    assert np.abs(a - b).max() <= 1e-12 * max(1.0, np.abs(b).max()), what


@pytest.mark.parametrize('case', ['unequal', 'square_odd', 'one_row', 'tied'])
def test_ref_chain_equals_autograd_in_f64(cases, case):
    """Forward, the three gradients handed back through the stage, and the four parameter gradients of each block."""
    convs, head, shape, table, tgt = cases[case]
    state = sr.new_state(convs, head, torch.float64)
    B = 6
    x = torch.from_numpy(table[:B]).double().reshape(B, *shape)
    T = torch.from_numpy(tgt[:B]).double()
    params = [p.clone().requires_grad_(True) for n in sr.BLOCKS for p in state[n]['cw']] + \
             [p.clone().requires_grad_(True) for p in state['head']['w']]
    total, keep = _torch_stage(params, [state[n]['stats'] for n in sr.BLOCKS], x, T)
    total.backward()
    (f5, f6, f7), win, pooled = sr.stage_forward(state, x)
    for mine, theirs, name in zip((f5['F'], f6['F'], pooled, f7['F']), keep, ('F5', 'F6', 'pooled', 'F7')):
        _close(mine.numpy(), theirs.detach().numpy(), name)
    dfeat = keep[3].grad
    dpooled = sr.block_input_grad(state['b7']['cw'], f7, dfeat)
    _close(dpooled, keep[2].grad, 'dpooled')
    dF6 = sr.pool_backward(f6['F'], dpooled)
    assert np.array_equal(sr.pool_backward(f6['F'], keep[2].grad).numpy(), keep[1].grad.numpy())      # the pool is exact
    _close(dF6, keep[1].grad, 'dF6')
    dx6 = sr.block_input_grad(state['b6']['cw'], f6, dF6)
    _close(dx6, keep[0].grad, 'dx6')
    assert min(np.abs(g.numpy()).max() for g in (dpooled, dF6, dx6)) > 1e-6
    for i, (name, inp, fwd, dF) in enumerate((('b5', x, f5, dx6), ('b6', f5['F'], f6, dF6), ('b7', pooled, f7, dfeat))):
        for tname, g, p in zip(cr.CONV_TENSORS, cr.block_gradients(state[name]['cw'], inp, fwd, dF), params[4 * i:4 * i + 4]):
            _close(g, p.grad, f'{name} {tname}')
    if case == 'square_odd':                              # row 4 and column 6 lie outside every window
        g = dF6.numpy()
        assert not g[:, :, 4].any() and not g[:, :, :, 6].any() and g[:, :, :4, :6].any()
    if case == 'tied':
        # Zero and constant rows: F5 is one constant per channel away from the border (zero rows: everywhere), so F6 is
        # one wherever no tap of either block reaches the zero padding. On 6 x 6 maps that is the window of pixels
        # (2..3, 2..3): its four values are equal, and its gradient sits at (2, 2). The windows along the border see the
        # padding and do not tie.
        v = f6['F'].numpy()[:, :, 2:4, 2:4].reshape(B, -1, 4)
        assert (v == v[..., :1]).all()
        g = dF6.numpy()[:, :, 2:4, 2:4]
        assert (g[:, :, 0, 0] != 0).all() and not g[:, :, 0, 1].any() and not g[:, :, 1].any()


@pytest.mark.parametrize('depth', [2, 3])
def test_three_ref_steps_equal_torch_optim_adam(cases, depth):
    convs, head, shape, table, tgt = cases['square_odd']
    lr, wd = 1e-2, 0.05
    state, _, snaps = sr.ref_steps(convs, head, shape, table, tgt, BATCHES, LAM, [lr] * 3, wd, depth=depth)
    X = torch.from_numpy(table).double().reshape(len(table), *shape)
    T = torch.from_numpy(tgt).double()
    params = [torch.from_numpy(a).double().requires_grad_(True) for c in convs for a in c[:4]] + \
             [torch.from_numpy(a).double().requires_grad_(True) for a in head]
    opt = torch.optim.Adam(params[4 * (3 - depth):], lr=lr, weight_decay=wd)
    for idx in BATCHES:
        total, _ = _torch_stage(params, [state[n]['stats'] for n in sr.BLOCKS], X[idx], T[idx])
        opt.zero_grad()
        total.backward()
        opt.step()
    mine = [a for n in sr.BLOCKS for a in snaps[-1][n]['cw']] + snaps[-1]['w']
    start = [a for c in convs for a in c[:4]] + list(head)
    for i, (a, theirs, w0) in enumerate(zip(mine, params, start)):
        if i < 4 * (3 - depth):
            assert np.array_equal(a, w0.astype(np.float64)), i         # a forward-only block keeps its tensors
        else:
            assert np.abs(theirs.detach().numpy() - w0).max() > 1e-3, i
        _close(a, theirs.detach().numpy(), i)


# ------------------------------------------------------------------------------------------------ the pool
@pytest.mark.parametrize('shape', sr.POOL_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_ref_pool_is_torchs_cpu_pool_bit_for_bit(shape):
    n, H, W = shape
    x = torch.from_numpy(sr.pool_input(n, H, W, seed=H * W))[None].clone().requires_grad_(True)
    out = F.max_pool2d(x, 2, 2)
    dout = torch.from_numpy(np.random.default_rng(1).normal(0, 1, tuple(out.shape)).astype(np.float32))
    out.backward(dout)
    mine = sr.pool_forward(x.detach())
    assert mine.numpy().tobytes() == out.detach().numpy().tobytes()
    assert sr.pool_backward(x.detach(), dout).numpy().tobytes() == x.grad.numpy().tobytes()


@pytest.mark.parametrize('fault', ['pool_last', 'pool_all_ties', 'pool_odd_row'])
def test_pool_faults_differ_exactly(fault):
    assert fault in sr.FAULTS
    x = torch.from_numpy(sr.pool_input(5, 5, 7, seed=35))[None]
    dout = torch.from_numpy(np.random.default_rng(1).normal(0, 1, (1, 5, 2, 3)).astype(np.float32))
    good, bad = sr.pool_backward(x, dout), sr.pool_backward(x, dout, fault=fault)
    assert not np.array_equal(good.numpy(), bad.numpy())
    if fault == 'pool_odd_row':
        assert np.array_equal(good.numpy()[:, :, :4], bad.numpy()[:, :, :4]) and bad.numpy()[:, :, 4].any()


# ------------------------------------------------------------------------------------------------ the judge
def _reversed_run(args, depth=3):
    convs, head, shape, table, tgt, batches, lam, lrs, wd = args
    _, outs, snaps = sr.yard_steps(convs, head, shape, table, tgt, [b[::-1] for b in batches], lam, lrs, wd, depth=depth)
    for o in outs:
        for q in sr.QUANTITIES:
            if q in o:
                o[q] = o[q][::-1].copy()
    return outs, snaps


@pytest.mark.parametrize('case', ['unequal', 'square_odd', 'one_row', 'tied'])
def test_judge_accepts_a_correct_f32_step_in_another_order(cases, case):
    """An f32 run that sums in another order (the batch reversed) passes the restarted judgement at the caps."""
    args = (*cases[case], BATCHES, LAM, [1e-2] * 3, 0.05)
    outs, snaps = _reversed_run(args)
    sr.judge_restarted(outs, snaps, args, (0, 2), label=case, bound=CAPS)


@pytest.mark.parametrize('fault,case', [('no_flip', 'unequal'), ('transposed', 'square_odd'), ('no_slope', 'unequal'),
                                        ('post_update_dx', 'unequal')])
def test_judge_rejects_seeded_faults_on_their_named_case(cases, fault, case):
    """Each fault of the data gradient exceeds the caps 8 / 4, in the step it is made in."""
    assert fault in sr.FAULTS
    args = (*cases[case], BATCHES, LAM, [1e-2] * 3, 0.05)
    _, outs, snaps = sr.yard_steps(*args, fault=fault)
    failures = []
    sr.judge_restarted(outs, snaps, args, (0,), label=case, bound=CAPS, collect=failures)
    assert any(f.startswith(('dx6', 'dpooled')) for f in failures), failures[:3]
    with pytest.raises(tr.TrainMismatch):
        sr.judge_restarted(outs, snaps, args, (2,), label=case, bound=CAPS)


# ------------------------------------------------------------------------------------------------ the library, without a GPU
NEW = ('axt_conv_trainer_input_grad', 'axt_maxpool2_forward', 'axt_maxpool2_backward')


def test_new_symbols_are_declared_exported_and_bound():
    main = open(os.path.join(ROOT, 'include', 'axtrack_hip.h')).read()
    header = open(os.path.join(ROOT, 'include', 'axtrack_hip_stage.h')).read()
    assert re.search(r'^#include "axtrack_hip_stage.h"$', main, flags=re.M)
    lib = _lib.load()
    assert lib.axt_abi_version() == 1
    for n in NEW:
        assert re.search(r'\bint\s+' + n + r'\s*\(', header), f'{n} is not declared in include/axtrack_hip_stage.h'
        assert n in _lib.SIGNATURES and hasattr(lib, n), n


def test_new_entry_points_refuse_bad_arguments_before_any_device_call():
    lib = _lib.load()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    assert lib.axt_conv_trainer_input_grad(None, p, 1, p, None) == AXT_EINVAL
    for H, W in ((1, 2), (2, 1), (0, 4), (32769, 2), (2, 32769)):
        assert lib.axt_maxpool2_forward(p, 1, H, W, p, None) == AXT_EINVAL, (H, W)
        assert b'axt_maxpool2_forward' in lib.axt_last_error()
        assert lib.axt_maxpool2_backward(p, p, 1, H, W, p, None) == AXT_EINVAL, (H, W)
        assert b'axt_maxpool2_backward' in lib.axt_last_error()
    for n_maps in (-1, (1 << 38) // 4 + 1):
        assert lib.axt_maxpool2_forward(p, n_maps, 2, 2, p, None) == AXT_EINVAL
        assert lib.axt_maxpool2_backward(p, p, n_maps, 2, 2, p, None) == AXT_EINVAL
    assert lib.axt_maxpool2_forward(None, 1, 2, 2, p, None) == AXT_EINVAL
    assert lib.axt_maxpool2_forward(p, 1, 2, 2, None, None) == AXT_EINVAL
    for args in ((None, p, p), (p, None, p), (p, p, None)):
        assert lib.axt_maxpool2_backward(args[0], args[1], 1, 2, 2, args[2], None) == AXT_EINVAL
    assert lib.axt_maxpool2_forward(p, 0, 2, 2, p, None) == 0               # no maps: nothing to do
    assert lib.axt_maxpool2_backward(p, p, 0, 2, 2, p, None) == 0
    tiles = np.zeros(2, np.int32)
    assert lib.axt_cnn_block_features_frames(None, p, 5, 512, 512, 0, 1, tiles.ctypes.data, 1, 4, p, None) == AXT_EINVAL
    assert b'block' not in lib.axt_last_error()                             # block 4 is known: the null detector is refused
    assert lib.axt_cnn_block_features_frames(None, p, 5, 512, 512, 0, 1, tiles.ctypes.data, 1, 5, p, None) == AXT_EINVAL
    assert b'block' in lib.axt_last_error()


def test_block_table_and_stage_layout():
    from axtrack_amd import hotpath, training
    assert hotpath.BLOCK_FEATURES == {7: 160 * 16 * 16, 6: 80 * 16 * 16, 4: 80 * 32 * 32}
    assert [hotpath.conv_block_key(i) for i in training.STAGE_BLOCKS] == ['ConvNet.ConvBlock_7', 'ConvNet.ConvBlock_8',
                                                                            'ConvNet.ConvBlock_10']
    assert hotpath.conv_block_key(7) == training.LAST_CONV_BLOCK
    assert [hotpath.CONV_MAP_SIDE[i] for i in training.STAGE_BLOCKS] == [32, 32, 16]
    assert [hotpath.CONV_POOLED[i] for i in training.STAGE_BLOCKS] == [False, True, False]
    assert hasattr(training.ConvBlockTrainer, 'input_grad')


def test_fine_tune_head_refuses_before_any_gpu_work():
    """The depth, its clash with train_last_conv and a frame-sharded timelapse are refused before anything touches a GPU:
    this runs without one."""
    import axtrack_amd
    from axtrack_amd import training
    sig = inspect.signature(training.fine_tune_head)
    assert sig.parameters['train_conv_blocks'].default is None and sig.parameters['train_last_conv'].default is False

    class Tl:
        frame_sharded = False

        def __len__(self):
            return 1

    for depth in (-1, 4, 1.5, '3', True):
        with pytest.raises(ValueError, match='train_conv_blocks'):
            axtrack_amd.fine_tune_head(Tl(), [([1], [1])], {}, train_conv_blocks=depth)
    for depth in (0, 2, 3):
        with pytest.raises(ValueError, match='train_last_conv'):
            axtrack_amd.fine_tune_head(Tl(), [([1], [1])], {}, train_conv_blocks=depth, train_last_conv=True)
    sharded = Tl()
    sharded.frame_sharded = True
    for depth in (1, 2, 3):
        with pytest.raises(NotImplementedError):
            axtrack_amd.fine_tune_head(sharded, [([1], [1])], {}, train_conv_blocks=depth)
    with pytest.raises(ValueError, match='depth'):
        training.ConvStageTrainer({}, depth=0)

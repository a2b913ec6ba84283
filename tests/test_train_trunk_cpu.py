"""The trunk trainer's reference (tests/train_trunk_reference.py) against torch autograd in f64 through torch's own
conv2d(stride=), batch_norm, leaky_relu and max_pool2d, and against train_bn_reference at stride 1; the judge against every
seeded fault at the bounds in use; the side condition of every case the GPU file runs; the new header and bindings; what the
new entry points and fine_tune_detector refuse without a GPU. No GPU."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import train_bn_reference as bn
import train_conv_reference as cr
import train_reference as tr
import train_trunk_reference as tk
from axtrack_amd import _lib

AXT_EINVAL = -22
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(c, 2) for c in tk.BLOCK_CASES] + [(tk.WIDE_CASE, 1), ((3, 4, 6, 7, 2), 1)]


def _close(a, b, what, tol=1e-11):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    err = np.abs(a - b).max() / (np.abs(b).max() + 1e-30) if a.size else 0.0
    assert a.shape == b.shape and err < tol, f'{what}: relative difference {err:.3g}'


# ------------------------------------------------------------------------------------------------ against autograd
@pytest.mark.parametrize('batch_stats', [False, True])
@pytest.mark.parametrize('case,s', CASES, ids=lambda v: 'x'.join(map(str, v)) if isinstance(v, tuple) else f's{v}')
def test_block_gradients_are_autograds(case, s, batch_stats):
    conv, x, dF = tk.block_case(case, s)
    w = [torch.from_numpy(a).double() for a in conv]
    xt, dFt = torch.from_numpy(x).double(), torch.from_numpy(dF).double()
    fwd = tk.block_forward(w[:4], (w[4], w[5]), xt, s, batch_stats)
    grads, dz = tk.block_gradients(w[:4], xt, fwd, dFt, s, batch_stats)
    dx = tk.input_grad(w[0], dz, xt.shape[2:], s)
    p = [a.clone().requires_grad_(True) for a in w[:4]]
    xa = xt.clone().requires_grad_(True)
    z = F.conv2d(xa, p[0], p[1], stride=s, padding=1)
    assert z.shape[2:] == (tk.out_size(x.shape[2], s), tk.out_size(x.shape[3], s)) == dF.shape[2:]
    y = F.batch_norm(z, w[4].clone(), w[5].clone(), p[2], p[3], training=batch_stats, momentum=tk.MOMENTUM, eps=tk.BN_EPS)
    out = F.leaky_relu(y, tk.SLOPE)
    _close(fwd['F'], out.detach(), 'F')
    out.backward(dFt)
    _close(dx, xa.grad, 'dx', 1e-10)
    for g, q, name in zip(grads, p, cr.CONV_TENSORS):
        if batch_stats and name == 'conv.bias':
            assert not g.any() and np.abs(q.grad.numpy()).max() < 1e-9 * max(1.0, float(dFt.abs().sum()))
        else:
            _close(g, q.grad, name, 1e-10)


def test_batch_statistics_need_two_values():
    conv, x, dF = tk.block_case((2, 3, 1, 1, 2))
    w = [torch.from_numpy(a).double() for a in conv]
    tk.block_forward(w[:4], (w[4], w[5]), torch.from_numpy(x).double(), 2, True)        # B = 2 on a 1 x 1 map: n = 2
    with pytest.raises(ValueError):
        tk.block_forward(w[:4], (w[4], w[5]), torch.from_numpy(x[:1]).double(), 2, True)


@pytest.mark.parametrize('dtype', [torch.float64, torch.float32])
def test_stride_one_is_the_references_below(dtype):
    """At stride 1 the restated block is train_conv_reference's and train_bn_reference's bit for bit."""
    conv, x, dF = tk.block_case((3, 4, 6, 7, 2), 1)
    w = [torch.from_numpy(a).to(dtype) for a in conv]
    xt, dFt = torch.from_numpy(x).to(dtype), torch.from_numpy(dF).to(dtype)
    same = lambda a, b: a.numpy().tobytes() == b.numpy().tobytes()
    a, b = tk.block_forward(w[:4], (w[4], w[5]), xt), cr.block_forward(w[:4], (w[4], w[5]), xt)
    assert same(a['F'], b['F']) and all(same(u, v) for u, v in zip(tk.block_gradients(w[:4], xt, a, dFt)[0],
                                                                   cr.block_gradients(w[:4], xt, b, dFt)))
    a, b = tk.block_forward(w[:4], (w[4], w[5]), xt, 1, True), bn.bn_forward(w[:4], (w[4], w[5]), xt)
    ga, gb = tk.block_gradients(w[:4], xt, a, dFt, 1, True), bn.bn_gradients(w[:4], xt, b, dFt)
    assert same(a['F'], b['F']) and all(same(u, v) for u, v in zip(a['stats'], b['stats']))
    assert all(same(u, v) for u, v in zip(ga[0], gb[0])) and same(ga[1], gb[1])
    _close(tk.input_grad(w[0], ga[1], xt.shape[2:], 1), bn.bn_input_grad(w[:4], gb[1]), 'dx', 1e-6)


def _torch_chain(convs, spec, x, dfeat, batch_stats):
    params = [[torch.from_numpy(a).double().requires_grad_(True) for a in c[:4]] for c in convs]
    h, keep = torch.from_numpy(x).double(), []
    for p, c, (s, pooled, trained) in zip(params, convs, spec):
        z = F.conv2d(h, p[0], p[1], stride=s, padding=1)
        y = F.batch_norm(z, torch.from_numpy(c[4]).double(), torch.from_numpy(c[5]).double(), p[2], p[3],
                         training=batch_stats and trained, momentum=tk.MOMENTUM, eps=tk.BN_EPS)
        h = F.leaky_relu(y, tk.SLOPE)
        keep.append(h)
        if pooled:
            h = F.max_pool2d(h, 2, 2)
    (h.reshape(len(x), -1) * torch.from_numpy(dfeat).double()).sum().backward()
    return params, keep, h


@pytest.mark.parametrize('first,n_trained,batch_stats', [(0, 8, False), (0, 6, False), (3, 5, False), (3, 4, True), (0, 8, True)])
def test_chain_step_is_autograd_and_adam(first, n_trained, batch_stats):
    """One chained step: every trained tensor moves as torch.optim.Adam moves it from autograd's gradient through torch's own
    operators; a forward-only block keeps its tensors; the side condition holds for the case."""
    convs, spec, shape, table, batches, dfeats, lrs, wd = tk.trunk_case(first, n_trained, batch_stats)
    outs, snaps = tk.run_steps(convs, spec, shape, table, batches[:1], dfeats[:1], lrs[:1], wd, torch.float64, eps=1e-3,
                               batch_stats=batch_stats)
    assert outs[0]['near_zero'] == 0
    x = table[batches[0]].reshape(len(batches[0]), *shape)
    params, keep, h = _torch_chain(convs, spec, x, dfeats[0], batch_stats)
    _close(outs[0][f'F{len(spec) - 1}'], keep[-1].detach().reshape(len(x), -1), 'the chain\'s output')
    trained = [p for p, sp in zip(params, spec) if sp[2]]
    if batch_stats:
        for p in trained:
            p[1].grad = torch.zeros_like(p[1])                              # 0 by definition, not autograd's rounding noise
    opt = torch.optim.Adam([q for p in trained for q in p], lr=lrs[0], weight_decay=wd, eps=1e-3)
    opt.step()
    for k, (p, sp) in enumerate(zip(params, spec)):
        for i, name in enumerate(cr.CONV_TENSORS):
            if sp[2]:
                _close(snaps[0][k]['cw'][i] - convs[k][i].astype(np.float64), p[i].detach().numpy() - convs[k][i].astype(np.float64),
                       f'block {k} {name}', 1e-7)
            else:
                assert snaps[0][k]['cw'][i].tobytes() == convs[k][i].astype(np.float64).tobytes() and snaps[0][k]['t'] == 0


@pytest.mark.parametrize('depth', [1, 2, 3])
def test_chain_step_is_the_stage_references_step(depth):
    """The two references agree on the stage: chain_step on strides (1, 1, 1), pooled (F, T, F), fed the dfeat that
    train_stage_reference.stage_step forms, reproduces that step on CASES['unequal'] in f64.
    Bit for bit, where both compute a quantity the same way (test_stride_one_is_the_references_below: the forward and a
    block's parameter gradients; the pool is one function for both): F5, F6, pooled, F, and the last block's four updated
    tensors, whose gradients come from the same dfeat.
    Within tolerance, where the data gradient is an einsum over shifted maps in one and a gather per tap in the other:
    dpooled, dF6 (the pool's routing of dpooled), dx6 at test_block_gradients_are_autograds' 1e-10 for dx, and the updates
    of the blocks in front, which take those gradients, at test_chain_step_is_autograd_and_adam's 1e-7."""
    import train_stage_reference as sr
    dims, heads = sr.CASES['unequal']
    convs, head, shape, table, targets = sr.synth_stage(dims, heads, seed=100, n=40)
    idx = torch.tensor([7, 31, 7])
    X = torch.from_numpy(table).double().reshape(len(table), *shape)[idx]
    T = torch.from_numpy(targets).double().reshape(-1, tr.S, tr.S, 4)[idx]
    lr, wd, eps = 1e-2, 0.05, 1e-3
    stage = sr.new_state(convs, head, torch.float64)
    want = sr.stage_step(stage, X, T, (49.5, 1.0, 49.5), lr, wd, depth, eps=eps)
    chain = tk.new_state(convs, torch.float64)
    spec = [(1, pooled, k >= 3 - depth) for k, pooled in enumerate((False, True, False))]
    got = tk.chain_step(chain, spec, X, want['dfeat'], lr, wd, eps=eps)
    same = lambda a, b: a.shape == b.shape and a.numpy().tobytes() == b.numpy().tobytes()
    for mine, theirs in (('F0', 'F5'), ('F1', 'F6'), ('P1', 'pooled'), ('F2', 'F')):
        assert same(got[mine], want[theirs]) and want[theirs].abs().max() > 0, theirs
    handed_on = [('dP1', 'dpooled'), ('dF1', 'dF6'), ('dF0', 'dx6')][:(0, 2, 3)[depth - 1]]
    assert {k for k in got if k.startswith('d')} == {m for m, _ in handed_on}
    assert {k for k in want if k in ('dpooled', 'dF6', 'dx6')} == {t for _, t in handed_on}
    for mine, theirs in handed_on:
        assert want[theirs].abs().max() > 0
        _close(got[mine], want[theirs], theirs, 1e-10)
    for k, (name, conv) in enumerate(zip(sr.BLOCKS, convs)):
        for i, tensor in enumerate(cr.CONV_TENSORS):
            a, b, start = chain[k]['cw'][i], stage[name]['cw'][i], torch.from_numpy(conv[i]).double()
            if k < 3 - depth:
                assert same(a, start) and same(b, start) and chain[k]['t'] == 0, f'{name} {tensor} runs forward only'
            elif k == 2:
                assert same(a, b) and not same(a, start), f'{name} {tensor}'
            else:
                assert not same(b, start)
                _close(a - start, b - start, f'{name} {tensor}', 1e-7)


# ------------------------------------------------------------------------------------------------ the judge and the faults
FAULT_CASES = {'window0': ((5, 20, 8, 9, 3), 2), 'size_up': ((20, 40, 6, 6, 1), 2), 'no_parity': ((5, 20, 7, 10, 2), 2),
               'parity_shift': ((5, 20, 7, 10, 2), 2), 'hw_swapped': ((5, 20, 7, 10, 2), 2)}
CAPS = (tr.CAP_MAX, tr.CAP_RMS)


@pytest.mark.parametrize('fault', tk.BLOCK_FAULTS)
def test_the_judge_catches_every_block_fault_at_the_caps(fault):
    """The plain f32 run passes the default bound; the same run with the fault seeded exceeds the caps, under which every
    bound in use lies (train_trunk_reference.bound_for asserts that)."""
    case, s = FAULT_CASES[fault]
    conv, x, dF = tk.block_case(case, s)
    clean = tk.judge_block(None, conv, x, dF, s, 'clean')[1]
    tk.judge_block(clean, conv, x, dF, s, 'clean f32', bound=tr.BOUND_DEFAULT)
    bad = tk.judge_block(None, conv, x, dF, s, fault, fault=fault)[1]
    failures = []
    tk.judge_block(bad, conv, x, dF, s, fault, bound=CAPS, collect=failures)
    assert failures, f'{fault} passes the judge at the caps'


@pytest.mark.parametrize('fault', tk.CHAIN_FAULTS)
def test_the_judge_catches_every_chain_fault_at_the_caps(fault):
    args = tk.trunk_case(0, 6)
    convs, spec, shape, table, batches, dfeats, lrs, wd = args
    outs, snaps = tk.run_steps(*args, dtype=torch.float32, eps=1e-3)
    drop = lambda outs: [{k: v for k, v in o.items() if k != 'near_zero'} for o in outs]
    tk.judge_restarted(drop(outs), snaps, args, (0, 1, 2), 'clean f32', eps=1e-3)
    bad_o, bad_s = tk.run_steps(*args, dtype=torch.float32, eps=1e-3, fault=fault)
    failures = []
    keep = set(outs[0])                                   # an extra gradient alone would give the stepping block away
    tk.judge_restarted([{k: v for k, v in o.items() if k in keep} for o in drop(bad_o)], bad_s, args, (0,), fault, eps=1e-3,
                       bound=CAPS, collect=failures)
    assert failures, f'{fault} passes the judge at the caps'
    assert fault != 'frozen_steps' or any('forward-only block' in f for f in failures)


def test_every_override_lies_under_the_caps():
    for name in tk.BOUND_OVERRIDES:
        tk.bound_for(name)
    assert tk.bound_for('F') == tr.BOUND_DEFAULT or 'F' in tk.BOUND_OVERRIDES


@pytest.mark.parametrize('batch_stats', [False, True])
def test_no_gpu_case_breaks_the_side_condition(batch_stats):
    cases = [(c, 2) for c in (tk.BN_CASES if batch_stats else tk.BLOCK_CASES)] + ([] if batch_stats else [(tk.WIDE_CASE, 1)])
    for case, s in cases:
        conv, x, dF = tk.block_case(case, s, batch_stats)
        r = tk.judge_block(None, conv, x, dF, s, '', batch_stats=batch_stats)[0]
        assert r['near_zero'] == 0, (case, r['near_zero'])


# ------------------------------------------------------------------------------------------------ the library, without a GPU
NEW_NAMES = {'axt_conv_trainer_create_strided', 'axt_tile_stacks'}


def test_new_header_declares_and_binds_the_new_names():
    header = open(os.path.join(ROOT, 'include', 'axtrack_hip_trunk.h')).read()
    names = set(re.findall(r'^int (axt_\w+)\s*\(', header, re.M))
    assert names == NEW_NAMES
    main = open(os.path.join(ROOT, 'include', 'axtrack_hip.h')).read()
    assert '#include "axtrack_hip_trunk.h"' in main and not any(re.search(rf'\b{n}\s*\(', main) for n in NEW_NAMES)
    lib = _lib.load()
    assert lib.axt_abi_version() == 1
    for n in NEW_NAMES:
        assert n in _lib.SIGNATURES and hasattr(lib, n), n


def test_create_strided_refuses_before_any_device_call():
    lib = _lib.load()
    Ci, Co = 2, 3
    arrs = [np.zeros(s, np.float32) for s in ((Co, Ci, 3, 3), (Co,), (Co,), (Co,), (Co,), (Co,))]
    ptrs = [a.ctypes.data for a in arrs]
    handle = ctypes.c_void_p()

    def create(Ci=Ci, Co=Co, H=8, W=8, stride=2, ptrs=ptrs, max_batch=4, out=ctypes.byref(handle)):
        return lib.axt_conv_trainer_create_strided(Ci, Co, H, W, stride, *ptrs, max_batch, out)

    bad = [dict(stride=0), dict(stride=3), dict(stride=-1), dict(Ci=0), dict(Ci=513), dict(Co=0), dict(Co=513), dict(H=0),
           dict(W=0), dict(H=513), dict(W=513), dict(H=257, stride=1), dict(W=129, stride=1), dict(max_batch=0),
           dict(max_batch=65), dict(out=None)] + [dict(ptrs=ptrs[:i] + [None] + ptrs[i + 1:]) for i in range(6)]
    for kw in bad:
        assert create(**kw) == AXT_EINVAL, kw
        assert not handle.value
        assert b'axt_conv_trainer_create_strided' in lib.axt_last_error(), kw


def test_tile_stacks_refuses_before_any_device_call():
    lib = _lib.load()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    tiles = np.zeros(2, np.int32)

    def call(frames=p, T_all=7, H=520, W=700, t0=0, n_frames=3, yx=tiles.ctypes.data, n_tiles=1, index=p, B=1, out=p):
        return lib.axt_tile_stacks(frames, T_all, H, W, t0, n_frames, yx, n_tiles, index, B, out, None)

    far = np.array([0, 2], np.int32)                                        # a tile that starts beyond W
    bad = [dict(frames=None), dict(yx=None), dict(index=None), dict(out=None), dict(H=0), dict(W=0), dict(n_tiles=0),
           dict(n_tiles=257), dict(t0=-1), dict(n_frames=0), dict(n_frames=4), dict(t0=1, n_frames=3), dict(B=0), dict(B=1025),
           dict(yx=far.ctypes.data)]
    for kw in bad:
        assert call(**kw) == AXT_EINVAL, kw
        assert b'axt_tile_stacks' in lib.axt_last_error(), kw


def test_block_two_is_known_and_the_others_stay_refused():
    lib = _lib.load()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    tiles = np.zeros(2, np.int32)
    for block in (-1, 0, 1, 3, 5, 8):
        assert lib.axt_cnn_block_features_frames(None, p, 5, 512, 512, 0, 1, tiles.ctypes.data, 1, block, p, None) == AXT_EINVAL
        assert b'block' in lib.axt_last_error()
    assert lib.axt_cnn_block_features_frames(None, p, 5, 512, 512, 0, 1, tiles.ctypes.data, 1, 2, p, None) == AXT_EINVAL
    assert b'block' not in lib.axt_last_error()                             # block 2 is known: the null detector is refused


# ------------------------------------------------------------------------------------------------ the Python layer
def test_tables_and_the_depth_mapping():
    from axtrack_amd import hotpath, training
    assert hotpath.TRUNK_FEATURES == {2: 80 * 64 * 64}
    assert hotpath.BLOCK_FEATURES == {7: 160 * 16 * 16, 6: 80 * 16 * 16, 4: 80 * 32 * 32}
    assert training.DEPTH_INPUT == {0: (7, None), 1: (6, 7), 2: (4, 5), 3: (4, 5), 4: (2, 3), 5: (2, 3), 6: (None, 0),
                                    7: (None, 0), 8: (None, 0)}
    for depth, (block, first) in training.DEPTH_INPUT.items():
        if depth >= 4:                                                      # the trunk reads what the table's block writes
            assert first == (0 if block is None else block + 1) and 8 - first >= depth
    sig = inspect.signature(hotpath.Detector.trunk_features_frames)
    assert list(sig.parameters) == ['self', 'frames', 'tile_yx', 'block', 't0', 'n_frames', 'out']
    assert sig.parameters['block'].default == 2
    assert list(inspect.signature(hotpath.tile_stacks).parameters) == ['frames', 'tile_yx', 'index', 'out']


def test_signatures():
    from axtrack_amd import training
    import axtrack_amd
    head, det = inspect.signature(training.fine_tune_head), inspect.signature(training.fine_tune_detector)
    assert list(head.parameters)[-1] == 'train_last_conv' and head.parameters['train_conv_blocks'].default is None
    assert list(det.parameters) == list(head.parameters)[:-1]
    assert det.parameters['train_conv_blocks'].default == 0
    for name, p in det.parameters.items():
        if name != 'train_conv_blocks':
            assert p.default == head.parameters[name].default, name
    blk = inspect.signature(training.ConvBlockTrainer).parameters
    assert blk['stride'].default == 1 and blk['in_size'].default is None and list(blk)[-2:] == ['stride', 'in_size']
    assert list(inspect.signature(training.ConvTrunkTrainer).parameters) == [
        'state_dict', 'first_block', 'n_trained', 'parameters', 'max_batch', 'device', 'batch_stats', 'momentum', 'block_keys',
        'strides', 'pooled', 'in_size']
    assert axtrack_amd.fine_tune_detector is training.fine_tune_detector
    assert axtrack_amd.ConvTrunkTrainer is training.ConvTrunkTrainer


def test_fine_tune_detector_refuses_before_any_gpu_work():
    import axtrack_amd

    class Tl:
        frame_sharded = False

        def __len__(self):
            return 1

    for depth in (-1, 9, 1.5, '3', True, None):
        with pytest.raises(ValueError, match='train_conv_blocks'):
            axtrack_amd.fine_tune_detector(Tl(), [([1], [1])], {}, train_conv_blocks=depth)
    with pytest.raises(ValueError, match='bn_batch_stats'):
        axtrack_amd.fine_tune_detector(Tl(), [([1], [1])], {}, bn_batch_stats=True)
    with pytest.raises(ValueError, match='bn_momentum'):
        axtrack_amd.fine_tune_detector(Tl(), [([1], [1])], {}, train_conv_blocks=8, bn_batch_stats=True, bn_momentum=0)
    sharded = Tl()
    sharded.frame_sharded = True
    for depth in range(9):
        with pytest.raises(NotImplementedError):
            axtrack_amd.fine_tune_detector(sharded, [([1], [1])], {}, train_conv_blocks=depth)
    with pytest.raises(ValueError, match='fine_tune_detector needs the model'):
        axtrack_amd.fine_tune_detector(Tl(), [([1], [1])], None, train_conv_blocks=5)
    for depth in (4, 9):                                                    # fine_tune_head keeps its range
        with pytest.raises(ValueError, match='train_conv_blocks'):
            axtrack_amd.fine_tune_head(Tl(), [([1], [1])], {}, train_conv_blocks=depth)

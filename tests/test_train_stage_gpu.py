"""Training of the whole last conv stage with the head on the GPU (csrc/train_conv.hip: conv_dgrad_k, maxpool2_fwd_k,
maxpool2_bwd_k; axtrack_amd/training.py: ConvStageTrainer, fine_tune_head(train_conv_blocks=)) against
tests/train_stage_reference.py under train_stage_reference.judge_restarted: the outputs of the three blocks and the pool,
the gradients handed back through the stage, and the updates and Adam moments of every trained tensor, each no further from
the f64 reference than a small multiple of what plain f32 on the CPU is on the same input. The pool and its gradient are
compared with torch's CPU max_pool2d bit for bit. The stage is ConvTrunkTrainer's three-block case: the chain's loop against
the same ConvBlockTrainer and pool calls written out by hand, byte for byte (test_the_stage_is_its_blocks_called_by_hand).

The tile edges of conv_dgrad_k, each with a case on either side (test_input_grad_tile_edges):
  input channels     64 per workgroup (the kernel's output rows)                      Ci = 64 | 65
  r = B*H*W          64 per workgroup                                                 r = 64 | 65
  q = 9*Co           tiles 16 deep                                                    9*Co = 144 (whole tiles) | 63, 72
The stage cases are (Ci, C5, C6, C7, H, W) with heads (H1, H2): no two channel counts equal and the third block on 3 x 3
maps; a square middle block on odd maps (the pool floors 5 x 7 to 2 x 3: row 4 and column 6 get zero gradient); a pooled map
of one row; and the first case on rows that are all zero or one constant. In the last one the pooling windows that no tap
reaches the zero padding from tie exactly (on 6 x 6 maps the middle one of nine; the windows along the border see the
padding and do not tie).
"""

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import helpers
import train_conv_reference as cr
import train_reference as tr
import train_stage_reference as sr
from axtrack_amd import synth, training
from axtrack_amd.hotpath import conv_block_key

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
LAM = (49.5, 1.0, 49.5)
LR, WD = 1e-2, 0.05                 # as tests/test_train_conv_gpu.py: an update is far above the judge's absolute floors
EPS = 1e-3                          # Adam's eps in the judged steps, for the reason test_train_gpu.py gives
KEYS = ('b5', 'b6', 'b7')


def _state_dict(convs, head_w):
    sd = {f'{key}.{k}': a for key, conv in zip(KEYS, convs) for k, a in zip(training.CONV_SUFFIXES + training.CONV_STATS, conv)}
    sd.update(zip(training.FC_KEYS, head_w))
    return sd


def _trainers(convs, head_w, shape, max_batch, depth=3, lr=LR, wd=WD):
    P = dict(LR=lr, WEIGHT_DECAY=wd)
    sd = _state_dict(convs, head_w)
    st = training.ConvStageTrainer(sd, depth, P, max_batch=max_batch, device=DEV, block_keys=KEYS, map_size=shape[1:])
    return st, training.HeadTrainer(sd, P, max_batch=max_batch, device=DEV)


def _snapshot(st, ht):
    hm = [ht.moments(l) for l in range(3)]
    snap = dict(w=ht.weights(), m=[a for mm in hm for a in (mm[0], mm[2])], v=[a for mm in hm for a in (mm[1], mm[3])],
                t=[hm[0][4]])
    for name, blk in zip(sr.BLOCKS, st.blocks):
        mom = [blk.moments(i) for i in range(4)]
        snap[name] = dict(cw=blk.weights(), cm=[m[0] for m in mom], cv=[m[1] for m in mom])
        snap['t'].append(mom[0][2])
    return snap


def _cpu_pool(f6, dpooled, B, C, H, W):
    """torch's CPU max_pool2d and its autograd on the run's own F6 -> (pooled, dF6) as [B, .] arrays."""
    x = torch.from_numpy(f6).reshape(B, C, H, W).clone().requires_grad_(True)
    out = F.max_pool2d(x, 2, 2)
    if dpooled is None:
        return out.detach().reshape(B, -1).numpy(), None
    out.backward(torch.from_numpy(dpooled).reshape(out.shape))
    return out.detach().reshape(B, -1).numpy(), x.grad.reshape(B, -1).numpy()


def _run_gpu(st, ht, table, targets, batches, lrs, eps=EPS):
    """The joint step of fine_tune_head(train_conv_blocks=depth) per batch -> (outs, snapshots) shaped like
    train_stage_reference.run_steps'. The pool's two results are compared with torch's on the CPU on the way."""
    d_table, d_tgt = torch.from_numpy(table).to(DEV), torch.from_numpy(targets).to(DEV)
    outs, snaps = [], []
    for idx, lr in zip(batches, lrs):
        Fo = st.forward(d_table, idx)
        f5, f6, pooled, _ = helpers.stage_kept(st)
        y = ht.forward(Fo)
        _, dy = ht.loss(y, d_tgt, idx)
        dfeat = ht.input_grad(dy)
        grads = st.backward_and_step(d_table, idx, dfeat, lr=lr, eps=eps)
        ht.step(Fo, None, dy, lr=lr, eps=eps)
        out = dict(F5=f5, F6=f6, pooled=pooled, F=Fo, dfeat=dfeat)
        out.update({k: grads[g] for k, g in (('dpooled', 'p6'), ('dF6', 'f6'), ('dx6', 'f5')) if g in grads})
        out = {k: v.cpu().numpy() for k, v in out.items()}
        want_p, want_g = _cpu_pool(out['F6'], out.get('dpooled'), len(idx), st.blocks[1].Co, st.H, st.W)
        assert out['pooled'].tobytes() == want_p.tobytes(), 'the pooled maps are not torch\'s'
        if want_g is not None:
            assert out['dF6'].tobytes() == want_g.tobytes(), 'the pool\'s gradient is not torch\'s'
        outs.append(out)
        snaps.append(_snapshot(st, ht))
    return outs, snaps


def _judge(outs, snaps, args, steps, label, depth=3, eps=EPS):
    failures = []
    sr.judge_restarted(outs, snaps, args, steps, depth, label, eps=eps, log=print, collect=failures)
    for s in steps:
        assert snaps[s]['t'] == [s + 1] + [s + 1 if i >= 3 - depth else 0 for i in range(3)]
    assert not failures, f'{len(failures)} comparisons failed:\n' + '\n'.join(failures[:10])


def _batches(B, n, steps=3):
    rng = np.random.default_rng(B)
    batches = [rng.integers(0, n, B)[::-1].copy() for _ in range(steps)]       # with repetition, out of order
    if B > 1:
        batches[0][1] = batches[0][0]
    return batches


@pytest.fixture(scope='module')
def stage_cases():
    out = {name: sr.synth_stage(dims, heads, seed=100 + i, n=40) for i, (name, (dims, heads)) in enumerate(sr.CASES.items())}
    convs, head, shape, table, tgt = out['unequal']
    out['tied'] = (convs, head, shape, sr.tied_table(table), tgt)
    return out


# ------------------------------------------------------------------------------------------------ the stage, small and awkward
@pytest.mark.parametrize('B', [1, 3, 33])
@pytest.mark.parametrize('case', ['unequal', 'square_odd', 'one_row', 'tied'])
def test_small_stage_steps(stage_cases, case, B):
    """Three joint depth-3 steps; steps 1 and 3 are judged. The batch rows repeat and come out of order."""
    convs, head_w, shape, table, tgt = stage_cases[case]
    batches = _batches(B, len(table))
    lrs = [LR * 0.9 ** s for s in range(3)]
    st, ht = _trainers(convs, head_w, shape, max_batch=33)
    outs, snaps = _run_gpu(st, ht, table, tgt, batches, lrs)
    _judge(outs, snaps, (convs, head_w, shape, table, tgt, batches, LAM, lrs, WD), (0, 2), f'{case} B={B}')
    if case == 'square_odd':
        g = outs[0]['dF6'].reshape(B, 6, 5, 7)
        assert not g[:, :, 4].any() and not g[:, :, :, 6].any() and g[:, :, :4, :6].any()
    if case == 'tied':                                    # the window that ties gives its gradient to its first element
        g = outs[0]['dF6'].reshape(B, 4, 6, 6)[:, :, 2:4, 2:4]
        v = outs[0]['F6'].reshape(B, 4, 6, 6)[:, :, 2:4, 2:4].reshape(B, 4, 4)
        assert (v == v[..., :1]).all() and g[:, :, 0, 0].any() and not g[:, :, 0, 1].any() and not g[:, :, 1].any()


def test_depth_two_leaves_the_first_block_alone(stage_cases):
    """depth = 2: block 5 runs forward only; its tensors and moments stay what they were, the rest is judged."""
    convs, head_w, shape, table, tgt = stage_cases['square_odd']
    batches = _batches(3, len(table))
    st, ht = _trainers(convs, head_w, shape, max_batch=3, depth=2)
    outs, snaps = _run_gpu(st, ht, table, tgt, batches, [LR] * 3)
    assert 'dF6' in outs[0] and 'dx6' not in outs[0]
    _judge(outs, snaps, (convs, head_w, shape, table, tgt, batches, LAM, [LR] * 3, WD), (0, 2), 'depth 2', depth=2)
    for a, b in zip(snaps[-1]['b5']['cw'], convs[0][:4]):
        assert a.tobytes() == b.tobytes()
    assert not any(a.any() for a in snaps[-1]['b5']['cm'] + snaps[-1]['b5']['cv'])
    sd = st.state_dict(ht.state_dict())
    assert all(sd[f'b5.{k}'] is st._sd[f'b5.{k}'] for k in training.CONV_SUFFIXES + training.CONV_STATS)
    assert np.abs(sd['b6.conv.weight'] - convs[1][0]).max() > LR / 2


# ------------------------------------------------------------------------------------------------ the chain is its blocks
def _block_state(blk):
    """Everything a ConvBlockTrainer holds, as bytes: the tensors, the Adam moments with their step counts, BatchNorm's
    statistics with the batch count."""
    mom = [blk.moments(i) for i in range(4)]
    st = blk.stats()
    arrays = blk.weights() + [a for m in mom for a in m[:2]] + [np.array([m[2] for m in mom] + [st['num_batches_tracked']])]
    arrays += [st[k] for k in ('running_mean', 'running_var', 'batch_mean', 'batch_var') if st[k] is not None]
    return [a.tobytes() for a in arrays]


@pytest.mark.parametrize('batch_stats', [False, True])
@pytest.mark.parametrize('depth', [1, 2, 3])
def test_the_stage_is_its_blocks_called_by_hand(stage_cases, depth, batch_stats):
    """ConvStageTrainer.forward / backward_and_step against three ConvBlockTrainers of the same state dict driven by the
    sequence the chain stands for, written out with no loop: after each of three steps (rows repeated and out of order, a
    learning rate per step, a seeded random dfeat) the output, every gradient handed on, and every block's tensors, moments,
    step counts and statistics are the same bytes. A forward-only block runs with its running statistics in both."""
    convs, head_w, shape, table, _ = stage_cases['unequal']
    (_, H, W), B = shape, 3
    P = dict(LR=LR, WEIGHT_DECAY=WD)
    sd = _state_dict(convs, head_w)
    st = training.ConvStageTrainer(sd, depth, P, max_batch=B, device=DEV, block_keys=KEYS, map_size=(H, W),
                                   batch_stats=batch_stats)
    b5, b6, b7 = (training.ConvBlockTrainer(sd, key, P, map_size=size, max_batch=B, device=DEV,
                                            batch_stats=batch_stats and i >= 3 - depth)
                  for i, (key, size) in enumerate(zip(KEYS, [(H, W), (H, W), (H // 2, W // 2)])))
    assert [b.batch_stats for b in st.blocks] == [b.batch_stats for b in (b5, b6, b7)]
    d_table = torch.from_numpy(table).to(DEV)
    rows = torch.arange(B, dtype=torch.int32, device=DEV)
    rng = np.random.default_rng(depth)
    same = lambda a, b: a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    for step, idx in enumerate(_batches(B, len(table))):
        lr = LR * 0.9 ** step
        dfeat = torch.from_numpy(rng.normal(0, 1, (B, st.out_width)).astype(np.float32)).to(DEV)
        out = st.forward(d_table, idx)
        grads = st.backward_and_step(d_table, idx, dfeat, lr=lr, eps=EPS)
        # the same by hand
        f5 = b5.forward(d_table, idx)
        f6 = b6.forward(f5, rows)
        pooled = training.maxpool2_forward(f6, H, W).reshape(B, b7.in_width)
        f7 = b7.forward(pooled, rows)
        want = {}
        if depth >= 2:
            want['p6'] = b7.input_grad(dfeat)
        b7.step(pooled, rows, dfeat, lr=lr, eps=EPS)
        if depth >= 2:
            want['f6'] = training.maxpool2_backward(f6, want['p6'], H, W)
            if depth >= 3:
                want['f5'] = b6.input_grad(want['f6'])
            b6.step(f5, rows, want['f6'], lr=lr, eps=EPS)
        if depth >= 3:
            b5.step(d_table, idx, want['f5'], lr=lr, eps=EPS)
        assert same(out, f7) and out.abs().max().item() > 0, f'step {step}: the output'
        assert list(grads) == list(want) == ['p6', 'f6', 'f5'][:(0, 2, 3)[depth - 1]]
        for k in want:
            assert grads[k].numel() == want[k].numel() and same(grads[k], want[k]), f'step {step}: gradient {k}'
        for name, mine, theirs in zip(KEYS, st.blocks, (b5, b6, b7)):
            assert _block_state(mine) == _block_state(theirs), f'step {step}: {name}'
    steps = [b.moments(0)[2] for b in st.blocks]
    assert steps == [3 if i >= 3 - depth else 0 for i in range(3)]
    assert [b.stats()['num_batches_tracked'] for b in st.blocks] == (steps if batch_stats else [0, 0, 0])


# ------------------------------------------------------------------------------------------------ the data gradient alone
EDGES =[(64, 7, 4, 4, 4),       # Ci = 64: one whole tile of input channels; 9 Co = 63; r = 64
         (65, 8, 5, 13, 1),      # Ci = 65; 9 Co = 72; r = 65: one past each
         (3, 16, 3, 5, 2),       # 9 Co = 144: nine whole depth tiles
         (5, 3, 7, 9, 64)]       # r = 4032: 63 whole tiles, the largest batch


def _block(Ci, Co, H, W, B, seed):
    conv = cr.synth_block(Ci, Co, seed, scale=2.0)
    sd = {f'blk.{k}': a for k, a in zip(training.CONV_SUFFIXES + training.CONV_STATS, conv)}
    ct = training.ConvBlockTrainer(sd, 'blk', dict(LR=LR, WEIGHT_DECAY=WD), map_size=(H, W), max_batch=B, device=DEV)
    x, _ = cr.synth_inputs(B, Ci, H, W, seed + 1)
    dF = np.random.default_rng(seed + 2).normal(0, 1, (B, Co * H * W)).astype(np.float32)
    return conv, ct, x, dF


def _ref_input_grad(conv, x, dF, shape, dtype):
    Ci, Co, H, W = shape
    w = [torch.from_numpy(a).to(dtype) for a in conv]
    fwd = cr.block_forward(w[:4], (w[4], w[5]), torch.from_numpy(x).to(dtype).reshape(-1, Ci, H, W))
    return sr.block_input_grad(w[:4], fwd, torch.from_numpy(dF).to(dtype).reshape(-1, Co, H, W)).reshape(len(x), -1).numpy()


@pytest.mark.parametrize('edge', EDGES, ids=lambda e: 'x'.join(map(str, e)))
def test_input_grad_tile_edges(edge):
    """ConvBlockTrainer.input_grad on either side of every tile edge of conv_dgrad_k (module docstring), from a random dF."""
    Ci, Co, H, W, B = edge
    conv, ct, x, dF = _block(Ci, Co, H, W, B, seed=Ci * 100 + Co)
    ct.forward(torch.from_numpy(x).to(DEV))
    got = ct.input_grad(torch.from_numpy(dF).to(DEV)).cpu().numpy()
    assert got.shape == (B, Ci * H * W)
    ref, yard = (_ref_input_grad(conv, x, dF, (Ci, Co, H, W), d) for d in (torch.float64, torch.float32))
    tr.judge(got, ref, yard, f'dx alone @edge {edge}', log=print, bound=tr.BOUND_DEFAULT)


def test_input_grad_takes_the_slope_at_y_zero():
    """Output channel 0 sits at y == 0 exactly (train_conv_reference.y_zero_block's bias, mean and beta, on a zero input, so
    that its weights can stay what they were) and alone carries gradient: its dz is 0.1 dF gamma / sigma."""
    Ci, Co, H, W, B = 3, 8, 5, 5, 3
    conv = cr.synth_block(Ci, Co, 9, scale=2.0)
    pinned = cr.y_zero_block(conv)
    pinned[0][0] = conv[0][0]
    sd = {f'blk.{k}': a for k, a in zip(training.CONV_SUFFIXES + training.CONV_STATS, pinned)}
    ct = training.ConvBlockTrainer(sd, 'blk', map_size=(H, W), max_batch=B, device=DEV)
    x = np.zeros((B, Ci * H * W), np.float32)
    dF = np.zeros((B, Co, H, W), np.float32)
    dF[:, 0] = np.random.default_rng(11).normal(0, 1, (B, H, W))
    dF = dF.reshape(B, -1)
    out = ct.forward(torch.from_numpy(x).to(DEV)).cpu().numpy().reshape(B, Co, H, W)
    assert not out[:, 0].any() and out[:, 1:].all()
    got = ct.input_grad(torch.from_numpy(dF).to(DEV)).cpu().numpy()
    ref, yard = (_ref_input_grad(pinned, x, dF, (Ci, Co, H, W), d) for d in (torch.float64, torch.float32))
    assert np.abs(ref).max() > 1e-3
    tr.judge(got, ref, yard, 'dx alone @y == 0', log=print, bound=tr.BOUND_DEFAULT)


def test_input_grad_changes_nothing_and_repeats(stage_cases):
    """step() gives identical bytes with and without an input_grad before it; two calls give identical bits; the trainer
    holds the memory it held; another B than the last forward's is refused as step() refuses it."""
    Ci, Co, H, W, B = 5, 41, 10, 10, 33
    runs = []
    for with_grad in (False, True):
        conv, ct, x, dF = _block(Ci, Co, H, W, B, seed=77)
        d_x, d_dF = torch.from_numpy(x).to(DEV), torch.from_numpy(dF).to(DEV)
        held = ct.device_bytes
        for _ in range(2):
            ct.forward(d_x)
            if with_grad:
                g1, g2 = ct.input_grad(d_dF), ct.input_grad(d_dF)
                assert g1.cpu().numpy().tobytes() == g2.cpu().numpy().tobytes() and g1.abs().max().item() > 0
            ct.step(d_x, None, d_dF, lr=LR, eps=EPS)
        assert ct.device_bytes == held
        runs.append(ct.weights() + [a for i in range(4) for a in ct.moments(i)[:2]])
    for a, b in zip(*runs):
        assert a.tobytes() == b.tobytes()
    assert np.abs(runs[0][0] - conv[0]).max() > LR / 2
    ct.forward(d_x)
    with pytest.raises(Exception, match='stashed'):
        ct.input_grad(d_dF[:2].contiguous())
    for bad in (0, 34):
        assert ct._lib.axt_conv_trainer_input_grad(ct._h, d_dF.data_ptr(), bad, d_dF.data_ptr(), None) == -22
    with pytest.raises(ValueError):
        ct.input_grad(d_dF[:, :-1].contiguous())


# ------------------------------------------------------------------------------------------------ the pool alone
@pytest.mark.parametrize('shape', sr.POOL_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_pool_is_torchs_cpu_pool_bit_for_bit(shape):
    """Ties at each of the four positions, -0.0 against +0.0, whole constant maps; d_din poisoned before the call."""
    n, H, W = shape
    x = sr.pool_input(n, H, W, seed=H * W)
    xt = torch.from_numpy(x)[None].clone().requires_grad_(True)
    out = F.max_pool2d(xt, 2, 2)
    dout = np.random.default_rng(1).normal(0, 1, tuple(out.shape[1:])).astype(np.float32)
    out.backward(torch.from_numpy(dout)[None])
    d_x, d_dout = torch.from_numpy(x).to(DEV), torch.from_numpy(dout).to(DEV)
    got = training.maxpool2_forward(d_x, H, W)
    assert got.cpu().numpy().tobytes() == out.detach().numpy().tobytes()
    assert training.maxpool2_backward(d_x, d_dout, H, W).cpu().numpy().tobytes() == xt.grad.numpy().tobytes()
    din = torch.full((n, H, W), float('nan'), device=DEV)                   # every element is written
    lib = training._lib.load()
    with torch.cuda.device(DEV):
        assert lib.axt_maxpool2_backward(d_x.data_ptr(), d_dout.data_ptr(), n, H, W, din.data_ptr(), None) == 0
        torch.cuda.synchronize()
    assert din.cpu().numpy().tobytes() == xt.grad.numpy().tobytes()


def test_pool_refuses_a_map_of_one_row():
    x = torch.zeros((2, 1, 6), device=DEV)
    lib = training._lib.load()
    assert lib.axt_maxpool2_forward(x.data_ptr(), 2, 1, 6, x.data_ptr(), None) == -22
    assert lib.axt_maxpool2_backward(x.data_ptr(), x.data_ptr(), 2, 1, 6, x.data_ptr(), None) == -22
    with pytest.raises(Exception, match='axt_maxpool2_forward'):
        training.maxpool2_forward(x, 1, 6)


# ------------------------------------------------------------------------------------------------ the deployed stage
@pytest.fixture(scope='module')
def deployed(weights):
    import axtrack_amd
    frames = torch.from_numpy(synth.synth_frames(6, 512, 512, seed=3)).to(DEV)
    det = axtrack_amd.Detector(weights, max_batch=2, device=DEV)
    return det, frames


def test_block_four_features(deployed):
    """block=4 is the detector's buffer 4 byte for byte; blocks 6 and 7 return what they return without it in between."""
    det, frames = deployed
    x6, x7 = (det.features_frames(frames, [(0, 0)], block=b).cpu().numpy() for b in (6, 7))
    x4 = det.features_frames(frames, [(0, 0)], block=4)
    assert tuple(x4.shape) == (2, 80 * 32 * 32)
    act4 = helpers.cnn_activation(det, 4, 0, 2)
    assert x4.cpu().numpy().tobytes() == act4.tobytes() and np.abs(act4).max() > 0
    for b, old in ((6, x6), (7, x7)):
        assert det.features_frames(frames, [(0, 0)], block=b).cpu().numpy().tobytes() == old.tobytes()
    with pytest.raises(ValueError):
        det.features_frames(frames, [(0, 0)], block=5)
    table = torch.zeros((3, 80 * 32 * 32), device=DEV)                       # spare rows, as under augmentation
    part = det.features_frames(frames, [(0, 0)], out=table, block=4)
    assert part.data_ptr() == table.data_ptr() and part.cpu().numpy().tobytes() == act4.tobytes() and not table[2].any()


def test_stage_forward_at_the_initial_weights_is_the_detectors(deployed, weights):
    """ConvStageTrainer.forward on the block-4 table: every block against the same block in f64 on the chain's own input to
    it (cnn_reference.judge, the bounds of a direct f32 kernel), and the pooled maps within the sum of both bounds of
    features_frames(block=6)."""
    import cnn_reference as cnr
    det, frames = deployed
    x4 = det.features_frames(frames, [(0, 0)], block=4)
    x6 = det.features_frames(frames, [(0, 0)], block=6).cpu().numpy().reshape(2, 80, 16, 16)
    st = training.ConvStageTrainer(weights, 3, max_batch=2, device=DEV)
    assert [(b.Ci, b.Co, b.H, b.W) for b in st.blocks] == [(80, 80, 32, 32), (80, 80, 32, 32), (80, 160, 16, 16)]
    st.forward(x4)
    f5, f6, pooled, f7 = (a.cpu().numpy() for a in helpers.stage_kept(st))
    h4, f5, pooled, f7 = x4.cpu().numpy().reshape(2, 80, 32, 32), f5.reshape(2, 80, 32, 32), pooled.reshape(2, 80, 16, 16), \
        f7.reshape(2, 160, 16, 16)
    for layer, got, inp in ((5, f5, h4), (6, pooled, f5), (7, f7, pooled)):
        ref, yard = cnr.ref_block(weights, layer, inp), cnr.yard_block(weights, layer, inp)
        r = cnr.judge(got, ref, yard, *cnr.bound_for('f32_direct', layer), layer=f'ConvStageTrainer.forward (conv block {layer})')
        print(f'ConvStageTrainer.forward conv block {layer} against f64: {r[0]:.3f} (max) {r[1]:.3f} (rms) of the f32 yardstick')
    ref = cnr.ref_block(weights, 6, cnr.ref_block(weights, 5, h4))
    yard = cnr.yard_block(weights, 6, cnr.yard_block(weights, 5, h4))
    c_direct, c_det = cnr.bound_for('f32_direct', 6), cnr.bound_for('f32_winograd', 6)
    diff, allowed = np.abs(pooled - x6).max(), (c_direct[0] + c_det[0]) * (np.abs(yard - ref).max() + cnr.FLOOR_MAX)
    print(f'the chain\'s pooled maps against features_frames(block=6): max difference {diff:.3g}, allowed {allowed:.3g}')
    assert diff <= allowed


def test_full_size_stage_step(deployed, weights):
    """The deployed stage and head on the trunk features of 2 frames x 1 tile: one joint depth-3 step at B = 2 meets the
    same judgement as the small stages."""
    det, frames = deployed
    x4 = det.features_frames(frames, [(0, 0)], block=4).cpu().numpy()
    P = dict(LR=LR, WEIGHT_DECAY=WD)
    st = training.ConvStageTrainer(weights, 3, P, max_batch=2, device=DEV)
    ht = training.HeadTrainer(weights, P, max_batch=2, device=DEV)
    convs = [[np.asarray(weights[k], np.float32) for k in b.keys] for b in st.blocks]
    head_w = [np.asarray(weights[k], np.float32) for k in training.FC_KEYS]
    lx, ly, cnt = training.label_arrays([([100, 400], [200, 30]), ([250, 251], [77, 300])])
    tgt = tr.ref_targets(lx, ly, cnt, [(0, 0)]).reshape(2, 12, 12, 4)
    batches = [np.array([1, 0])]
    outs, snaps = _run_gpu(st, ht, x4, tgt, batches, [LR])
    _judge(outs, snaps, (convs, head_w, (80, 32, 32), x4, tgt, batches, LAM, [LR], WD), (0,), 'full size B=2')
    sd = st.state_dict(ht.state_dict())
    trained = {k for b in st.blocks for k in b.keys[:4]} | set(training.FC_KEYS)
    assert set(sd) == set(weights) and all(sd[k] is weights[k] for k in weights if k not in trained)
    for name, b in zip(sr.BLOCKS, st.blocks):
        assert all(np.array_equal(sd[k], a) for k, a in zip(b.keys[:4], snaps[0][name]['cw']))


# ------------------------------------------------------------------------------------------------ end to end
def _e2e_setup(weights):
    import axtrack_amd
    E = tr.E2E
    frames = synth.synth_frames(E['T_all'], E['H'], E['W'], seed=E['frames_seed'])
    tl = axtrack_amd.Timelapse(frames, name='train', device=DEV)
    det = axtrack_amd.Detector(weights, max_batch=8, device=DEV)
    return E, tl, det, tr.e2e_labels()


def _same(a, b):
    return set(a) == set(b) and all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in a)


@pytest.fixture(scope='module')
def depth3_run(weights, tmp_path_factory):
    import axtrack_amd
    E, tl, det, labels = _e2e_setup(weights)
    dest = str(tmp_path_factory.mktemp('depth3'))
    sd, hist = axtrack_amd.fine_tune_head(tl, labels, det, E['parameters'], E['epochs'], dest_dir=dest, seed=E['seed'],
                                          train_conv_blocks=3)
    return E, tl, det, labels, sd, hist, dest


def test_fine_tune_with_the_last_stage_end_to_end(weights, depth3_run):
    """8 items, shuffled batches of 5 and 3, 3 epochs at depth 3: the history against the f64 replay of the same schedule
    on the GPU's own block-4 table; the state dict loads into a Detector and the checkpoint through setup_inference's
    loader."""
    import axtrack_amd
    from axtrack_amd.interface import _load_state_dict
    from axtrack_amd.training import TRAIN_DEFAULTS
    E, tl, det, labels, sd, hist, dest = depth3_run
    assert list(hist.index) == list(tr.COMPONENTS) and list(hist.columns) == list(range(E['epochs']))
    h4 = det.features_frames(tl.frames, tl.tile_yx, block=4).cpu().numpy()
    assert h4.shape == (8, 80 * 32 * 32)
    lx, ly, cnt = training.label_arrays(labels)
    targets = tr.ref_targets(lx, ly, cnt, tl.tile_yx).reshape(-1, 12, 12, 4)
    P = dict(TRAIN_DEFAULTS, **E['parameters'])
    sched = tr.epoch_schedule(8, E['epochs'], P['BATCH_SIZE'], P['SHUFFLE'], P['DROP_LAST'], E['seed'], P['LR'], P['LR_DECAYRATE'])
    assert [len(b) for _, b, _ in sched] == [5, 3] * E['epochs']
    keys = [tuple(f'{conv_block_key(i)}.{k}' for k in training.CONV_SUFFIXES + training.CONV_STATS)
            for i in training.STAGE_BLOCKS]
    convs = [[np.asarray(weights[k], np.float32) for k in ks] for ks in keys]
    head_w = [np.asarray(weights[k], np.float32) for k in training.FC_KEYS]
    args = (convs, head_w, (80, 32, 32), h4, targets, [b for _, b, _ in sched], (P['L_OBJECT'], P['L_NOBJECT'], P['L_COORD_ANCHOR']),
            [lr for _, _, lr in sched], P['WEIGHT_DECAY'])
    (_, r_outs, r_snaps), (_, y_outs, _) = sr.ref_steps(*args), sr.yard_steps(*args)
    r_hist, y_hist = tr.history(sched, r_outs, E['epochs']), tr.history(sched, y_outs, E['epochs'])
    total = r_hist[tr.COMPONENTS.index('total_summed_loss')]
    got_total = hist.loc['total_summed_loss'].to_numpy()
    print('reference total_summed_loss per epoch:', total, ' GPU:', got_total)
    assert total[-1] < total[0] and got_total[-1] < got_total[0]
    failures = []
    for i, name in enumerate(tr.COMPONENTS):
        try:
            tr.judge(hist.loc[name].to_numpy(), r_hist[i], y_hist[i], f'history {name}', log=print,
                     bound=sr.bound_for(f'history {name}'))
        except tr.TrainMismatch as e:
            failures.append(str(e))
    assert not failures, '\n'.join(failures)
    # every trained tensor has moved, in the direction the reference moves it; conv blocks 0-4, the running statistics and
    # num_batches_tracked are the very objects that went in
    trained = set(training.FC_KEYS)
    for ks, name in zip(keys, sr.BLOCKS):
        trained |= set(ks[:4])
        for k, r in zip(ks[:4], r_snaps[-1][name]['cw']):
            moved, want = np.asarray(sd[k], np.float64) - weights[k], r - weights[k]
            assert np.abs(moved).max() > 0 and np.sum(moved * want) > 0.5 * np.sum(want * want), k
    assert set(sd) == set(weights) and all(sd[k] is weights[k] for k in weights if k not in trained)
    assert len(trained) == 18 and all('running' not in k and 'num_batches' not in k for k in trained)
    back = _load_state_dict(f'{dest}/E{E["epochs"] - 1:04}.pth')
    assert all(np.array_equal(back[k].numpy(), np.asarray(sd[k])) for k in sd)
    grids = axtrack_amd.Detector(sd, max_batch=8, device=DEV).detect_frames(tl.frames, tl.tile_yx)
    assert (grids - axtrack_amd.Detector(back, max_batch=8, device=DEV).detect_frames(tl.frames, tl.tile_yx)).abs().max().item() == 0
    assert (grids - det.detect_frames(tl.frames, tl.tile_yx)).abs().max().item() > 1e-2


def test_two_depth_three_runs_end_byte_identical(weights, depth3_run):
    import axtrack_amd
    E, tl, det, labels, sd, hist, _ = depth3_run
    sd2, hist2 = axtrack_amd.fine_tune_head(tl, labels, det, E['parameters'], E['epochs'], seed=E['seed'], train_conv_blocks=3)
    assert _same(sd, sd2) and hist.to_numpy().tobytes() == hist2.to_numpy().tobytes()


def test_depth_one_is_train_last_conv_byte_for_byte(weights, tmp_path):
    import axtrack_amd
    from axtrack_amd.interface import _load_state_dict
    E, tl, det, labels = _e2e_setup(weights)
    runs = []
    for name, kw in (('a', dict(train_last_conv=True)), ('b', dict(train_conv_blocks=1)),
                     ('c', dict(train_conv_blocks=1, train_last_conv=True))):
        sd, hist = axtrack_amd.fine_tune_head(tl, labels, det, E['parameters'], E['epochs'], dest_dir=f'{tmp_path}/{name}',
                                              seed=E['seed'], **kw)
        back = _load_state_dict(f'{tmp_path}/{name}/E{E["epochs"] - 1:04}.pth')
        runs.append((sd, hist.to_numpy().tobytes(), {k: v.numpy() for k, v in back.items()}))
    for sd, hist, back in runs[1:]:
        assert _same(sd, runs[0][0]) and hist == runs[0][1] and _same(back, runs[0][2])
    assert np.abs(np.asarray(runs[0][0][f'{training.LAST_CONV_BLOCK}.conv.weight']) - weights[f'{training.LAST_CONV_BLOCK}.conv.weight']).max() > 0
    sd0, hist0 = axtrack_amd.fine_tune_head(tl, labels, det, E['parameters'], E['epochs'], seed=E['seed'], train_conv_blocks=0)
    sdd, histd = axtrack_amd.fine_tune_head(tl, labels, det, E['parameters'], E['epochs'], seed=E['seed'])
    assert _same(sd0, sdd) and hist0.to_numpy().tobytes() == histd.to_numpy().tobytes()


def test_depth_two_returns_block_five_as_it_came(weights):
    import axtrack_amd
    E, tl, det, labels = _e2e_setup(weights)
    sd, hist = axtrack_amd.fine_tune_head(tl, labels, det, E['parameters'], E['epochs'], seed=E['seed'], train_conv_blocks=2)
    k5, k6, k7 = (conv_block_key(i) for i in training.STAGE_BLOCKS)
    trained = {f'{k}.{s}' for k in (k6, k7) for s in training.CONV_SUFFIXES} | set(training.FC_KEYS)
    assert set(sd) == set(weights) and all(sd[k] is weights[k] for k in weights if k not in trained)
    assert all(np.asarray(sd[f'{k5}.{s}']).tobytes() == np.asarray(weights[f'{k5}.{s}'], np.float32).tobytes()
               for s in training.CONV_SUFFIXES)
    assert all(np.abs(np.asarray(sd[k], np.float64) - weights[k]).max() > 0 for k in trained)
    assert np.isfinite(hist.to_numpy()).all()


def test_errors_come_before_any_gpu_work(weights):
    import axtrack_amd
    E, tl, det, labels = _e2e_setup(weights)
    for kw in (dict(train_conv_blocks=4), dict(train_conv_blocks=-1), dict(train_conv_blocks=0, train_last_conv=True),
               dict(train_conv_blocks=3, train_last_conv=True)):
        with pytest.raises(ValueError):
            axtrack_amd.fine_tune_head(tl, labels, det, E['parameters'], 1, **kw)
    tl.frame_sharded = True
    with pytest.raises(NotImplementedError):
        axtrack_amd.fine_tune_head(tl, labels, det, E['parameters'], 1, train_conv_blocks=3)

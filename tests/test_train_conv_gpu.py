"""The conv-block trainer and the joint step with the head on the GPU (csrc/train_conv.hip, csrc/train.hip,
axtrack_amd/training.py) against tests/train_conv_reference.py: the block's output F, the head's input gradient, and the
updates and Adam moments of the four conv tensors and the six head tensors under train_reference.judge (error against the
f64 reference no more than a small multiple of what plain f32 on the CPU makes on the same input).

The tile edges of the kernels, each with a case on either side (test_tile_edges):
  output channels    64 per workgroup (conv_fwd_k, conv_wgrad_k)                      Co = 64 | 65
  r = B*H*W          64 per workgroup (conv_fwd_k)                                    r = 64 | 65
  q = 9*Ci           tiles 16 deep (conv_fwd_k), 64 per workgroup (conv_wgrad_k)      9*Ci = 144 (whole tiles) | 63, 72
  r = B*H*W          256 per pass of a channel's workgroup (conv_bn_back_k)           r = 255, 256 | 272
  split of r         runs of ceil(r / 64) rounded up to 16 (conv_wgrad_k)             r = 1024: 64 runs of 16 | 1025: 33 of 32
  input gradient     one slab written in place | several summed (head_gemm's split)   H1 = 32, 1024 | H1 = 72, 130
Every judged tensor has at least 8 elements (8 output channels, a head of 32 and 24 units) except in the one-row case
(2,3,1,6): the judge compares the largest and the rms error of a tensor with the yardstick's, and over three numbers that
is a ratio of single draws of the roundings upstream, whatever the kernel does.
"""
import numpy as np
import pytest
import torch

import train_conv_reference as cr
import train_reference as tr
from axtrack_amd import synth, training

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
LAM = (49.5, 1.0, 49.5)
LR, WD = 1e-2, 0.05                 # as tests/test_train_gpu.py: an update is far above the judge's absolute floors
EPS = 1e-3                          # Adam's eps in the judged steps, for the reason test_train_gpu.py gives
KEY = 'blk'


def _trainers(conv, head_w, shape, max_batch, lr=LR, wd=WD):
    Ci, H, W = shape
    sd = {f'{KEY}.{k}': a for k, a in zip(training.CONV_SUFFIXES + training.CONV_STATS, conv)}
    P = dict(LR=lr, WEIGHT_DECAY=wd)
    ct = training.ConvBlockTrainer(sd, KEY, P, map_size=(H, W), max_batch=max_batch, device=DEV)
    ht = training.HeadTrainer(dict(zip(training.FC_KEYS, head_w)), P, max_batch=max_batch, device=DEV)
    return ct, ht


def _snapshot(ct, ht):
    mom = [ct.moments(i) for i in range(4)]
    hm = [ht.moments(l) for l in range(3)]
    return dict(cw=ct.weights(), cm=[m[0] for m in mom], cv=[m[1] for m in mom], t=mom[0][2], w=ht.weights(),
                m=[a for mm in hm for a in (mm[0], mm[2])], v=[a for mm in hm for a in (mm[1], mm[3])], ht=hm[0][4])


def _run_gpu(ct, ht, table, targets, batches, lrs, eps=EPS, input_grad=True):
    """The joint step of fine_tune_head(train_last_conv=True) per batch -> (outs, snapshots) shaped like
    train_conv_reference.run_steps'. input_grad=False: head steps only, on the conv block's output."""
    d_table, d_tgt = torch.from_numpy(table).to(DEV), torch.from_numpy(targets).to(DEV)
    outs, snaps = [], []
    for idx, lr in zip(batches, lrs):
        F = ct.forward(d_table, idx)
        y = ht.forward(F)
        _, dy = ht.loss(y, d_tgt, idx)
        out = dict(F=F.cpu().numpy())
        if input_grad:
            dfeat = ht.input_grad(dy)
            ct.step(d_table, idx, dfeat, lr=lr, eps=eps)
            out['dfeat'] = dfeat.cpu().numpy()
        ht.step(F, None, dy, lr=lr, eps=eps)
        outs.append(out)
        snaps.append(_snapshot(ct, ht))
    return outs, snaps


def _judge(outs, snaps, args, steps, label, eps=EPS):
    failures = []
    cr.judge_restarted(outs, snaps, args, steps, label, eps=eps, log=print, collect=failures)
    for s in steps:
        assert snaps[s]['t'] == s + 1 and snaps[s]['ht'] == s + 1
    assert not failures, f'{len(failures)} comparisons failed:\n' + '\n'.join(failures[:10])


def _case(Ci, Co, H, W, head, n=70, seed=None):
    seed = Ci * 1000 + Co if seed is None else seed
    conv = cr.synth_block(Ci, Co, seed, scale=2.0)
    head_w = tr.synth_head(Co * H * W, *head, seed=seed + 1, scale=3.0)
    table, tgt = cr.synth_inputs(n, Ci, H, W, seed + 2)
    return conv, head_w, (Ci, H, W), table, tgt


@pytest.fixture(scope='module')
def small_cases():
    return {dims: _case(*dims[:4], dims[4:]) for dims in ((3, 8, 5, 5, 72, 40), (5, 41, 10, 10, 130, 68))}


def _batches(B, n, steps=5):
    rng = np.random.default_rng(B)
    batches = [rng.integers(0, n, B)[::-1].copy() for _ in range(steps)]       # with repetition, out of order
    if B > 1:
        batches[0][1] = batches[0][0]
    return batches


# ------------------------------------------------------------------------------------------------ small awkward blocks
@pytest.mark.parametrize('B', [1, 3, 32, 33, 64])
@pytest.mark.parametrize('dims', [(3, 8, 5, 5, 72, 40), (5, 41, 10, 10, 130, 68)])
def test_small_joint_steps(small_cases, dims, B):
    """No size is a multiple of the kernels' tiles; the batch rows repeat and come out of order. F, the input gradient and
    every updated tensor and moment of both trainers after 1 step and after 5."""
    conv, head_w, shape, table, tgt = small_cases[dims]
    batches = _batches(B, len(table))
    lrs = [LR * 0.9 ** s for s in range(5)]
    ct, ht = _trainers(conv, head_w, shape, max_batch=64)
    outs, snaps = _run_gpu(ct, ht, table, tgt, batches, lrs)
    _judge(outs, snaps, (conv, head_w, shape, table, tgt, batches, LAM, lrs, WD), (0, 4), f'{dims} B={B}')


EDGES = [(7, 64, 4, 4, 4),       # 9 Ci = 63: one column short of a wgrad workgroup; Co = 64; r = 64: whole tiles
         (8, 65, 5, 13, 1),      # 9 Ci = 72; Co = 65; r = 65: one past each
         (16, 8, 15, 17, 1),     # 9 Ci = 144: nine whole depth tiles; r = 255: one short of a pass of conv_bn_back_k
         (2, 8, 16, 16, 1),      # r = 256: one pass exactly
         (2, 8, 17, 16, 1),      # r = 272: a second pass
         (2, 8, 4, 4, 64),       # r = 1024: 64 runs of one tile
         (2, 8, 5, 5, 41)]       # r = 1025: 33 runs of two tiles, the last one short


@pytest.mark.parametrize('edge', EDGES, ids=lambda e: 'x'.join(map(str, e)))
def test_tile_edges(edge):
    """One joint step on either side of every tile edge (module docstring), with a head 32 -> 24 whose input gradient is
    one slab written in place."""
    Ci, Co, H, W, B = edge
    conv, head_w, shape, table, tgt = _case(Ci, Co, H, W, (32, 24), n=B + 2)
    batches = [np.random.default_rng(B).permutation(B + 2)[:B]]
    ct, ht = _trainers(conv, head_w, shape, max_batch=B)
    outs, snaps = _run_gpu(ct, ht, table, tgt, batches, [LR])
    _judge(outs, snaps, (conv, head_w, shape, table, tgt, batches, LAM, [LR], WD), (0,), f'edge {edge}')


def test_one_row_map_leaves_the_taps_without_data_alone():
    """(Ci,Co,H,W) = (2,3,1,6): rows above and below the only row are padding, so only the ky = 1 taps see data. Without
    weight decay the six other taps of dW are exactly 0, and their weights, m and v stay bit-unchanged through 3 steps."""
    conv, head_w, shape, table, tgt = _case(2, 3, 1, 6, (7, 5), n=9)
    batches = _batches(4, 9, steps=3)
    ct, ht = _trainers(conv, head_w, shape, max_batch=4, wd=0.0)
    outs, snaps = _run_gpu(ct, ht, table, tgt, batches, [LR] * 3)
    _judge(outs, snaps, (conv, head_w, shape, table, tgt, batches, LAM, [LR] * 3, 0.0), (0, 2), 'one-row map')
    w, m, v = snaps[-1]['cw'][0], snaps[-1]['cm'][0], snaps[-1]['cv'][0]
    for ky in (0, 2):
        assert m[:, :, ky].tobytes() == np.zeros_like(m[:, :, ky]).tobytes() and not v[:, :, ky].any()
        assert w[:, :, ky].tobytes() == conv[0][:, :, ky].tobytes()
    assert np.abs(w[:, :, 1] - conv[0][:, :, 1]).min() > 0 and (v[:, :, 1] > 0).all()


def test_border_ring_input(small_cases):
    """The input is non-zero on the outermost ring of each map only: every product of the weight gradient sits next to
    padding, where wrap-around or a shifted window would show."""
    conv, head_w, shape, table, tgt = small_cases[(3, 8, 5, 5, 72, 40)]
    ring = cr.border_ring(table, *shape)
    assert np.abs(ring.reshape(-1, 3, 5, 5)[:, :, 1:4, 1:4]).max() == 0 and np.abs(ring).max() > 0
    batches = _batches(3, len(table), steps=1)
    ct, ht = _trainers(conv, head_w, shape, max_batch=3)
    outs, snaps = _run_gpu(ct, ht, ring, tgt, batches, [LR])
    _judge(outs, snaps, (conv, head_w, shape, ring, tgt, batches, LAM, [LR], WD), (0,), 'border ring')


def test_update_at_the_default_eps(small_cases):
    """torch's eps = 1e-8, first step, on the elements with |g| >= 1e-3: the bound of test_train_gpu.py's test of the same
    name (slope of the update in g <= 1e-4 there, f32 error of g <= 1e-4, three roundings of the update, half an ulp of
    the largest weight), for the four conv tensors and the six head tensors."""
    conv, head_w, shape, table, tgt = small_cases[(5, 41, 10, 10, 130, 68)]
    batches = [np.random.default_rng(33).integers(0, len(table), 33)]
    args = (conv, head_w, shape, table, tgt, batches, LAM, [LR], WD)
    _, _, r_snaps = cr.ref_steps(*args)
    ct, ht = _trainers(conv, head_w, shape, max_batch=33)
    _, snaps = _run_gpu(ct, ht, table, tgt, batches, [LR], eps=training.ADAM_EPS)
    for kw, km, start, names in (('cw', 'cm', conv[:4], cr.CONV_TENSORS), ('w', 'm', head_w, tr.TENSORS)):
        for i, name in enumerate(names):
            bound = 1e-8 + 2e-9 + 0.5 * float(np.spacing(np.float32(np.abs(start[i]).max())))
            well = np.abs(r_snaps[0][km][i]) >= 1e-4                         # |g| >= 1e-3
            assert well.mean() > 0.5, name
            diff = np.abs((snaps[0][kw][i] - start[i].astype(np.float64)) - (r_snaps[0][kw][i] - start[i]))[well]
            print(f'default eps | update {name} | {well.sum()} of {well.size} elements | max difference {diff.max():.3g} | bound {bound:.3g}')
            assert diff.max() <= bound, name


# ------------------------------------------------------------------------------------------------ state and determinism
def test_input_grad_leaves_the_head_step_byte_identical(small_cases):
    conv, head_w, shape, table, tgt = small_cases[(5, 41, 10, 10, 130, 68)]
    batches = _batches(33, len(table), steps=3)
    runs = []
    for with_grad in (False, True):
        ct, ht = _trainers(conv, head_w, shape, max_batch=33)
        d_table, d_tgt = torch.from_numpy(table).to(DEV), torch.from_numpy(tgt).to(DEV)
        for idx in batches:
            F = ct.forward(d_table, idx)            # the conv block never steps here: both runs feed the head the same rows
            y = ht.forward(F)
            _, dy = ht.loss(y, d_tgt, idx)
            if with_grad:
                g1 = ht.input_grad(dy)
                g2 = ht.input_grad(dy)
                assert g1.cpu().numpy().tobytes() == g2.cpu().numpy().tobytes() and g1.abs().max().item() > 0
            ht.step(F, None, dy, lr=LR, eps=EPS)
        runs.append(_snapshot(ct, ht))
    for k in ('w', 'm', 'v'):
        for a, b, name in zip(runs[0][k], runs[1][k], tr.TENSORS):
            assert a.tobytes() == b.tobytes(), (k, name)
    assert np.abs(runs[0]['w'][0] - head_w[0]).max() > LR


def test_two_pairs_of_trainers_end_byte_identical(small_cases):
    conv, head_w, shape, table, tgt = small_cases[(5, 41, 10, 10, 130, 68)]
    batches = _batches(33, len(table), steps=3)
    runs = []
    for _ in range(2):
        ct, ht = _trainers(conv, head_w, shape, max_batch=33)
        outs, snaps = _run_gpu(ct, ht, table, tgt, batches, [LR] * 3)
        runs.append((outs[-1], snaps[-1]))
    for q in ('F', 'dfeat'):
        assert runs[0][0][q].tobytes() == runs[1][0][q].tobytes(), q
    for k, names in (('cw', cr.CONV_TENSORS), ('cm', cr.CONV_TENSORS), ('cv', cr.CONV_TENSORS), ('w', tr.TENSORS),
                     ('m', tr.TENSORS), ('v', tr.TENSORS)):
        for a, b, name in zip(runs[0][1][k], runs[1][1][k], names):
            assert a.tobytes() == b.tobytes(), (k, name)
    assert np.abs(runs[0][1]['cw'][0] - conv[0]).max() > LR / 2


def test_trainers_refuse_bad_input(small_cases):
    conv, head_w, shape, table, tgt = small_cases[(3, 8, 5, 5, 72, 40)]
    ct, ht = _trainers(conv, head_w, shape, max_batch=4)
    d_table, d_tgt = torch.from_numpy(table).to(DEV), torch.from_numpy(tgt).to(DEV)
    with pytest.raises(ValueError):
        ct.forward(d_table, np.arange(5))                                   # B > max_batch
    with pytest.raises(IndexError):
        ct.forward(d_table, [0, len(table)])
    with pytest.raises(ValueError):
        ct.forward(d_table[:, :-1].contiguous(), [0])
    lib = ct._lib
    for B in (0, 5):                                                        # the library's own check of B
        assert lib.axt_conv_trainer_forward(ct._h, d_table.data_ptr(), None, B, d_table.data_ptr(), None) == -22
        assert lib.axt_head_trainer_input_grad(ht._h, d_table.data_ptr(), B, d_table.data_ptr(), None) == -22
    F = ct.forward(d_table, [0, 1, 2])
    y = ht.forward(F)
    _, dy = ht.loss(y, d_tgt, [0, 1, 2])
    dfeat = ht.input_grad(dy)
    assert tuple(dfeat.shape) == (3, 200)
    with pytest.raises(Exception, match='stashed'):
        ct.step(d_table, [0, 1], dfeat[:2].contiguous())
    with pytest.raises(Exception, match='stashed'):
        ht.input_grad(dy[:2].contiguous())
    assert ct.device_bytes > 3 * 4 * conv[0].size
    with pytest.raises(KeyError):
        training.ConvBlockTrainer({}, KEY, device=DEV)
    with pytest.raises(Exception, match='map'):
        training.ConvBlockTrainer({f'{KEY}.{k}': a for k, a in zip(training.CONV_SUFFIXES + training.CONV_STATS, conv)}, KEY,
                                  map_size=(65, 5), device=DEV)


# ------------------------------------------------------------------------------------------------ the deployed block
@pytest.fixture(scope='module')
def deployed(weights):
    import axtrack_amd
    frames = torch.from_numpy(synth.synth_frames(6, 512, 512, seed=3)).to(DEV)
    det = axtrack_amd.Detector(weights, max_batch=2, device=DEV)
    return det, frames


def test_block_features(deployed):
    """block=7 is the old call byte for byte, through Python and through the new entry point; block=6 is the detector's
    buffer 6; the old entry point itself is untouched by a block=6 call in between."""
    import helpers
    det, frames = deployed
    old = det.features_frames(frames, [(0, 0)])
    x6 = det.features_frames(frames, [(0, 0)], block=6)
    assert tuple(x6.shape) == (2, 80 * 16 * 16)
    act6 = helpers.cnn_activation(det, 6, 0, 2)
    assert x6.cpu().numpy().tobytes() == act6.tobytes() and np.abs(act6).max() > 0
    assert det.features_frames(frames, [(0, 0)], block=7).cpu().numpy().tobytes() == old.cpu().numpy().tobytes()
    new = torch.empty_like(old)
    tiles = np.zeros(2, np.int32)
    with torch.cuda.device(DEV):
        rc = det._lib.axt_cnn_block_features_frames(det._h, frames.data_ptr(), 6, 512, 512, 0, 2, tiles.ctypes.data, 1, 7,
                                                    new.data_ptr(), None)
        torch.cuda.synchronize()
    assert rc == 0 and new.cpu().numpy().tobytes() == old.cpu().numpy().tobytes()
    with pytest.raises(ValueError):
        det.features_frames(frames, [(0, 0)], block=5)
    # a table with spare rows, as fine_tune_head uses under augmentation
    table = torch.zeros((3, 80 * 16 * 16), device=DEV)
    part = det.features_frames(frames, [(0, 0)], out=table, block=6)
    assert part.data_ptr() == table.data_ptr() and part.cpu().numpy().tobytes() == act6.tobytes() and not table[2].any()


def test_forward_at_the_initial_weights_is_the_detectors_block(deployed, weights):
    """ConvBlockTrainer.forward on the block-6 table against Detector.features_frames(block=7), both against conv block 7 in
    f64 on that table: cnn_reference.judge with layer 7's bounds for a direct f32 kernel, and the two within the sum of
    their bounds of each other."""
    import cnn_reference as cnr
    det, frames = deployed
    x6 = det.features_frames(frames, [(0, 0)], block=6)
    f7 = det.features_frames(frames, [(0, 0)], block=7).cpu().numpy().reshape(2, 160, 16, 16)
    ct = training.ConvBlockTrainer(weights, max_batch=2, device=DEV)
    assert (ct.Ci, ct.Co, ct.H, ct.W) == (80, 160, 16, 16)
    got = ct.forward(x6).cpu().numpy().reshape(2, 160, 16, 16)
    h6 = x6.cpu().numpy().reshape(2, 80, 16, 16)
    ref, yard = cnr.ref_block(weights, 7, h6), cnr.yard_block(weights, 7, h6)
    c_direct, c_det = cnr.bound_for('f32_direct', 7), cnr.bound_for('f32_winograd', 7)
    r = cnr.judge(got, ref, yard, *c_direct, layer='ConvBlockTrainer.forward (conv block 7)')
    print(f'ConvBlockTrainer.forward against f64: {r[0]:.3f} (max) {r[1]:.3f} (rms) of the f32 yardstick')
    cnr.judge(f7, ref, yard, *c_det, layer='features_frames(block=7)')
    diff, allowed = np.abs(got - f7).max(), (c_direct[0] + c_det[0]) * (np.abs(yard - ref).max() + cnr.FLOOR_MAX)
    print(f'ConvBlockTrainer.forward against features_frames(block=7): max difference {diff:.3g}, allowed {allowed:.3g}')
    assert diff <= allowed


def test_full_size_joint_step(deployed, weights):
    """80 -> 160 on 16 x 16 maps with the deployed head 40960 -> 1024 -> 1024 -> 432 on the trunk features of 2 frames x 1
    tile: one joint step at B = 2 meets the same judgement as the small blocks."""
    det, frames = deployed
    x6 = det.features_frames(frames, [(0, 0)], block=6).cpu().numpy()
    P = dict(LR=LR, WEIGHT_DECAY=WD)
    ct = training.ConvBlockTrainer(weights, parameters=P, max_batch=2, device=DEV)
    ht = training.HeadTrainer(weights, P, max_batch=2, device=DEV)
    conv = [np.asarray(weights[k], np.float32) for k in ct.keys]
    head_w = [np.asarray(weights[k], np.float32) for k in training.FC_KEYS]
    lx, ly, cnt = training.label_arrays([([100, 400], [200, 30]), ([250, 251], [77, 300])])
    tgt = tr.ref_targets(lx, ly, cnt, [(0, 0)]).reshape(2, 12, 12, 4)
    batches = [np.array([1, 0])]
    outs, snaps = _run_gpu(ct, ht, x6, tgt, batches, [LR])
    _judge(outs, snaps, (conv, head_w, (80, 16, 16), x6, tgt, batches, LAM, [LR], WD), (0,), 'full size B=2')
    sd = ct.state_dict(ht.state_dict())
    assert set(sd) == set(weights)
    trained = set(ct.keys[:4]) | set(training.FC_KEYS)
    assert all(sd[k] is weights[k] for k in weights if k not in trained)
    assert all(np.array_equal(sd[k], a) for k, a in zip(ct.keys[:4], snaps[0]['cw']))
    assert all(np.array_equal(sd[k], a) for k, a in zip(training.FC_KEYS, snaps[0]['w']))


# ------------------------------------------------------------------------------------------------ end to end
def _e2e_setup(weights):
    import axtrack_amd
    E = tr.E2E
    frames = synth.synth_frames(E['T_all'], E['H'], E['W'], seed=E['frames_seed'])
    tl = axtrack_amd.Timelapse(frames, name='train', device=DEV)
    det = axtrack_amd.Detector(weights, max_batch=8, device=DEV)
    return E, tl, det, tr.e2e_labels()


def test_fine_tune_with_the_last_conv_block_end_to_end(weights, tmp_path):
    """8 items, shuffled batches of 5 and 3, 3 epochs: the history against the f64 replay of the same schedule on the GPU's
    own block-6 table; the checkpoint reloads through setup_inference's loader into a Detector that gives the trainers' own
    grids."""
    import axtrack_amd
    from axtrack_amd.interface import _load_state_dict
    from axtrack_amd.training import TRAIN_DEFAULTS
    E, tl, det, labels = _e2e_setup(weights)
    sd, hist = axtrack_amd.fine_tune_head(tl, labels, det, E['parameters'], E['epochs'], dest_dir=str(tmp_path), seed=E['seed'],
                                          train_last_conv=True)
    assert list(hist.index) == list(tr.COMPONENTS) and list(hist.columns) == list(range(E['epochs']))
    x6 = det.features_frames(tl.frames, tl.tile_yx, block=6)
    h6 = x6.cpu().numpy()
    assert h6.shape == (8, 80 * 16 * 16)
    lx, ly, cnt = training.label_arrays(labels)
    targets = tr.ref_targets(lx, ly, cnt, tl.tile_yx).reshape(-1, 12, 12, 4)
    P = dict(TRAIN_DEFAULTS, **E['parameters'])
    sched = tr.epoch_schedule(8, E['epochs'], P['BATCH_SIZE'], P['SHUFFLE'], P['DROP_LAST'], E['seed'], P['LR'], P['LR_DECAYRATE'])
    assert [len(b) for _, b, _ in sched] == [5, 3] * E['epochs']
    keys = tuple(f'{training.LAST_CONV_BLOCK}.{k}' for k in training.CONV_SUFFIXES + training.CONV_STATS)
    conv = [np.asarray(weights[k], np.float32) for k in keys]
    head_w = [np.asarray(weights[k], np.float32) for k in training.FC_KEYS]
    args = (conv, head_w, (80, 16, 16), h6, targets, [b for _, b, _ in sched], (P['L_OBJECT'], P['L_NOBJECT'], P['L_COORD_ANCHOR']),
            [lr for _, _, lr in sched], P['WEIGHT_DECAY'])
    (_, r_outs, r_snaps), (_, y_outs, _) = cr.ref_steps(*args), cr.yard_steps(*args)
    r_hist, y_hist = tr.history(sched, r_outs, E['epochs']), tr.history(sched, y_outs, E['epochs'])
    total = r_hist[tr.COMPONENTS.index('total_summed_loss')]
    print('reference total_summed_loss per epoch:', total, ' GPU:', hist.loc['total_summed_loss'].to_numpy())
    assert total[-1] < total[0]
    failures = []
    for i, name in enumerate(tr.COMPONENTS):
        try:
            tr.judge(hist.loc[name].to_numpy(), r_hist[i], y_hist[i], f'history {name}', log=print,
                     bound=cr.bound_for(f'history {name}'))
        except tr.TrainMismatch as e:
            failures.append(str(e))
    assert not failures, '\n'.join(failures)
    # both sets of tensors have moved, in the direction the reference moves them, and nothing else has
    for k, r in zip(keys[:4], r_snaps[-1]['cw']):
        moved, want = np.asarray(sd[k], np.float64) - weights[k], r - weights[k]
        assert np.abs(moved).max() > 0 and np.sum(moved * want) > 0.5 * np.sum(want * want), k
    trained = set(keys[:4]) | set(training.FC_KEYS)
    assert set(sd) == set(weights) and all(sd[k] is weights[k] for k in weights if k not in trained)
    # the checkpoint is the returned dict, and a Detector built from it gives the trainers' own grids
    back = _load_state_dict(f'{tmp_path}/E{E["epochs"] - 1:04}.pth')
    assert all(np.array_equal(back[k].numpy(), np.asarray(sd[k])) for k in sd)
    det2 = axtrack_amd.Detector(back, max_batch=8, device=DEV)
    grids = det2.detect_frames(tl.frames, tl.tile_yx)
    own = training.HeadTrainer(sd, max_batch=8, device=DEV).forward(training.ConvBlockTrainer(sd, max_batch=8, device=DEV).forward(x6))
    # The two paths differ in the kernel of conv block 7 (Winograd there, direct here): features that differ by d <= 1e-4
    # (test_forward_at_the_initial_weights_is_the_detectors_block's allowance) with independent signs move a first-layer
    # sum of 40960 products with |w| <= 1/sqrt(40960) by about d, a sigmoid by a quarter of that, and the grid by no more.
    err = (grids[:, 0] - own).abs().max().item()
    print(f'trainers against the Detector built from the checkpoint: max difference {err:.3g}')
    assert err <= 1e-4
    assert (grids - det.detect_frames(tl.frames, tl.tile_yx)).abs().max().item() > 1e-2
    tl.frame_sharded = True
    with pytest.raises(NotImplementedError):
        axtrack_amd.fine_tune_head(tl, labels, det, E['parameters'], 1, train_last_conv=True)


def test_without_the_option_fine_tune_head_is_the_loop_of_the_public_pieces(weights):
    """train_last_conv=False (and the default) against forward / loss / step on features_frames' table, written out here:
    history and all six tensors byte for byte, and every other tensor the very object that went in."""
    import axtrack_amd
    from axtrack_amd.training import TRAIN_DEFAULTS
    E, tl, det, labels = _e2e_setup(weights)
    sd, hist = axtrack_amd.fine_tune_head(tl, labels, det, E['parameters'], E['epochs'], seed=E['seed'], train_last_conv=False)
    sd_default, hist_default = axtrack_amd.fine_tune_head(tl, labels, det, E['parameters'], E['epochs'], seed=E['seed'])
    P = dict(TRAIN_DEFAULTS, **E['parameters'])
    feats = det.features_frames(tl.frames, tl.tile_yx)
    targets = training.yolo_targets(labels, tl.tile_yx, device=DEV).reshape(-1, 12, 12, 4)
    t = training.HeadTrainer(weights, P, max_batch=5, device=DEV)
    rng = np.random.default_rng(E['seed'])
    want = {}
    for epoch in range(E['epochs']):
        lr = training.learning_rate(P['LR'], P['LR_DECAYRATE'], epoch)
        rows = []
        for batch in training.epoch_batches(8, P['BATCH_SIZE'], P['SHUFFLE'], P['DROP_LAST'], rng):
            y = t.forward(feats, batch)
            comp, dy = t.loss(y, targets, batch)
            t.step(feats, batch, dy, lr=lr)
            rows.append([comp[k] for k in training.COMPONENTS])
        want[epoch] = np.mean(np.array(rows, np.float64), axis=0)
    for h in (hist, hist_default):
        assert all(h[e].to_numpy().tobytes() == want[e].tobytes() for e in range(E['epochs']))
    for out in (sd, sd_default):
        assert all(np.asarray(out[k]).tobytes() == a.tobytes() for k, a in zip(training.FC_KEYS, t.weights()))
        assert all(out[k] is weights[k] for k in weights if k not in training.FC_KEYS)

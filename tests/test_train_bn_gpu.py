"""Train-mode BatchNorm in the trained conv blocks on the GPU (csrc/train_conv.hip: bn_batch_fwd_k, bn_batch_back_k,
conv_dgrad_k<DzStored>; axtrack_amd/training.py: ConvBlockTrainer(batch_stats=), ConvStageTrainer(batch_stats=),
fine_tune_head(bn_batch_stats=)) against tests/train_bn_reference.py. Every step is judged on its own by the restarted
scheme: against one step of the f64 reference and of the f32 yardstick, restarted from what the GPU held after the step
before -- tensors, moments, running statistics and batch count. Judged: F, dfeat, dx, the batch's mean and variance, the
running statistics by their update, the count (exact), and update, m, v of every tensor; conv.bias's update is the
reference's decay-only one, its gradient being 0 by definition.

The sizes are train_bn_reference.BLOCK_CASES: n = B*H*W per channel from 2 to 6400, on either side of the 256 a workgroup
takes per pass, a one-row map, a constant channel (exact), a channel with |mu| >> sigma, negative gammas throughout."""
import numpy as np
import pytest
import torch

import helpers
import train_bn_reference as br
import train_conv_reference as cr
import train_reference as tr
import train_stage_reference as sr
from axtrack_amd import synth, training
from axtrack_amd.hotpath import conv_block_key

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
LAM, LR, WD, EPS = br.LAM, br.LR, br.WD, br.EPS
KEY = 'blk'
KEYS = ('b5', 'b6', 'b7')
ALL = training.CONV_SUFFIXES + training.CONV_STATS


# ------------------------------------------------------------------------------------------------ one block with the head
def _trainers(conv, head_w, shape, max_batch, **kw):
    Ci, H, W = shape
    sd = {f'{KEY}.{k}': a for k, a in zip(ALL, conv)}
    P = dict(LR=LR, WEIGHT_DECAY=WD)
    ct = training.ConvBlockTrainer(sd, KEY, P, map_size=(H, W), max_batch=max_batch, device=DEV, **kw)
    ht = training.HeadTrainer(dict(zip(training.FC_KEYS, head_w)), P, max_batch=max_batch, device=DEV)
    return ct, ht


def _block_snapshot(ct):
    mom = [ct.moments(i) for i in range(4)]
    st = ct.stats()
    return dict(cw=ct.weights(), cm=[m[0] for m in mom], cv=[m[1] for m in mom], t=mom[0][2],
                stats=[st['running_mean'], st['running_var']], nbt=st['num_batches_tracked'])


def _head_snapshot(ht):
    hm = [ht.moments(l) for l in range(3)]
    return dict(w=ht.weights(), m=[a for mm in hm for a in (mm[0], mm[2])], v=[a for mm in hm for a in (mm[1], mm[3])])


def _run_gpu(ct, ht, table, targets, batches, lrs, eps=EPS, input_grad=True):
    d_table, d_tgt = torch.from_numpy(table).to(DEV), torch.from_numpy(targets).to(DEV)
    outs, snaps = [], []
    for idx, lr in zip(batches, lrs):
        F = ct.forward(d_table, idx)
        st = ct.stats()
        y = ht.forward(F)
        _, dy = ht.loss(y, d_tgt, idx)
        dfeat = ht.input_grad(dy)
        out = dict(F=F.cpu().numpy(), dfeat=dfeat.cpu().numpy(), mu=st['batch_mean'], var=st['batch_var'])
        if input_grad:
            out['dx'] = ct.input_grad(dfeat).cpu().numpy()
        ct.step(d_table, idx, dfeat, lr=lr, eps=eps)
        ht.step(F, None, dy, lr=lr, eps=eps)
        outs.append(out)
        snaps.append(dict(_block_snapshot(ct), **_head_snapshot(ht)))
    return outs, snaps


@pytest.mark.parametrize('name', list(br.BLOCK_CASES))
def test_block_steps_in_batch_mode(name):
    conv, head_w, shape, table, tgt, batches, lrs, judged = br.block_case(name)
    B = len(batches[0])
    ct, ht = _trainers(conv, head_w, shape, max_batch=B, batch_stats=True)
    assert ct.stats()['num_batches_tracked'] == 0 and ct.stats()['batch_mean'] is None
    outs, snaps = _run_gpu(ct, ht, table, tgt, batches, lrs)
    failures = []
    br.judge_restarted(outs, snaps, (conv, head_w, shape, table, tgt, batches, LAM, lrs, WD), judged, name, eps=EPS, log=print,
                       collect=failures)
    assert [s['t'] for s in snaps] == [s['nbt'] for s in snaps] == list(range(1, len(batches) + 1))
    assert not failures, f'{len(failures)} comparisons failed:\n' + '\n'.join(failures[:10])
    if name == 'constant':
        Co = conv[0].shape[0]
        m = np.float32(br.MOMENTUM)
        assert outs[0]['mu'][0] == 0.5 and outs[0]['var'][0] == 0
        assert not outs[0]['F'].reshape(B, Co, -1)[:, 0].any()                  # zhat == 0, y == beta == 0
        _, _, (ys,) = br.yard_steps(conv, head_w, shape, table, tgt, batches, LAM, lrs, WD, eps=EPS)
        assert snaps[0]['stats'][1][0] == ys['stats'][1][0] == np.float32(1 - br.MOMENTUM) * conv[5][0]
        assert snaps[0]['stats'][0][0] == ys['stats'][0][0]
        # dgamma == 0: gamma's first moment is its weight decay's alone
        want = np.float32(0.1) * (np.float32(WD) * conv[2][0])
        assert abs(snaps[0]['cm'][2][0] - want) <= np.spacing(np.abs(want)), (snaps[0]['cm'][2][0], want)
    if name == 'n=2':
        assert ct.stats()['running_var'].min() > 0


def test_one_value_per_channel_is_refused_before_anything_runs():
    conv = cr.synth_block(2, 3, 1)
    head_w = tr.synth_head(3, 7, 5, seed=2)
    ct, ht = _trainers(conv, head_w, (2, 1, 1), max_batch=2, batch_stats=True)
    x = torch.ones((2, 2), device=DEV)
    before = _block_snapshot(ct)
    with pytest.raises(ValueError, match='batch statistics need more than 1 value per channel'):
        ct.forward(x, [0])
    out = torch.zeros((1, 3), device=DEV)
    assert ct._lib.axt_conv_trainer_forward(ct._h, x.data_ptr(), None, 1, out.data_ptr(), None) == -22
    torch.cuda.synchronize()
    after = _block_snapshot(ct)
    assert not out.any() and after['nbt'] == 0 and all(a.tobytes() == b.tobytes() for a, b in zip(before['stats'], after['stats']))
    with pytest.raises(Exception, match='stashed'):                          # no batch is stashed
        ct.step(x, [0], out)
    ct.forward(x, [0, 1])                                                     # n = 2 is enough
    assert ct.stats()['num_batches_tracked'] == 1
    for bad in (0.0, -0.1, 1.5):
        assert ct._lib.axt_conv_trainer_set_batch_stats(ct._h, 1, bad) == -22
        with pytest.raises(ValueError):
            _trainers(conv, head_w, (2, 1, 1), max_batch=2, batch_stats=True, momentum=bad)


def test_input_grad_repeats_and_leaves_the_step_byte_identical():
    conv, head_w, shape, table, tgt, batches, lrs, _ = br.block_case('5x41x10x10 B=33')
    runs = []
    for with_grad in (False, True):
        ct, ht = _trainers(conv, head_w, shape, max_batch=33, batch_stats=True)
        held = ct.device_bytes
        d_table = torch.from_numpy(table).to(DEV)
        dF = torch.from_numpy(np.random.default_rng(5).normal(0, 1, (33, ct.out_width)).astype(np.float32)).to(DEV)
        for idx in batches[:2]:
            ct.forward(d_table, idx)
            if with_grad:
                g1, g2 = ct.input_grad(dF), ct.input_grad(dF)
                assert g1.cpu().numpy().tobytes() == g2.cpu().numpy().tobytes() and g1.abs().max().item() > 0
            ct.step(d_table, idx, dF, lr=LR, eps=EPS)
        assert ct.device_bytes == held
        s = _block_snapshot(ct)
        runs.append(s['cw'] + s['cm'] + s['cv'] + s['stats'])
    assert all(a.tobytes() == b.tobytes() for a, b in zip(*runs))
    assert np.abs(runs[0][0] - conv[0]).max() > LR / 2


def test_two_trainers_end_byte_identical():
    conv, head_w, shape, table, tgt, batches, lrs, _ = br.block_case('5x41x10x10 B=33')
    runs = []
    for _ in range(2):
        ct, ht = _trainers(conv, head_w, shape, max_batch=33, batch_stats=True)
        outs, snaps = _run_gpu(ct, ht, table, tgt, batches, lrs)
        runs.append((outs[-1], snaps[-1]))
    for q in ('F', 'dfeat', 'dx', 'mu', 'var'):
        assert runs[0][0][q].tobytes() == runs[1][0][q].tobytes(), q
    for k in ('cw', 'cm', 'cv', 'stats', 'w', 'm', 'v'):
        assert all(a.tobytes() == b.tobytes() for a, b in zip(runs[0][1][k], runs[1][1][k])), k
    assert runs[0][1]['nbt'] == runs[1][1]['nbt'] == 3
    assert np.abs(runs[0][1]['stats'][0] - conv[4]).max() > 0


def test_mode_off_is_the_trainer_it_was():
    """Never switched, switched off explicitly, and switched on and off again before the first forward: the same bytes; the
    first holds the memory it held, and its statistics read back as they went in."""
    conv, head_w, shape, table, tgt, batches, lrs, _ = br.block_case('5x41x10x10 B=33')
    runs, held = [], []
    for mode in ('never', 'off', 'on_off'):
        ct, ht = _trainers(conv, head_w, shape, max_batch=33)
        held.append(ct.device_bytes)
        if mode != 'never':
            for on in ((1, 0) if mode == 'on_off' else (0,)):
                assert ct._lib.axt_conv_trainer_set_batch_stats(ct._h, on, 0.1) == 0
        d_table, d_tgt = torch.from_numpy(table).to(DEV), torch.from_numpy(tgt).to(DEV)
        res = []
        for idx, lr in zip(batches, lrs):
            F = ct.forward(d_table, idx)
            y = ht.forward(F)
            _, dy = ht.loss(y, d_tgt, idx)
            dfeat = ht.input_grad(dy)
            res += [F.cpu().numpy(), ct.input_grad(dfeat).cpu().numpy()]
            ct.step(d_table, idx, dfeat, lr=lr, eps=EPS)
            ht.step(F, None, dy, lr=lr, eps=EPS)
        s = _block_snapshot(ct)
        assert s['nbt'] == 0 and s['stats'][0].tobytes() == conv[4].tobytes() and s['stats'][1].tobytes() == conv[5].tobytes()
        assert ct.stats()['batch_mean'] is None
        runs.append(res + s['cw'] + s['cm'] + s['cv'])
        if mode != 'on_off':
            assert ct.device_bytes == held[-1]
        else:
            assert ct.device_bytes == held[-1] + 4 * 4 * conv[0].shape[0]
        sd = ct.state_dict()
        assert all(sd[f'{KEY}.{k}'] is ct._sd[f'{KEY}.{k}'] for k in training.CONV_STATS)
    assert held[0] == held[1] == held[2]
    for other in runs[1:]:
        assert all(a.tobytes() == b.tobytes() for a, b in zip(runs[0], other))


def test_state_dict_keeps_dtype_and_container():
    conv, head_w, shape, table, tgt, batches, lrs, _ = br.block_case('3x8x5x5 B=3')
    sd = {f'{KEY}.{k}': a for k, a in zip(ALL, conv)}
    sd[f'{KEY}.batchnorm.running_mean'] = torch.from_numpy(conv[4]).double()
    sd[f'{KEY}.batchnorm.num_batches_tracked'] = torch.tensor(7)
    ct = training.ConvBlockTrainer(sd, KEY, map_size=shape[1:], max_batch=3, device=DEV, batch_stats=True, momentum=0.5)
    d_table = torch.from_numpy(table).to(DEV)
    for idx in batches[:2]:
        ct.forward(d_table, idx)
    out, st = ct.state_dict(), ct.stats()
    rm, rv, n = (out[f'{KEY}.batchnorm.{k}'] for k in ('running_mean', 'running_var', 'num_batches_tracked'))
    assert isinstance(rm, torch.Tensor) and rm.dtype == torch.float64 and np.array_equal(rm.numpy(), st['running_mean'].astype(np.float64))
    assert isinstance(rv, np.ndarray) and rv.dtype == np.float32 and np.array_equal(rv, st['running_var'])
    assert isinstance(n, torch.Tensor) and n.dtype == torch.int64 and int(n) == 9
    assert int(sd[f'{KEY}.batchnorm.num_batches_tracked']) == 7 and not np.array_equal(rv, conv[5])
    del sd[f'{KEY}.batchnorm.num_batches_tracked']
    n = ct.state_dict()[f'{KEY}.batchnorm.num_batches_tracked']
    assert isinstance(n, np.ndarray) and n.dtype == np.int64 and int(n) == 2


# ------------------------------------------------------------------------------------------------ the stage
def _stage_trainers(convs, head_w, shape, max_batch, depth=3, batch_stats=True, weights=None):
    P = dict(LR=LR, WEIGHT_DECAY=WD)
    if weights is not None:
        st = training.ConvStageTrainer(weights, depth, P, max_batch=max_batch, device=DEV, batch_stats=batch_stats)
        return st, training.HeadTrainer(weights, P, max_batch=max_batch, device=DEV)
    sd = {f'{key}.{k}': a for key, conv in zip(KEYS, convs) for k, a in zip(ALL, conv)}
    sd.update(zip(training.FC_KEYS, head_w))
    st = training.ConvStageTrainer(sd, depth, P, max_batch=max_batch, device=DEV, block_keys=KEYS, map_size=shape[1:],
                                   batch_stats=batch_stats)
    return st, training.HeadTrainer(sd, P, max_batch=max_batch, device=DEV)


def _run_stage(st, ht, table, targets, batches, lrs, eps=EPS):
    d_table, d_tgt = torch.from_numpy(table).to(DEV), torch.from_numpy(targets).to(DEV)
    outs, snaps = [], []
    for idx, lr in zip(batches, lrs):
        Fo = st.forward(d_table, idx)
        f5, f6, pooled, _ = helpers.stage_kept(st)
        stats = [b.stats() for b in st.blocks]
        y = ht.forward(Fo)
        _, dy = ht.loss(y, d_tgt, idx)
        dfeat = ht.input_grad(dy)
        grads = st.backward_and_step(d_table, idx, dfeat, lr=lr, eps=eps)
        ht.step(Fo, None, dy, lr=lr, eps=eps)
        out = dict(F5=f5, F6=f6, pooled=pooled, F=Fo, dfeat=dfeat)
        out.update({k: grads[g] for k, g in (('dpooled', 'p6'), ('dF6', 'f6'), ('dx6', 'f5')) if g in grads})
        out = {k: v.cpu().numpy() for k, v in out.items()}
        for name, s, trained in zip(sr.BLOCKS, stats, st.trained):
            if trained:
                out[f'mu {name}'], out[f'var {name}'] = s['batch_mean'], s['batch_var']
        outs.append(out)
        snap = _head_snapshot(ht)
        snap.update({name: _block_snapshot(b) for name, b in zip(sr.BLOCKS, st.blocks)})
        snaps.append(snap)
    return outs, snaps


def _judge_stage(outs, snaps, args, steps, label, depth=3):
    failures = []
    br.judge_stage_restarted(outs, snaps, args, steps, depth, label, eps=EPS, log=print, collect=failures)
    for s in steps:
        want = [s + 1 if i >= 3 - depth else 0 for i in range(3)]
        assert [snaps[s][n]['t'] for n in sr.BLOCKS] == want and [snaps[s][n]['nbt'] for n in sr.BLOCKS] == want
    assert not failures, f'{len(failures)} comparisons failed:\n' + '\n'.join(failures[:10])


@pytest.mark.parametrize('B', [3, 33])
def test_stage_steps_in_batch_mode(B):
    """Three depth-3 steps of the 'unequal' stage, steps 1 and 3 judged, the pool's winners taken from the GPU's own F6."""
    convs, head_w, shape, table, tgt, batches, lrs = br.stage_case(B)
    st, ht = _stage_trainers(convs, head_w, shape, max_batch=B)
    outs, snaps = _run_stage(st, ht, table, tgt, batches, lrs)
    _judge_stage(outs, snaps, (convs, head_w, shape, table, tgt, batches, LAM, lrs, WD), (0, 2), f'unequal B={B}')


def test_depth_two_leaves_block_five_and_its_statistics_alone():
    convs, head_w, shape, table, tgt, batches, lrs = br.stage_case(3)
    st, ht = _stage_trainers(convs, head_w, shape, max_batch=3, depth=2)
    assert [b.batch_stats for b in st.blocks] == [False, True, True]
    outs, snaps = _run_stage(st, ht, table, tgt, batches, lrs)
    _judge_stage(outs, snaps, (convs, head_w, shape, table, tgt, batches, LAM, lrs, WD), (0, 2), 'depth 2', depth=2)
    b5 = snaps[-1]['b5']
    assert all(a.tobytes() == b.tobytes() for a, b in zip(b5['cw'] + b5['stats'], convs[0])) and b5['nbt'] == 0
    ev, _ = _stage_trainers(convs, head_w, shape, max_batch=3, depth=2, batch_stats=False)
    for s, idx in enumerate(batches):
        ev.forward(torch.from_numpy(table).to(DEV), idx)
        assert helpers.stage_kept(ev)[0].cpu().numpy().tobytes() == outs[s]['F5'].tobytes()
    assert helpers.stage_kept(ev)[1].cpu().numpy().tobytes() != outs[-1]['F6'].tobytes()
    sd = st.state_dict(ht.state_dict())
    assert all(sd[f'b5.{k}'] is st._sd[f'b5.{k}'] for k in ALL) and 'b5.batchnorm.num_batches_tracked' not in sd
    assert int(sd['b6.batchnorm.num_batches_tracked']) == int(sd['b7.batchnorm.num_batches_tracked']) == 3
    assert np.abs(sd['b6.batchnorm.running_var'] - convs[1][5]).max() > 0


def test_full_size_stage_step_in_batch_mode(weights):
    """The deployed stage and head on the trunk features of 2 frames x 1 tile: one depth-3 step at B = 2. Frames of seed 4:
    with seed 3, which the eval-mode tests use, two of the 410 000 y of the f64 reference lie within the margin of 0 (the
    side condition of train_bn_reference, which the judge asserts)."""
    import axtrack_amd
    frames = torch.from_numpy(synth.synth_frames(6, 512, 512, seed=4)).to(DEV)
    det = axtrack_amd.Detector(weights, max_batch=2, device=DEV)
    x4 = det.features_frames(frames, [(0, 0)], block=4).cpu().numpy()
    st, ht = _stage_trainers(None, None, None, max_batch=2, weights=weights)
    convs = [[np.asarray(weights[k], np.float32) for k in b.keys] for b in st.blocks]
    head_w = [np.asarray(weights[k], np.float32) for k in training.FC_KEYS]
    lx, ly, cnt = training.label_arrays([([100, 400], [200, 30]), ([250, 251], [77, 300])])
    tgt = tr.ref_targets(lx, ly, cnt, [(0, 0)]).reshape(2, 12, 12, 4)
    batches = [np.array([1, 0])]
    outs, snaps = _run_stage(st, ht, x4, tgt, batches, [LR])
    _judge_stage(outs, snaps, (convs, head_w, (80, 32, 32), x4, tgt, batches, LAM, [LR], WD), (0,), 'full size B=2')


# ------------------------------------------------------------------------------------------------ end to end
def _e2e_setup(weights):
    import axtrack_amd
    E = tr.E2E
    frames = synth.synth_frames(E['T_all'], E['H'], E['W'], seed=E['frames_seed'])
    labels = [(x, y, [0]) for x, y in tr.e2e_labels()]
    tl = axtrack_amd.Timelapse(frames, name='train', device=DEV, labels=labels)
    test = axtrack_amd.Timelapse(frames[:8], name='test', device=DEV, labels=labels[:4])
    return E, tl, test, axtrack_amd.Detector(weights, max_batch=8, device=DEV)


def _same(a, b):
    return set(a) == set(b) and all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in a)


def test_fine_tune_with_batch_statistics_end_to_end(weights, tmp_path):
    import axtrack_amd
    from axtrack_amd.interface import _load_state_dict
    E, tl, test, det = _e2e_setup(weights)
    kw = dict(model=det, parameters=E['parameters'], epochs=E['epochs'], seed=E['seed'], train_conv_blocks=3)
    sd, hist = axtrack_amd.fine_tune_head(tl, dest_dir=str(tmp_path), test_timelapse=test, bn_batch_stats=True, **kw)
    steps = 2 * E['epochs']                                                   # batches of 5 and 3 per epoch
    assert np.isfinite(hist.to_numpy()).all() and list(hist.columns) == list(range(E['epochs']))
    for i in training.STAGE_BLOCKS:
        key = conv_block_key(i)
        for k in training.CONV_STATS:
            assert np.abs(np.asarray(sd[f'{key}.{k}'], np.float64) - np.asarray(weights[f'{key}.{k}'], np.float64)).max() > 0, (key, k)
            assert np.asarray(sd[f'{key}.{k}']).dtype == np.asarray(weights[f'{key}.{k}']).dtype
        k = f'{key}.{training.CONV_COUNTER}'
        assert int(np.asarray(sd[k])) == (int(np.asarray(weights[k])) if k in weights else 0) + steps
    frozen = [k for k in weights if not any(k.startswith(conv_block_key(i) + '.') for i in training.STAGE_BLOCKS)
              and k not in training.FC_KEYS]
    assert frozen and all(sd[k] is weights[k] for k in frozen)
    metrics = hist.attrs['metrics']
    assert list(metrics.columns) == [(0, 'train'), (0, 'test')] and ((metrics.to_numpy() >= 0) & (metrics.to_numpy() <= 1)).all()
    # the checkpoint is the returned dict, and loads into a Detector that reads the moved statistics
    back = _load_state_dict(f'{tmp_path}/E{E["epochs"] - 1:04}.pth')
    assert set(back) == set(sd) and all(np.array_equal(back[k].numpy(), np.asarray(sd[k])) for k in sd)
    grids = axtrack_amd.Detector(back, max_batch=8, device=DEV).detect_frames(tl.frames, tl.tile_yx)
    assert torch.isfinite(grids).all()
    assert (grids - axtrack_amd.Detector(sd, max_batch=8, device=DEV).detect_frames(tl.frames, tl.tile_yx)).abs().max().item() == 0
    assert (grids - det.detect_frames(tl.frames, tl.tile_yx)).abs().max().item() > 1e-2
    # two runs with one seed; and the option off or omitted is the run it was
    sd2, hist2 = axtrack_amd.fine_tune_head(tl, bn_batch_stats=True, **kw)
    assert _same(sd, sd2) and hist.to_numpy().tobytes() == hist2.to_numpy().tobytes()
    sd_off, hist_off = axtrack_amd.fine_tune_head(tl, bn_batch_stats=False, **kw)
    sd_def, hist_def = axtrack_amd.fine_tune_head(tl, **kw)
    assert _same(sd_off, sd_def) and hist_off.to_numpy().tobytes() == hist_def.to_numpy().tobytes()
    assert hist_off.to_numpy().tobytes() != hist.to_numpy().tobytes()
    assert all(sd_def[f'{conv_block_key(i)}.{k}'] is weights[f'{conv_block_key(i)}.{k}'] for i in training.STAGE_BLOCKS
               for k in training.CONV_STATS)


def test_batch_statistics_with_the_head_alone_are_refused_before_any_gpu_work(weights):
    import axtrack_amd

    class Untouchable:
        frame_sharded = False

        def __getattr__(self, name):
            raise AssertionError(f'the timelapse was touched ({name}) before the arguments were checked')

    for kw in (dict(), dict(train_conv_blocks=0), dict(train_last_conv=False)):
        with pytest.raises(ValueError, match='bn_batch_stats'):
            axtrack_amd.fine_tune_head(Untouchable(), [], weights, bn_batch_stats=True, **kw)
    with pytest.raises(ValueError, match='bn_momentum'):
        axtrack_amd.fine_tune_head(Untouchable(), [], weights, train_conv_blocks=1, bn_batch_stats=True, bn_momentum=0.0)

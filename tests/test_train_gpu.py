"""The head trainer on the GPU (csrc/train.hip, axtrack_amd/training.py) against tests/train_reference.py: YOLO targets bit
for bit, and forward pass, loss, gradient, updated weights and Adam moments under the judge (error against the f64
reference no more than a small multiple of what plain f32 on the CPU makes on the same input)."""
import numpy as np
import pytest
import torch

import train_reference as tr
from axtrack_amd import synth, training

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
LAM = (49.5, 1.0, 49.5)
LR, WD = 1e-2, 0.05                 # large enough that an update is far above the judge's absolute floors
# Adam's eps in the judged steps. At torch's default 1e-8 the first updates are lr * g / (|g| + 1e-8): -lr * sign(g) for
# nearly every element, and for the few of half a million whose gradient cancels to |g| ~ 1e-8 a function with slope
# lr / (4 eps) = 250,000 -- an f32 rounding of g (1e-9) decides between -lr and +lr, in the CPU yardstick exactly as on
# the GPU (its largest error on such a tensor is 0.06 ... 2 lr), and the weight that moved the other way sends the later
# steps of the two runs apart. The ratio of two such draws measures luck. With eps = 1e-3 the update is a function of g
# with slope <= lr / eps = 10, so the judge sees the arithmetic; m and v do not depend on eps. The update at the default
# eps is checked by test_update_at_the_default_eps on the elements where it is well-conditioned.
EPS = 1e-3


def _trainer(w, max_batch, lr=LR, wd=WD):
    sd = dict(zip(training.FC_KEYS, w))
    return training.HeadTrainer(sd, dict(LR=lr, WEIGHT_DECAY=wd), max_batch=max_batch, device=DEV)


def _snapshot(t):
    w = t.weights()
    mom = [t.moments(l) for l in range(3)]
    return dict(w=w, m=[a for mm in mom for a in (mm[0], mm[2])], v=[a for mm in mom for a in (mm[1], mm[3])],
                t=mom[0][4])


def _run_gpu(t, feats, targets, batches, lrs, eps=EPS):
    """forward / loss / step per batch -> (outs, snapshots) shaped like train_reference.run_steps'."""
    d_feats, d_tgt = torch.from_numpy(feats).to(DEV), torch.from_numpy(targets).to(DEV)
    outs, snaps = [], []
    for idx, lr in zip(batches, lrs):
        y = t.forward(d_feats, idx)
        comps, dy = t.loss(y, d_tgt, idx)
        t.step(d_feats, idx, dy, lr=lr, eps=eps)
        outs.append(dict(y=y.reshape(len(idx), -1).cpu().numpy(), comps=np.array([comps[k] for k in tr.COMPONENTS]),
                         dy=dy.reshape(len(idx), -1).cpu().numpy()))
        snaps.append(_snapshot(t))
    return outs, snaps


def _judge_steps(outs, snaps, ref, yard, w0, steps, label, targets):
    (_, r_outs, r_snaps), (_, y_outs, y_snaps) = ref, yard
    failures = []

    def one(got, r, y, name):
        try:
            tr.judge(got, r, y, f'{name} @{label}', log=print)
        except tr.TrainMismatch as e:
            failures.append(str(e))

    for s in steps:
        one(outs[s]['y'], r_outs[s]['y'], y_outs[s]['y'], 'y')
        # The loss and its gradient are judged on the grids the GPU itself produced, as tests/cnn_reference.py feeds every
        # layer the GPU's own input: a component is ONE number that sums 432 B squared errors weighted up to 49.5, so the f32
        # rounding of the forward pass moves it by several of its own ulps, in the yardstick's chain and in the GPU's
        # alike, and the ratio of two such single draws says nothing about the loss kernel.
        tgt = targets[s]
        for dt, store in ((torch.float64, 'r'), (torch.float32, 'y')):
            c, d = tr.loss(torch.from_numpy(outs[s]['y']).to(dt), torch.from_numpy(tgt).to(dt), LAM)
            if store == 'r':
                r_c, r_d = c.numpy(), d.numpy()
            else:
                y_c, y_d = c.numpy(), d.numpy()
        one(outs[s]['comps'], r_c, y_c, 'comps')
        one(outs[s]['dy'], r_d, y_d, 'dy')
        assert snaps[s]['t'] == s + 1
        for i, name in enumerate(tr.TENSORS):
            w0_64 = np.asarray(w0[i], np.float64)
            one(snaps[s]['w'][i] - w0_64, r_snaps[s]['w'][i] - w0_64, y_snaps[s]['w'][i] - w0_64, f'update {name}')
            one(snaps[s]['m'][i], r_snaps[s]['m'][i], y_snaps[s]['m'][i], f'm {name}')
            one(snaps[s]['v'][i], r_snaps[s]['v'][i], y_snaps[s]['v'][i], f'v {name}')
    assert not failures, f'{len(failures)} comparisons failed:\n' + '\n'.join(failures[:10])


# ------------------------------------------------------------------------------------------------ targets
def test_yolo_targets_bit_equal_and_repeatable():
    """A 1024 x 700 frame: 4 tiles, tile (1, 0) not kept. Labels at 0, 511 and 512, in the last row and column, a negative
    'missing' entry, one in the dropped tile, two in one cell, cap larger than any count, an empty frame."""
    tiles = [(0, 0), (0, 1), (1, 1)]
    xs = [[0, 511, 512, 699, -1, 100, 300, 301, 511, 0], [], [640, 20, 20, 600]]
    ys = [[0, 511, 512, 1023, -1, 600, 100, 101, 0, 511], [], [30, 1000, 400, 1023]]
    cap = 13
    lx, ly = np.full((3, cap), -7, np.int32), np.full((3, cap), -7, np.int32)
    for f, (x, y) in enumerate(zip(xs, ys)):
        lx[f, :len(x)], ly[f, :len(y)] = x, y
    cnt = np.array([len(x) for x in xs], np.int32)
    want = tr.ref_targets(lx, ly, cnt, tiles)
    assert want[0, 0, 7, 2].tolist()[0::3] == [1.0, 7.0] and want[..., 0].sum() == 10      # label 7 won cell (7, 2); (100, 600) and (20, 1000) are dropped
    got = training.yolo_targets((lx, ly, cnt), tiles, device=DEV)
    assert tuple(got.shape) == (3, 3, 12, 12, 4)
    assert got.cpu().numpy().tobytes() == want.tobytes()
    again = training.yolo_targets((lx, ly, cnt), tiles, device=DEV)
    assert again.cpu().numpy().tobytes() == got.cpu().numpy().tobytes()
    # the list format of set_groundtruth gives the same targets
    lists = training.yolo_targets([(x, y) for x, y in zip(xs, ys)], tiles, device=DEV)
    assert lists.cpu().numpy().tobytes() == want.tobytes()


# ------------------------------------------------------------------------------------------------ small awkward heads
@pytest.fixture(scope='module')
def small_cases():
    """Per head size: weights, tables and -- computed once -- nothing else; the references are per batch size."""
    out = {}
    for dims in ((200, 72, 40), (4100, 130, 68)):
        w = tr.synth_head(*dims, seed=dims[0], scale=3.0)
        feats, tgt = tr.synth_table(70, dims[0], seed=dims[1])
        out[dims] = (w, feats, tgt)
    return out


@pytest.mark.parametrize('B', [1, 3, 32, 33, 64])
@pytest.mark.parametrize('dims', [(200, 72, 40), (4100, 130, 68)])
def test_small_head_steps(small_cases, dims, B):
    """Neither head size is a multiple of the kernels' tiles; the batch rows repeat and come out of order. Forward, the
    five loss components, dY and every updated tensor and moment after 1 step and after 5."""
    w, feats, tgt = small_cases[dims]
    rng = np.random.default_rng(B)
    batches = [rng.integers(0, 70, B)[::-1].copy() for _ in range(5)]      # with repetition
    if B > 1:
        batches[0][1] = batches[0][0]
    lrs = [LR * 0.9 ** s for s in range(5)]
    args = (w, feats, tgt, batches, LAM, lrs, WD)
    ref, yard = tr.ref_steps(*args, eps=EPS), tr.yard_steps(*args, eps=EPS)
    t = _trainer(w, max_batch=64)
    outs, snaps = _run_gpu(t, feats, tgt, batches, lrs)
    _judge_steps(outs, snaps, ref, yard, w, (0, 4), f'{dims} B={B}', [tgt[b] for b in batches])


def test_trainer_refuses_bad_input(small_cases):
    w, feats, tgt = small_cases[(200, 72, 40)]
    t = _trainer(w, max_batch=4)
    d_feats = torch.from_numpy(feats).to(DEV)
    with pytest.raises(ValueError):
        t.forward(d_feats, np.arange(5))
    with pytest.raises(IndexError):
        t.forward(d_feats, [0, 70])
    y = t.forward(d_feats, [0, 1, 2])
    _, dy = t.loss(y, torch.from_numpy(tgt).to(DEV), [0, 1, 2])
    with pytest.raises(Exception, match='stashed'):
        t.step(d_feats, [0, 1], dy[:2].contiguous())
    assert t.device_bytes > 3 * 4 * (200 * 72 + 72 * 40 + 40 * 432)
    with pytest.raises(Exception, match='NOUT'):
        training.HeadTrainer(dict(zip(training.FC_KEYS, tr.synth_head(200, 72, 40, 1)[:4] + [np.zeros((10, 40), np.float32), np.zeros(10, np.float32)])), device=DEV)


def test_three_steps_are_byte_identical_between_two_trainers(small_cases):
    w, feats, tgt = small_cases[(4100, 130, 68)]
    rng = np.random.default_rng(1)
    batches = [rng.integers(0, 70, 33) for _ in range(3)]
    runs = []
    for _ in range(2):
        t = _trainer(w, max_batch=33)
        _, snaps = _run_gpu(t, feats, tgt, batches, [LR] * 3)
        runs.append(snaps[-1])
    for k in ('w', 'm', 'v'):
        for a, b, name in zip(runs[0][k], runs[1][k], tr.TENSORS):
            assert a.tobytes() == b.tobytes(), (k, name)
    assert np.abs(runs[0]['w'][0] - w[0]).max() > LR


def test_update_at_the_default_eps(small_cases):
    """torch's eps = 1e-8, first step: update = lr g / (|g| + eps) with g = m / (1 - beta1). Where |g| >= 1e-3 its slope in
    g is lr eps / g^2 <= 1e-4, so even the worst-case f32 error of g (33 products whose magnitudes sum to less than 50:
    33 * 2^-24 * 50 = 1e-4) moves it by <= 1e-8; the three roundings of step * (m / denom) add 3 * 2^-24 * lr = 2e-9, and
    the rounding of w - update half an ulp of the largest |w|: that sum bounds the GPU's distance from the f64 update."""
    w, feats, tgt = small_cases[(4100, 130, 68)]
    batches = [np.random.default_rng(33).integers(0, 70, 33)]
    _, _, r_snaps = tr.ref_steps(w, feats, tgt, batches, LAM, [LR], WD)
    t = _trainer(w, max_batch=33)
    _, snaps = _run_gpu(t, feats, tgt, batches, [LR], eps=training.ADAM_EPS)
    for i, name in enumerate(tr.TENSORS):
        bound = 1e-8 + 2e-9 + 0.5 * float(np.spacing(np.float32(np.abs(w[i]).max())))
        well = np.abs(r_snaps[0]['m'][i]) >= 1e-4                          # |g| >= 1e-3
        assert well.mean() > 0.5, name
        diff = np.abs((snaps[0]['w'][i] - w[i].astype(np.float64)) - (r_snaps[0]['w'][i] - w[i]))[well]
        print(f'default eps | update {name} | {well.sum()} of {well.size} elements | max difference {diff.max():.3g} | bound {bound:.3g}')
        assert diff.max() <= bound, name


# ------------------------------------------------------------------------------------------------ the deployed head
def test_full_size_head_step(weights):
    """40960 -> 1024 -> 1024 -> 432 on the trunk features of 2 frames x 1 tile: the forward pass is detect_frames', and one
    step at B = 2 meets the same judgement as the small heads."""
    import axtrack_amd
    frames = torch.from_numpy(synth.synth_frames(6, 512, 512, seed=3)).to(DEV)
    det = axtrack_amd.Detector(weights, max_batch=2, device=DEV)
    feats = det.features_frames(frames, [(0, 0)])
    assert tuple(feats.shape) == (2, 40960)
    grids = det.detect_frames(frames, [(0, 0)])
    w = [np.asarray(weights[k], np.float32) for k in training.FC_KEYS]
    t = training.HeadTrainer(weights, dict(LR=LR, WEIGHT_DECAY=WD), max_batch=2, device=DEV)
    y = t.forward(feats)
    err = (y - grids[:, 0]).abs().max().item()
    print(f'HeadTrainer.forward against detect_frames: max difference {err:.3g}')
    assert err <= 1e-5
    assert t.device_bytes >= 3 * 4 * (40960 * 1024 + 1024 * 1024 + 432 * 1024)
    lx, ly, cnt = training.label_arrays([([100, 400], [200, 30]), ([250, 251], [77, 300])])
    tgt = tr.ref_targets(lx, ly, cnt, [(0, 0)]).reshape(2, 12, 12, 4)
    h_feats = feats.cpu().numpy()
    batches = [np.array([1, 0])]
    args = (w, h_feats, tgt, batches, LAM, [LR], WD)
    ref, yard = tr.ref_steps(*args, eps=EPS), tr.yard_steps(*args, eps=EPS)
    outs, snaps = _run_gpu(t, h_feats, tgt, batches, [LR])
    _judge_steps(outs, snaps, ref, yard, w, (0,), 'full size B=2', [tgt[b] for b in batches])
    sd = t.state_dict()
    assert set(sd) == set(weights) and all(sd[k] is weights[k] for k in weights if k not in training.FC_KEYS)
    assert all(np.array_equal(sd[k], a) for k, a in zip(training.FC_KEYS, snaps[0]['w']))


# ------------------------------------------------------------------------------------------------ end to end
def test_fine_tune_head_end_to_end(weights, tmp_path):
    import axtrack_amd
    from axtrack_amd.interface import _load_state_dict
    E = tr.E2E
    frames = synth.synth_frames(E['T_all'], E['H'], E['W'], seed=E['frames_seed'])
    tl = axtrack_amd.Timelapse(frames, name='train', device=DEV)
    det = axtrack_amd.Detector(weights, max_batch=8, device=DEV)
    labels = tr.e2e_labels()
    sd, hist = axtrack_amd.fine_tune_head(tl, labels, det, E['parameters'], E['epochs'], dest_dir=str(tmp_path), seed=E['seed'])
    assert list(hist.index) == list(tr.COMPONENTS) and list(hist.columns) == list(range(E['epochs']))
    # the f64 replay of the same batch order on the GPU's own trunk features, and the same in f32 on the CPU
    feats = det.features_frames(tl.frames, tl.tile_yx)
    h_feats = feats.cpu().numpy()
    lx, ly, cnt = training.label_arrays(labels)
    targets = tr.ref_targets(lx, ly, cnt, tl.tile_yx).reshape(-1, 12, 12, 4)
    w0 = [np.asarray(weights[k], np.float32) for k in training.FC_KEYS]
    r_hist, _, _ = tr.e2e_reference(w0, h_feats, targets)
    y_hist, _, _ = tr.e2e_reference(w0, h_feats, targets, dtype=torch.float32)
    total = r_hist[tr.COMPONENTS.index('total_summed_loss')]
    print('reference total_summed_loss per epoch:', total, ' GPU:', hist.loc['total_summed_loss'].to_numpy())
    assert total[-1] < 0.5 * total[0]
    failures = []
    for i, name in enumerate(tr.COMPONENTS):
        try:
            tr.judge(hist.loc[name].to_numpy(), r_hist[i], y_hist[i], f'history {name}', log=print)
        except tr.TrainMismatch as e:
            failures.append(str(e))
    assert not failures, '\n'.join(failures)
    # the checkpoint is the returned dict, and a Detector built from it gives the trainer's own grids
    back = _load_state_dict(f'{tmp_path}/E{E["epochs"] - 1:04}.pth')
    assert all(np.array_equal(back[k].numpy(), np.asarray(sd[k])) for k in sd)
    det2 = axtrack_amd.Detector(back, max_batch=8, device=DEV)
    grids = det2.detect_frames(tl.frames, tl.tile_yx)
    own = training.HeadTrainer(sd, max_batch=8, device=DEV).forward(feats)
    assert (grids[:, 0] - own).abs().max().item() <= 1e-5
    assert (grids - det.detect_frames(tl.frames, tl.tile_yx)).abs().max().item() > 1e-2        # and they have moved
    tl.frame_sharded = True          # what Timelapse.sync_tile_occupancy() records in a run of several ranks
    with pytest.raises(NotImplementedError):
        axtrack_amd.fine_tune_head(tl, labels, det, E['parameters'], 1)

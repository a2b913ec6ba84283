"""The test-set loss of every epoch (fine_tune_head / fine_tune_detector(test_loss=True)): the trainers
export their weights into one evaluation detector on the device, which runs the test set.

The reference of every number is the epoch's CHECKPOINT, which goes through the host: Detector(checkpoint state dict) is
built by the host packers, runs its forward on the test frames, and HeadTrainer.loss is taken on the same batches. The
device export is byte-identical to the host packing (tests/test_repack_gpu.py) and every kernel is deterministic, so the
five components agree exactly: no tolerance.

The set: a 512 x 1024 timelapse (two tiles), 4 detection frames to train on and 3 to test on, a few labels each;
BATCH_SIZE=4, two epochs, a checkpoint after each. Depths 0, 1 and 8, the last with train-mode BatchNorm, whose moved
running statistics the evaluation has to see."""
import os

import numpy as np
import pytest
import torch

import axtrack_amd
from axtrack_amd import synth, training
from axtrack_amd.hotpath import S, Detector
from axtrack_amd.interface import _load_state_dict

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
EPOCHS, SEED = 2, 4
PARAMS = dict(BATCH_SIZE=4, LR=0.001, SHUFFLE=True, DROP_LAST=False, MODEL_CHECKPOINTS=[0, 1])
DEPTHS = [(0, False), (1, False), (8, True)]


def _labels(n, shift):
    return [([70 + 90 * i + 11 * t + shift for i in range(4 + t % 2)], [60 + 100 * i - 7 * t for i in range(4 + t % 2)])
            for t in range(n)]


@pytest.fixture(scope='module')
def data():
    train = axtrack_amd.Timelapse(synth.synth_frames(8, 512, 1024, seed=21), name='train', device=DEV, labels=_labels(4, 0))
    test = axtrack_amd.Timelapse(synth.synth_frames(7, 512, 1024, seed=22), name='test', device=DEV, labels=_labels(3, 500))
    assert len(train) == 4 and len(test) == 3
    assert len(np.reshape(train.tile_yx, (-1, 2))) == 2 and len(np.reshape(test.tile_yx, (-1, 2))) == 2
    return train, test


@pytest.fixture(scope='module')
def model(weights):
    return Detector(weights, max_batch=8, device=DEV)


@pytest.fixture(scope='module')
def judge(weights, data):
    """(state dict, DROP_LAST) -> the five components of that state dict on the test set, by the host route."""
    _, test = data
    head = training.HeadTrainer(weights, PARAMS, max_batch=4, device=DEV)       # for its loss only: it reads no weights
    targets = training.yolo_targets(test.labels, test.tile_yx, device=DEV).reshape(-1, S, S, 4)
    assert targets.shape[0] == 6

    def components(sd, drop_last):
        yolo = Detector(sd, max_batch=8, device=DEV).detect_frames(test.frames, test.tile_yx).reshape(-1, S, S, 3)
        batches = training.epoch_batches(6, 4, False, drop_last, None)
        assert [len(b) for b in batches] == ([4] if drop_last else [4, 2])
        rows = []
        for b in batches:
            comp, _ = head.loss(yolo[int(b[0]):int(b[-1]) + 1].contiguous(), targets, b)
            rows.append([comp[k] for k in training.COMPONENTS])
        return np.mean(np.array(rows, np.float64), axis=0)
    return components


def _run(data, model, depth, batch_stats, dest, test_loss, **params):
    train, test = data
    return axtrack_amd.fine_tune_detector(train, model=model, parameters=dict(PARAMS, **params), epochs=EPOCHS, dest_dir=dest,
                                          seed=SEED, train_conv_blocks=depth, bn_batch_stats=batch_stats,
                                          test_timelapse=test if test_loss else None, metrics_every=0, test_loss=test_loss)


def _same(a, b):
    return list(a) == list(b) and all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in a)


@pytest.mark.parametrize('depth,batch_stats', DEPTHS, ids=[f'depth{d}' for d, _ in DEPTHS])
def test_test_loss_is_the_checkpoints_loss_and_changes_nothing(depth, batch_stats, data, model, judge, weights, tmp_path):
    sd, hist = _run(data, model, depth, batch_stats, f'{tmp_path}/with', True)
    tl = hist.attrs['test_loss']
    assert list(tl.index) == list(training.COMPONENTS) == list(hist.index) and list(tl.columns) == [0, 1]
    assert 'metrics' not in hist.attrs
    per_epoch = []
    for epoch in range(EPOCHS):
        ck = {k: v.numpy() for k, v in _load_state_dict(f'{tmp_path}/with/E{epoch:04}.pth').items()}
        ref = judge(ck, False)
        got = tl[epoch].to_numpy()
        print(f'depth {depth} epoch {epoch}: test loss {got.tolist()} (checkpoint: {ref.tolist()})')
        assert got.tobytes() == ref.tobytes()
        assert np.isfinite(got).all() and got[3] > 0
        per_epoch.append(got)
    assert not np.array_equal(per_epoch[0], per_epoch[1])           # the second epoch's weights were exported, not the first's
    assert _same({k: np.asarray(v) for k, v in sd.items()},
                 {k: v.numpy() for k, v in _load_state_dict(f'{tmp_path}/with/E0001.pth').items()})
    if batch_stats:                                                 # the evaluation saw statistics that had moved
        k = 'ConvNet.ConvBlock_0.batchnorm.running_var'
        assert not np.array_equal(np.asarray(sd[k]), weights[k])
    # the same run without: history, state dict and checkpoints to the byte
    sd0, hist0 = _run(data, model, depth, batch_stats, f'{tmp_path}/without', False)
    assert 'test_loss' not in hist0.attrs
    assert hist0.to_numpy().tobytes() == hist.to_numpy().tobytes() and list(hist0.columns) == list(hist.columns)
    assert _same(sd0, sd)
    for epoch in range(EPOCHS):
        a, b = (f'{tmp_path}/{d}/E{epoch:04}.pth' for d in ('with', 'without'))
        assert _same({k: v.numpy() for k, v in _load_state_dict(a).items()}, {k: v.numpy() for k, v in _load_state_dict(b).items()})
        assert open(a, 'rb').read() == open(b, 'rb').read()
    assert model.state_dict_source is weights                       # the model passed in is not the one exported into


def test_drop_last_uses_one_test_batch(data, model, judge, tmp_path):
    sd, hist = _run(data, model, 0, False, str(tmp_path), True, DROP_LAST=True)
    tl = hist.attrs['test_loss']
    for epoch in range(EPOCHS):
        ck = {k: v.numpy() for k, v in _load_state_dict(f'{tmp_path}/E{epoch:04}.pth').items()}
        one, two = judge(ck, True), judge(ck, False)
        assert tl[epoch].to_numpy().tobytes() == one.tobytes() and not np.array_equal(one, two)


def test_metrics_use_the_evaluation_detector(data, model, tmp_path, monkeypatch):
    """With test_loss=True the every-n-th-epoch evaluation of the test set runs on the detector the trainers export into:
    the same table as the one from a detector built from the weights of that moment."""
    train, test = data
    kw = dict(model=model, parameters=PARAMS, epochs=1, seed=SEED, train_conv_blocks=1, test_timelapse=test, metrics_every=1)
    _, plain = axtrack_amd.fine_tune_detector(train, **kw)
    built = []
    create = Detector.__init__
    monkeypatch.setattr(Detector, '__init__', lambda self, *a, **k: (built.append(1), create(self, *a, **k))[1])
    _, with_loss = axtrack_amd.fine_tune_detector(train, test_loss=True, **kw)
    assert len(built) == 2                                          # the evaluation detector, and the train set's metrics
    m0, m1 = plain.attrs['metrics'], with_loss.attrs['metrics']
    assert list(m0.columns) == list(m1.columns) == [(0, 'train'), (0, 'test')]
    assert m0.to_numpy().tobytes() == m1.to_numpy().tobytes()
    assert list(with_loss.attrs['test_loss'].columns) == [0]


def test_test_loss_needs_a_labelled_test_timelapse(data, model):
    train, test = data
    with pytest.raises(ValueError, match='test_loss'):
        axtrack_amd.fine_tune_detector(train, model=model, parameters=PARAMS, test_loss=True)
    bare = axtrack_amd.Timelapse(test.frames, device=DEV)
    with pytest.raises(ValueError, match='test_loss'):
        axtrack_amd.fine_tune_detector(train, model=model, parameters=PARAMS, test_timelapse=bare, metrics_every=0, test_loss=True)
    with pytest.raises(ValueError, match='test_loss'):
        axtrack_amd.fine_tune_head(train, model=model, parameters=PARAMS, test_loss=True)
    with pytest.raises(ValueError, match='larger than the training batches'):
        axtrack_amd.fine_tune_detector(axtrack_amd.Timelapse(train.frames[:5], device=DEV, labels=train.labels[:1]), model=model,
                                       parameters=PARAMS, test_timelapse=test, metrics_every=0, test_loss=True)

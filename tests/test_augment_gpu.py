"""The augmentation warp on the GPU (csrc/augment.hip, axtrack_amd/augment.py) against tests/augment_reference.py, and
fine_tune_head's augmented epochs end to end. Translations and flips bit for bit; rotations bit for bit outside the band
of near-ties of the f64 map (augment_reference.judge_rotation), one of the candidate roundings inside it."""
import numpy as np
import pytest
import torch

import augment_reference as ar
import axtrack_amd
from axtrack_amd import _lib, augment, synth, training
from axtrack_amd.augment import Transform

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
TS = 512
# the kernel's frame chunk (kAugFrameChunk in csrc/augment.hip, axt_augment_frame_chunk): [7, 96, 160] is one frame more
FRAME_CHUNK = 6


@pytest.fixture(scope='module')
def stacks():
    """Per shape of augment_reference.SHAPES: frames with positive, negative and zero pixels (about a third each), every
    pixel its own value; in the large one a tile without a positive pixel in frame 0 and an empty partial tile in frame 2."""
    out = {}
    for shape in ar.SHAPES:
        rng = np.random.default_rng(shape[2])
        f = (rng.normal(0, 1, shape) * (rng.random(shape) < 0.66)).astype(np.float32)
        if shape[1] > TS:
            f[0, :TS, TS:2 * TS] = -np.abs(f[0, :TS, TS:2 * TS])
            f[2, TS:, 2 * TS:] = 0
        out[shape] = (f, torch.from_numpy(f).to(DEV))
    return out


def _occ_of(out):
    """u8 [T, tiles] from the warped frames themselves, with torch."""
    T, H, W = out.shape
    rows = []
    for y0 in range(0, H, TS):
        for x0 in range(0, W, TS):
            rows.append((out[:, y0:y0 + TS, x0:x0 + TS] > 0).flatten(1).any(1))
    return torch.stack(rows, 1).to(torch.uint8)


def _run(d_frames, tf):
    out, occ = augment.augment_frames(d_frames, tf, return_occupancy=True)
    assert occ.shape == (d_frames.shape[0], -(-d_frames.shape[1] // TS) * -(-d_frames.shape[2] // TS))
    assert torch.equal(occ, _occ_of(out)), f'occupancy, {tf}'
    plain = augment.augment_frames(d_frames, tf)
    assert torch.equal(plain, out)
    return out.cpu().numpy(), occ.cpu().numpy()


def test_the_frame_chunk_is_the_one_the_shapes_were_chosen_for():
    assert augment.frame_chunk() == FRAME_CHUNK and ar.SHAPES[1][0] == FRAME_CHUNK + 1


@pytest.mark.parametrize('shape', ar.SHAPES)
def test_translations_and_flips_bit_equal(stacks, shape):
    f, d = stacks[shape]
    T, H, W = shape
    got, occ = _run(d, Transform())
    assert got.tobytes() == f.tobytes()
    if H > TS:
        assert occ.tolist() == [[1, 0, 1, 1, 1, 1], [1] * 6, [1, 1, 1, 1, 1, 0]]
    cases = [Transform(dy=7), Transform(dy=-5), Transform(dx=9), Transform(dx=-13), Transform(dy=H // 2 + 1, dx=-(W // 2) - 2),
             Transform(flip_y=True), Transform(flip_x=True), Transform(flip_y=True, flip_x=True),
             Transform(dy=6, flip_y=True), Transform(dx=-7, flip_x=True), Transform(dy=-8, dx=10, flip_y=True, flip_x=True),
             Transform(dy=H - 1, dx=1 - W)]
    for tf in cases:
        got, _ = _run(d, tf)
        want = ar.warp(f, None, tf.flip_y, tf.flip_x, tf.dy, tf.dx)
        assert got.tobytes() == want.tobytes(), tf
        assert want.any()
    for tf in (Transform(dy=H), Transform(dy=-H), Transform(dy=H + 3, flip_x=True), Transform(dy=-2 ** 31), Transform(dy=2 ** 40),
               Transform(dx=W), Transform(dx=-W - 1000), Transform(dy=H, angle=11.0)):
        got, occ = _run(d, tf)
        assert not got.any() and not occ.any(), tf


@pytest.mark.parametrize('name', list(ar.ROTATIONS))
@pytest.mark.parametrize('shape', ar.SHAPES)
def test_rotations(stacks, shape, name):
    f, d = stacks[shape]
    angle, fy, fx, dy, dx = ar.ROTATIONS[name]
    got, _ = _run(d, Transform(dy=dy, dx=dx, flip_y=fy, flip_x=fx, angle=angle))
    ar.judge_rotation(got, f, angle, fy, fx, dy, dx, name=name)


def test_bad_input_is_an_error_code_not_a_launch(stacks):
    f, d = stacks[ar.SHAPES[1]]
    T, H, W = d.shape
    lib = _lib.load()
    out = torch.empty_like(d)
    st = torch.cuda.current_stream().cuda_stream

    def call(d_in, T_, d_out):
        return lib.axt_augment_frames(d_in, T_, H, W, 0, 0, 0, 0, 0, 1.0, 0.0, 0.0, 1.0, d_out, None, st)
    assert call(d.data_ptr(), T, d.data_ptr()) == -22                     # in place
    assert b'overlap' in lib.axt_last_error()
    assert call(d.data_ptr(), T - 1, d[1:].data_ptr()) == -22             # overlapping
    assert call(None, T, out.data_ptr()) == -22 and call(d.data_ptr(), T, None) == -22
    assert call(d.data_ptr(), 0, out.data_ptr()) == -22 and call(d.data_ptr(), -3, out.data_ptr()) == -22
    assert call(d.data_ptr(), T, out.data_ptr()) == 0
    with pytest.raises(_lib.AxtError, match='overlap'):
        augment.augment_frames(d, Transform(dy=1), out=d)
    with pytest.raises(ValueError):
        augment.augment_frames(d[:, :, ::2], Transform())
    with pytest.raises(ValueError):
        augment.augment_frames(d, Transform(), out=out[1:])


# ------------------------------------------------------------------------------------------------ end to end
E2E = dict(T_all=7, H=520, W=600, frames_seed=13, epochs=2, seed=9, parameters=dict(BATCH_SIZE=5, LR=0.0001, SHUFFLE=True,
                                                                                    DROP_LAST=False))
KEYS = ['vflip', 'hflip', 'rot', 'translateY', 'translateX']


def _labels():
    """Per detection frame 8 labels spread over the middle of the frame, each in a YOLO cell of its own."""
    return [([90 + 55 * i + 7 * t for i in range(8)], [120 + 37 * i - 5 * t for i in range(8)]) for t in range(E2E['T_all'] - 4)]


@pytest.fixture(scope='module')
def e2e(weights):
    frames = synth.synth_frames(E2E['T_all'], E2E['H'], E2E['W'], seed=E2E['frames_seed'])
    tl = axtrack_amd.Timelapse(frames, name='augment', device=DEV)
    det = axtrack_amd.Detector(weights, max_batch=8, device=DEV)
    return tl, det, _labels()


def _same(a, b):
    (sd_a, h_a), (sd_b, h_b) = a, b
    assert set(sd_a) == set(sd_b)
    for k in sd_a:
        assert np.asarray(sd_a[k]).tobytes() == np.asarray(sd_b[k]).tobytes(), k
    assert h_a.to_numpy().tobytes() == h_b.to_numpy().tobytes() and list(h_a.columns) == list(h_b.columns)


def _tune(e2e, **kw):
    tl, det, labels = e2e
    return axtrack_amd.fine_tune_head(tl, labels, det, E2E['parameters'], E2E['epochs'], seed=E2E['seed'], **kw)


def test_a_no_transforms_is_the_cached_path(e2e):
    plain = _tune(e2e)
    _same(plain, _tune(e2e, use_transforms=[]))
    _same(plain, _tune(e2e, use_transforms=None, transforms=None, min_pos_rate=0.65, max_redraws=50))
    assert 'transforms' not in plain[1].attrs


def test_b_explicit_transforms_equal_a_loop_of_the_public_pieces(e2e, weights):
    tl, det, labels = e2e
    H, W = E2E['H'], E2E['W']
    tfs = [Transform(dy=-9, dx=11, flip_y=True, flip_x=True, angle=11.0), dict(dx=-300)]
    sd, hist = _tune(e2e, transforms=tfs)
    assert hist.attrs['transforms'] == [tfs[0], Transform(dx=-300)]
    P = dict(training.TRAIN_DEFAULTS, **E2E['parameters'])
    trainer = training.HeadTrainer(weights, P, max_batch=P['BATCH_SIZE'], device=DEV)
    rng = np.random.default_rng(E2E['seed'])
    n_tiles, rows = [], []
    for epoch, tf in enumerate(tfs):
        warped, occ = augment.augment_frames(tl.frames, tf, return_occupancy=True)
        tiles = [divmod(int(i), tl.xtiles) for i in torch.nonzero(occ.amax(0)).flatten()]
        n_tiles.append(len(tiles))
        lab = augment.transform_labels(labels, tf, H, W)
        feats = det.features_frames(warped, tiles)
        tgt = training.yolo_targets(lab, tiles, device=DEV).reshape(-1, 12, 12, 4)
        lr = training.learning_rate(P['LR'], P['LR_DECAYRATE'], epoch)
        comps = []
        for batch in training.epoch_batches(feats.shape[0], P['BATCH_SIZE'], P['SHUFFLE'], P['DROP_LAST'], rng):
            y = trainer.forward(feats, batch)
            comp, dy = trainer.loss(y, tgt, batch)
            trainer.step(feats, batch, dy, lr=lr)
            comps.append([comp[k] for k in training.COMPONENTS])
        rows.append(np.mean(np.array(comps, np.float64), axis=0))
    assert n_tiles[0] > n_tiles[1] == 2                    # the second transform empties the right-hand tile column
    for k, w in zip(training.FC_KEYS, trainer.weights()):
        assert np.asarray(sd[k]).tobytes() == w.tobytes(), k
    assert hist.to_numpy().tobytes() == np.array(rows).T.tobytes()
    assert any(np.asarray(sd[k]).tobytes() != np.asarray(weights[k]).tobytes() for k in training.FC_KEYS)
    assert all(sd[k] is weights[k] for k in weights if k not in training.FC_KEYS)


def test_c_drawn_transforms_repeat_and_replay(e2e):
    one = _tune(e2e, use_transforms=KEYS)
    _same(one, _tune(e2e, use_transforms=KEYS))
    used = one[1].attrs['transforms']
    assert len(used) == E2E['epochs'] and all(isinstance(t, Transform) for t in used)
    assert any(not t.identity for t in used)
    _same(one, _tune(e2e, transforms=used))
    with pytest.raises(ValueError):
        _tune(e2e, transforms=used[:1])
    with pytest.raises(ValueError):
        _tune(e2e, use_transforms=['rotate'])


def test_d_an_unreachable_rate_raises_after_max_redraws(e2e):
    with pytest.raises(RuntimeError, match='3 redraws.*best'):
        _tune(e2e, use_transforms=KEYS, min_pos_rate=1e9, max_redraws=3)
    tl, det, labels = e2e
    tl.frame_sharded = True
    try:
        with pytest.raises(NotImplementedError):
            _tune(e2e, use_transforms=KEYS)
    finally:
        tl.frame_sharded = False

"""Labelled timelapses on the GPU: the per-frame statistics kernel and the frame-wise preprocessing kernel
(csrc/preproc.hip) against axt_preprocess_u16 -- which is not under test here -- and numpy; estimate_stnd_scaler against the
restated Timelapse._standardize (tests/scaler_reference.py); prepare_training_data, the labelled AxonDetections and
fine_tune_head's validation metrics end to end."""
import numpy as np
import pytest
import torch

import scaler_reference as sr
from axtrack_amd import hotpath as hp, params, timelapse as tlm

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
U = 2.0 ** -53


@pytest.fixture(scope='module')
def cases():
    """name -> (raw on the device, mask, offset, clip, log_correct, the frames axt_preprocess_u16 writes at scale 1 (host))."""
    out = {}
    for name in sr.SHAPES:
        raw, mask, kw = sr.raw_case(name)
        d_raw, m, off, lo = tlm._raw_on_device(raw, mask, kw['offset'], kw['clip'], DEV)
        ones = hp.preprocess_u16(d_raw, m, off, lo, kw['log_correct'], 1.0).cpu().numpy()
        out[name] = (d_raw, m, off, lo, kw['log_correct'], ones)
    return out


# ------------------------------------------------------------------------------------------------ statistics
@pytest.mark.parametrize('name', list(sr.SHAPES))
def test_stats_against_numpy(cases, name):
    d_raw, m, off, lo, logc, ones = cases[name]
    st = hp.preprocess_stats_u16(d_raw, m, off, lo, logc)
    again = hp.preprocess_stats_u16(d_raw, m, off, lo, logc)
    n, s, q, mx = sr.frame_parts(ones)
    print(name, 'n', st['n'], 'max', st['max'], 'rel sum', np.abs(st['sum'] - s) / np.maximum(s, 1e-300),
          'rel sumsq', np.abs(st['sumsq'] - q) / np.maximum(q, 1e-300))
    assert st.shape == (len(ones),)
    assert np.array_equal(st['n'], n)
    assert np.array_equal(st['max'], mx) and st['max'].dtype == np.float32
    # any two summation orders of N non-negative f64 terms (zeros add nothing) agree within 2 N 2^-53
    bound = 2 * np.maximum(n, 1) * U
    assert np.all(np.abs(st['sum'] - s) <= bound * s)
    assert np.all(np.abs(st['sumsq'] - q) <= bound * q)
    assert st.tobytes() == again.tobytes()                      # deterministic: identical bits
    if name == 'edge_frames':
        assert st['n'].tolist() == [1, 0, 15] and st['sum'][1] == 0 and st['sumsq'][1] == 0 and st['max'][1] == 0
        assert st['sum'][0] == float(ones[0, -1, -1]) and st['sumsq'][0] == float(ones[0, -1, -1]) ** 2


# ------------------------------------------------------------------------------------------------ frame-wise scales
@pytest.mark.parametrize('name', ['edge_frames', 'vector_masked', 'no_log'])
def test_framewise_is_bit_equal_to_frame_by_frame(cases, name):
    d_raw, m, off, lo, logc, _ = cases[name]
    T = d_raw.shape[0]
    scales = np.array([0.5, 0.0152, 3.0, 1.0, 0.015176106, 7.25e-3][:T], np.float32)
    got = hp.preprocess_u16_framewise(d_raw, scales, m, off, lo, logc)
    for t in range(T):
        alone = hp.preprocess_u16(d_raw[t:t + 1], m, off, lo, logc, float(scales[t]))
        assert torch.equal(got[t:t + 1], alone), f'{name}: frame {t}'
    assert torch.isfinite(got).all()
    for bad in (0.0, -1.0, np.inf, np.nan):
        s = scales.copy()
        s[-1] = bad
        with pytest.raises(ValueError, match=rf'\[{T - 1}\]'):
            hp.preprocess_u16_framewise(d_raw, s, m, off, lo, logc)
    with pytest.raises(ValueError, match='scales'):
        hp.preprocess_u16_framewise(d_raw, scales[:-1], m, off, lo, logc)


# ------------------------------------------------------------------------------------------------ estimate_stnd_scaler
@pytest.mark.parametrize('mode', ['zscore', '0to1'])
@pytest.mark.parametrize('framewise', [False, True])
def test_estimate_stnd_scaler_end_to_end(cases, mode, framewise):
    raw, mask, kw = sr.raw_case('vector_masked')
    ones = cases['vector_masked'][5]
    scaler, per_frame = tlm.estimate_stnd_scaler(raw, mask, standardize=mode, framewise=framewise, device=DEV, **kw)
    r_scaler, r_scales, per = sr.ref_standardize(ones, mode, framewise)
    assert list(per_frame.columns) == ['n', 'mean', 'std', 'max'] and len(per_frame) == len(raw)
    assert np.all(per['kappa'] < 10)
    N = per['n']
    std_rtol, mean_rtol = 4 * N * U * per['kappa'], 2 * N * U
    print(mode, framewise, scaler, r_scaler, 'std rel', np.abs(per_frame['std'] - per['std']) / per['std'], 'allowed', std_rtol)
    assert np.array_equal(per_frame['n'], N) and np.array_equal(per_frame['max'], per['max'])
    assert np.all(np.abs(per_frame['std'] - per['std']) <= std_rtol * per['std'])
    assert np.all(np.abs(per_frame['mean'] - per['mean']) <= mean_rtol * per['mean'])
    assert scaler[0] == mode
    if framewise:
        assert scaler[1] is None and r_scaler[1] is None
        scales = tlm.frame_scales(scaler, per_frame)
        assert np.all(np.abs(scales - r_scales) <= (std_rtol if mode == 'zscore' else 0) * r_scales)
        frames = tlm.preprocess(raw, mask, scale=scales, device=DEV, **kw).cpu().numpy()
        assert np.array_equal(frames, ones / scales.astype(np.float32)[:, None, None])      # an f32 division by the f32 scale
    elif mode == 'zscore':
        assert abs(scaler[1][0] - r_scaler[1][0]) <= std_rtol.max() * r_scaler[1][0]
        assert abs(scaler[1][1] - r_scaler[1][1]) <= mean_rtol.max() * r_scaler[1][1]
    else:
        assert scaler[1] == r_scaler[1]


def test_estimate_refuses_what_would_put_nan_into_a_frame(cases):
    raw, _, kw = sr.raw_case('edge_frames')
    top = float(cases['edge_frames'][5].max())
    with pytest.raises(ValueError, match=r'frames \[1\]'):
        tlm.estimate_stnd_scaler(raw, device=DEV, **kw)
    with pytest.raises(ValueError, match=r'frames \[1\]'):
        tlm.estimate_stnd_scaler(raw, standardize='0to1', framewise=True, device=DEV, **kw)
    with pytest.raises(ValueError, match=r'frames \[0, 1, 2\]'):                    # one value / equal values: std 0
        tlm.estimate_stnd_scaler(raw[[0, 2, 2]], framewise=True, device=DEV, **kw)
    scaler, per_frame = tlm.estimate_stnd_scaler(raw, standardize='0to1', device=DEV, **kw)
    assert scaler == ('0to1', (top, 0.0)) and per_frame['n'].tolist() == [1, 0, 15]
    # a mask per frame zeroes the raw counts, as preprocess does it
    m3 = np.ones(raw.shape, bool)
    m3[2, :2] = False
    _, per_frame = tlm.estimate_stnd_scaler(raw, m3, standardize='0to1', device=DEV, **kw)
    assert per_frame['n'].tolist() == [1, 0, 9]


# ------------------------------------------------------------------------------------------------ dataset and training
def _parameters(files, pad):
    P = params.load_parameters()
    P.update(TIMELAPSE_FILE=files[0], LABELS_FILE=files[1], MASK_FILE=None, TRAIN_TIMEPOINTS=sr.DATASET['train'],
             TEST_TIMEPOINTS=sr.DATASET['test'], OFFSET=121, CLIP_LOWERLIM=55 / 2 ** 16, PAD=pad, LOG_CORRECT=True,
             STANDARDIZE=('zscore', None), STANDARDIZE_FRAMEWISE=False, CACHE=None, DEVICE=DEV, BATCH_SIZE=8)
    return P


@pytest.fixture(scope='module')
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp('labelled')
    raw = sr.dataset_raw()
    x, y = sr.dataset_label_table(raw)
    np.save(d / 'timelapse.npy', raw)
    sr.write_labels_csv(str(d / 'axon_anchor_labels.csv'), [f'Axon_{i:03}' for i in range(10, 18)], x, y)
    return str(d / 'timelapse.npy'), str(d / 'axon_anchor_labels.csv'), raw


@pytest.fixture(scope='module')
def dataset(files):
    import axtrack_amd
    P = _parameters(files, [0, 0, 0, 0])
    train, test = axtrack_amd.prepare_training_data(P)
    return P, train, test


@pytest.mark.parametrize('pad', [[0, 0, 0, 0], [0, 300, 0, 300]])
def test_prepare_training_data(files, dataset, pad, tmp_path):
    import pickle
    import axtrack_amd
    raw = files[2]
    if any(pad):
        P = _parameters(files, pad)
        train, test = axtrack_amd.prepare_training_data(P, CACHE=str(tmp_path))
        with open(tmp_path / 'train_stnd_scaler.pkl', 'rb') as f:
            assert pickle.load(f) == train.stnd_scaler
    else:
        P, train, test = dataset
    kw = dict(offset=P['OFFSET'], clip=P['CLIP_LOWERLIM'], log_correct=True, device=DEV)
    scaler, _ = tlm.estimate_stnd_scaler(raw, **kw)
    assert train.stnd_scaler == scaler and test.stnd_scaler == train.stnd_scaler and scaler[0] == 'zscore'
    H, W = 512 + pad[0] + pad[2], 512 + pad[1] + pad[3]
    assert (len(train), len(test)) == (6, 2) and tuple(train.frames.shape) == (10, H, W) and tuple(test.frames.shape) == (6, H, W)
    want = tlm.preprocess(raw, scale=scaler[1][0], pad=pad, **kw)
    assert torch.equal(train.frames, want[0:10]) and torch.equal(test.frames, want[6:12])
    labels = sr.ref_labels(files[1], pad, (H, W))
    for ds, tps in ((train, sr.DATASET['train']), (test, sr.DATASET['test'])):
        assert ds.labelled and len(ds.labels) == len(tps)
        for got, t in zip(ds.labels, tps):
            assert got[0].tolist() == labels[t][0].tolist() and got[1].tolist() == labels[t][1].tolist()
            assert got[2].tolist() == (labels[t][2] + 10).tolist()                   # Axon_010 .. Axon_017
    assert len(train.labels[0][0]) == (7 if any(pad) else 6)                         # the label right of the unpadded frame
    if any(pad):
        assert train.mask2d is not None and train.mask2d[:, 300:812].all() and not train.mask2d[:, :300].any()


def test_labelled_detections_and_fp_fn(dataset, weights):
    import axtrack_amd
    P, train, _ = dataset
    det = axtrack_amd.Detector(weights, max_batch=8, device=DEV)
    ad = axtrack_amd.AxonDetections(det, train, P, None)
    assert ad.labelled
    ad.detect_dataset()
    cm = ad.detection_confusion()
    assert cm.shape == (6, 3, 13)
    for t in range(len(ad)):
        prc, rcl, f1 = ad.get_detection_metrics('all', t)
        assert all(0 <= v <= 1 for v in (prc, rcl, f1))
        assert np.array_equal(ad.compute_TP_FP_FN('all', t), cm[t])
        truth = ad.get_frame_dets('groundtruth', t)
        assert truth.anchor_x.tolist() == train.labels[t][0].tolist() and truth.anchor_y.tolist() == train.labels[t][1].tolist()
        assert list(truth.index) == [f'Axon_{i:0>3}' for i in train.labels[t][2]]
        fp_mask, fn_mask = ad.compute_TP_FP_FN('confident', t, return_FP_FN_mask=True)
        fp, fn = ad.get_frame_dets('FP_FN', t)
        assert fp.equals(ad.get_frame_dets('confident', t)[fp_mask]) and fn.equals(truth[fn_mask])
        print(t, 'confident', len(fp_mask), 'FP', len(fp), 'labels', len(truth), 'FN', len(fn))
    # a subset of frames takes the labels of those frames
    sub = axtrack_amd.AxonDetections(det, train, P, None, timepoint_subset=[4, 1])
    assert sub.get_frame_dets('groundtruth', 0).anchor_x.tolist() == train.labels[4][0].tolist()
    with pytest.raises(ValueError, match='which_dets'):
        ad.render_frames('FP_FN')
    plain = axtrack_amd.AxonDetections(det, axtrack_amd.Timelapse(train.frames, device=DEV), P, None)
    assert not plain.labelled
    with pytest.raises(ValueError, match='no labels'):
        plain.get_frame_dets('FP_FN', 0)


def test_fine_tune_head_with_validation(dataset, weights):
    import pandas as pd
    import axtrack_amd
    P, train, test = dataset
    sd0, hist0 = axtrack_amd.fine_tune_head(train, model=weights, parameters=P, epochs=11, seed=3)
    sd1, hist1 = axtrack_amd.fine_tune_head(train, model=weights, parameters=P, epochs=11, seed=3, test_timelapse=test)
    assert 'metrics' not in hist0.attrs
    assert hist1.equals(hist0) and list(hist1.columns) == list(range(11))
    assert set(sd0) == set(sd1) and all(np.array_equal(np.asarray(sd0[k]), np.asarray(sd1[k])) for k in sd0)
    # the explicit labels give the same run
    sd2, hist2 = axtrack_amd.fine_tune_head(train, train.labels, weights, P, 2, seed=3)
    assert hist2.equals(hist0[[0, 1]])
    metrics = hist1.attrs['metrics']
    assert list(metrics.columns) == [(0, 'train'), (0, 'test'), (10, 'train'), (10, 'test')]
    det = axtrack_amd.Detector(sd1, max_batch=8, device=DEV)
    ad = axtrack_amd.AxonDetections(det, test, P, None)
    ad.detect_dataset()
    want = ad.compute_prc_rcl_F1(ad.detection_confusion().sum(axis=0), return_dataframe=True)
    assert metrics.index.equals(want.index) and len(want) == 3 * 13
    assert np.array_equal(metrics[(10, 'test')].to_numpy(), want.to_numpy())        # epoch 10 is the last: the returned weights
    assert ((metrics.to_numpy() >= 0) & (metrics.to_numpy() <= 1)).all()
    print(metrics.loc['F1'])
    with pytest.raises(ValueError, match='no labels'):
        axtrack_amd.fine_tune_head(axtrack_amd.Timelapse(train.frames, device=DEV), model=weights)
    with pytest.raises(ValueError, match='carries no labels'):
        axtrack_amd.fine_tune_head(train, model=weights, test_timelapse=axtrack_amd.Timelapse(test.frames, device=DEV))

"""Labelled timelapses, host side: the scaler from per-frame statistics, the labels reader, the time-point
arithmetic of prepare_training_data, the dataset cache, the library's exports. No GPU."""
import ctypes
import os
import pickle

import numpy as np
import pytest
import torch

import scaler_reference as sr
from axtrack_amd import _lib, interface, timelapse as tlm


# ------------------------------------------------------------------------------------------------ scaler from statistics
def _parts():
    """Four frames of known non-zero values, as (n, sum, sumsq, max) and as the values themselves."""
    vals = [np.array([0.5, 1.5, 1.0]), np.array([2.0, 4.0]), np.array([0.25, 0.25, 0.75, 1.75]), np.array([3.0, 1.0])]
    n = np.array([len(v) for v in vals])
    return vals, n, np.array([v.sum() for v in vals]), np.array([(v * v).sum() for v in vals]), np.array([v.max() for v in vals])


@pytest.mark.parametrize('mode', ['zscore', '0to1'])
@pytest.mark.parametrize('framewise', [False, True])
def test_scaler_from_stats(mode, framewise):
    vals, n, s, q, mx = _parts()
    scaler, per_frame, scales = tlm.scaler_from_stats(n, s, q, mx, mode, framewise)
    assert list(per_frame.columns) == ['n', 'mean', 'std', 'max'] and len(per_frame) == 4
    np.testing.assert_array_equal(per_frame['n'], n)
    np.testing.assert_allclose(per_frame['mean'], [v.mean() for v in vals], rtol=1e-15)
    np.testing.assert_allclose(per_frame['std'], [v.std() for v in vals], rtol=1e-14)
    np.testing.assert_array_equal(per_frame['max'], mx)
    # the same through the restated _standardize on dense frames that hold those values
    frames = np.zeros((4, 2, 4), np.float32)
    for t, v in enumerate(vals):
        frames[t].reshape(-1)[:len(v)] = v
    r_scaler, r_scales, _ = sr.ref_standardize(frames, mode, framewise)
    assert scaler[0] == r_scaler[0] == mode
    if framewise:
        assert scaler[1] is None and r_scaler[1] is None
        np.testing.assert_allclose(scales, r_scales, rtol=1e-14)
        np.testing.assert_allclose(tlm.frame_scales(scaler, per_frame), r_scales, rtol=1e-14)
    else:
        assert scales is None and isinstance(scaler[1][0], float)
        np.testing.assert_allclose(scaler[1], r_scaler[1], rtol=1e-14)
        assert tlm.frame_scales(scaler, per_frame) == scaler[1][0]
        if mode == '0to1':
            assert scaler[1] == (4.0, 0.0)


def test_scaler_error_cases():
    vals, n, s, q, mx = _parts()
    n0, s0, q0, mx0 = n.copy(), s.copy(), q.copy(), mx.copy()
    n0[[1, 3]], s0[[1, 3]], q0[[1, 3]], mx0[[1, 3]] = 0, 0, 0, 0               # frames without a non-zero pixel
    for framewise in (False, True):
        with pytest.raises(ValueError, match=r'\[1, 3\]'):
            tlm.scaler_from_stats(n0, s0, q0, mx0, 'zscore', framewise)
    with pytest.raises(ValueError, match=r'\[1, 3\]'):
        tlm.scaler_from_stats(n0, s0, q0, mx0, '0to1', True)
    scaler, per_frame, _ = tlm.scaler_from_stats(n0, s0, q0, mx0, '0to1', False)   # the other frames carry the maximum
    assert scaler == ('0to1', (1.75, 0.0)) and np.isnan(per_frame['mean'][1])
    with pytest.raises(ValueError, match='scale of the timelapse'):
        tlm.scaler_from_stats(n0 * 0, s0 * 0, q0 * 0, mx0 * 0, '0to1', False)
    # a frame of one value (or of equal values) has std 0: no frame-wise zscore scale
    with pytest.raises(ValueError, match=r'\[2\]'):
        tlm.scaler_from_stats([3, 2, 2], [3.0, 3.0, 1.0], [5.0, 5.0, 0.5], [2.0, 2.0, 0.5], 'zscore', True)
    # equal values that are no power of two: sumsq / n - mean^2 is summation noise, not a scale
    v = np.full(1000, np.float32(0.1), np.float64)
    with pytest.raises(ValueError, match=r'\[1\]'):
        tlm.scaler_from_stats([3, 1000], [3.0, np.sum(v[::-1])], [5.0, np.sum(v * v)], [2.0, v[0]], 'zscore', True)
    with pytest.raises(ValueError, match='standardize must be'):
        tlm.scaler_from_stats(n, s, q, mx, 'minmax', False)
    with pytest.raises(ValueError, match='standardize must be'):
        tlm.estimate_stnd_scaler(np.zeros((1, 2, 2), np.uint16), standardize=None)


# ------------------------------------------------------------------------------------------------ the reference's own run
@pytest.mark.parametrize('mode', ['zscore', '0to1'])
@pytest.mark.parametrize('framewise', [False, True])
def test_scaler_agrees_with_reference_golden(golden, mode, framewise):
    """The f64 scaler against Timelapse._standardize's own f32 result (scaler_parts.npz). The reference sums in f32: its mean
    and std carry the pairwise-summation error (ceil(log2 N) + 2) * 2^-24 * kappa, kappa = (sumsq / n) / var for the std
    and 1 for the mean of positive values; the bound is computed from the fixture."""
    g = golden('scaler_parts')
    frames = g['frames']
    assert frames.shape == (7, 64, 96) and frames.dtype == np.float32
    n, s, q, mx = sr.frame_parts(frames)
    dens = n / frames[0].size
    assert dens[3] > 0.5 and np.all(np.delete(dens, 3) < 0.08)                     # one frame much denser
    scaler, per_frame, scales = tlm.scaler_from_stats(n, s, q, mx, mode, framewise)
    _, _, per = sr.ref_standardize(frames, mode, framewise)
    std_bound = sr.f32_sum_bound(n, per['kappa'])
    mean_bound = sr.f32_sum_bound(n)
    key = f'{mode}_{"framewise" if framewise else "global"}'
    ref_frames = g[f'{key}_frames']
    if not framewise:
        ref_var, ref_mean = g[f'{key}_scaler']
        if mode == 'zscore':
            assert abs(scaler[1][0] - ref_var) <= std_bound.max() * ref_var, (scaler, ref_var, std_bound)
            assert abs(scaler[1][1] - ref_mean) <= mean_bound.max() * ref_mean
        else:
            assert scaler[1] == (float(ref_var), 0.0) and ref_mean == 0          # a maximum is exact
        # the reference divides f32 frames by its f32 scalar
        assert np.array_equal(frames / np.float32(ref_var), ref_frames)
        ours = frames / np.float32(scaler[1][0])
        tol = (std_bound.max() if mode == 'zscore' else 0.0) + 2.0 ** -23
        assert np.all(np.abs(ours - ref_frames) <= tol * np.abs(ref_frames))
    else:
        assert scaler[1] is None and np.all(np.isnan(g[f'{key}_scaler']))
        for t in range(len(frames)):
            # the reference's scale of frame t, recovered from its largest value: max / max' (to f32 rounding)
            nz = frames[t] != 0
            ref_scale = np.median(frames[t][nz].astype(np.float64) / ref_frames[t][nz].astype(np.float64))
            tol = (std_bound[t] if mode == 'zscore' else 0.0) + 2.0 ** -22
            assert abs(scales[t] - ref_scale) <= tol * ref_scale, (t, scales[t], ref_scale, tol)
            ours = frames[t] / np.float32(scales[t])
            assert np.all(np.abs(ours - ref_frames[t]) <= (tol + 2.0 ** -23) * np.abs(ref_frames[t]))
            assert np.array_equal(ours == 0, ref_frames[t] == 0)


# ------------------------------------------------------------------------------------------------ labels
NAN = np.nan


def test_load_labels_csv_values(tmp_path):
    """NaN entries, truncation toward zero, the pad shift, labels outside the frame, an unsorted index."""
    fname = str(tmp_path / 'labels.csv')
    names = ['Axon_003', 'Axon_000', 'Axon_012']
    x = np.array([[10.9, NAN, 99.99], [NAN, 5.2, 100.0], [0.4, 64.0, -0.5], [3.0, -1.0, 50.0]])
    y = np.array([[20.1, NAN, 0.0], [NAN, 59.9, 7.0], [60.0, 7.5, 3.0], [NAN, 4.0, -2.5]])
    sr.write_labels_csv(fname, names, x, y, index=[2, 0, 3, 1])              # rows out of order: frame 0 is the second row
    got = tlm.load_labels_csv(fname, shape=(60, 100))
    want = [([5], [59], [0]),                      # frame 0: Axon_012 at x = 100 is right of a 100-column frame
            ([], [], []),                          # frame 1: Axon_003 lacks y, Axon_000 at x = -1, Axon_012's y -2.5 -> -2
            ([10, 99], [20, 0], [3, 12]),          # frame 2: Axon_000 absent; 10.9 -> 10, 99.99 -> 99
            ([64, 0], [7, 3], [0, 12])]            # frame 3: y = 60 is below a 60-row frame; (-0.5, 3.0) -> (0, 3)
    assert len(got) == 4
    for t, (g, w) in enumerate(zip(got, want)):
        assert all(a.dtype == np.int64 for a in g)
        assert [a.tolist() for a in g] == [list(v) for v in w], f'frame {t}: {g}'
    # and the restated _load_bboxes + construct_tiles agree (their ids are column positions)
    pos = {3: 0, 0: 1, 12: 2}
    for g, r in zip(got, sr.ref_labels(fname, None, (60, 100))):
        assert g[0].tolist() == r[0].tolist() and g[1].tolist() == r[1].tolist() and [pos[i] for i in g[2]] == r[2].tolist()
    # without a shape only what is left of / above the frame goes
    assert [a.tolist() for a in tlm.load_labels_csv(fname)[0]] == [[5, 100], [59, 7], [0, 12]]
    # pad = (top, right, bottom, left): +7 on y, +30 on x, and the frame grows
    padded = tlm.load_labels_csv(fname, pad=[7, 11, 0, 30], shape=(67, 141))
    assert [a.tolist() for a in padded[0]] == [[35, 130], [66, 14], [0, 12]]
    assert [a.tolist() for a in padded[1]] == [[29, 80], [11, 4], [0, 12]]          # x = -1 + 30, y = -2.5 + 7 -> 4
    assert [a.tolist() for a in padded[2]] == [[40, 129], [27, 7], [3, 12]]
    for g, r in zip(padded, sr.ref_labels(fname, [7, 11, 0, 30], (67, 141))):
        assert g[0].tolist() == r[0].tolist() and g[1].tolist() == r[1].tolist()


def test_load_labels_csv_ids(tmp_path):
    x, y = np.array([[1.0, 2.0, 3.0]]), np.array([[4.0, 5.0, 6.0]])
    cases = {('Axon_007', 'Axon_002', 'ax11'): [7, 2, 11],                  # every name ends in a number, all distinct
             ('Axon_007', 'growthcone', 'Axon_001'): [0, 1, 2],              # a name without a number: column positions
             ('a_1', 'b_1', 'c_2'): [0, 1, 2]}                               # numbers that collide: column positions
    for names, ids in cases.items():
        fname = str(tmp_path / f'{"-".join(names)}.csv')
        sr.write_labels_csv(fname, names, x, y)
        (gx, gy, gid), = tlm.load_labels_csv(fname)
        assert gx.tolist() == [1, 2, 3] and gy.tolist() == [4, 5, 6] and gid.tolist() == ids


# ------------------------------------------------------------------------------------------------ prepare_training_data
@pytest.fixture
def stubbed(monkeypatch, tmp_path):
    """prepare_training_data with the two GPU calls replaced: `preprocess` returns frames that hold their own input frame
    number, `estimate_stnd_scaler` a fixed answer; both record their arguments."""
    import pandas as pd
    calls = []
    T, H, W = 14, 6, 8
    raw = (np.arange(T, dtype=np.uint16)[:, None, None] + np.zeros((1, H, W), np.uint16))

    def preprocess(imseq, mask=None, offset=121, clip=55, log_correct=True, scale=1.0, device='cpu', pad=None):
        calls.append(('preprocess', np.asarray(imseq)[:, 0, 0].tolist(), np.copy(scale), pad))
        out = torch.from_numpy(np.asarray(imseq).astype(np.float32))
        if pad is not None and any(pad):
            out = torch.nn.functional.pad(out, (pad[3], pad[1], pad[0], pad[2]))
        return out

    def estimate(imseq, mask=None, offset=None, clip=None, log_correct=True, standardize='zscore', framewise=False,
                 device='cpu'):
        calls.append(('estimate', len(imseq), standardize, framewise))
        per = pd.DataFrame({'n': np.ones(T, np.int64), 'mean': np.ones(T), 'std': 1.0 + np.arange(T), 'max': 100.0 + np.arange(T)})
        return ((standardize, None) if framewise else (standardize, (0.25, 0.125))), per

    monkeypatch.setattr(interface, 'preprocess', preprocess)
    monkeypatch.setattr(interface, 'estimate_stnd_scaler', estimate)
    labels = str(tmp_path / 'labels.csv')
    x = np.arange(T, dtype=np.float64)[:, None] % W + np.zeros((1, 2))
    sr.write_labels_csv(labels, ['Axon_000', 'Axon_001'], x, x * 0 + 1)
    P = dict(TIMELAPSE_FILE=raw, LABELS_FILE=labels, MASK_FILE=None, TRAIN_TIMEPOINTS=[3, 4, 5, 6], TEST_TIMEPOINTS=[9, 10],
             OFFSET=None, CLIP_LOWERLIM=None, PAD=[0, 0, 0, 0], LOG_CORRECT=True, STANDARDIZE=('zscore', None),
             STANDARDIZE_FRAMEWISE=False, TEMPORAL_CONTEXT=2, TILESIZE=512, CACHE=None, DEVICE='cpu')
    return P, calls


def test_prepare_training_data_timepoints(stubbed, tmp_path):
    P, calls = stubbed
    train, test = interface.prepare_training_data(P, CACHE=str(tmp_path / 'cache'))
    assert calls[0] == ('estimate', 14, 'zscore', False)                          # all frames of the file take part
    assert calls[1][1] == list(range(1, 9)) and calls[1][2] == 0.25               # [min - 2, max + 2]
    assert calls[2][1] == list(range(7, 13)) and calls[2][2] == 0.25
    assert (train.name, len(train), test.name, len(test)) == ('train', 4, 'test', 2)
    assert train.labelled and test.labelled and train.stnd_scaler == ('zscore', (0.25, 0.125))
    assert test.stnd_scaler == train.stnd_scaler
    assert [l[0].tolist() for l in train.labels] == [[t % 8] * 2 for t in (3, 4, 5, 6)]
    assert [l[0].tolist() for l in test.labels] == [[1, 1], [2, 2]]
    with open(tmp_path / 'cache' / 'train_stnd_scaler.pkl', 'rb') as f:
        assert pickle.load(f) == train.stnd_scaler
    # a passed scaler is used as it is, nothing is estimated; skip_test
    del calls[:]
    train, test = interface.prepare_training_data(P, skip_test=True, STANDARDIZE=('zscore', (0.5, 0.1)), TRAIN_TIMEPOINTS=[11, 10])
    assert test is None and [c[0] for c in calls] == ['preprocess'] and calls[0][1] == list(range(8, 14)) and calls[0][2] == 0.5
    assert train.stnd_scaler == ('zscore', (0.5, 0.1))
    # frame-wise: (name, None), every set takes its own frames' scales; the pad reaches preprocess and the labels
    del calls[:]
    train, test = interface.prepare_training_data(P, STANDARDIZE=('0to1', None), STANDARDIZE_FRAMEWISE=True, PAD=[1, 2, 3, 4])
    assert calls[0] == ('estimate', 14, '0to1', True)
    assert calls[1][2].tolist() == [101.0 + k for k in range(8)] and calls[2][2].tolist() == [107.0 + k for k in range(6)]
    assert train.stnd_scaler == ('0to1', None) and test.stnd_scaler == ('0to1', None)
    assert (train.sizey, train.sizex) == (6 + 4, 8 + 6) and calls[1][3] == [1, 2, 3, 4]
    assert train.labels[0][0].tolist() == [3 + 4, 3 + 4] and train.labels[0][1].tolist() == [2, 2]
    assert train.mask2d is not None and train.mask2d.sum() == 6 * 8 and train.mask2d[1:7, 4:12].all()


def test_prepare_training_data_refusals(stubbed):
    P, _ = stubbed
    with pytest.raises(ValueError, match=r"TRAIN_TIMEPOINTS has gaps.*'3\.\.4', '7\.\.8'"):
        interface.prepare_training_data(P, TRAIN_TIMEPOINTS=[3, 4, 7, 8])
    with pytest.raises(ValueError, match=r"TEST_TIMEPOINTS has gaps.*'5\.\.5', '9\.\.10'"):
        interface.prepare_training_data(P, TEST_TIMEPOINTS=[9, 10, 5])
    with pytest.raises(ValueError, match='need the input frames'):
        interface.prepare_training_data(P, TRAIN_TIMEPOINTS=[1, 2])
    with pytest.raises(ValueError, match='need the input frames'):
        interface.prepare_training_data(P, TEST_TIMEPOINTS=[12])
    with pytest.raises(ValueError, match='STANDARDIZE_FRAMEWISE'):
        interface.prepare_training_data(P, STANDARDIZE=('zscore', (0.5, 0.1)), STANDARDIZE_FRAMEWISE=True)
    with pytest.raises(ValueError, match='empty'):
        interface.prepare_training_data(P, TRAIN_TIMEPOINTS=[])


# ------------------------------------------------------------------------------------------------ cache, exports
def test_cache_round_trip_with_and_without_labels(tmp_path):
    from axtrack_amd import Timelapse
    frames = np.random.default_rng(0).random((7, 4, 6)).astype(np.float32)
    labels = [(np.array([1, 2]), np.array([3, 0]), np.array([7, 9])), (np.array([], int), np.array([], int), np.array([], int)),
              (np.array([5]), np.array([2]), np.array([7]))]
    tl = Timelapse(frames, name='train', device='cpu', labels=labels, stnd_scaler=('zscore', (0.02, 0.01)))
    assert tl.labelled and len(tl) == 3
    tl.to_cache(str(tmp_path))
    back = Timelapse.from_cache(str(tmp_path), 'train', device='cpu')
    assert back.labelled and back.stnd_scaler == ('zscore', (0.02, 0.01)) and torch.equal(back.frames, tl.frames)
    assert all(np.array_equal(a, b) for l, m in zip(back.labels, labels) for a, b in zip(l, m))
    # an unlabelled one, and a cache file written before the two keys existed
    plain = Timelapse(frames, name='plain', device='cpu')
    assert not plain.labelled and plain.labels is None and plain.stnd_scaler is None
    plain.to_cache(str(tmp_path))
    fname = tmp_path / 'plain_dataset_cached.pkl'
    with open(fname, 'rb') as f:
        d = pickle.load(f)
    assert d['labels'] is None and d['stnd_scaler'] is None
    del d['labels'], d['stnd_scaler']
    with open(fname, 'wb') as f:
        pickle.dump(d, f)
    old = Timelapse.from_cache(str(tmp_path), 'plain', device='cpu')
    assert not old.labelled and old.stnd_scaler is None and torch.equal(old.frames, plain.frames)
    with pytest.raises(ValueError, match='label frames'):
        Timelapse(frames, device='cpu', labels=labels[:2])


def test_library_exports_and_scratch_query():
    lib = _lib.load()
    assert lib.axt_abi_version() == 1
    assert hasattr(lib, 'axt_preprocess_stats_u16') and hasattr(lib, 'axt_preprocess_u16_framewise')
    # the size query touches no device: partials of 32 bytes, frames x blocks per frame, under the cap of 2048 blocks
    need = ctypes.c_size_t(0)
    for (T, H, W), blocks in {(1, 3, 5): 1, (3, 5, 3): 3, (6, 520, 1032): 6 * 263, (5, 1024, 1024): 5 * 409,
                              (4, 37, 41): 4, (3000, 64, 64): 3000}.items():
        assert lib.axt_preprocess_stats_u16(None, None, T, H, W, 0, 0, 1, None, None, ctypes.byref(need), None) == 0
        assert need.value == 32 * blocks, (T, H, W, need.value)
    assert lib.axt_preprocess_stats_u16(None, None, 0, 4, 4, 0, 0, 1, None, None, ctypes.byref(need), None) < 0
    assert lib.axt_preprocess_stats_u16(None, None, 1, 4, 4, 0, 0, 1, None, None, None, None) < 0
    for bad in [(None, 1, 1, 2, 2, 1), (1, None, 1, 2, 2, 1), (1, 1, None, 2, 2, 1), (1, 1, 1, 0, 2, 2), (1, 1, 1, 2, 0, 2),
                (1, 1, 1, 2, 2, 0)]:
        raw, scale, out, T, H, W = bad
        assert lib.axt_preprocess_u16_framewise(raw, None, T, H, W, 0, 0, 1, scale, out, None) == -22     # AXT_EINVAL, before any launch


def test_gpu_inputs_have_the_properties_the_gpu_tests_rest_on():
    """Chosen on the CPU: every route the cases claim, and kappa < 10 for the end-to-end comparison."""
    raw, mask, kw = sr.raw_case('vector_masked')
    assert raw[0].size % 8 == 0 and raw[0].size // 8 > 256 and mask is not None and kw['offset'] and kw['clip']
    _, _, per = sr.ref_standardize(sr.host_preprocess(raw, mask, **kw), 'zscore', True)
    assert np.all(per['kappa'] < 10) and np.all(per['n'] > 1000)
    raw, _, _ = sr.raw_case('grid_bound')
    assert raw.size > 2048 * 256 * 8 and raw[0].size % 8 == 0
    raw, _, _ = sr.raw_case('edge_frames')
    assert (raw[0] != 0).sum() == 1 and raw[0, -1, -1] != 0 and not raw[1].any() and (raw[2] == 65535).all()
    for name in ('one_partial', 'no_log'):
        raw, _, kw = sr.raw_case(name)
        assert raw[0].size % 8 != 0 and all((f != 0).any() for f in raw)
    assert sr.raw_case('no_log')[2]['log_correct'] is False
    x, y = sr.dataset_label_table(sr.dataset_raw())
    assert np.isnan(x).sum() == 11 and (x[:, 7] > 512).all()          # (frame 7's gap falls on the off-frame column)

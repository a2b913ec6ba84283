"""The reference's scaler estimation and labels reader restated in numpy f64, and the inputs the scaler tests share.

ref_standardize restates Timelapse._standardize (Timelapse.py:277-326) on dense preprocessed frames: per frame the mean, the
population std and the max of the non-zero values (`frame.data` of the reference's sparse frames), collapsed to one scaler or
kept per frame. The reference does this arithmetic in f32; here it is f64, and tests/golden/scaler_parts.npz (the reference's
own run, make_golden_scaler.py) pins the restatement to the reference within the f32 summation bound.
ref_labels restates Timelapse._load_bboxes (:377-383) and what construct_tiles makes of the table (:514, :532-534).
Pure numpy / pandas, no GPU: shared by tests/test_scaler_cpu.py and tests/test_scaler_gpu.py."""
import numpy as np
import pandas as pd

U = 2.0 ** -53


def frame_parts(frames):
    """f32 [T,H,W] preprocessed, unscaled frames -> per frame (n, sum, sumsq, max) of the values as the kernel defines them,
    in f64 with numpy's own summation order."""
    f = np.asarray(frames)
    assert f.dtype == np.float32
    d = f.reshape(len(f), -1).astype(np.float64)
    return (f.reshape(len(f), -1) != 0).sum(1).astype(np.int64), d.sum(1), (d * d).sum(1), f.reshape(len(f), -1).max(1)


def ref_standardize(frames, standardize, framewise):
    """-> (stnd_scaler, frame scales f64 [T] (the one scaler repeated when not framewise), per-frame dict of f64 arrays
    mean / std / max / n / kappa). A frame without a non-zero value gives NaN, as in the reference."""
    f = np.asarray(frames)
    means, stds, maxs, ns, kappas = [], [], [], [], []
    for fr in f:
        data = fr[fr != 0].astype(np.float64)
        ns.append(len(data))
        if len(data) == 0:
            means.append(np.nan), stds.append(np.nan), maxs.append(np.nan), kappas.append(np.nan)
            continue
        means.append(np.mean(data)), stds.append(np.std(data)), maxs.append(np.max(data))
        var = np.var(data)
        kappas.append(np.mean(data * data) / var if var > 0 else np.inf)
    per = dict(mean=np.array(means), std=np.array(stds), max=np.array(maxs), n=np.array(ns), kappa=np.array(kappas))
    if standardize == 'zscore':
        mean_scalars, var_scalars = per['mean'], per['std']
    else:
        mean_scalars, var_scalars = np.zeros(len(f)), per['max']
    if framewise:
        return (standardize, None), np.array(var_scalars, np.float64), per
    var_scalar = np.mean(var_scalars) if standardize == 'zscore' else np.max(var_scalars)
    return (standardize, (float(var_scalar), float(np.mean(mean_scalars)))), np.full(len(f), var_scalar), per


def f32_sum_bound(n, kappa=1.0):
    """Relative error bound of the reference's own f32 pairwise sums over n terms, amplified by the condition number kappa
    of what is computed from them: (ceil(log2 n) + 2) * 2^-24 * kappa."""
    return (np.ceil(np.log2(np.maximum(n, 2))) + 2) * 2.0 ** -24 * kappa


def ref_labels(fname, pad, shape):
    """_load_bboxes + construct_tiles' integer table: per input frame (x, y, column position) of the labels that land in a
    tile of the (padded) frame of `shape`."""
    bboxes = pd.read_csv(fname, index_col=0, header=[0, 1])
    bboxes = bboxes.loc[:, (slice(None), ['anchor_x', 'anchor_y'])].sort_index()
    bboxes = bboxes.reset_index(drop=True)
    if pad is not None and (pad[0] or pad[3]):
        bboxes.loc[:, (slice(None), 'anchor_y')] += pad[0]
        bboxes.loc[:, (slice(None), 'anchor_x')] += pad[3]
    ints = bboxes.fillna(-1).astype(int)
    axons = list(dict.fromkeys(ints.columns.get_level_values(0)))
    out = []
    for t in range(len(ints)):
        row = [(int(ints.loc[t, (a, 'anchor_x')]), int(ints.loc[t, (a, 'anchor_y')]), k) for k, a in enumerate(axons)
               if not (np.isnan(bboxes.loc[t, (a, 'anchor_x')]) or np.isnan(bboxes.loc[t, (a, 'anchor_y')]))]
        row = [(x, y, k) for x, y, k in row if 0 <= x < shape[1] and 0 <= y < shape[0]]
        out.append(tuple(np.array([r[i] for r in row], np.int64) for i in range(3)))
    return out


def write_labels_csv(fname, names, x, y, index=None):
    """x, y f64 [F, n_axons] (NaN = absent) -> a file in the reference's layout: header rows (axon, property), index the
    frame number."""
    cols = pd.MultiIndex.from_product([list(names), ['anchor_x', 'anchor_y']], names=('axon', 'prop'))
    vals = np.stack([np.asarray(x, np.float64), np.asarray(y, np.float64)], -1).reshape(len(x), -1)
    pd.DataFrame(vals, columns=cols, index=range(len(x)) if index is None else index).to_csv(fname)


# ------------------------------------------------------------------------------------------------ GPU test inputs
# name -> (T, H, W, seed, mask?, offset, clip, log_correct). offset / clip as `preprocess` takes them (ints: counts / 2^16).
SHAPES = {
    'one_partial': (1, 3, 5, 3, False, None, None, True),             # scalar path, one block, one partial
    'edge_frames': (3, 5, 3, 0, False, None, None, True),             # crafted frames, see raw_case
    'vector_masked': (6, 520, 1032, 11, True, 121, 55, True),          # vector path, several blocks per frame
    'grid_bound': (5, 1024, 1024, 12, False, 121, None, True),         # more than 2048 * 256 * 8 pixels
    'no_log': (4, 37, 41, 13, False, None, 260, False),                # odd frame size (scalar path), frames not 16-byte aligned
}


def raw_case(name):
    """-> (raw u16 [T,H,W], mask bool [H,W] or None, kwargs of preprocess / estimate_stnd_scaler)."""
    T, H, W, seed, masked, offset, clip, log_correct = SHAPES[name]
    rng = np.random.default_rng(seed)
    raw = np.where(rng.random((T, H, W)) < 0.03, rng.integers(200, 4001, (T, H, W)), 0).astype(np.uint16)
    if name == 'one_partial':
        raw[0, 1, 2], raw[0, 2, 4] = 1234, 777                        # 15 pixels at 3 % would mostly be an empty frame
    if name == 'edge_frames':
        raw[0], raw[1], raw[2] = 0, 0, 65535
        raw[0, -1, -1] = 3000                                          # frame 0: only its last pixel; frame 1: nothing
    mask = None
    if masked:
        mask = np.ones((H, W), bool)
        mask[:, :40], mask[100:140, :] = False, False
        mask[rng.random((H, W)) < 0.1] = False
    return raw, mask, dict(offset=offset, clip=clip, log_correct=log_correct)


def host_preprocess(raw, mask, offset, clip, log_correct):
    """The arithmetic of axt_preprocess_u16 at scale 1 in numpy f32 (log2 to numpy's rounding, not the GPU's: for choosing
    seeds and checking the inputs' properties on the CPU, not for bit comparisons)."""
    x = raw.astype(np.float32) * np.float32(1.0 / 65535.0)
    if mask is not None:
        x = np.where(mask, x, np.float32(0))
    if offset:
        x = np.maximum(x - np.float32(offset / 2 ** 16 if isinstance(offset, int) else offset), np.float32(0))
    if clip:
        x = np.where(x < np.float32(clip / 2 ** 16 if isinstance(clip, int) else clip), np.float32(0), x)
    if log_correct:
        x = np.log2(np.float32(1) + x)
    return x.astype(np.float32)


# ------------------------------------------------------------------------------------------------ the dataset of the end-to-end tests
DATASET = dict(T=12, H=512, W=512, frames_seed=7, train=list(range(2, 8)), test=[8, 9], gain=1000.0)


def dataset_raw():
    """12 raw frames whose preprocessed form looks like synth.synth_frames (speckle and moving blobs): counts = 1000 * value."""
    from axtrack_amd import synth
    D = DATASET
    f = synth.synth_frames(D['T'], D['H'], D['W'], seed=D['frames_seed'])
    return np.clip(np.rint(f * D['gain']), 0, 65535).astype(np.uint16)


def dataset_label_table(raw):
    """f64 x, y [T, 8]: per frame the brightest pixel of each 128-row band of the left and of the right half (a blob, mostly),
    half a pixel off so that truncation shows, NaN in a few slots, one label off the unpadded frame's right edge."""
    T, H, W = raw.shape
    x, y = np.full((T, 8), np.nan), np.full((T, 8), np.nan)
    for t in range(T):
        for k in range(8):
            y0, x0 = (k // 2) * 128, (k % 2) * 256
            blk = raw[t, y0:y0 + 128, x0:x0 + 256]
            iy, ix = np.unravel_index(np.argmax(blk), blk.shape)
            x[t, k], y[t, k] = x0 + ix + 0.5, y0 + iy + 0.75
        x[t, t % 8], y[t, t % 8] = np.nan, np.nan
    x[:, 7], y[:, 7] = W + 20.0, 40.0           # outside at PAD 0, inside the padded frame
    return x, y

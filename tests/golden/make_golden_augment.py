"""Generate tests/golden/augment_parts.npz: inputs and outputs of the reference's own augmentation functions
(data_utils.py): transform_X for translations and flips on a small dense stack, transform_Y for every kind of transform, and
the arguments apply_transformations passes on for a table of uniforms. torchvision is absent where this runs, so the image
rotation (TF.rotate) cannot be recorded; tests/augment_reference.py restates it with torch's grid_sample. Runs only where
the read-only reference checkout is present (tests/golden/_ref_import.py); only the data it writes is committed.

    python tests/golden/make_golden_augment.py
"""
import os
import sys

import numpy as np
import pandas as pd
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from _ref_import import import_reference  # noqa: E402

KEYS = ['vflip', 'hflip', 'rot', 'translateY', 'translateX']

# (angle, flip_dims, dy, dx) as apply_transformations hands them to transform_X / transform_Y
X_CASES = {
    'identity': (None, [], 0, 0),
    'dy_pos': (None, [], 7, 0), 'dy_neg': (None, [], -5, 0), 'dx_pos': (None, [], 0, 9), 'dx_neg': (None, [], 0, -13),
    'dy_out': (None, [], 40, 0), 'dx_out': (None, [], 0, -56), 'dydx': (None, [], 3, -4),
    'flip_y': (None, [2], 0, 0), 'flip_x': (None, [3], 0, 0), 'flip_yx': (None, [2, 3], 0, 0),
    'dy_flip_y': (None, [2], 6, 0), 'dx_flip_x': (None, [3], 0, -7), 'all_four': (None, [2, 3], -8, 10),
}
Y_CASES = {
    'identity': (None, [], 0, 0),
    'dy_pos': (None, [], 7, 0), 'dy_neg': (None, [], -9, 0), 'dx_pos': (None, [], 0, 11), 'dx_neg': (None, [], 0, -13),
    'dydx': (None, [], 5, -6),
    'flip_y': (None, [2], 0, 0), 'flip_x': (None, [3], 0, 0), 'flip_yx': (None, [2, 3], 0, 0),
    'dy_flip_y': (None, [2], 7, 0),
    'rot_4.04': (4.04, [], 0, 0), 'rot_11': (11.0, [], 0, 0), 'rot_20': (20.0, [], 0, 0), 'rot_m7': (-7.0, [], 0, 0),
    'rot_m19.96': (-19.96, [], 0, 0),
    'dy_rot': (11.0, [], 7, 0),
    'all_five': (11.0, [2, 3], -9, 11),
}
# one row per draw, one uniform per key of KEYS in order; 0.6 itself and what rounds to it stay off
UNIFORMS = np.array([
    [0.0, 0.0, 0.0, 0.0, 0.0],
    [0.6, 0.6, 0.6, 0.6, 0.6],
    [0.6004, 0.60049, 0.6004, 0.6004, 0.6004],
    [0.6006, 0.601, 0.6006, 0.6006, 0.601],
    [0.9996, 0.99951, 0.9999, 0.99999, 0.9996],
    [0.7, 0.2, 0.601, 0.75, 0.7625],
    [0.3, 0.9, 0.5, 0.8734, 0.61],
    [0.61, 0.59, 0.9, 0.1, 0.99],
    [0.123456, 0.654321, 0.777777, 0.888888, 0.999999],
    [0.65, 0.65, 0.5, 0.7509765625, 0.7490234375],
])


def label_frame(lx, ly):
    """f64 [F, cap] anchors (NaN = none) -> the reference's target DataFrame: rows the time points, columns
    (Axon_xxx, anchor_x | anchor_y)."""
    F, cap = lx.shape
    cols = pd.MultiIndex.from_product([[f'Axon_{i:03}' for i in range(cap)], ['anchor_x', 'anchor_y']])
    vals = np.stack([lx, ly], -1).reshape(F, cap * 2)
    return pd.DataFrame(vals, columns=cols, index=range(F))


def label_sets():
    """Two frames sizes; per set f64 [F, cap] x and y. NaN slots, frames of different counts (one empty), labels next to
    the borders (lost on one axis under a shift, rotated out in the corners), half-integer anchors (the last rounding)."""
    nan = np.nan
    sets = {}
    H, W = 70, 93
    x = [[2, 46, 90, 47, nan, 30.5], [8, nan, 80, 47, 60, nan], [nan] * 6, [91, 1, 46.5, 12, 88, 47]]
    y = [[35, 3, 66, 35.5, nan, 12.5], [61, nan, 5, 20, 64, nan], [nan] * 6, [68, 1, 34.5, 60, 2, 35.5]]
    sets['a'] = (H, W, np.array(x, np.float64), np.array(y, np.float64))
    H, W = 96, 160
    rng = np.random.default_rng(20240911)
    x = rng.integers(0, W, (5, 9)).astype(np.float64)
    y = rng.integers(0, H, (5, 9)).astype(np.float64)
    drop = rng.random((5, 9)) < 0.2
    x[drop], y[drop] = nan, nan
    x[0, 0], y[0, 0] = 80.5, 48.5                     # the rotation centre itself: x_rot + x_mid is a tie
    x[1, :3], y[1, :3] = [1, 158, 3], [1, 94, 93]      # corners
    sets['b'] = (H, W, x, y)
    return sets


def main():
    import_reference()
    from reference.axtrack import data_utils as du
    out = {}
    # ---- transform_X: translations and flips of a sparse [T, C, H, W] stack (rotation needs torchvision)
    rng = np.random.default_rng(20240910)
    T, C, H, W = 5, 3, 40, 56
    dense = (rng.integers(1, 256, (T, C, H, W)) / 256 * (rng.random((T, C, H, W)) < 0.3)).astype(np.float32)   # (compresses)
    dense[:, :, 0, :], dense[:, :, -1, :], dense[:, :, :, 0], dense[:, :, :, -1] = 0.11, 0.22, 0.33, 0.44     # marked edges
    out['x_in'] = dense
    out['x_names'] = np.array(list(X_CASES))
    for name, (angle, flips, dy, dx) in X_CASES.items():
        X = torch.from_numpy(dense.copy()).to_sparse().coalesce()
        got = du.transform_X(X, 2, angle, list(flips), dy, dx, H, W, 'cpu')
        out[f'x_{name}_args'] = np.array([dy, dx, 2 in flips, 3 in flips], np.int64)
        out[f'x_{name}_out'] = got.numpy().astype(np.float32)
        assert got.shape == dense.shape
    # (transform_X shifts the indices of the coalesced tensor it was given in place; every case above got its own copy)
    # ---- transform_Y. rotate_indices stores a pair of one-element tensors into a numpy row, which numpy >= 2 refuses
    # ("setting an array element with a sequence"); while it runs, torch.round hands its result back as a 0-dim tensor
    # of the same value, which numpy stores as the number it is. No arithmetic changes.
    real_round = torch.round
    torch.round = lambda t, *a, **k: real_round(t, *a, **k).reshape(()) if t.numel() == 1 else real_round(t, *a, **k)
    out['y_names'] = np.array(list(Y_CASES))
    for sname, (H, W, lx, ly) in label_sets().items():
        out[f'y_{sname}_size'] = np.array([H, W], np.int64)
        out[f'y_{sname}_lx'], out[f'y_{sname}_ly'] = lx, ly
        for name, (angle, flips, dy, dx) in Y_CASES.items():
            target = label_frame(lx, ly)
            got = du.transform_Y(target, angle, list(flips), dy, dx, H, W)
            assert list(got.columns) == list(target.columns)
            gx = got.xs('anchor_x', axis=1, level=1).to_numpy(np.float64)
            gy = got.xs('anchor_y', axis=1, level=1).to_numpy(np.float64)
            asint = got.fillna(-1).astype(int)                              # construct_tiles, Timelapse.py:514
            out[f'y_{sname}_{name}_args'] = np.array([np.nan if angle is None else angle, dy, dx, 2 in flips, 3 in flips], np.float64)
            out[f'y_{sname}_{name}_x'], out[f'y_{sname}_{name}_y'] = gx, gy
            out[f'y_{sname}_{name}_xi'] = asint.xs('anchor_x', axis=1, level=1).to_numpy(np.int64)
            out[f'y_{sname}_{name}_yi'] = asint.xs('anchor_y', axis=1, level=1).to_numpy(np.int64)
    torch.round = real_round
    # ---- apply_transformations: what it passes on for a table of uniforms
    calls = []
    real = (du.transform_X, du.transform_Y, torch.rand)
    du.transform_X = lambda X, tchunksize, angle, flip_dims, dy, dx, sizey, sizex, device: calls.append(
        ('X', angle, list(flip_dims), dy, dx)) or X
    du.transform_Y = lambda target, angle, flip_dims, dy, dx, sizey, sizex: calls.append(
        ('Y', angle, list(flip_dims), dy, dx)) or target
    try:
        rows = []
        for u in UNIFORMS:
            feed = iter(u)
            torch.rand = lambda *a, **k: torch.tensor([next(feed)], dtype=torch.float64)
            del calls[:]
            du.apply_transformations(list(KEYS), None, None, 70, 93, 'cpu')
            (_, angle, flips, dy, dx), y_call = calls
            assert y_call[1:] == (angle, flips, dy, dx)
            assert isinstance(dy, int) and isinstance(dx, int)
            rows.append([np.nan if angle is None else angle, dy, dx, 2 in flips, 3 in flips])
    finally:
        du.transform_X, du.transform_Y, torch.rand = real
    out['u_keys'] = np.array(KEYS)
    out['u_table'] = UNIFORMS
    out['u_args'] = np.array(rows, np.float64)                  # angle (NaN = None), dy, dx, flip dim 2, flip dim 3
    np.savez_compressed(os.path.join(HERE, 'augment_parts.npz'), **out)
    print({k: v.shape for k, v in out.items() if not k.startswith('y_') or k.endswith('_size')}, len(out), 'arrays')


if __name__ == '__main__':
    main()

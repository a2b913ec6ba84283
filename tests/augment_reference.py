"""Reference for the training augmentation (CPU only; nothing here is taken from csrc/augment.hip or axtrack_amd/augment.py).

`warp`: data_utils.transform_X restated on dense frames with core torch: translate (zero fill), torch.flip, and the rotation
of torchvision's TF.rotate for tensors (nearest, no expand, fill 0) rebuilt from its parts -- _get_inverse_affine_matrix,
_gen_affine_grid, torch.nn.functional.grid_sample. torchvision is not installed where the goldens are made, so the rotation
half is pinned to torch's grid_sample, not to torchvision itself; translate and flip are pinned to the reference's own
output (tests/golden/augment_parts.npz). `labels` / `transform_from_uniforms`: transform_Y and apply_transformations
restated label by label; every restatement takes a `fault` that test_augment_cpu.py seeds.

`rotation_map_f64`: the same rotation map in f64, with the pixels whose source coordinate lies within BAND px of a rounding
tie on either axis: there an f32 evaluation may round the other way, and a comparison pixel by pixel has to leave them out
(they must still equal one of the candidate roundings, or 0)."""
import math

import numpy as np
import torch

BAND = 1e-3                    # px
MAX_EXCLUDED = 0.01            # share of a frame's pixels that may lie in the band
KEYS = ('vflip', 'hflip', 'rot', 'translateY', 'translateX')

# the kernel cases of test_augment_gpu.py: shapes, and per rotation case (angle, flip_y, flip_x, dy, dx)
SHAPES = ((1, 70, 93), (7, 96, 160), (3, 520, 1030))
ROTATIONS = {'rot_4.04': (4.04, False, False, 0, 0), 'rot_11': (11.0, False, False, 0, 0),
             'rot_20': (20.0, False, False, 0, 0), 'rot_m7': (-7.0, False, False, 0, 0),
             'all_five': (11.0, True, True, -9, 11)}


# ------------------------------------------------------------------------------------------------ pixels
def translate_flip(X, dy, dx, flip_y, flip_x, fault=None):
    """X torch [N, H, W] -> the same after transform_X's translation (sources outside the frame: 0) and torch.flip."""
    N, H, W = X.shape

    def shift(A):
        out = torch.zeros_like(A)
        if abs(dy) < H and abs(dx) < W:
            ys, xs = slice(max(dy, 0), H + min(dy, 0)), slice(max(dx, 0), W + min(dx, 0))
            yd, xd = slice(max(-dy, 0), H + min(-dy, 0)), slice(max(-dx, 0), W + min(-dx, 0))
            out[:, ys, xs] = A[:, yd, xd]
        return out

    def flip(A):
        dims = [d for d, on in ((1, flip_y), (2, flip_x)) if on]
        return torch.flip(A, dims) if dims else A

    return shift(flip(X)) if fault == 'flip_first' else flip(shift(X))


def inverse_matrix(angle, fault=None):
    """_get_inverse_affine_matrix([0, 0], -angle, [0, 0], 1, [0, 0]) as TF.rotate(img, angle) calls it."""
    rot = math.radians(angle if fault == 'rot_sign' else -angle)
    return [math.cos(rot), math.sin(rot), 0.0, -math.sin(rot), math.cos(rot), 0.0]


def affine_grid(H, W, angle, dtype=torch.float32, fault=None):
    """_gen_affine_grid(theta, w, h, ow=w, oh=h) -> [1, H, W, 2] normalised (x, y). theta is rounded to f32 first whatever
    `dtype` is: the f64 map is the SAME map, evaluated more precisely."""
    theta = torch.tensor(inverse_matrix(angle, fault), dtype=torch.float32).to(dtype).reshape(1, 2, 3)
    d = 0.5
    base = torch.empty(1, H, W, 3, dtype=dtype)
    base[..., 0].copy_(torch.linspace(-W * 0.5 + d, W * 0.5 + d - 1, steps=W, dtype=dtype))
    base[..., 1].copy_(torch.linspace(-H * 0.5 + d, H * 0.5 + d - 1, steps=H, dtype=dtype).unsqueeze_(-1))
    base[..., 2].fill_(1)
    rescaled = theta.transpose(1, 2) / torch.tensor([0.5 * W, 0.5 * H], dtype=dtype)
    return base.view(1, H * W, 3).bmm(rescaled).view(1, H, W, 2)


def rotate(X, angle, fault=None):
    """TF.rotate(X, angle) for a float tensor [N, H, W]: nearest, no expand, fill 0."""
    N, H, W = X.shape
    grid = affine_grid(H, W, angle, X.dtype, fault)
    return torch.nn.functional.grid_sample(X[None], grid, mode='nearest', padding_mode='zeros', align_corners=False)[0]


def warp(frames, angle=None, flip_y=False, flip_x=False, dy=0, dx=0, fault=None):
    """numpy f32 [N, H, W] -> transform_X's result: translate, then flip, then rotate."""
    X = translate_flip(torch.from_numpy(np.ascontiguousarray(frames)), dy, dx, flip_y, flip_x, fault)
    if angle:
        X = rotate(X, angle, fault)
    return X.numpy()


def rotation_map_f64(H, W, angle):
    """-> (sx, sy: i64 [H, W] the rounded source pixel of every output pixel in f64, possibly outside the frame;
    band_x, band_y: bool [H, W], the coordinate lies within BAND of a rounding tie; fx, fy: i64 floor of the coordinate,
    whose candidates in the band are fx and fx + 1)."""
    g = affine_grid(H, W, angle, torch.float64)[0].numpy()
    ix, iy = ((g[..., 0] + 1) * W - 1) / 2, ((g[..., 1] + 1) * H - 1) / 2
    out = []
    for c in (ix, iy):
        out.append((np.rint(c).astype(np.int64), np.abs(c - np.floor(c) - 0.5) < BAND, np.floor(c).astype(np.int64)))
    (sx, bx, fx), (sy, by, fy) = out
    return sx, sy, bx, by, fx, fy


def sample(pre, sy, sx):
    """pre [N, H, W], integer source arrays [...] -> pre[:, sy, sx] with 0 where the source is outside the frame."""
    N, H, W = pre.shape
    ok = (sy >= 0) & (sy < H) & (sx >= 0) & (sx < W)
    v = pre[:, np.clip(sy, 0, H - 1), np.clip(sx, 0, W - 1)]
    return np.where(ok[None], v, np.float32(0))


def judge_rotation(got, frames, angle, flip_y, flip_x, dy, dx, log=print, name=''):
    """The kernel's `got` [N, H, W] for a case with a rotation: outside the band bit-equal to warp(); inside it one of the
    candidate roundings of the translated and flipped frames, or 0. The band holds at most MAX_EXCLUDED of the pixels."""
    N, H, W = frames.shape
    want = warp(frames, angle, flip_y, flip_x, dy, dx)
    sx, sy, bx, by, fx, fy = rotation_map_f64(H, W, angle)
    band = bx | by
    share = band.mean()
    differ = int(((got != want).any(0) & ~band).sum())
    log(f'AUGMENT | {name} {frames.shape} | band share {share:.4%} | pixels off outside the band {differ} | '
        f'inside {int(((got != want).any(0) & band).sum())} of {int(band.sum())}')
    assert share <= MAX_EXCLUDED, f'{name}: {share:.3%} of the pixels lie in the tie band'
    assert differ == 0, f'{name}: {differ} pixels outside the tie band differ from the reference'
    pre = translate_flip(torch.from_numpy(np.ascontiguousarray(frames)), dy, dx, flip_y, flip_x).numpy()
    yy, xx = np.nonzero(band)
    g = got[:, yy, xx]
    ok = g == 0
    for cy in (fy[yy, xx], fy[yy, xx] + 1):
        for cx in (fx[yy, xx], fx[yy, xx] + 1):
            use_y = np.where(by[yy, xx], cy, sy[yy, xx])
            use_x = np.where(bx[yy, xx], cx, sx[yy, xx])
            ok |= g == sample(pre, use_y, use_x)
    assert ok.all(), f'{name}: {int((~ok).sum())} values in the tie band are none of their candidates'
    return share


# ------------------------------------------------------------------------------------------------ labels
def _round(v, fault):
    return math.floor(v + 0.5) if fault == 'half_away' else float(np.round(v))


def labels(lx, ly, angle, flip_y, flip_x, dy, dx, H, W, fault=None):
    """transform_Y label by label, then fillna(-1).astype(int). lx, ly f64 [F, cap] with NaN = no label -> i64 x, y."""
    f32 = np.float32
    ox, oy = np.full(lx.shape, -1, np.int64), np.full(ly.shape, -1, np.int64)
    y_mid, x_mid = ((H - 1) / 2., (W - 1) / 2.) if fault == 'centre' else ((H + 1) / 2., (W + 1) / 2.)
    if angle:
        a = torch.tensor([angle * np.pi / 180.])
        c, s = f32(torch.cos(a).item()), f32(torch.sin(a).item())
    for i in np.ndindex(lx.shape):
        x, y = float(lx[i]), float(ly[i])
        if dy or dx:
            if dy:
                y = y + dy
                y = np.nan if (1 >= y or y >= H - 1) else y
            if dx:
                x = x + dx
                x = np.nan if (1 >= x or x >= W - 1) else x
        if flip_y:
            y = y_mid + (y_mid - y)
        if flip_x:
            x = x_mid + (x_mid - x)
        if angle:
            if np.isnan(x) or np.isnan(y):
                x = y = np.nan
            else:
                xr = f32(f32(f32(x - x_mid) * c) + f32(f32(y - y_mid) * s))
                yr = f32(f32(f32(-1.0 * (x - x_mid)) * s) + f32(f32(y - y_mid) * c))
                xr, yr = _round(float(f32(xr + f32(x_mid))), fault), _round(float(f32(yr + f32(y_mid))), fault)
                x, y = (xr, yr) if (0 < xr < W and 0 < yr < H) else (np.nan, np.nan)
        ox[i] = -1 if np.isnan(x) else int(_round(x, fault))
        oy[i] = -1 if np.isnan(y) else int(_round(y, fault))
    return ox, oy


def transform_from_uniforms(u, keys=KEYS, fault=None):
    """apply_transformations' mapping: uniforms in the order of `keys` -> (angle or None, flip_y, flip_x, dy, dx)."""
    c = {k: round(float(v), 3) for k, v in zip(keys, u)}
    on = (lambda k: c.get(k, 0) >= .6) if fault == 'ge' else (lambda k: c.get(k, 0) > .6)
    dy = round(512 * (c['translateY'] - .75)) if on('translateY') else 0
    dx = round(512 * (c['translateX'] - .75)) if on('translateX') else 0
    angle = c['rot'] * 40 - 20 if on('rot') else None
    return angle, on('hflip'), on('vflip'), dy, dx

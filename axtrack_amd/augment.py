"""Training augmentation: the reference's random translate / flip / rotate of a whole timelapse and of
its labels, redrawn every epoch (Timelapse.construct_tiles -> data_utils.apply_transformations, transform_X, transform_Y;
core_functionality.one_epoch redraws while the labels-per-tile rate is below 0.65).

The frames are warped on the GPU in one launch (csrc/augment.hip, axt_augment_frames). The transform draw, the label
transform and the rate are a few hundred numbers of host arithmetic in numpy, restated with the reference's quirks kept
(see transform_labels)."""
import dataclasses
import math

import numpy as np
import torch

from . import _lib
from .hotpath import TILE, _require_gpu, _stream

TRANSFORM_KEYS = ('vflip', 'hflip', 'rot', 'translateY', 'translateX')       # exp_parameters.py:28, USE_TRANSFORMS
SWITCH = 0.6                          # a key's rounded uniform above this switches it on (data_utils.py:149-163)


@dataclasses.dataclass(frozen=True)
class Transform:
    """One draw of apply_transformations: translate by (dy, dx), then flip, then rotate by `angle` degrees (None or 0: no
    rotation), in that order (data_utils.transform_X)."""
    dy: int = 0
    dx: int = 0
    flip_y: bool = False              # 'hflip': the reference flips dim 2 of [T, C, H, W], the rows
    flip_x: bool = False              # 'vflip': dim 3, the columns
    angle: float = None

    @property
    def flip_dims(self):
        """The dims of [T, C, H, W] that the reference's torch.flip gets."""
        return [d for d, on in ((2, self.flip_y), (3, self.flip_x)) if on]

    @property
    def identity(self):
        return not (self.dy or self.dx or self.flip_y or self.flip_x or self.angle)


def as_transform(t):
    """A Transform, a dict of its fields or None (identity) -> Transform."""
    if t is None:
        return Transform()
    if isinstance(t, Transform):
        return t
    return Transform(**dict(t))


def transform_from_uniforms(u):
    """apply_transformations, data_utils.py:141-165: `u` maps a key of TRANSFORM_KEYS to its uniform in [0, 1). Each value is
    rounded to 3 decimals; a rounded value above 0.6 switches its key on."""
    c = {k: round(float(v), 3) for k, v in u.items()}
    dy = dx = 0
    if c.get('translateY', 0) > SWITCH:
        dy = round(512 * (c.get('translateY', 0) - .75))
    if c.get('translateX', 0) > SWITCH:
        dx = round(512 * (c.get('translateX', 0) - .75))
    angle = None
    if c.get('rot', 0) > SWITCH:
        angle = c['rot'] * 40 - 20
    return Transform(dy=int(dy), dx=int(dx), flip_y=c.get('hflip', 0) > SWITCH, flip_x=c.get('vflip', 0) > SWITCH,
                     angle=angle)


def draw_transform(use_transforms, rng):
    """One rng.random() per key of `use_transforms`, in the list's order (rng: a numpy Generator) -> Transform."""
    return transform_from_uniforms({k: rng.random() for k in use_transforms})


def rotation_matrix_f32(angle):
    """The four entries (m00, m01, m10, m11) of torchvision's _get_inverse_affine_matrix([0, 0], -angle, [0, 0], 1, [0, 0])
    that TF.rotate(img, angle) builds its grid from, rounded to f32 as its torch.tensor(matrix, dtype=img.dtype) does."""
    rot = math.radians(-angle)
    return tuple(float(np.float32(v)) for v in (math.cos(rot), math.sin(rot), -math.sin(rot), math.cos(rot)))


def frame_chunk():
    """The number of frames one workgroup of the warp kernel loops over (axt_augment_frame_chunk)."""
    return int(_lib.load().axt_augment_frame_chunk())


def augment_frames(frames, transform, return_occupancy=False, out=None):
    """Warp frames f32 [T, H, W] on the GPU by `transform` (translate, then flip, then rotate; nearest neighbour, zero
    outside) -> the warped stack, a new tensor or `out` (never `frames` itself). With return_occupancy also u8
    [T, tile_rows * tile_cols]: 1 where the warped frame has a pixel > 0 in that 512-tile (partial edge tiles count)."""
    _require_gpu()
    tf = as_transform(transform)
    if not (isinstance(frames, torch.Tensor) and frames.is_cuda and frames.dtype == torch.float32 and frames.dim() == 3
            and frames.is_contiguous()):
        raise ValueError('frames must be a contiguous f32 tensor [T, H, W] on the GPU')
    T, H, W = frames.shape
    if out is None:
        out = torch.empty_like(frames)
    elif not (out.is_contiguous() and out.dtype == torch.float32 and out.device == frames.device
              and out.shape == frames.shape):
        raise ValueError('out must be a contiguous f32 tensor of the frames\' shape on their device')
    occ = None
    if return_occupancy:
        occ = torch.empty((T, -(-H // TILE) * -(-W // TILE)), dtype=torch.uint8, device=frames.device)
    rotate = bool(tf.angle)
    m = rotation_matrix_f32(tf.angle) if rotate else (1.0, 0.0, 0.0, 1.0)
    lim = 1 << 30                                     # |d| >= the frame size already empties the frame
    dy, dx = (max(-lim, min(lim, int(d))) for d in (tf.dy, tf.dx))
    with torch.cuda.device(frames.device):
        _lib.check(_lib.load().axt_augment_frames(frames.data_ptr(), T, H, W, dy, dx, int(tf.flip_y), int(tf.flip_x),
                                                  int(rotate), *m, out.data_ptr(), _lib.dptr(occ), _stream()),
                   'axt_augment_frames')
    return (out, occ) if return_occupancy else out


def label_floats(labels):
    """Labels per detection frame (x, y) or (x, y, ids), or the (lx, ly, count) arrays of training.label_arrays -> f64
    [F, cap] x, y with NaN where there is no label (a slot beyond the frame's count, a negative or a NaN coordinate)."""
    if isinstance(labels, tuple) and len(labels) == 3 and np.ndim(labels[0]) == 2 and np.ndim(labels[2]) == 1:
        lx, ly = (np.array(a, np.float64) for a in labels[:2])
        beyond = np.arange(lx.shape[1])[None, :] >= np.asarray(labels[2])[:, None]
        lx[beyond], ly[beyond] = np.nan, np.nan
    else:
        cap = max([len(l[0]) for l in labels] + [1])
        lx, ly = np.full((len(labels), cap), np.nan), np.full((len(labels), cap), np.nan)
        for t, l in enumerate(labels):
            if len(l[0]) != len(l[1]):
                raise ValueError(f'frame {t}: {len(l[0])} x anchors and {len(l[1])} y anchors')
            lx[t, :len(l[0])], ly[t, :len(l[1])] = np.asarray(l[0], np.float64), np.asarray(l[1], np.float64)
    lx[lx < 0], ly[ly < 0] = np.nan, np.nan
    return lx, ly


def transform_labels(labels, transform, H, W):
    """data_utils.transform_Y on the anchors, then construct_tiles' fillna(-1).astype(int): -> (lx, ly, count) as
    training.yolo_targets takes them, i32 [F, cap] with -1 where a coordinate was lost. A lost label keeps its slot (the
    slot index is the fourth target channel, and of two labels in a cell the higher index wins). The quirks, kept:
      translation  an axis is lost where 1 >= a or a >= size - 1 AFTER the shift, per axis: a label may keep one coordinate
                   (it is then in no tile, yolo_targets drops it); only an axis whose shift is non-zero is tested;
      flip         a -> size + 1 - a, i.e. about (size + 1) / 2, 2 px off the pixel flip size - 1 - a;
      rotation     only labels that still have both coordinates; about ((W + 1) / 2, (H + 1) / 2); each offset rounded to
                   f32, f32 cos / sin of the f32 angle, two rounded products and a rounded sum, + the f32 centre,
                   torch.round (half to even); lost on BOTH axes unless 0 < a < size on both;
      last         round half to even, NaN -> -1."""
    tf = as_transform(transform)
    x, y = label_floats(labels)
    count = np.full(x.shape[0], x.shape[1], np.int32)
    with np.errstate(invalid='ignore'):
        if tf.dy or tf.dx:
            if tf.dy:
                y = y + tf.dy
                y[(1 >= y) | (y >= H - 1)] = np.nan
            if tf.dx:
                x = x + tf.dx
                x[(1 >= x) | (x >= W - 1)] = np.nan
        y_mid, x_mid = (H + 1) / 2., (W + 1) / 2.
        if tf.flip_y:
            y = y_mid + (y_mid - y)
        if tf.flip_x:
            x = x_mid + (x_mid - x)
        if tf.angle:
            f32 = np.float32
            a = torch.tensor([tf.angle * np.pi / 180.])                      # f32, and torch's cos / sin, as the reference
            c, s = f32(torch.cos(a).item()), f32(torch.sin(a).item())
            both = ~(np.isnan(x) | np.isnan(y))
            ox, oy = (x - x_mid).astype(f32), (y - y_mid).astype(f32)
            nox = (-1.0 * (x - x_mid)).astype(f32)
            xr = np.round((ox * c + oy * s) + f32(x_mid))
            yr = np.round((nox * s + oy * c) + f32(y_mid))
            keep = both & (xr > 0) & (xr < W) & (yr > 0) & (yr < H)
            x = np.where(keep, xr.astype(np.float64), np.nan)
            y = np.where(keep, yr.astype(np.float64), np.nan)
        x, y = np.round(x), np.round(y)
    lx = np.where(np.isnan(x), -1, x).astype(np.int64).astype(np.int32)
    ly = np.where(np.isnan(y), -1, y).astype(np.int64).astype(np.int32)
    return lx, ly, count


def pos_label_rate(occ, lx, ly, count):
    """prepare_data's rate (core_functionality.py:129-136): n_pos_labels / (n_nonempty + 1). n_nonempty counts the
    (tile, frame) pairs of `occ` u8 [F or F + 4, n_tiles] that are not empty; n_pos_labels is the sum of the target grids'
    first channel over every tile, kept or not: the occupied YOLO cells, so two labels in one cell count once, and a label
    counts when it has both coordinates (neither is negative). Both are taken over the detection frames: this package has no
    labels for the two context frames at either end, so with F + 4 rows of `occ` the first and last two are left out."""
    occ = occ.cpu().numpy() if isinstance(occ, torch.Tensor) else np.asarray(occ)
    lx, ly, count = np.asarray(lx), np.asarray(ly), np.asarray(count)
    F = len(count)
    if occ.shape[0] == F + 4:
        occ = occ[2:-2]
    if occ.ndim != 2 or occ.shape[0] != F:
        raise ValueError(f'occupancy of {occ.shape[0]} frames for {F} label frames')
    cells = set()
    for f in range(F):
        for l in range(min(int(count[f]), lx.shape[1])):
            x, y = int(lx[f, l]), int(ly[f, l])
            if x >= 0 and y >= 0:
                cells.add((f, x * 12 // TILE, y * 12 // TILE))            # 12 * (a / 512) is exact in f32 for a < 2^19
    return len(cells) / (int((occ > 0).sum()) + 1)

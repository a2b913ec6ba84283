"""The training augmentation without a GPU: tests/augment_reference.py and the host half of axtrack_amd/augment.py against
what the reference's own transform_X, transform_Y and apply_transformations gave (tests/golden/augment_parts.npz, made by
tests/golden/make_golden_augment.py), bit for bit; seeded faults that each must show on a named case; and the condition
under which the GPU test compares rotated pixels one by one."""
import os

import numpy as np
import pytest
import torch

import augment_reference as ar
from axtrack_amd import augment

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'augment_parts.npz')


@pytest.fixture(scope='module')
def gold():
    return dict(np.load(GOLDEN))


def _x_case(gold, name, fault=None):
    dy, dx, fy, fx = (int(v) for v in gold[f'x_{name}_args'])
    x = gold['x_in']
    got = ar.warp(x.reshape(-1, *x.shape[2:]), None, bool(fy), bool(fx), dy, dx, fault=fault).reshape(x.shape)
    return got, gold[f'x_{name}_out']


def _y_case(gold, s, name):
    angle, dy, dx, fy, fx = gold[f'y_{s}_{name}_args']
    H, W = (int(v) for v in gold[f'y_{s}_size'])
    return (None if np.isnan(angle) else float(angle), bool(fy), bool(fx), int(dy), int(dx), H, W)


# ------------------------------------------------------------------------------------------------ against the goldens
def test_translate_and_flip_pixels_equal_transform_X(gold):
    for name in gold['x_names']:
        got, want = _x_case(gold, name)
        assert got.tobytes() == want.tobytes(), name
    assert not gold['x_dy_out_out'].any() and not gold['x_dx_out_out'].any()
    assert gold['x_identity_out'].tobytes() == gold['x_in'].tobytes()


@pytest.mark.parametrize('s', ['a', 'b'])
def test_labels_equal_transform_Y(gold, s):
    lx, ly = gold[f'y_{s}_lx'], gold[f'y_{s}_ly']
    for name in gold['y_names']:
        angle, fy, fx, dy, dx, H, W = _y_case(gold, s, name)
        wx, wy = gold[f'y_{s}_{name}_xi'], gold[f'y_{s}_{name}_yi']
        rx, ry = ar.labels(lx, ly, angle, fy, fx, dy, dx, H, W)
        assert np.array_equal(rx, wx) and np.array_equal(ry, wy), f'reference, {name}'
        tf = augment.Transform(dy=dy, dx=dx, flip_y=fy, flip_x=fx, angle=angle)
        cnt = np.full(len(lx), lx.shape[1], np.int32)
        px, py, pc = augment.transform_labels((lx, ly, cnt), tf, H, W)
        assert px.dtype == np.int32 and np.array_equal(px, wx) and np.array_equal(py, wy), f'package, {name}'
        assert np.array_equal(pc, cnt)                                   # a lost label keeps its slot
        # the list format of set_groundtruth, NaN slots left out where a frame's labels are a prefix
        if s == 'a' and name == 'identity':
            lists = [(list(x[~np.isnan(x)]), list(y[~np.isnan(y)])) for x, y in zip(lx[2:], ly[2:])]
            qx, qy, _ = augment.transform_labels(lists, tf, H, W)
            assert np.array_equal(qx, wx[2:]) and np.array_equal(qy, wy[2:])


def test_golden_label_cases_hold_what_they_are_for(gold):
    """A label lost on one axis only, a label rotated out, NaN slots, frames of different counts."""
    x, y = gold['y_a_dy_pos_x'], gold['y_a_dy_pos_y']
    assert (np.isnan(y) & ~np.isnan(x) & ~np.isnan(gold['y_a_ly'])).any()
    for s in 'ab':
        lost = np.isnan(gold[f'y_{s}_rot_20_x']) & ~np.isnan(gold[f'y_{s}_lx'])
        assert lost.any(), s
        assert np.isnan(gold[f'y_{s}_lx']).any()
    n = (~np.isnan(gold['y_a_lx'])).sum(1)
    assert len(set(n)) > 2 and 0 in n


def test_uniforms_equal_apply_transformations(gold):
    assert tuple(gold['u_keys']) == ar.KEYS == augment.TRANSFORM_KEYS
    for u, want in zip(gold['u_table'], gold['u_args']):
        w = (None if np.isnan(want[0]) else float(want[0]), bool(want[3]), bool(want[4]), int(want[1]), int(want[2]))
        assert ar.transform_from_uniforms(u) == w, u
        tf = augment.transform_from_uniforms(dict(zip(gold['u_keys'], u)))
        assert (tf.angle, tf.flip_y, tf.flip_x, tf.dy, tf.dx) == w, u
        assert tf.flip_dims == [d for d, on in ((2, w[1]), (3, w[2])) if on]

        class Feed:                                   # draw_transform: one random() per key, in the list's order
            def __init__(self, vals):
                self.vals = list(vals)

            def random(self):
                return self.vals.pop(0)
        assert augment.draw_transform(list(gold['u_keys']), Feed(u)) == tf
    some = augment.draw_transform(['rot', 'translateX'], np.random.default_rng(3))
    assert not (some.flip_y or some.flip_x or some.dy)
    assert augment.draw_transform([], np.random.default_rng(3)).identity


def test_pos_label_rate_on_a_hand_case():
    """3 detection frames of 2 x 2 tiles. Non-empty (tile, frame) pairs: 2 + 1 + 3 = 6. Labels: frame 0 has two in one
    cell (one count) and one lost on y; frame 1 has one in an EMPTY tile (it counts: the reference sums over every tile) and
    one beyond its count; frame 2 has two in neighbouring cells of different tiles. 1 + 1 + 2 = 4 -> 4 / 7."""
    occ = np.array([[1, 1, 0, 0], [0, 0, 0, 1], [1, 0, 1, 1]], np.uint8)
    lx = np.array([[100, 101, 300], [600, 5, -1], [511, 512, -1]], np.int32)
    ly = np.array([[40, 41, -1], [10, 5, -1], [700, 700, -1]], np.int32)
    cnt = np.array([3, 1, 2], np.int32)
    assert augment.pos_label_rate(occ, lx, ly, cnt) == 4 / 7
    # with the context frames' rows, two at either end, which are left out
    full = np.concatenate([np.ones((2, 4), np.uint8), occ, np.ones((2, 4), np.uint8)])
    assert augment.pos_label_rate(torch.from_numpy(full), lx, ly, cnt) == 4 / 7
    with pytest.raises(ValueError):
        augment.pos_label_rate(full[:5], lx, ly, cnt)


# ------------------------------------------------------------------------------------------------ seeded faults
def test_fault_flip_before_translate_shows_on_dy_flip_y(gold):
    got, want = _x_case(gold, 'dy_flip_y', fault='flip_first')
    assert got.tobytes() != want.tobytes()


def test_fault_rotation_sign_shows_on_rot_11():
    """No golden holds rotated pixels; the direction is pinned by hand: TF.rotate turns counter-clockwise for a positive
    angle, so a dot right of the centre moves UP (to a smaller row)."""
    x = np.zeros((1, 41, 41), np.float32)
    x[0, 20, 35] = 1
    (yy, xx), = np.argwhere(ar.warp(x, 11.0)[0])
    assert (yy, xx) == (17, 35)                       # 15 px right of the centre: 15 sin 11 = 2.86 up, 15 cos 11 = 14.7
    (yy, xx), = np.argwhere(ar.warp(x, 11.0, fault='rot_sign')[0])
    assert (yy, xx) == (23, 35)


def test_fault_label_centre_shows_on_flip_x_and_rot_11(gold):
    lx, ly = gold['y_b_lx'], gold['y_b_ly']
    for name in ('flip_x', 'rot_11'):
        angle, fy, fx, dy, dx, H, W = _y_case(gold, 'b', name)
        rx, ry = ar.labels(lx, ly, angle, fy, fx, dy, dx, H, W, fault='centre')
        assert not (np.array_equal(rx, gold[f'y_b_{name}_xi']) and np.array_equal(ry, gold[f'y_b_{name}_yi'])), name


def test_fault_ge_switch_shows_on_the_row_of_point_six(gold):
    row = gold['u_table'][1]
    assert (row == 0.6).all()
    assert ar.transform_from_uniforms(row) == (None, False, False, 0, 0)
    assert ar.transform_from_uniforms(row, fault='ge') != (None, False, False, 0, 0)


def test_fault_round_half_away_shows_on_the_half_integer_labels(gold):
    """Set a holds anchors at x.5 (the last rounding); set b one on the rotation centre (torch.round's tie)."""
    for s, name in (('a', 'identity'), ('b', 'rot_11')):
        angle, fy, fx, dy, dx, H, W = _y_case(gold, s, name)
        rx, ry = ar.labels(gold[f'y_{s}_lx'], gold[f'y_{s}_ly'], angle, fy, fx, dy, dx, H, W, fault='half_away')
        assert not (np.array_equal(rx, gold[f'y_{s}_{name}_xi']) and np.array_equal(ry, gold[f'y_{s}_{name}_yi'])), name


# ------------------------------------------------------------------------------------------------ the near-tie condition
@pytest.mark.parametrize('shape', ar.SHAPES)
def test_near_tie_band_is_small_and_holds_every_f32_difference(shape):
    """For every rotation case of test_augment_gpu.py: at most 1 % of the pixels lie within 1e-3 px of a rounding tie, and
    torch's own f32 grid_sample differs from the f64 map only there."""
    T, H, W = shape
    rng = np.random.default_rng(H)
    ramp = (1 + np.arange(H * W, dtype=np.float32)).reshape(1, H, W)         # every pixel its own value
    for name, (angle, fy, fx, dy, dx) in ar.ROTATIONS.items():
        sx, sy, bx, by, fx64, fy64 = ar.rotation_map_f64(H, W, angle)
        band = bx | by
        want64 = ar.sample(ramp, sy, sx)[0]
        got32 = ar.rotate(torch.from_numpy(ramp), angle)[0].numpy()
        off = got32 != want64
        print(f'AUGMENT-CPU | {name} {H}x{W} | band share {band.mean():.4%} | f32 grid_sample differs at {int(off.sum())} '
              f'pixels, {int((off & ~band).sum())} outside the band')
        assert band.mean() <= ar.MAX_EXCLUDED, name
        assert not (off & ~band).any(), name
    del rng
